"""Host side of the reverberant-mixture path (rtfs_reverb_plan, rtfs_mix_reverb_plan, datas.MixRecipe / draw_mix_recipe with RIRs,
datas.synthetic_rir) and the conditions tests/reverb_oracle.py itself has to meet.  None of it touches a device: both planners are host
functions of the library and every refusal tested here returns before anything is launched.  The addresses in the recipes are made-up
numbers; nothing dereferences them."""
import ctypes as C
import fractions
import os
import random
import re

import numpy as np
import pytest

from tests import mix_oracle as MO
from tests import reverb_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["rtfs_reverb_plan", "rtfs_reverb_f32", "rtfs_mix_reverb_plan", "rtfs_mix_reverb_f32"]
J, RW, TW, MAX_L = 4, 8, 4, 1 << 20                  # the mix constants (tests/test_mix_host.py)
MAX_TAPS, JOB_IN, JOB_OUT, RIR_W = 16384, 7, 6, 6
REASON = {"argument": 1, "length": 2, "n_out": 3, "segment": 4, "reference": 5, "empty_row": 6, "misaligned": 7, "dtype": 8, "taps": 9,
          "offset": 10}
SENTINEL = -0x5a5a5a5a5a5a5a5


def datas():
    from rtfs_net_amd import datas as D
    return D


def lib():
    from rtfs_net_amd import _lib
    return _lib.load()


def test_new_symbols_in_binding_table_header_makefile_and_library():
    from rtfs_net_amd import _lib
    with open(os.path.join(ROOT, "include", "rtfs_amd.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert hasattr(lib(), name)
    D = datas()
    for name, value in [("RTFS_REVERB_TILE", D.REVERB_TILE), ("RTFS_REVERB_TAP_CHUNK", D.REVERB_TAP_CHUNK), ("RTFS_REVERB_MAX_TAPS", MAX_TAPS),
                        ("RTFS_REVERB_RECIPE_WORDS", JOB_IN), ("RTFS_REVERB_JOB_WORDS", JOB_OUT), ("RTFS_MIX_RIR_WORDS", RIR_W),
                        ("RTFS_REVERB_BAD_TAPS", 9), ("RTFS_REVERB_BAD_OFFSET", 10)]:
        assert re.search(r"#define\s+" + name + r"\s+" + re.escape(str(value)) + r"\s*\n", header), name
    assert (D.REVERB_MAX_TAPS, D.REVERB_RECIPE_WORDS, D.REVERB_JOB_WORDS, D.MIX_RIR_WORDS) == (MAX_TAPS, JOB_IN, JOB_OUT, RIR_W)
    assert D.REVERB_TILE >= 64 and D.REVERB_TAP_CHUNK >= 4
    assert set(D.REVERB_REASONS) == set(REASON.values())
    assert "Reverberant mixtures" in header and header.index("Training mixtures on the device") < header.index("Reverberant mixtures")
    with open(os.path.join(ROOT, "rtfs-net_amd", "csrc", "Makefile")) as f:
        assert "k_reverb.hip" in f.read()
    import rtfs_net_amd as R
    assert callable(D.reverberate) and callable(D.load_rirs) and callable(D.synthetic_rir) and callable(R.System.mix_batch)


# ---------------------------------------------------------------- rtfs_reverb_plan
def reverb_plan(jobs, S, L, with_table=True, jobs_null=False):
    jobs = np.ascontiguousarray(jobs, np.int64)
    table = np.full(max(S, 1) * JOB_OUT, SENTINEL, np.int64)
    refused = (C.c_int * 2)(77, 77)
    code = lib().rtfs_reverb_plan(None if jobs_null else C.c_void_p(jobs.ctypes.data), S, L, C.c_void_p(table.ctypes.data) if with_table else None,
                                  refused)
    return code, table, (refused[0], refused[1])


def good_jobs(L):
    """[source address | length | dtype | start | RIR address | taps | offset]: a float32 and an int16 source, a shared RIR, a one-tap
    RIR, a segment that ends on the last sample, the largest tap count with the largest offset."""
    return np.array([[0x10004, L + 50, 0, 10, 0x70004, 4096, 0],
                     [0x90002, L + 9, 1, 9, 0x70004, 4096, 4095],
                     [0x10004, L + 50, 0, 0, 0x80000, 1, 0],
                     [0x50008, L, 0, 0, 0x7000c, MAX_TAPS, MAX_TAPS - 1]], np.int64)


def test_reverb_plan_table():
    L = 1000
    jobs = good_jobs(L)
    code, table, refused = reverb_plan(jobs, 4, L)
    assert code == 0 and refused == (77, 77)
    want = np.stack([jobs[:, 0], jobs[:, 1], jobs[:, 3] + jobs[:, 6], jobs[:, 4], jobs[:, 5], jobs[:, 2]], axis=1)
    assert np.array_equal(table.reshape(4, JOB_OUT), want)
    code, table, _ = reverb_plan(jobs, 4, L, with_table=False)
    assert code == 0 and (table == SENTINEL).all()
    assert reverb_plan(jobs[:1], 1, MAX_L)[2] == (0, REASON["segment"])  # the largest length passes the length check


def reverb_refusal(jobs, S, L, where, reason, **kw):
    code, table, refused = reverb_plan(jobs, S, L, **kw)
    assert code == -4 and refused == (where, REASON[reason]), (code, refused, where, reason)
    assert (table == SENTINEL).all()  # nothing else is written


def test_reverb_plan_refusals_name_themselves_and_write_nothing():
    L = 1000
    jobs = good_jobs(L)
    for S in (0, -2):
        reverb_refusal(jobs, S, L, -1, "argument")
    reverb_refusal(jobs, 4, L, -1, "argument", jobs_null=True)
    for bad in (0, -1, MAX_L + 1):
        reverb_refusal(jobs, 4, bad, -1, "length")

    def changed(s, word, value):
        j = jobs.copy()
        j[s, word] = value
        return j

    reverb_refusal(changed(1, 5, 0), 4, L, 1, "taps")
    reverb_refusal(changed(3, 5, MAX_TAPS + 1), 4, L, 3, "taps")
    reverb_refusal(changed(0, 6, -1), 4, L, 0, "offset")
    reverb_refusal(changed(0, 6, 4096), 4, L, 0, "offset")          # offset = taps
    reverb_refusal(changed(2, 6, 1), 4, L, 2, "offset")             # a one-tap RIR has offset 0 only
    reverb_refusal(changed(1, 3, 10), 4, L, 1, "segment")           # one sample past the end
    reverb_refusal(changed(3, 3, 1), 4, L, 3, "segment")
    reverb_refusal(changed(2, 3, -1), 4, L, 2, "segment")           # a negative start: history is read, the segment is not moved
    reverb_refusal(changed(0, 0, 0x10006), 4, L, 0, "misaligned")   # float32 at a 2-byte address
    reverb_refusal(changed(1, 0, 0x90003), 4, L, 1, "misaligned")   # int16 at an odd address
    reverb_refusal(changed(2, 4, 0x80002), 4, L, 2, "misaligned")   # an RIR at a 2-byte address
    assert reverb_plan(changed(1, 0, 0x90006), 4, L)[0] == 0        # int16 at any 2-byte alignment
    reverb_refusal(changed(3, 2, 2), 4, L, 3, "dtype")
    reverb_refusal(changed(1, 0, 0), 4, L, 1, "argument")           # no source
    reverb_refusal(changed(1, 4, 0), 4, L, 1, "argument")           # no RIR
    j = changed(3, 5, 0)
    j[1, 6] = -1
    reverb_refusal(j, 4, L, 1, "offset")                            # the first refusal in job order wins


def test_reverb_plan_refuses_a_work_list_past_2_31():
    D = datas()
    L = MAX_L
    tiles = -(-L // D.REVERB_TILE)
    S = (2 ** 31 - 1) // tiles + 1
    assert S < 2 ** 31
    # jobs is never read: the size check comes first (a list of S records would be hundreds of megabytes)
    reverb_refusal(np.zeros((1, JOB_IN), np.int64), S, L, -1, "argument", with_table=False)


# ---------------------------------------------------------------- rtfs_mix_reverb_plan
def mix_plan(slots, a, B, L, n_out):
    table = np.full(B * J * TW, SENTINEL, np.int64)
    ws, refused = C.c_size_t(0), (C.c_int * 2)(77, 77)
    code = lib().rtfs_mix_plan(C.c_void_p(np.ascontiguousarray(slots).ctypes.data), C.c_void_p(np.ascontiguousarray(a).ctypes.data), B, L, n_out,
                               C.c_void_p(table.ctypes.data), C.byref(ws), refused)
    assert code == 0
    return table, int(ws.value)


def mix_reverb_plan(slots, a, rirs, B, L, n_out, images=0x4000000, with_table=True, rirs_null=False, slots_null=False):
    slots, a, rirs = np.ascontiguousarray(slots, np.int64), np.ascontiguousarray(a, np.float64), np.ascontiguousarray(rirs, np.int64)
    table = np.full(2 * max(B, 1) * J * JOB_OUT + max(B, 1) * J * TW, SENTINEL, np.int64)
    n, ws, refused = C.c_int(-5), C.c_size_t(12345), (C.c_int * 2)(77, 77)
    code = lib().rtfs_mix_reverb_plan(None if slots_null else C.c_void_p(slots.ctypes.data), C.c_void_p(a.ctypes.data),
                                      None if rirs_null else C.c_void_p(rirs.ctypes.data), B, L, n_out, images,
                                      C.c_void_p(table.ctypes.data) if with_table else None, C.byref(n), C.byref(ws), refused)
    return code, table, n.value, int(ws.value), (refused[0], refused[1])


def target_rows(B, L):
    """B rows of a float32 target (slot 0) and three interferers whose reference is the row's target segment; interferer 2 is int16."""
    slots, a = np.zeros((B, J, RW), np.int64), np.zeros((B, J))
    for b in range(B):
        tgt = [0x10000 + 0x1000 * b, L + 40, 0, 7 + b]
        slots[b, 0] = tgt + [0, 0, 0, 0]
        slots[b, 1] = [0x200000 + 0x1000 * b, L + 3, 0, 3] + tgt
        slots[b, 2] = [0x300002 + 0x1000 * b, L + 5, 1, 0] + tgt
        slots[b, 3] = [0x400000 + 0x1000 * b, L + 9, 0, 9] + tgt
        a[b] = [1.0, 0.5, 2.0, 0.25]
    return slots, a


def test_mix_reverb_plan_shares_the_targets_image_with_its_three_references():
    B, L, IM = 2, 3000, 0x4000000
    slots, a = target_rows(B, L)
    rirs = np.zeros((B, J, RIR_W), np.int64)
    for b in range(B):
        for j in range(J):
            rirs[b, j, :3] = [0x700000 + 0x10000 * j, 100 + j, j]   # every slot its own RIR
            if j:
                rirs[b, j, 3:] = rirs[b, 0, :3]                     # every reference: the target's RIR and offset
    code, table, n, ws, refused = mix_reverb_plan(slots, a, rirs, B, L, 2, images=IM)
    assert code == 0 and refused == (77, 77) and n == B * (1 + 3) and ws == lib().rtfs_mix_workspace_bytes(B, L)
    jobs = table[:n * JOB_OUT].reshape(n, JOB_OUT)
    for b in range(B):
        for j in range(J):  # rows in the order the slots name them; the references add none
            w = slots[b, j]
            assert jobs[4 * b + j].tolist() == [w[0], w[1], w[3] + j, 0x700000 + 0x10000 * j, 100 + j, w[2]]
    # the mix table: every segment is its image row, every reference the row's target image, all float32
    want = slots.copy()
    for b in range(B):
        for j in range(J):
            want[b, j, :4] = [IM + 4 * L * (4 * b + j), L, 0, 0]
            if j:
                want[b, j, 4:] = [IM + 4 * L * (4 * b), L, 0, 0]
    assert np.array_equal(table[n * JOB_OUT:n * JOB_OUT + B * J * TW], mix_plan(want, a, B, L, 2)[0])
    assert (table[n * JOB_OUT + B * J * TW:] == SENTINEL).all()
    # sizes only: no table, no image address needed
    code, table, n2, ws2, _ = mix_reverb_plan(slots, a, rirs, B, L, 2, images=0, with_table=False)
    assert code == 0 and (n2, ws2) == (n, ws) and (table == SENTINEL).all()
    # a dry reference next to a reverberant target is another signal: it stays dry, and a different offset is another image
    r2 = rirs.copy()
    r2[0, 1, 3:] = 0
    r2[1, 2, 5] = 1
    code, table, n, _, _ = mix_reverb_plan(slots, a, r2, B, L, 2, images=IM)
    assert code == 0 and n == B * 4 + 1
    t = table[n * JOB_OUT:n * JOB_OUT + B * J * TW].reshape(-1, TW)
    assert t[1, 1] == slots[0, 0, 0] + 4 * slots[0, 0, 3]                                     # row 0, slot 1: the dry target segment
    new = 4 + 3                                                                               # named behind row 1's slots 0, 1 and 2
    assert table[new * JOB_OUT:(new + 1) * JOB_OUT].tolist() == [slots[1, 0, 0], slots[1, 0, 1], slots[1, 0, 3] + 1, 0x700000, 100, 0]
    assert t[J + 2, 1] == IM + 4 * L * new and t[J + 2, 0] == IM + 4 * L * (new - 1) and t[J + 3, 0] == IM + 4 * L * (new + 1)


def test_mix_reverb_plan_without_rirs_is_the_mix_plan():
    for B, L in [(1, 5), (3, 4097)]:
        slots, a = target_rows(B, L)
        slots[0, 2, 0] = 0  # an empty slot
        rirs = np.zeros((B, J, RIR_W), np.int64)
        rirs[0, 2, :3] = [0x700000, 10, 0]  # the RIR of an empty slot is ignored
        want, want_ws = mix_plan(slots, a, B, L, 3)
        for images in (0, 0x4000000):
            code, table, n, ws, refused = mix_reverb_plan(slots, a, rirs, B, L, 3, images=images)
            assert code == 0 and n == 0 and ws == want_ws and refused == (77, 77)
            assert np.array_equal(table[:B * J * TW], want) and (table[B * J * TW:] == SENTINEL).all()


def mix_refusal(slots, a, rirs, B, L, n_out, where, reason, **kw):
    code, table, n, ws, refused = mix_reverb_plan(slots, a, rirs, B, L, n_out, **kw)
    assert code == -4 and refused == (where, REASON[reason]), (code, refused, where, reason)
    assert (table == SENTINEL).all() and n == -5 and ws == 12345  # nothing else is written


def test_mix_reverb_plan_refusals_name_themselves_and_write_nothing():
    B, L = 3, 1000
    slots, a = target_rows(B, L)
    rirs = np.zeros((B, J, RIR_W), np.int64)
    rirs[:, :, :3] = [0x700000, 512, 3]
    rirs[:, 1:, 3:] = [0x700000, 512, 3]
    assert mix_reverb_plan(slots, a, rirs, B, L, 2)[0] == 0
    # everything the dry plan refuses, with its own pair
    mix_refusal(slots, a, rirs, 0, L, 2, -1, "argument")
    mix_refusal(slots, a, rirs, B, L, 2, -1, "argument", slots_null=True)
    mix_refusal(slots, a, rirs, B, L, 2, -1, "argument", rirs_null=True)
    for bad in (0, MAX_L + 1):
        mix_refusal(slots, a, rirs, B, bad, 2, -1, "length")
    mix_refusal(slots, a, rirs, B, L, J + 1, -1, "n_out")

    def changed(arr, b, j, word, value):
        s = arr.copy()
        s[b, j, word] = value
        return s

    mix_refusal(changed(slots, 1, 0, 3, 41), a, rirs, B, L, 2, 1 * J + 0, "segment")
    mix_refusal(changed(slots, 2, 1, 7, 99), a, rirs, B, L, 2, 2 * J + 1, "reference")
    mix_refusal(changed(slots, 1, 2, 0, 0x300001), a, rirs, B, L, 2, 1 * J + 2, "misaligned")
    mix_refusal(changed(slots, 0, 1, 2, 5), a, rirs, B, L, 2, 0 * J + 1, "dtype")
    s = slots.copy()
    s[1, :, 0] = 0
    mix_refusal(s, a, rirs, B, L, 2, 1 * J, "empty_row")
    # the RIRs
    mix_refusal(slots, a, rirs, B, L, 2, -1, "misaligned", images=0x4000002)
    mix_refusal(slots, a, changed(rirs, 1, 2, 1, 0), B, L, 2, 1 * J + 2, "taps")
    mix_refusal(slots, a, changed(rirs, 2, 0, 1, MAX_TAPS + 1), B, L, 2, 2 * J + 0, "taps")
    mix_refusal(slots, a, changed(rirs, 0, 3, 4, 0), B, L, 2, 0 * J + 3, "taps")            # the reference's RIR
    mix_refusal(slots, a, changed(rirs, 0, 1, 2, 512), B, L, 2, 0 * J + 1, "offset")
    mix_refusal(slots, a, changed(rirs, 2, 3, 5, -1), B, L, 2, 2 * J + 3, "offset")
    mix_refusal(slots, a, changed(rirs, 1, 1, 0, 0x700002), B, L, 2, 1 * J + 1, "misaligned")
    mix_refusal(slots, a, changed(rirs, 1, 1, 3, 0x700001), B, L, 2, 1 * J + 1, "misaligned")
    assert mix_reverb_plan(slots, a, changed(rirs, 1, 0, 1, MAX_TAPS), B, L, 2)[0] == 0
    mix_refusal(slots, a, rirs, B, L, 2, -1, "argument", images=0)                          # a table of images without a buffer
    r = changed(rirs, 2, 3, 1, 0)
    r[0, 1, 2] = -1
    mix_refusal(slots, a, r, B, L, 2, 0 * J + 1, "offset")                                  # the first in row-major order wins


# ---------------------------------------------------------------- recipes
def parents_draw(lengths, batch, length, n_src, snr_db, align, rng):
    """The draw order of draw_mix_recipe before it knew RIRs, restated: per row the utterances, the starts, the SNRs."""
    pool = [i for i, n in enumerate(lengths) if n >= length]
    rows, starts, dbs = [], [], []
    for _ in range(batch):
        row = rng.sample(pool, n_src)
        rows.append(row)
        starts.append([align * rng.randint(0, (lengths[i] - length) // align) for i in row])
        dbs.append([rng.uniform(snr_db[0], snr_db[1]) for _ in row[1:]])
    return np.array(rows), np.array(starts), np.array(dbs)


def test_draw_mix_recipe_without_rirs_is_the_parents_draw_and_with_them_draws_after_the_snrs():
    D = datas()
    lengths = [48000, 31999, 32000, 100000, 640, 70000, 33000]
    rows, starts, dbs = parents_draw(lengths, 16, 32000, 3, (-5.0, 5.0), 640, random.Random(7))
    r = D.draw_mix_recipe(lengths, 16, 32000, n_src=3, align=640, rng=random.Random(7))
    assert np.array_equal(r.src, rows) and np.array_equal(r.start, starts)
    assert np.array_equal(r.a, np.concatenate([np.ones((16, 1)), 10.0 ** (-dbs / 20.0)], axis=1))
    assert (r.rir == -1).all() and (r.ref_rir == -1).all() and (r.rir_offset == 0).all() and (r.ref_offset == 0).all() and not r.reverberant
    # with RIRs: the same draws per row, then per slot random() < rir_prob and randrange(n_rirs)
    rng = random.Random(7)
    pool = [i for i, n in enumerate(lengths) if n >= 32000]
    offsets = [5, 0, 17, 2, 9]
    want = []
    for _ in range(16):
        row = rng.sample(pool, 3)
        _ = [rng.randint(0, (lengths[i] - 32000) // 640) for i in row]
        _ = [rng.uniform(-5.0, 5.0) for _ in row[1:]]
        picks = []
        for _ in row:
            picks.append(rng.randrange(5) if rng.random() < 0.6 else -1)
        want.append(picks)
    want = np.array(want)
    q = D.draw_mix_recipe(lengths, 16, 32000, n_src=3, align=640, rng=random.Random(7), n_rirs=5, rir_prob=0.6, rir_offsets=offsets)
    assert np.array_equal(q.rir, want) and (want == -1).any() and (want >= 0).any() and q.reverberant
    assert np.array_equal(q.rir_offset, np.where(want >= 0, np.array(offsets)[want], 0))
    assert np.array_equal(q.ref_rir[:, 1:], np.repeat(want[:, :1], 2, axis=1)) and (q.ref_rir[:, 0] == -1).all()
    assert np.array_equal(q.ref_offset[:, 1:], np.repeat(q.rir_offset[:, :1], 2, axis=1))
    assert np.array_equal(q.src[0], rows[0]) and np.array_equal(q.start[0], starts[0])  # row 0 is drawn before any RIR draw
    full = D.draw_mix_recipe(lengths, 4, 32000, rng=random.Random(1), n_rirs=2)
    assert (full.rir >= 0).all() and (full.rir_offset == 0).all()
    with pytest.raises(ValueError):
        D.draw_mix_recipe(lengths, 4, 32000, n_rirs=0)
    with pytest.raises(ValueError):
        D.draw_mix_recipe(lengths, 4, 32000, n_rirs=2, rir_offsets=[1])


def test_snr_recipe_with_rirs():
    D = datas()
    r = D.MixRecipe.snr([3, 1], [[0, 2], [4, -1]], [[10, 20, 30], [40, 50, 60]], 0.0, rirs=[[2, -1, 0], [-1, 1, 1]], offsets=[[7, 9, 1], [3, 4, 5]])
    assert r.rir.tolist() == [[2, -1, 0], [-1, 1, -1]]             # an empty slot has no RIR
    assert r.rir_offset.tolist() == [[7, 0, 1], [0, 4, 0]]         # a dry slot no offset
    assert r.ref_rir.tolist() == [[-1, 2, 2], [-1, -1, -1]] and r.ref_offset.tolist() == [[0, 7, 7], [0, 0, 0]]
    dry = D.MixRecipe.snr([3, 1], [[0, 2], [4, -1]], [[10, 20, 30], [40, 50, 60]], 0.0)
    assert np.array_equal(dry.src, r.src) and np.array_equal(dry.a, r.a) and not dry.reverberant and r.reverberant
    with pytest.raises(ValueError):
        D.MixRecipe([[0, 1]], [[0, 0]], [[1.0, 1.0]], rir=[[0]])
    with pytest.raises(ValueError):
        D.MixRecipe.snr([0], [[1]], [[0, 0]], 0.0, rirs=[[0, 1, 2]])


def test_synthetic_rir():
    D = datas()
    for n, delay in [(1, 0), (2, 1), (512, 0), (4096, 37), (16384, 100)]:
        h = D.synthetic_rir(n, 0.3, delay=delay, rng=np.random.RandomState(n))
        assert h.shape == (n,) and h.dtype == np.float32 and int(np.abs(h).argmax()) == delay and h[delay] == 1.0
        assert (h[:delay] == 0).all() and np.isfinite(h).all()
    h = D.synthetic_rir(8000, 0.2, drr_db=3.0, rng=np.random.RandomState(1)).astype(np.float64)
    tail = h[1:]
    assert abs(10 * np.log10(1.0 / (tail @ tail)) - 3.0) < 1e-3                             # the direct-to-reverberant ratio
    e = np.cumsum((tail ** 2)[::-1])[::-1]                                                  # Schroeder: -60 dB at t60
    assert 10 * np.log10(e[1600] / e[0]) < -25 and 10 * np.log10(e[800] / e[0]) > -20
    assert np.array_equal(D.synthetic_rir(100, 0.1), D.synthetic_rir(100, 0.1))             # the default generator is seeded
    for bad in [dict(n_taps=0, t60=0.3), dict(n_taps=MAX_TAPS + 1, t60=0.3), dict(n_taps=10, t60=0.3, delay=10), dict(n_taps=10, t60=0.0)]:
        with pytest.raises(ValueError):
            D.synthetic_rir(**bad)


def test_entries_refuse_host_tensors_before_the_library_is_asked():
    import torch
    D = datas()
    with pytest.raises(ValueError):
        D.reverberate([torch.zeros(10)], [torch.zeros(3)], [0], [0], [0], 5)
    with pytest.raises(ValueError):
        D.mix_batch([torch.zeros(10)], D.MixRecipe([[0]], [[0]], [[1.0]], rir=[[0]]), 5, rirs=[torch.zeros(3)])
    with pytest.raises(ValueError):
        D.load_rirs([np.zeros(3, np.float64)])
    with pytest.raises(ValueError):
        D.load_rirs([np.zeros(MAX_TAPS + 1, np.float32)])
    with pytest.raises(ValueError):
        D.load_rirs([])


# ---------------------------------------------------------------- the oracle's own conditions
def test_oracle_image_against_convolve_and_the_unit_impulse():
    rng = np.random.RandomState(3)
    x = rng.randn(400).astype(np.float32)
    pcm = (rng.randn(300) * 5000).astype(np.int16)
    for src in (x, pcm):
        for N, p, o, L in [(1, 0, 0, 50), (5, 0, 0, 60), (5, 2, 4, 60), (37, 10, 0, 100), (37, 40, 36, len(src) - 40), (64, 63, 5, 7)]:
            h = rng.randn(N).astype(np.float32)
            full = np.convolve(RO.samples(src), h.astype(np.float64))  # full[n] = sum_k h[k] x[n - k], zeros outside the utterance
            full = np.concatenate([full, np.zeros(N)])
            want = full[p + o:p + o + L]
            exact, fast = RO.image64(src, p, h, o, L, exact=True), RO.image64(src, p, h, o, L, exact=False)
            A = np.convolve(np.abs(RO.window(src, p, N, o, L)), np.abs(h.astype(np.float64)), mode="valid")
            assert exact.shape == (L,) and (np.abs(exact - want) <= N * 2.0 ** -52 * A).all()
            assert (np.abs(fast - exact) <= N * 2.0 ** -52 * A).all()
            assert RO.image(src, p, h, o, L).dtype == np.float32
    one = np.ones(1, np.float32)
    assert np.array_equal(RO.image(x, 17, one, 0, 123), x[17:140])
    assert np.array_equal(RO.image(pcm, 5, one, 0, 40), (pcm[5:45].astype(np.float32) / np.float32(32768)))
    d = np.zeros(9, np.float32)
    d[4] = 1.0
    assert np.array_equal(RO.image(x, 2, d, 0, 20), np.concatenate([np.zeros(2, np.float32), x[:18]]))   # shifted by 4, zeros shifted in
    assert np.array_equal(RO.image(x, 2, d, 4, 20), x[2:22])                                              # the offset undoes it
    assert np.array_equal(RO.image(x, 390, d, 8, 10), np.concatenate([x[394:], np.zeros(4, np.float32)]))  # silence past the last sample


def test_oracle_bound_against_an_exact_rational_sum():
    """Five taps: the float64 image is the exactly rounded rational sum, and sums taken in either direction in plain float64, then
    rounded to float32 (what a device may do), stay inside the bound; a result that is off by two float32 steps does not."""
    rng = np.random.RandomState(11)
    x = (rng.randn(40) * np.array([1e-3, 1.0, 1e3, 1.0] * 10)).astype(np.float32)
    h = np.array([1.0, -0.7, 0.33, 1e-4, -250.0], np.float32)
    p, o, L = 3, 2, 30
    r = RO.image64(x, p, h, o, L)
    bar = RO.bound(x, p, h, o, L)
    w = RO.window(x, p, 5, o, L)
    for t in range(L):
        terms = [fractions.Fraction(float(h[k])) * fractions.Fraction(float(w[t + 4 - k])) for k in range(5)]
        true = sum(terms)
        assert r[t] == float(true)  # exactly rounded
        for order in (range(5), range(4, -1, -1)):
            acc = 0.0
            for k in order:
                acc += float(h[k]) * float(w[t + 4 - k])
            dev = np.float32(acc)
            assert abs(fractions.Fraction(float(dev)) - true) <= fractions.Fraction(float(bar[t])), (t, list(order))
        off = np.nextafter(np.nextafter(np.float32(r[t]), np.float32(np.inf)), np.float32(np.inf))
        assert abs(float(off) - r[t]) > bar[t]
    assert (RO.bound(x, p, h, o, L, exact=False) > bar).all() and (RO.bound(x, p, h, o, L, exact=False) < 2 * bar).all()


def test_oracle_mix_is_the_dry_mix_of_the_images():
    rng = np.random.RandomState(5)
    src = [rng.randn(900).astype(np.float32), (rng.randn(800) * 3000).astype(np.int16), rng.randn(700).astype(np.float32)]
    rirs = [datas().synthetic_rir(64, 0.05, delay=3, rng=rng), datas().synthetic_rir(17, 0.02, rng=rng)]
    L = 300
    rec = (np.array([[0, 1, 2]]), np.array([[100, 70, 5]]), np.array([[1.0, 0.5, 2.0]]), np.array([[-1, 0, 0]]), np.array([[0, 100, 100]]),
           np.array([[0, 1, -1]]), np.array([[-1, 0, 0]]), np.array([[3, 0, 0]]), np.array([[0, 3, 3]]))
    m, s, st, images, image_map = RO.mix(src, rirs, rec, L, 3)
    assert len(images) == 2 and image_map.tolist() == [[0, 1, -1]]
    r0, r1 = RO.image(src[0], 100, rirs[0], 3, L), RO.image(src[1], 70, rirs[1], 0, L)
    assert np.array_equal(images[0], r0) and np.array_equal(images[1], r1)
    dry = (np.array([[0, 1, 2]]), np.array([[0, 0, 5]]), rec[2], np.array([[-1, 0, 0]]), np.array([[0, 0, 0]]))
    m2, s2, st2 = MO.mix([r0, r1, src[2]], dry, L, 3)
    assert np.array_equal(m, m2) and np.array_equal(s, s2) and np.array_equal(st, st2)
    e = [MO.energy(r0.astype(np.float64)), MO.energy(r1.astype(np.float64)), MO.energy(MO.segment(src, 2, 5, L))]
    assert abs(st[0, 1] ** 2 * e[1] / e[0] - 0.25) < 1e-12 and abs(st[0, 2] ** 2 * e[2] / e[0] - 4.0) < 1e-12  # energies of images
