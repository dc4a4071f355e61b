"""Host side of the training-mixture path (rtfs_mix_plan, rtfs_mix_workspace_bytes, datas.MixRecipe / draw_mix_recipe) and the conditions
tests/mix_oracle.py itself has to meet.  None of it touches a device: the planner is a host function of the library and every refusal
tested here returns before anything is launched.  The addresses in the recipes are made-up numbers; nothing dereferences them."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest
import torch

from tests import mix_oracle as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["rtfs_mix_workspace_bytes", "rtfs_mix_plan", "rtfs_mix_f32"]
J, CHUNK, MAX_L, RW, TW, MOMENTS = 4, 4096, 1 << 20, 8, 4, 18
REASON = {"argument": 1, "length": 2, "n_out": 3, "segment": 4, "reference": 5, "empty_row": 6, "misaligned": 7, "dtype": 8}
LENGTHS = [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3]


def datas():
    from rtfs_net_amd import datas as D
    return D


def lib():
    from rtfs_net_amd import _lib
    return _lib.load()


def test_new_symbols_in_binding_table_header_and_makefile():
    from rtfs_net_amd import _lib
    with open(os.path.join(ROOT, "include", "rtfs_amd.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert hasattr(lib(), name)
    for name, value in [("RTFS_MIX_MAX_SOURCES", J), ("RTFS_MIX_CHUNK", CHUNK), ("RTFS_MIX_MAX_LENGTH", "(1 << 20)"), ("RTFS_MIX_RECIPE_WORDS", RW),
                        ("RTFS_MIX_TABLE_WORDS", TW), ("RTFS_MIX_MOMENTS", MOMENTS), ("RTFS_MIX_F32", 0), ("RTFS_MIX_I16", 1)] + \
                       [("RTFS_MIX_" + k, v) for k, v in [("BAD_ARGUMENT", 1), ("BAD_LENGTH", 2), ("BAD_N_OUT", 3), ("SEGMENT_RANGE", 4),
                                                          ("REFERENCE_RANGE", 5), ("EMPTY_ROW", 6), ("MISALIGNED", 7), ("BAD_DTYPE", 8)]]:
        assert re.search(r"#define\s+" + name + r"\s+" + re.escape(str(value)) + r"\s*\n", header), name
    D = datas()
    assert (D.MIX_MAX_SOURCES, D.MIX_CHUNK, D.MIX_MAX_LENGTH, D.MIX_RECIPE_WORDS, D.MIX_TABLE_WORDS) == (J, CHUNK, MAX_L, RW, TW)
    assert set(D.MIX_REASONS) == set(REASON.values())
    with open(os.path.join(ROOT, "rtfs-net_amd", "csrc", "Makefile")) as f:
        assert "k_mix.hip" in f.read()
    import rtfs_net_amd as R
    assert callable(R.System.online_mixing_collate) and callable(R.System.mix_batch) and callable(D.mix_batch)


# ---------------------------------------------------------------- the planner
SENTINEL = -0x5a5a5a5a5a5a5a5


def plan(slots, a, B, L, n_out, with_table=True, slots_null=False, a_null=False):
    """-> (code, table, ws_bytes, refused); table / ws / refused start as sentinels so that a write shows."""
    slots = np.ascontiguousarray(slots, np.int64)
    a = np.ascontiguousarray(a, np.float64)
    table = np.full(max(B, 1) * J * TW, SENTINEL, np.int64)
    ws, refused = C.c_size_t(12345), (C.c_int * 2)(77, 77)
    code = lib().rtfs_mix_plan(None if slots_null else C.c_void_p(slots.ctypes.data), None if a_null else C.c_void_p(a.ctypes.data), B, L, n_out,
                               C.c_void_p(table.ctypes.data) if with_table else None, C.byref(ws), refused)
    return code, table, int(ws.value), (refused[0], refused[1])


def good_recipe(B, L, seed=0):
    """B rows: slot 0 a float32 target, slot 1 an int16 interferer with the target as reference, slot 2 empty, slot 3 a float32 segment
    that ends on its source's last sample, with an int16 reference."""
    rng = random.Random(seed)
    slots, a = np.zeros((B, J, RW), np.int64), np.zeros((B, J))
    for b in range(B):
        start0, start1 = rng.randint(0, 50), rng.randint(0, 50)
        slots[b, 0] = [0x10000 + 4 * b, L + 50, 0, start0, 0, 0, 0, 0]
        slots[b, 1] = [0x90002, L + 50, 1, start1, 0x10000 + 4 * b, L + 50, 0, start0]
        slots[b, 3] = [0x50004, L + 7, 0, 7, 0x90002, L + 9, 1, 9]
        a[b] = [1.0, 0.5, 123.0, -0.25]
    return slots, a


def expected_table(slots, a):
    B = slots.shape[0]
    t = np.zeros((B, J, TW), np.int64)
    for b in range(B):
        for j in range(J):
            w = slots[b, j]
            if w[0] == 0:
                continue
            t[b, j, 0] = w[0] + w[3] * (2 if w[2] else 4)
            t[b, j, 1] = w[4] + w[7] * (2 if w[6] else 4) if w[4] else 0
            t[b, j, 2] = np.float64(a[b, j]).view(np.int64)
            t[b, j, 3] = (1 if w[2] else 0) + (2 if w[4] and w[6] else 0)
    return t.reshape(-1)


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("B", [1, 3])
def test_workspace_and_table_against_a_restatement(B, L):
    want_ws = B * (-(-L // CHUNK)) * MOMENTS * 8
    assert lib().rtfs_mix_workspace_bytes(B, L) == want_ws
    slots, a = good_recipe(B, L, seed=B + L)
    for n_out in (0, 1, J):
        code, table, ws, refused = plan(slots, a, B, L, n_out)
        assert code == 0 and ws == want_ws and refused == (77, 77)
        assert np.array_equal(table, expected_table(slots, a))
    code, table, ws, _ = plan(slots, a, B, L, 1, with_table=False)  # validation and sizes only
    assert code == 0 and ws == want_ws and (table == SENTINEL).all()


def test_workspace_query_refuses_what_the_plan_refuses():
    for B, L in [(0, 100), (-1, 100), (1, 0), (1, -5), (1, MAX_L + 1)]:
        assert lib().rtfs_mix_workspace_bytes(B, L) == 0, (B, L)
    assert lib().rtfs_mix_workspace_bytes(1, MAX_L) == 256 * MOMENTS * 8


def refusal(slots, a, B, L, n_out, where, reason, **kw):
    code, table, ws, refused = plan(slots, a, B, L, n_out, **kw)
    assert code == -4 and refused == (where, REASON[reason]), (code, refused, where, reason)
    assert (table == SENTINEL).all() and ws == 12345  # nothing else is written


def test_every_refusal_names_itself_and_writes_nothing():
    B, L = 3, 1000
    slots, a = good_recipe(B, L)
    assert plan(slots, a, B, L, 2)[0] == 0
    refusal(slots, a, 0, L, 2, -1, "argument")
    refusal(slots, a, -3, L, 2, -1, "argument")
    refusal(slots, a, B, L, 2, -1, "argument", slots_null=True)
    refusal(slots, a, B, L, 2, -1, "argument", a_null=True)
    for bad in (0, -1, MAX_L + 1):
        refusal(slots, a, B, bad, 2, -1, "length")
    for bad in (-1, J + 1):
        refusal(slots, a, B, L, bad, -1, "n_out")
    assert plan(slots, a, B, MAX_L, 2)[1][0] == SENTINEL  # the largest length passes the length check (and fails on the short sources)

    def changed(b, j, word, value):
        s = slots.copy()
        s[b, j, word] = value
        return s

    refusal(changed(1, 0, 3, 51), a, B, L, 2, 1 * J + 0, "segment")      # one sample past the end
    assert plan(changed(1, 0, 3, 50), a, B, L, 2)[0] == 0                # ends on the last sample
    refusal(changed(2, 1, 3, -1), a, B, L, 2, 2 * J + 1, "segment")      # a negative start
    refusal(changed(0, 3, 1, L + 6), a, B, L, 2, 0 * J + 3, "segment")   # a source one sample too short
    refusal(changed(2, 1, 7, 51), a, B, L, 2, 2 * J + 1, "reference")
    refusal(changed(0, 3, 5, L + 8), a, B, L, 2, 0 * J + 3, "reference")
    refusal(changed(1, 0, 0, 0x10002), a, B, L, 2, 1 * J + 0, "misaligned")  # float32 at a 2-byte address
    refusal(changed(1, 1, 0, 0x90001), a, B, L, 2, 1 * J + 1, "misaligned")  # int16 at an odd address
    refusal(changed(1, 3, 4, 0x90001), a, B, L, 2, 1 * J + 3, "misaligned")  # the reference
    assert plan(changed(1, 1, 0, 0x90006), a, B, L, 2)[0] == 0               # int16 at any 2-byte alignment
    refusal(changed(0, 1, 2, 2), a, B, L, 2, 0 * J + 1, "dtype")
    refusal(changed(0, 1, 6, -1), a, B, L, 2, 0 * J + 1, "dtype")
    s = slots.copy()
    s[1, :, 0] = 0
    refusal(s, a, B, L, 2, 1 * J, "empty_row")
    s = slots.copy()
    s[0, 0, 0] = s[0, 3, 0] = 0  # empty slots at the start and the end of a row are fine; their other words are ignored
    s[0, 0, 2] = 99
    assert plan(s, a, B, L, 2)[0] == 0


def test_the_first_refusal_in_row_major_order_wins():
    slots, a = good_recipe(2, 100)
    slots[1, 0, 3] = 10 ** 6
    slots[0, 3, 0] += 1
    code, _, _, refused = plan(slots, a, 2, 100, 1)
    assert code == -4 and refused == (3, REASON["misaligned"])


# ---------------------------------------------------------------- recipes
def test_snr_recipe_factors():
    D = datas()
    r = D.MixRecipe.snr([3, 1], [[0, 2], [4, -1]], [[10, 20, 30], [40, 50, 60]], [[-5.0, 5.0], [0.0, 0.0]])
    assert r.shape == (2, 3)
    assert r.src.tolist() == [[3, 0, 2], [1, 4, -1]] and r.start.tolist() == [[10, 20, 30], [40, 50, 60]]
    assert r.ref_src.tolist() == [[-1, 3, 3], [-1, 1, -1]] and r.ref_start.tolist() == [[0, 10, 10], [0, 40, 0]]
    want = [[1.0, 10 ** 0.25, 10 ** -0.25], [1.0, 1.0, 1.0]]
    assert np.allclose(r.a, want, rtol=1e-15, atol=0) and r.a.dtype == np.float64
    r = D.MixRecipe.snr([0], [[1]], [[0, 0]], 20.0)  # a scalar SNR: the interferer ends 20 dB below the target
    assert r.a.tolist() == [[1.0, 0.1]]
    # ... which is what the oracle's gains make of it
    rng = np.random.RandomState(0)
    src = [rng.randn(500).astype(np.float32), (3.0 * rng.randn(700)).astype(np.float32)]
    rec = (r.src, r.start, r.a, r.ref_src, r.ref_start)
    g = MO.gains(src, rec, 400)
    e0, e1 = MO.energy(MO.segment(src, 0, 0, 400)), MO.energy(MO.segment(src, 1, 0, 400))
    assert abs(10 * np.log10(e0 / (g[0, 1] ** 2 * e1)) - 20.0) < 1e-9 and g[0, 0] == 1.0 and (g[0, 2:] == 0).all()
    for bad in [dict(src=[[0] * 5], start=[[0] * 5], a=[[1.0] * 5]), dict(src=[0, 1], start=[0, 0], a=[1.0, 1.0]),
                dict(src=[[0, 1]], start=[[0]], a=[[1.0, 1.0]])]:
        with pytest.raises(ValueError):
            D.MixRecipe(**bad)


def test_draw_mix_recipe():
    D = datas()
    lengths = [48000, 31999, 32000, 100000, 640, 70000, 33000]
    a = D.draw_mix_recipe(lengths, 64, 32000, n_src=3, align=640, rng=random.Random(7))
    b = D.draw_mix_recipe(lengths, 64, 32000, n_src=3, align=640, rng=random.Random(7))
    for u, v in zip((a.src, a.start, a.a, a.ref_src, a.ref_start), (b.src, b.start, b.a, b.ref_src, b.ref_start)):
        assert np.array_equal(u, v)  # reproducible from a seeded random.Random
    c = D.draw_mix_recipe(lengths, 64, 32000, n_src=3, align=640, rng=random.Random(8))
    assert not np.array_equal(a.src, c.src)
    assert a.shape == (64, 3)
    assert set(a.src.reshape(-1).tolist()) <= {0, 2, 3, 5, 6} and len(set(a.src.reshape(-1).tolist())) == 5  # never a short one
    for row in a.src:
        assert len(set(row.tolist())) == 3  # distinct utterances in a row
    assert (a.start % 640 == 0).all() and (a.start >= 0).all()
    assert (a.start + 32000 <= np.array(lengths)[a.src]).all()
    assert (a.start[a.src == 2] == 0).all() and (a.start[a.src == 6] <= 640).all() and a.start.max() > 32000
    assert (a.a[:, 0] == 1.0).all() and (a.ref_src[:, 0] == -1).all()
    assert (a.ref_src[:, 1:] == a.src[:, :1]).all() and (a.ref_start[:, 1:] == a.start[:, :1]).all()
    db = -20 * np.log10(a.a[:, 1:])
    assert (db >= -5.0 - 1e-9).all() and (db <= 5.0 + 1e-9).all() and db.std() > 1.0
    random.seed(3)  # without rng: the random module, as RandomCrop.offsets / HorizontalFlip.draw
    d = D.draw_mix_recipe(lengths, 4, 32000)
    random.seed(3)
    e = D.draw_mix_recipe(lengths, 4, 32000)
    assert np.array_equal(d.src, e.src) and np.array_equal(d.a, e.a) and d.shape == (4, 2)
    one = D.draw_mix_recipe(lengths, 5, 640, n_src=1, rng=random.Random(1))
    assert one.shape == (5, 1) and (one.a == 1.0).all()
    with pytest.raises(ValueError):
        D.draw_mix_recipe([100, 200, 31999], 2, 32000)  # none is long enough
    with pytest.raises(ValueError):
        D.draw_mix_recipe([32000, 100], 2, 32000, n_src=2)  # one is: no two distinct ones
    with pytest.raises(ValueError):
        D.draw_mix_recipe(lengths, 2, 32000, n_src=5)


def test_mix_batch_refuses_host_tensors_before_the_library_is_asked():
    D = datas()
    r = D.MixRecipe([[0]], [[0]], [[1.0]])
    for bad in ([torch.zeros(10)], [torch.zeros(10, dtype=torch.float64)], [np.zeros(10, np.float32)], []):
        with pytest.raises(ValueError):
            D.mix_batch(bad, r, 5)
    with pytest.raises(ValueError):
        D.mix_batch([torch.zeros(10)], "recipe", 5)


# ---------------------------------------------------------------- the oracle's own conditions
def test_oracle_collate_conserves_energy_and_follows_torch_randperm():
    rng = np.random.RandomState(5)
    B, n_src, L = 7, 3, 333
    t = (rng.randn(B, n_src, L) * rng.uniform(0.01, 10.0, (B, n_src, 1))).astype(np.float32)
    torch.manual_seed(123)
    perms = [torch.randperm(B).tolist() for _ in range(n_src)]  # the reference's call, in source order
    torch.manual_seed(123)
    again = [torch.randperm(B).tolist() for _ in range(n_src)]
    assert perms == again and all(sorted(p) == list(range(B)) for p in perms) and len({tuple(p) for p in perms}) > 1
    inputs, new = MO.collate(t, perms)
    assert inputs.shape == (B, L) and new.shape == (B, n_src, L)
    e_old, e_new = (t.astype(np.float64) ** 2).sum(-1), (new ** 2).sum(-1)
    assert np.abs(e_new / e_old - 1).max() <= 1e-12  # new source i of row b has the energy of the source it replaces
    for i in range(n_src):
        for b in range(B):
            s = t[perms[i][b], i].astype(np.float64)
            assert np.allclose(new[b, i] / np.sqrt(e_old[b, i]), s / np.sqrt((s ** 2).sum()), rtol=1e-12, atol=1e-15)
    assert np.array_equal(inputs, new.sum(1))
    # the same thing as a mix recipe: the oracle's two statements agree
    flat = [t.reshape(-1)]
    src = np.zeros((B, n_src), np.int64)
    start = np.array([[(perms[i][b] * n_src + i) * L for i in range(n_src)] for b in range(B)])
    ref_start = np.array([[(b * n_src + i) * L for i in range(n_src)] for b in range(B)])
    mixture, out, stats = MO.mix(flat, (src, start, np.ones((B, n_src)), src, ref_start), L, n_src)
    assert np.abs(out - new).max() <= 1e-6 * np.abs(new).max() and np.abs(mixture - inputs).max() <= 1e-6 * np.abs(inputs).max()


def test_oracle_mix_given_its_own_stats_is_mix():
    rng = np.random.RandomState(9)
    src = [rng.randn(900).astype(np.float32), (rng.randn(800) * 3000).astype(np.int16), (100.0 + rng.randn(1000)).astype(np.float32)]
    rec = (np.array([[0, 1, -1, 2], [2, -1, 0, -1]]), np.array([[5, 6, 0, 7], [100, 0, 3, 0]]), np.array([[1.0, 0.5, 0, -0.25], [1.0, 0, 2.0, 0]]),
           np.array([[-1, 0, -1, 0], [-1, -1, 2, -1]]), np.array([[0, 5, 0, 5], [0, 0, 100, 0]]))
    for normalize in (False, True):
        m, s, st = MO.mix(src, rec, 777, 4, normalize=normalize)
        m2, s2 = MO.mix_given_stats(src, rec, 777, 4, st, normalize=normalize)
        assert np.array_equal(m, m2)
        assert np.abs(s - s2).max() <= 1e-6 * np.abs(s).max()  # the source means are stated differently (g mean(x) vs mean(g x))
        if normalize:
            assert abs(m.astype(np.float64).mean(-1)).max() < 1e-6 and np.abs(m.astype(np.float64).std(-1, ddof=1) - 1).max() < 1e-6
    assert MO.max_abs_corr(src, rec, 777) < 0.2
    twice = (np.array([[0, 0]]), np.array([[0, 0]]), np.array([[1.0, 0.5]]), np.array([[-1, -1]]), np.array([[0, 0]]))
    assert MO.max_abs_corr([src[0]], twice, 500) == 0.0  # the same segment in two slots is one signal
    anti = [src[0], (-src[0] + 0.01 * rng.randn(900)).astype(np.float32)]  # two utterances that all but cancel
    rec = (np.array([[0, 1]]), np.array([[0, 0]]), np.array([[1.0, 1.0]]), np.array([[-1, -1]]), np.array([[0, 0]]))
    assert MO.max_abs_corr(anti, rec, 500) > 0.999 and MO.moment_bounds(anti, rec, 500)[2][0] > 1e4
