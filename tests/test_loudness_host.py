"""Host side of the loudness path (rtfs_loudness_design, rtfs_loudness_plan, datas.MixRecipe.lufs, draw_mix_recipe(loudness=...)) and
the conditions tests/loudness_oracle.py itself has to meet: the restatements against the 80-bit run, the measured bar, the gate margin
of every GPU input.  None of it touches a device: the planner is a host function of the library and every refusal tested here returns
before anything is launched.  The addresses in the records are made-up numbers; nothing dereferences them."""
import ctypes as C
import math
import os
import random
import re

import numpy as np
import pytest

from tests import loudness_oracle as LO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["rtfs_loudness_design", "rtfs_loudness_plan", "rtfs_loudness_f32", "rtfs_loudness_gain_f32"]
RW, HW, TW, MAX_L, CHUNK = 3, 64, 8, 1 << 26, 4096
REASON = {"argument": 1, "rate": 2, "short": 3, "long": 4, "misaligned": 5, "dtype": 6}
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
    for name, value in [("RTFS_LOUD_LANES", LO.LANES), ("RTFS_LOUD_CHUNK", CHUNK), ("RTFS_LOUD_MAX_LENGTH", "(1 << 26)"),
                        ("RTFS_LOUD_MIN_RATE", D.LOUD_MIN_RATE), ("RTFS_LOUD_MAX_RATE", D.LOUD_MAX_RATE), ("RTFS_LOUD_RECORD_WORDS", RW),
                        ("RTFS_LOUD_HEADER_WORDS", HW), ("RTFS_LOUD_TABLE_WORDS", TW)] + \
                       [("RTFS_LOUD_" + k, v) for k, v in [("BAD_ARGUMENT", 1), ("BAD_RATE", 2), ("TOO_SHORT", 3), ("TOO_LONG", 4),
                                                           ("MISALIGNED", 5), ("BAD_DTYPE", 6)]]:
        assert re.search(r"#define\s+" + name + r"\s+" + re.escape(str(value)) + r"\s*\n", header), name
    assert (D.LOUD_RECORD_WORDS, D.LOUD_HEADER_WORDS, D.LOUD_TABLE_WORDS, D.LOUD_MAX_LENGTH) == (RW, HW, TW, MAX_L)
    assert (D.LOUD_MIN_RATE, D.LOUD_MAX_RATE) == (8000, 192000) and set(D.LOUD_REASONS) == set(REASON.values())
    assert "\n/* Loudness (" in header and header.index("Reverberant mixtures") < header.index("\n/* Loudness (")
    with open(os.path.join(ROOT, "rtfs-net_amd", "csrc", "Makefile")) as f:
        assert "k_loudness.hip" in f.read()
    import rtfs_net_amd as R
    assert callable(D.loudness) and callable(D.loudness_many) and callable(D.loudness_normalize) and callable(D.MixRecipe.lufs)
    assert callable(R.System.mix_batch)


# ---------------------------------------------------------------- the design
def test_coefficients_at_48_khz_are_the_standards_table_and_at_16_khz_the_stated_ones():
    b0, b1, b2, a1, a2, c1, c2 = LO.design(48000)
    want = [1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585, -1.99004745483398, 0.99007225036621]
    assert max(abs(g - w) for g, w in zip((b0, b1, b2, a1, a2, c1, c2), want)) <= 1e-14
    want = [1.4432952234913587, -1.8315753812604594, 0.6816587574119699, -1.1015337691069944, 0.39491236874986363, -1.9702895280044335,
            0.9705104905358434]
    assert max(abs(g - w) for g, w in zip(LO.design(16000), want)) <= 1e-15


def test_the_librarys_design_is_the_oracles_bit_for_bit():
    """The high-pass is nearly critically damped: one ulp in its denominator can move the response near 38 Hz by parts in 10^12, so the
    oracle and the planner have to hold the same coefficients, not nearly the same."""
    for fs in (8000, 16000, 22050, 44100, 48000, 96000, 192000):
        buf = (C.c_double * 8)()
        assert lib().rtfs_loudness_design(fs, buf) == 0
        assert tuple(buf) == LO.design(fs) + (LO.ABS_GATE,), fs
    for fs in (7990, 11025, 192010, 0, -8000):
        assert lib().rtfs_loudness_design(fs, (C.c_double * 8)()) == -4


# ---------------------------------------------------------------- the oracle's own conditions
def test_device_formulation_against_the_80_bit_run_and_scipy():
    from scipy import signal
    rng = np.random.RandomState(9)
    for fs in (8000, 16000, 44100, 48000):
        H = fs // 10
        x = (0.1 * rng.randn(5 * H + 77) + 0.05).astype(np.float32)
        E, z = LO.device64(x, fs)
        (Et,), (zt,) = LO.truth([x], fs)
        assert E.shape == (5,) and z.shape == (2,)
        assert LO.rel_dev(E, Et) <= LO.BAR and LO.rel_dev(z, zt) <= LO.BAR, fs
        y = x.astype(np.float64)
        for b, a in LO.biquads(fs):
            y = signal.lfilter(b, a, y)
        Es = (y[:5 * H] ** 2).reshape(5, H).sum(axis=1)
        assert LO.rel_dev(E, Es) <= LO.BAR and LO.rel_dev(Es, Et) <= LO.BAR, fs
        (Ep,), _ = LO.plain64([x], fs)
        assert LO.rel_dev(Ep, Et) <= LO.BAR
    # the powers: A^(m + n) = A^m A^n to rounding, A^0 = 1
    assert np.array_equal(LO.power(16000, 0), np.eye(4))
    assert np.allclose(LO.power(16000, 25) @ LO.power(16000, 50), LO.power(16000, 75), rtol=0, atol=1e-13)


def test_the_bar_is_eight_times_the_measured_deviation_under_the_ceiling():
    m = LO.measure()
    print({k: tuple(f"{v:.3g}" for v in vs) for k, vs in m.items()})
    worst = max(v for vs in m.values() for v in vs)
    assert worst <= LO.MEASURED and worst >= LO.MEASURED / 2   # the constant is the measurement, rounded up
    assert LO.BAR == 8 * LO.MEASURED and LO.BAR <= LO.CEILING == 1e-9
    assert LO.LUFS_BAR == 10.0 / math.log(10.0) * LO.BAR


def test_every_gpu_input_keeps_its_blocks_away_from_both_gates():
    tr = LO.truth_of_cases()
    names = [n for n, _, _ in LO.gpu_cases()]
    assert len(set(names)) == len(names) == len(tr)
    for n in names:
        LO.assert_gate_margin(tr[n][1], n)
    # and both gates are at work where the cases say so
    z = np.asarray(tr["zeros"][1], np.float64)
    assert z[12] < LO.ABS_GATE and z[12] > 0 and LO.gate(z)[1] < len(z)
    z = np.asarray(tr["quiet40"][1], np.float64)
    lufs, kept = LO.gate(z)
    assert (z > LO.ABS_GATE).all() and kept < len(z) and (z[9:16] < 0.1 * z.mean()).all()
    assert LO.gate(tr["under70"][1]) == (float("-inf"), 0)
    with pytest.raises(AssertionError):
        LO.assert_gate_margin(np.array([1.0, 1.0, 0.2 / 2.9 * (1 + 1e-7)]))   # t = 0.1 (2 + t) / 3 at t = 0.2 / 2.9
    LO.assert_gate_margin(np.array([1.0, 1.0, 0.2 / 2.9 * (1 + 1e-5)]))
    with pytest.raises(AssertionError):
        LO.assert_gate_margin(np.array([LO.ABS_GATE * (1 - 1e-7), 1.0]))


def test_known_answers():
    fs = 48000
    x = np.sin(2 * np.pi * 997.0 * np.arange(2 * fs) / fs).astype(np.float32)
    lufs, kept = LO.gate(LO.device64(x, fs)[1])
    assert abs(lufs - (-3.01)) <= 0.01 and kept == 17
    assert LO.gate(LO.device64(np.zeros(8000, np.float32), 16000)[1]) == (float("-inf"), 0)
    assert LO.gate(LO.truth([np.zeros(8000, np.float32)], 16000)[1][0]) == (float("-inf"), 0)
    z = np.array([1.0, np.nan, 1.0])
    assert math.isnan(LO.gate(z)[0]) and LO.gate(z)[1] == 0


# ---------------------------------------------------------------- rtfs_loudness_plan
def plan(recs, R, fs, with_table=True, recs_null=False):
    recs = np.ascontiguousarray(recs, np.int64)
    table = np.full(HW + max(R, 1) * TW, SENTINEL, np.int64)
    ws, totals, refused = C.c_size_t(12345), (C.c_longlong * 4)(-5, -5, -5, -5), (C.c_int * 2)(77, 77)
    code = lib().rtfs_loudness_plan(None if recs_null else C.c_void_p(recs.ctypes.data), R, fs,
                                    C.c_void_p(table.ctypes.data) if with_table else None, C.byref(ws), totals, refused)
    return code, table, int(ws.value), tuple(totals), (refused[0], refused[1])


def good_recs(H):
    """[address | length | dtype]: float32 and int16 at odd element offsets, the shortest length, a ragged tail, the longest length."""
    return np.array([[0x10004, 4 * H, 0], [0x90002, 5 * H - 1, 1], [0x5000c, 37 * H + 5, 0], [0x70006, MAX_L, 1]], np.int64)


def test_plan_table():
    for fs in (8000, 16000, 44100, 48000):
        H = fs // 10
        recs = good_recs(H)
        code, table, ws, totals, refused = plan(recs, 4, fs)
        assert code == 0 and refused == (77, 77)
        nh = recs[:, 1] // H
        chunks = -(-recs[:, 1] // CHUNK)
        assert totals == (nh.sum(), nh.sum() - 12, recs[:, 1].sum(), chunks.sum())
        assert ws == nh.sum() * (4 * LO.LANES + 9) * 8
        p = -(-H // LO.LANES)
        assert table[:8].tolist() == [fs, H, p, 4, *totals]
        assert table[8:16].view(np.float64).tolist() == list(LO.design(fs)) + [LO.ABS_GATE]
        for at, n in ((16, p), (32, H % p), (48, H)):
            assert np.array_equal(table[at:at + 16].view(np.float64).reshape(4, 4), LO.power(fs, n)), (fs, n)
        rec = table[HW:].reshape(4, TW)
        first = lambda v: np.concatenate([[0], np.cumsum(v)[:-1]])
        want = np.stack([recs[:, 0], recs[:, 1], recs[:, 2], nh, first(nh), first(recs[:, 1]), first(chunks), first(nh - 3)], axis=1)
        assert np.array_equal(rec, want)
        code, table, ws2, totals2, _ = plan(recs, 4, fs, with_table=False)
        assert code == 0 and (table == SENTINEL).all() and (ws2, totals2) == (ws, totals)


def refusal(recs, R, fs, where, reason, **kw):
    code, table, ws, totals, refused = plan(recs, R, fs, **kw)
    assert code == -4 and refused == (where, REASON[reason]), (code, refused, where, reason)
    assert (table == SENTINEL).all() and ws == 12345 and totals == (-5, -5, -5, -5)  # nothing else is written


def test_plan_refusals_name_themselves_and_write_nothing():
    fs, H = 16000, 1600
    recs = good_recs(H)
    for R in (0, -3):
        refusal(recs, R, fs, -1, "argument")
    refusal(recs, 4, fs, -1, "argument", recs_null=True)
    for bad in (11025, 7990, 192010, 16001, 0, -16000):    # no multiple of 10, out of range either side
        refusal(recs, 4, bad, -1, "rate")
    assert plan(recs[:3], 3, 8000)[0] == 0 and plan(recs[:1] * [1, 12, 1], 1, 192000)[0] == 0

    def changed(r, word, value):
        c = recs.copy()
        c[r, word] = value
        return c

    refusal(changed(0, 1, 4 * H - 1), 4, fs, 0, "short")
    refusal(changed(2, 1, 0), 4, fs, 2, "short")
    refusal(changed(3, 1, MAX_L + 1), 4, fs, 3, "long")
    refusal(changed(0, 0, 0x10006), 4, fs, 0, "misaligned")   # float32 at a 2-byte address
    refusal(changed(1, 0, 0x90003), 4, fs, 1, "misaligned")   # int16 at an odd address
    assert plan(changed(1, 0, 0x90006), 4, fs)[0] == 0        # int16 at any 2-byte alignment
    refusal(changed(2, 2, 2), 4, fs, 2, "dtype")
    refusal(changed(1, 0, 0), 4, fs, 1, "argument")           # no recording
    c = changed(3, 1, MAX_L + 1)
    c[1, 1] = 5
    refusal(c, 4, fs, 1, "short")                             # the first refusal in pool order wins


def test_entries_refuse_host_tensors_and_bad_pools_before_the_library_is_asked():
    import torch
    D = datas()
    with pytest.raises(ValueError):
        D.loudness(torch.zeros(8000), 16000)
    with pytest.raises(ValueError):
        D.loudness_many([], 16000)
    with pytest.raises(ValueError):
        D.loudness_normalize([torch.zeros(8000)], 16000)
    with pytest.raises(ValueError):
        D.loudness(torch.zeros(2, 2, 8000), 16000)


# ---------------------------------------------------------------- recipes
def test_lufs_recipe_arithmetic():
    D = datas()
    ul = [-20.0, -31.5, -17.25, float("-inf"), float("nan")]
    r = D.MixRecipe.lufs([[0, 1, 2], [2, -1, 0]], [[10, 20, 30], [40, 50, 60]], [[-23.0, -28.0, -33.0], [-25.0, -26.0, -27.0]], ul)
    want = np.array([[10 ** ((-23.0 + 20.0) / 20), 10 ** ((-28.0 + 31.5) / 20), 10 ** ((-33.0 + 17.25) / 20)],
                     [10 ** ((-25.0 + 17.25) / 20), 0.0, 10 ** ((-27.0 + 20.0) / 20)]])
    assert np.array_equal(r.a, want) and r.src.tolist() == [[0, 1, 2], [2, -1, 0]] and r.start.tolist() == [[10, 20, 30], [40, 50, 60]]
    assert (r.ref_src == -1).all() and (r.ref_start == 0).all() and not r.reverberant   # no reference segment: the gains are fixed
    assert np.array_equal(D.MixRecipe.lufs([[0], [1]], [[0], [0]], -23.0, ul).a, [[10 ** (-3.0 / 20)], [10 ** (8.5 / 20)]])
    assert np.array_equal(D.MixRecipe.lufs([[0, 1], [1, 2]], [[0, 0], [0, 0]], [-20.0, -30.0], ul).a,
                          [[1.0, 10 ** (11.5 / 20)], [10 ** (1.5 / 20), 10 ** (-12.75 / 20)]])
    for bad in (3, 4):
        with pytest.raises(ValueError, match=f"source {bad}"):
            D.MixRecipe.lufs([[0, bad]], [[0, 0]], -23.0, ul)
    assert D.MixRecipe.lufs([[0, -1]], [[0, 0]], -23.0, ul).shape == (1, 2)            # an unused silent utterance is no error
    with pytest.raises(ValueError):
        D.MixRecipe.lufs([[0, 5]], [[0, 0]], -23.0, ul)
    with pytest.raises(ValueError):
        D.MixRecipe.lufs([[0, 1]], [[0, 0]], float("nan"), ul)
    q = D.MixRecipe.lufs([[0, 1]], [[5, 6]], -23.0, ul, rirs=[[2, -1]], offsets=[[7, 9]])
    assert q.rir.tolist() == [[2, -1]] and q.rir_offset.tolist() == [[7, 0]] and (q.ref_rir == -1).all() and q.reverberant
    assert np.array_equal(q.a, D.MixRecipe.lufs([[0, 1]], [[5, 6]], -23.0, ul).a)      # the level is the dry utterance's


def parents_draw(lengths, batch, length, n_src, snr_db, align, rng):
    """The draw order of draw_mix_recipe before it knew loudness, restated: per row the utterances, the starts, the SNRs."""
    pool = [i for i, n in enumerate(lengths) if n >= length]
    rows, starts, dbs = [], [], []
    for _ in range(batch):
        row = rng.sample(pool, n_src)
        rows.append(row)
        starts.append([align * rng.randint(0, (lengths[i] - length) // align) for i in row])
        dbs.append([rng.uniform(snr_db[0], snr_db[1]) for _ in row[1:]])
    return np.array(rows), np.array(starts), np.array(dbs)


def test_draw_mix_recipe_without_loudness_is_the_parents_draw_and_with_it_draws_a_target_per_slot():
    D = datas()
    lengths = [48000, 31999, 32000, 100000, 640, 70000, 33000]
    for seed in (7, 8, 1234):
        rows, starts, dbs = parents_draw(lengths, 16, 32000, 3, (-5.0, 5.0), 640, random.Random(seed))
        r = D.draw_mix_recipe(lengths, 16, 32000, n_src=3, align=640, rng=random.Random(seed))
        assert np.array_equal(r.src, rows) and np.array_equal(r.start, starts)
        assert np.array_equal(r.a, np.concatenate([np.ones((16, 1)), 10.0 ** (-dbs / 20.0)], axis=1))
        assert np.array_equal(r.ref_src[:, 1:], np.repeat(rows[:, :1], 2, axis=1)) and (r.rir == -1).all()
    ul = [-20.0, -21.0, -22.0, -23.0, -24.0, -25.0, -26.0]
    rng = random.Random(7)
    pool = [i for i, n in enumerate(lengths) if n >= 32000]
    want_src, want_start, want_t = [], [], []
    for _ in range(16):
        row = rng.sample(pool, 3)
        want_src.append(row)
        want_start.append([640 * rng.randint(0, (lengths[i] - 32000) // 640) for i in row])
        want_t.append([rng.uniform(-33.0, -25.0) for _ in row])
    q = D.draw_mix_recipe(lengths, 16, 32000, n_src=3, align=640, rng=random.Random(7), loudness=(-33.0, -25.0), utter_lufs=ul)
    assert np.array_equal(q.src, want_src) and np.array_equal(q.start, want_start) and (q.ref_src == -1).all()
    assert np.array_equal(q.a, 10.0 ** ((np.array(want_t) - np.array(ul)[np.array(want_src)]) / 20.0))
    with pytest.raises(ValueError):
        D.draw_mix_recipe(lengths, 4, 32000, loudness=(-30.0, -20.0))
    with pytest.raises(ValueError):
        D.draw_mix_recipe(lengths, 4, 32000, utter_lufs=ul)
    with pytest.raises(ValueError):
        D.draw_mix_recipe(lengths, 4, 32000, loudness=(-30.0, -20.0), utter_lufs=ul[:3])
    full = D.draw_mix_recipe(lengths, 4, 32000, rng=random.Random(1), loudness=(-30.0, -20.0), utter_lufs=ul, n_rirs=2, rir_offsets=[3, 4])
    assert (full.rir >= 0).all() and (full.ref_rir == -1).all() and set(full.rir_offset.ravel().tolist()) <= {3, 4}
