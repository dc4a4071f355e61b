"""Host side of scoring many recordings of different lengths in one pooled pass (rtfs_score_many_plan, metrics.stoi_many / sdr_many,
ALLMetricsTracker.update_many, System.evaluate_many): the bindings, the planner's refusals, its table against a restatement of the
layout documented in include/rtfs_amd.h, the raggedness of the workspace, and every ValueError of the Python entries on CPU tensors.
None of it touches a device."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS = 11
SYMBOLS = ("rtfs_score_many_plan", "rtfs_stoi_many_f32", "rtfs_sdr_many_f32")


def lib():
    from rtfs_net_amd import _lib
    return _lib.load()


def plan(Ls, n_src=1, fs=16000):
    """-> (rc, table as COLS lists of R + 1 words, ws_bytes)"""
    R = len(Ls)
    table = (ctypes.c_int * (COLS * (R + 1)))(*([-7] * (COLS * (R + 1))))
    nbytes = ctypes.c_size_t(0)
    rc = lib().rtfs_score_many_plan((ctypes.c_longlong * max(R, 1))(*Ls), R, n_src, fs, table, ctypes.byref(nbytes))
    t = list(table)
    return rc, [t[c * (R + 1):(c + 1) * (R + 1)] for c in range(COLS)], nbytes.value


def cdiv(a, b):
    return -(-a // b)


def restated_table(Ls, n_src, fs):
    """The layout of include/rtfs_amd.h restated: four per-recording columns, then seven exclusive prefix sums closed by their totals."""
    res = fs == 16000
    L10 = [cdiv(5 * L, 8) if res else L for L in Ls]
    K0 = [cdiv(l - 256, 128) for l in L10]
    Fmax = [k - 1 for k in K0]
    per = [[l if res else 0 for l in L10],                                   # rs_off: floats of the 10 kHz copy
           K0,                                                               # fr_off
           Fmax,                                                             # bd_off
           [cdiv(l, 1024) if res else 0 for l in L10],                       # rs0
           [cdiv(f, 4) for f in Fmax],                                       # bg0
           [cdiv(15 * (f - 29), 256) if f >= 30 else 0 for f in Fmax],       # cc0
           [cdiv(L, 4096) for L in Ls]]                                      # mc0
    cols = [Ls + [n_src], L10 + [fs], K0 + [len(Ls)], Fmax + [0]]
    for p in per:
        cols.append([sum(p[:r]) for r in range(len(Ls) + 1)])
    return cols


def test_symbols_in_header_bindings_and_makefile():
    from rtfs_net_amd import _lib
    with open(os.path.join(ROOT, "include", "rtfs_amd.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SIGNATURES and getattr(lib(), name).argtypes == _lib.SIGNATURES[name][1]
        # as many arguments in the header's declaration as in the binding
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    from rtfs_net_amd import metrics
    assert f"#define RTFS_SCORE_COLS {COLS}" in header and metrics.SCORE_COLS == COLS
    with open(os.path.join(ROOT, "rtfs-net_amd", "csrc", "Makefile")) as f:
        assert "k_score.hip" in f.read().split("SRCS :=", 1)[1].split("\n", 1)[0]


def test_planner_refusals():
    assert plan([], 1, 16000)[0] == -4                      # R = 0
    assert plan([32000], 5, 16000)[0] == -4 and plan([32000], 0, 16000)[0] == -4
    assert plan([32000], 1, 8000)[0] == -4
    assert plan([32000, 409], 1, 16000)[0] == -1 and plan([410], 1, 16000)[0] == 0
    assert plan([256], 1, 10000)[0] == -1 and plan([257], 1, 10000)[0] == 0
    assert plan([(1 << 26) + 1], 1, 16000)[0] == -1
    assert plan([1 << 26] * 64, 4, 16000)[0] == -1          # 64 * 41943040 resampled floats: an offset past int32
    assert lib().rtfs_score_many_plan(None, 1, 1, 16000, (ctypes.c_int * 22)(), None) == -4
    assert lib().rtfs_score_many_plan((ctypes.c_longlong * 1)(32000), 1, 1, 16000, None, None) == -4
    # the launches refuse before they touch a device: null pointers, and a plan made for other arguments
    rc, _, nbytes = plan([32000, 410])
    tab = (ctypes.c_int * (COLS * 3))()
    lib().rtfs_score_many_plan((ctypes.c_longlong * 2)(32000, 410), 2, 1, 16000, tab, None)
    assert lib().rtfs_stoi_many_f32(None, 8, 8, tab, 2, 1, 16000, 8, nbytes, 8, 8, None) == -4
    assert lib().rtfs_stoi_many_f32(8, 8, 8, tab, 2, 1, 10000, 8, nbytes, 8, 8, None) == -4
    assert lib().rtfs_stoi_many_f32(8, 8, 8, tab, 2, 2, 16000, 8, nbytes, 8, 8, None) == -4
    assert lib().rtfs_stoi_many_f32(8, 8, 8, tab, 2, 1, 16000, 8, nbytes - 1, 8, 8, None) == -2
    assert lib().rtfs_sdr_many_f32(8, 8, None, 8, tab, 2, 1, 16000, 8, nbytes, 8, 8, None) == -4
    assert lib().rtfs_sdr_many_f32(8, 8, 8, 8, tab, 3, 1, 16000, 8, nbytes, 8, 8, None) == -4
    assert lib().rtfs_sdr_many_f32(8, 8, 8, 8, tab, 2, 1, 16000, 8, nbytes - 1, 8, 8, None) == -2


@pytest.mark.parametrize("Ls,n_src,fs", [([410, 6554, 1639], 1, 16000), ([6553, 410, 32769, 64003], 2, 16000), ([257, 4097, 20001], 1, 10000)])
def test_table_matches_the_documented_layout(Ls, n_src, fs):
    rc, cols, nbytes = plan(Ls, n_src, fs)
    assert rc == 0
    assert cols == restated_table(Ls, n_src, fs)
    if Ls == [410, 6554, 1639]:  # spelled out once: L10 257 / 4097 / 1025, K0 1 / 31 / 7
        assert cols[1][:3] == [257, 4097, 1025] and cols[2][:3] == [1, 31, 7] and cols[3][:3] == [0, 30, 6]
        assert cols[7] == [0, 1, 6, 8] and cols[8] == [0, 0, 8, 10] and cols[9] == [0, 0, 1, 1] and cols[10] == [0, 1, 3, 4]
    # the nine regions, each rounded up to 256 bytes
    tot = [c[-1] for c in cols]
    moments = 2 * (2 * n_src + 1) + n_src * n_src + n_src
    regions = [4 * tot[4], 4 * tot[4], 8 * tot[5], 4 * tot[5], 4 * len(Ls), 120 * tot[6], 120 * tot[6], 8 * tot[9], 8 * moments * tot[10]]
    off = 0
    for b in regions:
        off = cdiv(off, 256) * 256 + b
    assert nbytes == off


@pytest.mark.parametrize("Ls", [[410, 192000], [32000] * 16], ids=["short_and_12s", "16x2s"])
def test_workspace_is_ragged(Ls):
    """Within the sum of the single-recording STOI plans plus the moment partials (3 signals at n_src 1: 8 doubles per 4096 samples).
    Stated slack: none per recording; the nine regions of the CALL are each rounded up to 256 bytes."""
    L_ = lib()
    rc, cols, nbytes = plan(Ls)
    assert rc == 0
    singles = sum(L_.rtfs_stoi_workspace_bytes(1, L, 16000) for L in Ls)
    moments = sum(cdiv(L, 4096) * 8 * 8 for L in Ls)
    assert nbytes <= singles + moments + 9 * 255
    if Ls == [410, 192000]:
        one = plan([192000])[2]
        assert nbytes < 1.01 * one < 2 * one  # a padded (2, 192000) block would need twice the long recording's


def _rec(L=32000, n=1, dtype=torch.float32):
    return torch.zeros(L, dtype=dtype), torch.zeros(n, L, dtype=dtype), torch.zeros(n, L, dtype=dtype)


def test_python_entries_refuse_with_the_recording_index(tmp_path):
    from rtfs_net_amd.metrics import ALLMetricsTracker, sdr_many, stoi_many
    from rtfs_net_amd.system import System
    tracker = ALLMetricsTracker(str(tmp_path / "m.csv"))
    m, c, e = _rec()
    good = ([m], [c], [e])

    def each(match, mixes, cleans, ests, stoi_too=True):
        """every entry refuses the same pool with the same reason"""
        with pytest.raises(ValueError, match=match):
            sdr_many(mixes, cleans, ests)
        with pytest.raises(ValueError, match=match):
            tracker.update_many(mixes, cleans, ests, [f"k{r}" for r in range(len(cleans))])
        if stoi_too:
            with pytest.raises(ValueError, match=match):
                stoi_many([x[0] for x in cleans], [x[0] for x in ests])

    each("at least 1", [], [], [])
    each("same number", [m, m], [c, c], [e])
    with pytest.raises(ValueError, match="same number"):
        tracker.update_many([m], [c], [e], ["a", "b"])
    each("recording 1 must be", [m, m[None, None]], [c, c], [e, e], stoi_too=False)             # wrong rank
    each("recording 1 must be", [m, m], [c, c[0]], [e, e], stoi_too=False)
    with pytest.raises(ValueError, match="estimate 1 must be"):
        stoi_many([c[0], c], [e[0], torch.zeros(2, 32000)])
    m2, c2, e2 = _rec(n=2)
    each("recording 1 has 2 clean and 2 estimated", [m, m2], [c, c2], [e, e2], stoi_too=False)   # n_src differs between recordings
    each("recording 1 has 1 clean and 2 estimated", [m, m], [c, c], [e, e2], stoi_too=False)     # ... between clean and estimate
    each("n_src 1 .. 4", [m], [torch.zeros(5, 32000)], [torch.zeros(5, 32000)], stoi_too=False)
    each("recording 1 has lengths", [m, m], [c, c], [e, e[:, :-1]])                              # length mismatch inside a recording
    each("recording 1 has lengths", [m, m[:-1]], [c, c], [e, e], stoi_too=False)
    md, cd, ed = _rec(dtype=torch.float64)
    each("recording 1 is .*float64", [m, md], [c, cd], [e, ed])
    ms, cs, es = _rec(L=409)
    each("recording 2 has 409 samples", [m, m, ms], [c, c, cs], [e, e, es])                      # a length the planner refuses
    with pytest.raises(ValueError, match="recording 0 has 256 samples"):
        stoi_many([torch.zeros(256)], [torch.zeros(256)], fs=10000)
    with pytest.raises(ValueError, match="fs must be"):
        stoi_many([c[0]], [e[0]], fs=8000)
    each("no CPU fallback", *good)                                                                # CPU tensors
    mm, cm, em = (t.to("meta") for t in (m, c, e))
    each("recording 1 lies on", [m, m], [c, cm], [e, e])                                          # mixed devices
    assert not hasattr(stoi_many, "extended") and "extended" not in stoi_many.__code__.co_varnames
    # evaluate_many is separate_many, then update_many: its signature, and nothing written by the refusals above
    import inspect
    assert list(inspect.signature(System.evaluate_many).parameters)[:6] == ["self", "wavs", "cleans", "mouths", "keys", "tracker"]
    assert tracker.all_stois == []
    tracker.results_csv.close()
