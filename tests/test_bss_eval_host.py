"""Host side of BSS-eval SIR and SAR: the float64 oracle (tests/bss_eval_oracle.py) -- the definition (dense joint solve, explicit
convolutions, time-domain energies) against the closed forms the device takes, the numpy restatement of the device's block Levinson
against the dense solve, and the properties the figures have by construction -- then the C entries' declarations, bindings, workspace
sizes and refusals through ctypes, and the tracker's two columns through ``record`` alone.  None of it touches a device.
Measured: max |eval_def - eval_moments| = 1.5e-8 dB over the 23 regular cases of the GPU file and the permutation case (bound 1e-6;
joint condition numbers up to 7.0e6); block Levinson against the dense solve 8.8e-9 dB over the nine conditioning cases and n = 4."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from tests import bss_eval_oracle as E
from tests import bss_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"rtfs_bss_eval_workspace_bytes": "size_t", "rtfs_bss_eval_f32": "int", "rtfs_bss_eval_many_workspace_bytes": "size_t",
           "rtfs_bss_eval_many_f32": "int", "rtfs_debug_bss_eval_f64": "int"}


def lib():
    from rtfs_net_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------- the oracle
def test_definition_and_closed_forms_agree_on_every_case():
    cases = dict(E.regular_cases())
    cases["perm"] = E.sir_perm_case() + (None, None)
    worst = 0.0
    for name, (clean, est, others, mix) in cases.items():
        assert clean.shape[1] >= 512 * (len(clean) + (0 if others is None else len(others))) + 512, name  # the Gram matrix has full rank
        for rule in ("sdr", "sir") if len(clean) > 1 else ("sdr",):  # one scored source: one permutation
            a, b = E.eval_def(clean, est, others, mix, rule), E.eval_moments(clean, est, others, mix, rule)
            assert a[4] == b[4], (name, rule)
            for k in range(4):
                if a[k] is not None:
                    assert np.isfinite(a[k]).all() and np.isfinite(b[k]).all() and a[k].max() <= 61.0, (name, a[k], b[k])
                    worst = max(worst, np.abs(a[k] - b[k]).max())
    print(f"max |eval_def - eval_moments| = {worst:.2e} dB over {len(cases)} cases")
    assert worst <= 1e-6 and len(cases) == 24


def test_block_levinson_restatement_against_the_dense_solve():
    worst = 0.0
    pairs = [E.cond_case(p, level) for p in range(len(E.COND_PAIRS)) for level in E.COND_LEVELS]
    pairs.append((O.source_case(4)[0], O.source_case(4)[1][:1], None))
    for clean, est, others in pairs:
        S = clean if others is None else np.concatenate([clean, others])
        R, D = E.cross_correlations(S), E.right_hand_side(S, est[0])
        C, order = E.block_levinson(R, D[:, :, None])
        assert order == 512
        dense = E.figures_moments(S, 0, est[0])
        lev = E.figures_moments(S, 0, est[0], C[:, :, 0])
        worst = max(worst, *(abs(a - b) for a, b in zip(dense, lev)))
    print(f"block Levinson against the dense solve: max {worst:.2e} dB over {len(pairs)} systems")
    assert worst <= 1e-6


def test_one_source_is_the_scalar_projection():
    for name, s, e in list(O.conditioning_cases())[:6]:
        sdr, sir, sar, _, perm = E.eval_moments(s[None], e[None])
        assert sdr[0] == O.sdr_moments(s, e) and sir[0] == np.inf and sar[0] == sdr[0] and perm == [0], name
    s, e = O.conditioning_cases()[0][1:]
    sdr, sir, sar, _, _ = E.eval_def(s[None], e[None])
    assert abs(sdr[0] - O.sdr_lu(s, e)) <= 1e-9 and (sir[0] == np.inf or sir[0] >= 200.0) and abs(sar[0] - sdr[0]) <= 1e-6


def test_a_silent_other_reduces_to_one_source():
    clean, est, others = E.edge_case(4097)
    alone = E.eval_moments(clean, est)
    silent = E.eval_moments(clean, est, np.zeros_like(others))
    assert all(np.array_equal(a, b) for a, b in zip(alone[:3], silent[:3])) and silent[1][0] == np.inf
    loud = E.eval_moments(clean, est, others)
    assert loud[0][0] == alone[0][0] and np.isfinite(loud[1][0]) and loud[2][0] > alone[2][0]  # the SDR does not see the others
    C, order = E.block_levinson(E.cross_correlations(np.concatenate([clean, np.zeros_like(others)])),
                                E.right_hand_side(np.concatenate([clean, others * 0]), est[0])[:, :, None])
    assert order == 512 and (C[:, 1] == 0).all() and np.abs(C[:, 0]).max() > 0  # the solver's own rule: decoupled, taps 0


def test_the_stop_rule_fires_on_identical_sources():
    clean, est, _ = E.edge_case(4097)
    S = np.concatenate([clean, clean])
    C, order = E.block_levinson(E.cross_correlations(S), E.right_hand_side(S, est[0])[:, :, None])
    assert order == 0 and (C == 0).all()


def test_sir_rule_differs_from_sdr_rule_and_is_the_brute_force_search():
    clean, est = E.sir_perm_case()
    by_sdr, by_sir = E.eval_moments(clean, est, perm_by="sdr"), E.eval_moments(clean, est, perm_by="sir")
    assert by_sdr[4] == [0, 1] and by_sir[4] == [1, 0]
    for n, (cl, es) in ((2, (clean, est)), (3, O.source_case(3)[:2])):
        S = cl.astype(np.float64)
        sir = [[E.figures_moments(S, j, es[i])[1] for j in range(n)] for i in range(n)]
        best = max(itertools.permutations(range(n)), key=lambda p: np.mean([sir[p[j]][j] for j in range(n)]))
        got = E.eval_moments(cl, es, perm_by="sir")
        assert got[4] == list(best) and np.allclose(got[1], [sir[best[j]][j] for j in range(n)], atol=1e-9)
    with pytest.raises(ValueError):
        E.eval_moments(clean, est, perm_by="snr")


# ---------------------------------------------------------------- the C entries
def test_symbols_in_header_bindings_and_library():
    from rtfs_net_amd import _lib
    with open(os.path.join(ROOT, "include", "rtfs_amd.h")) as f:
        text = f.read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, res in SYMBOLS.items():
        decl = re.search(r"\b" + res + " " + name + r"\(([^;]*)\);", header)
        assert decl, name
        fn = getattr(lib(), name)
        assert name in _lib.SIGNATURES and getattr(fn, "__wrapped__", fn).argtypes == _lib.SIGNATURES[name][1]
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert "#define RTFS_BSS_PERM_BY_SDR 0" in text and "#define RTFS_BSS_PERM_BY_SIR 1" in text
    import rtfs_net_amd
    from rtfs_net_amd import metrics
    assert rtfs_net_amd.bss_eval is metrics.bss_eval and rtfs_net_amd.bss_eval_many is metrics.bss_eval_many
    assert metrics._PERM_BY == {"sdr": 0, "sir": 1}


def _plan(Ls, n_src=1, fs=16000):
    R = len(Ls)
    table = (ctypes.c_int * (11 * (R + 1)))()
    assert lib().rtfs_score_many_plan((ctypes.c_longlong * R)(*Ls), R, n_src, fs, table, None) == 0
    return table


def _bytes(G, rows, n, m, with_mix):
    """the three regions of the SDR (partials (G, n, 1 + NR, 512), sums of squares (G, NR), num / den (rows, n, NR, 2)), then the joint
    partials (G, J, J + n, 512) and p_all / ee (rows, n, 2), each starting at a multiple of 256"""
    NR, J, up = n + with_mix, n + m, lambda v: -(-v // 256) * 256
    sdr = up(up(8 * G * n * (1 + NR) * 512) + 8 * G * NR) + 8 * rows * n * NR * 2
    return up(up(sdr) + 8 * G * J * (J + n) * 512) + 8 * rows * n * 2


def test_workspace_sizes():
    L_ = lib()
    for B, n, m, L, wm in ((1, 1, 0, 1, 0), (1, 1, 1, 4096, 1), (3, 2, 2, 4097, 1), (5, 4, 0, 32003, 0), (256, 1, 1, 32000, 1), (2, 1, 3, 9000, 0)):
        assert L_.rtfs_bss_eval_workspace_bytes(B, n, m, L, wm) == _bytes(B * -(-L // O.CHUNK), B, n, m, wm), (B, n, m, L, wm)
        assert L_.rtfs_bss_eval_workspace_bytes(B, n, m, L, wm) > L_.rtfs_bss_sdr_workspace_bytes(B, n, L, wm)
    for bad in ((0, 1, 0, 100, 0), (1, 0, 1, 100, 0), (1, 5, 0, 100, 1), (1, 2, 3, 100, 1), (1, 1, -1, 100, 0), (1, 1, 0, 0, 0)):
        assert L_.rtfs_bss_eval_workspace_bytes(*bad) == 0
    for Ls, n, m in (([410, 6554, 1639], 1, 1), ([6553, 410, 32769, 64003], 2, 0), ([4096, 4097, 8193], 2, 2)):
        tab, R = _plan(Ls, n), len(Ls)
        G = sum(-(-L // O.CHUNK) for L in Ls)
        for wm in (0, 1):
            assert L_.rtfs_bss_eval_many_workspace_bytes(tab, R, m, wm) == _bytes(G, R, n, m, wm)
        assert L_.rtfs_bss_eval_many_workspace_bytes(tab, R + 1, m, 1) == 0 and L_.rtfs_bss_eval_many_workspace_bytes(None, R, m, 1) == 0
        assert L_.rtfs_bss_eval_many_workspace_bytes(tab, R, 4, 1) == 0 and L_.rtfs_bss_eval_many_workspace_bytes(tab, R, -1, 1) == 0


def test_refusals_come_before_any_device_is_touched():
    L_ = lib()
    ws = L_.rtfs_bss_eval_workspace_bytes(2, 2, 1, 5000, 1)
    n0 = L_.rtfs_debug_launch_count()
    ok = dict(clean=8, est=8, mix=8, other=8, B=2, n=2, m=1, L=5000, ws=8, nb=ws, sdr=8, sir=8, sar=8, sdr_i=8, perm=8, by=1)

    def block(**kw):
        a = {**ok, **kw}
        return L_.rtfs_bss_eval_f32(a["clean"], a["est"], a["mix"], a["other"], a["B"], a["n"], a["m"], a["L"], a["ws"], a["nb"], a["sdr"],
                                    a["sir"], a["sar"], a["sdr_i"], a["perm"], a["by"], None)

    for key in ("clean", "est", "other", "ws", "sdr", "sir", "sar", "sdr_i", "perm"):
        assert block(**{key: None}) == -4, key
    for kw in (dict(B=0), dict(B=-1), dict(L=0), dict(n=0), dict(n=4), dict(m=3), dict(m=-1), dict(n=5, m=0), dict(by=2), dict(by=-1)):
        assert block(**kw) == -4, kw
    assert block(nb=ws - 1) == -2 and block(nb=0) == -2
    assert block(mix=None, sdr_i=None, other=None, m=0, nb=L_.rtfs_bss_eval_workspace_bytes(2, 2, 0, 5000, 0) - 1) == -2
    dbg = lambda r=8, o=8, nb=ws: L_.rtfs_debug_bss_eval_f64(8, 8, 8, 8, 2, 2, 1, 5000, 8, nb, 8, 8, 8, 8, 8, 0, r, 8, 8, 8, o, None)  # noqa: E731
    assert dbg(r=None) == -4 and dbg(o=None) == -4 and dbg(nb=ws - 1) == -2
    tab = _plan([32000, 410], 2)
    own = L_.rtfs_bss_eval_many_workspace_bytes(tab, 2, 1, 1)

    def many(mixes=8, cleans=8, ests=8, others=8, table=8, plan=tab, R=2, n=2, m=1, fs=16000, ws_=8, nb=own, sdr=8, sir=8, sar=8, sdr_i=8,
             perm=8, by=0):
        return L_.rtfs_bss_eval_many_f32(mixes, cleans, ests, others, table, plan, R, n, m, fs, ws_, nb, sdr, sir, sar, sdr_i, perm, by, None)

    for kw in (dict(cleans=None), dict(ests=None), dict(others=None), dict(table=None), dict(plan=None), dict(ws_=None), dict(sdr=None),
               dict(sir=None), dict(sar=None), dict(sdr_i=None), dict(perm=None), dict(fs=10000), dict(fs=8000), dict(n=1), dict(n=5),
               dict(m=3), dict(R=3), dict(R=0), dict(by=2)):
        assert many(**kw) == -4, kw
    assert many(nb=own - 1) == -2
    assert many(mixes=None, sdr_i=None, others=None, m=0, nb=L_.rtfs_bss_eval_many_workspace_bytes(tab, 2, 0, 0) - 1) == -2
    assert L_.rtfs_debug_launch_count() == n0


def test_python_entries_refuse_before_any_launch():
    import torch
    from rtfs_net_amd.metrics import bss_eval, bss_eval_many
    x = torch.zeros(2, 2, 1000)
    with pytest.raises(ValueError, match="same"):
        bss_eval(x, torch.zeros(2, 2, 999))
    with pytest.raises(ValueError, match="mix must be"):
        bss_eval(x, x, torch.zeros(2, 999))
    with pytest.raises(ValueError, match=r"others must be \(B, m, L\)"):
        bss_eval(x, x, others=torch.zeros(2, 1000))
    with pytest.raises(ValueError, match=r"others must be \(m, L\)"):
        bss_eval(x[0, 0], x[0, 0], others=torch.zeros(1, 1, 1000))
    with pytest.raises(ValueError, match=r"n_src \+ others <= 4, got 2 \+ 3"):
        bss_eval(x, x, others=torch.zeros(2, 3, 1000))
    with pytest.raises(ValueError, match="float32"):
        bss_eval(x, x, others=torch.zeros(2, 1, 1000, dtype=torch.float64))
    with pytest.raises(ValueError, match="perm_by must be"):
        bss_eval(x, x, perm_by="snr")
    with pytest.raises(ValueError, match="empty"):
        bss_eval(torch.zeros(2, 2, 0), torch.zeros(2, 2, 0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bss_eval(x, x, others=torch.zeros(2, 2, 1000), perm_by="sir")
    with pytest.raises(ValueError, match="others 1 must be a float32 tensor"):
        bss_eval_many([x[0], x[1]], [x[0], x[1]], others=[torch.zeros(1, 1000), torch.zeros(1, 999)])
    with pytest.raises(ValueError, match="others 1 holds 2"):
        bss_eval_many([x[0], x[1]], [x[0], x[1]], others=[torch.zeros(1, 1000), torch.zeros(2, 1000)])
    with pytest.raises(ValueError, match="others 0 holds 3"):
        bss_eval_many([x[0]], [x[0]], others=[torch.zeros(3, 1000)])
    with pytest.raises(ValueError, match="sequences of"):
        bss_eval_many([x[0], x[1]], [x[0], x[1]], others=[torch.zeros(1, 1000)])
    with pytest.raises(ValueError, match="perm_by must be"):
        bss_eval_many([x[0]], [x[0]], perm_by="best")
    with pytest.raises(ValueError, match="no CPU fallback"):
        bss_eval_many([x[0]], [x[0]], others=[torch.zeros(1000)])


# ---------------------------------------------------------------- the tracker through record alone
@pytest.mark.parametrize("estoi", [False, True])
def test_tracker_records_the_two_columns(tmp_path, estoi):
    import csv
    from rtfs_net_amd.metrics import ALLMetricsTracker
    rng = np.random.default_rng(7)
    n = 4
    vals = np.stack([-rng.uniform(5, 15, n), rng.uniform(-12, -3, n), -rng.uniform(4, 14, n), rng.uniform(-11, -2, n), rng.uniform(0.5, 0.95, n)]
                    + ([rng.uniform(0.3, 0.9, n)] if estoi else [])
                    + [rng.uniform(8, 30, n), rng.uniform(3, 20, n), rng.uniform(10, 40, n), rng.uniform(9, 35, n)], 1).astype(np.float32)
    t = ALLMetricsTracker(str(tmp_path / "t.csv"), estoi=estoi, bss_eval=True)
    assert t.bss_sdr and t.bss_eval
    t.record([f"k{i}" for i in range(n)], vals, [float("nan")] * n)
    assert t.all_bss_sdrs == [float(v) for v in vals[:, -4]] and t.all_bss_sdrs_i == [float(v) for v in vals[:, -3]]
    assert t.all_bss_sirs == [float(v) for v in vals[:, -2]] and t.all_bss_sars == [float(v) for v in vals[:, -1]]
    if estoi:
        assert t.all_estois == [float(v) for v in vals[:, 5]]
    mean, std = t.get_mean(), t.get_std()
    t.final()
    rows = list(csv.DictReader(open(tmp_path / "t.csv")))
    assert list(rows[0]) == ALLMetricsTracker.COLUMNS + (["estoi"] if estoi else []) + ["bss_sdr", "bss_sdr_i", "bss_sir", "bss_sar"]
    assert float(rows[-2]["bss_sir"]) == mean["bss_sir"] == np.mean(t.all_bss_sirs) and float(rows[-1]["bss_sar"]) == std["bss_sar"]
    with pytest.raises(ValueError, match=f"takes {9 + estoi}"):
        ALLMetricsTracker(str(tmp_path / "u.csv"), estoi=estoi, bss_eval=True).record(["a"], vals[:1, :-2], [0.0])
    plain = ALLMetricsTracker(str(tmp_path / "v.csv"), estoi=estoi, bss_sdr=True)  # without the option: the tracker of before
    assert not plain.bss_eval and plain.columns == ALLMetricsTracker.COLUMNS + (["estoi"] if estoi else []) + ["bss_sdr", "bss_sdr_i"]
    plain.record(["a"], vals[:1, :-2], [0.0])
    assert not hasattr(plain, "all_bss_sirs") and "bss_sir" not in plain.get_mean()
