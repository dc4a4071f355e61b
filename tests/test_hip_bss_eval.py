"""BSS-eval SDR, SIR and SAR on the MI355X: rtfs_bss_eval_f32 / rtfs_bss_eval_many_f32 / rtfs_debug_bss_eval_f64 (csrc/k_bss.hip) through
metrics.bss_eval, metrics.bss_eval_many and ALLMetricsTracker(bss_eval=True), against the float64 oracle's definition
(tests/bss_eval_oracle.eval_def: dense joint solve, explicit convolutions, time-domain energies; agreement with the mir_eval package itself
is not measured, it is not installed).

Bar: |device - eval_def| <= 1e-4 dB, the project's bar for dB figures, on every regular case (all have L >= 512 J + 512; float32 output
rounding is 4e-6 dB at 60 dB).  The correlation stage is pinned apart from the solve through the debug entry: r_ij at all 1023 lags to
1e-12 of sqrt(r_ii[0] r_jj[0]), p_all to 1e-10 relative, joint order 512 on every regular case.
Measured on the MI355X (each test prints its figures): worst |device - eval_def| 8.8e-7 dB over the eight chunk edges, 9.0e-7 over the
source cases (n = 2, 3, 4, both rules), 8.4e-7 with n = 1 among 1 and 3 others, 1.65e-6 over the nine conditioning cases (at 57 dB:
float32 rounding of the output), 7.5e-7 on the case where the two rules differ, 1.1e-6 in the tracker's columns; r_ij within 1.4e-15
of its scale, D_all 1.2e-15, p_all 4.6e-15 relative; estimate == reference scores 147.5 / 151.8 / 149.5 dB (SDR / SIR / SAR)."""
import csv
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import bss_eval_oracle as E
from tests import bss_oracle as O
from tests import metrics_oracle as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 1e-4
NAMES = ("sdr", "sir", "sar", "sdr_i", "perm")


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(*ts):
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in ts]


def _same(a, b):
    return all((u is None and v is None) or u.tobytes() == v.tobytes() for u, v in zip(a, b))


def run(clean, est, mix=None, others=None, perm_by="sdr"):
    """metrics.bss_eval on numpy (B,n,L) / (B,L) / (B,m,L) arrays -> [sdr, sir, sar, sdr_i | None, perm] as numpy"""
    from rtfs_net_amd.metrics import bss_eval
    return _host(*bss_eval(_dev(clean), _dev(est), _dev(mix), _dev(others), perm_by=perm_by))


def debug(clean, est, mix=None, others=None, perm_by="sdr"):
    """rtfs_debug_bss_eval_f64 -> dict of numpy arrays: the five outputs, r (B,J,J,1023), d (B,n,J,512), pall (B,n), pj (B,n,n), order (B)"""
    from rtfs_net_amd import _lib
    lib = _lib.load()
    B, n, L = clean.shape
    m = 0 if others is None else others.shape[1]
    J = n + m
    c, e, mx, o = _dev(clean), _dev(est), _dev(mix), _dev(others)
    f32 = lambda *s: _lib.empty(*s, device=DEV, dtype=torch.float32)  # noqa: E731
    f64 = lambda *s: _lib.empty(*s, device=DEV, dtype=torch.float64)  # noqa: E731
    out = dict(sdr=f32(B, n), sir=f32(B, n), sar=f32(B, n), sdr_i=None if mix is None else f32(B, n),
               perm=_lib.empty(B, n, device=DEV, dtype=torch.int32), r=f64(B, J, J, 2 * O.F - 1), d=f64(B, n, J, O.F), pall=f64(B, n),
               pj=f64(B, n, n), order=_lib.empty(B, device=DEV, dtype=torch.int32))
    ws = _lib.workspace(lib.rtfs_bss_eval_workspace_bytes(B, n, m, L, int(mix is not None)), DEV)
    P = _lib.ptr
    _lib.check(lib.rtfs_debug_bss_eval_f64(P(c), P(e), P(mx), P(o), B, n, m, L, P(ws), ws.numel(), P(out["sdr"]), P(out["sir"]), P(out["sar"]),
                                           P(out["sdr_i"]), P(out["perm"]), {"sdr": 0, "sir": 1}[perm_by], P(out["r"]), P(out["d"]),
                                           P(out["pall"]), P(out["pj"]), P(out["order"]), _lib.stream_of(c)), "rtfs_debug_bss_eval_f64")
    return dict(zip(out, _host(*out.values())))


@functools.lru_cache(maxsize=None)
def want(name, perm_by="sdr"):
    """the definition's figures of a named regular case; computed once"""
    clean, est, others, mix = E.regular_cases()[name]
    return E.eval_def(clean, est, others, mix, perm_by)


def _against(name, got, perm_by="sdr", row=0):
    """worst |device - eval_def| over the figures of one case; asserts the bar and the permutation"""
    w = want(name, perm_by)
    assert got[4][row].tolist() == w[4], (name, got[4][row], w[4])
    worst = 0.0
    for k in range(4):
        if w[k] is None:
            assert got[k] is None
            continue
        err = np.abs(got[k][row].astype(np.float64) - w[k]).max()
        print(f"{name} by {perm_by}: {NAMES[k]} device {got[k][row].tolist()} oracle {w[k].tolist()} |diff| {err:.2e}")
        worst = max(worst, err)
    assert worst <= BAR, (name, worst)
    return worst


def _call(name, perm_by="sdr", fn=run):
    clean, est, others, mix = E.regular_cases()[name]
    return fn(clean[None], est[None], None if mix is None else mix[None], None if others is None else others[None], perm_by)


# ---------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("L", E.EDGE_LENGTHS)
def test_chunk_edges_and_the_correlation_stage(L):
    name = f"edge_L{L}"
    clean, est, others, _ = E.regular_cases()[name]
    got = _call(name, fn=debug)
    _against(name, [got[k] for k in NAMES])
    assert _same(_call(name), [got[k] for k in NAMES])  # the debug entry is the production call
    S = np.concatenate([clean, others]).astype(np.float64)
    R = E.cross_correlations(S)
    full = np.concatenate([R[:0:-1].transpose(0, 2, 1), R]).transpose(1, 2, 0)  # (J, J, 1023): lag k at 511 + k
    scale = np.sqrt(np.outer(np.diag(R[0]), np.diag(R[0])))[:, :, None]
    err_r = (np.abs(got["r"][0] - full) / scale).max()
    D = E.right_hand_side(S, est[0])
    p_all = float(np.sum(E.joint_taps(S, est[0]) * D))
    err_d = np.abs(got["d"][0, 0] - D.T).max() / np.sqrt(R[0][0][0] * np.dot(est[0].astype(np.float64), est[0].astype(np.float64)))
    err_p = abs(got["pall"][0, 0] - p_all) / p_all
    print(f"{name}: r_ij {err_r:.2e} D_all {err_d:.2e} p_all {err_p:.2e} order {got['order'][0]}")
    assert err_r <= 1e-12 and err_d <= 1e-12 and err_p <= 1e-10 and got["order"][0] == 512


@pytest.mark.parametrize("perm_by", ["sdr", "sir"])
@pytest.mark.parametrize("tag", ["src2", "src2i", "src3", "src4"])
def test_source_cases_by_both_rules(tag, perm_by):
    got = _call(tag, perm_by, fn=debug)
    worst = _against(tag, [got[k] for k in NAMES], perm_by)
    assert got["order"][0] == 512
    print(f"{tag} by {perm_by}: max |device - eval_def| = {worst:.2e} dB")


@pytest.mark.parametrize("m", [1, 3])
def test_one_scored_source_among_others(m):
    got = _call(f"others{m}", fn=debug)
    worst = _against(f"others{m}", [got[k] for k in NAMES])
    assert got["order"][0] == 512
    print(f"n = 1, m = {m}: max |device - eval_def| = {worst:.2e} dB")


def test_conditioning_by_level():
    names = [f"cond{p}_{level:g}" for p in range(len(E.COND_PAIRS)) for level in E.COND_LEVELS]
    cases = [E.regular_cases()[k] for k in names]
    clean, est, others = (np.stack([c[k] for c in cases]) for k in range(3))
    got = debug(clean, est, None, others)
    assert (got["order"] == 512).all(), got["order"]
    worst = max(_against(k, [got[f] for f in NAMES], row=b) for b, k in enumerate(names))
    print(f"conditioning: max |device - eval_def| = {worst:.2e} dB over {len(names)} cases")


def test_the_two_permutation_rules_differ_where_they_should():
    clean, est = E.sir_perm_case()
    by_sdr, by_sir = run(clean[None], est[None]), run(clean[None], est[None], perm_by="sir")
    assert by_sdr[4][0].tolist() == [0, 1] and by_sir[4][0].tolist() == [1, 0]
    for got, rule in ((by_sdr, "sdr"), (by_sir, "sir")):
        w = E.eval_def(clean, est, perm_by=rule)
        assert got[4][0].tolist() == w[4]
        for k in range(3):
            err = np.abs(got[k][0] - w[k]).max()
            print(f"perm by {rule}: {NAMES[k]} {got[k][0].tolist()} oracle {w[k].tolist()} |diff| {err:.2e}")
            assert err <= BAR


def test_input_ranks_are_mirrored():
    from rtfs_net_amd.metrics import bss_eval
    clean, est, others = (np.stack([E.edge_case(L)[k][0] for L in (4096, 4096)]) for k in range(3))  # (2,L)
    mix = (clean + others).astype(np.float32)
    full = run(clean[:, None], est[:, None], mix, others[:, None])
    c, e, m, o = _dev(clean), _dev(est), _dev(mix), _dev(others)
    flat = bss_eval(c, e, m, o[:, None])                      # (B,L): n_src = 1
    assert all(t.shape == (2,) for t in flat) and _same(_host(*flat), [v[:, 0] for v in full])
    solo = bss_eval(c[1], e[1], others=o[1:2])                # (L,), others (m,L)
    assert solo.sdr_i is None and solo.sir.shape == () and _host(solo.sir)[0].tobytes() == full[1][1, 0].tobytes()
    assert solo._fields == NAMES


# ---------------------------------------------------------------- 2. bits
def _batch(B, n, m, L, seed):
    rng = np.random.default_rng(seed)
    clean = np.stack([[O.coloured(rng, L, O.REFERENCES[(b + j) % 5]) for j in range(n)] for b in range(B)])
    others = np.stack([[O.coloured(rng, L, O.REFERENCES[(b + j + 2) % 5]) for j in range(m)] for b in range(B)]) if m else None
    est = np.stack([[O.noisy(rng, clean[b, (j + b) % n], "white", 0.1 + 0.05 * j, "white") for j in range(n)] for b in range(B)])
    mix = clean.sum(1) + (others.sum(1) if m else 0.0)
    est = (est + 0.2 * mix[:, None]).astype(np.float32)  # every estimate holds some of every source
    return clean, est, mix.astype(np.float32), others


def _rows(args, sl):
    return [None if a is None else a[sl] for a in args]


@pytest.mark.parametrize("n,m", [(1, 1), (2, 0), (2, 2)])
def test_perm_by_sdr_gives_the_bits_of_bss_sdr(n, m):
    from rtfs_net_amd.metrics import bss_sdr
    clean, est, mix, others = _batch(3, n, m, 8193, 200 + n + m)
    got = run(clean, est, mix, others)
    ref = _host(*bss_sdr(_dev(clean), _dev(est), _dev(mix), return_perm=True))
    assert _same([got[0], got[3], got[4]], ref)
    alone = run(clean, est, None, others)  # without the mixture: the same figures, no sdr_i
    assert alone[3] is None and _same(alone[:3] + alone[4:], got[:3] + got[4:])


@pytest.mark.parametrize("n,m", [(1, 1), (2, 0)])
def test_rows_do_not_depend_on_the_batch(n, m):
    args = _batch(5, n, m, 8193, 210 + n)
    for rule in ("sdr", "sir"):
        full = run(*_rows(args, slice(None)), perm_by=rule)
        for b in range(5):
            clean, est, mix, others = _rows(args, slice(b, b + 1))
            assert _same(run(clean, est, mix, others, rule), [None if v is None else v[b:b + 1] for v in full]), (rule, b)


@pytest.mark.parametrize("n,m", [(1, 1), (2, 0)])
def test_pooled_rows_are_block_rows(n, m):
    from rtfs_net_amd.metrics import bss_eval_many
    recs = [_batch(1, n, m, L, 220 + L % 7) for L in (1024, 4097, 8193, 32003)]
    cleans, ests, mixes = ([_dev(r[k][0]) for r in recs] for k in range(3))
    others = [_dev(r[3][0]) for r in recs] if m else None
    pooled = _host(*bss_eval_many(cleans, ests, mixes, others, perm_by="sir"))
    assert all(v.shape == (4, n) for v in pooled) and all(np.isfinite(v).all() for v in pooled)
    for r, (c, e, mx, o) in enumerate(recs):
        assert _same(run(c, e, mx, o, "sir"), [v[r:r + 1] for v in pooled]), r
    rev = _host(*bss_eval_many(cleans[::-1], ests[::-1], mixes[::-1], others and others[::-1], perm_by="sir"))
    assert _same([v[::-1] for v in rev], pooled)  # the pool's order changes nothing
    alone = bss_eval_many(cleans, ests, None, others, perm_by="sir")  # without mixtures
    assert alone.sdr_i is None and _same(_host(*alone[:3], alone.perm), pooled[:3] + pooled[4:])


def test_graph_capture_replays_eager():
    from rtfs_net_amd.metrics import bss_eval
    clean, est, mix, others = _batch(3, 2, 1, 4097, 230)
    cd, ed, md, od = _dev(clean), _dev(est), _dev(mix), _dev(others)
    eager = bss_eval(cd, ed, md, od, perm_by="sir")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        bss_eval(cd, ed, md, od, perm_by="sir")  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = bss_eval(cd, ed, md, od, perm_by="sir")
    for t, a in ((cd, clean), (ed, est), (md, mix), (od, others)):
        t.copy_(_dev(a[::-1].copy()))  # new inputs in the captured buffers
    g.replay()
    torch.cuda.synchronize()
    for o, e in zip(out, eager):
        assert torch.equal(o, e.flip(0))


# ---------------------------------------------------------------- 3. degenerate rows
def test_degenerate_rows_inside_a_batch():
    from rtfs_net_amd.metrics import bss_sdr
    clean, est, mix, others = _batch(6, 1, 1, 4097, 240)
    clean[1] = 0                      # silent clean source: the joint set is the other source alone
    others[2] = 0                     # silent other: the joint set is the clean source alone
    est[3] = 0                        # silent estimate
    est[4] = clean[4]                 # estimate == reference
    got = debug(clean, est, mix, others)
    sdr, sir, sar = got["sdr"][:, 0], got["sir"][:, 0], got["sar"][:, 0]
    print(f"degenerate rows: sdr {sdr.tolist()} sir {sir.tolist()} sar {sar.tolist()} order {got['order'].tolist()}")
    assert sdr[1] == -np.inf and sir[1] == -np.inf and np.isfinite(sar[1])
    assert sir[2] == np.inf and sar[2].tobytes() == sdr[2].tobytes() and np.isfinite(sdr[2])
    assert np.isnan(sdr[3]) and np.isnan(sir[3]) and np.isnan(sar[3])
    assert (sdr[4] == np.inf or sdr[4] >= 120.0) and (sir[4] == np.inf or sir[4] >= 100.0) and (sar[4] == np.inf or sar[4] >= 100.0)
    assert got["order"].tolist() == [512] * 6 and (got["perm"] == 0).all()
    ref = _host(*bss_sdr(_dev(clean), _dev(est), _dev(mix)))
    assert got["sdr"].tobytes() == ref[0].tobytes() and got["sdr_i"].tobytes() == ref[1].tobytes()
    for b in (0, 5):                  # the regular rows are their solo runs, bit for bit
        assert all(np.isfinite(got[k][b]).all() for k in NAMES)
        assert _same(run(*_rows((clean, est, mix, others), slice(b, b + 1))), [got[k][b:b + 1] for k in NAMES]), b


def test_identical_and_silent_sources_among_two_scored():
    clean, est, mix, _ = _batch(4, 2, 0, 4097, 250)
    clean[1, 1] = clean[1, 0]         # two identical clean sources: M[0] is singular, the recursion stops at order 0, p_all = 0
    clean[2, 1] = 0                   # one silent scored source: the joint set is source 0 alone
    got = debug(clean, est, mix)
    print(f"identical / silent: sdr {got['sdr'].tolist()} sir {got['sir'].tolist()} sar {got['sar'].tolist()} order {got['order'].tolist()}")
    assert got["order"].tolist() == [512, 0, 512, 512]
    assert (got["sir"][1] == np.inf).all() and (got["sar"][1] == -np.inf).all() and np.isfinite(got["sdr"][1]).all()
    assert got["sir"][2, 0] == np.inf and got["sar"][2, 0].tobytes() == got["sdr"][2, 0].tobytes()
    assert got["sdr"][2, 1] == -np.inf and got["sir"][2, 1] == -np.inf
    for b in (0, 3):
        assert _same(run(clean[b:b + 1], est[b:b + 1], mix[b:b + 1]), [got[k][b:b + 1] for k in NAMES]), b


@pytest.mark.parametrize("L", [1, 2, 511, 513, 1023])
def test_short_rows_finish(L):
    """rows below 512 J + 512 samples are rank-deficient by construction: the call finishes, the SDR is bss_sdr's, rows stay independent"""
    from rtfs_net_amd.metrics import bss_sdr
    clean, est, mix, others = _batch(2, 1, 1, L, 260 + L)
    got = run(clean, est, mix, others)
    print(f"L = {L}: sdr {got[0][:, 0].tolist()} sir {got[1][:, 0].tolist()} sar {got[2][:, 0].tolist()}")
    ref = _host(*bss_sdr(_dev(clean), _dev(est), _dev(mix)))
    assert got[0].tobytes() == ref[0].tobytes() and got[3].tobytes() == ref[1].tobytes()
    for b in range(2):
        assert _same(run(*_rows((clean, est, mix, others), slice(b, b + 1))), [v[b:b + 1] for v in got]), b


# ---------------------------------------------------------------- 4. poison, refusals
@pytest.mark.parametrize("byte", [0xFF, 0x7F], ids=["nan", "big"])
def test_poisoned_workspace_and_outputs(monkeypatch, byte):
    from rtfs_net_amd import _lib
    from rtfs_net_amd.metrics import bss_eval_many
    blocks = [_batch(2, 1, 1, 8193, 270), _batch(1, 3, 1, 4097, 271), _batch(2, 2, 0, 1536, 272)]
    recs = [_batch(1, 1, 1, L, 273 + i) for i, L in enumerate((1024, 4097, 9000))]
    cleans, ests, mixes, others = ([_dev(r[k][0]) for r in recs] for k in range(4))

    def go():
        out = [run(*b, perm_by="sir") for b in blocks] + [run(b[0], b[1], None, b[3]) for b in blocks]
        out.append(_host(*bss_eval_many(cleans, ests, mixes, others, perm_by="sir")))
        out.append(_host(*bss_eval_many(cleans, ests, None, others)))
        return out

    clean = go()
    monkeypatch.setattr(_lib, "_POISON", byte)
    poisoned = go()  # _lib.check() verifies the guard band after the workspace of every call
    for a, b in zip(clean, poisoned):
        assert _same(a, b) and all(np.isfinite(v).all() for v in b if v is not None)


def test_refusals_leave_the_launch_count_unchanged():
    from rtfs_net_amd import _lib
    lib = _lib.load()
    P = _lib.ptr
    x = torch.zeros(2, 2, 5000, device=DEV)
    m = torch.zeros(2, 5000, device=DEV)
    out = [torch.zeros(2, 2, device=DEV) for _ in range(4)]
    perm = torch.zeros(2, 2, device=DEV, dtype=torch.int32)
    nb = lib.rtfs_bss_eval_workspace_bytes(2, 2, 2, 5000, 1)
    assert nb > lib.rtfs_bss_eval_workspace_bytes(2, 2, 0, 5000, 1) > lib.rtfs_bss_sdr_workspace_bytes(2, 2, 5000, 1)
    assert lib.rtfs_bss_eval_workspace_bytes(2, 2, 3, 5000, 1) == 0 and lib.rtfs_bss_eval_workspace_bytes(2, 0, 1, 5000, 1) == 0
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    n0 = lib.rtfs_debug_launch_count()

    def call(c=x, e=x, mx=m, o=x, B=2, n=2, k=2, L=5000, w=ws, nbytes=nb, s=out[0], si=out[1], sa=out[2], sdi=out[3], p=perm, by=0):
        return lib.rtfs_bss_eval_f32(P(c), P(e), P(mx), P(o), B, n, k, L, P(w), nbytes, P(s), P(si), P(sa), P(sdi), P(p), by, st)

    assert call(c=None) == -4 and call(e=None) == -4 and call(w=None) == -4 and call(s=None) == -4 and call(si=None) == -4
    assert call(sa=None) == -4 and call(sdi=None) == -4 and call(p=None) == -4 and call(o=None) == -4
    assert call(B=0) == -4 and call(L=0) == -4 and call(n=0) == -4 and call(k=3) == -4 and call(k=-1) == -4 and call(n=5, k=0) == -4
    assert call(by=2) == -4 and call(by=-1) == -4 and call(nbytes=nb - 1) == -2
    plan = (ctypes.c_int * 33)()
    assert lib.rtfs_score_many_plan((ctypes.c_longlong * 2)(5000, 5000), 2, 2, 16000, plan, None) == 0
    own = lib.rtfs_bss_eval_many_workspace_bytes(plan, 2, 1, 1)
    assert own > lib.rtfs_bss_sdr_many_workspace_bytes(plan, 2, 1) and lib.rtfs_bss_eval_many_workspace_bytes(plan, 2, 3, 1) == 0
    assert lib.rtfs_bss_eval_many_workspace_bytes(plan, 3, 1, 1) == 0 and lib.rtfs_bss_eval_many_workspace_bytes(None, 2, 1, 1) == 0
    rows = torch.tensor([x[0].data_ptr(), x[1].data_ptr()], dtype=torch.int64, device=DEV)
    mrows = torch.tensor([m[0].data_ptr(), m[1].data_ptr()], dtype=torch.int64, device=DEV)
    tab = torch.tensor(list(plan), dtype=torch.int32, device=DEV)
    wsm = torch.zeros(own, dtype=torch.uint8, device=DEV)

    def many(fs=16000, n=2, k=1, R=2, nbytes=own, sdi=out[3], o=mrows, by=1):
        return lib.rtfs_bss_eval_many_f32(P(mrows), P(rows), P(rows), P(o), P(tab), plan, R, n, k, fs, P(wsm), nbytes, P(out[0]), P(out[1]),
                                          P(out[2]), P(sdi), P(perm), by, st)

    assert many(fs=10000) == -4 and many(n=1) == -4 and many(R=3) == -4 and many(sdi=None) == -4 and many(o=None) == -4
    assert many(k=3) == -4 and many(by=7) == -4 and many(nbytes=own - 1) == -2
    torch.cuda.synchronize()
    assert lib.rtfs_debug_launch_count() == n0
    assert many() == 0 and call() == 0   # four launches each; all-zero rows are 0 / 0
    torch.cuda.synchronize()
    assert lib.rtfs_debug_launch_count() == n0 + 8 and all(bool(torch.isnan(t).all()) for t in out[:3])


def test_python_refusals():
    from rtfs_net_amd.metrics import bss_eval, bss_eval_many
    x = torch.zeros(2, 2, 600, device=DEV)
    for bad in (dict(others=torch.zeros(2, 3, 600, device=DEV)), dict(others=torch.zeros(2, 1, 599, device=DEV)),
                dict(others=torch.zeros(3, 1, 600, device=DEV)), dict(others=torch.zeros(2, 1, 600, device=DEV, dtype=torch.float64)),
                dict(others=torch.zeros(2, 1, 600)), dict(perm_by="snr"), dict(mix=torch.zeros(2, 599, device=DEV))):
        with pytest.raises(ValueError, match="bss_eval"):
            bss_eval(x, x, **bad)
    rows = [x[0], x[1]]
    for bad in (dict(others=[torch.zeros(3, 600, device=DEV)] * 2), dict(others=[torch.zeros(1, 600, device=DEV)]),
                dict(others=[torch.zeros(1, 599, device=DEV)] * 2), dict(perm_by="best")):
        with pytest.raises(ValueError, match="bss_eval_many"):
            bss_eval_many(rows, rows, **bad)


# ---------------------------------------------------------------- 5. the tracker
def _tracker(tmp_path, name, feed, **kw):
    from rtfs_net_amd.metrics import ALLMetricsTracker
    t = ALLMetricsTracker(str(tmp_path / name), **kw)
    feed(t)
    mean, std = t.get_mean(), t.get_std()
    lists = (list(t.all_bss_sirs), list(t.all_bss_sars)) if kw.get("bss_eval") else None
    t.final()
    return list(csv.DictReader(open(tmp_path / name))), mean, std, lists


@functools.lru_cache(maxsize=None)
def _tracker_case(n):
    """(mix (B,L), clean (B,n,L), est (B,n,L)) speech-like two-talker mixtures, and the oracle's per-row means of sdr, sdr_i, sir, sar;
    n = 1: the second talker is not scored, the oracle's other source is mix - clean in float32 as the tracker forms it"""
    rng = np.random.default_rng(280 + n)
    B, L = 3, 8000
    talk = np.stack([[M.speech_like(rng, L, 16000) for _ in range(2)] for _ in range(B)])
    mix = talk.sum(1).astype(np.float32)
    clean = talk[:, :n]
    est = np.stack([[O.noisy(rng, (clean[b, (n - 1) - j] + np.float32(0.1) * mix[b]).astype(np.float32), "white", 0.1 + 0.1 * j, "white")
                     for j in range(n)] for b in range(B)])
    w = [E.eval_def(clean[b], est[b], (mix[b] - clean[b, 0])[None] if n == 1 else None, mix[b]) for b in range(B)]
    return mix, clean, est, [[float(np.mean(v[k])) for k in (0, 3, 1, 2)] for v in w]  # in the columns' order


@pytest.mark.parametrize("n", [1, 2])
def test_tracker_columns_by_every_entry(tmp_path, n):
    mix, clean, est, wanted = _tracker_case(n)
    md, cd, ed = _dev(mix), _dev(clean), _dev(est)
    keys = [f"k{b}" for b in range(len(mix))]
    kw = dict(estoi=n == 2, bss_eval=True)
    rows, mean, std, lists = _tracker(tmp_path, "batch.csv", lambda t: t.update_batch(md, cd, ed, keys), **kw)
    many = _tracker(tmp_path, "many.csv", lambda t: t.update_many(list(md), list(cd), list(ed), keys), **kw)
    call = _tracker(tmp_path, "call.csv", lambda t: [t(m, c, e, k) for m, c, e, k in zip(md, cd, ed, keys)], **kw)
    _tracker(tmp_path, "sdr_only.csv", lambda t: t.update_batch(md, cd, ed, keys), estoi=n == 2, bss_sdr=True)
    new = ["bss_sdr", "bss_sdr_i", "bss_sir", "bss_sar"]
    names = ["snt_id", "sdr", "sdr_i", "si-snr", "si-snr_i", "pesq", "stoi"] + (["estoi"] if n == 2 else []) + new
    assert list(rows[0]) == names and [r["snt_id"] for r in rows] == keys + ["avg", "std"]
    for other in (many, call):  # the three entries give the same text in the new columns (the same kernels); the same accumulators
        assert [[r[k] for k in new] for r in other[0]] == [[r[k] for k in new] for r in rows]
        assert other[3] == lists
    # without the two columns the file is the one bss_sdr=True writes, byte for byte
    cut = [",".join(line.split(",")[:-2]) for line in open(tmp_path / "batch.csv").read().splitlines()]
    assert cut == open(tmp_path / "sdr_only.csv").read().splitlines()
    worst = 0.0
    for b in range(len(keys)):
        errs = [abs(float(rows[b][k]) - wanted[b][i]) for i, k in enumerate(new)]
        worst = max(worst, *errs)
        assert max(errs) <= BAR, (b, rows[b], wanted[b])
    sirs, sars = lists
    assert sirs == [float(r["bss_sir"]) for r in rows[:-2]] and sars == [float(r["bss_sar"]) for r in rows[:-2]]
    assert mean["bss_sir"] == np.mean(sirs) and std["bss_sar"] == np.std(sars)
    assert float(rows[-2]["bss_sir"]) == mean["bss_sir"] and float(rows[-1]["bss_sir"]) == std["bss_sir"]
    assert float(rows[-2]["bss_sar"]) == mean["bss_sar"] and float(rows[-1]["bss_sar"]) == std["bss_sar"]
    print(f"tracker (n = {n}): max |column - oracle| = {worst:.2e} dB; bss_sir {sirs} bss_sar {sars}")


def test_tracker_without_the_option_is_unchanged(tmp_path):
    mix, clean, est, _ = _tracker_case(1)
    md, cd, ed = _dev(mix), _dev(clean), _dev(est)
    keys = [f"k{b}" for b in range(len(mix))]
    plain = _tracker(tmp_path, "plain.csv", lambda t: t.update_batch(md, cd, ed, keys))
    assert list(plain[0][0]) == ["snt_id", "sdr", "sdr_i", "si-snr", "si-snr_i", "pesq", "stoi"] and "bss_sir" not in plain[1]
    full = _tracker(tmp_path, "full.csv", lambda t: t.update_batch(md, cd, ed, keys), bss_eval=True)
    for a, b in zip(plain[0], full[0]):  # the columns the tracker had do not notice the four
        assert all(b[k] == v or (k == "pesq" and v == "nan") for k, v in a.items()), (a, b)
    from rtfs_net_amd.metrics import ALLMetricsTracker
    t = ALLMetricsTracker(str(tmp_path / "record.csv"), bss_eval=True)
    with pytest.raises(ValueError, match="takes 9"):
        t.record(["a"], np.zeros((1, 7), np.float32), [0.0])
    t.record(["a"], np.arange(9, dtype=np.float32)[None], [0.0])
    assert (t.all_bss_sdrs, t.all_bss_sdrs_i, t.all_bss_sirs, t.all_bss_sars) == ([5.0], [6.0], [7.0], [8.0])
    t.final()
