"""BSS-eval SDR on the MI355X: rtfs_bss_sdr_f32 / rtfs_bss_sdr_many_f32 / rtfs_debug_bss_f64 (csrc/k_bss.hip) through metrics.bss_sdr,
metrics.bss_sdr_many and ALLMetricsTracker(bss_sdr=True), against the float64 oracle's definition (tests/bss_oracle.sdr_lu: dense solve,
explicit convolution, time-domain energies; agreement with the mir_eval package itself is not measured, it is not installed).

Bar: |device - sdr_lu| <= 1e-4 dB, the project's bar for dB figures, on every regular case (all at or below 60.3 dB, where float32
output rounding is 4e-6 dB).  At L = 1 every estimate is a multiple of the reference, so those two rows are held to the rule of the
degenerate "estimate == reference" rows instead: +inf or >= 120 dB.  Stage 1 is pinned apart from the solve through the debug entry:
r, d to 1e-12 of r[0] (resp. sqrt(r[0] ee)), ee to 1e-12 relative, order 512 reached on every regular case, with both solver forms.
Measured on the MI355X (each test prints its figures): worst |device - sdr_lu| 1.66e-6 dB over the 15 conditioning x SDR cases (at 60 dB:
float32 rounding of the output), 6.1e-7 over the length edges, 9.0e-7 over the source cases, 4.2e-7 in the tracker's columns; r, d and ee
within 1.7e-15 of their scale; estimate == reference scores 147.5 dB.  The two solver forms gave equal values on every case."""
import csv
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import bss_oracle as O
from tests import metrics_oracle as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 1e-4


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(*ts):
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in ts]


@functools.lru_cache(maxsize=None)
def _pairs():
    return {name: (s, e) for name, s, e in O.all_pairs()}


@functools.lru_cache(maxsize=None)
def lu(name):
    """the definition's value of a named pair of the case sets; computed once"""
    return O.sdr_lu(*_pairs()[name])


def debug(clean, est, mix=None, form=0):
    """rtfs_debug_bss_f64 on (B,n,L) arrays -> dict of numpy arrays: sdr, sdr_i, perm, r (B,n,512), d (B,n,NR,512), ee (B,n,NR), order (B,n)"""
    from rtfs_net_amd import _lib
    lib = _lib.load()
    B, n, L = clean.shape
    NR = n + (mix is not None)
    c, e, m = _dev(clean), _dev(est), None if mix is None else _dev(mix)
    f32 = lambda *s: _lib.empty(*s, device=DEV, dtype=torch.float32)  # noqa: E731
    f64 = lambda *s: _lib.empty(*s, device=DEV, dtype=torch.float64)  # noqa: E731
    out = dict(sdr=f32(B, n), sdr_i=None if mix is None else f32(B, n), perm=_lib.empty(B, n, device=DEV, dtype=torch.int32),
               r=f64(B, n, O.F), d=f64(B, n, NR, O.F), ee=f64(B, n, NR), order=_lib.empty(B, n, device=DEV, dtype=torch.int32))
    ws = _lib.workspace(lib.rtfs_bss_sdr_workspace_bytes(B, n, L, int(mix is not None)), DEV)
    P = _lib.ptr
    _lib.check(lib.rtfs_debug_bss_f64(P(c), P(e), P(m), B, n, L, P(ws), ws.numel(), P(out["sdr"]), P(out["sdr_i"]), P(out["perm"]), form,
                                      P(out["r"]), P(out["d"]), P(out["ee"]), P(out["order"]), _lib.stream_of(c)), "rtfs_debug_bss_f64")
    return dict(zip(out, _host(*out.values())))


def run(clean, est, mix=None):
    """metrics.bss_sdr on numpy arrays -> (sdr, sdr_i | None, perm) as numpy"""
    from rtfs_net_amd.metrics import bss_sdr
    out = bss_sdr(_dev(clean), _dev(est), None if mix is None else _dev(mix), return_perm=True)
    sdr, sdr_i, perm = (out[0], None, out[1]) if mix is None else out
    return _host(sdr, sdr_i, perm)


def _same(a, b):
    return all((u is None and v is None) or u.tobytes() == v.tobytes() for u, v in zip(a, b))


# ---------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("L", O.LENGTH_EDGES)
def test_length_edges(L):
    cases = [c for c in O.length_cases() if len(c[1]) == L]
    assert len(cases) == 2
    for name, s, e in cases:
        r, d, ee = O.correlations(s, e)
        prod = run(s[None, None], e[None, None])
        for form in (0, 64, 512):
            got = debug(s[None, None], e[None, None], form=form)
            err_r = np.abs(got["r"][0, 0] - r).max() / r[0]
            err_d = np.abs(got["d"][0, 0, 0] - d).max() / np.sqrt(r[0] * ee)
            err_e = abs(got["ee"][0, 0, 0] - ee) / ee
            v, want = float(got["sdr"][0, 0]), lu(name)
            print(f"{name} form {form}: r {err_r:.2e} d {err_d:.2e} ee {err_e:.2e} order {got['order'][0, 0]} sdr {v!r} lu {want!r} "
                  f"|diff| {abs(v - want) if np.isfinite(want) else 0.0:.2e}")
            assert err_r <= 1e-12 and err_d <= 1e-12 and err_e <= 1e-12 and got["order"][0, 0] == 512
            if L == 1:
                assert want >= 120.0 and v >= 120.0
            else:
                assert abs(v - want) <= BAR
            if form == 0:
                assert got["sdr"].tobytes() == prod[0].tobytes() and got["perm"][0, 0] == prod[2][0, 0] == 0


def test_conditioning_by_sdr():
    cases = O.conditioning_cases()
    clean = np.stack([s for _, s, _ in cases])[:, None]
    est = np.stack([e for _, _, e in cases])[:, None]
    sdr = run(clean, est)[0]
    worst = 0.0
    for form in (64, 512):
        got = debug(clean, est, form=form)
        assert (got["order"] == 512).all(), got["order"]
        for b, (name, _, _) in enumerate(cases):
            err = abs(float(got["sdr"][b, 0]) - lu(name))
            worst = max(worst, err)
            print(f"{name} form {form}: device {got['sdr'][b, 0]!r} lu {lu(name)!r} |diff| {err:.2e}")
            assert err <= BAR
    assert debug(clean, est)["sdr"].tobytes() == sdr.tobytes()  # form 0 is the production solver
    print(f"conditioning x SDR: max |device - sdr_lu| = {worst:.2e} dB over {len(cases)} cases, two solver forms")


@pytest.mark.parametrize("n", [2, 3, 4])
def test_sources_shuffled_identical_and_with_mix(n):
    worst = 0.0
    for identical in (False, True):
        clean, est, mix, shuffle = O.source_case(n, identical)
        tag = f"src{n}{'i' if identical else ''}"
        M_ = [[lu(f"{tag}_e{i}_s{j}") for j in range(n)] for i in range(n)]
        want_perm = O.best_perm(M_)
        if not identical:
            assert want_perm == [shuffle.index(j) for j in range(n)] != list(range(n))
        else:
            assert want_perm.index(0) < want_perm.index(1)  # estimates 0 and 1 are copies: the first maximum
        sdr, sdr_i, perm = run(clean[None], est[None], mix[None])
        assert perm[0].tolist() == want_perm, (perm, want_perm)
        for j in range(n):
            want = M_[want_perm[j]][j]
            base = lu(f"{tag}_mix_s{j}")
            e1, e2 = abs(float(sdr[0, j]) - want), abs(float(sdr_i[0, j]) - (want - base))
            worst = max(worst, e1, e2)
            print(f"{tag} source {j}: sdr {sdr[0, j]!r} lu {want!r} |diff| {e1:.2e}; sdr_i {sdr_i[0, j]!r} |diff| {e2:.2e}")
            assert e1 <= BAR and e2 <= BAR
        alone = run(clean[None], est[None])  # without the mixture: the same sdr and perm
        assert alone[0].tobytes() == sdr.tobytes() and alone[2].tobytes() == perm.tobytes() and alone[1] is None
    print(f"n = {n}: max |device - sdr_lu| = {worst:.2e} dB")


def test_input_ranks_are_mirrored():
    from rtfs_net_amd.metrics import bss_sdr
    clean, est, mix, _ = O.source_case(2)
    full = run(clean[:, None], est[:, None], mix=np.stack([mix, mix]))
    c, e, m = _dev(clean), _dev(est), _dev(np.stack([mix, mix]))
    s2, i2, p2 = bss_sdr(c, e, m, return_perm=True)       # (B,L): n_src = 1
    assert s2.shape == i2.shape == p2.shape == (2,)
    assert _same(_host(s2, i2, p2), [v[:, 0] for v in full])
    s1 = bss_sdr(c[0], e[0])                                # (L,)
    assert s1.shape == () and _host(s1)[0].tobytes() == full[0][0, 0].tobytes()
    s1, i1 = bss_sdr(c[1], e[1], m[1])
    assert s1.shape == i1.shape == () and _host(i1)[0].tobytes() == full[1][1, 0].tobytes()


# ---------------------------------------------------------------- 2. bits
def _batch(B, n, L, seed):
    rng = np.random.default_rng(seed)
    clean = np.stack([[O.coloured(rng, L, O.REFERENCES[(b + j) % 5]) for j in range(n)] for b in range(B)])
    est = np.stack([[O.noisy(rng, clean[b, (j + b) % n], "white", 0.1 + 0.05 * j, "white") for j in range(n)] for b in range(B)])
    mix = (clean.sum(1) + 0.5 * rng.standard_normal((B, L))).astype(np.float32)  # n = 1: not the reference itself
    return clean, est, mix


def test_rows_do_not_depend_on_the_batch():
    clean, est, mix = _batch(5, 2, 8193, 70)
    full = run(clean, est, mix)
    for b in range(5):
        assert _same(run(clean[b:b + 1], est[b:b + 1], mix[b:b + 1]), [v[b:b + 1] for v in full]), b


@pytest.mark.parametrize("n", [1, 2])
def test_pooled_rows_are_block_rows(n):
    from rtfs_net_amd.metrics import bss_sdr_many
    recs = [_batch(1, n, L, 80 + L % 7) for L in (410, 4097, 8193, 32003)]
    cleans, ests, mixes = ([_dev(r[k][0]) for r in recs] for k in range(3))
    sdr, sdr_i, perm = _host(*bss_sdr_many(cleans, ests, mixes, return_perm=True))
    assert sdr.shape == sdr_i.shape == perm.shape == (4, n) and sdr.dtype == np.float32 and np.isfinite(sdr).all()
    for r, (c, e, m) in enumerate(recs):
        assert _same(run(c, e, m), [sdr[r:r + 1], sdr_i[r:r + 1], perm[r:r + 1]]), r
    rev = _host(*bss_sdr_many(cleans[::-1], ests[::-1], mixes[::-1], return_perm=True))
    assert _same([v[::-1] for v in rev], [sdr, sdr_i, perm])             # the pool's order changes nothing
    alone, perm_a = _host(*bss_sdr_many(cleans, ests, return_perm=True))  # without mixtures
    assert alone.tobytes() == sdr.tobytes() and perm_a.tobytes() == perm.tobytes()
    if n == 1:
        flat = _host(bss_sdr_many([c[0] for c in cleans], [e[0] for e in ests]))[0]  # (L_r) rows
        assert flat.tobytes() == sdr.tobytes()


def test_graph_capture_replays_eager():
    from rtfs_net_amd.metrics import bss_sdr
    clean, est, mix = _batch(3, 2, 4097, 90)
    cd, ed, md = _dev(clean), _dev(est), _dev(mix)
    eager = bss_sdr(cd, ed, md, return_perm=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        bss_sdr(cd, ed, md)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = bss_sdr(cd, ed, md, return_perm=True)
    cd.copy_(_dev(clean[::-1].copy()))  # new inputs in the captured buffers
    ed.copy_(_dev(est[::-1].copy()))
    md.copy_(_dev(mix[::-1].copy()))
    g.replay()
    torch.cuda.synchronize()
    for o, e in zip(out, eager):
        assert torch.equal(o, e.flip(0))


def test_degenerate_rows_inside_a_batch():
    clean, est, mix = _batch(6, 1, 4097, 100)
    clean[1] = 0                      # zero reference
    est[2] = 0                        # zero estimate
    clean[3] = 0
    est[3] = 0                        # both zero
    est[4] = clean[4]                 # estimate == reference
    sdr, sdr_i, perm = run(clean, est, mix)
    got = debug(clean, est, mix)
    print(f"degenerate rows: sdr {sdr[:, 0].tolist()} sdr_i {sdr_i[:, 0].tolist()} order {got['order'][:, 0].tolist()}")
    assert sdr[1, 0] == -np.inf and np.isnan(sdr[2, 0]) and np.isnan(sdr[3, 0])
    assert sdr[4, 0] == np.inf or sdr[4, 0] >= 120.0
    assert got["order"][:, 0].tolist() == [512, 0, 512, 0, 512, 512]  # a silent reference stops the recursion at order 0
    assert (perm == 0).all()
    for b in (0, 5):                  # the regular rows are their solo runs, bit for bit
        assert np.isfinite(sdr[b, 0]) and np.isfinite(sdr_i[b, 0])
        assert _same(run(clean[b:b + 1], est[b:b + 1], mix[b:b + 1]), [v[b:b + 1] for v in (sdr, sdr_i, perm)])


# ---------------------------------------------------------------- 3. poison, refusals
@pytest.mark.parametrize("byte", [0xFF, 0x7F], ids=["nan", "big"])
def test_poisoned_workspace_and_outputs(monkeypatch, byte):
    from rtfs_net_amd import _lib
    from rtfs_net_amd.metrics import bss_sdr_many
    blocks = [_batch(2, 2, 8193, 110), _batch(1, 3, 4097, 111), _batch(3, 1, 513, 112)]
    recs = [_batch(1, 2, L, 113 + i) for i, L in enumerate((410, 4097, 9000))]
    cleans, ests, mixes = ([_dev(r[k][0]) for r in recs] for k in range(3))

    def go():
        out = [run(c, e, m) for c, e, m in blocks] + [run(c, e) for c, e, _ in blocks]
        out.append(_host(*bss_sdr_many(cleans, ests, mixes, return_perm=True)))
        out.append(_host(*bss_sdr_many(cleans, ests, return_perm=True)))
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
    sdr, sdr_i = torch.zeros(2, 2, device=DEV), torch.zeros(2, 2, device=DEV)
    perm = torch.zeros(2, 2, device=DEV, dtype=torch.int32)
    nb = lib.rtfs_bss_sdr_workspace_bytes(2, 2, 5000, 1)
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    n0 = lib.rtfs_debug_launch_count()
    call = lambda c=x, e=x, mx=m, B=2, n=2, L=5000, w=ws, nbytes=nb, s=sdr, si=sdr_i, p=perm: lib.rtfs_bss_sdr_f32(  # noqa: E731
        P(c), P(e), P(mx), B, n, L, P(w), nbytes, P(s), P(si), P(p), st)
    assert call(c=None) == -4 and call(e=None) == -4 and call(w=None) == -4 and call(s=None) == -4 and call(si=None) == -4
    assert call(p=None) == -4 and call(B=0) == -4 and call(L=0) == -4 and call(n=0) == -4 and call(n=5) == -4
    assert call(nbytes=nb - 1) == -2
    plan = (ctypes.c_int * 33)()
    assert lib.rtfs_score_many_plan((ctypes.c_longlong * 2)(5000, 5000), 2, 2, 16000, plan, None) == 0
    own = lib.rtfs_bss_sdr_many_workspace_bytes(plan, 2, 1)
    rows = torch.tensor([x[0].data_ptr(), x[1].data_ptr()], dtype=torch.int64, device=DEV)
    mrows = torch.tensor([m[0].data_ptr(), m[1].data_ptr()], dtype=torch.int64, device=DEV)
    tab = torch.tensor(list(plan), dtype=torch.int32, device=DEV)
    wsm = torch.zeros(own, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    n0 = lib.rtfs_debug_launch_count()
    many = lambda fs=16000, n=2, R=2, nbytes=own, si=sdr_i: lib.rtfs_bss_sdr_many_f32(  # noqa: E731
        P(mrows), P(rows), P(rows), P(tab), plan, R, n, fs, P(wsm), nbytes, P(sdr), P(si), P(perm), st)
    assert many(fs=10000) == -4 and many(n=1) == -4 and many(R=3) == -4 and many(si=None) == -4 and many(nbytes=own - 1) == -2
    assert lib.rtfs_debug_launch_count() == n0
    assert many() == 0 and call() == 0   # three launches each; all-zero rows are 0 / 0
    torch.cuda.synchronize()
    assert lib.rtfs_debug_launch_count() == n0 + 6 and bool(torch.isnan(sdr).all())


# ---------------------------------------------------------------- 4. the tracker
def _tracker(tmp_path, name, feed, **kw):
    from rtfs_net_amd.metrics import ALLMetricsTracker
    t = ALLMetricsTracker(str(tmp_path / name), **kw)
    feed(t)
    mean, std = t.get_mean(), t.get_std()
    lists = (list(t.all_bss_sdrs), list(t.all_bss_sdrs_i)) if kw.get("bss_sdr") else None
    t.final()
    return list(csv.DictReader(open(tmp_path / name))), mean, std, lists


@functools.lru_cache(maxsize=None)
def _tracker_case():
    """(mix (B,L), clean (B,n,L), est (B,n,L)) speech-like, and the oracle's per-row means over the sources of sdr and sdr_i"""
    rng = np.random.default_rng(120)
    B, n, L = 3, 2, 8000
    clean = np.stack([[M.speech_like(rng, L, 16000) for _ in range(n)] for _ in range(B)])
    est = np.stack([[O.noisy(rng, clean[b, 1 - j], "white", 0.2 + 0.1 * j, "white") for j in range(n)] for b in range(B)])  # swapped
    mix = clean.sum(1).astype(np.float32)
    want = [O.bss_eval(clean[b], est[b], mix[b]) for b in range(B)]
    assert all(w[2] == [1, 0] for w in want)
    return mix, clean, est, [float(np.mean(w[0])) for w in want], [float(np.mean(w[1])) for w in want]


@pytest.mark.parametrize("estoi", [False, True])
def test_tracker_columns_by_every_entry(tmp_path, estoi):
    mix, clean, est, want, want_i = _tracker_case()
    md, cd, ed = _dev(mix), _dev(clean), _dev(est)
    keys = [f"k{b}" for b in range(len(mix))]
    kw = dict(estoi=estoi, bss_sdr=True)
    rows, mean, std, lists = _tracker(tmp_path, "batch.csv", lambda t: t.update_batch(md, cd, ed, keys), **kw)
    many = _tracker(tmp_path, "many.csv", lambda t: t.update_many(list(md), list(cd), list(ed), keys), **kw)
    call = _tracker(tmp_path, "call.csv", lambda t: [t(m, c, e, k) for m, c, e, k in zip(md, cd, ed, keys)], **kw)
    plain = _tracker(tmp_path, "plain.csv", lambda t: t.update_batch(md, cd, ed, keys), estoi=estoi)[0]
    names = ["snt_id", "sdr", "sdr_i", "si-snr", "si-snr_i", "pesq", "stoi"] + (["estoi"] if estoi else []) + ["bss_sdr", "bss_sdr_i"]
    assert list(rows[0]) == names and [r["snt_id"] for r in rows] == keys + ["avg", "std"]
    for other in (many, call):  # the three entries give the same text in the new columns (and in stoi); the same accumulators
        assert [[r[k] for k in names[6:]] for r in other[0]] == [[r[k] for k in names[6:]] for r in rows]
        assert other[3] == lists
    for a, b in zip(plain, rows):  # the columns the tracker had do not notice the two
        assert all(b[k] == v or (k == "pesq" and v == "nan") for k, v in a.items()), (a, b)
    worst = 0.0
    for b in range(len(keys)):
        e1, e2 = abs(float(rows[b]["bss_sdr"]) - want[b]), abs(float(rows[b]["bss_sdr_i"]) - want_i[b])
        worst = max(worst, e1, e2)
        assert e1 <= BAR and e2 <= BAR and float(rows[b]["bss_sdr"]) > 0, (b, rows[b], want[b], want_i[b])
        assert float(rows[b]["sdr"]) < 0 < float(rows[b]["bss_sdr"])  # the reference's sign quirk next to it: its sdr column is the loss
    got, got_i = lists
    assert got == [float(r["bss_sdr"]) for r in rows[:-2]] and got_i == [float(r["bss_sdr_i"]) for r in rows[:-2]]
    assert mean["bss_sdr"] == np.mean(got) and std["bss_sdr"] == np.std(got) and mean["bss_sdr_i"] == np.mean(got_i)
    assert float(rows[-2]["bss_sdr"]) == mean["bss_sdr"] and float(rows[-1]["bss_sdr"]) == std["bss_sdr"]
    assert float(rows[-2]["bss_sdr_i"]) == mean["bss_sdr_i"] and float(rows[-1]["bss_sdr_i"]) == std["bss_sdr_i"]
    print(f"tracker (estoi={estoi}): max |column - oracle| = {worst:.2e} dB; bss_sdr {got} bss_sdr_i {got_i}")
