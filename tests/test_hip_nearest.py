"""GPU: nearest up-sampling at the lengths where torch's float32 index rule - what the reference runs - is not floor(dst * n_in / n_out).

The rule (csrc/common.h nearest_src, oracle.rtfs_oracle.nearest_index; DESIGN.md "Nearest up-sampling"):
    src(dst) = min(int(floorf(dst * (float(n_in) / float(n_out)))), n_in - 1)
It departs from the integer quotient on 5 987 pairs with n_in <= 256, n_out <= 1030, among them (Tv, T) = (16, 82), (32, 164), (40, 205)
of the CAF and 16 -> 122 inside the VP block at Tv = 122.  Every committed fixture before these sat on an agreeing pair
(tests/test_nearest_host.py), so a kernel on the integer rule passed the suite and missed the reference by 0.1 ... 1 at these lengths.

Checked here: the device index tables bit for bit (against the numpy closed form and against F.interpolate on the device), then each
place that up-samples - CAF cell, whole forward (fused and per-kernel), separate_speakers, the VP block (fused long instance and
per-layer route), the TFAR kernels, and the training-side combine kernels with their adjoints - against the oracle and against vectors
captured from the reference (oracle/make_golden_nearest.py).  Module and forward cases run on poisoned scratch and outputs, once per
pattern (0xFF: NaN, 0x7F: 3.4e38); a run that RTFS_POISON_WS already poisons keeps its own pattern."""
import copy
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import rtfs_oracle as O
from oracle.params import make_inputs
from oracle.rtfs_oracle import nearest_index
from tests import nearest_cases as NC
from tests.test_hip_long_separator import VBLK, launches, model  # (that file's instances: a whole forward leaves a side stream on the model)
from tests.test_hip_parity import BLK, CELL, TOL, close, dev, host
from tests.util import check_probe, frame_rel_err, l2_rel, load_golden, rand, rel_err

pytestmark = pytest.mark.gpu

BATCH_BAR = 2e-6  # a mixture in a batch vs its own run (tests/test_hip_parity.py, tests/test_hip_speakers.py)
_CACHE = {}


@pytest.fixture(params=[0xFF, 0x7F], ids=["nan", "big"])
def poison(request, monkeypatch):
    from rtfs_net_amd import _lib
    if _lib._POISON is None:
        monkeypatch.setattr(_lib, "_POISON", request.param)
    return _lib._POISON


def cached(key, fn):
    """A CPU reference computed once, shared between tests and poison patterns, never written to."""
    if key not in _CACHE:
        ref = fn()
        ref.setflags(write=False)
        _CACHE[key] = ref
    return _CACHE[key]


def time_frame_err(got, ref):
    """tests.util.frame_rel_err per TIME frame of a (B, C, T, F) tensor: C and F folded together."""
    B, C, T, Fq = ref.shape
    fold = lambda x: np.asarray(x).transpose(0, 1, 3, 2).reshape(B, C * Fq, T)
    return frame_rel_err(fold(got), fold(ref))


# ---------------------------------------------------------------- 1. the index tables
def test_device_index_tables_bit_equal():
    """nearest_src(dst) for every dst and nearest_first_dst(j) for every source j <= n_in, for every departing pair and the stride sample,
    in one launch (rtfs_selftest_nearest_index): bit-equal to the numpy closed form, and - the departing pairs - to F.interpolate on a
    float32 tensor on the device."""
    from rtfs_net_amd import _lib
    lib = _lib.load()
    dep = list(NC.departing_pairs())
    assert len(dep) == 5987 and (16, 82) in dep and (16, 122) in dep
    pairs = dep + [p for p in NC.stride_sample() if p not in set(dep)] + [p for p in NC.used_pairs() if p not in set(dep)]
    pa = np.array(pairs, np.int32)
    off = np.zeros((len(pairs), 2), np.int64)
    off[1:, 0] = np.cumsum(pa[:-1, 1])          # n_out entries of out_src per pair
    off[1:, 1] = np.cumsum(pa[:-1, 0] + 1)      # n_in + 1 entries of out_first_dst per pair
    n_src, n_first = int(pa[:, 1].sum()), int((pa[:, 0] + 1).sum())
    assert n_src < 2 ** 31
    d_pairs, d_off = dev(pa.reshape(-1)), dev(off.astype(np.int32).reshape(-1))
    out_src = torch.full((n_src,), -1, dtype=torch.int32, device="cuda")
    out_first = torch.full((n_first,), -1, dtype=torch.int32, device="cuda")
    _lib.check(lib.rtfs_selftest_nearest_index(_lib.ptr(d_pairs), len(pairs), _lib.ptr(d_off), _lib.ptr(out_src), _lib.ptr(out_first),
                                               _lib.stream_of(out_src)), "rtfs_selftest_nearest_index")
    got_src, got_first = host(out_src), host(out_first)
    want_src = np.concatenate([nearest_index(i, o) for i, o in pairs]).astype(np.int32)
    # first destination whose source is >= j: the closed form's table is non-decreasing, so a binary search states it
    want_first = np.concatenate([np.searchsorted(nearest_index(i, o), np.arange(i + 1), side="left") for i, o in pairs]).astype(np.int32)
    bad = np.flatnonzero(got_src != want_src)
    assert bad.size == 0, f"nearest_src differs from the closed form at {bad.size} entries, first in pair {pairs[int(np.searchsorted(off[:, 0], bad[0], 'right')) - 1]}"
    bad = np.flatnonzero(got_first != want_first)
    assert bad.size == 0, f"nearest_first_dst differs at {bad.size} entries, first in pair {pairs[int(np.searchsorted(off[:, 1], bad[0], 'right')) - 1]}"
    # the pre-images [first(j), first(j + 1)) tile [0, n_out) for every pair
    assert np.array_equal(got_first[off[:, 1]], np.zeros(len(pairs), np.int32))
    assert np.array_equal(got_first[off[:, 1] + pa[:, 0]], pa[:, 1])
    # stock torch on the device, float32: mismatches counted on the device, one read-back
    ramp = torch.arange(int(pa[:, 0].max()), dtype=torch.float32, device="cuda").view(1, 1, -1)
    wrong = torch.zeros((), dtype=torch.int64, device="cuda")
    for k, (i, o) in enumerate(dep):
        idx = F.interpolate(ramp[:, :, :i], size=o, mode="nearest").view(-1).to(torch.int32)
        wrong += (idx != out_src[int(off[k, 0]):int(off[k, 0]) + o]).sum()
    assert int(wrong) == 0, f"{int(wrong)} entries differ from F.interpolate(mode='nearest') on a float32 CUDA tensor"


def test_selftest_entry_rejects_bad_arguments():
    from rtfs_net_amd import _lib
    lib = _lib.load()
    z = torch.zeros(8, dtype=torch.int32, device="cuda")
    assert lib.rtfs_selftest_nearest_index(None, 1, _lib.ptr(z), _lib.ptr(z), _lib.ptr(z), _lib.stream_of(z)) != 0
    assert lib.rtfs_selftest_nearest_index(_lib.ptr(z), 0, _lib.ptr(z), _lib.ptr(z), _lib.ptr(z), _lib.stream_of(z)) != 0


# ---------------------------------------------------------------- 2. CAF cell, inference
# (2, 163, 129, 32): the agreeing neighbour of (32, 164); (1, 205, 129, 40): three departing frames, no reference vector (oracle only)
CAF_CASES = [(2, 82, 129, 16, 201, "mod_caf_T82_Tv16", (41,)), (2, 164, 129, 32, 203, "mod_caf_T164_Tv32", (41, 82)),
             (1, 205, 129, 40, 207, None, (41, 82, 164)), (2, 163, 129, 32, 209, None, ())]


@pytest.mark.parametrize("B,T,Fq,Tv,seed,golden,frames", CAF_CASES, ids=[f"T{c[1]}_Tv{c[3]}" for c in CAF_CASES])
def test_caf_module(B, T, Fq, Tv, seed, golden, frames, poison):
    assert NC.departs(Tv, T) == bool(frames)
    a, v = rand((B, 256, T, Fq), seed), rand((B, 512, Tv), seed + 1)
    ref = cached(("caf", B, T, Fq, Tv, seed), lambda: O.caf(a, v, CELL))
    with torch.no_grad():
        y, _ = model().refinement_module.crossmodal_fusion.fusion_module(dev(a), dev(v))
    y = host(y)
    close(f"caf T={T} Tv={Tv} poison {poison:#x}", y, ref)
    fe = time_frame_err(y, ref)
    print(f"[nearest] caf T={T} Tv={Tv}: worst time frame {fe:.3e}")
    assert fe <= TOL, f"caf T={T} Tv={Tv}: worst time frame {fe:.3e}"
    if golden:
        g = load_golden(golden)
        check_probe(g, "out", y, TOL)
        for fr in frames:
            want = g[f"out.frame{fr}"] if f"out.frame{fr}" in g else load_golden(f"{golden}_frame{fr}")[f"out.frame{fr}"]
            close(f"caf T={T} frame {fr} vs reference", y[:, :, fr], want)


# ---------------------------------------------------------------- 3. whole forward at L = 20900: (Tv, T) = (32, 164)
L_DEP, TV_DEP, SEED_DEP = 20900, 32, 41


@pytest.mark.parametrize("fused", [True, False])
def test_forward_vs_reference_golden(fused, poison):
    """The fused separator (k_pws / k_b2b gather the CAF's video frames themselves) and the per-kernel path (k_caf) against the
    reference's output; the bars of test_end_to_end_vs_golden."""
    m = model(4)
    m.fused = fused
    wav, emb = make_inputs(1, L_DEP, TV_DEP, SEED_DEP)
    try:
        with torch.no_grad():
            out = host(m(dev(wav), dev(emb)))
    finally:
        m.fused = True
    close(f"e2e_R4_L20900_B1 fused={fused} poison {poison:#x}", out, load_golden("e2e_R4_L20900_B1")["out"])


def test_forward_row_of_a_batch_equals_its_own_run(poison):
    m = model(4)
    wav, emb = make_inputs(1, L_DEP, TV_DEP, SEED_DEP)
    w2, e2 = make_inputs(2, L_DEP, TV_DEP, SEED_DEP + 1000)
    wb, eb = np.concatenate([w2[:1], wav, w2[1:]]), np.concatenate([e2[:1], emb, e2[1:]])
    with torch.no_grad():
        full = host(m(dev(wb), dev(eb)))
        one = host(m(dev(wav), dev(emb)))
    assert full.shape == (3, 1, L_DEP) and np.isfinite(full).all()
    close("e2e_R4_L20900 as row 1 of B = 3 vs reference", full[1:2], load_golden("e2e_R4_L20900_B1")["out"])
    e = rel_err(full[1:2], one)
    print(f"[nearest] L=20900 row 1 of B=3 vs its own run: {e:.3e}")
    assert e <= BATCH_BAR, e


def test_separate_speakers_equals_forward_on_the_replicated_batch(poison):
    from tests.test_hip_speakers import model as speakers_model
    m = speakers_model(4)  # that file's instance: separate_speakers leaves a side stream on the model, and other files deepcopy model()
    K = 2
    wav, emb = make_inputs(1, L_DEP, TV_DEP, SEED_DEP)
    lips = np.concatenate([emb[:, None], np.random.RandomState(SEED_DEP + 2).randn(1, 1, 512, TV_DEP).astype(np.float32)], axis=1)
    w, e = dev(wav), dev(lips)
    with torch.no_grad():
        got = host(m.separate_speakers(w, e))
        ref = host(m(w.repeat_interleave(K, 0), e.reshape(K, 512, TV_DEP)))
    assert got.shape == (1, K, L_DEP) and np.isfinite(got).all()
    worst = max(rel_err(got[0, k], ref[k, 0]) for k in range(K))
    print(f"[nearest] separate_speakers L=20900 K=2: worst per-target max-rel {worst:.3e} vs forward")
    assert worst <= BATCH_BAR, worst
    close("separate_speakers L=20900 speaker 0 vs reference", got[:, :1], load_golden("e2e_R4_L20900_B1")["out"])


# ---------------------------------------------------------------- 4. VP block
def vp_close(name, got, ref):
    close(name, got, ref)
    fe = frame_rel_err(got, ref)
    print(f"[nearest] {name}: worst frame {fe:.3e}")
    assert fe <= TOL, f"{name}: worst frame {fe:.3e}"


@pytest.mark.parametrize("tv,seed", [(122, 205), (121, 211), (123, 213)])
def test_vp_block_fused_long_instance(tv, seed, poison):
    """Tv = 122: pyramid 122 / 61 / 31 / 16, whose 16 -> 122 up-sampling departs; one launch of the fused kernel.  121 and 123: controls."""
    assert any(NC.departs(*p) for p in NC.vp_pairs(tv)) == (tv == 122)
    v = rand((2, 512, tv), seed)
    ref = cached(("vp", tv, seed), lambda: O.vp_block(v, VBLK))
    vd = dev(v)
    y, n = launches(lambda: model().refinement_module.video_net.blocks(vd))
    y = host(y)
    assert n == 1, f"Tv={tv}: {n} launches (fused VP block: 1)"
    vp_close(f"vp block Tv={tv} poison {poison:#x}", y, ref)
    if tv == 122:
        g = load_golden("mod_vp122")
        check_probe(g, "out", y, TOL)
        whole = np.stack([g[f"out.frame{fr}"] for fr in range(59, 64)], axis=2)
        vp_close("vp block Tv=122 frames 59..63 vs reference", y[:, :, 59:64], whole)


def test_vp_block_per_layer_route_284(poison):
    """Past 256 frames the block runs layer by layer; 284 / 142 / 71 / 36: its 36 -> 284 up-sampling departs."""
    assert [p for p in NC.vp_pairs(284) if NC.departs(*p)] == [(36, 284)]
    v = rand((2, 512, 284), 215)
    ref = cached(("vp", 284, 215), lambda: O.vp_block(v, VBLK))
    vd = dev(v)
    y, n = launches(lambda: model().refinement_module.video_net.blocks(vd))
    assert n > 1, n
    vp_close(f"vp block Tv=284 (per-layer) poison {poison:#x}", host(y), ref)


# ---------------------------------------------------------------- 5. TFAR: the model never meets a departing pair here (T // 2 -> T and
# 64 -> 129 agree), the kernels accept one: (14, 26) -> (46, 44), the two smallest departing pairs
def test_tfar_module_at_a_departing_pair(poison):
    assert NC.departs(14, 46) and NC.departs(26, 44)
    loc, glo = rand((2, 64, 46, 44), 221), rand((2, 64, 14, 26), 222)
    ref = cached(("tfar", 221), lambda: O.injection_multi_sum(loc, glo, O._sub(BLK, "fusion_layers.0")))
    with torch.no_grad():
        y = host(model().refinement_module.audio_net.blocks.fusion_layers[0](dev(loc), dev(glo)))
    close(f"tfar (14, 26) -> (46, 44) poison {poison:#x}", y, ref)
    fe = time_frame_err(y, ref)
    assert fe <= TOL, f"tfar (14, 26) -> (46, 44): worst time frame {fe:.3e}"


def gather_up(x, size, axes):
    """Up-sampling as an explicit gather through the closed-form indices (float64 torch, differentiable)."""
    for ax, n_out in zip(axes, size):
        x = x.index_select(ax, torch.from_numpy(nearest_index(x.shape[ax], n_out)))
    return x


@pytest.mark.parametrize("rows,C", [(False, 3), (True, 3), (True, 8)], ids=["planes", "rows_c3", "rows_c8"])
def test_tfar_combine_and_adjoint_at_a_departing_pair(rows, C):
    """rtfs_tfar_combine_f32 / rtfs_tfar_combine_backward_f32 at (Hg, Wg) -> (H, W) = (14, 26) -> (46, 44) against autograd over an explicit
    gather; channel-first planes and (B, H, W, C) rows with the scalar (C = 3) and the 4-wide (C = 8) kernels.  Bars of
    test_pool_and_tfar_combine_adjoints."""
    import rtfs_net_amd as R
    H, W, Hg, Wg = 46, 44, 14, 26
    hi, lo = ((2, H, W, C), (2, Hg, Wg, C)) if rows else ((2, C, H, W), (2, C, Hg, Wg))
    axes = (1, 2) if rows else (2, 3)
    le, ga, ge, do = rand(hi, 231), rand(lo, 232), rand(lo, 233), rand(hi, 234)
    ts = [dev(a).requires_grad_(True) for a in (le, ga, ge)]
    o = R.layers._TfarCombineFn.apply(*ts, rows)
    o.backward(dev(do))
    rs = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (le, ga, ge)]
    orf = rs[0] * gather_up(rs[1], (H, W), axes) + gather_up(rs[2], (H, W), axes)
    orf.backward(torch.tensor(do, dtype=torch.float64))
    close("tfar combine (14, 26) -> (46, 44)", host(o), orf.detach().numpy(), tol=1e-6)
    for t, r, nm in zip(ts, rs, ("dlocal", "dgate", "dglobal")):
        close(f"tfar combine {nm}", host(t.grad), r.grad.numpy(), tol=2e-6)


# ---------------------------------------------------------------- 6. training side
@pytest.mark.parametrize("rows,B,C,T,Fq,Tv", [(False, 1, 3, 82, 5, 16), (False, 2, 4, 164, 7, 32), (True, 1, 4, 82, 5, 16), (True, 2, 64, 164, 3, 32),
                                              (True, 1, 8, 205, 2, 40)])
def test_caf_combine_and_adjoints(rows, B, C, T, Fq, Tv):
    """rtfs_caf_combine_f32 / rtfs_caf_combine_rows_f32 and their backwards: key * up(resized) + up(att) * value against autograd over an
    explicit gather.  One rounding per product and a sum of up to ~6 F (planes) or 6 (rows: atomics over F-partials) terms per video
    frame: 1e-6 forward, 2e-6 on the gradients, as the TFAR combine."""
    import rtfs_net_amd as R
    assert NC.departs(Tv, T)
    shape = (B, T, Fq, C) if rows else (B, C, T, Fq)
    key, val, do = rand(shape, 241), rand(shape, 242), rand(shape, 243)
    res, att = rand((B, C, Tv), 244), rand((B, C, Tv), 245)
    ts = [dev(a).requires_grad_(True) for a in (key, val, res, att)]
    o = R.layers._CafCombineFn.apply(*ts, rows)
    o.backward(dev(do))
    rs = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (key, val, res, att)]
    up = lambda x: gather_up(x, (T,), (2,))  # (B, C, T)
    shaped = (lambda x: up(x).permute(0, 2, 1).unsqueeze(2)) if rows else (lambda x: up(x).unsqueeze(-1))
    orf = rs[0] * shaped(rs[2]) + shaped(rs[3]) * rs[1]
    orf.backward(torch.tensor(do, dtype=torch.float64))
    close(f"caf combine rows={rows} T={T} Tv={Tv}", host(o), orf.detach().numpy(), tol=1e-6)
    for t, r, nm in zip(ts, rs, ("dkey", "dvalue", "dresized", "datt")):
        close(f"caf combine {nm}", host(t.grad), r.grad.numpy(), tol=2e-6)


@pytest.mark.parametrize("B,T,Fq,Tv,seed", [(1, 82, 5, 16, 251), (2, 164, 16, 32, 252)])
def test_caf_cell_training(B, T, Fq, Tv, seed):
    """test_caf_training_forward_backward's harness and bars at departing (Tv, T)."""
    import tests.test_hip_training as TR
    TR.test_caf_training_forward_backward(B, T, Fq, Tv, seed, False)


def test_vp_block_training_122():
    """test_vp_block_training_forward_backward's harness and bars at Tv = 122 (the training route up-samples with torch on the device)."""
    import tests.test_hip_training as TR
    TR.test_vp_block_training_forward_backward(2, 122, False, 261)


def test_training_step_vs_reference_gradients():
    """One training step at L = 10400, (Tv, T) = (16, 82), R = 2, B = 1, BatchNorm frozen, against gradients the reference produced
    (tests/golden/grad_R2_L10400_B1.npz, oracle/make_golden_nearest.py; tensors over 1024 elements as 1024 samples).  Bars of
    test_training_gradients_vs_reference_golden."""
    import rtfs_net_amd as R
    from tests.test_hip_parity import model as pristine_model  # the training files' instances: only ever deep-copied, never run
    gold = load_golden("grad_R2_L10400_B1")
    m = copy.deepcopy(pristine_model(2)).train()
    ga = m.refinement_module.video_net.get_block(0).globalatt[0]
    ga.MHSA.dropout, ga.MHSA.dropout_layer.p, ga.FFN.dropout = 0.0, 0.0, 0.0
    for mod_ in m.modules():
        if isinstance(mod_, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
            mod_.eval()
    B, L, Tv = 1, 10400, 16
    wav, emb = make_inputs(B, L, Tv, seed=42)
    tgt = (0.05 * np.random.default_rng(43).standard_normal((B, 1, L))).astype(np.float32)
    out = m(dev(wav), dev(emb))
    loss = R.losses.PITLossWrapper(R.losses.PairwiseNegSDR("snr"), pit_from="pw_mtx")(out, dev(tgt))
    loss.backward()
    close("hip vs reference separated waveform, L=10400", host(out), gold["eval/est"], tol_l2=3e-5)  # training-side bf16x3 GEMMs
    assert abs(float(loss) - float(gold["eval/loss"])) <= 1e-5 * abs(float(gold["eval/loss"]))
    errs = {}
    gscale = max(np.abs(gold[f"eval/{k}"]).max() for k, _ in m.named_parameters())
    for k, p_ in m.named_parameters():
        g = host(p_.grad).reshape(-1).astype(np.float64)
        ref = gold[f"eval/{k}"]
        if g.size > 1024:
            rs = np.random.RandomState(zlib.crc32(k.encode()) & 0x7FFFFFFF)
            g = g[rs.choice(g.size, 1024, replace=False).astype(np.int64)]
        if np.abs(ref).max() > 1e-6 * gscale:
            errs[k] = l2_rel(g, ref)
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:3]
    print(f"[nearest] hip vs reference gradients at (Tv, T) = (16, 82), {len(errs)} tensors: median l2-rel {np.median(list(errs.values())):.3e}, worst {worst}")
    assert np.median(list(errs.values())) <= 5e-3
    assert np.mean([v <= 2e-2 for v in errs.values()]) >= 0.9, worst
