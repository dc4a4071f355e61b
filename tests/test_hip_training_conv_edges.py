"""Boundary sweeps of csrc/k_train_conv.hip, the training kernels tests/test_hip_training_edges.py does not touch: the depthwise
forward / input-gradient / weight-gradient kernels over every route of launch_cl_dw_chunk (stride, W >= 4, 4 | C, kw <= 4, 256-channel
slices), their two folds and grid caps, the bias column sums, the ConvNormAct stage kernels (forward, backward reduction,
cl_stage_reduce2_kernel, apply) at their fold switch and 256-workgroup cap, the block gateway, and the pool / TFAR / CAF glue called by
name through the C ABI, plus the refusals include/rtfs_amd.h documents.

Two techniques.  Exact integers: a depthwise convolution without norm and activation on x, w in {-2..2}, dout, bias in {-1, 0, 1} sums
at most B.H.W terms of magnitude <= 4 (33,000 at the largest case here), far below 2^24, so every float32 sum is exact in any order and
out, dx, dW and dbias must EQUAL an int64 reference: one dropped, doubled or misplaced row behind a grid cap or a fold cannot hide
below a relative bar.  Kinks: where a case has a ReLU / PReLU, the float64 reference evaluates it on the kernel's own sign pattern
(pre-activation: the saved rows; post-activation: the forward output, PReLU slopes kept positive), as mhsa2d_training_case does, so no
element is left out of any comparison.

Bars are those of the existing tests of the same kernels: forward close() default, every gradient 2e-4 (test_conv_norm_act_training_
forward_backward, test_caf_training_forward_backward), gateway 1e-6 / 1e-5 (test_gateway_one_pass_forward_backward), pool / combine glue
1e-6 / 2e-6 (test_pool_and_tfar_combine_adjoints)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.test_hip_parity import close, dev, host
from tests.test_hip_training_edges import ERR_SHAPE, ERR_WORKSPACE, _nan
from tests.util import rand, rel_err

pytestmark = pytest.mark.gpu

WORST = {}  # section -> worst max-rel error seen (printed when the module is done; DESIGN.md quotes it)
GUARD = 4096  # floats behind every output of a by-name call


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for k in sorted(WORST):
        print(f"[worst] {k}: max-rel {WORST[k]:.3e}")


def _chk(section, name, got, ref, tol=None):
    WORST[section] = max(WORST.get(section, 0.0), rel_err(got, ref))
    if tol is None:
        close(name, got, ref)
    else:
        close(name, got, ref, tol=tol)


def _same(name, got, ref):
    """Exact-integer comparison: every element of ``got`` equals the int64 reference."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, f"{name}: shape {got.shape} != {ref.shape}"
    assert ref.dtype == np.int64 and int(np.abs(ref).max(initial=0)) < 2 ** 24
    bad = got.astype(np.float64) != ref
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.size} elements differ from the integer reference, first at {i}: "
                             f"got {got[i]!r}, want {int(ref[i])}")


def _guarded(*shape):
    """An output of ``shape`` that starts as NaN, followed by GUARD floats of a known pattern."""
    n = int(np.prod(shape))
    t = torch.empty(n + GUARD, dtype=torch.float32, device="cuda")
    t[:n] = float("nan")
    t[n:] = torch.arange(GUARD, dtype=torch.float32, device="cuda") + 0.5
    return t


def _unguard(t, shape, name):
    h, n = host(t), int(np.prod(shape))
    want = np.arange(GUARD, dtype=np.float32) + 0.5
    assert np.array_equal(h[n:].view(np.uint32), want.view(np.uint32)), f"{name}: written past its end"
    return h[:n].reshape(shape)


def _lib():
    from rtfs_net_amd import _lib as L
    return L.load(), L


# ------------------------------------------------------------------------------------------------ depthwise convolution: reference and case
def _dw_ref(x, w, b, dout, k, stride):
    """Depthwise cross-correlation of ConvNormAct and its three adjoints as shifted-slice sums, in the dtype of the inputs (int64 or
    float64): x (B, C, H, W) or (B, C, L), w (C, 1, kh, kw) or (C, 1, k).  Stride 1: "same" with the smaller half of the padding first;
    stride 2: (k - 1) // 2 on every side."""
    is2d = x.ndim == 4
    if not is2d:
        x, dout = x[:, :, None, :], dout[:, :, None, :]
    kh = k if is2d else 1
    w = w.reshape(w.shape[0], kh, k)
    B, C, H, W = x.shape
    p = (k - 1) // 2
    pt = p if is2d else 0
    if stride == 1:
        Ho, Wo, pb, pr = H, W, kh - 1 - pt, k - 1 - p
    else:
        Ho, Wo, pb, pr = (H + 2 * pt - kh) // stride + 1, (W + 2 * p - k) // stride + 1, pt, p
    assert dout.shape == (B, C, Ho, Wo), (dout.shape, (B, C, Ho, Wo))
    xp = np.zeros((B, C, H + pt + pb, W + p + pr), x.dtype)
    xp[:, :, pt:pt + H, p:p + W] = x
    out = np.zeros((B, C, Ho, Wo), x.dtype)
    dxp, dw = np.zeros_like(xp), np.zeros_like(w)
    for ki in range(kh):
        for kj in range(k):
            sl = (slice(None), slice(None), slice(ki, ki + (Ho - 1) * stride + 1, stride), slice(kj, kj + (Wo - 1) * stride + 1, stride))
            wc = w[None, :, ki, kj, None, None]
            out += wc * xp[sl]
            dxp[sl] += wc * dout
            dw[:, ki, kj] = (dout * xp[sl]).sum((0, 2, 3))
    if b is not None:
        out += b[None, :, None, None]
    dx = dxp[:, :, pt:pt + H, p:p + W]
    if not is2d:
        out, dx = out[:, :, 0], dx[:, :, 0]
    return out, dx, dw, dout.sum((0, 2, 3))


def _dw_out_shape(shape, k, stride):
    if stride == 1:
        return tuple(shape)
    p = (k - 1) // 2
    return tuple(shape[:2]) + tuple((n + 2 * p - k) // stride + 1 for n in shape[2:])


def _dw_case(section, shape, k, stride, integer, seed, bias=True, check_torch=False):
    """ConvNormAct(C, C, k, groups = C) without norm and activation through the training kernels: forward, dx, dW and dbias.
    integer: the exact-integer inputs (see the module docstring) against the int64 reference, compared for equality; else standard normal
    inputs against float64 at the bars of test_conv_norm_act_training_forward_backward.  Returns "refused" where the configuration is
    one ConvNormAct must refuse (stride 2 on a padded map smaller than the window), after asserting that it does."""
    import rtfs_net_amd as R
    is2d, C = len(shape) == 4, shape[1]
    rng = np.random.default_rng(seed)
    if integer:
        draw = lambda lo, hi, s: rng.integers(lo, hi + 1, s)
    else:
        draw = lambda lo, hi, s: rng.standard_normal(s).astype(np.float32).astype(np.float64)
    mod = R.layers.ConvNormAct(C, C, k, stride=stride, groups=C, bias=bias, is2d=is2d)
    conv = mod.full_layer[2]
    w, b, x = draw(-2, 2, tuple(conv.weight.shape)), (draw(-1, 1, (C,)) if bias else None), draw(-2, 2, tuple(shape))
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(w.astype(np.float32)))
        if bias:
            conv.bias.copy_(torch.from_numpy(b.astype(np.float32)))
    mod = mod.cuda().train()
    xt = dev(x.astype(np.float32)).requires_grad_(True)
    p = (k - 1) // 2
    if stride > 1 and any(n + 2 * p < k for n in shape[2:]):
        with pytest.raises(RuntimeError, match="bad shape"):
            mod(xt)
        return "refused"
    out = mod(xt)
    oshape = _dw_out_shape(shape, k, stride)
    assert tuple(out.shape) == oshape, (tuple(out.shape), oshape)
    dout = draw(-1, 1, oshape)
    out.backward(dev(dout.astype(np.float32)))
    refs = _dw_ref(x, w, b, dout, k, stride)
    if check_torch:  # the shifted-slice reference itself against F.conv under autograd
        xr, wr = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (x, w)]
        br = torch.tensor(b, dtype=torch.float64, requires_grad=True) if bias else None
        yr = (F.conv2d if is2d else F.conv1d)(xr, wr, br, stride=stride, padding=p if stride > 1 else "same", groups=C)
        yr.backward(torch.tensor(dout, dtype=torch.float64))
        for mine, theirs in zip(refs, (yr.detach(), xr.grad, wr.grad) + ((br.grad,) if bias else ())):
            assert np.allclose(np.asarray(mine, np.float64).reshape(theirs.shape), theirs.numpy(), rtol=1e-12, atol=1e-12)
    got = [out, xt.grad, conv.weight.grad] + ([conv.bias.grad] if bias else [])
    tag = f"dw {tuple(shape)} k{k} s{stride}"
    for nm, g, r in zip(("out", "dx", "dW", "dbias"), got, refs):
        g = host(g).reshape(r.shape)
        if integer:
            _same(f"{tag} {nm}", g, r)
        else:
            _chk(section, f"{tag} {nm}", g, r, None if nm == "out" else 2e-4)
    return "ran"


# ------------------------------------------------------------------------------------------------ 1. depthwise routing at small sizes
S1 = "1 depthwise routing"
VARIANTS = pytest.mark.parametrize("integer", [False, True], ids=["float", "exact"])


@VARIANTS
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_depthwise_2d_routing_small(k, stride, integer):
    """Every route of launch_cl_dw_chunk on 2-D maps: H in {1, 2, 3, 5}, W in 1..9, C in {2, 4, 64}, B = 2.  Stride 2 or W < 4:
    cl_dw_fwd_kernel, cl_dw_bwd_data_kernel and the per-pixel weight gradients (cl_dw_wgrad_kernel at C = 2, _c4 otherwise); stride 1 and
    W >= 4: cl_dw_s1_w4_kernel<false / true> at C = 2, cl_dw_s1_w4c4_kernel<false / true> and cl_dw_wgrad_w4c4_kernel at 4 | C, over
    every W % 4, windows taller or wider than the map, and the mirrored padding of the flipped kernel at even k.  C = 2 folds with
    cl_dw_wgrad_reduce1_kernel at 1 and 9 taps, cl_dw_wgrad_reduce_kernel otherwise; dbias comes from cl_colsum_any_kernel (C = 2) or
    cl_colsum_kernel.  Stride 2 with an even k on a map of height or width 1 (padded size k - 1) is refused, as nn.Conv refuses it."""
    refused = 0
    for C in (2, 4, 64):
        for H in (1, 2, 3, 5):
            for W in range(1, 10):
                r = _dw_case(S1, (2, C, H, W), k, stride, integer, 100000 * k + 10000 * stride + 100 * C + 10 * H + W, check_torch=True)
                refused += r == "refused"
    assert refused == (36 if stride == 2 and k % 2 == 0 else 0)  # per C: H = 1 (9 widths) and W = 1 at the other three heights


@VARIANTS
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_depthwise_1d_routing_small(k, integer):
    """The same on sequences (is2d = False): L in 1..9, C in {2, 128}, both strides; k = 5 is the kw > 4 route to the dword kernels at
    C = 128 too, and C = 2 with 3 / 5 taps the third and fourth way into cl_dw_wgrad_reduce1_kernel."""
    refused = 0
    for stride in (1, 2):
        for C in (2, 128):
            for L in range(1, 10):
                r = _dw_case(S1, (2, C, L), k, stride, integer, 200000 * k + 10000 * stride + 10 * C + L, check_torch=True)
                refused += r == "refused"
    assert refused == (2 if k in (2, 4) else 0)  # stride 2, L = 1, both channel counts


# ------------------------------------------------------------------------------------------------ 2. depthwise at the grid edges (exact)
@pytest.mark.parametrize("shape,k,stride", [((2, 512, 6, 7), 4, 1), ((2, 512, 6, 7), 4, 2), ((2, 1024, 6, 7), 3, 1), ((2, 1024, 6, 7), 3, 2),
                                            ((2, 512, 23), 5, 1), ((2, 512, 23), 5, 2)])
def test_depthwise_wide_slices_exact(shape, k, stride):
    """C > 256 runs as 256-channel slices with a pitch, with more than one tap: weights, bias, dW and dbias of every slice.  kh.kw.C is
    8192 / 9216 for the 2-D cases: above the 5120 floats per workgroup rtfs_cna_workspace_bytes budgets for the weight-gradient scratch,
    which rtfs_cna_backward_f32 used to take for all C channels at once (RTFS_ERR_WORKSPACE on the buffer its own query sized)."""
    assert _dw_case("2", shape, k, stride, True, 31 * shape[1] + 7 * k + stride) == "ran"


@pytest.mark.parametrize("H", [122, 123, 129])
def test_depthwise_wgrad_w4c4_rebalanced_grid_exact(H):
    """cl_dw_wgrad_w4c4_kernel re-balances its grid once ceil(B.Ho.ceil(Wo / 4) / (1024 / C)) passes 768 resident workgroups: at
    (1, 256, H, 100), k = 4 that count is 763 (H = 122: one round, 768 workgroups), 769 (H = 123: two rounds of 385 -> 392) and 807
    (H = 129: 404 -> 408)."""
    assert _dw_case("2", (1, 256, H, 100), 4, 1, True, 500 + H) == "ran"


@pytest.mark.parametrize("shape,k", [((1, 128, 1920), 5), ((1, 128, 2048), 5), ((1, 256, 1280, 3), 4), ((1, 256, 1355, 3), 4),
                                     ((1, 256, 20, 96), 4), ((1, 256, 16, 128), 4)])
def test_depthwise_wgrad_fold_switch_exact(shape, k):
    """cl_dw_wgrad_reduce_kernel takes ceil(g / 4) row slices below g = 128 partial rows and 32 from there on: g = 120 and 128 behind
    each first stage - cl_dw_wgrad_kernel (k = 5: 16 rows per workgroup), cl_dw_wgrad_c4_kernel (W = 3: 32 rows per workgroup) and
    cl_dw_wgrad_w4c4_kernel (4 column quads per workgroup)."""
    assert _dw_case("2", shape, k, 1, True, sum(shape) + k) == "ran"


@pytest.mark.parametrize("L", [32768, 33000])
def test_depthwise_wgrad_grid_cap_exact(L):
    """CL_DW_WGRAD_MAX_WG = 2048 on cl_dw_wgrad_kernel (C = 128, k = 5: two row lanes, 16 rows per workgroup): B.L = 32768 is exactly
    2048 workgroups of one pass, 33000 is capped and starts the grid-stride loop with a ragged second pass.  The cap of
    cl_dw_wgrad_c4_kernel is not reached here: it needs 2048 . 8 . 1024 floats = 268 MB of gradient."""
    assert _dw_case("2", (1, 128, L), 5, 1, True, L) == "ran"


@pytest.mark.parametrize("shape", [(1, 64, 1800), (1, 64, 2048), (1, 64, 15360), (1, 64, 16384), (1, 64, 32768), (1, 64, 33000), (1, 2, 1000),
                                   (2, 1024, 3, 5)])
def test_bias_column_sum_edges_exact(shape):
    """dbias of a depthwise 1x1: cl_colsum_kernel on g = ceil(rows . C / 8192) workgroups.  g = 15: atomics and no second stage; 16:
    the two-stage path; 120 / 128: its fold (cl_dw_wgrad_reduce_kernel, one tap) on both sides of the slice switch; 256: the cap, met
    exactly and passed (grid-stride loop); C = 2: cl_colsum_any_kernel over 16 row chunks; C = 1024: every thread its own quad."""
    assert _dw_case("2", shape, 1, 1, True, sum(shape)) == "ran"


# ------------------------------------------------------------------------------------------------ 3. stage kernels
S3 = "3 stage kernels"
DW_GLN_PRELU = dict(kernel_size=4, depthwise=True, norm_type="gLN", act_type="PReLU")  # tfar_gate-like, PReLU for the slope's gradient
PRE_GLN_RELU = dict(kernel_size=1, pre_norm_type="gLN", pre_act_type="ReLU")  # audio_bn


def _ref_forward(x, P, mod, masks, bn):
    """ConvNormAct in float64 torch ops from the module's own stage types; ReLU / PReLU on the given sign patterns."""
    pre_n, pre_a, conv, nrm, act = mod.full_layer

    def act_fn(v, m, slope, mask):
        if isinstance(m, nn.ReLU):
            return torch.where(mask, v, torch.zeros_like(v))
        if isinstance(m, nn.PReLU):
            return torch.where(mask, v, slope * v)
        return torch.sigmoid(v) if isinstance(m, nn.Sigmoid) else v
    if not isinstance(pre_n, nn.Identity):
        x = F.group_norm(x, 1, P["full_layer.0.norm.weight"], P["full_layer.0.norm.bias"], 1e-5)
    x = act_fn(x, pre_a, P.get("full_layer.1.weight"), masks.get("pre"))
    k, s = mod.kernel_size, mod.stride
    x = (F.conv2d if isinstance(conv, nn.Conv2d) else F.conv1d)(x, P["full_layer.2.weight"], P.get("full_layer.2.bias"), stride=s,
                                                                padding=(k - 1) // 2 if s > 1 else "same", groups=conv.groups)
    if bn:
        x = F.batch_norm(x, P["full_layer.3.running_mean"], P["full_layer.3.running_var"], P["full_layer.3.weight"], P["full_layer.3.bias"],
                         bn == "train", 0.1, 1e-5)
    elif not isinstance(nrm, nn.Identity):
        x = F.group_norm(x, 1, P["full_layer.3.norm.weight"], P["full_layer.3.norm.bias"], 1e-5)
    return act_fn(x, act, P.get("full_layer.4.weight"), masks.get("post"))


def _cna_case(name, C, kw, shape, seed, rows=None, bn=None):
    """One ConvNormAct through forward and backward of the training kernels against float64 autograd: output, dx, every parameter
    gradient, and for BatchNorm the running buffers.  shape is channel-first; rows = (input, output) runs _forward_train on (B, H, W, C)
    rows instead.  dout has mean 0.25, so that the PReLU slope's gradient (one sum over the whole tensor) is not a cancelled sum."""
    import rtfs_net_amd as R
    kw = dict(kw)
    groups = C if kw.pop("depthwise", False) else 1
    torch.manual_seed(seed)
    mod = R.layers.ConvNormAct(C, C, groups=groups, is2d=len(shape) == 4, **kw)
    pre_n, pre_a, conv, nrm, act = mod.full_layer
    with torch.no_grad():
        for k, v in mod.named_parameters():  # away from the init values (gamma 1, beta 0); PReLU slopes stay positive
            if k in ("full_layer.1.weight", "full_layer.4.weight"):
                v.fill_(0.2 if k[11] == "1" else 0.3)
            elif not k.startswith("full_layer.2.") or k.endswith("bias"):
                v.add_(0.3 * torch.randn_like(v))
        if bn:
            nrm.running_mean.copy_(0.3 * torch.randn_like(nrm.running_mean))
            nrm.running_var.copy_(1 + 0.5 * torch.rand_like(nrm.running_var))
    names = [k for k, _ in mod.named_parameters()]
    P = {k: v.detach().double().clone().requires_grad_(k in names) for k, v in mod.state_dict().items() if "num_batches" not in k}
    mod = mod.cuda().train()
    if bn == "frozen":
        nrm.eval()
    x = rand(shape, seed)
    to_rows = lambda a: np.ascontiguousarray(np.moveaxis(a, 1, -1))
    xt = dev(to_rows(x) if rows and rows[0] else x).requires_grad_(True)
    out = mod(xt) if rows is None else mod._forward_train(xt, rows)
    saved = out.grad_fn.saved_tensors[1]  # r0 | r2 = the pre-stage's output as rows | r3 | statistics (api_train.hip CnaSaved)
    o = host(out)
    if rows and rows[1]:
        o = np.moveaxis(o, -1, 1)
    dout = rand(o.shape, seed + 1) + np.float32(0.25)
    out.backward(dev(to_rows(dout) if rows and rows[1] else dout))
    masks = {}
    if isinstance(pre_a, (nn.ReLU, nn.PReLU)):
        r2 = np.moveaxis(host(saved[x.size:2 * x.size]).reshape((shape[0],) + tuple(shape[2:]) + (C,)), -1, 1)
        masks["pre"] = torch.from_numpy(np.ascontiguousarray(r2 > 0 if isinstance(pre_a, nn.ReLU) else r2 >= 0))
    if isinstance(act, (nn.ReLU, nn.PReLU)):
        masks["post"] = torch.from_numpy(np.ascontiguousarray(o > 0 if isinstance(act, nn.ReLU) else o >= 0))
    xr = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    ref = _ref_forward(xr, P, mod, masks, bn)
    ref.backward(torch.tensor(dout, dtype=torch.float64))
    _chk(S3, f"{name} forward", o, ref.detach().numpy())
    dx = host(xt.grad)
    _chk(S3, f"{name} dx", np.moveaxis(dx, -1, 1) if rows and rows[0] else dx, xr.grad.numpy(), 2e-4)
    for k, v in mod.named_parameters():
        assert v.grad is not None, k
        _chk(S3, f"{name} d {k}", host(v.grad).reshape(P[k].shape), P[k].grad.numpy(), 2e-4)
    if bn:  # nn.BatchNorm's buffers: untouched when frozen, the momentum update (unbiased variance) in train mode
        close(f"{name} running_mean", host(nrm.running_mean), P["full_layer.3.running_mean"].numpy(), tol=1e-5)
        close(f"{name} running_var", host(nrm.running_var), P["full_layer.3.running_var"].numpy(), tol=1e-5)
        assert int(nrm.num_batches_tracked) == (1 if bn == "train" else 0)


STAGE_SHAPES = [(1, 64, 62, 128), (1, 64, 64, 128), (1, 64, 127, 128), (1, 64, 129, 128), (3, 64, 5, 7)]


@pytest.mark.parametrize("shape", STAGE_SHAPES)
@pytest.mark.parametrize("cfg", ["dw_gln_prelu", "pre_gln_relu"])
def test_stage_kernels_fold_switch_and_grid_cap(cfg, shape):
    """The stage kernels at C = 64 behind a depthwise k = 4 + gLN + PReLU (post-stage) and in front of a dense 1x1 as gLN + ReLU
    (pre-stage, audio_bn's configuration).  The backward reduction runs gx = ceil4(n / 4096) workgroups per sample, n = H.W.C, capped at
    256: (62, 128) and (64, 128) leave 124 and 128 partial rows, either side of cl_stage_reduce2_kernel's slice switch; (127, 128) and
    (129, 128) are n just under and over 1,048,576, the cap (grid-stride loop, 2048-workgroup cap of forward and apply not reached);
    (3, 64, 5, 7): three samples whose n / 4 = 560 is no multiple of 256."""
    kw = DW_GLN_PRELU if cfg == "dw_gln_prelu" else PRE_GLN_RELU
    _cna_case(f"{cfg} {shape}", 64, kw, shape, 3000 + sum(shape))


@pytest.mark.parametrize("name,C,kw,shape", [
    ("dw C1024", 1024, DW_GLN_PRELU, (2, 1024, 3, 5)),
    ("dense C1024", 1024, dict(kernel_size=1, pre_norm_type="gLN", pre_act_type="ReLU", norm_type="gLN", act_type="PReLU"), (2, 1024, 3, 5)),
    ("dw C4", 4, DW_GLN_PRELU, (2, 4, 5, 7)),
    ("dw C4 wide", 4, DW_GLN_PRELU, (1, 4, 64, 65)),
    ("dw C2", 2, DW_GLN_PRELU, (2, 2, 5, 7)),
    ("dw C2 wide", 2, DW_GLN_PRELU, (1, 2, 40, 41)),
    ("dw sigmoid", 64, dict(DW_GLN_PRELU, act_type="Sigmoid"), (2, 64, 10, 33)),
    ("dw no act", 64, dict(DW_GLN_PRELU, act_type=None), (2, 64, 10, 33)),
    ("dw relu no norm", 64, dict(kernel_size=4, depthwise=True, act_type="ReLU"), (2, 64, 10, 33)),
    ("dw pre gLN PReLU", 64, dict(kernel_size=4, depthwise=True, pre_norm_type="gLN", pre_act_type="PReLU"), (2, 64, 10, 33)),
    ("dw stride 2", 64, dict(DW_GLN_PRELU, stride=2), (2, 64, 11, 33)),
])
def test_stage_kernels_channel_counts_and_activations(name, C, kw, shape):
    """C = 1024: every thread of a workgroup its own channel quad (depthwise in slices, and dense with both stages); C = 4: 64 threads
    per quad; C = 2: the V = 1 variants of the three stage kernels (one and 16 workgroups per sample); Sigmoid, no activation, an
    activation without a norm and a PReLU pre-stage (its slope's gradient slot) at one mid-size map; stride 2 (n_out != n_in)."""
    _cna_case(name, C, kw, shape, 3100 + C + sum(shape))


@pytest.mark.parametrize("bn,shape", [("frozen", (2, 512, 50)), ("train", (2, 512, 1)), ("train", (3, 512, 1)), ("train", (1, 512, 3)),
                                      ("train", (4, 512, 300))])
def test_stage_kernels_batchnorm(bn, shape):
    """BatchNorm1d + ReLU behind a depthwise 1x1 at C = 512 (the CAF cell's key_embed): frozen statistics (norm 2), and train mode
    (norm 3: cl_chan_stats_kernel's C >= 256 route, bn_update_kernel) over 2 and 3 rows and over 1200 (the statistics' grid capped
    at 1024 workgroups), against F.batch_norm in float64, running buffers and batch counter included."""
    _cna_case(f"bn {bn} {shape}", 512, dict(kernel_size=1, depthwise=True, norm_type="BatchNorm1d", act_type="ReLU", bias=False), shape,
              3200 + sum(shape), bn=bn)


@pytest.mark.parametrize("rows", [(True, True), (True, False)])
@pytest.mark.parametrize("cfg", ["dw_gln_prelu", "pre_gln_relu"])
def test_stage_kernels_rows_in_place_dx(cfg, rows):
    """_forward_train on (B, H, W, C) rows: the backward then writes the module's dx in place of an intermediate - the convolution's
    input gradient (depthwise, no pre-stage) or the pre-stage's apply pass (dense)."""
    kw = DW_GLN_PRELU if cfg == "dw_gln_prelu" else PRE_GLN_RELU
    _cna_case(f"{cfg} rows {rows}", 64, kw, (2, 64, 9, 13), 3300 + rows[1], rows=rows)


# ------------------------------------------------------------------------------------------------ 4. gateway
@pytest.mark.parametrize("shape,with_res", [((3, 5, 7, 4), True), ((3, 5, 7, 4), False), ((1, 3, 7, 1024), True), ((1, 1, 1984, 256), False),
                                            ((1, 1, 2048, 256), True), ((1, 1, 8101, 256), False), ((1, 1, 8301, 256), True),
                                            ((1, 1, 8301, 256), False)])
def test_gateway_edges(shape, with_res):
    """rtfs_gateway_*: C = 4 (105 quads: one ragged workgroup) and C = 1024; rows = 1984 and 2048 at C = 256 leave 124 and 128 partial
    rows (the fold's slice switch); rows . C = 2.07 M and 2.13 M are under and over the backward's 512-workgroup cap, with rows . C / 4
    no multiple of 256.  Reference, kink handling (|z| > 1e-3) and bars of test_gateway_one_pass_forward_backward."""
    import rtfs_net_amd as R
    from rtfs_net_amd import layers as L
    S4 = "4 gateway"
    C, seed = shape[-1], 4000 + sum(shape) + int(with_res)
    cna = R.layers.ConvNormAct(C, C, 1, groups=C, act_type="PReLU", is2d=True).cuda().train()
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        cna.full_layer[2].weight.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, (C, 1, 1, 1)).astype(np.float32)))
        cna.full_layer[2].bias.copy_(torch.from_numpy(rng.uniform(-0.2, 0.2, C).astype(np.float32)))
        cna.full_layer[4].weight.fill_(0.3)
    x = rand(shape, seed)
    res = rand(shape, seed + 1) if with_res else None
    w64 = cna.full_layer[2].weight.detach().double().cpu().reshape(C)
    b64 = cna.full_layer[2].bias.detach().double().cpu()
    z0 = w64 * (torch.from_numpy(x).double() + (torch.from_numpy(res).double() if with_res else 0)) + b64
    x = np.where(np.abs(z0.numpy()) < 1e-3, x + 0.01, x).astype(np.float32)  # move the few pre-activations near 0 away from the kink
    dout = rand(shape, seed + 2)
    xt = dev(x).requires_grad_(True)
    rt = dev(res).requires_grad_(True) if with_res else None
    out = L.gateway_train(cna, xt, rt)
    assert out is not None
    out.backward(dev(dout))
    x64 = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    r64 = torch.tensor(res, dtype=torch.float64, requires_grad=True) if with_res else None
    w, b = w64.clone().requires_grad_(True), b64.clone().requires_grad_(True)
    sl = torch.tensor([0.3], dtype=torch.float64, requires_grad=True)
    z = w * (x64 + r64 if with_res else x64) + b
    ref = torch.where(z >= 0, z, sl * z)
    ref.backward(torch.tensor(dout, dtype=torch.float64))
    _chk(S4, "gateway forward", host(out), ref.detach().numpy(), 1e-6)
    _chk(S4, "gateway dx", host(xt.grad), x64.grad.numpy(), 1e-5)
    if with_res:
        _chk(S4, "gateway dx_res", host(rt.grad), r64.grad.numpy(), 1e-5)
    _chk(S4, "gateway dweight", host(cna.full_layer[2].weight.grad).reshape(C), w.grad.numpy(), 1e-5)
    _chk(S4, "gateway dbias", host(cna.full_layer[2].bias.grad), b.grad.numpy(), 1e-5)
    _chk(S4, "gateway dslope", host(cna.full_layer[4].weight.grad), sl.grad.numpy(), 1e-5)


# ------------------------------------------------------------------------------------------------ 5. glue by name through the C ABI
S5 = "5 glue"


def _t64(a):
    return torch.tensor(a, dtype=torch.float64, requires_grad=True)


def _up(t, T):
    """(..., Tv) -> (..., T), F.interpolate(mode="nearest") over the last axis."""
    return F.interpolate(t.reshape(1, -1, t.shape[-1]), size=T, mode="nearest").reshape(t.shape[:-1] + (T,))


@pytest.mark.parametrize("Tv", [1, 2, 63, 64, 65, 128, 129, 255, 256])
def test_caf_attention_c_abi(Tv):
    """rtfs_caf_attention_f32 / _backward_f32: one wave per (b, c) with four positions per lane, Tv at and next to the wave size and
    its multiples up to the 256 the kernel holds; B.C = 9, so the third workgroup has one live wave of four."""
    lib, L = _lib()
    B, C = 3, 3
    emb, datt = rand((B, 4 * C, Tv), 5000 + Tv), rand((B, C, Tv), 5300 + Tv)
    er = _t64(emb)
    ar = torch.softmax(er.reshape(B, C, 4, Tv).mean(2), -1)
    ar.backward(torch.tensor(datt, dtype=torch.float64))
    e, d, att, demb = dev(emb), dev(datt), _guarded(B, C, Tv), _guarded(B, 4 * C, Tv)
    st = L.stream_of(e)
    L.check(lib.rtfs_caf_attention_f32(L.ptr(e), L.ptr(att), B, C, Tv, st), "rtfs_caf_attention_f32")
    _chk(S5, f"caf attention Tv {Tv}", _unguard(att, (B, C, Tv), "att"), ar.detach().numpy())
    L.check(lib.rtfs_caf_attention_backward_f32(L.ptr(att), L.ptr(d), L.ptr(demb), B, C, Tv, st), "rtfs_caf_attention_backward_f32")
    _chk(S5, f"caf attention Tv {Tv} d embed", _unguard(demb, (B, 4 * C, Tv), "demb"), er.grad.numpy(), 2e-4)


@pytest.mark.parametrize("Fq", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("T,Tv", [(5, 1), (5, 5), (9, 4)])
def test_caf_combine_c_abi(T, Tv, Fq):
    """rtfs_caf_combine_f32 / _backward_f32 on channel-first planes: one wave per (n, tv) strides over F, so F at and next to the wave
    size; Tv = 1 (every frame reads the one video frame), Tv = T and an uneven fan-out."""
    lib, L = _lib()
    N = 3
    key, value, dout = [rand((N, T, Fq), 5500 + 10 * Fq + i) for i in range(3)]
    r, att = rand((N, Tv), 5600 + Tv), rand((N, Tv), 5700 + Tv)
    kr, vr, rr, ar = [_t64(a) for a in (key, value, r, att)]
    ref = kr * _up(rr, T)[:, :, None] + _up(ar, T)[:, :, None] * vr
    ref.backward(torch.tensor(dout, dtype=torch.float64))
    kd, vd, rd, ad, dd = [dev(a) for a in (key, value, r, att, dout)]
    out, dk, dv, dr, da = _guarded(N, T, Fq), _guarded(N, T, Fq), _guarded(N, T, Fq), _guarded(N, Tv), _guarded(N, Tv)
    st = L.stream_of(kd)
    L.check(lib.rtfs_caf_combine_f32(L.ptr(kd), L.ptr(vd), L.ptr(rd), L.ptr(ad), L.ptr(out), N, T, Fq, Tv, st), "rtfs_caf_combine_f32")
    L.check(lib.rtfs_caf_combine_backward_f32(L.ptr(dd), L.ptr(kd), L.ptr(vd), L.ptr(rd), L.ptr(ad), L.ptr(dk), L.ptr(dv), L.ptr(dr), L.ptr(da),
                                              N, T, Fq, Tv, st), "rtfs_caf_combine_backward_f32")
    _chk(S5, "caf combine", _unguard(out, (N, T, Fq), "out"), ref.detach().numpy(), 1e-6)
    for nm, g, rf in (("dkey", dk, kr), ("dvalue", dv, vr), ("dresized", dr, rr), ("datt", da, ar)):
        _chk(S5, f"caf combine {nm}", _unguard(g, tuple(rf.shape), nm), rf.grad.numpy(), 2e-6)


@pytest.mark.parametrize("T,Tv", [(9, 4), (33, 7), (5, 5), (6, 1)])
@pytest.mark.parametrize("C,Fq", [(4, 5), (4, 300), (64, 3), (64, 129), (1024, 1), (1024, 3)])
def test_caf_combine_rows_c_abi(C, Fq, T, Tv):
    """rtfs_caf_combine_rows_f32 / _backward_f32: one workgroup per (b, t) slab of F.C / 4 quads - 5 and 48 (fewer than its threads),
    300 and 2064 (no multiple of 256), 256 and 768 at C = 1024 (every thread its own quad); several frames t share one video frame tv,
    so dresized / datt are met by atomics from several workgroups."""
    lib, L = _lib()
    B = 2
    key, value, dout = [rand((B, T, Fq, C), 5800 + C + Fq + i) for i in range(3)]
    r, att = rand((B, C, Tv), 5900 + Tv), rand((B, C, Tv), 6000 + Tv)
    kr, vr, rr, ar = [_t64(a) for a in (key, value, r, att)]
    rows = lambda t: _up(t, T).permute(0, 2, 1)[:, :, None, :]  # (B, C, T) -> (B, T, 1, C)
    ref = kr * rows(rr) + rows(ar) * vr
    ref.backward(torch.tensor(dout, dtype=torch.float64))
    kd, vd, rd, ad, dd = [dev(a) for a in (key, value, r, att, dout)]
    out, dk, dv, dr, da = _guarded(B, T, Fq, C), _guarded(B, T, Fq, C), _guarded(B, T, Fq, C), _guarded(B, C, Tv), _guarded(B, C, Tv)
    st = L.stream_of(kd)
    L.check(lib.rtfs_caf_combine_rows_f32(L.ptr(kd), L.ptr(vd), L.ptr(rd), L.ptr(ad), L.ptr(out), B, T, Fq, C, Tv, st), "rtfs_caf_combine_rows_f32")
    L.check(lib.rtfs_caf_combine_rows_backward_f32(L.ptr(dd), L.ptr(kd), L.ptr(vd), L.ptr(rd), L.ptr(ad), L.ptr(dk), L.ptr(dv), L.ptr(dr),
                                                   L.ptr(da), B, T, Fq, C, Tv, st), "rtfs_caf_combine_rows_backward_f32")
    _chk(S5, "caf combine rows", _unguard(out, (B, T, Fq, C), "out"), ref.detach().numpy(), 1e-6)
    for nm, g, rf in (("dkey", dk, kr), ("dvalue", dv, vr), ("dresized", dr, rr), ("datt", da, ar)):
        _chk(S5, f"caf combine rows {nm}", _unguard(g, tuple(rf.shape), nm), rf.grad.numpy(), 2e-6)


@pytest.mark.parametrize("inner", [1, 2, 4, 64])
def test_pool_and_tfar_combine_inner_channels_c_abi(inner):
    """rtfs_adaptive_avg_pool2d_* and rtfs_tfar_combine_* on rows with inner = C channels fastest (1: planes, 2: the scalar variants,
    4 and 64: the V = 4 ones) over the four size pairs of test_pool_and_tfar_combine_adjoints, against F.adaptive_avg_pool2d and
    F.interpolate(mode="nearest") on the channel-first view."""
    lib, L = _lib()
    N = 6 if inner == 1 else 2
    cf = lambda a: torch.tensor(np.ascontiguousarray(np.moveaxis(a, -1, 1)), dtype=torch.float64, requires_grad=True)
    back = lambda t: np.moveaxis(t.numpy(), 1, -1)
    for (H, W, Ho, Wo) in [(17, 129, 8, 64), (251, 9, 125, 4), (8, 64, 8, 64), (5, 7, 2, 3)]:
        big, small = (N, H, W, inner), (N, Ho, Wo, inner)
        x, dy = rand(big, H + W + inner), rand(small, H + inner)
        xr = cf(x)
        yr = F.adaptive_avg_pool2d(xr, (Ho, Wo))
        yr.backward(cf(dy).detach())
        xd, dyd, y, dx = dev(x), dev(dy), _guarded(*small), _guarded(*big)
        st = L.stream_of(xd)
        L.check(lib.rtfs_adaptive_avg_pool2d_f32(L.ptr(xd), L.ptr(y), N, H, W, Ho, Wo, inner, st), "rtfs_adaptive_avg_pool2d_f32")
        L.check(lib.rtfs_adaptive_avg_pool2d_backward_f32(L.ptr(dyd), L.ptr(dx), N, H, W, Ho, Wo, inner, st), "rtfs_adaptive_avg_pool2d_backward_f32")
        tag = f"{H}x{W}->{Ho}x{Wo} inner {inner}"
        _chk(S5, f"pool {tag}", _unguard(y, small, "y"), back(yr.detach()), 1e-6)
        _chk(S5, f"pool adjoint {tag}", _unguard(dx, big, "dx"), back(xr.grad), 1e-6)
        le, ga, ge, do = rand(big, 1), rand(small, 2), rand(small, 3), rand(big, 4)
        rs = [cf(a) for a in (le, ga, ge)]
        orf = rs[0] * F.interpolate(rs[1], size=(H, W), mode="nearest") + F.interpolate(rs[2], size=(H, W), mode="nearest")
        orf.backward(cf(do).detach())
        led, gad, ged, dod = [dev(a) for a in (le, ga, ge, do)]
        o, dl, dg, de = _guarded(*big), _guarded(*big), _guarded(*small), _guarded(*small)
        L.check(lib.rtfs_tfar_combine_f32(L.ptr(led), L.ptr(gad), L.ptr(ged), L.ptr(o), N, H, W, Ho, Wo, inner, st), "rtfs_tfar_combine_f32")
        L.check(lib.rtfs_tfar_combine_backward_f32(L.ptr(dod), L.ptr(led), L.ptr(gad), L.ptr(dl), L.ptr(dg), L.ptr(de), N, H, W, Ho, Wo, inner, st),
                "rtfs_tfar_combine_backward_f32")
        _chk(S5, f"tfar combine {tag}", _unguard(o, big, "out"), back(orf.detach()), 1e-6)
        for nm, g, shp, rf in (("dlocal", dl, big, rs[0]), ("dgate", dg, small, rs[1]), ("dglobal", de, small, rs[2])):
            _chk(S5, f"tfar combine {nm} {tag}", _unguard(g, shp, nm), back(rf.grad), 2e-6)


# ------------------------------------------------------------------------------------------------ 6. refusals
def _cna_abi(cfg, B, H, W, short=0):
    """rtfs_cna_forward_train_f32 and rtfs_cna_backward_f32 by name on NaN-filled buffers of the sizes the queries give.  Returns the two
    return codes after asserting that nothing was launched and nothing written."""
    lib, L = _lib()
    carr = (ctypes.c_int * 15)(*cfg)
    cin, cout = cfg[0], cfg[1]
    x, dout = dev(rand((B, cin, H, W), 1)), dev(rand((B, cout, H, W), 2))
    params = torch.zeros(lib.rtfs_cna_param_floats(carr), device="cuda")
    ws_bytes = lib.rtfs_cna_workspace_bytes(carr, B, H, W)
    outs = dict(out=_nan(B * cout * H * W), saved=_nan(lib.rtfs_cna_saved_floats(carr, B, H, W)), dx=_nan(B * cin * H * W),
                dparams=_nan(lib.rtfs_cna_grad_floats(carr)), ws=_nan((ws_bytes + 3) // 4))
    st = L.stream_of(x)
    torch.cuda.synchronize()
    n0 = lib.rtfs_debug_launch_count()
    rc_f = lib.rtfs_cna_forward_train_f32(L.ptr(x), L.ptr(params), L.ptr(outs["out"]), L.ptr(outs["saved"]), carr, B, H, W, L.ptr(outs["ws"]),
                                          ws_bytes - short, st)
    rc_b = lib.rtfs_cna_backward_f32(None, L.ptr(params), L.ptr(outs["saved"]), L.ptr(dout), L.ptr(outs["dx"]), L.ptr(outs["dparams"]), carr, B, H, W,
                                     L.ptr(outs["ws"]), ws_bytes - short, st)
    torch.cuda.synchronize()
    assert lib.rtfs_debug_launch_count() == n0, "a refused call launched a kernel"
    for name, t in outs.items():
        assert bool(torch.isnan(t).all()), f"{name} was written by a refused call"
    return rc_f, rc_b


#          Cin Cout k  s dw pre_norm pre_act norm act bias is2d phase world in_rows out_rows
CNA_REFUSED = {
    "channels not a power of two": ((96, 96, 1, 1, 1, 0, 0, 0, 0, 1, 1, 0, 1, 0, 0), 5, 7),
    "dense k = 3": ((64, 64, 3, 1, 0, 0, 0, 1, 2, 1, 1, 0, 1, 0, 0), 5, 7),
    "k = 5 on a 2-D map": ((64, 64, 5, 1, 1, 0, 0, 0, 0, 1, 1, 0, 1, 0, 0), 6, 7),
    "stride 3": ((64, 64, 3, 3, 1, 0, 0, 0, 0, 1, 1, 0, 1, 0, 0), 7, 7),
    "stride 2, padded height below k": ((64, 64, 4, 2, 1, 0, 0, 0, 0, 1, 1, 0, 1, 0, 0), 1, 8),
    "stride 2, padded width below k": ((64, 64, 2, 2, 1, 0, 0, 0, 0, 1, 0, 0, 1, 0, 0), 1, 1),
}


@pytest.mark.parametrize("why", sorted(CNA_REFUSED))
def test_cna_refused_shapes(why):
    """Configurations outside the ConvNormAct contract of include/rtfs_amd.h: RTFS_ERR_SHAPE from forward and backward, nothing
    launched, every output, the saved state and the workspace still NaN."""
    cfg, H, W = CNA_REFUSED[why]
    assert _cna_abi(cfg, 2, H, W) == (ERR_SHAPE, ERR_SHAPE)


def test_cna_and_gateway_workspace_one_byte_short():
    """One byte less than rtfs_cna_workspace_bytes / rtfs_gateway_workspace_bytes ask for: RTFS_ERR_WORKSPACE, nothing launched or
    written."""
    assert _cna_abi((64, 64, 4, 1, 1, 0, 0, 1, 2, 1, 1, 0, 1, 0, 0), 2, 5, 7, short=1) == (ERR_WORKSPACE, ERR_WORKSPACE)
    lib, L = _lib()
    C, rows = 64, 9
    x, dout, w, b, sl = [dev(rand(s, i)) for i, s in enumerate([(rows, C), (rows, C), (C,), (C,), (1,)])]
    ws_bytes = lib.rtfs_gateway_workspace_bytes(C)
    dx, dpar, ws = _nan(rows, C), _nan(lib.rtfs_gateway_grad_floats(C)), _nan((ws_bytes + 3) // 4)
    torch.cuda.synchronize()
    n0 = lib.rtfs_debug_launch_count()
    rc = lib.rtfs_gateway_backward_f32(L.ptr(x), None, L.ptr(w), L.ptr(b), L.ptr(sl), L.ptr(dout), L.ptr(dx), L.ptr(dpar), rows, C, L.ptr(ws),
                                       ws_bytes - 1, L.stream_of(x))
    torch.cuda.synchronize()
    assert rc == ERR_WORKSPACE and lib.rtfs_debug_launch_count() == n0
    assert all(bool(torch.isnan(t).all()) for t in (dx, dpar, ws))


def test_glue_refused_shapes():
    """Tv = 257 for the CAF attention (one wave holds 256 positions), Tv > T for both combines, a global map taller than the local one
    for the TFAR combine and a pooled map taller than its input: RTFS_ERR_SHAPE from every entry point, nothing launched, outputs NaN."""
    lib, L = _lib()
    a = dev(rand((4096,), 1))  # every input: large enough for each call below had it been accepted
    p, st = L.ptr(a), L.stream_of(a)
    outs = [_nan(4096) for _ in range(4)]
    o = [L.ptr(t) for t in outs]
    torch.cuda.synchronize()
    n0 = lib.rtfs_debug_launch_count()
    rcs = {
        "caf attention Tv 257": lib.rtfs_caf_attention_f32(p, o[0], 1, 1, 257, st),
        "caf attention backward Tv 257": lib.rtfs_caf_attention_backward_f32(p, p, o[0], 1, 1, 257, st),
        "caf combine Tv > T": lib.rtfs_caf_combine_f32(p, p, p, p, o[0], 2, 3, 5, 4, st),
        "caf combine backward Tv > T": lib.rtfs_caf_combine_backward_f32(p, p, p, p, p, o[0], o[1], o[2], o[3], 2, 3, 5, 4, st),
        "caf combine rows Tv > T": lib.rtfs_caf_combine_rows_f32(p, p, p, p, o[0], 1, 3, 5, 4, 4, st),
        "caf combine rows backward Tv > T": lib.rtfs_caf_combine_rows_backward_f32(p, p, p, p, p, o[0], o[1], o[2], o[3], 1, 3, 5, 4, 4, st),
        "tfar combine Hg > H": lib.rtfs_tfar_combine_f32(p, p, p, o[0], 2, 3, 5, 4, 5, 1, st),
        "tfar combine backward Hg > H": lib.rtfs_tfar_combine_backward_f32(p, p, p, o[0], o[1], o[2], 2, 3, 5, 4, 5, 1, st),
        "pool Ho > H": lib.rtfs_adaptive_avg_pool2d_f32(p, o[0], 2, 3, 5, 4, 5, 1, st),
        "pool backward Ho > H": lib.rtfs_adaptive_avg_pool2d_backward_f32(p, o[0], 2, 3, 5, 4, 5, 1, st),
    }
    torch.cuda.synchronize()
    assert all(rc == ERR_SHAPE for rc in rcs.values()), rcs
    assert lib.rtfs_debug_launch_count() == n0, "a refused call launched a kernel"
    assert all(bool(torch.isnan(t).all()) for t in outs)
