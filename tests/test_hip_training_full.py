"""The training side at the shape it trains at: 2 s segments at batch 4 (every RTFS-Net yaml: segment 2.0, batch_size 4; what
`bench.py --train` times), batch 16, and the longest segment the backward takes.  The launchers in k_train_conv.hip / k_train_gemm.hip
choose grids and code paths from the tensor size; the tests in test_hip_training.py run at 0.26 s or less and never reach the
large-size branches.  Each branch, the test that reaches it and the grid it runs with there (kernel trace of this file,
profiles/training_full_grids.csv; grids in workgroups):

- launch_gateway, backward grid capped at 2 x CL_STAGE_MAX_WG: gateway_kernel<true> (512) for 2,072,256 float4 quads per pass
  (8,095 uncapped), each thread striding over the grid; then cl_stage_reduce2_kernel (9, 32), the 32-row second stage.
  test_gateway_one_pass_2s, the row-layout steps.
- launch_cl_norm_act_bwd, reduction capped at CL_STAGE_MAX_WG: cl_norm_act_bwd_reduce_kernel<4> (256, B) for 129,516 quads per sample
  (506 uncapped); then cl_stage_reduce2_kernel with 32 rows (9, 32) / (33, 32).  test_conv_norm_act_training_2s[projection], the
  channel-first step, test_training_step_batch16_equals_mean_of_four_batch4_steps ((256, 16)).
- launch_cl_colsum, two-stage `partial` fold: cl_colsum_kernel (256) + cl_dw_wgrad_reduce_kernel (1, 32) for C = 64 and (4, 32) for
  C = 256.  The bias gradients: test_conv_norm_act_training_2s[residual_conv / downsample], every step.
- cl_dw_wgrad_reduce_kernel after a depthwise weight gradient with >= 128 workgroups: (4, 32).  launch_cl_dw_chunk's kernels by
  shape: cl_dw_wgrad_w4c4_kernel (696 for C = 64, 760 for C = 256, stride 1), cl_dw_wgrad_c4_kernel (256 at B = 4, 1000 at B = 16,
  the stride-2 level), all under CL_DW_WGRAD_MAX_WG = 2048.  test_conv_norm_act_training_2s[downsample / tfar_gate / gateway],
  test_batchnorm_train_conv_norm_act_2s, the steps.
- launch_gemm_tn, weight gradient split over K: gemm_tn_kernel 2032 = 127 workgroups of four chunks x 16 tiles (K = 129,516 or 518,064
  in 506 chunks merged by f32 atomics).  The steps; test_training_gemms' K = 129,516 / 518,064 rows (test_hip_training.py).
- BatchNorm training statistics, double atomics: cl_chan_stats_kernel at its 1024-workgroup cap over 129,516 rows per channel.
  test_batchnorm_train_conv_norm_act_2s, the all-train steps (CAF BatchNorm).
- The 256-position backward limit (TRAIN_MAX_SWEEP): test_training_step_at_the_length_limit_vs_float64 at it,
  test_training_step_past_the_length_limit_refused_before_any_launch one frame past it.

Oracles are float64 torch autograd (oracle/grad_oracle.py); the 2 s x 4 whole-step oracle is computed once per module and shared by
the two layouts.  The file takes 183 s and 19.5 GB of host memory on an MI355X box's 16-CPU share (most of both: that oracle)."""
import copy

import numpy as np
import pytest
import torch

from oracle import grad_oracle as G
from oracle import rtfs_oracle as O
from oracle.params import make_inputs
from tests import test_hip_training as TT
from tests.test_hip_parity import BLK, close, dev, host, lstm_model, model
from tests.util import l2_rel, rand, rel_err

pytestmark = pytest.mark.gpu

B, L, TV = 4, 32000, 50       # 2 s at 16 kHz, 25 fps video: the reference's training segment and batch
T, F = 1 + L // 128, 129      # 251 STFT frames, 129 bins
T2, F2 = 125, 64              # after the block's stride-2 level: what the dual-path sweeps and the TF attention run over
L_MAX, L_OVER = 65663, 65664  # 4.104 s: the longest segment whose coarsest time sweep is TRAIN_MAX_SWEEP = 256 positions, and one past it


def _loss_mod():
    import rtfs_net_amd as R
    return R.losses.PITLossWrapper(R.losses.PairwiseNegSDR("snr"), pit_from="pw_mtx")


def _all_train(m):
    """Plain .train(): every parameter trains, BatchNorm on batch statistics; the VP block's dropout 0 so the oracle can follow."""
    m.train()
    ga = m.refinement_module.video_net.get_block(0).globalatt[0]
    ga.MHSA.dropout, ga.MHSA.dropout_layer.p, ga.FFN.dropout = 0.0, 0.0, 0.0
    return m


def _smooth(m):
    """The activation kinks out of reach, as in test_avnet_training_step_end_to_end: every PReLU slope 1, the mask ReLU inactive."""
    with torch.no_grad():
        for k, v in m.named_parameters():
            if k.endswith("act.weight") or k.endswith("full_layer.4.weight") or k == "mask_generator.mask_generator.0.weight":
                v.fill_(1.0)
        m.mask_generator.mask_generator[1].full_layer[2].bias.add_(5.0)
    return m


def _hip_step(m, wav, emb, tgt):
    out = m(dev(wav), dev(emb))
    loss = _loss_mod()(out, dev(tgt))
    loss.backward()
    return dict(out=host(out), loss=float(loss), grads={k: host(v.grad) for k, v in m.named_parameters() if v.requires_grad},
                stats={k: host(v) for k, v in m.state_dict().items() if "running" in k})


def _oracle_step(m, wav, emb, tgt, repeats):
    """The same step in float64: AVNet forward with the VP block differentiated and BatchNorm on batch statistics, PIT neg-SNR loss,
    every parameter gradient, and the BatchNorm running statistics after torch's momentum update."""
    p = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items() if "num_batches" not in k}
    pt = {k: torch.tensor(v, dtype=torch.float64, requires_grad=("running" not in k and not k.endswith("pos_enc.pe"))) for k, v in p.items()}
    f64 = dict(dtype=torch.float64)
    o = G.avnet_torch(torch.tensor(wav, **f64), torch.tensor(emb, **f64), pt, repeats, vp_trainable=True, bn_train=True)
    loss = G.pit_loss_torch(o, torch.tensor(tgt, **f64), "snr")
    loss.backward()
    return dict(out=o.detach().numpy(), loss=float(loss), grads={k: v.grad.numpy() for k, v in pt.items() if v.requires_grad},
                stats={k: v.detach().numpy() for k, v in pt.items() if "running" in k})


def _check_step(name, got, ref):
    """test_avnet_training_step_end_to_end's smooth bounds: forward l2-rel <= 3e-5, loss <= 1e-5, median gradient l2-rel <= 5e-4,
    >= 95 % of the gradient tensors <= 2e-3, the worst <= 2e-2; BatchNorm running statistics 1e-5."""
    close(f"{name} forward", got["out"], ref["out"], tol_l2=3e-5)
    close(f"{name} loss", np.array([got["loss"]]), np.array([ref["loss"]]), tol=1e-5)
    assert set(got["grads"]) == set(ref["grads"])
    gsc = max(float(np.abs(v).max()) for v in ref["grads"].values())
    l2 = {k: l2_rel(g, ref["grads"][k]) for k, g in got["grads"].items() if float(np.abs(ref["grads"][k]).max()) > 1e-7 * gsc}
    worst = sorted(l2.items(), key=lambda kv: -kv[1])[:3]
    med = float(np.median(list(l2.values())))
    print(f"[parity] {name}: {len(l2)} parameter gradients: median l2-rel {med:.3e}, worst {worst}")
    assert med <= 5e-4
    assert np.mean([v <= 2e-3 for v in l2.values()]) >= 0.95 and worst[0][1] <= 2e-2, worst
    assert set(got["stats"]) == set(ref["stats"]) and got["stats"]
    for k in sorted(ref["stats"]):
        close(f"{name} {k}", got["stats"][k], ref["stats"][k], tol=1e-5)


@pytest.fixture(scope="module")
def step_2s_b4():
    """RTFS-Net-4 (SRU cell) in plain .train(), smoothed; 4 mixtures of 2 s; the float64 oracle of one training step, computed once."""
    m = _smooth(_all_train(copy.deepcopy(model(4))))
    wav, emb = make_inputs(B, L, TV, seed=21)
    tgt = rand((B, 1, L), 22) * 0.05
    return dict(model=m, inputs=(wav, emb, tgt), ref=_oracle_step(m, wav, emb, tgt, 4), hip={})


def test_training_step_2s_batch4_vs_float64(step_2s_b4, monkeypatch):
    """The whole step at the benchmarked shape on the row layout (block and mask generator in train mode)."""
    monkeypatch.delenv("RTFS_TRAIN_CF", raising=False)
    got = step_2s_b4["hip"]["rows"] = _hip_step(copy.deepcopy(step_2s_b4["model"]), *step_2s_b4["inputs"])
    _check_step("2 s x 4 step, rows", got, step_2s_b4["ref"])


def test_training_step_2s_batch4_channel_first(step_2s_b4, monkeypatch):
    """The same step on the channel-first layout (RTFS_TRAIN_CF): against the same oracle, and against the row layout."""
    if "rows" not in step_2s_b4["hip"]:
        monkeypatch.delenv("RTFS_TRAIN_CF", raising=False)
        step_2s_b4["hip"]["rows"] = _hip_step(copy.deepcopy(step_2s_b4["model"]), *step_2s_b4["inputs"])
    monkeypatch.setenv("RTFS_TRAIN_CF", "1")
    got = _hip_step(copy.deepcopy(step_2s_b4["model"]), *step_2s_b4["inputs"])
    _check_step("2 s x 4 step, channel-first", got, step_2s_b4["ref"])
    _check_step("2 s x 4 step, channel-first vs rows", got, step_2s_b4["hip"]["rows"])


def test_training_step_batch16_equals_mean_of_four_batch4_steps():
    """Batch 16 (DESIGN.md's other training batch) without a float64 oracle: with BatchNorm frozen and the PIT loss a batch mean, the
    B = 16 gradient is the mean of the gradients of its four B = 4 quarters.  Unsmoothed parameters: the kinked path at size.
    Measured on an MI355X: worst tensor l2-rel 8e-6 .. 1.4e-5 over three runs (a PReLU slope: a scalar sum with cancellation),
    median 2.9e-7; bound 5e-5."""
    m = copy.deepcopy(model(4)).freeze_for_finetune()
    wav, emb = make_inputs(16, L, TV, seed=23)
    tgt = rand((16, 1, L), 24) * 0.05
    loss_mod = _loss_mod()

    def grads(sl):
        for q in m.parameters():
            q.grad = None
        loss_mod(m(dev(wav[sl]), dev(emb[sl])), dev(tgt[sl])).backward()
        return {k: host(v.grad).astype(np.float64) for k, v in m.named_parameters() if v.requires_grad}
    g16 = grads(slice(0, 16))
    quarters = [grads(slice(4 * i, 4 * i + 4)) for i in range(4)]
    mean = {k: sum(q[k] for q in quarters) / 4 for k in g16}
    gmax = max(float(np.abs(v).max()) for v in mean.values())
    # exactly-zero gradients (a bias in front of a norm, a constant in front of a softmax) are rounding noise: not compared
    l2 = {k: l2_rel(g16[k], mean[k]) for k in g16 if float(np.abs(mean[k]).max()) > 1e-6 * gmax}
    worst = sorted(l2.items(), key=lambda kv: -kv[1])[:3]
    print(f"[parity] B = 16 vs mean of 4 x B = 4 over {len(l2)} gradient tensors: median l2-rel {np.median(list(l2.values())):.3e}, worst {worst}")
    assert len(l2) >= 150 and worst[0][1] <= 5e-5, worst


def _attention_sign_pattern(out, Bn, Tn):
    """The TF attention's PReLU sign pattern ("pre-activation >= 0", what mhsa2d_torch's masks take) from the saved state of the one
    attention call in ``out``'s autograd graph (layout as in test_mhsa2d_training_forward_backward)."""
    from rtfs_net_amd import _lib
    n = int(_lib.load().rtfs_tf_attention_saved_floats(Bn, Tn))
    seen, todo, found = set(), [out.grad_fn], []
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        try:
            st = f.saved_tensors
        except (AttributeError, RuntimeError):
            st = ()
        if len(st) > 1 and isinstance(st[1], torch.Tensor) and st[1].numel() == n:
            found.append(st[1])
        todo.extend(g for g, _ in f.next_functions)
    assert len(found) == 1, len(found)
    sv = found[0]
    Rr, Tp = Bn * Tn * 64, (Tn + 63) // 64 * 64
    Z = host(sv[Rr * 64:Rr * 192]).reshape(Bn, Tn, 64, 128).transpose(0, 3, 1, 2)
    off2 = Rr * 192 + Bn * Tn * 32 + 4 * Bn * Tp * (256 + 256 + 1024) + 4 * Bn * Tp * Tp + Rr * 64
    Z2 = host(sv[off2:off2 + Rr * 64]).reshape(Bn, Tn, 64, 64).transpose(0, 3, 1, 2)
    masks, c0 = {}, 0
    for i, m in enumerate([f"Queries.{h}" for h in range(4)] + [f"Keys.{h}" for h in range(4)] + [f"Values.{h}" for h in range(4)]):
        c = 4 if i < 8 else 16
        masks[m] = torch.from_numpy(Z[:, c0:c0 + c] >= 0)
        c0 += c
    masks["attn_concat_proj"] = torch.from_numpy(Z2 >= 0)
    return masks


@pytest.mark.parametrize("cell,layout,seed", [("SRU", "rows", 161), ("SRU", "cf", 161), ("LSTM", "cf", 162)])
def test_block_training_2s(cell, layout, seed, monkeypatch):
    """The RTFS block at (2, 256, 251, 129) with the residual input and its configured PReLU slopes, on both training layouts (the LSTM
    cell has only the channel-first one), against the autograd oracle.  The attention's PReLUs go into the oracle with the kernels' own
    sign pattern, as in test_mhsa2d_training_forward_backward: of its 1.5 M pre-activations at this size one or two land on the other
    side of 0 than in float64 (bf16x3 rounding), and each such element moves the input gradient by ~2e-4 l2-rel (DESIGN.md "parity /
    kinks at 2 s").  A wrong pattern would show in the forward, which the oracle evaluates with it.  Bounds tighter than
    test_block_training_forward_backward's."""
    if layout == "cf":
        monkeypatch.setenv("RTFS_TRAIN_CF", "1")
    else:
        monkeypatch.delenv("RTFS_TRAIN_CF", raising=False)
    if cell == "LSTM":
        lm, lsd = lstm_model()
        p = {k: v.copy() for k, v in O._sub(lsd, "refinement_module.audio_net.blocks").items()}
        blk = copy.deepcopy(lm.refinement_module.audio_net.get_block(0)).train()
    else:
        p = {k: v.copy() for k, v in BLK.items()}
        blk = copy.deepcopy(model().refinement_module.audio_net.get_block(0)).train()
    shape = (2, 256, T, F)
    x, res, dout = rand(shape, seed), rand(shape, seed + 1), rand(shape, seed + 100)
    xt, rt = dev(x).requires_grad_(True), dev(res).requires_grad_(True)
    out = blk(xt, rt)
    masks = _attention_sign_pattern(out, 2, T2)
    out.backward(dev(dout))
    o_ref, dx_ref, g_ref = G.module_grads(lambda a, q: G.rtfs_block_torch(a, q, att_masks=masks), x + res, p, dout)
    close(f"block {cell} {layout} 2 s forward", host(out), o_ref)
    dx_l2 = l2_rel(host(xt.grad), dx_ref)
    print(f"[parity] block {cell} {layout} 2 s dx: max-rel {rel_err(host(xt.grad), dx_ref):.3e} l2-rel {dx_l2:.3e}")
    assert dx_l2 <= 1e-4
    assert torch.equal(rt.grad, xt.grad)
    got = {k: v.grad for k, v in blk.named_parameters()}
    assert set(got) == set(g_ref)
    gscale = {k: float(np.abs(v).max()) for k, v in g_ref.items()}
    l2 = {k: l2_rel(host(got[k]).reshape(g_ref[k].shape), g_ref[k]) for k in g_ref if gscale[k] > 1e-9 * max(gscale.values())}
    worst = sorted(l2.items(), key=lambda kv: -kv[1])[:3]
    print(f"[parity] block {cell} {layout} 2 s, {len(g_ref)} parameter gradients: median l2-rel {np.median(list(l2.values())):.3e}, worst {worst}")
    assert np.median(list(l2.values())) <= 1e-4
    assert worst[0][1] <= 5e-3, worst  # the PReLU slopes' gradients: scalar sums with cancellation


def _away_from_kink(x, pre, step):
    """Move the inputs whose float64 pre-activation ``pre(x)`` lies within 1e-4 of a ReLU kink by ``step`` (as
    test_gateway_one_pass_forward_backward does), so an fp32 pre-activation cannot land on the other side of it."""
    for _ in range(3):
        near = np.abs(pre(x)) < 1e-4
        if not near.any():
            return x
        x = np.where(near, x + step, x).astype(np.float32)
    assert not (np.abs(pre(x)) < 1e-4).any()
    return x


# CNA_CASES names at the size their tensor has in a 2 s x 4 step: (B, C, T, F) of the block input, its stride-2 level, the coarsest level
CNA_2S = {"audio_bn": (B, 256, T, F), "projection": (B, 256, T, F), "gateway": (B, 256, T, F), "downsample": (B, 64, T, F),
          "tfar_gate": (B, 64, T2, F2), "residual_conv": (B, 64, T, F)}


@pytest.mark.parametrize("name", sorted(CNA_2S))
def test_conv_norm_act_training_2s(name):
    """test_conv_norm_act_training_forward_backward's configurations at 2 s x 4 (33 M-element tensors), same bounds: forward 1e-4,
    every gradient 2e-4 max-rel.  Kinks: the gateway's PReLU and the audio bottleneck's pre-activation ReLU have their inputs moved off
    0, the projection's PReLU (slope 0.4, behind its gLN) goes into the oracle with the kernel's own sign pattern."""
    import rtfs_net_amd as R
    kw, _ = TT.CNA_CASES[name]
    shape = CNA_2S[name]
    torch.manual_seed(sum(map(ord, name)))
    mod = R.layers.ConvNormAct(**kw)
    with torch.no_grad():
        for k, v in mod.named_parameters():  # away from the init values, as in the small-shape test
            if "norm" in k or k.endswith("1.weight") or k.endswith("4.weight") or k.endswith("bias"):
                v.add_(0.3 * torch.randn_like(v))
        if name == "projection":  # a positive slope: the output's sign is the pre-activation's (the kernel's sign pattern, below)
            mod.full_layer[4].weight.fill_(0.4)
    p = {k: v.detach().numpy().copy() for k, v in mod.state_dict().items()}
    mod = mod.cuda().train()
    conv = mod.full_layer[2]
    code = R.layers._ACT_CODE
    cfg = (conv.in_channels, conv.out_channels, kw["kernel_size"], kw.get("stride", 1), int(conv.groups > 1),
           int(kw.get("pre_norm_type") == "gLN"), code[type(mod.full_layer[1])], int(kw.get("norm_type") == "gLN"),
           code[type(mod.full_layer[4])], int(conv.bias is not None), int(kw["is2d"]))
    x = rand(shape, 7)
    if kw.get("pre_act_type") == "ReLU":
        g, b = p["full_layer.0.norm.weight"].reshape(1, -1, 1, 1), p["full_layer.0.norm.bias"].reshape(1, -1, 1, 1)

        def pre(v):
            v = torch.from_numpy(v).double()
            return torch.nn.functional.group_norm(v, 1, torch.from_numpy(g.reshape(-1)).double(), torch.from_numpy(b.reshape(-1)).double(),
                                                  1e-5).numpy()
        x = _away_from_kink(x, pre, 0.02 * np.sign(g))
    if name == "gateway":  # depthwise 1x1 + bias, PReLU (slope != 1): pre-activation w_c x + b_c, moved off 0 per element
        w, b = p["full_layer.2.weight"].reshape(1, -1, 1, 1).astype(np.float64), p["full_layer.2.bias"].reshape(1, -1, 1, 1)
        x = _away_from_kink(x, lambda v: w * v + b, 0.02 / w)  # moves w x + b by 0.02 whatever |w|
    xt = dev(x).requires_grad_(True)
    out = mod(xt)
    dout = rand(tuple(out.shape), 8)
    out.backward(dev(dout))
    if name == "projection":  # PReLU behind a gLN: the oracle takes the kernel's sign pattern, as the attention test does
        mask = torch.from_numpy(host(out) >= 0)

        def proj(v, q):
            y = torch.nn.functional.conv2d(v, q["full_layer.2.weight"], q.get("full_layer.2.bias"))
            y = torch.nn.functional.group_norm(y, 1, q["full_layer.3.norm.weight"], q["full_layer.3.norm.bias"], 1e-5)
            return torch.where(mask, y, q["full_layer.4.weight"] * y)
        o_ref, dx_ref, g_ref = G.module_grads(proj, x, p, dout)
    else:
        o_ref, dx_ref, g_ref = G.cna_grads(x, p, cfg, dout)
    close(f"{name} 2 s x 4 forward", host(out), o_ref)
    close(f"{name} 2 s x 4 dx", host(xt.grad), dx_ref, tol=2e-4)
    got = {k: v.grad for k, v in mod.named_parameters()}
    assert set(got) == set(g_ref)
    for k in sorted(g_ref):
        assert got[k] is not None, k
        close(f"{name} 2 s x 4 d {k}", host(got[k]), g_ref[k], tol=2e-4)


def test_batchnorm_train_conv_norm_act_2s():
    """test_sync_batchnorm_two_emulated_ranks' ConvNormAct (depthwise 1x1, BatchNorm2d on batch statistics, ReLU) at (4, 256, 251, 129)
    against float64 torch: output, input gradient, the three parameter gradients and the running statistics (momentum 0.1, unbiased
    variance over 129,516 values per channel).  Inputs with a post-BatchNorm value within 1e-4 of the ReLU kink are moved off it."""
    import torch.nn.functional as Fn
    import rtfs_net_amd as R
    torch.manual_seed(3)
    mod = R.layers.ConvNormAct(in_chan=256, out_chan=256, kernel_size=1, groups=256, norm_type="BatchNorm2d", act_type="ReLU", bias=False,
                               is2d=True)
    with torch.no_grad():
        for v in mod.parameters():
            v.add_(0.3 * torch.randn_like(v))
    p = {k: torch.tensor(v.detach().numpy(), dtype=torch.float64) for k, v in mod.state_dict().items() if "num_batches" not in k}
    w, gam, bet = p["full_layer.2.weight"], p["full_layer.3.weight"], p["full_layer.3.bias"]

    def pre(v):
        y = Fn.conv2d(torch.from_numpy(v).double(), w, groups=256)
        return Fn.batch_norm(y, None, None, gam, bet, True, 0.0, 1e-5).numpy()
    shape = (B, 256, T, F)
    x = _away_from_kink(rand(shape, 1), pre, 0.02 * np.sign((w.reshape(-1) * gam).numpy()).reshape(1, -1, 1, 1))
    dout = rand(shape, 2)
    mod = mod.cuda().train()
    xt = dev(x).requires_grad_(True)
    out = mod(xt)
    out.backward(dev(dout))
    pt = {k: v.clone().requires_grad_("running" not in k) for k, v in p.items()}
    xr = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    y = Fn.conv2d(xr, pt["full_layer.2.weight"], groups=256)
    o_ref = torch.relu(Fn.batch_norm(y, pt["full_layer.3.running_mean"], pt["full_layer.3.running_var"], pt["full_layer.3.weight"],
                                     pt["full_layer.3.bias"], True, 0.1, 1e-5))
    o_ref.backward(torch.tensor(dout, dtype=torch.float64))
    close("bn-train cna 2 s x 4 forward", host(out), o_ref.detach().numpy(), tol=1e-5)
    close("bn-train cna 2 s x 4 dx", host(xt.grad), xr.grad.numpy(), tol=2e-4)
    for k, v in mod.named_parameters():
        close(f"bn-train cna 2 s x 4 d {k}", host(v.grad), pt[k].grad.numpy(), tol=2e-4)
    bn = mod.full_layer[3]
    close("bn-train cna running_mean", host(bn.running_mean), pt["full_layer.3.running_mean"].numpy(), tol=1e-5)
    close("bn-train cna running_var", host(bn.running_var), pt["full_layer.3.running_var"].numpy(), tol=1e-5)
    assert int(bn.num_batches_tracked) == 1


def test_gateway_one_pass_2s():
    """The block's fused gateway (rows, with the residual input) at the 2 s x 4 tensor: test_gateway_one_pass_forward_backward's 1e-5."""
    TT.test_gateway_one_pass_forward_backward((B, T, F, 256), True, 163)


@pytest.mark.parametrize("cell,idx,seed", [("SRU", 0, 164), ("SRU", 1, 165), ("LSTM", 0, 166), ("LSTM", 1, 167)])
def test_dualpath_training_2s(cell, idx, seed):
    """DualPathRNN along F (idx 0) and along T (idx 1) over the full row count of a 2 s x 4 step (4 x 125 x 64 positions):
    test_dualpath_training_forward_backward / test_dualpath_lstm_training_forward_backward at size, same bounds."""
    fn = TT.test_dualpath_training_forward_backward if cell == "SRU" else TT.test_dualpath_lstm_training_forward_backward
    fn(idx, (B, 64, T2, F2), seed)


def test_length_constants_derive_from_the_library():
    """L_MAX / L_OVER and the 2 s pyramid from rtfs_num_frames and the block's stride-2 level (layers.coarsest_sweep)."""
    from rtfs_net_amd import _lib, layers
    lib = _lib.load()
    blk = model(2).refinement_module.audio_net.get_block(0)
    assert int(lib.rtfs_num_frames(L)) == T and layers.coarsest_sweep(T, blk) == T2 and layers.coarsest_sweep(F, blk) == F2
    n = max(n for n in range(2, 4 * layers.TRAIN_MAX_SWEEP) if layers.coarsest_sweep(n, blk) <= layers.TRAIN_MAX_SWEEP)
    assert layers.coarsest_sweep(n, blk) == layers.TRAIN_MAX_SWEEP == 256
    assert int(lib.rtfs_num_frames(L_MAX)) == n and int(lib.rtfs_num_frames(L_OVER)) == n + 1  # L_MAX = 128 n - 1
    assert layers.coarsest_sweep(n + 1, blk) == layers.TRAIN_MAX_SWEEP + 1


def test_training_step_at_the_length_limit_vs_float64():
    """B = 1, R = 2 at L_MAX (513 frames, a 256-position time sweep), everything training, smoothed: test_training_step_2s_batch4's
    bounds against the float64 oracle."""
    m = _smooth(_all_train(copy.deepcopy(model(2))))
    wav, emb = make_inputs(1, L_MAX, 103, seed=25)
    tgt = rand((1, 1, L_MAX), 26) * 0.05
    ref = _oracle_step(m, wav, emb, tgt, 2)
    _check_step("4.1 s x 1 step at the sweep limit", _hip_step(m, wav, emb, tgt), ref)


def test_training_step_past_the_length_limit_refused_before_any_launch():
    """One frame more (L_OVER, a 257-position sweep): forward_train raises ValueError naming the limit before launching anything;
    inference at that length (no gradient) still runs."""
    from rtfs_net_amd import _lib
    lib = _lib.load()
    m = _all_train(copy.deepcopy(model(2)))
    wav, emb = make_inputs(1, L_OVER, 103, seed=27)
    wt, vt = dev(wav), dev(emb)
    torch.cuda.synchronize()
    n0 = lib.rtfs_debug_launch_count()
    with pytest.raises(ValueError, match="TRAIN_MAX_SWEEP = 256"):
        m(wt, vt)
    assert lib.rtfs_debug_launch_count() == n0
    with torch.no_grad():
        out = model(2)(wt, vt)
    assert out.shape == (1, 1, L_OVER) and bool(torch.isfinite(out).all())
