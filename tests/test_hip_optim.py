"""The fused optimizer step (csrc/k_optim.hip, rtfs_net_amd.optimizers.AdamW, System.optimization_step) on the GPU.

Oracle: stock torch on the CPU in float64 (clip_grad_norm_ + torch.optim.AdamW(foreach=False)), never the code under test.
Bound: no tolerance is fixed in advance.  Every comparison also runs stock torch in float32 on the CPU over the same sequence; its
distance d32 to the float64 oracle is the yardstick, and the kernel's distance to the oracle must be at most 4 x d32, separately for
the parameters (max abs), exp_avg (max abs), exp_avg_sq (max relative) and the returned norm (relative).  The factor 4 allows for a
different but equally valid float32 evaluation order (FMA contraction, float64 norm) accumulating over the steps; a wrong bias
correction, decay order or clip constant is off by 1e-3 relative or more."""
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FACTOR = 4.0
LR, WD, CLIP = 1e-3, 0.1, 5.0


def _rtfs4_shapes_and_init():
    import rtfs_net_amd as R
    from rtfs_net_amd.configs import RTFS4_AUDIONET
    torch.manual_seed(0)
    m = R.AVNet(print_macs=False, **copy.deepcopy(RTFS4_AUDIONET))
    init = [p.detach().clone() for p in m.parameters()]
    assert len(init) == 264 and sum(t.numel() for t in init) == 739952
    return init


def _random_grads(shapes, steps, scales, seed, missing=None):
    """steps x tensors float32 CPU gradients scale * randn (None where missing(step, tensor))."""
    g = torch.Generator().manual_seed(seed)
    return [[None if missing and missing(s, i) else scales[s % len(scales)] * torch.randn(sh, generator=g) for i, sh in enumerate(shapes)]
            for s in range(steps)]


def _groups(params, groups):
    if groups is None:
        return [{"params": list(params), "lr": LR, "weight_decay": WD}]
    return [{"params": [params[i] for i in g["idx"]], "lr": g["lr"], "weight_decay": g["weight_decay"]} for g in groups]


def _state_of(opt, params):
    m = [opt.state[p]["exp_avg"].detach().double().cpu() if "exp_avg" in opt.state.get(p, {}) else torch.zeros_like(p, dtype=torch.float64, device="cpu")
         for p in params]
    v = [opt.state[p]["exp_avg_sq"].detach().double().cpu() if "exp_avg_sq" in opt.state.get(p, {}) else torch.zeros_like(p, dtype=torch.float64, device="cpu")
         for p in params]
    return m, v


def run_stock(init, grads_seq, dtype, groups=None, max_norm=CLIP, lr_mult=None, state_dict=None, opt_out=None):
    """clip_grad_norm_ + torch.optim.AdamW(foreach=False) on the CPU in `dtype` -> (params, exp_avg, exp_avg_sq, norms) as float64."""
    params = [torch.nn.Parameter(t.detach().cpu().to(dtype).clone()) for t in init]  # (a copy: .to() of the same dtype aliases)
    gs = _groups(params, groups)
    opt = torch.optim.AdamW(gs, foreach=False)
    if state_dict is not None:
        opt.load_state_dict(state_dict)
    base = [g["lr"] for g in opt.param_groups]
    norms = []
    for s, grads in enumerate(grads_seq):
        for p, g in zip(params, grads):
            p.grad = None if g is None else g.detach().cpu().to(dtype).clone()
        for g, b in zip(opt.param_groups, base):
            g["lr"] = b * (lr_mult[s] if lr_mult else 1.0)
        with_grad = [p for p in params if p.grad is not None]
        if max_norm:
            norms.append(float(torch.nn.utils.clip_grad_norm_(with_grad, max_norm, foreach=False)))
        else:
            norms.append(float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in with_grad]))))
        opt.step()
    if opt_out is not None:
        opt_out.append(opt)
    m, v = _state_of(opt, params)
    return [p.detach().double() for p in params], m, v, norms


def run_fused(init, grads_seq, groups=None, max_norm=CLIP, lr_mult=None, state_dict=None, opt_out=None, params_out=None):
    from rtfs_net_amd import optimizers as O
    params = [torch.nn.Parameter(t.detach().to(torch.float32).clone().cuda()) for t in init]
    opt = O.AdamW(_groups(params, groups))
    if state_dict is not None:
        opt.load_state_dict(state_dict)
    base = [g["lr"] for g in opt.param_groups]
    norms = []
    for s, grads in enumerate(grads_seq):
        for p, g in zip(params, grads):
            p.grad = None if g is None else g.cuda()
        for g, b in zip(opt.param_groups, base):
            g["lr"] = b * (lr_mult[s] if lr_mult else 1.0)
        norms.append(opt.step(max_norm=max_norm).clone())
    torch.cuda.synchronize()
    if opt_out is not None:
        opt_out.append(opt)
    if params_out is not None:
        params_out.extend(params)
    m, v = _state_of(opt, params)
    return [p.detach().double().cpu() for p in params], m, v, [float(n) for n in norms]


def distances(got, ref):
    """(max |dp|, max |d exp_avg|, max relative d exp_avg_sq, max relative d norm) of one run against the float64 oracle."""
    dp = max(float((a - b).abs().max()) for a, b in zip(got[0], ref[0]))
    dm = max(float((a - b).abs().max()) for a, b in zip(got[1], ref[1]))
    dv = max(float(((a - b).abs() / b.abs().clamp_min(1e-30)).max()) for a, b in zip(got[2], ref[2]))
    dn = max(abs(a - b) / max(abs(b), 1e-30) for a, b in zip(got[3], ref[3]))
    return dp, dm, dv, dn


def check_against_oracle(what, fused, f64, f32):
    d32, dk = distances(f32, f64), distances(fused, f64)
    names = ("params max|d|", "exp_avg max|d|", "exp_avg_sq max rel", "norm rel")
    ratios = [k / y if y > 0 else (0.0 if k == 0 else float("inf")) for k, y in zip(dk, d32)]
    print(f"[optim] {what}: " + "; ".join(f"{n}: kernel {k:.3e}, d32 {y:.3e}, ratio {r:.2f}" for n, k, y, r in zip(names, dk, d32, ratios)))
    for n, k, y in zip(names, dk, d32):
        assert k <= FACTOR * y, f"{what}: {n}: kernel {k:.3e} > {FACTOR} x d32 ({y:.3e})"


@pytest.fixture(scope="module")
def rtfs4():
    init = _rtfs4_shapes_and_init()
    grads = _random_grads([t.shape for t in init], 20, (10.0, 1e-3), seed=1)
    return init, grads


def test_parity_over_20_steps_on_the_rtfs4_parameter_set(rtfs4):
    """Measured on one MI355X (20 steps, lr 1e-3, wd 0.1, max_norm 5): the printed ratios are recorded in DESIGN.md, "Optimizer step"."""
    init, grads = rtfs4
    f64 = run_stock(init, grads, torch.float64)
    assert any(n > CLIP for n in f64[3]) and any(n < CLIP for n in f64[3]), f64[3]  # both sides of the clamp are taken
    f32 = run_stock(init, grads, torch.float32)
    fused = run_fused(init, grads)
    check_against_oracle("20 steps, RTFS-Net-4 shapes", fused, f64, f32)


def test_determinism_of_the_20_step_run(rtfs4):
    init, grads = rtfs4
    a, b = run_fused(init, grads), run_fused(init, grads)
    for k in range(3):
        assert all(torch.equal(x, y) for x, y in zip(a[k], b[k])), ("params", "exp_avg", "exp_avg_sq")[k]
    assert a[3] == b[3]


@pytest.mark.parametrize("order", ["stock_then_fused", "fused_then_stock"])
def test_checkpoint_interchange_on_the_device(rtfs4, order):
    """5 steps of one implementation on the GPU, state_dict() into the other, 5 more: against 10 oracle steps, same bound."""
    from rtfs_net_amd import optimizers as O
    init, grads = rtfs4
    f64, f32 = run_stock(init, grads[:10], torch.float64), run_stock(init, grads[:10], torch.float32)
    params = [torch.nn.Parameter(t.cuda()) for t in init]
    make = {"stock": lambda: torch.optim.AdamW(params, lr=LR, weight_decay=WD), "fused": lambda: O.AdamW(params, lr=LR, weight_decay=WD)}
    first, second = order.split("_then_")
    norms = []

    def steps(opt, seq):
        for gr in seq:
            for p, g in zip(params, gr):
                p.grad = g.cuda()
            if isinstance(opt, O.AdamW):
                norms.append(float(opt.step(max_norm=CLIP)))
            else:
                norms.append(float(torch.nn.utils.clip_grad_norm_(params, CLIP)))
                opt.step()
    a = make[first]()
    steps(a, grads[:5])
    b = make[second]()
    b.load_state_dict(a.state_dict())
    steps(b, grads[5:10])
    torch.cuda.synchronize()
    assert all(float(b.state[p]["step"]) == 10.0 for p in params)
    m, v = _state_of(b, params)
    check_against_oracle(order, ([p.detach().double().cpu() for p in params], m, v, norms), f64, f32)


def _small_shapes():
    return [(64, 33), (), (5000,), (7,), (3, 4097), (1,)]


def _small_init(seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) for s in _small_shapes()]


def test_missing_gradients_are_skipped_as_torch_skips_them():
    """Tensor 2 (and the scalar, tensor 1) have .grad = None on odd steps: parameter, moments and step count do not move on those steps,
    bit for bit, and the norm excludes them."""
    from rtfs_net_amd import optimizers as O
    init = _small_init()
    miss = lambda s, i: s % 2 == 1 and i in (1, 2)  # noqa: E731
    grads = _random_grads(_small_shapes(), 6, (3.0, 1e-2), seed=4, missing=miss)
    f64, f32 = run_stock(init, grads, torch.float64), run_stock(init, grads, torch.float32)
    opts, params = [], []
    fused = run_fused(init, grads, opt_out=opts, params_out=params)
    check_against_oracle("missing gradients", fused, f64, f32)
    assert [int(opts[0].state[p]["step"]) for p in params] == [6, 3, 3, 6, 6, 6] == opts[0]._steps
    # one more step without those gradients: bit-identical parameter and moments
    before = [(params[i].detach().clone(), opts[0].state[params[i]]["exp_avg"].clone(), opts[0].state[params[i]]["exp_avg_sq"].clone()) for i in (1, 2)]
    vers = [params[i]._version for i in (1, 2)]
    for i, p in enumerate(params):
        p.grad = None if i in (1, 2) else torch.ones_like(p)
    norm = float(opts[0].step(max_norm=CLIP))
    expect = float(np.sqrt(sum(p.numel() for i, p in enumerate(params) if i not in (1, 2))))
    assert abs(norm - expect) <= 1e-6 * expect
    for (p0, m0, v0), i, ver in zip(before, (1, 2), vers):
        st = opts[0].state[params[i]]
        assert torch.equal(p0, params[i]) and torch.equal(m0, st["exp_avg"]) and torch.equal(v0, st["exp_avg_sq"]) and int(st["step"]) == 3
        assert params[i]._version == ver
    assert isinstance(opts[0], O.AdamW)


def test_parameter_groups_and_lr_read_every_step():
    init = _small_init()
    groups = [{"idx": [0, 1, 2], "lr": 1e-3, "weight_decay": 0.1}, {"idx": [3, 4, 5], "lr": 5e-3, "weight_decay": 0.0}]
    grads = _random_grads(_small_shapes(), 6, (3.0, 1e-2), seed=5)
    order = [i for g in groups for i in g["idx"]]
    assert order == list(range(6))
    lr_mult = [1.0, 1.0, 0.5, 0.5, 0.25, 0.25]  # halved between steps, as ReduceLROnPlateau would
    kw = dict(groups=groups, lr_mult=lr_mult)
    f64, f32 = run_stock(init, grads, torch.float64, **kw), run_stock(init, grads, torch.float32, **kw)
    check_against_oracle("two groups, lr halved", run_fused(init, grads, **kw), f64, f32)


def test_without_max_norm_nothing_is_clipped():
    init = _small_init()
    grads = _random_grads(_small_shapes(), 4, (3.0,), seed=6)
    f64, f32 = run_stock(init, grads, torch.float64, max_norm=None), run_stock(init, grads, torch.float32, max_norm=None)
    assert min(f64[3]) > CLIP  # a clip at 5 would have changed every step
    check_against_oracle("max_norm=None", run_fused(init, grads, max_norm=None), f64, f32)
    clipped = run_stock(init, grads, torch.float64)
    assert distances(clipped, f64)[1] > 1e-2  # ... and the comparison above would have seen it (Adam's step hardly depends on the scale, exp_avg does)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_gradient_gives_torchs_pattern(bad):
    """clip_grad_norm_ does not raise by default (error_if_nonfinite=False): the parameters take the same finite / NaN pattern as in
    stock float32 torch (inf: norm inf, coefficient 0, 0 * inf = NaN in that one element; NaN: everything)."""
    init = _small_init()
    grads = _random_grads(_small_shapes(), 1, (1.0,), seed=7)
    grads[0][2][17] = bad
    f32 = run_stock(init, grads, torch.float32)
    fused = run_fused(init, grads)
    for a, b in zip(fused[0], f32[0]):
        assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.isinf(a), torch.isinf(b))
        ok = torch.isfinite(b)
        assert float((a[ok] - b[ok]).abs().max() if ok.any() else 0.0) <= 1e-6
    n_nan = sum(int(torch.isnan(a).sum()) for a in fused[0])
    assert n_nan == (1 if bad == float("inf") else sum(t.numel() for t in init))
    assert (np.isinf(fused[3][0]) and np.isinf(f32[3][0])) or (np.isnan(fused[3][0]) and np.isnan(f32[3][0]))


# ---------------------------------------------------------------- through System.optimization_step
def _small_system(fused=True, seed=0):
    import rtfs_net_amd as R
    from rtfs_net_amd.configs import RTFS4_AUDIONET
    from oracle.params import make_inputs
    conf = copy.deepcopy(RTFS4_AUDIONET)
    conf["audio_params"]["repeats"] = 2
    torch.manual_seed(seed)
    m = R.AVNet(print_macs=False, **conf).cuda().train()
    ga = m.refinement_module.video_net.get_block(0).globalatt[0]
    ga.MHSA.dropout, ga.MHSA.dropout_layer.p, ga.FFN.dropout = 0.0, 0.0, 0.0  # no RNG in the comparison
    loss_mod = R.losses.PITLossWrapper(R.losses.PairwiseNegSDR("snr"), pit_from="pw_mtx")
    params = [p for p in m.parameters() if p.requires_grad]
    opt = R.make_optimizer(params, optimizer="adamw", lr=LR, weight_decay=WD) if fused else torch.optim.AdamW(params, lr=LR, weight_decay=WD)
    system = R.System(audio_model=m, optimizer=opt, loss_func={"train": loss_mod, "val": loss_mod})
    wav, emb = make_inputs(2, 4096, 7, seed=5)  # the shape of grad_R2_L4096_B2
    tgt = 0.05 * np.random.default_rng(6).standard_normal((2, 1, 4096)).astype(np.float32)
    batch = (torch.from_numpy(wav).cuda(), torch.from_numpy(tgt).cuda(), torch.from_numpy(emb).cuda(), None)
    return system, m, conf, batch


def test_fused_step_bumps_versions_and_the_next_forward_sees_the_new_weights():
    import rtfs_net_amd as R
    from rtfs_net_amd import optimizers as O
    from tests.util import rel_err
    system, m, conf, batch = _small_system()
    assert isinstance(system.optimizer, O.AdamW)
    params = system.trainable_parameters()
    vers = [p._version for p in params]
    loss1 = float(system.optimization_step(batch))
    assert all(p._version > v for p, v in zip(params, vers))
    assert system.last_grad_norm.is_cuda and system.last_grad_norm.ndim == 0 and np.isfinite(float(system.last_grad_norm))
    loss2 = float(system.optimization_step(batch))
    assert loss2 != loss1 and abs(loss2 - loss1) > 1e-6 * abs(loss1), (loss1, loss2)  # the second step ran on updated packs
    fresh = R.AVNet(print_macs=False, **conf)
    fresh.load_state_dict(m.state_dict())
    fresh = fresh.cuda().eval()
    m.eval()
    with torch.no_grad():
        got, ref = m(batch[0], batch[2]), fresh(batch[0], batch[2])
    err = rel_err(got.cpu().numpy(), ref.cpu().numpy())
    print(f"[optim] eval after two fused steps vs a fresh model with the same state_dict: rel err {err:.3e}")
    assert err <= 1e-4


def test_whole_fused_step_against_the_oracle():
    """One fused optimization_step; p.grad afterwards holds the raw gradients (the fused route does not scale or clip them in place);
    the float64 oracle fed with them from the saved initial parameters gives the expected parameters."""
    system, m, conf, batch = _small_system()
    params = system.trainable_parameters()
    init = [p.detach().clone().cpu() for p in params]
    system.optimization_step(batch)
    torch.cuda.synchronize()
    grads = [[None if p.grad is None else p.grad.detach().cpu() for p in params]]
    assert sum(g is not None for g in grads[0]) == len(params)
    f64, f32 = run_stock(init, grads, torch.float64), run_stock(init, grads, torch.float32)
    mom = _state_of(system.optimizer, params)
    fused = ([p.detach().double().cpu() for p in params], mom[0], mom[1], [float(system.last_grad_norm)])
    check_against_oracle("System.optimization_step, one step", fused, f64, f32)
    assert distances((init, f64[1], f64[2], f64[3]), f64)[0] > 1e-4  # the step moved the parameters by about lr


DDP_WORKER = r"""
import os, sys, copy
import numpy as np, torch
import torch.distributed as dist
sys.path.insert(0, os.environ["RTFS_ROOT"])
import rtfs_net_amd as R
from rtfs_net_amd.configs import RTFS4_AUDIONET
from oracle.params import make_inputs
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)   # two ranks share the one GPU of the box: gloo moves the CUDA tensors
conf = copy.deepcopy(RTFS4_AUDIONET); conf["audio_params"]["repeats"] = 2
torch.manual_seed(0)
m = R.AVNet(print_macs=False, **conf).cuda().train()
ga = m.refinement_module.video_net.get_block(0).globalatt[0]
ga.MHSA.dropout, ga.MHSA.dropout_layer.p, ga.FFN.dropout = 0.0, 0.0, 0.0
loss_mod = R.losses.PITLossWrapper(R.losses.PairwiseNegSDR("snr"), pit_from="pw_mtx")
params = [p for p in m.parameters() if p.requires_grad]
opt = R.make_optimizer(params, optimizer="adamw", lr=1e-3, weight_decay=0.1)
system = R.System(audio_model=m, optimizer=opt, loss_func={"train": loss_mod, "val": loss_mod})
system.broadcast_parameters()
init = [p.detach().cpu().numpy().copy() for p in params]
B = 4
wav, emb = make_inputs(B, 4096, 7, seed=5)
tgt = 0.05 * np.random.default_rng(6).standard_normal((B, 1, 4096)).astype(np.float32)
sl = slice(rank * B // world, (rank + 1) * B // world)            # a different batch on every rank
batch = (torch.from_numpy(wav[sl]).cuda(), torch.from_numpy(tgt[sl]).cuda(), torch.from_numpy(emb[sl]).cuda(), None)
count = [0]
real = dist.all_reduce
def counting(*a, **k):
    count[0] += 1
    return real(*a, **k)
dist.all_reduce = counting
system.optimization_step(batch)
dist.all_reduce = real
torch.cuda.synchronize()
out = {"n_allreduce": count[0], "norm": float(system.last_grad_norm)}
for i, p in enumerate(params):
    out[f"init{i}"] = init[i]
    out[f"p{i}"] = p.detach().cpu().numpy()
    out[f"g{i}"] = p.grad.detach().cpu().numpy()
    out[f"m{i}"] = opt.state[p]["exp_avg"].cpu().numpy()
    out[f"v{i}"] = opt.state[p]["exp_avg_sq"].cpu().numpy()
np.savez(os.environ["RTFS_OUT"] + f".{rank}.npz", **out)
dist.barrier(); dist.destroy_process_group()
"""


def test_two_ranks_one_allreduce_bit_identical_parameters(tmp_path):
    """Two processes (gloo, sharing the box's one GPU), a different batch each: one all_reduce in the step, parameters bit-identical
    across ranks and equal, within the bound, to the oracle fed with the mean of the two ranks' raw gradients."""
    import socket
    import subprocess
    import sys
    from tests.util import ROOT
    s_ = socket.socket(); s_.bind(("127.0.0.1", 0)); port = s_.getsockname()[1]; s_.close()
    out = str(tmp_path / "ddp")
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RTFS_ROOT=ROOT,
                   RTFS_OUT=out, HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, "-c", DDP_WORKER], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    for p_ in procs:
        o_, e_ = p_.communicate(timeout=600)
        assert p_.returncode == 0, e_[-3000:]
    r0, r1 = dict(np.load(out + ".0.npz")), dict(np.load(out + ".1.npz"))
    assert int(r0["n_allreduce"]) == 1 and int(r1["n_allreduce"]) == 1
    n = sum(1 for k in r0 if k.startswith("init"))
    assert n == 264
    for i in range(n):
        assert np.array_equal(r0[f"init{i}"], r1[f"init{i}"])
        assert np.array_equal(r0[f"p{i}"], r1[f"p{i}"]) and np.array_equal(r0[f"m{i}"], r1[f"m{i}"]) and np.array_equal(r0[f"v{i}"], r1[f"v{i}"]), i
    assert float(r0["norm"]) == float(r1["norm"])
    assert any(not np.array_equal(r0[f"g{i}"], r1[f"g{i}"]) for i in range(n))  # p.grad stays local: the batches differ
    init = [torch.from_numpy(r0[f"init{i}"]) for i in range(n)]
    mean = [[(torch.from_numpy(r0[f"g{i}"]).double() + torch.from_numpy(r1[f"g{i}"]).double()) / 2 for i in range(n)]]
    f64, f32 = run_stock(init, mean, torch.float64), run_stock(init, mean, torch.float32)
    fused = ([torch.from_numpy(r0[f"p{i}"]).double() for i in range(n)], [torch.from_numpy(r0[f"m{i}"]).double() for i in range(n)],
             [torch.from_numpy(r0[f"v{i}"]).double() for i in range(n)], [float(r0["norm"])])
    check_against_oracle("two ranks, one step", fused, f64, f32)
