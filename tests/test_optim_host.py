"""Host-side checks of rtfs_net_amd.optimizers (no GPU): the registry, the constructor's refusals, checkpoint interchange with
torch.optim.AdamW, the chunk plan of the C ABI, and that System.optimization_step keeps the stock route for every other optimizer."""
import ctypes as C

import pytest
import torch

import rtfs_net_amd as R
from rtfs_net_amd import _lib, optimizers as O


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((5, 3), (), (9000,), (7,))]


def test_registry_names_and_errors():
    assert O.get("AdamW") is O.AdamW and O.get("adamw") is O.AdamW and issubclass(O.AdamW, torch.optim.Optimizer)
    assert O.get("sgd") is torch.optim.SGD and O.get("Adam") is torch.optim.Adam and O.get("RMSprop") is torch.optim.RMSprop
    inst = torch.optim.SGD(_params(), lr=0.1)
    assert O.get(inst) is inst and O.make_optimizer(None, optimizer=inst) is inst
    for bad in ("nope", "optimizer", "make_optimizer", 3, None):
        with pytest.raises(ValueError, match="Could not interpret optimizer"):
            O.get(bad)
    with pytest.raises(ValueError, match="Could not interpret optimizer : ranger.*torch_optimizer"):
        O.get("ranger")
    opt = O.make_optimizer(_params(), optimizer="adamw", lr=3e-4, weight_decay=0.1)
    assert isinstance(opt, O.AdamW) and opt.param_groups[0]["lr"] == 3e-4 and opt.param_groups[0]["weight_decay"] == 0.1
    assert isinstance(O.make_optimizer(_params(), optimizer="sgd", lr=0.5), torch.optim.SGD)
    assert R.make_optimizer is O.make_optimizer and R.optimizers is O


def test_register_optimizer():
    class MyOpt(torch.optim.SGD):
        pass
    try:
        O.register_optimizer(MyOpt)
        assert O.get("myopt") is MyOpt
        with pytest.raises(ValueError, match="already exists"):
            O.register_optimizer(MyOpt)
    finally:
        vars(O).pop("MyOpt", None)

    class adamw(torch.optim.SGD):  # noqa: N801  (a name that differs only in case is taken too)
        pass
    with pytest.raises(ValueError, match="already exists"):
        O.register_optimizer(adamw)


@pytest.mark.parametrize("kw", [dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(differentiable=True)])
def test_constructor_refuses_what_the_kernel_does_not_do(kw):
    with pytest.raises(ValueError, match="MI355X AdamW supports"):
        O.AdamW(_params(), **kw)


def test_constructor_refuses_bad_parameters():
    with pytest.raises(ValueError, match="MI355X AdamW supports"):
        O.AdamW([torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))])
    with pytest.raises(ValueError, match="at most"):
        O.AdamW([torch.nn.Parameter(torch.zeros(1)) for _ in range(O.MAX_TENSORS + 1)])
    with pytest.raises(ValueError, match="invalid hyper-parameters"):
        O.AdamW(_params(), lr=-1.0)
    opt = O.AdamW(_params())
    with pytest.raises(NotImplementedError, match="MI355X AdamW supports"):
        opt.add_param_group({"params": _params(1)})


def test_step_on_cpu_parameters_raises_no_fallback():
    ps = _params()
    opt = O.AdamW(ps)
    for p in ps:
        p.grad = torch.ones_like(p)
    before = [p.detach().clone() for p in ps]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.gather_grads()
    assert all(torch.equal(a, p) for a, p in zip(before, ps))


def test_state_dict_interchange_with_torch_adamw():
    ps = _params()
    fused = O.AdamW([{"params": ps[:2], "lr": 2e-3}, {"params": ps[2:], "weight_decay": 0.3}], lr=1e-3, weight_decay=0.1)
    stock = torch.optim.AdamW([{"params": ps[:2], "lr": 2e-3}, {"params": ps[2:], "weight_decay": 0.3}], lr=1e-3, weight_decay=0.1)
    fsd, ssd = fused.state_dict(), stock.state_dict()
    assert [set(g) for g in fsd["param_groups"]] == [set(g) for g in ssd["param_groups"]]
    assert fsd["param_groups"] == ssd["param_groups"]
    # fresh fused -> stock: zero moments, step 0; a stock step from there equals a stock step from nothing
    stock.load_state_dict(fsd)
    for p in ps:
        p.grad = torch.full_like(p, 0.5)
    ref = [p.detach().clone() for p in ps]
    stock.step()
    fresh_ps = [torch.nn.Parameter(r.clone()) for r in ref]
    fresh = torch.optim.AdamW([{"params": fresh_ps[:2], "lr": 2e-3}, {"params": fresh_ps[2:], "weight_decay": 0.3}], lr=1e-3, weight_decay=0.1)
    for p in fresh_ps:
        p.grad = torch.full_like(p, 0.5)
    fresh.step()
    assert all(torch.equal(a, b) for a, b in zip(ps, fresh_ps))
    # stepped stock -> fused: values land IN the flat buffers, the views keep aliasing them, the step counts follow
    stock.param_groups[0]["lr"] = 7e-4
    fused.load_state_dict(stock.state_dict())
    assert fused.param_groups[0]["lr"] == 7e-4 and fused._steps == [1] * len(ps)
    for p, off in zip(ps, fused._offsets):
        st = fused.state[p]
        assert float(st["step"]) == 1.0 and st["exp_avg"].shape == p.shape
        for key, flat in (("exp_avg", fused._exp_avg), ("exp_avg_sq", fused._exp_avg_sq)):
            assert st[key].untyped_storage().data_ptr() == flat.untyped_storage().data_ptr()
            assert torch.equal(st[key], stock.state[p][key]) and float(st[key].abs().sum()) > 0
            assert torch.equal(flat[off:off + p.numel()], stock.state[p][key].reshape(-1))
    # ... and back: the fused optimizer's state_dict is one torch.optim.AdamW continues from
    back = torch.optim.AdamW([{"params": ps[:2]}, {"params": ps[2:]}])
    back.load_state_dict(fused.state_dict())
    assert back.param_groups[0]["lr"] == 7e-4 and back.param_groups[1]["weight_decay"] == 0.3
    for p in ps:
        assert float(back.state[p]["step"]) == 1.0 and torch.equal(back.state[p]["exp_avg_sq"], stock.state[p]["exp_avg_sq"])
    back.step()
    stock.step()
    assert all(float(back.state[p]["step"]) == 2.0 for p in ps)
    # a stock checkpoint in which one parameter never had a gradient: that slice restarts from zero
    half = torch.optim.AdamW([{"params": ps[:2]}, {"params": ps[2:]}])
    for p in ps[1:]:
        p.grad = torch.ones_like(p)
    ps[0].grad = None
    half.step()
    fused.load_state_dict(half.state_dict())
    assert fused._steps == [0, 1, 1, 1] and float(fused.state[ps[0]]["exp_avg"].abs().sum()) == 0.0
    with pytest.raises(ValueError, match="MI355X AdamW supports"):
        sd = half.state_dict()
        sd["param_groups"][0]["amsgrad"] = True
        fused.load_state_dict(sd)


def test_chunk_plan_of_the_c_abi():
    lib = _lib.load()
    numel = [15, 1, 9000, 4096, 4097]
    arr = (C.c_longlong * len(numel))(*numel)
    flat, nc = C.c_longlong(0), C.c_int(0)
    assert lib.rtfs_optim_plan(arr, len(numel), None, C.byref(flat), C.byref(nc)) == 0
    assert nc.value == 1 + 1 + 3 + 1 + 2 and flat.value == 16 + 4 + 9000 + 4096 + 4100
    table = (C.c_longlong * (2 * len(numel) + 2 * nc.value))()
    assert lib.rtfs_optim_plan(arr, len(numel), table, None, None) == 0
    T = len(numel)
    assert list(table[:T]) == [0, 16, 20, 9020, 13116] and list(table[T:2 * T]) == numel
    assert list(table[2 * T:2 * T + nc.value]) == [0, 1, 2, 2, 2, 3, 4, 4]
    assert list(table[2 * T + nc.value:]) == [0, 0, 0, 4096, 8192, 0, 0, 4096]
    assert lib.rtfs_optim_plan(arr, O.MAX_TENSORS + 1, None, None, None) == -4
    assert lib.rtfs_optim_plan((C.c_longlong * 1)(0), 1, None, None, None) == -1
    # argument checks come before any launch (no device is touched): misaligned flat buffer, too many tensors, bad hyper index
    ptrs = (C.c_void_p * T)()
    assert lib.rtfs_optim_gather_f32(ptrs, C.c_void_p(4096), T, nc.value, C.c_void_p(4100), None, 0, None) == -4
    assert lib.rtfs_optim_gather_f32(ptrs, C.c_void_p(4096), O.MAX_TENSORS + 1, 400, C.c_void_p(4096), None, 0, None) == -4
    assert lib.rtfs_optim_sumsq_f32(C.c_void_p(4096), T, nc.value, C.c_void_p(4104), C.c_void_p(4096), None) == -4
    idx = (C.c_ubyte * T)(*[3] * T)
    hy = (C.c_float * 8)()
    pp = (C.c_void_p * T)(*[4096] * T)
    a = C.c_void_p(4096)
    assert lib.rtfs_optim_adamw_f32(pp, idx, hy, 1, a, T, nc.value, a, a, a, a, 5.0, 1.0, None, None) == -4
    assert lib.rtfs_optim_adamw_f32(pp, idx, hy, O.MAX_HYPER + 1, a, T, nc.value, a, a, a, a, 5.0, 1.0, None, None) == -4


def test_optimization_step_keeps_the_stock_route_for_other_optimizers(monkeypatch):
    calls = []

    class Stub(torch.optim.Optimizer):
        def __init__(self, params):
            super().__init__(params, {})

        def step(self, closure=None):
            calls.append("step")

    w = torch.nn.Parameter(torch.ones(4))

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = w

    system = R.System(audio_model=Model(), optimizer=Stub([w]))
    system.training_step = lambda batch, nb: {"loss": (system.audio_model.w * batch).sum()}
    real_clip = torch.nn.utils.clip_grad_norm_

    def clip(params, max_norm, *a, **k):
        calls.append(("clip", len(list(params)), max_norm))
        return real_clip([w], max_norm, *a, **k)
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", clip)
    loss = system.optimization_step(torch.full((4,), 10.0))
    assert float(loss) == 40.0 and calls == [("clip", 1, 5.0), "step"]
    assert abs(float(w.grad.norm()) - 5.0) < 1e-4  # the stock route leaves the clipped gradient in p.grad
    assert not hasattr(system, "last_grad_norm")
