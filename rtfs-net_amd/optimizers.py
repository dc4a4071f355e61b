"""Mirror of the reference's ``src/system/optimizers.py`` (``make_optimizer`` / ``get`` / ``register_optimizer``, :58-108) with one
difference: ``"adamw"`` is the MI355X ``AdamW`` below, whose step (gradient gather, ``clip_grad_norm_``, the AdamW update) runs as two
HIP launches (csrc/k_optim.hip) instead of stock torch's per-tensor / ``_foreach`` chains.  Every other name the reference lists that
stock torch has maps to the ``torch.optim`` class; the ``torch_optimizer`` package is not a dependency, so its names are refused.

``AdamW`` keeps ``torch.optim.AdamW``'s keywords, ``param_groups`` and ``state_dict()`` format (checkpoints go both ways), but its
moments live in two flat device buffers (``state[p]["exp_avg"]`` / ``["exp_avg_sq"]`` are views into them) next to one flat gradient
buffer that a data-parallel caller all-reduces in place between ``gather_grads()`` and ``step()`` (``System.optimization_step``).
The update is not replayable inside a captured graph: the step count and the bias corrections are host values.
"""
from __future__ import annotations

import ctypes as C

import torch
from torch.optim import ASGD, SGD, Adadelta, Adagrad, Adam, Adamax, RMSprop  # noqa: F401  (the registry is this module's globals)
from torch.optim.optimizer import Optimizer

from . import _lib

__all__ = ["Adam", "RMSprop", "SGD", "Adadelta", "Adagrad", "Adamax", "AdamW", "ASGD", "make_optimizer", "get", "register_optimizer"]

# names the reference imports from the torch_optimizer package (optimizers.py:10-26), which is not a dependency here
_TORCH_OPTIMIZER_NAMES = ("accsgd", "adabound", "adamod", "diffgrad", "lamb", "novograd", "pid", "qhadam", "qhm", "radam", "sgdw", "yogi",
                          "ranger", "rangerqh", "rangerva")
MAX_TENSORS, MAX_HYPER, _SKIP = 320, 16, 255  # include/rtfs_amd.h: RTFS_OPTIM_MAX_TENSORS, RTFS_OPTIM_MAX_HYPER; hyper_index of a skipped tensor


class AdamW(Optimizer):
    """``torch.optim.AdamW`` whose step is two kernel launches for any number of parameter tensors (up to MAX_TENSORS): one gathers the
    gradients into a flat buffer and leaves per-chunk sums of squares, one finishes the global norm, clips (``max_norm``), decays and
    updates parameters and moments in place.  Same arithmetic as ``clip_grad_norm_`` + ``torch.optim.AdamW``; deterministic (no atomics);
    nothing is read back and nothing is allocated per step.  float32 CUDA parameters; the first ``step`` on CPU parameters raises (there
    is no CPU fallback).  ``foreach`` and ``fused`` are accepted for signature compatibility and have no effect."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False, foreach=None,
                 capturable=False, differentiable=False, fused=None):
        for name, val in (("amsgrad", amsgrad), ("maximize", maximize), ("capturable", capturable), ("differentiable", differentiable)):
            if val:
                raise ValueError(f"MI355X AdamW supports {name}=False only (got {val!r}); use torch.optim.AdamW for it")
        if isinstance(lr, torch.Tensor):
            raise ValueError("MI355X AdamW supports a float lr only (the bias corrections are host values)")
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= weight_decay or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError(f"MI355X AdamW: invalid hyper-parameters lr={lr} betas={betas} eps={eps} weight_decay={weight_decay}")
        self._built = False
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=foreach,
                                      capturable=False, differentiable=False, fused=fused, decoupled_weight_decay=True))
        self._build()

    # ------------------------------------------------------------------ layout
    def _build(self):
        ps = [p for g in self.param_groups for p in g["params"]]
        if len(ps) > MAX_TENSORS:
            raise ValueError(f"MI355X AdamW supports at most {MAX_TENSORS} parameter tensors (got {len(ps)}): the pointer tables travel "
                             "in the kernel arguments")
        for p in ps:
            if p.dtype != torch.float32 or p.device != ps[0].device or p.is_sparse or p.numel() == 0:
                raise ValueError("MI355X AdamW supports non-empty dense float32 parameters on one device")
        self._params = ps
        self._group_of = [gi for gi, g in enumerate(self.param_groups) for _ in g["params"]]
        lib = _lib.load()
        T = len(ps)
        numel = (C.c_longlong * T)(*[p.numel() for p in ps])
        flat, nc = C.c_longlong(0), C.c_int(0)
        _lib.check(lib.rtfs_optim_plan(numel, T, None, C.byref(flat), C.byref(nc)), "rtfs_optim_plan")
        self._n_chunks, self._flat_floats = nc.value, flat.value
        table = (C.c_longlong * (2 * T + 2 * nc.value))()
        _lib.check(lib.rtfs_optim_plan(numel, T, table, None, None), "rtfs_optim_plan")
        self._table_host = torch.tensor(list(table), dtype=torch.int64)
        self._offsets = list(table[:T])
        dev = ps[0].device
        self._exp_avg = torch.zeros(self._flat_floats, dtype=torch.float32, device=dev)
        self._exp_avg_sq = torch.zeros(self._flat_floats, dtype=torch.float32, device=dev)
        self._table = self._flat_g = self._partials = self._norm = None  # device-side scratch: allocated once, at the first step
        self._steps = [0] * T     # host mirror of state[p]["step"] (refreshed by load_state_dict)
        self._pending = None      # (has_grad, zero_missing) between gather_grads() and step()
        for p in ps:
            self.state[p] = {"step": torch.tensor(0.0, dtype=torch.float32)}
        self._install_views()
        self._built = True

    def _install_views(self):
        for p, off in zip(self._params, self._offsets):
            n = p.numel()
            self.state[p]["exp_avg"] = self._exp_avg[off:off + n].view(p.shape)
            self.state[p]["exp_avg_sq"] = self._exp_avg_sq[off:off + n].view(p.shape)

    def add_param_group(self, param_group):
        if getattr(self, "_built", False):
            raise NotImplementedError("MI355X AdamW supports parameter groups given at construction only (the flat state is laid out once)")
        super().add_param_group(param_group)

    def _device_state(self, dev):
        """Flat moments on the parameters' device (a model moved after construction takes them along) and the once-only scratch."""
        if self._exp_avg.device != dev:
            self._exp_avg, self._exp_avg_sq = self._exp_avg.to(dev), self._exp_avg_sq.to(dev)
            self._install_views()
            self._table = None
        if self._table is None:
            self._table = self._table_host.to(dev)
            self._flat_g = _lib.empty(self._flat_floats, device=dev)
            self._partials = _lib.empty(self._n_chunks, device=dev, dtype=torch.float64)
            self._norm = _lib.empty((), device=dev)

    # ------------------------------------------------------------------ checkpoints
    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """Accepts ``torch.optim.AdamW.state_dict()`` (and its own): the moments are copied INTO the flat buffers, so ``state[p]`` keeps
        aliasing them; a parameter without an entry (torch creates state at a parameter's first gradient) restarts from zero."""
        super().load_state_dict(state_dict)
        loaded = self.state
        for group in self.param_groups:
            for name in ("amsgrad", "maximize", "capturable", "differentiable"):
                if group.get(name, False):
                    raise ValueError(f"MI355X AdamW supports {name}=False only (loaded param_group has {name}={group[name]!r})")
            if not group.get("decoupled_weight_decay", True):
                raise ValueError("MI355X AdamW supports decoupled weight decay only (loaded param_group is torch.optim.Adam's)")
        for i, (p, off) in enumerate(zip(self._params, self._offsets)):
            st, n = loaded.get(p, {}), p.numel()
            for key, flat in (("exp_avg", self._exp_avg), ("exp_avg_sq", self._exp_avg_sq)):
                dst = flat[off:off + n]
                if key in st:
                    dst.copy_(st[key].reshape(-1))
                else:
                    dst.zero_()
            self._steps[i] = int(st["step"]) if "step" in st else 0
            self.state[p] = {"step": torch.tensor(float(self._steps[i]), dtype=torch.float32)}
        self._install_views()
        self._pending = None

    # ------------------------------------------------------------------ the step
    @torch.no_grad()
    def gather_grads(self, zero_missing=False):
        """One launch: every parameter's ``.grad`` -> the flat gradient buffer (returned; tensor i at ``[offset_i, offset_i + numel_i)``,
        offsets rounded up to 4 floats, the gaps zero).  A parameter without a gradient is skipped as torch skips it, or, with
        ``zero_missing`` (what a data-parallel caller needs: ranks may disagree on which gradients exist, and the collective reads the
        whole buffer), written as zeros and treated as having a gradient.  A collective on the returned buffer goes between this call
        and ``step``; ``step`` then takes the norm of the buffer as it finds it."""
        ps = self._params
        _lib.need_gpu(*ps)
        lib, dev = _lib.load(), ps[0].device
        self._device_state(dev)
        ptrs, has, keep = [], [], []
        for p in ps:
            g = p.grad
            if g is None:
                ptrs.append(0)
                has.append(bool(zero_missing))
                continue
            if g.is_sparse or g.dtype != torch.float32 or g.device != dev:
                raise RuntimeError("MI355X AdamW supports dense float32 gradients on the parameters' device")
            if not g.is_contiguous():
                g = g.contiguous()
                keep.append(g)  # (freed stream-ordered: the launch below is queued first)
            ptrs.append(g.data_ptr())
            has.append(True)
        T = len(ps)
        grads = (C.c_void_p * T)(*ptrs)
        _lib.check(lib.rtfs_optim_gather_f32(grads, _lib.ptr(self._table), T, self._n_chunks, _lib.ptr(self._flat_g),
                                             None if zero_missing else _lib.ptr(self._partials), int(bool(zero_missing)),
                                             _lib.stream_of(self._flat_g)), "rtfs_optim_gather_f32")
        self._pending = (has, bool(zero_missing))
        return self._flat_g

    @torch.no_grad()
    def step(self, closure=None, max_norm=None, grad_scale=1.0):
        """clip_grad_norm_(params, max_norm) + the AdamW update in one launch (plus the gather, unless ``gather_grads`` ran since the last
        step, plus one norm launch after a ``zero_missing`` gather).  ``max_norm`` None or <= 0: no clipping.  ``grad_scale`` multiplies
        the gathered gradients on the fly (1 / world size after an all-reduce(SUM)); the norm is that of the scaled gradients.  Returns
        the total norm as a 0-d device tensor: the optimizer's own buffer, overwritten by the next step (clone it to keep it).
        ``group["lr"]`` is read every step."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._pending is None:
            self.gather_grads()
        (has, after_collective), self._pending = self._pending, None
        ps, lib, T = self._params, _lib.load(), len(self._params)
        st = _lib.stream_of(self._flat_g)
        if after_collective:
            _lib.check(lib.rtfs_optim_sumsq_f32(_lib.ptr(self._table), T, self._n_chunks, _lib.ptr(self._flat_g), _lib.ptr(self._partials), st),
                       "rtfs_optim_sumsq_f32")
        sets, index, active = {}, [None] * T, []
        for i, h in enumerate(has):
            if not h:
                continue
            self._steps[i] += 1
            active.append(ps[i])
            index[i] = sets.setdefault((self._group_of[i], self._steps[i]), len(sets))
        hyper = []
        for gi, t in sets:  # (insertion order = index order)
            g = self.param_groups[gi]
            lr, (b1, b2) = float(g["lr"]), g["betas"]
            hyper.append([1.0 - lr * g["weight_decay"], 1.0 - b1, b2, 1.0 - b2, lr / (1.0 - b1 ** t), (1.0 - b2 ** t) ** 0.5, g["eps"], 0.0])
        params = (C.c_void_p * T)(*[p.data_ptr() for p in ps])
        mn = float(max_norm) if max_norm else 0.0
        for base in range(0, max(len(hyper), 1), MAX_HYPER):  # one launch unless more than MAX_HYPER (group, step count) pairs are live
            part = hyper[base:base + MAX_HYPER] or [[1.0, 0.0, 1.0, 0.0, 0.0, 1.0, 1.0, 0.0]]
            idx = (C.c_ubyte * T)(*[_SKIP if k is None or not base <= k < base + MAX_HYPER else k - base for k in index])
            hy = (C.c_float * (8 * len(part)))(*[x for row in part for x in row])
            _lib.check(lib.rtfs_optim_adamw_f32(params, idx, hy, len(part), _lib.ptr(self._table), T, self._n_chunks, _lib.ptr(self._flat_g),
                                                _lib.ptr(self._exp_avg), _lib.ptr(self._exp_avg_sq), _lib.ptr(self._partials), mn,
                                                float(grad_scale), _lib.ptr(self._norm), st), "rtfs_optim_adamw_f32")
        if active:
            torch._foreach_add_([self.state[p]["step"] for p in active], 1)
            # the kernel wrote through raw pointers: the pack caches key on (data_ptr, _version) (packing.cached_train_pack)
            torch.autograd.graph.increment_version(active)
        return self._norm if closure is None else loss

    def zero_grad(self, set_to_none=True):
        self._pending = None
        super().zero_grad(set_to_none=set_to_none)


def make_optimizer(params, optimizer="adam", **kwargs):
    """optimizers.py:58-75: ``get(optimizer)(params, **kwargs)``; an Optimizer instance is returned as it is."""
    opt = get(optimizer)
    return opt if isinstance(opt, Optimizer) else opt(params, **kwargs)


def register_optimizer(custom_opt):
    """optimizers.py:78-87: make a custom optimizer class gettable by (case-insensitive) name; an existing name is refused."""
    name = custom_opt.__name__
    if name in globals() or name.lower() in {k.lower() for k in globals()}:
        raise ValueError(f"Optimizer {name} already exists. Choose another name.")
    globals()[name] = custom_opt


def get(identifier):
    """optimizers.py:90-108: a class from a case-insensitive name, an Optimizer instance as it is, ValueError otherwise."""
    if isinstance(identifier, Optimizer):
        return identifier
    if isinstance(identifier, str):
        cls = {k.lower(): v for k, v in globals().items()}.get(identifier.lower())
        if isinstance(cls, type) and issubclass(cls, Optimizer) and cls is not Optimizer:
            return cls
        if identifier.lower() in _TORCH_OPTIMIZER_NAMES:
            raise ValueError(f"Could not interpret optimizer : {identifier} (the reference takes it from the torch_optimizer package, "
                             "which is not a dependency of this project; register_optimizer() a class of that name to use it)")
    raise ValueError(f"Could not interpret optimizer : {identifier}")
