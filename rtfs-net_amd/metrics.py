"""Evaluation metrics of the reference on the device: ``pystoi.stoi`` (classic STOI, the version 0.4.1 the reference pins) and
``src/metrics/allwrapper.py`` ``ALLMetricsTracker``, same class name, constructor, methods and CSV.  STOI runs in ``librtfs_amd.so``
(``rtfs_stoi_f32``, ``csrc/k_stoi.hip``); SI-SNR and SNR are the PIT loss kernel the losses use (``rtfs_pit_pairwise_sdr_f32``).
``stoi_many``, ``sdr_many`` and ``ALLMetricsTracker.update_many`` score R recordings of different lengths in one pooled pass
(``rtfs_score_many_plan``, ``rtfs_stoi_many_f32``, ``rtfs_sdr_many_f32``; DESIGN.md, "Scoring many recordings of different lengths").
``estoi`` / ``estoi_many`` are extended STOI (``rtfs_estoi_f32`` / ``rtfs_estoi_many_f32``; DESIGN.md, "Extended STOI"), alone or
together with classic STOI from the same band values; ``ALLMetricsTracker(..., estoi=True)`` adds it as a seventh column.
``bss_sdr`` / ``bss_sdr_many`` are the SDR of BSS-eval (``rtfs_bss_sdr_f32`` / ``rtfs_bss_sdr_many_f32``, ``csrc/k_bss.hip``; DESIGN.md,
"BSS-eval SDR"): the 512-tap projection in float64; ``ALLMetricsTracker(..., bss_sdr=True)`` adds it and its improvement as two columns.
``bss_eval`` / ``bss_eval_many`` add BSS-eval's SIR and SAR from the joint projection onto all true sources (``rtfs_bss_eval_f32`` /
``rtfs_bss_eval_many_f32``; DESIGN.md, "BSS-eval SIR and SAR"); ``ALLMetricsTracker(..., bss_eval=True)`` adds them as two more columns.
There is no CPU fallback.  PESQ (ITU-T P.862) is not implemented here: pass a host callable as ``pesq_fn`` (called as the reference
calls ``pypesq.pesq``: ``pesq_fn(estimate, clean, 16000)`` on numpy rows) or the ``pesq`` column is NaN (and so are its mean and std).
"""
from __future__ import annotations

import collections
import csv
import ctypes as C

import numpy as np
import torch

from . import _lib
from .losses import _pairwise

SCORE_COLS = 11  # RTFS_SCORE_COLS: columns of rtfs_score_many_plan's table (include/rtfs_amd.h)


def stoi(clean, estimate, fs=16000, extended=False, return_kept=False):
    """pystoi ``stoi(x, y, fs_sig, extended=False)`` for (B, L) or (L,) device tensors -> (B,) float32 (a 0-d tensor for 1-D input).
    fs 16000 (resampled to 10 kHz on the device) or 10000.  ``return_kept`` also returns the frames silence removal kept (int32), a
    speech-activity count.  Below 30 remaining STFT frames the score is 1e-5, as pystoi returns."""
    if extended:
        raise ValueError("stoi scores classic STOI only (the reference scores with extended=False); extended STOI is metrics.estoi")
    if fs not in (16000, 10000):
        raise ValueError(f"stoi: fs must be 16000 or 10000, got {fs}")
    if clean.shape != estimate.shape or clean.ndim not in (1, 2):
        raise ValueError(f"stoi: clean and estimate must have the same (B, L) or (L,) shape, got {tuple(clean.shape)} and {tuple(estimate.shape)}")
    _lib.need_gpu(clean, estimate)
    lib = _lib.load()
    one = clean.ndim == 1
    x = clean.reshape(1, -1) if one else clean
    y = estimate.reshape(1, -1) if one else estimate
    x, y = x.contiguous(), y.contiguous()
    B, L = x.shape
    d = _lib.empty(B, device=x.device, dtype=torch.float32)
    kept = _lib.empty(B, device=x.device, dtype=torch.int32)
    nbytes = lib.rtfs_stoi_workspace_bytes(B, L, fs)
    ws = _lib.workspace(nbytes, x.device)
    _lib.check(lib.rtfs_stoi_f32(_lib.ptr(x), _lib.ptr(y), B, L, fs, _lib.ptr(ws), ws.numel(), _lib.ptr(d), _lib.ptr(kept),
                                 _lib.stream_of(x)), "rtfs_stoi_f32")
    if one:
        d, kept = d[0], kept[0]
    return (d, kept) if return_kept else d


def estoi(clean, estimate, fs=16000, return_kept=False, with_classic=False):
    """Extended STOI (Jensen & Taal 2016; pystoi ``stoi(x, y, fs_sig, extended=True)`` without its noise terms and with the inverse of
    a zero norm taken as 0: DESIGN.md, "Extended STOI") for (B, L) or (L,) device tensors -> (B,) float32, shapes, rates and refusals
    as ``stoi``.  ``with_classic`` also returns classic STOI computed from the same band values in the same call, bit-equal to
    ``stoi``: ``(estoi, stoi)``; ``return_kept`` appends the kept-frame counts.  Below 30 remaining STFT frames both are 1e-5."""
    if fs not in (16000, 10000):
        raise ValueError(f"estoi: fs must be 16000 or 10000, got {fs}")
    if clean.shape != estimate.shape or clean.ndim not in (1, 2):
        raise ValueError(f"estoi: clean and estimate must have the same (B, L) or (L,) shape, got {tuple(clean.shape)} and {tuple(estimate.shape)}")
    _lib.need_gpu(clean, estimate)
    lib = _lib.load()
    one = clean.ndim == 1
    x = clean.reshape(1, -1) if one else clean
    y = estimate.reshape(1, -1) if one else estimate
    x, y = x.contiguous(), y.contiguous()
    B, L = x.shape
    d = _lib.empty(B, device=x.device, dtype=torch.float32)
    dc = _lib.empty(B, device=x.device, dtype=torch.float32) if with_classic else None
    kept = _lib.empty(B, device=x.device, dtype=torch.int32)
    ws = _lib.workspace(lib.rtfs_estoi_workspace_bytes(B, L, fs, int(bool(with_classic))), x.device)
    _lib.check(lib.rtfs_estoi_f32(_lib.ptr(x), _lib.ptr(y), B, L, fs, _lib.ptr(ws), ws.numel(), _lib.ptr(d), _lib.ptr(dc), _lib.ptr(kept),
                                  _lib.stream_of(x)), "rtfs_estoi_f32")
    out = (d, dc) if with_classic else (d,)
    if return_kept:
        out += (kept,)
    if one:
        out = tuple(t[0] for t in out)
    return out if len(out) > 1 else out[0]


def _mirror(one, flat, *ts):
    """(B,n) results in the rank the inputs came in: (B,) for (B,L) inputs, 0-d for (L,) inputs."""
    if one:
        return tuple(t[0, 0] for t in ts)
    return tuple(t[:, 0] for t in ts) if flat else ts


def bss_sdr(clean, estimate, mix=None, return_perm=False):
    """BSS-eval SDR (the SDR of ``mir_eval.separation.bss_eval_sources`` with ``fast_bss_eval``'s permutation rule; definition:
    include/rtfs_amd.h and DESIGN.md, "BSS-eval SDR") in positive dB: each estimate is projected onto the 512 delayed copies of each
    clean source in float64, so a fixed delay or a short linear distortion is allowed.  clean / estimate float32 device tensors
    (B,n_src,L), (B,L) or (L,), n_src <= 4; mix (B,L) or (L,) -> ``sdr`` float32 (B,n_src) in clean-source order after the permutation
    that maximises the mean SDR (itertools order, first maximum); the input rank is mirrored as ``stoi`` does ((B,) and 0-d).  With
    ``mix`` it returns ``(sdr, sdr_i)``, ``sdr_i = sdr - SDR(mix, clean)``; ``return_perm`` appends ``perm`` int32 (``perm[b][j]`` = the
    estimate assigned to clean source j).  +inf, -inf and NaN come as IEEE gives them (a perfect estimate, a silent reference, a silent
    estimate).  Three launches, no host copy: capturable in a graph.  ValueError before any launch for shape or dtype mismatches."""
    ts = (clean, estimate) + (() if mix is None else (mix,))
    if not all(isinstance(t, torch.Tensor) for t in ts):
        raise ValueError("bss_sdr: clean, estimate and mix must be tensors")
    if clean.shape != estimate.shape or clean.ndim not in (1, 2, 3):
        raise ValueError(f"bss_sdr: clean and estimate must have the same (B, n_src, L), (B, L) or (L,) shape, got {tuple(clean.shape)} "
                         f"and {tuple(estimate.shape)}")
    one, flat = clean.ndim == 1, clean.ndim < 3
    B, n, L = (1, 1, clean.shape[0]) if one else (clean.shape[0], 1, clean.shape[1]) if flat else clean.shape
    if mix is not None and tuple(mix.shape) != ((L,) if one else (B, L)):
        raise ValueError(f"bss_sdr: mix must be {'(L,)' if one else '(B, L)'} = {(L,) if one else (B, L)}, got {tuple(mix.shape)}")
    if not 1 <= n <= 4:
        raise ValueError(f"bss_sdr: n_src must be 1 .. 4, got {n}")
    if B < 1 or L < 1:
        raise ValueError(f"bss_sdr: empty input {tuple(clean.shape)}")
    if any(t.dtype != torch.float32 for t in ts):
        raise ValueError(f"bss_sdr: the kernels are float32, got {[str(t.dtype) for t in ts]}")
    if any(t.device != clean.device for t in ts):
        raise ValueError(f"bss_sdr: the tensors lie on {[str(t.device) for t in ts]}")
    _lib.need_gpu(*ts)
    lib = _lib.load()
    c, e = clean.reshape(B, n, L).contiguous(), estimate.reshape(B, n, L).contiguous()
    m = None if mix is None else mix.reshape(B, L).contiguous()
    sdr = _lib.empty(B, n, device=c.device, dtype=torch.float32)
    sdr_i = None if m is None else _lib.empty(B, n, device=c.device, dtype=torch.float32)
    perm = _lib.empty(B, n, device=c.device, dtype=torch.int32)
    ws = _lib.workspace(lib.rtfs_bss_sdr_workspace_bytes(B, n, L, int(m is not None)), c.device)
    _lib.check(lib.rtfs_bss_sdr_f32(_lib.ptr(c), _lib.ptr(e), _lib.ptr(m), B, n, L, _lib.ptr(ws), ws.numel(), _lib.ptr(sdr), _lib.ptr(sdr_i),
                                    _lib.ptr(perm), _lib.stream_of(c)), "rtfs_bss_sdr_f32")
    out = (sdr,) + (() if m is None else (sdr_i,)) + ((perm,) if return_perm else ())
    out = _mirror(one, flat, *out)
    return out if len(out) > 1 else out[0]


BssEval = collections.namedtuple("BssEval", ["sdr", "sir", "sar", "sdr_i", "perm"])
_PERM_BY = {"sdr": 0, "sir": 1}  # RTFS_BSS_PERM_BY_SDR, RTFS_BSS_PERM_BY_SIR


def bss_eval(clean, estimate, mix=None, others=None, perm_by="sdr"):
    """BSS-eval SDR, SIR and SAR (the three ratios of ``mir_eval.separation.bss_eval_sources``; definition: include/rtfs_amd.h and
    DESIGN.md, "BSS-eval SIR and SAR") in positive dB -> the named tuple ``(sdr, sir, sar, sdr_i, perm)``.  SIR says how much of what
    is lost is the other sources leaking through, SAR how much is damage that no true source explains; both need the projection of
    the estimate onto the 512 delayed copies of ALL true sources at once (block Levinson in float64 on the device).  clean / estimate
    and mix as ``bss_sdr``; ``others`` (B,m,L) -- (m,L) for (L,) inputs -- are true sources that belong to the span but are not scored
    (an interfering talker, noise), n_src + m <= 4.  ``perm_by="sdr"`` (default) assigns the estimates as ``bss_sdr`` does, and then
    ``sdr``, ``sdr_i`` and ``perm`` are bit-equal to ``bss_sdr``'s; ``perm_by="sir"`` is mir_eval's rule, the largest mean SIR.  ``sir``
    and ``sar`` float32 (B,n_src): of the estimate assigned to clean source j; ``sdr_i`` is None without ``mix``; ``perm`` int32.  The
    input rank is mirrored as ``bss_sdr`` does.  A silent source leaves the joint set; with one source left SIR is +inf and SAR = SDR.
    Four launches, no host copy: capturable in a graph.  ValueError before any launch for shape, dtype or device mismatches."""
    ts = (clean, estimate) + (() if mix is None else (mix,)) + (() if others is None else (others,))
    if not all(isinstance(t, torch.Tensor) for t in ts):
        raise ValueError("bss_eval: clean, estimate, mix and others must be tensors")
    if perm_by not in _PERM_BY:
        raise ValueError(f"bss_eval: perm_by must be 'sdr' or 'sir', got {perm_by!r}")
    if clean.shape != estimate.shape or clean.ndim not in (1, 2, 3):
        raise ValueError(f"bss_eval: clean and estimate must have the same (B, n_src, L), (B, L) or (L,) shape, got {tuple(clean.shape)} "
                         f"and {tuple(estimate.shape)}")
    one, flat = clean.ndim == 1, clean.ndim < 3
    B, n, L = (1, 1, clean.shape[0]) if one else (clean.shape[0], 1, clean.shape[1]) if flat else clean.shape
    if mix is not None and tuple(mix.shape) != ((L,) if one else (B, L)):
        raise ValueError(f"bss_eval: mix must be {'(L,)' if one else '(B, L)'} = {(L,) if one else (B, L)}, got {tuple(mix.shape)}")
    m = 0
    if others is not None:
        if others.ndim != (2 if one else 3) or (not one and others.shape[0] != B) or others.shape[-1] != L:
            raise ValueError(f"bss_eval: others must be {'(m, L)' if one else '(B, m, L)'} with L = {L}"
                             f"{'' if one else f', B = {B}'}, got {tuple(others.shape)}")
        m = others.shape[-2]
    if not 1 <= n or n + m > 4:
        raise ValueError(f"bss_eval: n_src >= 1 and n_src + others <= 4, got {n} + {m}")
    if B < 1 or L < 1:
        raise ValueError(f"bss_eval: empty input {tuple(clean.shape)}")
    if any(t.dtype != torch.float32 for t in ts):
        raise ValueError(f"bss_eval: the kernels are float32, got {[str(t.dtype) for t in ts]}")
    if any(t.device != clean.device for t in ts):
        raise ValueError(f"bss_eval: the tensors lie on {[str(t.device) for t in ts]}")
    _lib.need_gpu(*ts)
    lib = _lib.load()
    c, e = clean.reshape(B, n, L).contiguous(), estimate.reshape(B, n, L).contiguous()
    mx = None if mix is None else mix.reshape(B, L).contiguous()
    o = others.reshape(B, m, L).contiguous() if m else None
    sdr, sir, sar = (_lib.empty(B, n, device=c.device, dtype=torch.float32) for _ in range(3))
    sdr_i = None if mx is None else _lib.empty(B, n, device=c.device, dtype=torch.float32)
    perm = _lib.empty(B, n, device=c.device, dtype=torch.int32)
    ws = _lib.workspace(lib.rtfs_bss_eval_workspace_bytes(B, n, m, L, int(mx is not None)), c.device)
    _lib.check(lib.rtfs_bss_eval_f32(_lib.ptr(c), _lib.ptr(e), _lib.ptr(mx), _lib.ptr(o), B, n, m, L, _lib.ptr(ws), ws.numel(), _lib.ptr(sdr),
                                     _lib.ptr(sir), _lib.ptr(sar), _lib.ptr(sdr_i), _lib.ptr(perm), _PERM_BY[perm_by], _lib.stream_of(c)),
               "rtfs_bss_eval_f32")
    sdr, sir, sar, perm = _mirror(one, flat, sdr, sir, sar, perm)
    return BssEval(sdr, sir, sar, None if mx is None else _mirror(one, flat, sdr_i)[0], perm)


class _ScorePool:
    """R recordings of different lengths, validated and planned for ``rtfs_stoi_many_f32`` / ``rtfs_sdr_many_f32``: everything that can
    be refused is refused here, as ValueError naming the recording, before any upload or launch.  ``mixes`` None: STOI only, clean and
    estimate rows (L_r)|(1,L_r) -- with ``multi`` (BSS-eval SDR without a baseline) (L_r)|(n_src,L_r).  Otherwise mix (L_r)|(1,L_r) and
    clean / estimate (n_src,L_r).  ``both``: the workspace also holds the tenth region ``estoi(with_classic=True)`` needs.  ``others``
    (``bss_eval``): R tensors (m,L_r)|(L_r), the true sources that are not scored, or "residual": when the pool is single-source, mix -
    clean, formed with one float32 subtraction over the whole pool (none when n_src > 1)."""

    def __init__(self, what, mixes, cleans, estimates, fs, keys=None, both=False, multi=False, others=None):
        try:
            cleans, estimates = list(cleans), list(estimates)
            mixes = None if mixes is None else list(mixes)
            keys = None if keys is None else list(keys)
            others = others if others is None or isinstance(others, str) else list(others)
        except TypeError:
            raise ValueError(f"{what}: the recordings must come as sequences of tensors") from None
        R = len(cleans)
        counts = [len(s) for s in (mixes, cleans, estimates, keys, None if isinstance(others, str) else others) if s is not None]
        if R < 1 or any(c != R for c in counts):
            raise ValueError(f"{what}: sequences of {counts} entries; need the same number in each, at least 1")
        if fs not in (16000, 10000):
            raise ValueError(f"{what}: fs must be 16000 or 10000, got {fs}")
        n = None
        for r in range(R):
            row = (cleans[r], estimates[r]) if mixes is None else (mixes[r], cleans[r], estimates[r])
            if not all(isinstance(t, torch.Tensor) for t in row):
                raise ValueError(f"{what}: recording {r} is not made of tensors")
            if mixes is None and multi:
                if any(t.ndim not in (1, 2) for t in row):
                    raise ValueError(f"{what}: clean and estimate {r} must be (L) or (n_src,L); got {[tuple(t.shape) for t in row]}")
                cleans[r], estimates[r] = (t.reshape(1, -1) if t.ndim == 1 else t for t in row)
            elif mixes is None:
                flat = [t for t in row if t.ndim == 1 or (t.ndim == 2 and t.shape[0] == 1)]
                if len(flat) != 2:
                    raise ValueError(f"{what}: clean and estimate {r} must be (L) or (1,L); got {[tuple(t.shape) for t in row]}")
                cleans[r], estimates[r] = (t.reshape(1, -1) for t in row)
            else:
                m, c, e = row
                if not (m.ndim == 1 or (m.ndim == 2 and m.shape[0] == 1)) or c.ndim != 2 or e.ndim != 2:
                    raise ValueError(f"{what}: recording {r} must be mix (L)|(1,L), clean and estimate (n_src,L); "
                                     f"got {[tuple(t.shape) for t in row]}")
                mixes[r] = m.reshape(-1)
            c, e = cleans[r], estimates[r]
            n = c.shape[0] if n is None else n
            if c.shape[0] != n or e.shape[0] != n or not 1 <= n <= 4:
                raise ValueError(f"{what}: recording {r} has {c.shape[0]} clean and {e.shape[0]} estimated source(s); "
                                 f"recording 0 has {n} (n_src 1 .. 4, the same everywhere)")
            if e.shape[1] != c.shape[1] or (mixes is not None and mixes[r].shape[0] != c.shape[1]):
                lens = [int(t.shape[-1]) for t in row]
                raise ValueError(f"{what}: recording {r} has lengths {lens}; mix, clean and estimate must be equally long")
            if any(t.dtype != torch.float32 for t in row):
                raise ValueError(f"{what}: recording {r} is {[str(t.dtype) for t in row]}; the kernels are float32")
        m = 0
        if isinstance(others, list):
            for r, o in enumerate(others):
                if not isinstance(o, torch.Tensor) or o.ndim not in (1, 2) or o.shape[-1] != cleans[r].shape[1] or o.dtype != torch.float32:
                    raise ValueError(f"{what}: others {r} must be a float32 tensor (m,L)|(L) with L = {cleans[r].shape[1]}; got "
                                     f"{(tuple(o.shape), str(o.dtype)) if isinstance(o, torch.Tensor) else type(o).__name__}")
                others[r] = o.reshape(1, -1) if o.ndim == 1 else o
                m = others[r].shape[0] if r == 0 else m
                if others[r].shape[0] != m or m < 1 or n + m > 4:
                    raise ValueError(f"{what}: others {r} holds {others[r].shape[0]} source(s), others 0 holds {m} "
                                     f"(the same everywhere, n_src + others <= 4)")
        elif others is not None and (others != "residual" or mixes is None):
            raise ValueError(f"{what}: others must be a sequence of tensors (or the residual of a pool with mixtures)")
        lib = _lib.load()
        lens = [int(c.shape[1]) for c in cleans]
        self.plan = (C.c_int * (SCORE_COLS * (R + 1)))()
        nbytes = C.c_size_t(0)
        if lib.rtfs_score_many_plan((C.c_longlong * R)(*lens), R, n, fs, self.plan, C.byref(nbytes)) != 0:
            one, scratch = C.c_size_t(0), (C.c_int * (SCORE_COLS * 2))()
            for r, L in enumerate(lens):
                if lib.rtfs_score_many_plan((C.c_longlong * 1)(L), 1, n, fs, scratch, C.byref(one)) != 0:
                    raise ValueError(f"{what}: recording {r} has {L} samples; STOI at fs = {fs} needs "
                                     f"{410 if fs == 16000 else 257} .. 2^26")
            raise ValueError(f"{what}: {R} recordings of {sum(lens)} samples need a workspace offset past 2^31 - 1")
        device = cleans[0].device
        for r in range(R):
            row = (cleans[r], estimates[r]) if mixes is None else (mixes[r], cleans[r], estimates[r])
            row += (others[r],) if isinstance(others, list) else ()
            if any(t.device != device for t in row):
                raise ValueError(f"{what}: recording {r} lies on {[str(t.device) for t in row]}, recording 0 on {device}")
        if device.type != "cuda":
            raise ValueError(f"{what}: the recordings lie on {device}; the kernels run on the MI355X only (there is no CPU fallback)")
        self.lib, self.R, self.n, self.fs, self.device, self.keys = lib, R, n, fs, device, keys
        self.cleans, self.estimates = [c.contiguous() for c in cleans], [e.contiguous() for e in estimates]
        self.mixes = None if mixes is None else [m.contiguous() for m in mixes]
        groups = [self.cleans, self.estimates] + ([] if mixes is None else [self.mixes])
        if isinstance(others, str):  # the other source of a single-source row: for a clean two-talker mixture the interfering talker
            others = [o.reshape(1, -1) for o in torch._foreach_sub(self.mixes, [c[0] for c in self.cleans])] if n == 1 else None
            m = int(n == 1)
        self.others, self.m = None if others is None else [o.contiguous() for o in others], m
        ptrs = [t.data_ptr() for g in groups for t in g] + [o[k].data_ptr() for o in self.others or [] for k in range(m)]
        ptrs = np.array(ptrs, dtype=np.int64)
        host = np.concatenate([ptrs.view(np.uint8), np.ctypeslib.as_array(self.plan).view(np.uint8)])
        self.tab = torch.from_numpy(host).to(device)  # the one host-to-device copy: 2 R | 3 R (+ R m) pointers, then the plan's table
        base = self.tab.data_ptr()
        self.p_clean, self.p_est, self.p_mix = (C.c_void_p(base + 8 * R * k) for k in range(3))
        self.p_others = C.c_void_p(base + 8 * R * len(groups)) if m else None
        self.p_table = C.c_void_p(base + 8 * R * (len(groups) + m))
        self.both = bool(both)
        self.ws = _lib.workspace(lib.rtfs_estoi_many_workspace_bytes(self.plan, R, 1) if both else nbytes.value, device)
        self.stream = _lib.stream_of(self.tab)

    def stoi(self):
        d = _lib.empty(self.R, device=self.device, dtype=torch.float32)
        kept = _lib.empty(self.R, device=self.device, dtype=torch.int32)
        _lib.check(self.lib.rtfs_stoi_many_f32(self.p_clean, self.p_est, self.p_table, self.plan, self.R, self.n, self.fs, _lib.ptr(self.ws),
                                               self.ws.numel(), _lib.ptr(d), _lib.ptr(kept), self.stream), "rtfs_stoi_many_f32")
        return d, kept

    def estoi(self, with_classic=False):
        """-> (estoi, stoi | None, kept)"""
        if with_classic and not self.both:
            raise ValueError("this pool's workspace was not sized for extended and classic STOI together")
        d = _lib.empty(self.R, device=self.device, dtype=torch.float32)
        dc = _lib.empty(self.R, device=self.device, dtype=torch.float32) if with_classic else None
        kept = _lib.empty(self.R, device=self.device, dtype=torch.int32)
        _lib.check(self.lib.rtfs_estoi_many_f32(self.p_clean, self.p_est, self.p_table, self.plan, self.R, self.n, self.fs,
                                                _lib.ptr(self.ws), self.ws.numel(), _lib.ptr(d), _lib.ptr(dc), _lib.ptr(kept), self.stream),
                   "rtfs_estoi_many_f32")
        return d, dc, kept

    def sdr(self):
        out = _lib.empty(self.R, 4, device=self.device, dtype=torch.float32)
        perm = _lib.empty(self.R, self.n, device=self.device, dtype=torch.int32)
        _lib.check(self.lib.rtfs_sdr_many_f32(self.p_mix, self.p_clean, self.p_est, self.p_table, self.plan, self.R, self.n, self.fs,
                                              _lib.ptr(self.ws), self.ws.numel(), _lib.ptr(out), _lib.ptr(perm), self.stream),
                   "rtfs_sdr_many_f32")
        return out, perm

    def bss(self):
        """-> (sdr (R,n), sdr_i (R,n) | None without mixtures, perm (R,n)); a workspace of its own, the pool's table (columns 0 and 10)"""
        with_mix = self.mixes is not None
        sdr = _lib.empty(self.R, self.n, device=self.device, dtype=torch.float32)
        sdr_i = _lib.empty(self.R, self.n, device=self.device, dtype=torch.float32) if with_mix else None
        perm = _lib.empty(self.R, self.n, device=self.device, dtype=torch.int32)
        ws = _lib.workspace(self.lib.rtfs_bss_sdr_many_workspace_bytes(self.plan, self.R, int(with_mix)), self.device)
        _lib.check(self.lib.rtfs_bss_sdr_many_f32(self.p_mix if with_mix else None, self.p_clean, self.p_est, self.p_table, self.plan, self.R,
                                                  self.n, self.fs, _lib.ptr(ws), ws.numel(), _lib.ptr(sdr), _lib.ptr(sdr_i), _lib.ptr(perm),
                                                  self.stream), "rtfs_bss_sdr_many_f32")
        return sdr, sdr_i, perm

    def bss_eval(self, perm_by="sdr"):
        """-> BssEval of (R,n) tensors (sdr_i None without mixtures); a workspace of its own, the pool's table (columns 0 and 10)"""
        with_mix = self.mixes is not None
        sdr, sir, sar = (_lib.empty(self.R, self.n, device=self.device, dtype=torch.float32) for _ in range(3))
        sdr_i = _lib.empty(self.R, self.n, device=self.device, dtype=torch.float32) if with_mix else None
        perm = _lib.empty(self.R, self.n, device=self.device, dtype=torch.int32)
        ws = _lib.workspace(self.lib.rtfs_bss_eval_many_workspace_bytes(self.plan, self.R, self.m, int(with_mix)), self.device)
        _lib.check(self.lib.rtfs_bss_eval_many_f32(self.p_mix if with_mix else None, self.p_clean, self.p_est, self.p_others, self.p_table,
                                                   self.plan, self.R, self.n, self.m, self.fs, _lib.ptr(ws), ws.numel(), _lib.ptr(sdr),
                                                   _lib.ptr(sir), _lib.ptr(sar), _lib.ptr(sdr_i), _lib.ptr(perm), _PERM_BY[perm_by],
                                                   self.stream), "rtfs_bss_eval_many_f32")
        return BssEval(sdr, sir, sar, sdr_i, perm)


def bss_eval_many(cleans, estimates, mixes=None, others=None, perm_by="sdr"):
    """``bss_eval`` for R recordings of different lengths in one pooled pass: cleans / estimates / mixes as ``bss_sdr_many``, others None
    or R tensors (m,L_r)|(L_r) -> the named tuple ``(sdr, sir, sar, sdr_i, perm)`` of (R,n_src) tensors (``sdr_i`` None without mixes).
    Entry r is bit-equal to ``bss_eval`` on recording r (the same kernels).  The pool, its length limits (410 .. 2^26 samples) and its
    errors are ``bss_sdr_many``'s; the workspace is the call's own.  Not capturable (table upload)."""
    if perm_by not in _PERM_BY:
        raise ValueError(f"bss_eval_many: perm_by must be 'sdr' or 'sir', got {perm_by!r}")
    try:
        cleans, estimates = ([t.reshape(1, -1) if isinstance(t, torch.Tensor) and t.ndim == 1 else t for t in s] for s in (cleans, estimates))
    except TypeError:
        raise ValueError("bss_eval_many: the recordings must come as sequences of tensors") from None
    return _ScorePool("bss_eval_many", mixes, cleans, estimates, 16000, multi=True, others=others).bss_eval(perm_by)


def bss_sdr_many(cleans, estimates, mixes=None, return_perm=False):
    """``bss_sdr`` for R recordings of different lengths in one pooled pass: cleans / estimates R float32 device tensors (n_src,L_r) or
    (L_r), mixes None or R tensors (L_r)|(1,L_r) -> ``sdr`` (R,n_src) float32, with mixes ``(sdr, sdr_i)``, with ``return_perm`` ``perm``
    (R,n_src) int32 appended.  Entry r is bit-equal to ``bss_sdr`` on recording r (the same kernels).  The pool is the one of
    ``stoi_many`` (one planner call, one table upload, rows read where they lie), so STOI's length limits apply, 410 .. 2^26 samples,
    and are named in the error; the workspace is the call's own.  Not capturable (table upload)."""
    try:
        cleans, estimates = ([t.reshape(1, -1) if isinstance(t, torch.Tensor) and t.ndim == 1 else t for t in s] for s in (cleans, estimates))
    except TypeError:
        raise ValueError("bss_sdr_many: the recordings must come as sequences of tensors") from None
    sdr, sdr_i, perm = _ScorePool("bss_sdr_many", mixes, cleans, estimates, 16000, multi=True).bss()
    out = (sdr,) + (() if mixes is None else (sdr_i,)) + ((perm,) if return_perm else ())
    return out if len(out) > 1 else out[0]


def stoi_many(cleans, estimates, fs=16000, return_kept=False):
    """``stoi`` for R recordings of different lengths in one pooled pass: two sequences of R float32 device tensors (L_r)|(1,L_r) -> (R,)
    float32, and with ``return_kept`` the kept frames (R,) int32.  Entry r is bit-equal to ``stoi(cleans[r], estimates[r], fs)``.  The
    rows are read where they lie (separate allocations, any 4-byte alignment); one planner call, ONE host-to-device copy of the table
    and the 2 R row pointers, five launches whose grids are flat work lists, a workspace that grows with sum(L_r).  Because of the
    upload a call is not capturable in a HIP graph.  ValueError, before the upload, names the offending recording."""
    d, kept = _ScorePool("stoi_many", None, cleans, estimates, fs).stoi()
    return (d, kept) if return_kept else d


def estoi_many(cleans, estimates, fs=16000, return_kept=False, with_classic=False):
    """``estoi`` for R recordings of different lengths in one pooled pass, inputs and refusals as ``stoi_many`` -> (R,) float32; with
    ``with_classic`` ``(estoi, stoi)`` from the same band values, with ``return_kept`` the kept frames (R,) int32 appended.  Entry r is
    bit-equal to ``estoi(cleans[r], estimates[r], fs, with_classic=...)``.  Not capturable (table upload)."""
    d, dc, kept = _ScorePool("estoi_many", None, cleans, estimates, fs, both=with_classic).estoi(with_classic)
    out = (d, dc) if with_classic else (d,)
    if return_kept:
        out += (kept,)
    return out if len(out) > 1 else out[0]


def sdr_many(mixes, cleans, estimates):
    """The tracker's four PIT figures for R mixtures of different lengths in one pass over the samples: mixes R tensors (L_r)|(1,L_r),
    cleans / estimates R tensors (n_src,L_r) -> (R,4) float32 in the loss sign [sdr, sdr - baseline, sisnr, sisnr - baseline] (baseline =
    the mixture stacked n_src times against the clean sources) and the (R,n_src) int32 permutation of the estimate-vs-clean SI-SDR search.
    Float64 moments, so the figures agree with ``losses._pairwise`` to rounding, not bit for bit.  Not capturable (table upload)."""
    return _ScorePool("sdr_many", mixes, cleans, estimates, 16000).sdr()


class ALLMetricsTracker:
    """reference allwrapper.py:19-134.  Per mixture: SI-SNR, SI-SNRi, SDR, SDRi, PESQ and STOI; ``final()`` adds ``avg`` and ``std``
    rows and closes the CSV.  Signs as the reference: the CSV holds ``si-snr = -loss``, ``si-snr_i = -(loss - baseline)`` but
    ``sdr = loss`` and ``sdr_i = loss - baseline`` (negative dB); the accumulated means / stds are positive dB for all four.
    ``update_batch`` scores a whole batch in one set of launches and moves one small host array.  ``estoi=True`` (not in the
    reference) adds extended STOI as a seventh metric ``"estoi"`` after ``"stoi"`` everywhere -- rows, ``avg`` / ``std``, ``get_mean`` /
    ``get_std``, ``all_estois`` -- computed with classic STOI in one combined call; without it the tracker is the reference's.
    ``bss_sdr=True`` (not in the reference either) adds BSS-eval SDR (``metrics.bss_sdr``) as the columns ``"bss_sdr"`` and
    ``"bss_sdr_i"`` after ``"stoi"`` (after ``"estoi"`` when both options are on), each the mean over the sources, in POSITIVE dB in
    the CSV and in ``all_bss_sdrs`` / ``all_bss_sdrs_i`` alike -- unlike the reference's ``sdr`` / ``sdr_i`` next to them, which the
    CSV holds as negative dB and which are plain SNR: one sample of delay ruins those, a delay of up to 511 samples leaves these.
    ``bss_eval=True`` implies ``bss_sdr=True`` and appends ``"bss_sir"`` and ``"bss_sar"`` after ``"bss_sdr_i"`` (``metrics.bss_eval``
    with the SDR's permutation rule, so the two SDR columns do not notice), each the mean over the sources in positive dB, kept in
    ``all_bss_sirs`` / ``all_bss_sars``.  When ``n_src == 1`` the other true source of the joint projection is ``mix - clean``, one float32
    subtraction on the device: for a clean two-talker mixture that is the interfering talker (SIR then says how much of it leaks
    through), for a noisy mixture it is everything that is not the target.  With ``n_src > 1`` the span is the clean sources alone."""

    COLUMNS = ["snt_id", "sdr", "sdr_i", "si-snr", "si-snr_i", "pesq", "stoi"]

    def __init__(self, save_file: str = "", pesq_fn=None, fs: int = 16000, estoi: bool = False, bss_sdr: bool = False,
                 bss_eval: bool = False):
        self.all_sdrs, self.all_sdrs_i, self.all_sisnrs, self.all_sisnrs_i, self.all_pesqs, self.all_stois = [], [], [], [], [], []
        self.pesq_fn, self.fs, self.estoi, self.bss_sdr, self.bss_eval = pesq_fn, fs, bool(estoi), bool(bss_sdr or bss_eval), bool(bss_eval)
        self.columns = self.COLUMNS + (["estoi"] if self.estoi else []) + (["bss_sdr", "bss_sdr_i"] if self.bss_sdr else [])
        self.columns += ["bss_sir", "bss_sar"] if self.bss_eval else []
        if self.estoi:
            self.all_estois = []
        if self.bss_sdr:
            self.all_bss_sdrs, self.all_bss_sdrs_i = [], []
        if self.bss_eval:
            self.all_bss_sirs, self.all_bss_sars = [], []
        self.results_csv = open(save_file, "w")
        self.writer = csv.DictWriter(self.results_csv, fieldnames=self.columns)
        self.writer.writeheader()

    def __call__(self, mix, clean, estimate, key):
        """One mixture as the reference takes it: mix (L,), clean / estimate (n_src, L)."""
        self.update_batch(mix.unsqueeze(0), clean.unsqueeze(0), estimate.unsqueeze(0), [key])

    def update_batch(self, mix, clean, estimate, keys):
        """mix (B, L), clean / estimate (B, n_src, L), keys: B row ids.  STOI scores source 0 against target 0 (the reference passes
        the single-source rows of RTFS-Net)."""
        if estimate.ndim != 3 or clean.shape != estimate.shape or mix.shape != (clean.shape[0], clean.shape[2]) or len(keys) != clean.shape[0]:
            raise ValueError(f"update_batch: expected mix (B, L), clean / estimate (B, n_src, L) and B keys; got {tuple(mix.shape)}, "
                             f"{tuple(clean.shape)}, {tuple(estimate.shape)}, {len(keys)} keys")
        _lib.need_gpu(mix, clean, estimate)
        B, n, L = clean.shape
        clean, estimate = clean.contiguous(), estimate.contiguous()
        mixs = mix.unsqueeze(1).expand(B, n, L).contiguous()  # torch.stack([mix] * n_src)
        sisnr = _pairwise(estimate, clean, "sisdr", True, True)[1]
        sisnr_b = _pairwise(mixs, clean, "sisdr", True, True)[1]
        sdr = _pairwise(estimate, clean, "snr", True, True)[1]
        sdr_b = _pairwise(mixs, clean, "snr", True, True)[1]
        if self.estoi:  # stages 1-3 once: (estoi, stoi) from the same band values
            est, st = estoi(clean[:, 0], estimate[:, 0], self.fs, with_classic=True)
            cols = [sdr, sdr - sdr_b, sisnr, sisnr - sisnr_b, st, est]
        else:
            cols = [sdr, sdr - sdr_b, sisnr, sisnr - sisnr_b, stoi(clean[:, 0], estimate[:, 0], self.fs)]
        if self.bss_eval:  # each the mean over the sources, positive dB; a single source is scored against mix - clean as well
            ev = bss_eval(clean, estimate, mix, mix.unsqueeze(1) - clean if n == 1 else None)
            cols += [v.mean(1) for v in (ev.sdr, ev.sdr_i, ev.sir, ev.sar)]
        elif self.bss_sdr:
            cols += [v.mean(1) for v in bss_sdr(clean, estimate, mix)]
        vals = torch.stack(cols, 1).cpu().numpy()  # the one device -> host copy
        if self.pesq_fn is not None:
            est_h, cl_h = estimate[:, 0].cpu().numpy(), clean[:, 0].cpu().numpy()
            pesqs = [float(self.pesq_fn(est_h[b], cl_h[b], self.fs)) for b in range(B)]
        else:
            pesqs = [float("nan")] * B
        self.record(keys, vals, pesqs)

    def update_many(self, mixes, cleans, estimates, keys):
        """R mixtures of different lengths in one pooled pass (the scoring half of ``separate_many``): mixes R tensors (L_r)|(1,L_r),
        cleans / estimates R tensors (n_src,L_r), keys R row ids.  One planner call, one table upload, the launches of
        ``rtfs_sdr_many_f32`` and ``rtfs_stoi_many_f32`` on one workspace, ONE device-to-host copy of an (R,5) array, then ``record``:
        the CSV and the accumulators come out as R calls of ``__call__`` leave them, rows in input order (the stoi column identical,
        the dB columns to float64 rounding of the moments).  STOI scores source 0 against target 0, ``pesq_fn`` is called per recording.
        ValueError, before the upload, names the offending recording."""
        pool = _ScorePool("update_many", mixes, cleans, estimates, self.fs, keys, both=self.estoi,
                          others="residual" if self.bss_eval else None)
        if self.estoi:  # (R,6): stages 1-3 once, (estoi, stoi) from the same band values
            est, st, _ = pool.estoi(with_classic=True)
            cols = [pool.sdr()[0], st[:, None], est[:, None]]
        else:
            cols = [pool.sdr()[0], pool.stoi()[0][:, None]]
        if self.bss_eval:
            ev = pool.bss_eval()
            cols += [v.mean(1, keepdim=True) for v in (ev.sdr, ev.sdr_i, ev.sir, ev.sar)]
        elif self.bss_sdr:
            cols += [v.mean(1, keepdim=True) for v in pool.bss()[:2]]
        vals = torch.cat(cols, 1).cpu().numpy()  # the one device -> host copy
        if self.pesq_fn is not None:
            pesqs = [float(self.pesq_fn(e[0].cpu().numpy(), c[0].cpu().numpy(), self.fs)) for e, c in zip(pool.estimates, pool.cleans)]
        else:
            pesqs = [float("nan")] * pool.R
        self.record(pool.keys, vals, pesqs)

    def record(self, keys, vals, pesqs):
        """Write and accumulate rows from host values: vals (B, 5) = the losses (sdr, sdr - baseline, sisnr, sisnr - baseline) in the
        loss sign, then stoi; with ``estoi=True`` estoi follows; with ``bss_sdr=True`` bss_sdr and bss_sdr_i (positive dB, the means over the
        sources) follow, and with ``bss_eval=True`` bss_sir and bss_sar after them: 5 + estoi + 2 + 2 values per row; pesqs: B floats."""
        n_ext = int(self.estoi) + 2 * int(self.bss_sdr) + 2 * int(self.bss_eval)
        for b in range(len(keys)):
            l_sdr, l_sdr_i, l_sisnr, l_sisnr_i, s, *ext = (float(v) for v in vals[b])
            if len(ext) != n_ext:
                raise ValueError(f"record: {len(vals[b])} values per row; this tracker takes {5 + n_ext}")
            self.key = keys[b]
            row = {"snt_id": keys[b], "sdr": l_sdr, "sdr_i": l_sdr_i, "si-snr": -l_sisnr, "si-snr_i": -l_sisnr_i,
                   "pesq": pesqs[b], "stoi": s}
            if self.estoi:
                row["estoi"] = ext[0]
                self.all_estois.append(ext[0])
            if self.bss_sdr:
                k = int(self.estoi)
                row["bss_sdr"], row["bss_sdr_i"] = ext[k], ext[k + 1]
                self.all_bss_sdrs.append(ext[k])
                self.all_bss_sdrs_i.append(ext[k + 1])
            if self.bss_eval:
                row["bss_sir"], row["bss_sar"] = ext[-2], ext[-1]
                self.all_bss_sirs.append(ext[-2])
                self.all_bss_sars.append(ext[-1])
            self.writer.writerow(row)
            self.all_sdrs.append(-l_sdr)
            self.all_sdrs_i.append(-l_sdr_i)
            self.all_sisnrs.append(-l_sisnr)
            self.all_sisnrs_i.append(-l_sisnr_i)
            self.all_pesqs.append(pesqs[b])
            self.all_stois.append(s)

    def _lists(self):
        lists = {"sdr": self.all_sdrs, "sdr_i": self.all_sdrs_i, "si-snr": self.all_sisnrs, "si-snr_i": self.all_sisnrs_i,
                 "pesq": self.all_pesqs, "stoi": self.all_stois}
        if self.estoi:
            lists["estoi"] = self.all_estois
        if self.bss_sdr:
            lists["bss_sdr"], lists["bss_sdr_i"] = self.all_bss_sdrs, self.all_bss_sdrs_i
        if self.bss_eval:
            lists["bss_sir"], lists["bss_sar"] = self.all_bss_sirs, self.all_bss_sars
        return lists

    def get_mean(self):
        return {k: np.mean(v) for k, v in self._lists().items()}

    def get_std(self):
        return {k: np.std(v) for k, v in self._lists().items()}

    def final(self):
        self.writer.writerow({"snt_id": "avg", **{k: np.array(v).mean() for k, v in self._lists().items()}})
        self.writer.writerow({"snt_id": "std", **{k: np.array(v).std() for k, v in self._lists().items()}})
        self.results_csv.close()
