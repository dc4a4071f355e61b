"""Evaluation metrics of the reference on the device: ``pystoi.stoi`` (classic STOI, the version 0.4.1 the reference pins) and
``src/metrics/allwrapper.py`` ``ALLMetricsTracker``, same class name, constructor, methods and CSV.  STOI runs in ``librtfs_amd.so``
(``rtfs_stoi_f32``, ``csrc/k_stoi.hip``); SI-SNR and SNR are the PIT loss kernel the losses use (``rtfs_pit_pairwise_sdr_f32``).
There is no CPU fallback.  PESQ (ITU-T P.862) is not implemented here: pass a host callable as ``pesq_fn`` (called as the reference
calls ``pypesq.pesq``: ``pesq_fn(estimate, clean, 16000)`` on numpy rows) or the ``pesq`` column is NaN (and so are its mean and std).
"""
from __future__ import annotations

import csv

import numpy as np
import torch

from . import _lib
from .losses import _pairwise


def stoi(clean, estimate, fs=16000, extended=False, return_kept=False):
    """pystoi ``stoi(x, y, fs_sig, extended=False)`` for (B, L) or (L,) device tensors -> (B,) float32 (a 0-d tensor for 1-D input).
    fs 16000 (resampled to 10 kHz on the device) or 10000.  ``return_kept`` also returns the frames silence removal kept (int32), a
    speech-activity count.  Below 30 remaining STFT frames the score is 1e-5, as pystoi returns."""
    if extended:
        raise ValueError("extended STOI is not supported (the reference scores with extended=False)")
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


class ALLMetricsTracker:
    """reference allwrapper.py:19-134.  Per mixture: SI-SNR, SI-SNRi, SDR, SDRi, PESQ and STOI; ``final()`` adds ``avg`` and ``std``
    rows and closes the CSV.  Signs as the reference: the CSV holds ``si-snr = -loss``, ``si-snr_i = -(loss - baseline)`` but
    ``sdr = loss`` and ``sdr_i = loss - baseline`` (negative dB); the accumulated means / stds are positive dB for all four.
    ``update_batch`` scores a whole batch in one set of launches and moves one small host array."""

    COLUMNS = ["snt_id", "sdr", "sdr_i", "si-snr", "si-snr_i", "pesq", "stoi"]

    def __init__(self, save_file: str = "", pesq_fn=None, fs: int = 16000):
        self.all_sdrs, self.all_sdrs_i, self.all_sisnrs, self.all_sisnrs_i, self.all_pesqs, self.all_stois = [], [], [], [], [], []
        self.pesq_fn, self.fs = pesq_fn, fs
        self.results_csv = open(save_file, "w")
        self.writer = csv.DictWriter(self.results_csv, fieldnames=self.COLUMNS)
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
        st = stoi(clean[:, 0], estimate[:, 0], self.fs)
        vals = torch.stack([sdr, sdr - sdr_b, sisnr, sisnr - sisnr_b, st], 1).cpu().numpy()  # the one device -> host copy
        if self.pesq_fn is not None:
            est_h, cl_h = estimate[:, 0].cpu().numpy(), clean[:, 0].cpu().numpy()
            pesqs = [float(self.pesq_fn(est_h[b], cl_h[b], self.fs)) for b in range(B)]
        else:
            pesqs = [float("nan")] * B
        self.record(keys, vals, pesqs)

    def record(self, keys, vals, pesqs):
        """Write and accumulate rows from host values: vals (B, 5) = the losses (sdr, sdr - baseline, sisnr, sisnr - baseline) in the
        loss sign, then stoi; pesqs: B floats."""
        for b in range(len(keys)):
            l_sdr, l_sdr_i, l_sisnr, l_sisnr_i, s = (float(v) for v in vals[b])
            self.key = keys[b]
            self.writer.writerow({"snt_id": keys[b], "sdr": l_sdr, "sdr_i": l_sdr_i, "si-snr": -l_sisnr, "si-snr_i": -l_sisnr_i,
                                  "pesq": pesqs[b], "stoi": s})
            self.all_sdrs.append(-l_sdr)
            self.all_sdrs_i.append(-l_sdr_i)
            self.all_sisnrs.append(-l_sisnr)
            self.all_sisnrs_i.append(-l_sisnr_i)
            self.all_pesqs.append(pesqs[b])
            self.all_stois.append(s)

    def _lists(self):
        return {"sdr": self.all_sdrs, "sdr_i": self.all_sdrs_i, "si-snr": self.all_sisnrs, "si-snr_i": self.all_sisnrs_i,
                "pesq": self.all_pesqs, "stoi": self.all_stois}

    def get_mean(self):
        return {k: np.mean(v) for k, v in self._lists().items()}

    def get_std(self):
        return {k: np.std(v) for k, v in self._lists().items()}

    def final(self):
        self.writer.writerow({"snt_id": "avg", **{k: np.array(v).mean() for k, v in self._lists().items()}})
        self.writer.writerow({"snt_id": "std", **{k: np.array(v).std() for k, v in self._lists().items()}})
        self.results_csv.close()
