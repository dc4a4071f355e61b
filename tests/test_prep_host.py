"""Host side of the preparation path (rtfs-net_amd/datas.py, rtfs_resample_plan, the argument checks of rtfs_lips_prepare_u8) and the
conditions tests/prep_oracle.py itself has to meet.  None of it touches a device: the plan helpers are host functions of the library, and
the refusals tested here return before anything is launched."""
import ctypes
import math
import os
import random
import re

import numpy as np
import pytest
import torch

from tests import prep_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["rtfs_lips_prepare_u8", "rtfs_wav_normalize_workspace_bytes", "rtfs_wav_normalize_f32", "rtfs_resample_plan",
               "rtfs_resample_out_len", "rtfs_resample_f32"]
# every rate the device test resamples, and the extremes of the supported range
RATIOS = [(48000, 16000), (44100, 16000), (32000, 16000), (22050, 16000), (11025, 16000), (8000, 16000), (16000, 48000), (96000, 16000),
          (24000, 16000), (640, 1), (1, 640), (639, 640), (640, 639)]


def datas():
    from rtfs_net_amd import datas as D
    return D


def lib():
    from rtfs_net_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------- resampling: plan, bank, oracle
def test_bank_shape_per_ratio():
    assert PO.resample_plan(48000, 16000) == (3, 1, 19, 41)
    assert PO.resample_plan(44100, 16000) == (441, 160, 17, 475)
    assert PO.resample_plan(8000, 16000) == (1, 2, 7, 15)
    for a, b in RATIOS:
        o, n, width, taps = PO.resample_plan(a, b)
        assert datas().resample_plan(a, b) == (o, n, width, taps), (a, b)
        assert PO.resample_bank(a, b).shape == (n, taps) and PO.resample_bank(a, b).dtype == np.float32


def test_output_length_is_ceil():
    for a, b in RATIOS:
        o, n, width, taps = PO.resample_plan(a, b)
        for L in (1, 2, taps - 1, o - 1, o, o + 1, 16001, 48000 * 300):
            if L < 1:
                continue
            want = math.ceil(n * L / o) if n * L < 2 ** 50 else -(-n * L // o)
            assert PO.resample_out_len(a, b, L) == want == -(-n * L // o)
            assert lib().rtfs_resample_out_len(a, b, L) == want, (a, b, L)
    assert lib().rtfs_resample_out_len(641, 1, 100) == -1
    x = np.random.RandomState(0).randn(2, 1001)
    assert PO.resample(x, 44100, 16000).shape == (2, PO.resample_out_len(44100, 16000, 1001))


def test_c_bank_is_bit_equal_to_the_oracle_bank():
    for a, b in RATIOS:
        got = datas()._host_bank(a, b).numpy()
        want = PO.resample_bank(a, b)
        assert got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32)), (a, b)
    assert datas().resample_bank(44100, 16000) is datas().resample_bank(441, 160)  # cached per reduced ratio and device


def test_bank_support_the_kernel_relies_on():
    """Row p of the float32 bank is exactly zero outside taps [floor(o p / n), floor(o p / n) + 2 width]: the kernel sums those 2 width + 1
    taps only (rtfs_resample_plan refuses to build a bank for which that would not hold)."""
    for a, b in RATIOS:
        o, n, width, taps = PO.resample_plan(a, b)
        bank = PO.resample_bank(a, b)
        k = np.arange(taps)[None, :]
        c = (o * np.arange(n) // n)[:, None]
        outside = (k < c) | (k > c + 2 * width)
        assert not np.any(bank[outside] != 0.0), (a, b)
        assert (c + 2 * width).max() <= taps - 1


def sparse_resample(x, orig, new):
    """The kernel's form: y[j n + p] = sum_s bank[p, c + s] x[j o + c + s - width], c = floor(o p / n), zeros outside the recording."""
    o, n, width, taps = PO.resample_plan(orig, new)
    bank = PO.resample_bank(orig, new).astype(np.float64)
    L = x.shape[-1]
    Lout = -(-n * L // o)
    g = np.arange(Lout)
    j, p = g // n, g % n
    c = o * p // n
    y = np.zeros(Lout)
    for s in range(2 * width + 1):
        i = j * o + c + s - width
        ok = (i >= 0) & (i < L)
        y += bank[p, c + s] * np.where(ok, x[np.clip(i, 0, L - 1)], 0.0)
    return y


def test_sparse_form_equals_the_full_sum():
    rng = np.random.RandomState(1)
    for a, b in RATIOS[:9]:
        o, n, width, taps = PO.resample_plan(a, b)
        for L in (1, taps - 1, o, o + 1, 3 * o + 2 * width + 5):
            x = rng.randn(L)
            full, sparse = PO.resample(x, a, b), sparse_resample(x, a, b)
            assert full.shape == sparse.shape
            assert np.abs(full - sparse).max() <= 1e-13 * max(1.0, np.abs(full).max()), (a, b, L)


@pytest.mark.parametrize("fs", [48000, 44100, 22050, 32000, 8000])
def test_oracle_fidelity_on_a_sine(fs):
    """A condition on the oracle, not a parity bar: a unit sine well below both Nyquist rates survives to within 1e-3."""
    f = 500.0 if fs == 8000 else 1000.0
    x = np.sin(2 * np.pi * f * np.arange(fs) / fs)
    y = PO.resample(x, fs, 16000)
    assert y.shape == (16000,)
    want = np.sin(2 * np.pi * f * np.arange(16000) / 16000)
    err = float(np.abs(y - want)[200:-200].max())
    print(f"[prep] oracle {fs} -> 16000, {f:.0f} Hz sine: max error {err:.2e}")
    assert err < 1e-3, err


def test_equal_rates_return_the_input_and_bad_ratios_raise():
    x = torch.zeros(4)
    assert datas().resample(x, 16000, 16000) is x  # no device needed: nothing runs
    a = np.zeros(3)
    assert PO.resample(a, 8000, 8000) is a
    for orig, new in [(641, 1), (16000, 16001), (44101, 16000), (0, 16000), (-1, 16000)]:
        with pytest.raises(ValueError):
            datas().resample_plan(orig, new)
        with pytest.raises(ValueError):
            PO.resample_plan(orig, new)
        with pytest.raises(ValueError):
            datas().resample(torch.zeros(8), orig, new)
    assert lib().rtfs_resample_plan(641, 1, None, None, None, None, None) == -4
    assert datas().resample_plan(96000, 16000) == (6, 1, 37, 80)
    with pytest.raises(RuntimeError):  # a supported ratio on a host tensor: no CPU fallback
        datas().resample(torch.zeros(8), 48000, 16000)


# ---------------------------------------------------------------- lips: offsets, draws, chains, refusals
def test_center_offsets_follow_the_reference_rounding():
    D = datas()
    cc = D.CenterCrop((88, 88))
    assert cc.offsets(96, 96) == (4, 4) == PO.center_offsets(96, 96)
    assert cc.offsets(88, 88) == (0, 0)
    assert cc.offsets(112, 100) == (12, 6)
    # odd differences: int(round(9) / 2.0) = int(4.5) = 4, int(round(11) / 2.0) = 5 (truncation, not round-half-even)
    assert cc.offsets(97, 99) == (4, 5) == PO.center_offsets(97, 99)
    assert cc.offsets(89, 91) == (0, 1)


def test_train_draw_order_is_dx_dy_flip():
    D = datas()
    pipe = D.get_preprocessing_pipelines()["train"]
    random.seed(1234)
    want = []
    for _ in range(5):
        dx = random.randint(0, 100 - 88)
        dy = random.randint(0, 112 - 88)
        flip = 1 if random.random() < 0.5 else 0
        want.append((dy, dx, flip))
    random.seed(1234)
    assert pipe.table(5, 112, 100) == want
    assert pipe.table(5, 112, 100, rng=random.Random(1234)) == want
    random.seed(1234)
    assert [PO.draw_offsets(112, 100) for _ in range(5)] == want
    assert len({r[2] for r in pipe.table(64, 96, 96, rng=random.Random(0))}) == 2  # both flip values occur
    val = D.get_preprocessing_pipelines()["val"]
    state = random.getstate()
    assert val.table(3, 96, 96) == [(4, 4, 0)] * 3
    assert random.getstate() == state  # "val" draws nothing


def test_pipelines_and_chains():
    D = datas()
    pipes = D.get_preprocessing_pipelines()
    assert set(pipes) == {"train", "val", "test"} and pipes["test"] is pipes["val"]
    assert [type(t).__name__ for t in pipes["train"].preprocess] == ["Normalize", "RandomCrop", "HorizontalFlip", "Normalize"]
    assert [type(t).__name__ for t in pipes["val"].preprocess] == ["Normalize", "CenterCrop", "Normalize"]
    last = pipes["val"].preprocess[-1]
    assert (last.mean, last.std) == (0.421, 0.165) and pipes["train"].preprocess[2].flip_ratio == 0.5
    assert "CenterCrop" in repr(pipes["val"])
    roi = torch.zeros(2, 96, 96, dtype=torch.uint8)
    bad = [D.Compose([D.CenterCrop((88, 88)), D.Normalize(0.421, 0.165)]),
           D.Compose([D.Normalize(0.0, 255.0), D.CenterCrop((64, 64)), D.Normalize(0.421, 0.165)]),
           D.Compose([D.Normalize(0.0, 1.0), D.CenterCrop((88, 88)), D.Normalize(0.421, 0.165)]),
           D.Compose([D.Normalize(0.0, 255.0), D.HorizontalFlip(0.5), D.CenterCrop((88, 88)), D.Normalize(0.421, 0.165)]),
           D.Compose([D.Normalize(0.0, 255.0), D.CenterCrop((88, 88)), D.Normalize(0.421, 0.165), D.HorizontalFlip(0.5)]),
           D.Compose([])]
    for c in bad:
        with pytest.raises(ValueError):
            c(roi)
    with pytest.raises(RuntimeError):  # the reference's chain on a host tensor: no CPU fallback
        pipes["val"](roi)
    import rtfs_net_amd as R
    for name in ("Compose", "Normalize", "CenterCrop", "RandomCrop", "HorizontalFlip", "get_preprocessing_pipelines", "resample",
                 "normalize_tensor_wav", "normalize_mixture"):
        assert getattr(R, name) is getattr(D, name)


def test_lips_entry_refuses_bad_arguments_before_any_launch():
    """The checks run on the host table and return before a launch, so they can be exercised without a device (the pointers are never
    dereferenced on these paths)."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(rows, N, Tv, H, W, std=0.165):
        tab = (ctypes.c_int * (3 * len(rows)))(*[v for r in rows for v in r])
        return lib().rtfs_lips_prepare_u8(p, tab, p, N, Tv, H, W, 0.421, std, None)

    assert call([(9, 0, 0)], 1, 1, 96, 96) == -4      # dy + 88 > H
    assert call([(0, 13, 0)], 1, 1, 112, 100) == -4   # dx + 88 > W
    assert call([(-1, 0, 0)], 1, 1, 96, 96) == -4
    assert call([(0, -1, 1)], 1, 1, 96, 96) == -4
    assert call([(0, 0, 2)], 1, 1, 96, 96) == -4      # flip is 0 or 1
    assert call([(4, 4, 0), (4, 9, 0)], 2, 1, 96, 96) == -4  # the second track
    assert call([(0, 0, 0)], 1, 1, 87, 96) == -1      # ROI smaller than the crop
    assert call([(0, 0, 0)], 1, 0, 96, 96) == -1
    assert call([(0, 0, 0)], 0, 1, 96, 96) == -1
    assert call([(0, 0, 0)], 1, 1, 96, 96, std=0.0) == -4
    assert lib().rtfs_lips_prepare_u8(None, None, None, 1, 1, 96, 96, 0.421, 0.165, None) == -4
    with pytest.raises(ValueError):
        PO.lips_prepare(np.zeros((1, 1, 96, 96), np.uint8), [(9, 0, 0)])


def test_other_entries_refuse_bad_arguments_before_any_launch():
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    L_ = lib()
    assert L_.rtfs_wav_normalize_workspace_bytes(2, 1, 16384) == 2 * 2 * 1 * 16
    assert L_.rtfs_wav_normalize_workspace_bytes(1, 0, 16385) == 2 * 16
    assert L_.rtfs_wav_normalize_f32(p, None, None, p, None, 1, 0, 0, 1e-8, p, 4096, None) == -1
    assert L_.rtfs_wav_normalize_f32(p, None, None, p, None, 1, 1, 100, 1e-8, p, 4096, None) == -4   # K = 1 without sources
    assert L_.rtfs_wav_normalize_f32(p, None, None, p, None, 1, 0, 100, 1e-8, p, 8, None) == -2      # workspace too small
    assert L_.rtfs_wav_normalize_f32(None, None, None, p, None, 1, 0, 100, 1e-8, p, 4096, None) == -4
    assert L_.rtfs_resample_f32(p, p, p, 1, 100, 641, 1, None) == -4
    assert L_.rtfs_resample_f32(p, p, p, 1, 0, 3, 1, None) == -1
    assert L_.rtfs_resample_f32(p, p, p, 0, 100, 3, 1, None) == -1
    assert L_.rtfs_resample_f32(p, None, p, 1, 100, 3, 1, None) == -4
    assert L_.rtfs_resample_f32(p, p, p, 1, 2 ** 31 - 1, 1, 2, None) == -1  # the output would pass 2^31 - 1 samples


# ---------------------------------------------------------------- oracle sanity
def test_lips_oracle_is_the_reference_chain():
    rng = np.random.RandomState(2)
    roi = rng.randint(0, 256, (2, 3, 100, 96)).astype(np.uint8)
    got = PO.lips_prepare(roi, [(5, 2, 0), (12, 8, 1)])
    assert got.shape == (2, 1, 3, 88, 88) and got.dtype == np.float32
    f = (roi.astype(np.float64) - 0.0) / 255.0
    a = (f[0, :, 5:93, 2:90] - 0.421) / 0.165
    b = (f[1, :, 12:100, 8:96][:, :, ::-1] - 0.421) / 0.165
    assert np.array_equal(got[0, 0], a.astype(np.float32)) and np.array_equal(got[1, 0], b.astype(np.float32))
    assert len(np.unique(got)) <= 256


def test_normalize_oracle_matches_torch_in_float64():
    rng = np.random.RandomState(3)
    mix, src = rng.randn(3, 1000) * 0.1 + 2.0, rng.randn(3, 2, 1000)
    mo, so = PO.normalize_mixture(mix, src)
    tm, ts = torch.from_numpy(mix), torch.from_numpy(src)
    sd = tm.std(-1, keepdim=True)
    assert np.allclose(mo, ((tm - tm.mean(-1, keepdim=True)) / (sd + 1e-8)).numpy(), rtol=1e-12, atol=1e-12)
    assert np.allclose(so, ((ts - ts.mean(-1, keepdim=True)) / (sd.unsqueeze(1) + 1e-8)).numpy(), rtol=1e-12, atol=1e-12)
    assert np.allclose(PO.normalize_tensor_wav(mix), mo, rtol=1e-12, atol=1e-12)
    assert np.allclose(PO.normalize_tensor_wav(src, std=sd.unsqueeze(1).numpy()), so, rtol=1e-12, atol=1e-12)
    assert abs(mo.mean()) < 1e-12 and abs(mo.std(-1, ddof=1) - 1).max() < 1e-6
    one, _ = PO.normalize_mixture(np.ones((2, 1)))
    assert np.isnan(one).all()  # L = 1: torch.std gives NaN


# ---------------------------------------------------------------- System and the C surface
def test_prepare_batch_leaves_float_slots_untouched():
    import rtfs_net_amd as R
    s = R.System(audio_model=None, video_model=None)
    wav, tgt, lips = torch.zeros(2, 100), torch.zeros(2, 1, 100), torch.zeros(2, 1, 3, 88, 88)
    out = s.prepare_batch((wav, tgt, lips, ["a", "b"]), train=False)
    assert isinstance(out, tuple) and len(out) == 4
    assert out[0] is wav and out[1] is tgt and out[2] is lips and out[3] == ["a", "b"]
    out = s.prepare_batch([wav, tgt, ["a"]])
    assert isinstance(out, list) and out[0] is wav and out[1] is tgt
    with pytest.raises(ValueError):
        s.prepare_batch((wav, tgt, torch.zeros(2, 96, 96, dtype=torch.uint8), None))
    assert callable(s.separate_recording)


def test_new_symbols_in_binding_table_and_header():
    from rtfs_net_amd import _lib
    with open(os.path.join(ROOT, "include", "rtfs_amd.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "rtfs-net_amd", "csrc", "kernels.h")) as f:
        internal = f.read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert hasattr(lib(), name)
    for name in ("launch_lips_prepare", "launch_wav_normalize", "launch_resample", "resample_plan"):
        assert name in internal
    with open(os.path.join(ROOT, "rtfs-net_amd", "csrc", "Makefile")) as f:
        assert "k_prep.hip" in f.read()
