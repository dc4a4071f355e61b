"""Preparing raw recordings on the device: what the reference does on the host in front of the model inputs, with its names.

* ``resample``                       ``torchaudio.transforms.Resample(fs, 16000)`` of ``infer_any_video.py:66-68`` (its default kernel bank)
* ``normalize_tensor_wav`` / ``normalize_mixture``   ``src/datas/avspeech_dataset.py:18-22`` and its joint use at ``:145-148, 206-209``
* ``Compose``, ``Normalize``, ``CenterCrop``, ``RandomCrop``, ``HorizontalFlip``, ``get_preprocessing_pipelines``
                                     ``src/datas/transform.py``: on ``uint8`` device ROIs a pipeline is ONE ``rtfs_lips_prepare_u8`` launch
* ``mouth_affine`` / ``mouth_rois``  ``RTFSNet_file.py:20-73, 111-118`` (``align_face``, lip box, ``cv2.resize``, grey) as one affine map per
                                     (frame, face) and ONE ``rtfs_mouth_rois_u8`` launch on whole camera frames (``csrc/k_mouth.hip``)
* ``MixRecipe`` / ``draw_mix_recipe`` / ``mix_batch``   training mixtures formed on the device: ``System.online_mixing_collate``
                                     (``src/system/core.py:183-202``) and target + interferers at a drawn SNR, a host plan and TWO launches
                                     of ``rtfs_mix_f32`` (``csrc/k_mix.hip``)
* ``reverberate`` / ``load_rirs`` / ``synthetic_rir``   reverberant training mixtures: every source convolved with its own room impulse
                                     response on the device (``csrc/k_reverb.hip``), alone or in front of the two mix launches
                                     (``mix_batch(..., rirs=...)``)
* ``loudness`` / ``loudness_many`` / ``loudness_normalize`` / ``MixRecipe.lufs``   ITU-R BS.1770 integrated loudness on the device
                                     (K-weighting, 400 ms blocks, two gates; ``csrc/k_loudness.hip``) and levels set by it

All arithmetic runs in ``librtfs_amd.so`` (``csrc/k_prep.hip``); there is no host fallback.  ``tests/prep_oracle.py`` restates the three
in float64 numpy."""
from __future__ import annotations

import ctypes as C
import fractions
import operator
import random

import torch

from . import _lib

__all__ = ["Compose", "Normalize", "CenterCrop", "RandomCrop", "HorizontalFlip", "get_preprocessing_pipelines", "resample",
           "normalize_tensor_wav", "normalize_mixture", "resample_plan", "resample_bank", "open_resample_streams", "frame_rate_of", "frame_rate_map",
           "timestamp_map", "mouth_affine", "mouth_rois", "MixRecipe", "draw_mix_recipe", "mix_batch", "reverberate", "load_rirs",
           "synthetic_rir", "loudness", "loudness_many", "loudness_normalize"]

CROP = 88
MAX_RATIO = 640


# ---------------------------------------------------------------- resampling
def resample_plan(orig_freq, new_freq):
    """-> (o, n, width, taps) of ``rtfs_resample_plan``; ValueError for a reduced ratio past 640."""
    o, n, w, t = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
    if int(orig_freq) < 1 or int(new_freq) < 1 or \
            _lib.load().rtfs_resample_plan(int(orig_freq), int(new_freq), C.byref(o), C.byref(n), C.byref(w), C.byref(t), None) != 0:
        raise ValueError(f"resample {orig_freq} -> {new_freq}: positive rates with a reduced ratio of at most {MAX_RATIO}:{MAX_RATIO} only")
    return o.value, n.value, w.value, t.value


def _host_bank(orig_freq, new_freq):
    o, n, width, taps = resample_plan(orig_freq, new_freq)
    bank = _lib.empty(n, taps, device="cpu")
    _lib.check(_lib.load().rtfs_resample_plan(int(orig_freq), int(new_freq), None, None, None, None, C.c_void_p(bank.data_ptr())),
               "rtfs_resample_plan")
    return bank


_BANKS = {}


def resample_bank(orig_freq, new_freq, device="cpu"):
    """The (n, taps) float32 kernel bank of torchaudio's Resample defaults, built on the host in float64 once per (ratio, device)."""
    o, n, _, _ = resample_plan(orig_freq, new_freq)
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (o, n, str(device))
    if key not in _BANKS:
        _BANKS[key] = _host_bank(o, n).to(device)
    return _BANKS[key]


def resample(wav, orig_freq, new_freq=16000):
    """wav (L) | (B,L) float32 on the device -> (..., ceil(n L / o)).  Equal rates return the input tensor itself, as torchaudio does."""
    if int(orig_freq) == int(new_freq):
        return wav
    o, n, _, _ = resample_plan(orig_freq, new_freq)
    _lib.need_gpu(wav)
    if wav.ndim not in (1, 2) or wav.shape[-1] < 1:
        raise ValueError(f"resample: wav must be (L) or (B,L) with L >= 1; got {tuple(wav.shape)}")
    x = wav.reshape(-1, wav.shape[-1]).contiguous()
    B, L = int(x.shape[0]), int(x.shape[1])
    bank = resample_bank(o, n, x.device)
    Lout = int(_lib.load().rtfs_resample_out_len(o, n, L))
    y = _lib.empty(B, Lout, device=x.device)
    _lib.check(_lib.load().rtfs_resample_f32(_lib.ptr(x), _lib.ptr(bank), _lib.ptr(y), B, L, o, n, _lib.stream_of(x)), "rtfs_resample_f32")
    return y[0] if wav.ndim == 1 else y


def open_resample_streams(slots, orig_freq, new_freq=16000, max_chunk=None, device=None):
    """``slots`` live streams resampled chunk by chunk (DESIGN.md "Live streams at the microphone's rate") ->
    ``streaming.ResampleStreamPool``.  ``pool.push(slot_ids, chunks)`` takes float32 or int16 PCM chunks of at most ``max_chunk`` input
    samples (default one second) and returns the (k,) outputs that became final; ``pool.flush(slot_ids)`` ends streams.  For any
    chunking the concatenated outputs are bit-equal to ``resample`` of the whole recording, which ``resample`` per chunk is not: it pads
    every chunk edge with zeros and rounds every chunk's length up.  ValueError for equal rates and for what ``resample_plan`` refuses."""
    from . import streaming
    return streaming.open_resample_streams(slots, orig_freq, new_freq, max_chunk=max_chunk, device=device)


# ---------------------------------------------------------------- frame rates
def frame_rate_of(frame_rate):
    """A camera's frame rate as a reduced ``Fraction``: an int, a ``Fraction``, (num, den), or a float, which is taken as
    ``Fraction(x).limit_denominator(1001)`` (29.97 -> 2997/100, 29.97002997 -> 30000/1001).  ValueError for anything else, a rate
    outside [1, 240] fps or a term above 2^20 (what ``rtfs_frame_rate_map`` refuses)."""
    f = frame_rate
    try:
        if isinstance(f, bool):
            raise TypeError
        if isinstance(f, fractions.Fraction):
            rate = f
        elif isinstance(f, float):
            rate = fractions.Fraction(f).limit_denominator(1001)
        elif isinstance(f, (tuple, list)):
            if len(f) != 2 or any(isinstance(v, bool) for v in f):
                raise TypeError
            rate = fractions.Fraction(operator.index(f[0]), operator.index(f[1]))
        else:
            rate = fractions.Fraction(operator.index(f))
    except (TypeError, ValueError, ZeroDivisionError, OverflowError):
        raise ValueError(f"frame_rate = {frame_rate!r}; an int, a Fraction, (num, den) or a float") from None
    if not 1 <= rate <= 240 or max(rate.numerator, rate.denominator) > 1 << 20:
        raise ValueError(f"frame_rate = {frame_rate!r}; between 1 and 240 fps, numerator and denominator at most 2^20")
    return rate


def frame_rate_map(n, frame_rate):
    """The camera frames that the model's 25 fps frames show, for a track of ``n`` camera frames at ``frame_rate``: a list of P(n)
    indices, entry p = c(p) (``rtfs_frame_rate_map``; DESIGN.md "Live streams at the camera's frame rate").  At 25 fps it is 0 .. n - 1."""
    rate, n = frame_rate_of(frame_rate), operator.index(n)
    lib, out = _lib.load(), C.c_longlong(0)
    if n < 0 or lib.rtfs_frame_rate_map(rate.numerator, rate.denominator, n, C.byref(out), None) != 0:
        raise ValueError(f"frame_rate_map: n = {n} frames at {rate} fps")
    src = (C.c_longlong * max(out.value, 1))()
    _lib.check(lib.rtfs_frame_rate_map(rate.numerator, rate.denominator, n, C.byref(out), src), "rtfs_frame_rate_map")
    return list(src[:out.value])


def timestamp_map(timestamps, timebase, until=None):
    """The camera frames that the model's 25 fps frames show, for a whole track whose frames were taken at ``timestamps`` (increasing
    ints, or a CPU int64 tensor, in ticks of 1 / ``timebase`` s): a list, entry p = c(p), the last camera frame whose tick
    floor(25 t + 1/2) is at or before p and the first frame before that (``rtfs_timestamp_map``; DESIGN.md "Live streams with
    per-frame timestamps").  The track ends as a flushed stream does: with the last frame's own tick, or with the last model frame
    that ``until`` - the largest the stream was given - makes final.  ValueError for stamps that do not increase, are negative or
    reach 2^40, and for a timebase outside [1, 2^30]."""
    from .streaming import timebase_of
    tb = timebase_of(timebase)
    if tb is None:
        raise ValueError("timestamp_map: timebase must be an integer number of ticks per second")
    try:
        ts = timestamps.tolist() if isinstance(timestamps, torch.Tensor) else list(timestamps)
        if any(isinstance(t, bool) for t in ts):
            raise TypeError
        ts = [operator.index(t) for t in ts]
        u = 0 if until is None else operator.index(until)
    except TypeError:
        raise ValueError("timestamp_map: timestamps must be a sequence of integers and until an integer or None") from None
    n, LL = len(ts), C.c_longlong
    if any(not 0 <= t < 1 << 40 for t in ts) or not 0 <= u <= 1 << 40:
        raise ValueError("timestamp_map: timestamps lie in [0, 2^40), until in [0, 2^40]")
    lib, out, arr = _lib.load(), LL(0), (LL * max(n, 1))(*ts)
    if lib.rtfs_timestamp_map(arr, n, tb, u, C.byref(out), None) != 0:
        raise ValueError(f"timestamp_map: {n} timestamp(s) at {tb} ticks per second must increase (and give at most 2^36 model frames)")
    src = (LL * max(out.value, 1))()
    _lib.check(lib.rtfs_timestamp_map(arr, n, tb, u, C.byref(out), src), "rtfs_timestamp_map")
    return list(src[:out.value])


# ---------------------------------------------------------------- mouth ROIs from whole camera frames (DESIGN.md "Mouth ROIs from camera frames")
MOUTH_ORDERS = {"gray": 0, "bgr": 1, "rgb": 2}
MOUTH_JOB_WORDS = 12  # RTFS_MOUTH_JOB_WORDS: [source | destination | H | W | pitch | pixel stride + 65536 order | the six doubles of A]
MOUTH_MAX_DIM, MOUTH_MAX_OUT = 0x7fff, 4096


def _hw(v, what):
    try:
        h, w = v
        return operator.index(h), operator.index(w)
    except (TypeError, ValueError):
        raise ValueError(f"{what} = {v!r}; a pair of integers (H, W)") from None


def _mouth_sizes(out_hw, crop_hw, who):
    (Ho, Wo), (Hc, Wc) = _hw(out_hw, f"{who}: out_hw"), _hw(crop_hw, f"{who}: crop_hw")
    if not (1 <= Hc <= Ho <= MOUTH_MAX_OUT and 1 <= Wc <= Wo <= MOUTH_MAX_OUT):
        raise ValueError(f"{who}: crop_hw = {(Hc, Wc)} must lie in [1, out_hw = {(Ho, Wo)}] per axis, out_hw at most {MOUTH_MAX_OUT}")
    return Ho, Wo, Hc, Wc


def _landmarks(x, tail, what):
    """A host array of landmarks (numpy, a CPU tensor, nested lists) as a contiguous float64 CPU tensor (..., *tail)."""
    if isinstance(x, torch.Tensor) and x.is_cuda:
        raise ValueError(f"{what} lie on {x.device}: landmarks are host arrays (they come from a host-side tracker and feed the host planner)")
    try:
        t = x if isinstance(x, torch.Tensor) else torch.as_tensor(x, dtype=torch.float64)  # Python floats are float64 already
        if t.is_complex() or t.dtype == torch.bool:
            raise TypeError
        t = t.detach().to(torch.float64).contiguous()
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"{what} must be a numeric host array (..., {tail[0]}, {tail[1]})") from None
    if t.ndim < 2 or tuple(t.shape[-2:]) != tail:
        raise ValueError(f"{what} must be (..., {tail[0]}, {tail[1]}); got {tuple(t.shape)}")
    return t


def _mouth_affine(e, l, Ho, Wo, Hc, Wc, who):
    """The C planner on checked float64 CPU tensors e (...,2,2), l (...,4,2) -> A (...,2,3)."""
    if e.shape[:-2] != l.shape[:-2]:
        raise ValueError(f"{who}: eyes {tuple(e.shape)} and lips {tuple(l.shape)} do not name the same landmark sets")
    A = _lib.empty(*e.shape[:-2], 2, 3, device="cpu", dtype=torch.float64)
    n = e.numel() // 4
    if n:
        bad = C.c_longlong(-1)
        if _lib.load().rtfs_mouth_affine(_lib.ptr(e), _lib.ptr(l), n, Ho, Wo, Hc, Wc, _lib.ptr(A), C.byref(bad)) != 0:
            raise ValueError(f"{who}: landmark set {bad.value} of {n} is refused: a non-finite landmark, eye corners that coincide "
                             f"(dist == 0) or a map with a non-finite entry")
    return A


def mouth_affine(eyes, lips, out_hw=(96, 96), crop_hw=(88, 88)):
    """Landmarks -> the affine map of every (frame, face), on the host in float64 (``rtfs_mouth_affine``; DESIGN.md "Mouth ROIs from
    camera frames").  eyes (...,2,2): the eye corner that lies on the left IN THE IMAGE, then the right one (mediapipe 130, 359 in the
    reference); lips (...,4,2): the four points whose bounding box is the mouth (187, 411, 136, 365); both (x, y) in pixels of the source
    frame, numpy arrays or CPU tensors.  Returns A (...,2,3) of the same kind: ROI pixel (i, j) of an ``out_hw`` ROI shows the source point
    sx = A00 j + A01 i + A02, sy = A10 j + A11 i + A12, and the lip box of the reference's 256 x 256 aligned face fills the central
    ``crop_hw``.  ValueError for wrong shapes, ``crop_hw`` outside [1, ``out_hw``], non-finite landmarks, eye corners that coincide and
    a map with a non-finite entry."""
    Ho, Wo, Hc, Wc = _mouth_sizes(out_hw, crop_hw, "mouth_affine")
    A = _mouth_affine(_landmarks(eyes, (2, 2), "mouth_affine: eyes"), _landmarks(lips, (4, 2), "mouth_affine: lips"), Ho, Wo, Hc, Wc,
                      "mouth_affine")
    return A if isinstance(eyes, torch.Tensor) else A.numpy()


def _mouth_plan(frames, eyes, lips, out_hw, crop_hw, order, who, faces=None):
    """Everything of a ``mouth_rois`` call that needs no launch: checks the frame tensors and their landmarks and runs the host planner.
    frames, eyes, lips: equally long lists.  faces: None (the landmarks say whether they carry a face axis) or True (they must).
    -> {"items": [(frames (n,H,W[,3]), A (n,K,2,3) float64, has a face axis)], "hw": (Ho, Wo), "order": code, "device"}."""
    Ho, Wo, Hc, Wc = _mouth_sizes(out_hw, crop_hw, who)
    if not isinstance(order, str) or order not in MOUTH_ORDERS:
        raise ValueError(f"{who}: order = {order!r}; one of {tuple(MOUTH_ORDERS)}")
    if not (len(frames) == len(eyes) == len(lips)):
        raise ValueError(f"{who}: {len(frames)} frame tensor(s), {len(eyes)} eyes and {len(lips)} lips array(s)")
    items, device = [], None
    for r, (f, e, l) in enumerate(zip(frames, eyes, lips)):
        if not isinstance(f, torch.Tensor) or not f.is_cuda or f.dtype != torch.uint8:
            raise ValueError(f"{who}: frames {r} must be a uint8 tensor on the device; got "
                             f"{(f.dtype, f.device) if isinstance(f, torch.Tensor) else type(f).__name__}")
        device = f.device if device is None else device
        if f.device != device:
            raise ValueError(f"{who}: frames {r} lie on {f.device}, frames 0 on {device}")
        if f.ndim not in (3, 4) or (f.ndim == 4 and (f.shape[3] != 3 or f.stride(3) != 1 or order == "gray")):
            raise ValueError(f"{who}: frames {r} must be (n,H,W,3) with the channels adjacent (order bgr | rgb) or a grey plane (n,H,W); "
                             f"got {tuple(f.shape)} with strides {tuple(f.stride())}, order {order!r}")
        n, H, W = (int(v) for v in f.shape[:3])
        if not (1 <= H <= MOUTH_MAX_DIM and 1 <= W <= MOUTH_MAX_DIM):
            raise ValueError(f"{who}: frames {r} are {H} x {W}; between 1 and {MOUTH_MAX_DIM} pixels a side")
        if f.stride(1) >= 1 << 31 or f.stride(2) > 0xffff or (f.ndim == 4 and W > 1 and f.stride(2) < 3):
            raise ValueError(f"{who}: frames {r} have strides {tuple(f.stride())}: a row pitch below 2^31, a pixel stride in [3 | 1, 65535]")
        e, l = _landmarks(e, (2, 2), f"{who}: eyes {r}"), _landmarks(l, (4, 2), f"{who}: lips {r}")
        if e.ndim not in (3, 4) or l.ndim != e.ndim or e.shape[0] != n or (faces and e.ndim != 4):
            raise ValueError(f"{who}: frames {r} hold {n} frame(s); eyes must be ({n},{'K,' if faces else '[K,]'}2,2) and lips "
                             f"({n},{'K,' if faces else '[K,]'}4,2); got {tuple(e.shape)} and {tuple(l.shape)}")
        A = _mouth_affine(e, l, Ho, Wo, Hc, Wc, f"{who}: frames {r}")
        items.append((f, A.reshape(n, int(e.shape[1]) if e.ndim == 4 else 1, 2, 3), e.ndim == 4))
    return {"items": items, "hw": (Ho, Wo), "order": MOUTH_ORDERS[order], "device": device}


def _mouth_alloc(plan):
    """The ROI tensors of a plan, (n,K,Ho,Wo) uint8 per item: views of ONE new allocation."""
    Ho, Wo = plan["hw"]
    sizes = [int(A.shape[0]) * int(A.shape[1]) * Ho * Wo for _, A, _ in plan["items"]]
    flat = _lib.empty(sum(sizes), device=plan["device"], dtype=torch.uint8)
    return [c.view(int(A.shape[0]), int(A.shape[1]), Ho, Wo) for c, (_, A, _) in zip(flat.split(sizes), plan["items"])]


_MOUTH_TABLES = {}    # device -> (the job table of the last launch on the host, the same on the device)
_MOUTH_CAPTURED = []  # device tables that a captured graph reads: kept for the life of the process


def _mouth_run(plan, outs):
    """The one launch of a plan.  outs: per item a uint8 device tensor (n,K,Ho,Wo) whose (Ho,Wo) planes are contiguous; the other
    strides and the alignment are free.  The job table is built on the host and goes up in one copy; a call that repeats the previous
    call's table (the same tensors and landmarks, as a warmed-up call under HIP-graph capture does) reuses the copy on the device."""
    (Ho, Wo), dev, rows = plan["hw"], plan["device"], []
    for r, ((f, A, _), o) in enumerate(zip(plan["items"], outs)):
        n, K = int(A.shape[0]), int(A.shape[1])
        if not isinstance(o, torch.Tensor) or o.dtype != torch.uint8 or o.device != dev or tuple(o.shape) != (n, K, Ho, Wo) or \
                (Ho > 1 and o.stride(2) != Wo) or (Wo > 1 and o.stride(3) != 1):
            raise ValueError(f"mouth_rois: out {r} must be a uint8 tensor {(n, K, Ho, Wo)} on {dev} with contiguous ({Ho},{Wo}) planes")
        if n * K == 0:
            continue
        t = _lib.empty(n, K, MOUTH_JOB_WORDS, device="cpu", dtype=torch.int64)  # host table, every word written below
        idx = torch.arange(n, dtype=torch.int64).view(n, 1)
        t[:, :, 0] = f.data_ptr() + idx * f.stride(0)
        t[:, :, 1] = o.data_ptr() + idx * o.stride(0) + torch.arange(K, dtype=torch.int64).view(1, K) * o.stride(1)
        colour = f.ndim == 4
        t[:, :, 2], t[:, :, 3], t[:, :, 4] = int(f.shape[1]), int(f.shape[2]), int(f.stride(1))
        t[:, :, 5] = (max(int(f.stride(2)), 3) if colour else max(int(f.stride(2)), 1)) + 65536 * (plan["order"] if colour else 0)
        t[:, :, 6:] = A.reshape(n, K, 6).view(torch.int64)
        rows.append(t.view(n * K, MOUTH_JOB_WORDS))
    if not rows:
        return
    table = torch.cat(rows) if len(rows) > 1 else rows[0]
    J = int(table.shape[0])
    capturing = torch.cuda.is_current_stream_capturing()
    last = _MOUTH_TABLES.get(dev)
    if last is not None and last[0].shape == table.shape and torch.equal(last[0], table):
        tab = last[1]
        if capturing:
            _MOUTH_CAPTURED.append(tab)
    elif capturing:
        raise RuntimeError("mouth_rois under HIP-graph capture: the job table cannot be uploaded while capturing; run the same call "
                           "(the same frame, landmark and out= tensors) once before the capture")
    else:
        tab = table.to(dev)  # the one host-to-device copy of the call
        _MOUTH_TABLES[dev] = (table, tab)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().rtfs_mouth_rois_u8(_lib.ptr(tab), _lib.ptr(table), J, Ho, Wo, _lib.stream_of(tab)), "rtfs_mouth_rois_u8")


def mouth_rois(frames, eyes, lips, out_hw=(96, 96), crop_hw=(88, 88), order="bgr", out=None):
    """Whole camera frames + landmarks -> uint8 mouth ROIs on the device, ONE ``rtfs_mouth_rois_u8`` launch (DESIGN.md "Mouth ROIs from
    camera frames"): the reference's ``align_face``, lip box, ``cv2.resize`` and grey (``RTFSNet_file.py:20-73, 111-118``) composed
    into one affine map per (frame, face) (``mouth_affine``) and one bilinear sampling of the frame, bit-equal to
    ``tests/mouth_oracle.py``.  Agreement with the OpenCV chain itself is not measured (``cv2`` is no dependency).

    frames: a uint8 device tensor (n,H,W,3) in ``order`` "bgr" | "rgb", or a grey / luma plane (n,H,W) (any ``order``; "gray" takes
    nothing else).  The channels must be adjacent; row, pixel and frame strides are taken as they lie: nothing is copied.  eyes
    (n,2,2), lips (n,4,2): host arrays as ``mouth_affine`` takes them -> (n,Ho,Wo); with a face axis, eyes (n,K,2,2), lips (n,K,4,2)
    -> (n,K,Ho,Wo), the K faces reading the same frame.  ``out``: a uint8 device tensor of that shape to write into, its (Ho,Wo) planes
    contiguous, any other strides and any alignment; otherwise a new one (``_lib.empty``).

    frames may also be a SEQUENCE of such tensors of different resolutions and channel counts, eyes and lips (and ``out``) sequences
    with one entry per tensor: everything runs in the one launch and a list comes back.

    The default ``out_hw`` is the pools' default ``roi_hw``, whose 4-pixel rim is what ``CenterCrop`` / ``RandomCrop`` cut later; at
    ``out_hw == crop_hw == (88, 88)`` the ROI is the reference's crop.  A tap outside the frame is 0.  Reductions past about 2x alias
    (one bilinear tap set, no area filter).  ValueError - before the launch - for wrong dtypes, devices, ranks or counts, an unknown
    ``order`` and what ``mouth_affine`` refuses.  Capturable in a HIP graph once the same call has run before the capture."""
    single = isinstance(frames, torch.Tensor)
    try:
        fl, el, ll = ([frames], [eyes], [lips]) if single else (list(frames), list(eyes), list(lips))
        ol = None if out is None else ([out] if single else list(out))
    except TypeError:
        raise ValueError("mouth_rois: frames is a tensor or a sequence of tensors, with eyes, lips (and out) sequences of the same length") from None
    if not fl or (ol is not None and len(ol) != len(fl)):
        raise ValueError(f"mouth_rois: {len(fl)} frame tensor(s) and {0 if ol is None else len(ol)} out tensor(s); need at least one, as many")
    plan = _mouth_plan(fl, el, ll, out_hw, crop_hw, order, "mouth_rois")
    if ol is None:
        full = _mouth_alloc(plan)
    else:
        full = []
        for r, (o, (_, A, faces)) in enumerate(zip(ol, plan["items"])):
            if not isinstance(o, torch.Tensor) or o.ndim != (4 if faces else 3):
                raise ValueError(f"mouth_rois: out {r} must be a tensor ({A.shape[0]},{f'{A.shape[1]},' if faces else ''}{plan['hw'][0]},{plan['hw'][1]})")
            full.append(o if faces else o.unsqueeze(1))
    _mouth_run(plan, full)
    res = [o if faces else o.squeeze(1) for o, (_, _, faces) in zip(full, plan["items"])]
    if ol is not None:
        res = ol
    return res[0] if single else res


# ---------------------------------------------------------------- waveform normalisation
def _normalize(mix, src, std, eps):
    lib = _lib.load()
    B, L = int(mix.shape[0]), int(mix.shape[1])
    K = 0 if src is None else int(src.shape[1])
    mo = _lib.empty(B, L, device=mix.device)
    so = None if src is None else _lib.empty(B, K, L, device=mix.device)
    nbytes = lib.rtfs_wav_normalize_workspace_bytes(B, K, L)
    ws = _lib.workspace(nbytes, mix.device)
    _lib.check(lib.rtfs_wav_normalize_f32(_lib.ptr(mix), _lib.ptr(src), _lib.ptr(std), _lib.ptr(mo), _lib.ptr(so), B, K, L, float(eps),
                                          _lib.ptr(ws), nbytes, _lib.stream_of(mix)), "rtfs_wav_normalize_f32")
    return mo, so


def normalize_mixture(mixture, sources=None, eps=1e-8):
    """The dataset's joint form: mixture (L) | (B,L), sources (K,L) | (B,K,L) or None.  Every row gets zero mean and is divided by the
    MIXTURE's unbiased standard deviation + eps.  Returns ``mixture`` alone, or ``(mixture, sources)``."""
    _lib.need_gpu(mixture, sources)
    single = mixture.ndim == 1
    if mixture.ndim not in (1, 2) or mixture.shape[-1] < 1:
        raise ValueError(f"normalize_mixture: mixture must be (L) or (B,L); got {tuple(mixture.shape)}")
    mix = mixture.reshape(-1, mixture.shape[-1]).contiguous()
    src = None
    if sources is not None:
        if sources.ndim != mixture.ndim + 1 or sources.shape[-1] != mix.shape[1] or (not single and sources.shape[0] != mix.shape[0]):
            raise ValueError(f"normalize_mixture: sources {tuple(sources.shape)} do not go with mixture {tuple(mixture.shape)}")
        src = sources.reshape(mix.shape[0], -1, mix.shape[1]).contiguous()
    mo, so = _normalize(mix, src, None, eps)
    mo = mo[0] if single else mo
    if sources is None:
        return mo
    return mo, so.reshape(sources.shape)


def normalize_tensor_wav(wav_tensor, eps=1e-8, std=None):
    """avspeech_dataset.py:18-22: (wav - mean) / (std + eps) over the last axis, ``std`` the row's own unbiased deviation unless one that
    broadcasts against ``wav_tensor.std(-1, keepdim=True)`` is given."""
    _lib.need_gpu(wav_tensor)
    if wav_tensor.ndim < 1 or wav_tensor.shape[-1] < 1:
        raise ValueError(f"normalize_tensor_wav: got shape {tuple(wav_tensor.shape)}")
    L = wav_tensor.shape[-1]
    rows = wav_tensor.reshape(-1, L).contiguous()
    s = None
    if std is not None:
        s = torch.as_tensor(std, dtype=torch.float32, device=rows.device)
        s = s.expand(*wav_tensor.shape[:-1], 1).reshape(-1).contiguous()
    out, _ = _normalize(rows, None, s, eps)
    return out.reshape(wav_tensor.shape)


# ---------------------------------------------------------------- training mixtures (DESIGN.md "Training mixtures")
MIX_MAX_SOURCES, MIX_CHUNK, MIX_MAX_LENGTH = 4, 4096, 1 << 20  # RTFS_MIX_MAX_SOURCES, RTFS_MIX_CHUNK, RTFS_MIX_MAX_LENGTH
MIX_RECIPE_WORDS, MIX_TABLE_WORDS = 8, 4                        # RTFS_MIX_RECIPE_WORDS, RTFS_MIX_TABLE_WORDS
MIX_REASONS = {1: "a bad argument", 2: f"length outside [1, {MIX_MAX_LENGTH}]", 3: f"n_out outside [0, {MIX_MAX_SOURCES}]",
               4: "a segment that leaves its source", 5: "a reference segment that leaves its source", 6: "a row whose slots are all empty",
               7: "a source address that is misaligned for its dtype", 8: "an unknown dtype"}
REVERB_TILE, REVERB_TAP_CHUNK, REVERB_MAX_TAPS = 1024, 768, 16384  # RTFS_REVERB_TILE, RTFS_REVERB_TAP_CHUNK, RTFS_REVERB_MAX_TAPS
REVERB_RECIPE_WORDS, REVERB_JOB_WORDS, MIX_RIR_WORDS = 7, 6, 6     # RTFS_REVERB_RECIPE_WORDS, RTFS_REVERB_JOB_WORDS, RTFS_MIX_RIR_WORDS
REVERB_REASONS = {**MIX_REASONS, 7: "a source or RIR address that is misaligned for its dtype", 9: f"taps outside [1, {REVERB_MAX_TAPS}]",
                  10: "an offset outside [0, taps)"}


class MixRecipe:
    """Which segments make up every row of a batch of mixtures: plain host arrays (B, J), J <= 4, per (row, slot).
    ``src``: index into the list of sources, -1 for an empty slot; ``start``: first sample of the segment; ``a``: the slot's factor
    (float64); ``ref_src`` / ``ref_start``: the reference segment whose energy the slot is scaled to, -1 / 0 for none.  The gain of a
    slot is a, or a sqrt(E(ref) / E(segment)) with a reference (``rtfs_mix_plan``).
    Reverberant mixtures (``mix_batch(..., rirs=...)``): ``rir`` / ``ref_rir`` index the list of room impulse responses the slot's
    segment / its reference is convolved with (-1, the default: dry), ``rir_offset`` / ``ref_offset`` the sample of that response the
    image is aligned to (default 0; ``argmax |h|`` cancels the direct-path delay)."""

    def __init__(self, src, start, a, ref_src=None, ref_start=None, rir=None, ref_rir=None, rir_offset=None, ref_offset=None):
        import numpy as np
        try:
            self.src = np.array(src, dtype=np.int64)
            self.start = np.array(start, dtype=np.int64)
            self.a = np.array(a, dtype=np.float64)
            self.ref_src = np.full(self.src.shape, -1, np.int64) if ref_src is None else np.array(ref_src, dtype=np.int64)
            self.ref_start = np.zeros(self.src.shape, np.int64) if ref_start is None else np.array(ref_start, dtype=np.int64)
            self.rir = np.full(self.src.shape, -1, np.int64) if rir is None else np.array(rir, dtype=np.int64)
            self.ref_rir = np.full(self.src.shape, -1, np.int64) if ref_rir is None else np.array(ref_rir, dtype=np.int64)
            self.rir_offset = np.zeros(self.src.shape, np.int64) if rir_offset is None else np.array(rir_offset, dtype=np.int64)
            self.ref_offset = np.zeros(self.src.shape, np.int64) if ref_offset is None else np.array(ref_offset, dtype=np.int64)
        except (TypeError, ValueError, OverflowError):
            raise ValueError("MixRecipe: src, start, ref_src, ref_start (and rir, ref_rir, rir_offset, ref_offset) are integer arrays "
                             "(B, J) and a a float array (B, J)") from None
        if self.src.ndim != 2 or self.src.shape[0] < 1 or not 1 <= self.src.shape[1] <= MIX_MAX_SOURCES or \
                any(v.shape != self.src.shape for v in (self.start, self.a, self.ref_src, self.ref_start)):
            raise ValueError(f"MixRecipe: five arrays of one shape (B, J) with B >= 1 and 1 <= J <= {MIX_MAX_SOURCES}; got "
                             f"{[tuple(v.shape) for v in (self.src, self.start, self.a, self.ref_src, self.ref_start)]}")
        if any(v.shape != self.src.shape for v in (self.rir, self.ref_rir, self.rir_offset, self.ref_offset)):
            raise ValueError(f"MixRecipe: rir, ref_rir, rir_offset, ref_offset must have the recipe's shape {tuple(self.src.shape)}; got "
                             f"{[tuple(v.shape) for v in (self.rir, self.ref_rir, self.rir_offset, self.ref_offset)]}")

    @property
    def reverberant(self):
        """True if any slot or reference names an RIR."""
        return bool((self.rir >= 0).any() or (self.ref_rir >= 0).any())

    @property
    def shape(self):
        return tuple(int(v) for v in self.src.shape)

    def __repr__(self):
        return f"MixRecipe(B={self.shape[0]}, J={self.shape[1]})"

    @classmethod
    def snr(cls, targets, interferers, starts, snr_db, rirs=None, offsets=None):
        """The target-speaker recipe.  targets (B) source indices, interferers (B, K) source indices (-1: none), starts (B, 1 + K),
        snr_db a scalar, (B) or (B, K).  Slot 0 is the target with a = 1 and no reference; slot j >= 1 an interferer whose reference
        is the row's target segment, with a = 10^(-snr_db / 20): the target lies snr_db above that interferer.
        ``rirs`` (B, 1 + K): the RIR index of every slot (-1: dry), ``offsets`` (B, 1 + K) its alignment sample (default 0); every
        interferer's reference gets the target's RIR and offset, so the SNR holds between the reverberant images."""
        import numpy as np
        try:
            t = np.array(targets, dtype=np.int64).reshape(-1)
            k = np.array(interferers, dtype=np.int64).reshape(t.shape[0], -1)
            s = np.array(starts, dtype=np.int64).reshape(t.shape[0], -1)
            db = np.array(snr_db, dtype=np.float64)
            db = np.broadcast_to(db[:, None] if db.ndim == 1 else db, k.shape)
        except (TypeError, ValueError, OverflowError):
            raise ValueError("MixRecipe.snr: targets (B), interferers (B, K), starts (B, 1 + K), snr_db a scalar, (B) or (B, K)") from None
        if s.shape != (t.shape[0], 1 + k.shape[1]):
            raise ValueError(f"MixRecipe.snr: starts must be {(t.shape[0], 1 + k.shape[1])}; got {s.shape}")
        src = np.concatenate([t[:, None], k], axis=1)
        a = np.concatenate([np.ones((t.shape[0], 1)), 10.0 ** (-db / 20.0)], axis=1)
        ref = np.concatenate([np.full((t.shape[0], 1), -1, np.int64), np.where(k >= 0, t[:, None], -1)], axis=1)
        ref_start = np.concatenate([np.zeros((t.shape[0], 1), np.int64), np.where(k >= 0, s[:, :1], 0)], axis=1)
        if rirs is None and offsets is None:
            return cls(src, s, a, ref, ref_start)
        try:
            rr = np.full(src.shape, -1, np.int64) if rirs is None else np.array(rirs, dtype=np.int64).reshape(t.shape[0], -1)
            oo = np.zeros(src.shape, np.int64) if offsets is None else np.array(offsets, dtype=np.int64).reshape(t.shape[0], -1)
        except (TypeError, ValueError, OverflowError):
            raise ValueError("MixRecipe.snr: rirs and offsets are integer arrays (B, 1 + K)") from None
        if rr.shape != src.shape or oo.shape != src.shape:
            raise ValueError(f"MixRecipe.snr: rirs and offsets must be {src.shape}; got {rr.shape}, {oo.shape}")
        rr = np.where(src >= 0, rr, -1)
        oo = np.where(rr >= 0, oo, 0)
        ref_rir = np.where(ref >= 0, rr[:, :1], -1)
        return cls(src, s, a, ref, ref_start, rr, ref_rir, oo, np.where(ref_rir >= 0, oo[:, :1], 0))

    @classmethod
    def lufs(cls, srcs, starts, target_lufs, utter_lufs, rirs=None, offsets=None):
        """Levels by loudness (DESIGN.md "Loudness"): srcs (B, J) source indices (-1: an empty slot), starts (B, J), target_lufs a
        scalar, (B) or (B, J), utter_lufs a host sequence with the integrated loudness of every WHOLE utterance (``loudness_many``,
        measured once per dataset).  Every slot has the fixed gain a = 10^((target - utter_lufs[src]) / 20) and no reference segment:
        the level does not move with the crop.  ``rirs`` / ``offsets`` (B, J) as in ``snr``; the level is that of the dry utterance.
        ValueError naming the source for an utterance whose loudness is not finite (silence reads -inf)."""
        import numpy as np
        try:
            src = np.array(srcs, dtype=np.int64)
            s = np.array(starts, dtype=np.int64)
            tg = np.array(target_lufs, dtype=np.float64)
            tg = np.broadcast_to(tg[:, None] if tg.ndim == 1 else tg, src.shape)
            ul = np.array(utter_lufs, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError, OverflowError):
            raise ValueError("MixRecipe.lufs: srcs and starts (B, J), target_lufs a scalar, (B) or (B, J), utter_lufs one value per source") from None
        if src.ndim != 2 or s.shape != src.shape:
            raise ValueError(f"MixRecipe.lufs: srcs and starts must be one shape (B, J); got {src.shape}, {s.shape}")
        if src.size and (src.max() >= ul.shape[0] or src.min() < -1):
            raise ValueError(f"MixRecipe.lufs: srcs names a source outside [-1, {ul.shape[0]})")
        for i in np.unique(src[src >= 0]):
            if not np.isfinite(ul[i]):
                raise ValueError(f"MixRecipe.lufs: source {int(i)} has loudness {ul[i]}; a level by loudness needs a finite one")
        if not np.isfinite(tg[src >= 0]).all():
            raise ValueError("MixRecipe.lufs: target_lufs must be finite")
        a = np.where(src >= 0, 10.0 ** ((tg - ul[np.maximum(src, 0)]) / 20.0), 0.0)
        if rirs is None and offsets is None:
            return cls(src, s, a)
        try:
            rr = np.full(src.shape, -1, np.int64) if rirs is None else np.array(rirs, dtype=np.int64).reshape(src.shape[0], -1)
            oo = np.zeros(src.shape, np.int64) if offsets is None else np.array(offsets, dtype=np.int64).reshape(src.shape[0], -1)
        except (TypeError, ValueError, OverflowError):
            raise ValueError("MixRecipe.lufs: rirs and offsets are integer arrays (B, J)") from None
        if rr.shape != src.shape or oo.shape != src.shape:
            raise ValueError(f"MixRecipe.lufs: rirs and offsets must be {src.shape}; got {rr.shape}, {oo.shape}")
        rr = np.where(src >= 0, rr, -1)
        return cls(src, s, a, rir=rr, rir_offset=np.where(rr >= 0, oo, 0))


def draw_mix_recipe(lengths, batch, length, n_src=2, snr_db=(-5.0, 5.0), align=1, rng=None, n_rirs=None, rir_prob=1.0, rir_offsets=None,
                    loudness=None, utter_lufs=None):
    """A drawn target-speaker recipe (``MixRecipe.snr``) for ``batch`` rows of ``length`` samples out of utterances of ``lengths``
    samples: per row ``n_src`` distinct utterances (the first is the target), per utterance a uniform start that is a multiple of
    ``align``, per interferer a uniform SNR in ``snr_db`` = (low, high).  Draws come from ``rng`` (a ``random.Random``) or the ``random``
    module, per row in the order utterances, starts, SNRs.  An utterance shorter than ``length`` is never drawn; ValueError if fewer
    than ``n_src`` are long enough.
    ``n_rirs``: additionally draw, per row after that row's SNRs and per slot, ``rng.random() < rir_prob`` and, if so, an RIR index
    ``rng.randrange(n_rirs)`` (otherwise the slot stays dry); ``rir_offsets``: the alignment sample of every RIR (``load_rirs``'s second
    result; default 0).  Without ``n_rirs`` nothing more is drawn: a seed gives the dry recipe it always gave.
    ``loudness`` = (low, high) with ``utter_lufs`` (the loudness of every whole utterance, ``loudness_many``): levels by loudness
    (``MixRecipe.lufs``) instead of SNRs: in place of the row's SNRs a uniform target in LUFS is drawn per slot, the target speaker's
    included (``n_src`` draws where the SNR form makes ``n_src - 1``).  Without it the draws are the ones above, unchanged."""
    r = random if rng is None else rng
    if (loudness is None) != (utter_lufs is None):
        raise ValueError("draw_mix_recipe: loudness=(low, high) and utter_lufs go together")
    if loudness is not None:
        llo, lhi = (float(v) for v in loudness)
        utter_lufs = [float(v) for v in utter_lufs]
        if len(utter_lufs) != len(lengths):
            raise ValueError(f"draw_mix_recipe: {len(utter_lufs)} loudness value(s) for {len(lengths)} utterance(s)")
    batch, length, n_src, align = operator.index(batch), operator.index(length), operator.index(n_src), operator.index(align)
    lengths = [operator.index(n) for n in lengths]
    lo, hi = (float(v) for v in snr_db)
    if batch < 1 or length < 1 or align < 1 or not 1 <= n_src <= MIX_MAX_SOURCES:
        raise ValueError(f"draw_mix_recipe: batch, length, align >= 1 and 1 <= n_src <= {MIX_MAX_SOURCES}")
    pool = [i for i, n in enumerate(lengths) if n >= length]
    if len(pool) < n_src:
        raise ValueError(f"draw_mix_recipe: {len(pool)} of {len(lengths)} utterance(s) hold {length} samples; a row needs {n_src} distinct ones")
    if n_rirs is not None:
        n_rirs = operator.index(n_rirs)
        rir_offsets = [0] * n_rirs if rir_offsets is None else [operator.index(o) for o in rir_offsets]
        if n_rirs < 1 or len(rir_offsets) != n_rirs:
            raise ValueError(f"draw_mix_recipe: n_rirs >= 1 and one offset per RIR; got n_rirs {n_rirs}, {len(rir_offsets)} offset(s)")
    rows, starts, dbs, rirs = [], [], [], []
    for _ in range(batch):
        row = r.sample(pool, n_src)
        rows.append(row)
        starts.append([align * r.randint(0, (lengths[i] - length) // align) for i in row])
        dbs.append([r.uniform(lo, hi) for _ in row[1:]] if loudness is None else [r.uniform(llo, lhi) for _ in row])
        if n_rirs is not None:
            rirs.append([r.randrange(n_rirs) if r.random() < rir_prob else -1 for _ in row])
    if loudness is not None:
        if n_rirs is None:
            return MixRecipe.lufs(rows, starts, dbs, utter_lufs)
        return MixRecipe.lufs(rows, starts, dbs, utter_lufs, rirs=rirs, offsets=[[rir_offsets[i] if i >= 0 else 0 for i in row] for row in rirs])
    if n_rirs is None:
        return MixRecipe.snr([row[0] for row in rows], [row[1:] for row in rows], starts, dbs)
    return MixRecipe.snr([row[0] for row in rows], [row[1:] for row in rows], starts, dbs, rirs=rirs,
                         offsets=[[rir_offsets[i] if i >= 0 else 0 for i in row] for row in rirs])


def _mix_slots(sources, recipe, length, n_out):
    """The checks of ``mix_batch`` that need no library call and the recipe as ``rtfs_mix_plan`` takes it
    -> (slots (B, 4, 8) int64, a (B, 4) float64, B, L, n_out, device)."""
    import numpy as np
    if not isinstance(recipe, MixRecipe):
        raise ValueError(f"mix_batch: recipe must be a MixRecipe; got {type(recipe).__name__}")
    sources = list(sources)
    device = None
    for i, s in enumerate(sources):
        if not isinstance(s, torch.Tensor) or not s.is_cuda or s.ndim != 1 or s.dtype not in (torch.float32, torch.int16) or \
                (s.numel() > 1 and s.stride(0) != 1):
            raise ValueError(f"mix_batch: source {i} must be a 1-D float32 or int16 tensor on the device with adjacent samples (there is "
                             f"no CPU fallback); got {(tuple(s.shape), s.dtype, s.device) if isinstance(s, torch.Tensor) else type(s).__name__}")
        device = s.device if device is None else device
        if s.device != device:
            raise ValueError(f"mix_batch: source {i} lies on {s.device}, source 0 on {device}")
    if not sources:
        raise ValueError("mix_batch: no sources")
    B, Jr = recipe.shape
    L = operator.index(length)
    n_out = Jr if n_out is None else operator.index(n_out)
    if max(int(recipe.src.max()), int(recipe.ref_src.max())) >= len(sources) or min(int(recipe.src.min()), int(recipe.ref_src.min())) < -1:
        raise ValueError(f"mix_batch: the recipe names a source outside [-1, {len(sources)})")
    addr = np.array([s.data_ptr() for s in sources] + [0], dtype=np.int64)  # index -1: the empty slot
    size = np.array([s.numel() for s in sources] + [0], dtype=np.int64)
    kind = np.array([1 if s.dtype == torch.int16 else 0 for s in sources] + [0], dtype=np.int64)
    slots = np.zeros((B, MIX_MAX_SOURCES, MIX_RECIPE_WORDS), np.int64)
    a = np.zeros((B, MIX_MAX_SOURCES), np.float64)
    for w, (idx, start) in enumerate(((recipe.src, recipe.start), (recipe.ref_src, recipe.ref_start))):
        slots[:, :Jr, 4 * w], slots[:, :Jr, 4 * w + 1], slots[:, :Jr, 4 * w + 2] = addr[idx], size[idx], kind[idx]
        slots[:, :Jr, 4 * w + 3] = start
    a[:, :Jr] = recipe.a
    return slots, a, B, L, n_out, device


def _mix_plan(sources, recipe, length, n_out):
    """Everything of a ``mix_batch`` call that needs no launch -> (host table (B*J*4) int64, workspace bytes, B, n_out, device)."""
    slots, a, B, L, n_out, device = _mix_slots(sources, recipe, length, n_out)
    table = _lib.empty(B * MIX_MAX_SOURCES * MIX_TABLE_WORDS, device="cpu", dtype=torch.int64)  # host table, every word written by the plan
    ws, refused = C.c_size_t(0), (C.c_int * 2)(-1, 0)
    code = _lib.load().rtfs_mix_plan(C.c_void_p(slots.ctypes.data), C.c_void_p(a.ctypes.data), B, min(max(L, -1), 1 << 30),
                                     min(max(n_out, -1), 1 << 30), _lib.ptr(table), C.byref(ws), refused)
    if code != 0:
        where = "" if refused[0] < 0 else f" at row {refused[0] // MIX_MAX_SOURCES}, slot {refused[0] % MIX_MAX_SOURCES}"
        raise ValueError(f"mix_batch: {MIX_REASONS.get(refused[1], 'refused')}{where} (B {B}, length {L}, n_out {n_out})")
    return table, int(ws.value), B, n_out, device


def _check_rirs(rirs, device, what):
    """-> (addresses + [0], taps + [0]) of a list of 1-D float32 device RIRs; index -1 is the dry slot."""
    import numpy as np
    rirs = list(rirs)
    for i, h in enumerate(rirs):
        if not isinstance(h, torch.Tensor) or not h.is_cuda or h.ndim != 1 or h.dtype != torch.float32 or \
                (h.numel() > 1 and h.stride(0) != 1) or (device is not None and h.device != device):
            raise ValueError(f"{what}: RIR {i} must be a 1-D float32 tensor with adjacent taps on the sources' device (there is no CPU "
                             f"fallback); got {(tuple(h.shape), h.dtype, h.device) if isinstance(h, torch.Tensor) else type(h).__name__}")
    return (np.array([h.data_ptr() for h in rirs] + [0], dtype=np.int64), np.array([h.numel() for h in rirs] + [0], dtype=np.int64))


def _refused(what, refused, rows, detail):
    where = "" if refused[0] < 0 else (f" at row {refused[0] // MIX_MAX_SOURCES}, slot {refused[0] % MIX_MAX_SOURCES}" if rows
                                       else f" at job {refused[0]}")
    return ValueError(f"{what}: {REVERB_REASONS.get(refused[1], 'refused')}{where} ({detail})")


def reverberate(sources, rirs, src, start, rir, length, offset=None):
    """Reverberant images on the device (``rtfs_reverb_f32``; DESIGN.md "Reverberant mixtures"): a host plan, one table upload and ONE
    launch, nothing read back.  Job s convolves ``sources[src[s]]`` (1-D device tensors, float32 or int16 PCM taken as s / 32768, read
    where they lie) with ``rirs[rir[s]]`` (1-D float32 device tensors of 1 .. 16384 taps) and returns, as row s of the (S, length)
    float32 result, r[t] = sum_k h[k] x[start[s] + t + offset[s] - k], t = 0 .. length - 1, summed in float64 and rounded once.  The
    history in front of the segment is the utterance's own; before its first and past its last sample the room is silent.
    ``offset`` (default 0, within [0, taps)): ``argmax |h|`` keeps the image aligned with the dry segment.  There is no CPU fallback;
    what ``rtfs_reverb_plan`` refuses raises ValueError before anything is launched."""
    import numpy as np
    try:
        src, start, rir = (np.array(v, dtype=np.int64).reshape(-1) for v in (src, start, rir))
        offset = np.zeros(src.shape, np.int64) if offset is None else np.array(offset, dtype=np.int64).reshape(-1)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("reverberate: src, start, rir and offset are integer arrays (S)") from None
    S, L = int(src.shape[0]), operator.index(length)
    if S < 1 or any(v.shape != src.shape for v in (start, rir, offset)):
        raise ValueError(f"reverberate: src, start, rir, offset must be four arrays of one length S >= 1; got "
                         f"{[int(v.shape[0]) for v in (src, start, rir, offset)]}")
    recipe = MixRecipe(src[:, None], start[:, None], np.ones((S, 1)))  # the source checks of mix_batch, no library call
    slots, _, _, _, _, dev = _mix_slots(sources, recipe, max(L, 1), 0)
    addr, taps = _check_rirs(rirs, dev, "reverberate")
    if src.min() < 0 or rir.min() < 0 or rir.max() >= len(addr) - 1:
        raise ValueError(f"reverberate: a job names a source outside [0, {len(list(sources))}) or an RIR outside [0, {len(addr) - 1})")
    jobs = np.zeros((S, REVERB_RECIPE_WORDS), np.int64)
    jobs[:, :4] = slots[:, 0, :4]
    jobs[:, 4], jobs[:, 5], jobs[:, 6] = addr[rir], taps[rir], offset
    table = _lib.empty(S * REVERB_JOB_WORDS, device="cpu", dtype=torch.int64)
    refused = (C.c_int * 2)(-1, 0)
    if _lib.load().rtfs_reverb_plan(C.c_void_p(jobs.ctypes.data), S, min(max(L, -1), 1 << 30), _lib.ptr(table), refused) != 0:
        raise _refused("reverberate", refused, False, f"S {S}, length {L}")
    tab = table.to(dev)  # the one host-to-device copy of the call
    images = _lib.empty(S, L, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().rtfs_reverb_f32(_lib.ptr(tab), _lib.ptr(images), S, L, _lib.stream_of(tab)), "rtfs_reverb_f32")
    return images


def _mix_reverb(sources, recipe, length, n_out, normalize, eps, rirs):
    """``mix_batch`` with RIRs: two host plans (count the images, then write the one table), one upload, THREE launches
    -> (mixture, out, stats, images (S, L), image_map (B, Jr) int64 on the host)."""
    import numpy as np
    slots, a, B, L, n_out, dev = _mix_slots(sources, recipe, length, n_out)
    Jr = recipe.shape[1]
    addr, taps = _check_rirs([] if rirs is None else rirs, dev, "mix_batch")
    n = len(addr) - 1
    if max(int(recipe.rir.max()), int(recipe.ref_rir.max())) >= n or min(int(recipe.rir.min()), int(recipe.ref_rir.min())) < -1:
        raise ValueError(f"mix_batch: the recipe names an RIR outside [-1, {n})")
    rr = np.zeros((B, MIX_MAX_SOURCES, MIX_RIR_WORDS), np.int64)
    for w, (idx, off) in enumerate(((recipe.rir, recipe.rir_offset), (recipe.ref_rir, recipe.ref_offset))):
        rr[:, :Jr, 3 * w], rr[:, :Jr, 3 * w + 1], rr[:, :Jr, 3 * w + 2] = addr[idx], taps[idx], off
    lib = _lib.load()
    S, ws, refused = C.c_int(0), C.c_size_t(0), (C.c_int * 2)(-1, 0)
    args = (C.c_void_p(slots.ctypes.data), C.c_void_p(a.ctypes.data), C.c_void_p(rr.ctypes.data), B, min(max(L, -1), 1 << 30),
            min(max(n_out, -1), 1 << 30))
    if lib.rtfs_mix_reverb_plan(*args, 0, None, C.byref(S), C.byref(ws), refused) != 0:
        raise _refused("mix_batch", refused, True, f"B {B}, length {L}, n_out {n_out}")
    S, nbytes = int(S.value), int(ws.value)
    images = _lib.empty(S, L, device=dev)
    table = _lib.empty(S * REVERB_JOB_WORDS + B * MIX_MAX_SOURCES * MIX_TABLE_WORDS, device="cpu", dtype=torch.int64)
    if lib.rtfs_mix_reverb_plan(*args, images.data_ptr() if S else 0, _lib.ptr(table), None, None, refused) != 0:
        raise _refused("mix_batch", refused, True, f"B {B}, length {L}, n_out {n_out}")
    tab = table.to(dev)  # the one host-to-device copy of the call
    mixture = _lib.empty(B, L, device=dev)
    out = _lib.empty(B, n_out, L, device=dev)
    stats = _lib.empty(B, MIX_MAX_SOURCES + 2, device=dev, dtype=torch.float64)
    work = _lib.workspace(nbytes, dev)
    with torch.cuda.device(dev):
        _lib.check(lib.rtfs_mix_reverb_f32(_lib.ptr(tab), S, _lib.ptr(images) if S else None, _lib.ptr(mixture), _lib.ptr(out) if n_out else None,
                                           _lib.ptr(stats), B, L, n_out, 1 if normalize else 0, float(eps), _lib.ptr(work), nbytes,
                                           _lib.stream_of(tab)), "rtfs_mix_reverb_f32")
    # which image row a slot reads: the address the plan put into the slot's table entry (host arithmetic on the host table)
    seg = table[S * REVERB_JOB_WORDS:].numpy().reshape(B, MIX_MAX_SOURCES, MIX_TABLE_WORDS)[:, :Jr, 0]
    image_map = np.where((recipe.rir >= 0) & (recipe.src >= 0), (seg - images.data_ptr()) // (4 * L), -1).astype(np.int64)
    return mixture, out, stats, images, image_map


def mix_batch(sources, recipe, length, n_out=None, normalize=False, eps=1e-8, return_stats=False, rirs=None, return_images=False):
    """Training mixtures formed on the device (``rtfs_mix_f32``; DESIGN.md "Training mixtures"): a host plan, one table upload and TWO
    launches, nothing read back.  ``sources``: a list of 1-D device tensors, float32 or int16 PCM (taken as s / 32768), of any lengths;
    views at any offset are read where they lie, nothing is copied.  ``recipe``: a ``MixRecipe`` (B, J).  Returns mixture (B, length) and
    sources (B, n_out, length), the first ``n_out`` (default J) scaled slots of every row, plus ``stats`` (B, 6) float64
    [the four gains | the mixture's mean | 1 / (std + eps)] with ``return_stats``.  ``normalize``: the dataset's joint normalisation
    (``normalize_mixture``) in the same two launches.  There is no CPU fallback; what ``rtfs_mix_plan`` refuses (a segment that leaves
    its source, an empty row, length outside [1, 2^20], n_out outside [0, 4]) and sources that are not float32 / int16 device vectors
    raise ValueError before anything is launched.
    Reverberant mixtures (DESIGN.md "Reverberant mixtures"): ``rirs``, a list of 1-D float32 device tensors that the recipe's ``rir`` /
    ``ref_rir`` index.  Every distinct (source, start, RIR, offset) is convolved once (``rtfs_reverb_f32``, one more launch in front:
    THREE in all, still one upload) and the mixture definition is applied to the images: gains, SNRs and normalisation are between
    what the room makes of the sources; a slot without an RIR is read dry.  With ``rirs=None`` and a recipe without RIR indices the
    call is the dry one, unchanged.  ``return_images``: also return the (S, length) image tensor and the (B, J) host array of each
    slot's image row, -1 where the slot is dry."""
    if rirs is not None or (isinstance(recipe, MixRecipe) and recipe.reverberant):
        mixture, out, stats, images, image_map = _mix_reverb(sources, recipe, length, n_out, normalize, eps, rirs)
        return (mixture, out) + ((stats,) if return_stats else ()) + ((images, image_map) if return_images else ())
    table, nbytes, B, n_out, dev = _mix_plan(sources, recipe, length, n_out)
    L, lib = int(length), _lib.load()
    tab = table.to(dev)  # the one host-to-device copy of the call
    mixture = _lib.empty(B, L, device=dev)
    out = _lib.empty(B, n_out, L, device=dev)
    stats = _lib.empty(B, MIX_MAX_SOURCES + 2, device=dev, dtype=torch.float64)
    ws = _lib.workspace(nbytes, dev)
    with torch.cuda.device(dev):
        _lib.check(lib.rtfs_mix_f32(_lib.ptr(tab), _lib.ptr(mixture), _lib.ptr(out) if n_out else None, _lib.ptr(stats), B, L, n_out,
                                    1 if normalize else 0, float(eps), _lib.ptr(ws), nbytes, _lib.stream_of(tab)), "rtfs_mix_f32")
    if return_images:
        import numpy as np
        return (mixture, out) + ((stats,) if return_stats else ()) + (_lib.empty(0, L, device=dev), np.full(recipe.shape, -1, np.int64))
    return (mixture, out, stats) if return_stats else (mixture, out)


def load_rirs(rirs, device="cuda"):
    """Room impulse responses for ``reverberate`` / ``mix_batch``: a list of 1-D float32 host arrays (numpy or torch, 1 .. 16384 taps)
    -> (a list of device views into ONE allocation, uploaded with one copy, and the list of ``argmax |h|``, the direct-path sample of
    each, for ``offset`` / ``rir_offsets``).  A host helper: run it once when the RIR set is loaded, not per batch."""
    hs = []
    for i, h in enumerate(rirs):
        t = torch.as_tensor(h)
        if t.ndim != 1 or t.dtype != torch.float32 or t.is_cuda or not 1 <= t.numel() <= REVERB_MAX_TAPS:
            raise ValueError(f"load_rirs: RIR {i} must be a 1-D float32 host array of 1 .. {REVERB_MAX_TAPS} taps; got "
                             f"{(tuple(t.shape), t.dtype, t.device)}")
        hs.append(t)
    if not hs:
        raise ValueError("load_rirs: no RIRs")
    flat = torch.cat(hs).to(device)
    views, at = [], 0
    for t in hs:
        views.append(flat[at:at + t.numel()])
        at += t.numel()
    return views, [int(t.abs().argmax()) for t in hs]


def synthetic_rir(n_taps, t60, sample_rate=16000, delay=0, drr_db=0.0, rng=None):
    """A stand-in RIR for tests, the benchmark and ``tools/train_synthetic.py --reverb``; NOT a room simulation.  -> float32 numpy
    array (n_taps): a unit direct path at sample ``delay`` plus, behind it, Gaussian noise under an exponential envelope that falls by
    60 dB in ``t60`` seconds, scaled so that the direct-to-reverberant energy ratio is ``drr_db``.  ``rng``: a ``numpy.random.RandomState``
    (default: seed 0).  The tail is scaled below the direct path where needed, so ``argmax |h|`` is ``delay``."""
    import numpy as np
    n_taps, delay = operator.index(n_taps), operator.index(delay)
    if not 1 <= n_taps <= REVERB_MAX_TAPS or not 0 <= delay < n_taps or not float(t60) > 0 or not float(sample_rate) > 0:
        raise ValueError(f"synthetic_rir: 1 <= n_taps <= {REVERB_MAX_TAPS}, 0 <= delay < n_taps, t60 > 0, sample_rate > 0")
    rng = np.random.RandomState(0) if rng is None else rng
    h = np.zeros(n_taps, np.float64)
    n = n_taps - delay - 1
    if n > 0:
        tail = rng.randn(n) * np.exp(-3.0 * np.log(10.0) * np.arange(1, n + 1) / (float(t60) * float(sample_rate)))
        e = float(tail @ tail)
        if e > 0:
            tail *= np.sqrt(10.0 ** (-float(drr_db) / 10.0) / e)
            peak = float(np.abs(tail).max())
            if peak > 0.99:
                tail *= 0.99 / peak
        h[delay + 1:] = tail
    h[delay] = 1.0
    return h.astype(np.float32)


# ---------------------------------------------------------------- loudness (DESIGN.md "Loudness")
LOUD_MAX_LENGTH, LOUD_MIN_RATE, LOUD_MAX_RATE = 1 << 26, 8000, 192000  # RTFS_LOUD_MAX_LENGTH, RTFS_LOUD_MIN_RATE, RTFS_LOUD_MAX_RATE
LOUD_RECORD_WORDS, LOUD_HEADER_WORDS, LOUD_TABLE_WORDS = 3, 64, 8      # RTFS_LOUD_RECORD_WORDS, RTFS_LOUD_HEADER_WORDS, RTFS_LOUD_TABLE_WORDS
LOUD_REASONS = {1: "a bad argument", 2: f"a sample rate outside [{LOUD_MIN_RATE}, {LOUD_MAX_RATE}] or no multiple of 10",
                3: "a recording shorter than one 400 ms block", 4: f"a recording longer than {LOUD_MAX_LENGTH} samples",
                5: "an address that is misaligned for its dtype", 6: "an unknown dtype"}


def _loud_plan(wavs, sample_rate, who):
    """Everything of a loudness call that needs no launch: checks the recordings and runs the host planner
    -> (host table int64, (hops, blocks, samples, chunks), workspace bytes, lengths, device)."""
    import numpy as np
    wavs = list(wavs)
    device = None
    for i, w in enumerate(wavs):
        if not isinstance(w, torch.Tensor) or not w.is_cuda or w.ndim != 1 or w.dtype not in (torch.float32, torch.int16) or \
                (w.numel() > 1 and w.stride(0) != 1):
            raise ValueError(f"{who}: recording {i} must be a 1-D float32 or int16 tensor on the device with adjacent samples (there is no "
                             f"CPU fallback); got {(tuple(w.shape), w.dtype, w.device) if isinstance(w, torch.Tensor) else type(w).__name__}")
        device = w.device if device is None else device
        if w.device != device:
            raise ValueError(f"{who}: recording {i} lies on {w.device}, recording 0 on {device}")
    if not wavs:
        raise ValueError(f"{who}: no recordings")
    fs = operator.index(sample_rate)
    R = len(wavs)
    recs = np.array([[w.data_ptr(), w.numel(), 1 if w.dtype == torch.int16 else 0] for w in wavs], dtype=np.int64)
    table = _lib.empty(LOUD_HEADER_WORDS + R * LOUD_TABLE_WORDS, device="cpu", dtype=torch.int64)  # host table, every word written by the plan
    ws, totals, refused = C.c_size_t(0), (C.c_longlong * 4)(), (C.c_int * 2)(-1, 0)
    if _lib.load().rtfs_loudness_plan(C.c_void_p(recs.ctypes.data), R, min(max(fs, -1), 1 << 30), _lib.ptr(table), C.byref(ws), totals, refused) != 0:
        where = "" if refused[0] < 0 else f" at recording {refused[0]} ({int(recs[refused[0], 1])} samples)"
        raise ValueError(f"{who}: {LOUD_REASONS.get(refused[1], 'refused')}{where} (R {R}, sample_rate {fs})")
    return table, tuple(int(v) for v in totals), int(ws.value), [int(n) for n in recs[:, 1]], device


def _loud_measure(table, tab, totals, nbytes, dev, blocks):
    """The four launches -> (out (R, 2) float64 [lufs | kept], z flat float64 or None)."""
    R = (int(table.numel()) - LOUD_HEADER_WORDS) // LOUD_TABLE_WORDS
    out = _lib.empty(R, 2, device=dev, dtype=torch.float64)
    z = _lib.empty(totals[1], device=dev, dtype=torch.float64) if blocks else None
    ws = _lib.workspace(nbytes, dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().rtfs_loudness_f32(_lib.ptr(tab), _lib.ptr(table), _lib.ptr(out), _lib.ptr(z), _lib.ptr(ws), nbytes,
                                                 _lib.stream_of(tab)), "rtfs_loudness_f32")
    return out, z


def loudness_many(wavs, sample_rate, return_kept=False, return_blocks=False):
    """ITU-R BS.1770 integrated loudness of R mono recordings of different lengths in ONE pooled call (``rtfs_loudness_f32``; DESIGN.md
    "Loudness"): a host plan, one table upload and FOUR launches, nothing read back.  ``wavs``: 1-D device tensors, float32 or int16 PCM
    (taken as s / 32768), views at any offset read where they lie; ``sample_rate``: an integer in [8000, 192000] that 10 divides.
    Returns lufs (R,) float64 on the device; with ``return_kept`` also the (R,) int64 count of blocks that passed both gates, with
    ``return_blocks`` also a list of R float64 views, the mean squares z of every recording's 400 ms blocks.  Silence (no block
    passes) reads -inf, a non-finite sample NaN.  Entry r is bit-equal to recording r measured alone.  There is no CPU fallback;
    what ``rtfs_loudness_plan`` refuses (a recording under 400 ms or over 2^26 samples, a rate outside the definition) raises
    ValueError before anything is launched.  Agreement with pyloudnorm or torchaudio is not measured (neither is a dependency; they
    round the block count where this counts complete blocks)."""
    table, totals, nbytes, lengths, dev = _loud_plan(wavs, sample_rate, "loudness_many")
    tab = table.to(dev)  # the one host-to-device copy of the call
    out, z = _loud_measure(table, tab, totals, nbytes, dev, return_blocks)
    res = (out[:, 0],)
    if return_kept:
        res += (out[:, 1].to(torch.int64),)
    if return_blocks:
        H = int(sample_rate) // 10
        res += (list(z.split([n // H - 3 for n in lengths])),)
    return res[0] if len(res) == 1 else res


def _loud_rows(wav, who):
    if not isinstance(wav, torch.Tensor) or wav.ndim not in (1, 2) or (wav.ndim == 2 and wav.shape[0] < 1):
        raise ValueError(f"{who}: wav must be a tensor (L) or (B,L); got {tuple(wav.shape) if isinstance(wav, torch.Tensor) else type(wav).__name__}")
    return [wav] if wav.ndim == 1 else list(wav.unbind(0))


def loudness(wav, sample_rate):
    """Integrated loudness of wav (L) | (B,L), float32 or int16 on the device -> (B,) float64 on the device ((1,) for (L)); the rows
    are the recordings of one ``loudness_many`` call."""
    return loudness_many(_loud_rows(wav, "loudness"), sample_rate)


def loudness_normalize(wav, sample_rate, target=-23.0, return_stats=False):
    """Scale recordings to ``target`` LUFS on the device: the four launches of ``loudness_many`` and ONE more
    (``rtfs_loudness_gain_f32``), out = (float)(x g) with g = 10^((target - lufs) / 20) formed on the device in float64 from the
    device's own lufs: no readback.  ``wav``: a tensor (L) | (B,L) -> a float32 tensor of that shape, or a sequence of 1-D tensors
    of different lengths -> a list of float32 views of one allocation.  A recording whose loudness is not finite (silence, a
    non-finite sample) is copied with g = 1.  ``return_stats``: also (lufs (R,), g (R,)) float64 on the device."""
    single = isinstance(wav, torch.Tensor)
    rows = _loud_rows(wav, "loudness_normalize") if single else list(wav)
    table, totals, nbytes, lengths, dev = _loud_plan(rows, sample_rate, "loudness_normalize")
    tab = table.to(dev)  # the one host-to-device copy of the call
    loud, _ = _loud_measure(table, tab, totals, nbytes, dev, False)
    flat = _lib.empty(totals[2], device=dev)
    g = _lib.empty(len(rows), device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().rtfs_loudness_gain_f32(_lib.ptr(tab), _lib.ptr(table), _lib.ptr(loud), float(target), _lib.ptr(flat), _lib.ptr(g),
                                                      _lib.stream_of(tab)), "rtfs_loudness_gain_f32")
    out = flat.view(wav.shape) if single else list(flat.split(lengths))
    return (out, (loud[:, 0], g)) if return_stats else out


# ---------------------------------------------------------------- mouth-ROI transforms (src/datas/transform.py)
class Normalize:
    """Normalize(mean, std): (frames - mean) / std."""

    def __init__(self, mean, std):
        self.mean, self.std = mean, std

    def __repr__(self):
        return f"{self.__class__.__name__}(mean={self.mean}, std={self.std})"


class CenterCrop:
    def __init__(self, size):
        self.size = size

    def offsets(self, H, W, rng=None):
        th, tw = self.size
        return int(round((H - th)) / 2.0), int(round((W - tw)) / 2.0)  # the reference's rounding: an odd difference truncates

    def __repr__(self):
        return f"{self.__class__.__name__}(size={self.size})"


class RandomCrop:
    def __init__(self, size):
        self.size = size

    def offsets(self, H, W, rng=None):
        r = random if rng is None else rng
        th, tw = self.size
        dx = r.randint(0, W - tw)  # the reference draws the width offset first
        dy = r.randint(0, H - th)
        return dy, dx

    def __repr__(self):
        return f"{self.__class__.__name__}(size={self.size})"


class HorizontalFlip:
    def __init__(self, flip_ratio):
        self.flip_ratio = flip_ratio

    def draw(self, rng=None):
        return 1 if (random if rng is None else rng).random() < self.flip_ratio else 0

    def __repr__(self):
        return f"{self.__class__.__name__}(flip_ratio={self.flip_ratio})"


class Compose:
    """Compose(preprocess): the reference's two chains, [Normalize(0, 255), crop, (HorizontalFlip,) Normalize(mean, std)] with an 88 x 88
    crop, collapse into one offset table and two constants and run as ONE ``rtfs_lips_prepare_u8`` launch; any other chain raises."""

    def __init__(self, preprocess):
        self.preprocess = preprocess

    def __repr__(self):
        return self.__class__.__name__ + "(" + "".join(f"\n    {t}" for t in self.preprocess) + "\n)"

    def collapse(self):
        """-> (crop, flip or None, mean, std); ValueError for a chain the kernel does not express."""
        ts = list(self.preprocess)
        ok = len(ts) in (3, 4) and isinstance(ts[0], Normalize) and isinstance(ts[-1], Normalize) and \
            isinstance(ts[1], (CenterCrop, RandomCrop)) and (len(ts) == 3 or isinstance(ts[2], HorizontalFlip))
        if ok:
            ok = float(ts[0].mean) == 0.0 and float(ts[0].std) == 255.0 and tuple(ts[1].size) == (CROP, CROP) and float(ts[-1].std) != 0.0
        if not ok:
            raise ValueError("Compose: the device path runs the reference's chains only: Normalize(0, 255), CenterCrop | RandomCrop((88, 88)), "
                             f"[HorizontalFlip(r)], Normalize(mean, std); got {self!r}")
        return ts[1], (ts[2] if len(ts) == 4 else None), float(ts[-1].mean), float(ts[-1].std)

    def table(self, N, H, W, rng=None):
        """The (dy, dx, flip) rows of N tracks, drawn per track in the reference's order: dx, dy, flip."""
        crop, flip, _, _ = self.collapse()
        rows = []
        for _ in range(N):
            dy, dx = crop.offsets(H, W, rng)
            rows.append((dy, dx, flip.draw(rng) if flip is not None else 0))
        return rows

    def __call__(self, sample, rng=None, table=None, frame_rate=25):
        """sample uint8 (Tv,H,W) | (N,Tv,H,W) on the device -> float32 (N,1,Tv,88,88).  ``rng``: a ``random.Random`` for the draws (default:
        the ``random`` module); ``table``: explicit (dy, dx, flip) rows instead of the chain's own.  ``frame_rate`` other than 25: the
        track holds the camera's frames at that rate and the result the P(Tv) frames ``frame_rate_map`` selects, in the same launch."""
        _, _, mean, std = self.collapse()
        rate = frame_rate_of(frame_rate)
        if not isinstance(sample, torch.Tensor) or not sample.is_cuda:
            raise RuntimeError("rtfs_net_amd.datas pipelines run on the MI355X only: got a host array (there is no CPU fallback)")
        if sample.dtype != torch.uint8:
            raise RuntimeError(f"rtfs_net_amd.datas pipelines take uint8 mouth ROIs; got {sample.dtype}")
        if sample.ndim == 3:
            sample = sample.unsqueeze(0)
        if sample.ndim != 4 or sample.shape[-2] < CROP or sample.shape[-1] < CROP or sample.shape[0] < 1 or sample.shape[1] < 1:
            raise ValueError(f"mouth ROIs must be (Tv,H,W) or (N,Tv,H,W) with H, W >= {CROP}; got {tuple(sample.shape)}")
        roi = sample.contiguous()
        N, Tv, H, W = (int(v) for v in roi.shape)
        rows = self.table(N, H, W, rng) if table is None else [tuple(int(v) for v in r) for r in table]
        if len(rows) != N or any(len(r) != 3 for r in rows):
            raise ValueError(f"offset table must hold {N} rows of (dy, dx, flip)")
        tab = (C.c_int * (3 * N))(*[v for r in rows for v in r])
        if rate != 25:
            Tv_out = len(frame_rate_map(Tv, rate))
            if Tv_out < 1:
                raise ValueError(f"mouth ROIs of {Tv} frame(s) at {rate} fps hold no 25 fps frame")
            out = _lib.empty(N, 1, Tv_out, CROP, CROP, device=roi.device)
            code = _lib.load().rtfs_lips_prepare_rate_u8(C.c_void_p(roi.data_ptr()), tab, _lib.ptr(out), N, Tv, H, W, mean, std,
                                                         rate.numerator, rate.denominator, _lib.stream_of(roi))
            if code == -4:
                raise ValueError(f"rtfs_lips_prepare_rate_u8: an offset of {rows} leaves the {H} x {W} ROI")
            _lib.check(code, "rtfs_lips_prepare_rate_u8")
            return out
        out = _lib.empty(N, 1, Tv, CROP, CROP, device=roi.device)
        code = _lib.load().rtfs_lips_prepare_u8(C.c_void_p(roi.data_ptr()), tab, _lib.ptr(out), N, Tv, H, W, mean, std, _lib.stream_of(roi))
        if code == -4:
            raise ValueError(f"rtfs_lips_prepare_u8: an offset of {rows} leaves the {H} x {W} ROI")
        _lib.check(code, "rtfs_lips_prepare_u8")
        return out


def get_preprocessing_pipelines():
    """transform.py:151-167: {"train", "val", "test"}, LRW statistics."""
    crop_size = (CROP, CROP)
    mean, std = 0.421, 0.165
    preprocessing = {
        "train": Compose([Normalize(0.0, 255.0), RandomCrop(crop_size), HorizontalFlip(0.5), Normalize(mean, std)]),
        "val": Compose([Normalize(0.0, 255.0), CenterCrop(crop_size), Normalize(mean, std)]),
    }
    preprocessing["test"] = preprocessing["val"]
    return preprocessing
