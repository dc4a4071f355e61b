"""Live streams chunk by chunk: ``AVNet.open_streams`` -> ``StreamPool`` (DESIGN.md "Live streams", "Every face of a stream").

The stateful form of ``AVNet.separate_long``: audio and lip embeddings arrive a chunk at a time, every window of the long-form plan runs
as soon as its samples and its frames are there, and the samples no later window can touch leave at once.  For any way of cutting a
recording into chunks the concatenated outputs equal ``separate_long`` on the whole recording with the same ``window`` / ``hop``.

All arithmetic of a tick (counters, ready windows, ring positions, output ranges) is ``rtfs_live_plan`` (host only); Python keeps four
integers per slot and never reads anything back from the device."""
from __future__ import annotations

import contextlib
import ctypes
import operator

import torch

from . import _lib, models

SPF = 640  # samples per video frame: 16 kHz audio, 25 fps video
FS = 16000  # the model's sample rate
MAX_CAPACITY = 1 << 24  # RTFS_LIVE_MAX_CAPACITY: speakers * (window + max_chunk) at most, so that every launch grid fits
MAX_SPEAKERS = 16  # RTFS_MAX_SPEAKERS: the most targets per mixture rtfs_separator_speakers_f32 fans out to
FACES_PLAN_WORDS = 15  # RTFS_LIVE_FACES_PLAN_WORDS(Kmax) - 2 Kmax: the 13 of PLAN_WORDS | faces present | first target row
PLAN_WORDS = 13  # RTFS_LIVE_PLAN_WORDS: [slot | a | na | f | nf | e | cnt | row0 | o | end | out_off | apos | fpos]
_REASONS = {1: "bad argument", 2: "unknown slot id", 3: "slot named twice", 4: "chunk larger than max_chunk",
            5: "audio ran too far ahead of video: the push would overwrite samples a not-yet-emitted window needs",
            6: "video ran too far ahead of audio: the push would overwrite frames a not-yet-emitted window needs",
            7: "flush of a stream with samples but no video frame", 8: "inconsistent counters", 9: "push to a slot without a face",
            10: "frame rate outside [1, 240] fps or not a fraction of terms up to 2^20", 11: "timebase outside [1, 2^30] ticks per second",
            12: "timestamp outside [0, 2^40) or until outside [0, 2^40]",
            13: "timestamps must increase and none may lie below an earlier until or stamp of the stream",
            14: "more than max_frames model frames would become final at once: advance until in smaller steps"}


def _weights(window, hop, device):
    """The cross-fade weights of ``separate_long`` (models._longform_overlap_add_torch), float32."""
    V = window - hop
    i = torch.arange(window, device=device, dtype=torch.float32)
    return torch.ones_like(i) if V == 0 else torch.minimum(torch.ones_like(i), torch.minimum((i + 0.5) / V, (window - i - 0.5) / V))


def _join(mid, last):
    """The tail of a composite flush: per slot, what the middle push made final in front of the flush's own samples."""
    return [torch.cat([m, t], dim=1) if m.shape[1] else t for m, t in zip(mid, last)]


class _Pool:
    """What every pool shares: the checks of slot ids and ``reset``; for the table-driven pools (``_counters``, ``_reset_state``) also the
    call of their host planner."""

    _WORDS, _NAMES = 4, ("a", "f", "e", "o")  # host counters per slot, and those a refusal shows

    @staticmethod
    def _check_ids(slot_ids):
        try:
            ids = list(slot_ids)
        except TypeError:
            raise ValueError("slot_ids must be a sequence of integers") from None
        try:  # anything that indexes (int, numpy integers, 0-dim integer tensors), but no bool of python, numpy or torch
            if any(isinstance(s, bool) or str(getattr(s, "dtype", "")) in ("bool", "torch.bool") for s in ids):
                raise TypeError
            return [operator.index(s) for s in ids]
        except TypeError:
            raise ValueError(f"slot ids must be integers; got {ids}") from None

    def _check_slots(self, slot_ids):
        ids = self._check_ids(slot_ids)
        if len(set(ids)) != len(ids) or any(not 0 <= s < self.slots for s in ids):
            raise ValueError(f"{type(self).__name__}: slot ids {ids} must be distinct and in [0, {self.slots})")
        return ids

    def reset(self, slot_ids):
        """Drop the named streams without output."""
        ids = self._check_slots(slot_ids)
        if ids:
            self._drop(ids)

    def _drop(self, ids):
        self._reset_state(torch.tensor(ids, dtype=torch.int64).to(self.device), len(ids))
        for s in ids:
            self._counters[s] = [0] * self._WORDS

    def _call_planner(self, fn, ids, inputs, flush, consts, plan_words, n_sizes):
        """One call of the host planner ``fn(slot_ids, counters, *inputs, R, slots, flush, *consts, new_counters, table, sizes, refused)``
        for the named slots; ``inputs`` are the per-slot sizes of a push (NULL at a flush).  -> (new counters, table, sizes) as lists;
        ValueError with the planner's reason for what it refuses.  Nothing is changed."""
        R, W, LL = len(ids), self._WORDS, ctypes.c_longlong
        cnt = [c for s in ids for c in (self._counters[s] if 0 <= s < self.slots else (0,) * W)]
        new, table, sizes, refused = (LL * (W * R))(), (LL * (plan_words * R))(), (LL * n_sizes)(), (ctypes.c_int * 2)()
        rc = fn((LL * R)(*ids), (LL * (W * R))(*cnt), *(None if flush else (LL * R)(*v) for v in inputs), R, self.slots, int(flush), *consts,
                new, table, sizes, refused)
        if rc != 0:
            self._refused(ids, cnt, refused, flush)
        return list(new), list(table), [int(v) for v in sizes]

    def _refused(self, ids, cnt, refused, flush):
        """ValueError with the reason a planner gave in ``refused`` = [index into ids or -1 | RTFS_LIVE_* code]."""
        R, W = len(ids), self._WORDS
        r, why = refused[0], _REASONS.get(refused[1], refused[1])
        at = f" at slot {ids[r]}, counters ({', '.join(self._NAMES)}) = {tuple(cnt[W * r:W * r + len(self._NAMES)])}" if 0 <= r < R else ""
        raise ValueError(f"{type(self).__name__}.{'flush' if flush else 'push'}: refused ({why}){at}; no slot was changed")


class StreamPool(_Pool):
    """``slots`` concurrent live streams on one model (inference only).  Built by ``AVNet.open_streams``.

    A slot has one audio track and ``speakers`` = K lip tracks; this class is K = 1, ``SpeakerStreamPool`` any K.  Per slot the pool
    holds, on the model's device and allocated once: a history ring of C = window + max_chunk samples, K rings of C / 640 lip-embedding
    frames (512 channels), ``_vring`` (slots, K, 512, C / 640), and an overlap accumulator of C floats per row of a window's result
    (``n_src`` rows: the model's sources at K = 1, the K targets otherwise): 4 C (1 + n_src) + 2048 K C / 640 bytes, 717 KB at the
    defaults with n_src 1.  Next to them one tick's framed windows in and out for the most windows a tick can hold,
    slots * (1 + ceil(max_chunk / hop)) rows, the K video windows of a row behind each other.  A push allocates only its flat output, the
    tick table and one chunk's ``forward``.

    Host state is four integers per slot: a samples received, f frames received, e windows emitted, o samples output.  Window n is
    ready when a >= n hop + window and f >= n hop / 640 + window / 640.

    Because each tick uploads a small table (one host-to-device copy), ``push`` / ``flush`` are NOT capturable in a HIP graph."""

    def __init__(self, model, slots, window, hop, max_chunk, max_batch, speakers=1):
        self.model, self.slots, self.window, self.hop, self.max_chunk, self.max_batch = model, slots, window, hop, max_chunk, max_batch
        self.speakers = K = int(speakers)
        self.n_src = int(model.n_src) if K == 1 else K  # K > 1 has a target-speaker model: the plan, the accumulator and the results see K rows
        self.capacity = window + max_chunk
        self.device = next(model.parameters()).device
        self.on_hip = bool(model.fused) and self.device.type == "cuda"
        self._counters = [[0, 0, 0, 0] for _ in range(slots)]
        C, Wv, dev = self.capacity, window // SPF, self.device
        rows_cap = slots * (1 + -(-max_chunk // hop))
        self._aring = _lib.empty(slots, C, device=dev)
        self._vring = _lib.empty(slots, K, 512, C // SPF, device=dev)
        self._acc = _lib.empty(slots, self.n_src, C, device=dev)
        self._xw = _lib.empty(rows_cap, window, device=dev)
        self._vw = _lib.empty(rows_cap * K, 512, Wv, device=dev)
        self._y = _lib.empty(rows_cap, self.n_src, window, device=dev)
        self._reset_state(None, slots)

    # -- public
    def counters(self, slot):
        """(a, f, e, o) of a slot: samples received, frames received, windows emitted, samples output."""
        return tuple(self._counters[int(slot)])

    def push(self, slot_ids, audio_chunks, video_chunks):
        """One chunk of audio and one of lip embeddings for each slot named.  audio chunk (n)|(1,n) float32 with 0 <= n <= max_chunk, video
        chunk (512,m) float32 with 0 <= m <= max_chunk // 640, separate allocations on the pool's device; the two sides need not arrive in
        step and either may be empty.  Returns, per named slot, the (n_src, k) newly final samples (k may be 0): views of one flat output
        whose per-slot blocks start on 128-byte lines.

        Every ready window of every named slot runs in this call, laid out in the order the slots are named, then by window index, through
        ``forward`` in chunks of ``max_batch`` rows.  ValueError - before any launch, all state unchanged - for an unknown or repeated slot
        id, a bad shape / dtype / device, an oversize chunk, or a push that would overwrite history a not-yet-emitted window still needs
        (one side more than ``max_chunk`` ahead of the other).  Not capturable in a HIP graph (the tick table is uploaded per call)."""
        ids, na, nf, wavs, vids = self._check_chunks(slot_ids, audio_chunks, video_chunks)
        return self._tick(ids, na, nf, wavs, vids, flush=False)

    def flush(self, slot_ids):
        """End the named streams: run the windows ``separate_long``'s plan still owes for L = samples received and Tv = frames received
        (zeros past L, a frame index past Tv - 1 reads frame Tv - 1), return the remaining samples up to L per slot, and reset the slots.
        A slot that received nothing returns (n_src, 0); one with samples but no frame raises ValueError (state unchanged)."""
        ids = self._check_ids(slot_ids)
        return self._tick(ids, None, None, None, None, flush=True)

    # -- checks (no launch, no state change)
    def _tracks_of(self, r, v):
        """The lip tracks of video chunk r as a list of ``speakers`` (512,m) tensors; their shapes are checked by the caller."""
        return [v]

    def _check_chunks(self, slot_ids, audio_chunks, video_chunks):
        who = f"{type(self).__name__}.push"
        ids = self._check_ids(slot_ids)
        try:
            audio_chunks, video_chunks = list(audio_chunks), list(video_chunks)
        except TypeError:
            raise ValueError(f"{who}: audio_chunks and video_chunks must be sequences of tensors") from None
        if not len(ids) == len(audio_chunks) == len(video_chunks):
            raise ValueError(f"{who}: {len(ids)} slot id(s), {len(audio_chunks)} audio and {len(video_chunks)} video chunk(s)")
        wavs, vids = [], []
        for r, (w, v) in enumerate(zip(audio_chunks, video_chunks)):
            tracks = self._tracks_of(r, v)
            if not isinstance(w, torch.Tensor) or any(not isinstance(t, torch.Tensor) for t in tracks):
                raise ValueError(f"{who}: chunk {r} is not made of tensors")
            if w.ndim not in (1, 2) or (w.ndim == 2 and w.shape[0] != 1):
                raise ValueError(f"{who}: audio chunk {r} must be (n) or (1,n); got {tuple(w.shape)}")
            for t in tracks:
                if t.ndim != 2 or t.shape[0] != 512:
                    raise ValueError(f"{who}: every track of video chunk {r} must be (512,m); got {tuple(t.shape)}")
            for t in (w, *tracks):
                if t.dtype != torch.float32 or t.device != self.device:
                    raise ValueError(f"{who}: chunk {r} is {t.dtype} on {t.device}; the pool is float32 on {self.device}")
            if len({int(t.shape[1]) for t in tracks}) != 1:
                raise ValueError(f"{who}: the tracks of video chunk {r} hold {[int(t.shape[1]) for t in tracks]} frames; "
                                 "all speakers of a slot are pushed with one m")
            wavs.append(w.reshape(-1).contiguous())
            vids.append([t.contiguous() for t in tracks])
        return ids, [int(w.shape[0]) for w in wavs], [int(v[0].shape[1]) for v in vids], wavs, vids

    def _plan(self, ids, na, nf, flush):
        return self._call_planner(_lib.load().rtfs_live_plan, ids, (na, nf), flush, (self.window, self.hop, self.max_chunk, self.n_src),
                                  PLAN_WORDS, 5)

    def _plan_push(self, ids, na, nf):
        """The dry run of a push: ValueError for what the planner refuses.  (The composite pools have the same two methods.)"""
        return self._plan(ids, na, nf, False)

    def _plan_flush(self, ids):
        """The dry run of a flush."""
        return self._plan(ids, None, None, True)

    # -- one tick
    def _tick(self, ids, na, nf, wavs, vids, flush):
        if self.model.training:
            raise RuntimeError(f"{type(self).__name__} is inference only: call .eval() on the model")
        R = len(ids)
        if R == 0:
            return []
        new, table, (rows, floats, max_span, max_na, max_nf) = self._plan(ids, na, nf, flush)
        col = lambda k: table[k * R:(k + 1) * R]  # noqa: E731
        n_src = self.n_src
        with torch.no_grad():
            if self.on_hip:
                out = self._tick_hip(R, table, rows, floats, max_span, max_na, max_nf, wavs, vids, flush)
            else:
                out = self._tick_torch(R, table, rows, floats, wavs, vids, flush)
        for r, s in enumerate(ids):
            self._counters[s] = new[4 * r:4 * r + 4]
        res = []
        for o, end, off in zip(col(8), col(9), col(10)):
            k = end - o
            res.append(out[off:off + n_src * k].view(n_src, k))
        return res

    def _forward_rows(self, rows):
        K, Wv = self.speakers, self.window // SPF
        if K == 1:
            run = self.model.forward if self.on_hip else self.model.forward_modular
            for c0 in range(0, rows, self.max_batch):
                c1 = min(rows, c0 + self.max_batch)
                self._y[c0:c1].copy_(run(self._xw[c0:c1], self._vw[c0:c1]))
            return
        vw = self._vw.view(-1, K, 512, Wv)
        step = max(1, self.max_batch // K)
        for c0 in range(0, rows, step):
            c1 = min(rows, c0 + step)
            if self.on_hip:
                self._y[c0:c1].copy_(self.model.separate_speakers(self._xw[c0:c1], vw[c0:c1]))
            else:  # target k of a window = the model on that window with lips k
                y = self.model.forward_modular(self._xw[c0:c1].repeat_interleave(K, 0), self._vw[c0 * K:c1 * K])
                self._y[c0:c1].copy_(y.view(c1 - c0, K, self.window))

    def _tick_hip(self, R, table, rows, floats, max_span, max_na, max_nf, wavs, vids, flush):
        lib, dev, K = _lib.load(), self.device, self.speakers
        if flush:
            ptrs = [0] * ((1 + K) * R)
        else:  # columns [aptr | vptr_0 | .. | vptr_{K-1}]: one device address per (slot, track)
            ptrs = [w.data_ptr() for w in wavs] + [v[k].data_ptr() for k in range(K) for v in vids]
        tab = torch.tensor(table + ptrs, dtype=torch.int64).to(dev)  # the one host-to-device copy of the tick
        st = _lib.stream_of(self._xw)
        _lib.check(lib.rtfs_live_ingest_frame_speakers_f32(_lib.ptr(tab), _lib.ptr(self._aring), _lib.ptr(self._vring), _lib.ptr(self._xw),
                                                           _lib.ptr(self._vw), R, rows, K, max_na, max_nf, self.window, self.hop, self.max_chunk,
                                                           st), "rtfs_live_ingest_frame_speakers_f32")
        self._forward_rows(rows)
        out = _lib.empty(floats, device=dev)
        if max_span > 0:
            _lib.check(lib.rtfs_live_overlap_add_f32(_lib.ptr(tab), _lib.ptr(self._y), _lib.ptr(out), _lib.ptr(self._acc), R, max_span, self.n_src,
                                                     self.window, self.hop, self.max_chunk, int(flush), st), "rtfs_live_overlap_add_f32")
        if flush:
            self._reset_state(tab[:R], R)
        return out

    def _reset_state(self, ids, R):
        """Give the state of R slots (a device tensor of ids; None = the first R) defined contents.  No kernel reads a cell it was not
        told by the counters to hold data, so nothing depends on these zeros; they keep one stream's samples out of the next one's
        buffers and make every later read one of written memory."""
        if not self.on_hip:
            sel = slice(0, R) if ids is None else ids
            for t in (self._aring, self._vring, self._acc):
                t[sel] = 0
            return
        # one track and n_src accumulator rows, or K of each
        name = "rtfs_live_reset_f32" if self.speakers == 1 else "rtfs_live_reset_speakers_f32"
        _lib.check(getattr(_lib.load(), name)(_lib.ptr(ids), _lib.ptr(self._aring), _lib.ptr(self._vring), _lib.ptr(self._acc), R, self.n_src,
                                              self.window, self.max_chunk, _lib.stream_of(self._aring)), name)

    # -- the same tick in torch ops (fused = False, CPU tensors): ingest, gather from the rings, accumulate window by window
    def _tick_torch(self, R, table, rows, floats, wavs, vids, flush):
        self._frame_torch(R, table, wavs, vids, flush)
        self._forward_rows(rows)
        return self._overlap_add_torch(R, table, floats, flush)

    def _frame_torch(self, R, table, wavs, vids, flush):
        W, H, C, K, dev = self.window, self.hop, self.capacity, self.speakers, self.device
        Cv, Wv, Hv = C // SPF, W // SPF, H // SPF
        slot, a0, na, f0, nf, e0, cnt, row0, o0, end, off, apos, fpos = (table[k * R:(k + 1) * R] for k in range(PLAN_WORDS))
        iw, ifr = torch.arange(W, device=dev), torch.arange(Wv, device=dev)
        for r in range(R):
            if not flush:  # sequential here, so the windows can be gathered from the rings after the chunks went in
                self._aring[slot[r], (apos[r] + torch.arange(na[r], device=dev)) % C] = wavs[r]
                for k in range(K):
                    self._vring[slot[r], k][:, (fpos[r] + torch.arange(nf[r], device=dev)) % Cv] = vids[r][k]
            lim_a, lim_f = a0[r] + na[r], f0[r] + nf[r]
            for n in range(e0[r], e0[r] + cnt[r]):
                row, p = row0[r] + n - e0[r], n * H + iw
                self._xw[row] = torch.where(p < lim_a, self._aring[slot[r], p % C], torch.zeros((), device=dev))
                for k in range(K):  # the audio once, the K video windows of the row behind each other
                    self._vw[row * K + k] = self._vring[slot[r], k][:, (n * Hv + ifr).clamp(max=lim_f - 1) % Cv]

    def _overlap_add_torch(self, R, table, floats, flush):
        W, H, C, n_src, dev = self.window, self.hop, self.capacity, self.n_src, self.device
        slot, a0, na, f0, nf, e0, cnt, row0, o0, end, off, apos, fpos = (table[k * R:(k + 1) * R] for k in range(PLAN_WORDS))
        iw = torch.arange(W, device=dev)
        out = _lib.empty(floats, device=dev)
        w, V = _weights(W, H, dev), W - H
        for r in range(R):
            acc = self._acc[slot[r]]
            for n in range(e0[r], e0[r] + cnt[r]):  # ascending n; a cell no earlier window reached starts from this window's term
                wy, idx = w * self._y[row0[r] + n - e0[r]], (n * H + iw) % C
                first = V if n > 0 else 0
                acc[:, idx[:first]] += wy[:, :first]
                acc[:, idx[first:]] = wy[:, first:]
            k = end[r] - o0[r]
            if k == 0:
                continue
            den = torch.zeros(k, device=dev)
            for n in range(max(0, -(-(o0[r] - W + 1) // H)), e0[r] + cnt[r]):  # the windows emitted so far that reach [o, end)
                lo, hi = max(o0[r], n * H), min(end[r], n * H + W)
                if lo < hi:
                    den[lo - o0[r]:hi - o0[r]] += w[lo - n * H:hi - n * H]
            t = torch.arange(o0[r], end[r], device=dev)
            out[off[r]:off[r] + n_src * k] = (acc[:, t % C] / den).reshape(-1)
        if flush:
            self._reset_state(torch.tensor(slot, dtype=torch.int64, device=dev), R)
        return out


class SpeakerStreamPool(StreamPool):
    """``slots`` live streams with ``speakers`` = K faces each on one target-speaker model (n_src 1, inference only).  Built by
    ``AVNet.open_streams(..., speakers=K)``; the surface is ``StreamPool``'s, which also holds the state and runs the tick.

    Target k of a slot gets what a ``StreamPool`` gives for the same audio with lips k, but the audio is stored once (one ring), framed
    once per window and, for K > 1, run through the audio-only prefix once per window (``AVNet.separate_speakers`` on
    (rows, K, 512, window / 640) in chunks of max(1, max_batch // K) windows).  Host state stays four integers per slot: the K tracks
    are pushed together with one m, so they share f.  The tick table carries one device address per (slot, speaker): the K chunks of a
    slot are read where they lie, still one table upload per tick."""

    def push(self, slot_ids, audio_chunks, video_chunks):
        """As ``StreamPool.push``, with the video chunk of a slot a (K,512,m) tensor or a sequence of K (512,m) tensors - K separate
        allocations are read where they lie - with one m, 0 <= m <= max_chunk // 640.  Returns, per named slot, the (K, k) newly final
        samples.  ValueError - before any launch, all state unchanged - for what ``StreamPool.push`` refuses, for a wrong number of
        tracks and for tracks that differ in m."""
        return super().push(slot_ids, audio_chunks, video_chunks)

    def _tracks_of(self, r, v):
        K = self.speakers
        if isinstance(v, torch.Tensor):
            if v.ndim != 3:
                raise ValueError(f"SpeakerStreamPool.push: video chunk {r} must be ({K},512,m) or {K} tensors (512,m); got {tuple(v.shape)}")
            tracks = list(v.unbind(0))
        else:
            try:
                tracks = list(v)
            except TypeError:
                raise ValueError(f"SpeakerStreamPool.push: video chunk {r} must be ({K},512,m) or {K} tensors (512,m)") from None
        if len(tracks) != K:
            raise ValueError(f"SpeakerStreamPool.push: video chunk {r} holds {len(tracks)} track(s); the pool has {K} speakers per slot")
        return tracks



class FaceStreamPool(StreamPool):
    """``slots`` live streams whose faces come and go, on one target-speaker model (n_src 1, inference only; DESIGN.md "Faces that come
    and go").  Built by ``AVNet.open_streams(..., max_speakers=Kmax)``.

    Device state is a ``SpeakerStreamPool``'s with K = Kmax: every slot has Kmax PLANES of the video ring and of the accumulator, and a
    *face* is a plane that is in use.  Host state per slot is the four counters plus a birth window per plane (-1 = free); nothing is
    read back.  ``add_face`` / ``drop_face`` are host only, on an idle slot and in mid-stream: a face added when the slot has received
    f frames is born at window b = ceil(f / (hop / 640)), takes part in the windows n >= b only, and its concatenated output equals
    ``separate_long(audio[b hop:], lips[:, b hop / 640:])`` - what a single-track ``StreamPool`` started at that position gives; a
    dropped face's output is the leading part of that.  Each tick runs exactly the (window, face) targets that exist, through
    ``AVNet.separate_speakers(counts=)`` in the chunks of ``models.chunk_windows``; ``flush`` and ``reset`` clear the slot's faces."""

    def __init__(self, model, slots, window, hop, max_chunk, max_batch, max_speakers):
        super().__init__(model, slots, window, hop, max_chunk, max_batch, max_speakers)
        self.max_speakers = self.speakers
        self._births = [[-1] * self.speakers for _ in range(slots)]
        self._yt = self._y.view(-1, window)  # the ragged target rows of a tick

    # -- faces (host only)
    def _slot(self, slot, who):
        s = self._check_ids([slot])[0]
        if not 0 <= s < self.slots:
            raise ValueError(f"FaceStreamPool.{who}: slot {s} is not in [0, {self.slots})")
        return s

    def faces(self, slot):
        """The active face ids of a slot, ascending."""
        return [j for j, b in enumerate(self._births[self._slot(slot, "faces")]) if b >= 0]

    def birth(self, slot, face):
        """The birth window of an active face: its output starts at sample birth * hop of the slot's stream."""
        b = self._births[self._slot(slot, "birth")][operator.index(face)]
        if b < 0:
            raise ValueError(f"FaceStreamPool.birth: face {face} of slot {slot} is not active")
        return b

    def add_face(self, slot, face=None):
        """Declare a face on ``slot`` -> its id (the lowest free plane unless ``face`` names one).  No launch.  From the next push on
        the slot's video chunk carries this face's track too; its first frame is stream frame f.  ValueError when no plane is free or
        the plane is active."""
        s = self._slot(slot, "add_face")
        births = self._births[s]
        if face is None:
            free = [j for j, b in enumerate(births) if b < 0]
            if not free:
                raise ValueError(f"FaceStreamPool.add_face: slot {s} already has max_speakers = {self.max_speakers} faces")
            j = free[0]
        else:
            j = self._check_ids([face])[0]
            if not 0 <= j < self.max_speakers or births[j] >= 0:
                raise ValueError(f"FaceStreamPool.add_face: face {j} of slot {s} is active or not in [0, {self.max_speakers})")
        births[j] = -(-self._counters[s][1] // (self.hop // SPF))
        return j

    def drop_face(self, slot, face):
        """End a face: it takes part in no later tick, what was returned for it is final, its plane is free.  No launch.  ValueError
        for a face that is not active and for the last face of a slot that has received anything (flush or reset that slot)."""
        s = self._slot(slot, "drop_face")
        j = self._check_ids([face])[0]
        births = self._births[s]
        if not 0 <= j < self.max_speakers or births[j] < 0:
            raise ValueError(f"FaceStreamPool.drop_face: face {j} of slot {s} is not active")
        if sum(b >= 0 for b in births) == 1 and (self._counters[s][0] or self._counters[s][1]):
            raise ValueError(f"FaceStreamPool.drop_face: face {j} is the last of slot {s}, which has received data; flush or reset the slot")
        births[j] = -1

    def push(self, slot_ids, audio_chunks, video_chunks):
        """As ``SpeakerStreamPool.push``, with the video chunk of a slot holding one (512,m) track per ACTIVE face in ascending face id - a
        sequence of separate allocations or one (faces,512,m) tensor - with one m.  Returns, per named slot, a dict face id -> (k_j,)
        newly final samples of that face: views of one flat output whose per-slot blocks start on 128-byte lines.  ValueError - before
        any launch, all state unchanged - for what ``StreamPool.push`` refuses, for a slot without a face, a wrong number of tracks and
        tracks that differ in m."""
        return super().push(slot_ids, audio_chunks, video_chunks)

    def flush(self, slot_ids):
        """End the named streams.  A face takes part if the long-form plan of the samples received has a window at or behind its birth
        and it has a frame at or behind that window's start; another face returns (0,).  A slot with samples in which no face takes
        part is refused (state unchanged).  The slots' faces are cleared: a new stream declares them again."""
        return super().flush(slot_ids)

    # -- checks
    def _check_chunks(self, slot_ids, audio_chunks, video_chunks):
        ids = self._check_ids(slot_ids)
        if any(not 0 <= s < self.slots for s in ids):
            raise ValueError(f"FaceStreamPool.push: slot ids {ids} must be in [0, {self.slots})")
        self._expected = [sum(b >= 0 for b in self._births[s]) for s in ids]  # what _tracks_of(r, ..) asks of chunk r
        return super()._check_chunks(ids, audio_chunks, video_chunks)

    def _tracks_of(self, r, v):
        K = self._expected[r] if r < len(self._expected) else 0
        if K == 0:
            raise ValueError(f"FaceStreamPool.push: the slot of chunk {r} has no face; add_face first")
        if isinstance(v, torch.Tensor):
            if v.ndim != 3:
                raise ValueError(f"FaceStreamPool.push: video chunk {r} must be ({K},512,m) or {K} tensors (512,m); got {tuple(v.shape)}")
            tracks = list(v.unbind(0))
        else:
            try:
                tracks = list(v)
            except TypeError:
                raise ValueError(f"FaceStreamPool.push: video chunk {r} must be ({K},512,m) or {K} tensors (512,m)") from None
        if len(tracks) != K:
            raise ValueError(f"FaceStreamPool.push: video chunk {r} holds {len(tracks)} track(s); its slot has {K} active face(s)")
        return tracks

    def _plan_faces(self, ids, na, nf, flush):
        """``rtfs_live_faces_plan`` for the named slots -> (new counters, table, sizes, row_counts).  Nothing is changed."""
        LL, Kmax, cap = ctypes.c_longlong, self.max_speakers, int(self._xw.shape[0])
        births = (LL * (len(ids) * Kmax))(*[b for s in ids for b in (self._births[s] if 0 <= s < self.slots else [-1] * Kmax)])
        row_counts = (LL * cap)()
        plan = _lib.load().rtfs_live_faces_plan
        fn = lambda *a: plan(*a[:15], row_counts, *a[15:])  # noqa: E731  (.., new_counters, table | row_counts | sizes, refused)
        new, table, sizes = self._call_planner(fn, ids, (na, nf), flush, (self.window, self.hop, self.max_chunk, Kmax, births, cap),
                                               FACES_PLAN_WORDS + 2 * Kmax, 6)
        return new, table, sizes, [int(c) for c in row_counts[:sizes[0]]]

    def _plan(self, ids, na, nf, flush):
        return self._plan_faces(ids, na, nf, flush)[:3]

    # -- one tick
    def _present(self, table, R, r):
        """[(plane, birth)] of the faces present in row r of a tick table."""
        Kmax, P = self.max_speakers, table[13 * R + r]
        return [(table[(15 + i) * R + r], table[(15 + Kmax + i) * R + r]) for i in range(P)]

    @staticmethod
    def _target_row(trow0, e, present, n, i):
        """The ragged row of (window n, present face i): the kernels' faces_target_row."""
        return trow0 + sum(max(0, n - max(e, b)) for _, b in present) + sum(b <= n for _, b in present[:i])

    def _tick(self, ids, na, nf, wavs, vids, flush):
        if self.model.training:
            raise RuntimeError("FaceStreamPool is inference only: call .eval() on the model")
        R = len(ids)
        if R == 0:
            return []
        new, table, sizes, row_counts = self._plan_faces(ids, na, nf, flush)
        floats, max_span, max_na, max_nf = sizes[2:]
        with torch.no_grad():
            if self.on_hip:
                out = self._tick_hip(R, table, row_counts, floats, max_span, max_na, max_nf, wavs, vids, flush)
            else:
                out = self._tick_torch(R, table, row_counts, floats, wavs, vids, flush)
        res = []
        for r, s in enumerate(ids):
            o, end, off = table[8 * R + r], table[9 * R + r], table[10 * R + r]
            k, where = end - o, {j: (i, b) for i, (j, b) in enumerate(self._present(table, R, r))}
            views = {}
            for j in self.faces(s):
                if j in where:  # the face's slice of its row of the slot's (P, end - o) block
                    i, b = where[j]
                    views[j] = out[off + i * k + min(k, max(o, b * self.hop) - o):off + (i + 1) * k]
                else:
                    views[j] = out[:0]
            res.append(views)
            self._counters[s] = new[4 * r:4 * r + 4]
            if flush:
                self._births[s] = [-1] * self.max_speakers
        return res

    def _drop(self, ids):
        super()._drop(ids)
        for s in ids:
            self._births[s] = [-1] * self.max_speakers

    def _forward_targets(self, row_counts):
        """The separator on a tick's framed windows: ``_xw[w]`` with ``row_counts[w]`` targets, their lips in ``_vw`` and results in
        ``_yt`` at the ragged target rows.  A window without a target (its faces were dropped, the next is not born yet) is skipped."""
        live = [w for w, c in enumerate(row_counts) if c]
        if not live:
            return
        xw, counts = self._xw[:len(row_counts)], row_counts
        if len(live) != len(row_counts):
            xw, counts = xw[torch.tensor(live, device=self.device)], [row_counts[w] for w in live]
        for w0, w1, t0, t1 in models.chunk_windows(counts, self.max_batch):
            if self.on_hip:
                self._yt[t0:t1].copy_(self.model.separate_speakers(xw[w0:w1], self._vw[t0:t1], counts=counts[w0:w1]))
            else:  # a target = the model on its window with its own lips
                rep = torch.tensor(counts[w0:w1], device=self.device)
                self._yt[t0:t1].copy_(self.model.forward_modular(xw[w0:w1].repeat_interleave(rep, 0), self._vw[t0:t1])[:, 0])

    def _tick_hip(self, R, table, row_counts, floats, max_span, max_na, max_nf, wavs, vids, flush):
        lib, dev, Kmax = _lib.load(), self.device, self.max_speakers
        if flush:
            ptrs = [0] * ((1 + Kmax) * R)
        else:  # columns [aptr | vptr of present face 0 | ..]: the active faces of a push are its present faces, in the order pushed
            ptrs = [w.data_ptr() for w in wavs] + [v[i].data_ptr() if i < len(v) else 0 for i in range(Kmax) for v in vids]
        tab = torch.tensor(table + ptrs, dtype=torch.int64).to(dev)  # the one host-to-device copy of the tick
        st = _lib.stream_of(self._xw)
        _lib.check(lib.rtfs_live_ingest_frame_faces_f32(_lib.ptr(tab), _lib.ptr(self._aring), _lib.ptr(self._vring), _lib.ptr(self._xw),
                                                        _lib.ptr(self._vw), R, len(row_counts), Kmax, max_na, max_nf, self.window, self.hop,
                                                        self.max_chunk, st), "rtfs_live_ingest_frame_faces_f32")
        if row_counts:
            self._forward_targets(row_counts)
        out = _lib.empty(floats, device=dev)
        if max_span > 0:
            _lib.check(lib.rtfs_live_overlap_add_faces_f32(_lib.ptr(tab), _lib.ptr(self._yt), _lib.ptr(out), _lib.ptr(self._acc), R, max_span, Kmax,
                                                           self.window, self.hop, self.max_chunk, int(flush), st),
                       "rtfs_live_overlap_add_faces_f32")
        if flush:
            self._reset_state(tab[:R], R)
        return out

    def _reset_state(self, ids, R):
        if not self.on_hip:
            return super()._reset_state(ids, R)
        _lib.check(_lib.load().rtfs_live_reset_speakers_f32(_lib.ptr(ids), _lib.ptr(self._aring), _lib.ptr(self._vring), _lib.ptr(self._acc), R,
                                                            self.speakers, self.window, self.max_chunk, _lib.stream_of(self._aring)),
                   "rtfs_live_reset_speakers_f32")

    # -- the same tick in torch ops
    def _tick_torch(self, R, table, row_counts, floats, wavs, vids, flush):
        W, H, C, dev = self.window, self.hop, self.capacity, self.device
        Cv, Wv, Hv = C // SPF, W // SPF, H // SPF
        slot, a0, na, f0, nf, e0, cnt, row0, o0, end, off, apos, fpos, _, trow0 = (table[k * R:(k + 1) * R] for k in range(FACES_PLAN_WORDS))
        iw, ifr = torch.arange(W, device=dev), torch.arange(Wv, device=dev)
        present = [self._present(table, R, r) for r in range(R)]
        for r in range(R):
            if not flush:
                self._aring[slot[r], (apos[r] + torch.arange(na[r], device=dev)) % C] = wavs[r]
                for i, (j, _) in enumerate(present[r]):
                    self._vring[slot[r], j][:, (fpos[r] + torch.arange(nf[r], device=dev)) % Cv] = vids[r][i]
            lim_a, lim_f = a0[r] + na[r], f0[r] + nf[r]
            for n in range(e0[r], e0[r] + cnt[r]):
                p = n * H + iw
                self._xw[row0[r] + n - e0[r]] = torch.where(p < lim_a, self._aring[slot[r], p % C], torch.zeros((), device=dev))
                for i, (j, b) in enumerate(present[r]):
                    if b <= n:
                        t = self._target_row(trow0[r], e0[r], present[r], n, i)
                        self._vw[t] = self._vring[slot[r], j][:, (n * Hv + ifr).clamp(max=lim_f - 1) % Cv]
        if row_counts:
            self._forward_targets(row_counts)
        out = _lib.empty(floats, device=dev)
        w, V = _weights(W, H, dev), W - H
        for r in range(R):
            k = end[r] - o0[r]
            for i, (j, b) in enumerate(present[r]):
                acc = self._acc[slot[r], j]
                for n in range(max(e0[r], b), e0[r] + cnt[r]):  # ascending n; a cell no earlier window OF THIS FACE reached starts afresh
                    wy, idx = w * self._yt[self._target_row(trow0[r], e0[r], present[r], n, i)], (n * H + iw) % C
                    first = V if n > b else 0
                    acc[idx[:first]] += wy[:first]
                    acc[idx[first:]] = wy[first:]
                lo = max(o0[r], b * H)
                if lo >= end[r]:
                    continue
                den = torch.zeros(end[r] - lo, device=dev)
                for n in range(max(b, -(-(lo - W + 1) // H)), e0[r] + cnt[r]):
                    u0, u1 = max(lo, n * H), min(end[r], n * H + W)
                    if u0 < u1:
                        den[u0 - lo:u1 - lo] += w[u0 - n * H:u1 - n * H]
                t = torch.arange(lo, end[r], device=dev)
                out[off[r] + i * k + lo - o0[r]:off[r] + (i + 1) * k] = acc[t % C] / den
        if flush:
            self._reset_state(torch.tensor(slot, dtype=torch.int64, device=dev), R)
        return out


def speakers_of(speakers):
    """``speakers`` as an integer in 1 .. MAX_SPEAKERS; ValueError otherwise."""
    try:
        if isinstance(speakers, bool):
            raise TypeError
        K = operator.index(speakers)
    except TypeError:
        raise ValueError(f"open_streams: speakers must be an integer; got {speakers!r}") from None
    if not 1 <= K <= MAX_SPEAKERS:
        raise ValueError(f"open_streams: speakers = {K}; 1 .. {MAX_SPEAKERS} target speakers per stream")
    return K


def _open(cls, model, slots, K, window, hop, max_chunk, max_batch):
    """Check the arguments as ``separate_long`` does, then allocate the pool."""
    slots = int(slots)
    if slots < 1:
        raise ValueError(f"open_streams: slots = {slots}; at least 1")
    window, hop, max_batch, _ = models._window_args(model, "open_streams", window, hop, max_batch)
    max_chunk = window if max_chunk is None else int(max_chunk)
    if not _lib.load().rtfs_live_speakers_sizes_ok(window, hop, max_chunk, K):
        raise ValueError(f"open_streams: max_chunk = {max_chunk} must be a positive multiple of {SPF} with speakers * (window + max_chunk) "
                         f"<= {MAX_CAPACITY} (speakers = {K})")
    return cls(model, slots, window, hop, max_chunk, max_batch, K)


def open_streams(model, slots, window=32000, hop=None, max_chunk=None, max_batch=32, sample_rate=16000):
    """``AVNet.open_streams``: one lip track per slot."""
    if _rate(sample_rate) != FS:
        mc = int(window) if max_chunk is None else int(max_chunk)
        return _open_at_rate(lambda room: open_streams(model, slots, window, hop, mc + room, max_batch), sample_rate, mc)
    return _open(StreamPool, model, slots, 1, window, hop, max_chunk, max_batch)


def open_speaker_streams(model, slots, speakers, window=32000, hop=None, max_chunk=None, max_batch=32, sample_rate=16000):
    """``AVNet.open_streams(speakers=K)`` with K > 1: the checks of ``open_streams`` and those of ``separate_speakers``, then the pool."""
    K = speakers_of(speakers)
    if _rate(sample_rate) != FS:
        raise ValueError(f"open_streams: speakers = {K} with sample_rate = {sample_rate}: a pool with several speakers takes 16 kHz audio only")
    if int(model.n_src) != 1:
        raise ValueError("open_streams: speakers > 1 needs a target-speaker model (n_src 1)")
    return _open(SpeakerStreamPool, model, slots, K, window, hop, max_chunk, max_batch)


def open_face_streams(model, slots, max_speakers, window=32000, hop=None, max_chunk=None, max_batch=32, sample_rate=16000):
    """``AVNet.open_streams(max_speakers=Kmax)``: the checks of ``open_speaker_streams``, then the pool whose faces come and go."""
    try:
        Kmax = speakers_of(max_speakers)
    except ValueError:
        raise ValueError(f"open_streams: max_speakers = {max_speakers!r}; an integer in 1 .. {MAX_SPEAKERS}") from None
    if _rate(sample_rate) != FS:
        raise ValueError(f"open_streams: max_speakers = {Kmax} with sample_rate = {sample_rate}: this pool takes 16 kHz audio only")
    if int(model.n_src) != 1:
        raise ValueError("open_streams: max_speakers needs a target-speaker model (n_src 1)")
    return _open(FaceStreamPool, model, slots, Kmax, window, hop, max_chunk, max_batch)


# ================================================================ live streams from camera frames (DESIGN.md "Live streams from camera frames")
VIDEO_PLAN_WORDS = 8  # RTFS_LIVE_VIDEO_PLAN_WORDS: [slot | g | m | v | k | row0 | out_off | side]
RATE_PLAN_WORDS = 9  # RTFS_LIVE_VIDEO_RATE_PLAN_WORDS: the same in model frames | n0 camera frames received before the push
LOOKAHEAD = 2  # frames: the stem's temporal kernel is 5 with padding 2, so embedding q needs the prepared frames q - 2 .. q + 2
CROP = 88


class LipStreamPool(_Pool):
    """``slots`` concurrent lip tracks embedded chunk by chunk (inference only).  Built by ``FRCNNVideoModel.open_streams``.

    For any way of cutting a track into chunks, the concatenation of what ``push`` and the final ``flush`` return equals
    ``video_model(lips_whole)`` of that track.  Only the stem is temporal, so the state of a slot is its last four prepared frames (two
    buffers of 4 x 88 x 88 floats, read one and write the other: 248 KB per slot) and embeddings lag the frames received by two frames,
    80 ms at 25 fps.  Next to the state the pool holds one tick's stem input, slots * max_frames windows of (5, 94, 94).

    Host state per slot: g frames received, v embeddings emitted (and the side of the history that is current).  All arithmetic of a
    tick is ``rtfs_live_video_plan`` (host only); nothing is read back from the device.  Not capturable in a HIP graph (the tick table
    is uploaded per call)."""

    _WORDS, _NAMES = 3, ("g", "v")
    _PLAN_WORDS = VIDEO_PLAN_WORDS  # the columns of the tick table; the chunk pointers follow them

    def __init__(self, model, slots, max_frames, roi_hw, max_batch_frames):
        self.model, self.slots, self.max_frames, self.roi_hw, self.max_batch_frames = model, slots, max_frames, roi_hw, max_batch_frames
        self.device = next(model.parameters()).device
        self.on_hip = self.device.type == "cuda"
        self._counters = [[0] * self._WORDS for _ in range(slots)]
        self._hist = _lib.empty(slots, 2, 4, CROP, CROP, device=self.device)
        self._win = _lib.empty(slots * max(self._max_model_frames(), LOOKAHEAD), 5, 94, 94, device=self.device)
        self._reset_state(None, slots)

    def _max_model_frames(self):
        """The most model frames one push can complete."""
        return self.max_frames

    # -- public
    def counters(self, slot):
        """(g, v) of a slot: frames received, embeddings emitted."""
        return tuple(self._counters[int(slot)][:2])

    def push(self, slot_ids, chunks):
        """One chunk of mouth frames for each slot named: uint8 ROIs (m,H,W) with (H,W) == roi_hw, which go through the ``"val"`` pipeline
        (centre crop, scale, normalise) inside the ingest launch, or float32 prepared lips (m,88,88), taken as they are; one kind per
        call, 0 <= m <= max_frames, separate allocations on the pool's device.  Returns, per named slot, the (512, k) embeddings that
        became final (k may be 0): views of one flat output.  Embedding q is emitted once frame q + 2 has arrived.

        ValueError - before any launch, all state unchanged - for an unknown or repeated slot id, a bad shape / dtype / device or an
        oversize chunk."""
        ids, ms, chunks, u8 = self._check_chunks(slot_ids, chunks)
        return self._tick(ids, ms, chunks, u8, flush=False)

    def flush(self, slot_ids):
        """End the named tracks: the embeddings still owed, v .. g - 1, with the stem's end padding behind frame g - 1, then reset the slots.
        A slot that received nothing returns (512, 0)."""
        return self._tick(self._check_ids(slot_ids), None, None, False, flush=True)

    # -- checks (no launch, no state change)
    def _check_chunks(self, slot_ids, chunks, *stamps):
        """-> slot ids, what each chunk brings as ``_plan`` takes it (``_sizes``: its frames), the chunks, their kind.  ``stamps``: the
        timestamps and ``until`` of a ``StampLipStreamPool``."""
        ids = self._check_ids(slot_ids)
        try:
            chunks = list(chunks)
        except TypeError:
            raise ValueError("LipStreamPool.push: chunks must be a sequence of tensors") from None
        if len(ids) != len(chunks):
            raise ValueError(f"LipStreamPool.push: {len(ids)} slot id(s) and {len(chunks)} chunk(s)")
        if any(not isinstance(c, torch.Tensor) for c in chunks):
            raise ValueError("LipStreamPool.push: every chunk must be a tensor")
        kinds = {c.dtype for c in chunks}
        if len(kinds) > 1 or (kinds and not kinds <= {torch.uint8, torch.float32}):
            raise ValueError(f"LipStreamPool.push: chunks must be all uint8 ROIs or all float32 prepared lips; got {sorted(map(str, kinds))}")
        u8 = kinds == {torch.uint8}
        hw = self.roi_hw
        for r, c in enumerate(chunks):
            if c.ndim != 3:
                raise ValueError(f"LipStreamPool.push: chunk {r} must be (m,H,W); got {tuple(c.shape)}")
            if c.device != self.device:
                raise ValueError(f"LipStreamPool.push: chunk {r} lies on {c.device}, the pool on {self.device}")
            if u8:
                if hw is None:
                    hw = (int(c.shape[1]), int(c.shape[2]))
                if tuple(c.shape[1:]) != hw or min(hw) < CROP or max(hw) > 0x7fff:
                    raise ValueError(f"LipStreamPool.push: uint8 chunk {r} must be (m,{hw[0]},{hw[1]}) with H, W >= {CROP}; got {tuple(c.shape)}")
            elif tuple(c.shape[1:]) != (CROP, CROP):
                raise ValueError(f"LipStreamPool.push: float32 chunk {r} must be prepared lips (m,{CROP},{CROP}); got {tuple(c.shape)}")
            if c.shape[0] > self.max_frames:
                raise ValueError(f"LipStreamPool.push: chunk {r} holds {c.shape[0]} frames; max_frames = {self.max_frames}")
        ms = self._sizes(chunks, *stamps)
        self._plan(ids, ms, False)  # unknown / repeated ids
        if u8 and self.roi_hw is None:
            self.roi_hw = hw  # fixed by the first ROIs the pool sees
        return ids, ms, [c.contiguous() for c in chunks], u8

    def _sizes(self, chunks):
        return [int(c.shape[0]) for c in chunks]

    def _plan(self, ids, ms, flush):
        if not ids:
            return [], [], [0, 0, 0]
        return self._call_planner(_lib.load().rtfs_live_video_plan, ids, (ms,), flush, (self.max_frames,), VIDEO_PLAN_WORDS, 3)

    # -- one tick
    def _tick(self, ids, ms, chunks, u8, flush):
        if self.model.training:
            raise RuntimeError("LipStreamPool is inference only: call .eval() on the model")
        R = len(ids)
        if R == 0:
            return []
        new, table, sizes = self._plan(ids, ms, flush)
        (rows, floats, max_in), max_m, W = sizes[:3], sizes[-1], self._WORDS  # max_m: the largest m in model frames
        if not self.on_hip:
            raise RuntimeError("rtfs_net_amd kernels run on the MI355X only: the pool lies on a CPU device (there is no CPU fallback)")
        lib, dev = _lib.load(), self.device
        ptrs = [0] * R if flush else [c.data_ptr() for c in chunks]
        with torch.no_grad():
            P = self._PLAN_WORDS * R  # whatever a planner wrote behind its columns (a source list) follows the pointers
            tab = torch.tensor(table[:P] + ptrs + table[P:], dtype=torch.int64).to(dev)  # the one host-to-device copy of the tick
            st = _lib.stream_of(self._win)
            self._ingest(lib, tab, R, rows, max_m, flush, u8, st, max_in)
            out = _lib.empty(floats, device=dev)
            pk = self.model.pack()
            for c0 in range(0, rows, self.max_batch_frames):  # the trunk in pieces: the workspace is ~1.7 MB per frame
                n = min(rows - c0, self.max_batch_frames)
                ws = _lib.workspace(lib.rtfs_video_windows_workspace_bytes(n), dev)
                _lib.check(lib.rtfs_video_frontend_windows_f32(_lib.ptr(self._win), _lib.ptr(pk), _lib.ptr(tab), _lib.ptr(out), R, c0, n,
                                                               _lib.ptr(ws), ws.numel(), st), "rtfs_video_frontend_windows_f32")
            if flush:
                self._reset_state(tab[:R], R)
        for r, s in enumerate(ids):
            self._counters[s] = new[W * r:W * r + W]
        ks, offs = table[4 * R:5 * R], table[6 * R:7 * R]
        return [out[off:off + 512 * k].view(512, k) for k, off in zip(ks, offs)]

    def _ingest(self, lib, tab, R, rows, max_m, flush, u8, st, max_in):
        """The ingest launch of a tick: the chunks (or, at a flush, the end padding) -> the stem windows and the new history."""
        if u8:
            from . import datas
            H, W = self.roi_hw
            crop, _, mean, std = datas.get_preprocessing_pipelines()["val"].collapse()
            dy, dx = crop.offsets(H, W)
            _lib.check(lib.rtfs_live_video_ingest_u8(_lib.ptr(tab), _lib.ptr(self._hist), _lib.ptr(self._win), R, rows, max_m, int(flush), H, W,
                                                     dy, dx, mean, std, st), "rtfs_live_video_ingest_u8")
        else:
            _lib.check(lib.rtfs_live_video_ingest_f32(_lib.ptr(tab), _lib.ptr(self._hist), _lib.ptr(self._win), R, rows, max_m, int(flush), st),
                       "rtfs_live_video_ingest_f32")

    def _reset_state(self, ids, R):
        """Give both history buffers of R slots (a device tensor of ids; None = the first R) defined contents.  Which planes hold a frame
        follows from g, so nothing depends on these zeros."""
        if not self.on_hip:
            self._hist[slice(0, R) if ids is None else ids] = 0
            return
        _lib.check(_lib.load().rtfs_live_video_reset(_lib.ptr(ids), _lib.ptr(self._hist), R, _lib.stream_of(self._hist)), "rtfs_live_video_reset")


class RateLipStreamPool(LipStreamPool):
    """``LipStreamPool`` for a camera at ``frame_rate`` other than 25 fps (DESIGN.md "Live streams at the camera's frame rate").  Built
    by ``FRCNNVideoModel.open_streams(..., frame_rate=...)``.

    Chunks hold CAMERA frames, at most ``max_frames`` of them; the model frames they complete are selected inside the ingest launch by
    the rule of ``datas.frame_rate_map``, so for any chunking the outputs equal those of a ``LipStreamPool`` fed the selected frames of
    the whole track.  A slot keeps one more host counter, n camera frames received; everything downstream counts model frames.  A
    push may complete no model frame (one frame at 60 fps): it returns (512, 0) and leaves the history alone."""

    _WORDS, _NAMES = 4, ("g", "v", "side", "n")
    _PLAN_WORDS = RATE_PLAN_WORDS

    def __init__(self, model, slots, max_frames, roi_hw, max_batch_frames, rate):
        self.frame_rate = rate
        super().__init__(model, slots, max_frames, roi_hw, max_batch_frames)

    def _max_model_frames(self):
        """P(n0 + max_frames) - P(n0) <= ceil(25 max_frames / rate)."""
        return -(-25 * self.max_frames * self.frame_rate.denominator // self.frame_rate.numerator)

    def counters(self, slot):
        """(n, v) of a slot: camera frames received, embeddings emitted."""
        c = self._counters[int(slot)]
        return c[3], c[1]

    def _plan(self, ids, ms, flush):
        if not ids:
            return [], [], [0, 0, 0, 0]
        num, den = self.frame_rate.numerator, self.frame_rate.denominator
        return self._call_planner(_lib.load().rtfs_live_video_rate_plan, ids, (ms,), flush, (self.max_frames, num, den), RATE_PLAN_WORDS, 4)

    def _ingest(self, lib, tab, R, rows, max_m, flush, u8, st, max_in):
        num, den = self.frame_rate.numerator, self.frame_rate.denominator
        if u8:
            from . import datas
            H, W = self.roi_hw
            crop, _, mean, std = datas.get_preprocessing_pipelines()["val"].collapse()
            dy, dx = crop.offsets(H, W)
            _lib.check(lib.rtfs_live_video_ingest_rate_u8(_lib.ptr(tab), _lib.ptr(self._hist), _lib.ptr(self._win), R, rows, max_m, int(flush),
                                                          H, W, dy, dx, mean, std, num, den, st), "rtfs_live_video_ingest_rate_u8")
        else:
            _lib.check(lib.rtfs_live_video_ingest_rate_f32(_lib.ptr(tab), _lib.ptr(self._hist), _lib.ptr(self._win), R, rows, max_m, int(flush),
                                                           num, den, st), "rtfs_live_video_ingest_rate_f32")


STAMP_PLAN_WORDS = 12  # RTFS_LIVE_VIDEO_STAMP_PLAN_WORDS: the nine of the rate plan | hside | offset into the sources | camera frames
MAX_TIMEBASE, MAX_STAMP = 1 << 30, 1 << 40  # FR_MAX_TIMEBASE, FR_MAX_STAMP (csrc/frame_rate.h)


def _stamp(x, what):
    """A timestamp or an ``until`` as a Python int that fits the planner's int64 words; the planner judges its value."""
    try:
        if isinstance(x, bool) or str(getattr(x, "dtype", "")) in ("bool", "torch.bool"):
            raise TypeError
        x = operator.index(x)
    except TypeError:
        raise ValueError(f"StampLipStreamPool: {what} must be integers in the pool's timebase; got {x!r}") from None
    if not -(1 << 62) <= x <= 1 << 62:
        raise ValueError(f"StampLipStreamPool: {what} = {x} is out of range")
    return x


class StampLipStreamPool(LipStreamPool):
    """``LipStreamPool`` for a camera that stamps its frames: dropped frames, a changing rate, a tracker that loses the face (DESIGN.md
    "Live streams with per-frame timestamps").  Built by ``FRCNNVideoModel.open_streams(..., timebase=tb)``.

    Every camera frame comes with an integer capture time in ticks of 1 / ``timebase`` s, increasing within a stream.  Model frame p
    shows the last camera frame whose 25 fps tick is at or before p (the first camera frame before that), whatever the chunking: the
    outputs equal those of a ``LipStreamPool`` fed ``rois[datas.timestamp_map(stamps, timebase, until)]``.  A model frame is final once
    no frame that could change it is still to come: every push moves the slot's watermark W to its last stamp, and ``until`` moves it
    further - the caller's promise that every later frame of the slot is stamped ``>= until``, which keeps a stream going while the
    camera delivers nothing.  Without ``until`` a model frame on the last camera frame's own tick waits for the next frame: one camera
    frame more latency than ``frame_rate=``; with ``until`` at the next frame's nominal time the emission is that pool's.

    Next to the history a slot keeps ``held``, the prepared last camera frame received (two buffers of 88 x 88 floats, read one and
    write the other: 62 KB per slot): a model frame may show it although no earlier model frame did.  Host state per slot: g, v, the
    history side, n camera frames received, the last stamp, W and the held side; ``rtfs_live_video_stamp_plan`` (host only) decides
    which camera frame every new model frame shows and the source list goes up with the tick table in the one copy of a tick."""

    _WORDS, _NAMES = 7, ("g", "v", "side", "n", "last stamp", "W")
    _PLAN_WORDS = STAMP_PLAN_WORDS

    def __init__(self, model, slots, max_frames, roi_hw, max_batch_frames, timebase):
        self.timebase = timebase
        self._held = _lib.empty(slots, 2, CROP, CROP, device=next(model.parameters()).device)
        super().__init__(model, slots, max_frames, roi_hw, max_batch_frames)

    def _max_model_frames(self):
        """A flush emits the frames it finalises, at most max_frames, and the two embeddings that waited for their look-ahead."""
        return self.max_frames + LOOKAHEAD

    # -- public
    def counters(self, slot):
        """(n, v) of a slot: camera frames received, embeddings emitted."""
        c = self._counters[int(slot)]
        return c[3], c[1]

    def push(self, slot_ids, chunks, timestamps, until=None):
        """One chunk of camera frames for each slot named, as ``LipStreamPool.push`` takes them, with ``timestamps``: per named slot the
        m capture times of its chunk (a sequence of ints or a CPU int64 tensor; None for an empty chunk).  ``until``: None, one int for
        every named slot, or per named slot an int or None.  Returns, per named slot, the (512, k) embeddings that became final.

        ValueError - before any launch, all state unchanged - for what ``LipStreamPool.push`` refuses, for stamps that are not m
        integers, do not increase or lie below the slot's last stamp or an earlier ``until``, for a negative stamp or ``until``, and for
        a push that would make more than ``max_frames`` model frames final (advance ``until`` in smaller steps)."""
        ids, ms, chunks, u8 = self._check_chunks(slot_ids, chunks, timestamps, until)
        return self._tick(ids, ms, chunks, u8, flush=False)

    def flush(self, slot_ids, until=None):
        """End the named tracks at g_end = max(g, G(max(W, until)), the last camera frame's tick + 1): the last camera frame is shown
        at least by its own tick.  Returns the embeddings still owed and resets the slots; the next stream of a slot may start at any
        stamp.  A slot that received no frame returns (512, 0)."""
        ids = self._check_ids(slot_ids)
        return self._tick(ids, self._flush_sizes(len(ids), until), None, False, flush=True)

    # -- checks (no launch, no state change)
    @staticmethod
    def _untils(R, until):
        if until is None:
            return [0] * R  # no promise: the watermark is a maximum
        if isinstance(until, (list, tuple)):
            if len(until) != R:
                raise ValueError(f"StampLipStreamPool: {R} slot id(s) and {len(until)} until value(s)")
            return [0 if u is None else _stamp(u, "until") for u in until]
        return [_stamp(until, "until")] * R

    def _flush_sizes(self, R, until):
        return [(0, (), u) for u in self._untils(R, until)]

    def _sizes(self, chunks, timestamps=None, until=None):
        """What each chunk brings, as ``_plan`` takes it: (camera frames, their stamps, until)."""
        R = len(chunks)
        if timestamps is None:
            timestamps = [None] * R
        try:
            timestamps = list(timestamps)
        except TypeError:
            raise ValueError("StampLipStreamPool.push: timestamps must hold one sequence of integers per named slot") from None
        if len(timestamps) != R:
            raise ValueError(f"StampLipStreamPool.push: {R} chunk(s) and {len(timestamps)} timestamp sequence(s)")
        out = []
        for r, (c, ts, u) in enumerate(zip(chunks, timestamps, self._untils(R, until))):
            if isinstance(ts, torch.Tensor):
                if ts.device.type != "cpu" or ts.dtype != torch.int64 or ts.ndim != 1:
                    raise ValueError(f"StampLipStreamPool.push: timestamps {r} must be a CPU int64 tensor (m) or a sequence of ints: stamps are "
                                     f"host data")
                ts = ts.tolist()
            try:
                ts = () if ts is None else tuple(_stamp(t, "timestamps") for t in ts)
            except TypeError:
                raise ValueError(f"StampLipStreamPool.push: timestamps {r} must be a sequence of integers") from None
            if len(ts) != c.shape[0]:
                raise ValueError(f"StampLipStreamPool.push: chunk {r} holds {c.shape[0]} frames and has {len(ts)} timestamp(s)")
            out.append((int(c.shape[0]), ts, u))
        return out

    def _plan(self, ids, ms, flush):
        """``ms``: per named slot (camera frames, stamps, until); None: a flush without ``until``.  The table comes back with the source
        list behind its columns."""
        if not ids:
            return [], [], [0, 0, 0, 0]
        R, W, LL = len(ids), self._WORDS, ctypes.c_longlong
        ms = self._flush_sizes(R, None) if ms is None else ms
        stamps = [t for _, ts, _ in ms for t in ts]
        cnt = [c for s in ids for c in (self._counters[s] if 0 <= s < self.slots else (0,) * W)]
        new, table, src = (LL * (W * R))(), (LL * (STAMP_PLAN_WORDS * R))(), (LL * (self.max_frames * R))()
        sizes, refused = (LL * 5)(), (ctypes.c_int * 2)()
        rc = _lib.load().rtfs_live_video_stamp_plan((LL * R)(*ids), (LL * (W * R))(*cnt), (LL * R)(*(m for m, _, _ in ms)),
                                                    (LL * max(len(stamps), 1))(*stamps), (LL * R)(*(u for _, _, u in ms)), R, self.slots,
                                                    int(flush), self.max_frames, self.timebase, new, table, src, sizes, refused)
        if rc != 0:
            self._refused(ids, cnt, refused, flush)
        return list(new), list(table) + list(src[:sizes[4]]), [int(v) for v in sizes[:4]]

    def _ingest(self, lib, tab, R, rows, max_m, flush, u8, st, max_in):
        if u8:
            from . import datas
            H, W = self.roi_hw
            crop, _, mean, std = datas.get_preprocessing_pipelines()["val"].collapse()
            dy, dx = crop.offsets(H, W)
            _lib.check(lib.rtfs_live_video_ingest_stamp_u8(_lib.ptr(tab), _lib.ptr(self._hist), _lib.ptr(self._held), _lib.ptr(self._win), R, rows,
                                                           max_m, max_in, int(flush), H, W, dy, dx, mean, std, self.timebase, st),
                       "rtfs_live_video_ingest_stamp_u8")
        else:
            _lib.check(lib.rtfs_live_video_ingest_stamp_f32(_lib.ptr(tab), _lib.ptr(self._hist), _lib.ptr(self._held), _lib.ptr(self._win), R, rows,
                                                            max_m, max_in, int(flush), self.timebase, st), "rtfs_live_video_ingest_stamp_f32")

    def _reset_state(self, ids, R):
        """Defined contents for the history and the held planes of R slots; nothing depends on them (held is read only after a push
        wrote it)."""
        if not self.on_hip:
            self._hist[slice(0, R) if ids is None else ids] = 0
            self._held[slice(0, R) if ids is None else ids] = 0
            return
        _lib.check(_lib.load().rtfs_live_video_stamp_reset(_lib.ptr(ids), _lib.ptr(self._hist), _lib.ptr(self._held), R,
                                                           _lib.stream_of(self._hist)), "rtfs_live_video_stamp_reset")


def timebase_of(timebase):
    """``timebase=`` of the entries: None, or the ticks per second of the stamps, an int in [1, 2^30]."""
    if timebase is None:
        return None
    try:
        if isinstance(timebase, bool):
            raise TypeError
        tb = operator.index(timebase)
    except TypeError:
        raise ValueError(f"timebase = {timebase!r}; an integer number of ticks per second") from None
    if not 1 <= tb <= MAX_TIMEBASE:
        raise ValueError(f"timebase = {tb}; between 1 and 2^30 ticks per second")
    return tb


def open_lip_streams(model, slots, max_frames=50, roi_hw=None, max_batch_frames=1600, frame_rate=25, timebase=None):
    """``FRCNNVideoModel.open_streams``: check the arguments, then allocate the pool."""
    from . import datas
    rate, timebase = datas.frame_rate_of(frame_rate), timebase_of(timebase)
    if timebase is not None and rate != 25:
        raise ValueError(f"open_streams: timebase = {timebase} with frame_rate = {rate}: the stamps say when a frame was taken, give one or the other")
    try:
        slots, max_frames, max_batch_frames = operator.index(slots), operator.index(max_frames), operator.index(max_batch_frames)
        roi_hw = None if roi_hw is None else (operator.index(roi_hw[0]), operator.index(roi_hw[1]))
        if roi_hw is not None and len(roi_hw) != 2:
            raise TypeError
    except (TypeError, IndexError):
        raise ValueError("open_streams: slots, max_frames, max_batch_frames must be integers and roi_hw None or (H, W)") from None
    if slots < 1 or max_frames < 1 or max_batch_frames < 1 or slots * max(max_frames, LOOKAHEAD) > 0x7fffffff // 5:
        raise ValueError(f"open_streams: slots = {slots}, max_frames = {max_frames}, max_batch_frames = {max_batch_frames}; all at least 1")
    if roi_hw is not None and (min(roi_hw) < CROP or max(roi_hw) > 0x7fff):
        raise ValueError(f"open_streams: roi_hw = {roi_hw}; mouth ROIs must be at least {CROP} x {CROP}")
    if model.training:
        raise RuntimeError("FRCNNVideoModel.open_streams is inference only: call .eval()")
    if rate != 25:
        if slots * max(-(-25 * max_frames * rate.denominator // rate.numerator), LOOKAHEAD) > 0x7fffffff // 5:
            raise ValueError(f"open_streams: slots = {slots}, max_frames = {max_frames} at {rate} fps: too many frames per tick")
        return RateLipStreamPool(model, slots, max_frames, roi_hw, max_batch_frames, rate)
    if timebase is not None:
        if slots * (max_frames + LOOKAHEAD) > 0x7fffffff // 5:
            raise ValueError(f"open_streams: slots = {slots}, max_frames = {max_frames} with timestamps: too many frames per tick")
        return StampLipStreamPool(model, slots, max_frames, roi_hw, max_batch_frames, timebase)
    return LipStreamPool(model, slots, max_frames, roi_hw, max_batch_frames)


@contextlib.contextmanager
def _counters_as(pool, ids, new, words):
    """Plan a later step of a composite call: inside the block the named slots of ``pool`` carry the counters ``new`` (R x words, as a
    planner returned them); the pool's own are back afterwards, whatever happened."""
    saved = [pool._counters[s] for s in ids]
    try:
        for r, s in enumerate(ids):
            pool._counters[s] = list(new[words * r:words * r + words])
        yield
    finally:
        for s, c in zip(ids, saved):
            pool._counters[s] = c


def _as_list(x):
    """A sequence that is read twice (by the dry run and by the call itself) as a list; anything else as it is, for the checks to name."""
    try:
        return list(x)
    except TypeError:
        return x


class CameraStreamPool(_Pool):
    """``slots`` live streams from microphone samples and camera frames (inference only).  Built by ``System.open_camera_streams``.

    A ``LipStreamPool`` embeds each tick's mouth frames and its embeddings go straight on, as the video chunks, into the audio
    ``StreamPool``; the concatenated outputs equal ``System.separate_recording`` of the whole recording (16 kHz audio) with the same
    ``window`` / ``hop``.  Embeddings lag the frames received by two frames, so audio window n waits for frame n hop / 640 + window / 640 + 1
    (80 ms more than with ready embeddings), and the inner audio pool is opened with ``max_chunk + 1280``: audio in step with the camera
    stands up to 1280 samples further ahead of the EMBEDDED video than window + max_chunk allows for.

    With ``speakers`` = K faces per slot (``SpeakerCameraStreamPool``) the lip pool has slots * K tracks, track s K + k for face k of
    slot s, which move together; here K = 1 and track s is slot s."""

    def __init__(self, lips, audio, max_chunk):
        self.lips, self.audio, self.max_chunk = lips, audio, max_chunk
        self.slots, self.device, self.n_src, self.speakers = audio.slots, audio.device, audio.n_src, audio.speakers

    def _tracks(self, ids):
        K = self.speakers
        return [s * K + k for s in ids for k in range(K)]

    def _group(self, embs):
        """The per-track blocks of a lip tick as the audio pool's video chunks: K per slot (at K = 1 a plain ``StreamPool``: the block)."""
        K = self.speakers
        return embs if K == 1 else [embs[r:r + K] for r in range(0, len(embs), K)]

    def counters(self, slot):
        """((a, f, e, o) of the audio pool, (g, v) of the lip pool - (n, v) with n camera frames at another ``frame_rate``); f == v between
        calls."""
        return self.audio.counters(slot), self.lips.counters(slot)

    def _check_audio(self, ids, audio_chunks):
        who = f"{type(self).__name__}.push"
        try:
            audio_chunks = list(audio_chunks)
        except TypeError:
            raise ValueError(f"{who}: audio_chunks must be a sequence of tensors") from None
        if len(audio_chunks) != len(ids):
            raise ValueError(f"{who}: {len(ids)} slot id(s) and {len(audio_chunks)} audio chunk(s)")
        for r, w in enumerate(audio_chunks):
            if not isinstance(w, torch.Tensor) or w.ndim not in (1, 2) or (w.ndim == 2 and w.shape[0] != 1):
                raise ValueError(f"{who}: audio chunk {r} must be a tensor (n) or (1,n)")
            if w.dtype != torch.float32 or w.device != self.device:
                raise ValueError(f"{who}: audio chunk {r} is {w.dtype} on {w.device}; the pool is float32 on {self.device}")
            if w.numel() > self.max_chunk:
                raise ValueError(f"{who}: audio chunk {r} holds {w.numel()} samples; max_chunk = {self.max_chunk}")
        return audio_chunks

    def _check_rois(self, slot_ids, roi_chunks, *stamps):
        """-> slot ids, and frames per TRACK, chunks per track and their kind as ``LipStreamPool._check_chunks`` returns them."""
        return self.lips._check_chunks(slot_ids, roi_chunks, *stamps)

    def _stamps(self, who, timestamps, until):
        """The timestamps and ``until`` of a push as the lip pool's extra arguments: none unless the pool was opened with ``timebase=``."""
        if isinstance(self.lips, StampLipStreamPool):
            return (timestamps, until)
        if timestamps is not None or until is not None:
            raise ValueError(f"{type(self).__name__}.{who}: timestamps and until need a pool opened with timebase=")
        return ()

    def push(self, slot_ids, audio_chunks, roi_chunks, timestamps=None, until=None):
        """One chunk of 16 kHz audio ((n)|(1,n) float32, 0 <= n <= max_chunk) and one of mouth frames (as ``LipStreamPool.push`` takes them,
        at most max_chunk // 640; at another ``frame_rate`` camera frames, at most ``lips.max_frames``) for each slot named; either may be empty.  Returns, per named slot, the (n_src, k) newly final samples,
        as ``StreamPool.push`` does.  ValueError - before any launch, all state unchanged - for what either pool refuses.

        A pool opened with ``timebase=`` (DESIGN.md "Live streams with per-frame timestamps") takes the frames' capture times and
        ``until`` as ``StampLipStreamPool.push`` does; stamp 0 is audio sample 0.  The audio side counts model frames and is untouched."""
        ids, ms, rois, u8 = self._check_rois(slot_ids, roi_chunks, *self._stamps("push", timestamps, until))
        wavs = self._check_audio(ids, audio_chunks)
        if not ids:
            return []
        self._plan_push(ids, [int(w.numel()) for w in wavs], ms)  # refused here, nothing has moved yet
        if self.audio.model.training:
            raise RuntimeError(f"{type(self).__name__} is inference only: call .eval() on the model")
        embs = self.lips._tick(self._tracks(ids), ms, rois, u8, flush=False)
        return self.audio.push(ids, wavs, self._group(embs))

    # -- whole camera frames (DESIGN.md "Mouth ROIs from camera frames")
    def push_frames(self, slot_ids, audio_chunks, frame_chunks, eyes, lips, order="bgr", crop_hw=(CROP, CROP), timestamps=None, until=None):
        """``push`` from WHOLE camera frames: per named slot one chunk of frames, uint8 (m,H,W,3) in ``order`` "bgr" | "rgb" or a grey
        plane (m,H,W) on the pool's device - any resolution per slot, read where they lie - and that chunk's landmarks, host arrays eyes
        (m,2,2) and lips (m,4,2) as ``datas.mouth_affine`` takes them.  ONE ``rtfs_mouth_rois_u8`` launch cuts the mouth ROIs of all
        named slots at the pool's ``roi_hw`` (the lip box in its central ``crop_hw``); they then go into ``push`` as they are, so the
        outputs are bit-equal to ``push`` fed ``datas.mouth_rois`` of the same frames.  ``timestamps`` / ``until`` pass through on a pool
        opened with ``timebase=``.  At another ``frame_rate`` the chunk holds camera frames and ALL of them are cropped; the ingest
        launch selects afterwards, so at 30 fps about one crop in six is wasted.

        ValueError - before any launch, all state unchanged - for wrong frame or landmark shapes, counts, dtypes or devices, for what
        ``datas.mouth_affine`` refuses and for everything ``push`` refuses (both planners run dry on the chunk sizes first)."""
        audio_chunks = _as_list(audio_chunks)
        ids, plan, rois = self._plan_frames("one", slot_ids, frame_chunks, eyes, lips, order, crop_hw)
        chunks = [v[0] for v in rois]
        self._check_push(ids, audio_chunks, chunks, timestamps, until)
        self._crop(plan, rois)
        return self.push(ids, audio_chunks, chunks, timestamps, until)

    def _plan_frames(self, faces, slot_ids, frame_chunks, eyes, lips, order, crop_hw):
        """The host part of ``push_frames``: -> slot ids, the ``datas`` plan of the one crop launch (checked frames, one affine map per
        frame and face) and per named slot a new, still unwritten ROI tensor (K,m,Ho,Wo).  ``faces``: "one" (landmarks without a face
        axis) or the faces per named slot (a face axis of that length).  Launches nothing and changes nothing."""
        from . import datas
        who = f"{type(self).__name__}.push_frames"
        ids = self._check_slots(slot_ids)
        try:
            frame_chunks, eyes, lips = list(frame_chunks), list(eyes), list(lips)
        except TypeError:
            raise ValueError(f"{who}: frame_chunks, eyes and lips must be sequences with one entry per named slot") from None
        if not (len(ids) == len(frame_chunks) == len(eyes) == len(lips)):
            raise ValueError(f"{who}: {len(ids)} slot id(s), {len(frame_chunks)} frame chunk(s), {len(eyes)} eyes and {len(lips)} lips array(s)")
        if self.lips.roi_hw is None:
            raise ValueError(f"{who}: the pool was opened without roi_hw; the crop needs the ROI size")
        if not ids:
            return ids, None, []
        if faces != "one":  # a sequence of per-face arrays (m,2,2) / (m,4,2) is taken as (m,K,2,2) / (m,K,4,2)
            eyes = [self._face_axis(e) for e in eyes]
            lips = [self._face_axis(l) for l in lips]
        plan = datas._mouth_plan(frame_chunks, eyes, lips, self.lips.roi_hw, crop_hw, order, who, faces=None if faces == "one" else True)
        if plan["device"] != self.device:
            raise ValueError(f"{who}: the frames lie on {plan['device']}, the pool on {self.device}")
        Ho, Wo = plan["hw"]
        for r, (_, A, axis) in enumerate(plan["items"]):
            K = 1 if faces == "one" else faces[r]
            if (faces == "one") == axis or int(A.shape[1]) != K:
                raise ValueError(f"{who}: the landmarks of slot {ids[r]} must name {K} face(s) per frame"
                                 f"{' without a face axis' if faces == 'one' else ''}; got {'a face axis of ' + str(int(A.shape[1])) if axis else 'no face axis'}")
        sizes = [int(A.shape[0]) * int(A.shape[1]) * Ho * Wo for _, A, _ in plan["items"]]
        flat = _lib.empty(sum(sizes), device=self.device, dtype=torch.uint8)
        return ids, plan, [c.view(int(A.shape[1]), int(A.shape[0]), Ho, Wo) for c, (_, A, _) in zip(flat.split(sizes), plan["items"])]

    @staticmethod
    def _face_axis(x):
        if isinstance(x, (list, tuple)) and x and all(getattr(v, "ndim", 0) == 3 for v in x):
            return torch.stack([torch.as_tensor(v, dtype=torch.float64) if not isinstance(v, torch.Tensor) else v.to(torch.float64) for v in x], dim=1)
        return x

    @staticmethod
    def _crop(plan, rois):
        """The one crop launch: ROI tensor (K,m,Ho,Wo) of every named slot <- its frames."""
        if plan is not None:
            from . import datas
            datas._mouth_run(plan, [v.permute(1, 0, 2, 3) for v in rois])

    def _check_push(self, slot_ids, audio_chunks, roi_chunks, timestamps=None, until=None):
        """Everything ``push`` checks before its first launch, on ROI chunks whose contents do not matter yet: shapes, kinds and the dry
        run of both planners.  ValueError for what ``push`` would refuse; nothing is changed."""
        ids, ms, _, _ = self._check_rois(slot_ids, roi_chunks, *self._stamps("push_frames", timestamps, until))
        wavs = self._check_audio(ids, audio_chunks)
        if ids:
            self._plan_push(ids, [int(w.numel()) for w in wavs], ms)
        if self.audio.model.training:
            raise RuntimeError(f"{type(self).__name__} is inference only: call .eval() on the model")

    def _plan_push(self, ids, na, ms):
        """The dry run of a push of na samples per named slot and ms frames per named TRACK on both planners: ValueError for what
        either refuses."""
        K, R = self.speakers, len(ids)
        _, vtab, _ = self.lips._plan(self._tracks(ids), ms, False)
        ks = vtab[4 * R * K:5 * R * K][::K]  # the tracks of a slot share their counters: one k per slot
        gs, mm = vtab[R * K:2 * R * K][::K], vtab[2 * R * K:3 * R * K][::K]  # ... one g and one m, both in model frames
        # frames may run (window + max_chunk) / 640 + 2 ahead of the first window not yet emitted: the two embeddings a flush still owes
        # then always fit the inner pool's ring
        room = (self.audio.window + self.max_chunk) // SPF + LOOKAHEAD
        for s, g, m in zip(ids, gs, mm):
            if g + m - self.audio._counters[s][2] * (self.audio.hop // SPF) > room:
                raise ValueError(f"{type(self).__name__}.push: refused ({_REASONS[6]}) at slot {s}; no slot was changed")
        return self.audio._plan_push(ids, na, ks)

    def flush(self, slot_ids, until=None):
        """End the named streams: the lip pool's flush of the slots' tracks, its at most two remaining embeddings per track pushed with
        empty audio, then the audio pool's flush.  Returns the remaining samples per slot (the samples the middle step made final in
        front of the flush's own).  ``until``: with ``timebase=``, as ``StampLipStreamPool.flush`` takes it."""
        ids = self._check_slots(slot_ids)
        if not ids:
            return []
        ms = self.lips._flush_sizes(len(ids), until) if self._stamps("flush", None, until) else None
        self._plan_flush(ids, ms)
        if self.audio.model.training:
            raise RuntimeError(f"{type(self).__name__} is inference only: call .eval() on the model")
        embs = self.lips._tick(self._tracks(ids), ms, None, False, flush=True)
        empty = _lib.empty(0, device=self.device)
        mid = self.audio.push(ids, [empty] * len(ids), self._group(embs))
        return _join(mid, self.audio.flush(ids))

    def _plan_flush(self, ids, ms=None):
        """The dry run of a flush on both planners: ValueError for what either refuses.  ``ms``: what a ``StampLipStreamPool`` is flushed
        with."""
        K, R = self.speakers, len(ids)
        _, vtab, _ = self.lips._plan(self._tracks(ids), ms, True)
        new, _, _ = self.audio._plan_push(ids, [0] * R, vtab[4 * R * K:5 * R * K][::K])
        with _counters_as(self.audio, ids, new, 4):  # the inner flush is planned on the counters the middle push leaves
            self.audio._plan_flush(ids)

    def _drop(self, ids):
        self.lips.reset(self._tracks(ids))
        self.audio.reset(ids)


class SpeakerCameraStreamPool(CameraStreamPool):
    """``CameraStreamPool`` with ``speakers`` = K faces per slot.  Built by ``System.open_camera_streams(..., speakers=K)``.

    The audio pool is a ``SpeakerStreamPool``: the per-track embedding blocks of a tick go straight on, as the K video chunks of slot s,
    through the per-speaker addresses of the tick table.  The ROI chunk of a slot is (K,m,H,W) uint8 or (K,m,88,88) float32.  For any
    chunking output k of a slot equals ``System.separate_recording(wav, 16000, rois[k])``."""

    def counters(self, slot):
        """((a, f, e, o) of the audio pool, (g, v) of the slot's lip tracks, which move together); f == v between calls."""
        return self.audio.counters(slot), self.lips.counters(int(slot) * self.speakers)

    def push(self, slot_ids, audio_chunks, roi_chunks):
        """As ``CameraStreamPool.push``, with the mouth frames of a slot as ONE tensor (K,m,H,W) uint8 or (K,m,88,88) float32.  Returns,
        per named slot, the (K, k) newly final samples.  ValueError - before any launch, all state unchanged - for what either pool
        refuses and for a chunk that does not hold K tracks."""
        return super().push(slot_ids, audio_chunks, roi_chunks)

    def push_frames(self, slot_ids, audio_chunks, frame_chunks, eyes, lips, order="bgr", crop_hw=(CROP, CROP)):
        """As ``CameraStreamPool.push_frames`` with K faces in every frame: the landmarks of a slot carry a face axis, eyes (m,K,2,2) and
        lips (m,K,4,2).  Still ONE crop launch for all named slots and faces, the K faces of a frame reading the same frame; the ROIs
        are written as the (K,m,H,W) tensor ``push`` takes."""
        audio_chunks = _as_list(audio_chunks)
        ids, plan, rois = self._plan_frames([self.speakers] * len(self._check_slots(slot_ids)), slot_ids, frame_chunks, eyes, lips, order, crop_hw)
        self._check_push(ids, audio_chunks, rois)
        self._crop(plan, rois)
        return self.push(ids, audio_chunks, rois)

    def _check_rois(self, slot_ids, roi_chunks):
        K = self.speakers
        ids = self._check_slots(slot_ids)
        try:
            roi_chunks = list(roi_chunks)
        except TypeError:
            raise ValueError("SpeakerCameraStreamPool.push: roi_chunks must be a sequence of tensors") from None
        if len(roi_chunks) != len(ids):
            raise ValueError(f"SpeakerCameraStreamPool.push: {len(ids)} slot id(s) and {len(roi_chunks)} ROI chunk(s)")
        for r, c in enumerate(roi_chunks):
            if not isinstance(c, torch.Tensor) or c.ndim != 4 or c.shape[0] != K:
                raise ValueError(f"SpeakerCameraStreamPool.push: ROI chunk {r} must be a tensor ({K},m,H,W)")
        return (ids, *self.lips._check_chunks(self._tracks(ids), [t for c in roi_chunks for t in c.contiguous().unbind(0)])[1:])


class FaceCameraStreamPool(CameraStreamPool):
    """``CameraStreamPool`` whose slots hold up to ``max_speakers`` = Kmax faces each.  Built by
    ``System.open_camera_streams(..., max_speakers=Kmax)``.

    The audio pool is a ``FaceStreamPool`` and the lip pool has slots * Kmax tracks, track s Kmax + j for face j of slot s.  The ROI
    chunk of a slot holds one (m,H,W) uint8 block - or one (m,88,88) float32 block - per active face in ascending face id, as a
    sequence or as one tensor with a leading face axis.  ``add_face`` is allowed on an idle slot only: a lip track that joined in
    mid-stream would lag its slot by the stem's two look-ahead frames (DESIGN.md "Faces that come and go", the remaining follow-up).
    ``drop_face`` is allowed at any time and resets the face's lip track.  For any chunking the output of face j of a slot equals
    ``System.separate_recording(wav, 16000, rois[j])``; a dropped face's is the leading part of it."""

    def faces(self, slot):
        return self.audio.faces(slot)

    def add_face(self, slot, face=None):
        s = self.audio._slot(slot, "add_face")
        if any(self.audio._counters[s]) or any(any(self.lips.counters(s * self.speakers + j)) for j in range(self.speakers)):
            raise ValueError(f"FaceCameraStreamPool.add_face: slot {s} is in mid-stream; a face joins a camera stream on an idle slot only")
        return self.audio.add_face(s, face)

    def drop_face(self, slot, face):
        s = self.audio._slot(slot, "drop_face")
        self.audio.drop_face(s, face)
        self.lips.reset([s * self.speakers + self._check_ids([face])[0]])

    def counters(self, slot):
        """((a, f, e, o) of the audio pool, (g, v) of the slot's lip tracks, which move together; (0, 0) without a face)."""
        s, faces = int(slot), self.audio.faces(slot)
        return self.audio.counters(s), self.lips.counters(s * self.speakers + faces[0]) if faces else (0, 0)

    def _slot_tracks(self, ids):
        return [[s * self.speakers + j for j in self.audio.faces(s)] for s in ids]

    def _regroup(self, embs, groups):
        out, at = [], 0
        for g in groups:
            out.append(embs[at:at + len(g)])
            at += len(g)
        return out

    def _check_rois(self, slot_ids, roi_chunks):
        """-> slot ids, the lip tracks of every named slot, and frames per track, chunks per track and their kind."""
        ids = self._check_slots(slot_ids)
        try:
            roi_chunks = list(roi_chunks)
        except TypeError:
            raise ValueError("FaceCameraStreamPool.push: roi_chunks must be a sequence") from None
        if len(roi_chunks) != len(ids):
            raise ValueError(f"FaceCameraStreamPool.push: {len(ids)} slot id(s) and {len(roi_chunks)} ROI chunk(s)")
        groups, flat = self._slot_tracks(ids), []
        for r, (c, g) in enumerate(zip(roi_chunks, groups)):
            if not g:
                raise ValueError(f"FaceCameraStreamPool.push: slot {ids[r]} has no face; add_face first")
            if isinstance(c, torch.Tensor):
                blocks = list(c.contiguous().unbind(0)) if c.ndim == 4 else None
            else:
                try:
                    blocks = list(c)
                except TypeError:
                    blocks = None
            if blocks is None or len(blocks) != len(g) or any(not isinstance(b, torch.Tensor) or b.ndim != 3 for b in blocks):
                raise ValueError(f"FaceCameraStreamPool.push: ROI chunk {r} must hold one (m,H,W) block for each of the {len(g)} active face(s)")
            if len({int(b.shape[0]) for b in blocks}) != 1:
                raise ValueError(f"FaceCameraStreamPool.push: the faces of ROI chunk {r} hold {[int(b.shape[0]) for b in blocks]} frames; one m per slot")
            flat += blocks
        tracks = [t for g in groups for t in g]
        return (ids, groups, *self.lips._check_chunks(tracks, flat)[1:])

    def push_frames(self, slot_ids, audio_chunks, frame_chunks, eyes, lips, order="bgr", crop_hw=(CROP, CROP)):
        """As ``CameraStreamPool.push_frames`` with one landmark entry per ACTIVE face of the slot in ascending face id: eyes
        (m,Ka,2,2) and lips (m,Ka,4,2), or sequences of Ka arrays (m,2,2) / (m,4,2).  Still ONE crop launch for all named slots and
        faces; the ROIs go into ``push`` as one (Ka,m,H,W) tensor per slot."""
        audio_chunks = _as_list(audio_chunks)
        named = self._check_slots(slot_ids)
        for s in named:
            if not self.audio.faces(s):
                raise ValueError(f"FaceCameraStreamPool.push_frames: slot {s} has no face; add_face first")
        ids, plan, rois = self._plan_frames([len(self.audio.faces(s)) for s in named], slot_ids, frame_chunks, eyes, lips, order, crop_hw)
        self._check_push(ids, audio_chunks, rois)
        self._crop(plan, rois)
        return self.push(ids, audio_chunks, rois)

    def _check_push(self, slot_ids, audio_chunks, roi_chunks, timestamps=None, until=None):
        ids, groups, ms, _, _ = self._check_rois(slot_ids, roi_chunks)
        wavs = self._check_audio(ids, audio_chunks)
        if ids:
            self._plan_faces_push(ids, groups, [int(w.numel()) for w in wavs], ms)
        if self.audio.model.training:
            raise RuntimeError("FaceCameraStreamPool is inference only: call .eval() on the model")

    def _plan_faces_push(self, ids, groups, na, ms):
        """The dry run of a push on both planners (ms: frames per track): ValueError for what either refuses."""
        tracks = [t for g in groups for t in g]
        T = len(tracks)
        _, vtab, _ = self.lips._plan(tracks, ms, False)
        ks, at = [], 0
        room = (self.audio.window + self.max_chunk) // SPF + LOOKAHEAD
        for s, g in zip(ids, groups):  # the tracks of a slot share their counters: one k per slot
            ks.append(vtab[4 * T + at])
            if vtab[T + at] + vtab[2 * T + at] - self.audio._counters[s][2] * (self.audio.hop // SPF) > room:  # g + m in model frames
                raise ValueError(f"FaceCameraStreamPool.push: refused ({_REASONS[6]}) at slot {s}; no slot was changed")
            at += len(g)
        return self.audio._plan_push(ids, na, ks)

    def push(self, slot_ids, audio_chunks, roi_chunks):
        """As ``CameraStreamPool.push`` with one block of mouth frames per active face of each slot.  Returns, per named slot, a dict
        face id -> (k_j,) newly final samples.  ValueError - before any launch, all state unchanged - for what either pool refuses,
        for a slot without a face and for a chunk that does not hold one block per active face."""
        ids, groups, ms, rois, u8 = self._check_rois(slot_ids, roi_chunks)
        wavs = self._check_audio(ids, audio_chunks)
        if not ids:
            return []
        self._plan_faces_push(ids, groups, [int(w.numel()) for w in wavs], ms)
        if self.audio.model.training:
            raise RuntimeError("FaceCameraStreamPool is inference only: call .eval() on the model")
        embs = self.lips._tick([t for g in groups for t in g], ms, rois, u8, flush=False)
        return self.audio.push(ids, wavs, self._regroup(embs, groups))

    def flush(self, slot_ids):
        """End the named streams, as ``CameraStreamPool.flush``: per slot a dict face id -> the remaining samples of that face.  A slot
        without a face (it has received nothing) returns {}.  The slots' faces are cleared."""
        named = self._check_slots(slot_ids)
        ids = [s for s in named if self.audio.faces(s)]
        res = {s: {} for s in named}
        if ids:
            groups = self._slot_tracks(ids)
            tracks, R = [t for g in groups for t in g], len(ids)
            _, vtab, _ = self.lips._plan(tracks, None, True)
            firsts = [sum(len(g) for g in groups[:r]) for r in range(R)]
            new, _, _ = self.audio._plan_push(ids, [0] * R, [vtab[4 * len(tracks) + i] for i in firsts])
            with _counters_as(self.audio, ids, new, 4):
                self.audio._plan_flush(ids)
            if self.audio.model.training:
                raise RuntimeError("FaceCameraStreamPool is inference only: call .eval() on the model")
            embs = self.lips.flush(tracks)
            empty = _lib.empty(0, device=self.device)
            mid = self.audio.push(ids, [empty] * R, self._regroup(embs, groups))
            last = self.audio.flush(ids)
            for s, m, t in zip(ids, mid, last):
                res[s] = {j: torch.cat([m[j], t[j]]) if m[j].shape[0] else t[j] for j in t}
        return [res[s] for s in named]

    def _drop(self, ids):
        self.lips.reset([s * self.speakers + j for s in ids for j in range(self.speakers)])
        self.audio.reset(ids)


def open_camera_streams(system, slots, window=32000, hop=None, max_chunk=None, max_batch=32, roi_hw=(96, 96), sample_rate=16000, speakers=1,
                        max_speakers=None, frame_rate=25, timebase=None):
    """``System.open_camera_streams``: the lip pool and the audio pool of one set of slots."""
    from . import datas
    rate, timebase = datas.frame_rate_of(frame_rate), timebase_of(timebase)
    K = speakers_of(speakers)
    if timebase is not None and (K != 1 or max_speakers is not None or _rate(sample_rate) != FS or rate != 25):
        raise ValueError(f"open_camera_streams: timebase = {timebase} takes one face per slot, 16 kHz audio and no frame_rate (speakers = "
                         f"{speakers}, max_speakers = {max_speakers}, sample_rate = {sample_rate}, frame_rate = {rate})")
    if max_speakers is not None:
        if K != 1:
            raise ValueError("open_camera_streams: speakers and max_speakers exclude each other")
        try:
            K = speakers_of(max_speakers)
        except ValueError:
            raise ValueError(f"open_camera_streams: max_speakers = {max_speakers!r}; an integer in 1 .. {MAX_SPEAKERS}") from None
        if _rate(sample_rate) != FS:
            raise ValueError(f"open_camera_streams: max_speakers = {K} with sample_rate = {sample_rate}: this pool takes 16 kHz audio only")
    if K > 1 and _rate(sample_rate) != FS:
        raise ValueError(f"open_camera_streams: speakers = {K} with sample_rate = {sample_rate}: several speakers take 16 kHz audio only")
    if _rate(sample_rate) != FS:
        mc = (window if max_chunk is None else max_chunk)
        return _open_at_rate(lambda room: open_camera_streams(system, slots, window, hop, mc + room, max_batch, roi_hw, frame_rate=rate),
                             sample_rate, mc)
    if system.video_model is None:
        raise ValueError("open_camera_streams: the system has no video model; push lip embeddings through open_streams")
    try:
        window = operator.index(window)
        max_chunk = window if max_chunk is None else operator.index(max_chunk)
    except TypeError:
        raise ValueError("open_camera_streams: window and max_chunk must be integers") from None
    if max_chunk < SPF or max_chunk % SPF:
        raise ValueError(f"open_camera_streams: max_chunk = {max_chunk} must be a positive multiple of {SPF}")
    # the most camera frames whose model frames still number at most max_chunk // 640 per push: ceil(25 mc / rate) <= max_chunk // 640
    mc = (max_chunk // SPF) * rate.numerator // (25 * rate.denominator)
    if mc < 1:
        raise ValueError(f"open_camera_streams: max_chunk = {max_chunk} holds no camera frame at {rate} fps")
    audio = system.audio_model.open_streams(slots, window=window, hop=hop, max_chunk=max_chunk + LOOKAHEAD * SPF, max_batch=max_batch,
                                            **(dict(speakers=K) if max_speakers is None else dict(max_speakers=K)))
    if rate != 25:
        lips = system.video_model.open_streams(audio.slots * K, max_frames=mc, roi_hw=roi_hw, frame_rate=rate)
    elif timebase is not None:
        lips = system.video_model.open_streams(audio.slots * K, max_frames=max_chunk // SPF, roi_hw=roi_hw, timebase=timebase)
    else:
        lips = system.video_model.open_streams(audio.slots * K, max_frames=max_chunk // SPF, roi_hw=roi_hw)
    if lips.device != audio.device:
        raise ValueError(f"open_camera_streams: the video model lies on {lips.device}, the audio model on {audio.device}")
    if max_speakers is not None:
        return FaceCameraStreamPool(lips, audio, max_chunk)
    return (SpeakerCameraStreamPool if K > 1 else CameraStreamPool)(lips, audio, max_chunk)


# ================================================================ live streams at the microphone's rate (DESIGN.md "Live streams at the microphone's rate")
RESAMPLE_PLAN_WORDS = 7  # RTFS_LIVE_RESAMPLE_PLAN_WORDS: [slot | a | m | g | k | out_off | side]


class ResampleStreamPool(_Pool):
    """``slots`` concurrent streams resampled chunk by chunk.  Built by ``datas.open_resample_streams``.

    For any way of cutting a recording into chunks, the concatenation of what ``push`` and the final ``flush`` return is BIT-equal to
    ``datas.resample`` of the whole recording: every output is formed by the same chain of fused multiply-adds on the same values.  In
    the notation of ``datas.resample_plan`` output q = j n + p reads the inputs up to last(q) = j o + floor(o p / n) + width, and after
    a samples the outputs emitted are G(a) = ceil(n max(0, a - width) / o): an output leaves width / orig_freq seconds after the last
    sample it reads arrived (0.4 ms at 48 kHz).  The state of a slot is its last 2 width samples in two buffers, read one and write the
    other (304 bytes per slot at 48 kHz).

    Host state per slot: a samples received, g samples emitted (and the side of the history that is current).  All arithmetic of a tick
    is ``rtfs_live_resample_plan`` (host only); per tick one plan, one table upload, one launch, nothing read back.  Not capturable in
    a HIP graph (the tick table is uploaded per call)."""

    _WORDS, _NAMES = 3, ("a", "g")

    def __init__(self, slots, orig_freq, new_freq, max_chunk, device):
        from . import datas
        self.slots, self.orig_freq, self.new_freq, self.max_chunk = slots, orig_freq, new_freq, max_chunk
        self.o, self.n, self.width, _ = datas.resample_plan(orig_freq, new_freq)
        self.device = device
        self.on_hip = device.type == "cuda"
        self._counters = [[0, 0, 0] for _ in range(slots)]
        self._hist = _lib.empty(slots, 2, 2 * self.width, device=device)
        self._bank = datas.resample_bank(self.o, self.n, device) if self.on_hip else None
        self._reset_state(None, slots)

    # -- public
    def counters(self, slot):
        """(a, g) of a slot: input samples received, output samples emitted."""
        return tuple(self._counters[int(slot)][:2])

    def push(self, slot_ids, chunks):
        """One chunk for each slot named: (m)|(1,m) float32, or int16 PCM (a sample s enters as s / 32768, what reading a 16-bit file as
        float32 gives); one kind per call, 0 <= m <= max_chunk, separate allocations on the pool's device, read where they lie.  Returns,
        per named slot, the (k,) float32 outputs that became final (k may be 0): views of one flat output whose per-slot blocks start on
        128-byte lines.

        ValueError - before any launch, all state unchanged - for an unknown or repeated slot id, a bad shape / dtype / device or an
        oversize chunk."""
        ids, ms, chunks, i16, plan = self._check_chunks(slot_ids, chunks)
        return self._tick(ids, ms, chunks, i16, flush=False, plan=plan)

    def flush(self, slot_ids):
        """End the named streams: the outputs still owed up to ceil(n a / o), the length ``datas.resample`` gives the samples received,
        with zeros behind the last sample, then reset the slots.  A slot that received nothing returns (0,)."""
        return self._tick(self._check_ids(slot_ids), None, None, False, flush=True)

    # -- checks (no launch, no state change)
    def _check_chunks(self, slot_ids, chunks):
        ids = self._check_ids(slot_ids)
        try:
            chunks = list(chunks)
        except TypeError:
            raise ValueError("ResampleStreamPool.push: chunks must be a sequence of tensors") from None
        if len(ids) != len(chunks):
            raise ValueError(f"ResampleStreamPool.push: {len(ids)} slot id(s) and {len(chunks)} chunk(s)")
        if any(not isinstance(c, torch.Tensor) for c in chunks):
            raise ValueError("ResampleStreamPool.push: every chunk must be a tensor")
        kinds = {c.dtype for c in chunks}
        if len(kinds) > 1 or (kinds and not kinds <= {torch.int16, torch.float32}):
            raise ValueError(f"ResampleStreamPool.push: chunks must be all float32 or all int16 PCM; got {sorted(map(str, kinds))}")
        for r, c in enumerate(chunks):
            if c.ndim not in (1, 2) or (c.ndim == 2 and c.shape[0] != 1):
                raise ValueError(f"ResampleStreamPool.push: chunk {r} must be (m) or (1,m); got {tuple(c.shape)}")
            if c.device != self.device:
                raise ValueError(f"ResampleStreamPool.push: chunk {r} lies on {c.device}, the pool on {self.device}")
            if c.numel() > self.max_chunk:
                raise ValueError(f"ResampleStreamPool.push: chunk {r} holds {c.numel()} samples; max_chunk = {self.max_chunk}")
        ms = [int(c.numel()) for c in chunks]
        plan = self._plan(ids, ms, False)  # unknown / repeated ids; the tick that follows takes this plan
        return ids, ms, [c.reshape(-1).contiguous() for c in chunks], kinds == {torch.int16}, plan

    def _plan(self, ids, ms, flush):
        if not ids:
            return [], [], [0, 0, 0]
        return self._call_planner(_lib.load().rtfs_live_resample_plan, ids, (ms,), flush, (self.o, self.n, self.max_chunk),
                                  RESAMPLE_PLAN_WORDS, 3)

    # -- one tick
    def _tick(self, ids, ms, chunks, i16, flush, plan=None):
        R = len(ids)
        if R == 0:
            return []
        new, table, (floats, max_m, max_k) = plan or self._plan(ids, ms, flush)
        if not self.on_hip:
            raise RuntimeError("rtfs_net_amd kernels run on the MI355X only: the pool lies on a CPU device (there is no CPU fallback)")
        lib, dev = _lib.load(), self.device
        ptrs = [0] * R if flush else [c.data_ptr() for c in chunks]
        with torch.no_grad():
            tab = torch.tensor(table + ptrs, dtype=torch.int64).to(dev)  # the one host-to-device copy of the tick
            out = _lib.empty(floats, device=dev)
            run = lib.rtfs_live_resample_i16 if i16 else lib.rtfs_live_resample_f32
            _lib.check(run(_lib.ptr(tab), _lib.ptr(self._bank), _lib.ptr(self._hist), _lib.ptr(out), R, max_m, max_k, int(flush), self.o, self.n,
                           _lib.stream_of(self._hist)), "rtfs_live_resample_i16" if i16 else "rtfs_live_resample_f32")
            if flush:
                self._reset_state(tab[:R], R)
        for r, s in enumerate(ids):
            self._counters[s] = new[3 * r:3 * r + 3]
        ks, offs = table[4 * R:5 * R], table[5 * R:6 * R]
        return [out[off:off + k] for k, off in zip(ks, offs)]

    def _reset_state(self, ids, R):
        """Give both history buffers of R slots (a device tensor of ids; None = the first R) defined contents.  Which cells hold a sample
        follows from a, so nothing depends on these zeros."""
        if not self.on_hip:
            self._hist[slice(0, R) if ids is None else ids] = 0
            return
        _lib.check(_lib.load().rtfs_live_resample_reset(_lib.ptr(ids), _lib.ptr(self._hist), R, self.o, self.n, _lib.stream_of(self._hist)),
                   "rtfs_live_resample_reset")


def _rate(sample_rate):
    try:
        return operator.index(sample_rate)
    except TypeError:
        raise ValueError(f"sample_rate must be an integer number of Hz; got {sample_rate!r}") from None


def open_resample_streams(slots, orig_freq, new_freq=FS, max_chunk=None, device=None):
    """``datas.open_resample_streams``: check the arguments, then allocate the pool.  ``max_chunk`` (input samples per push and slot)
    defaults to one second."""
    from . import datas
    try:
        slots, orig_freq, new_freq = operator.index(slots), operator.index(orig_freq), operator.index(new_freq)
        max_chunk = orig_freq if max_chunk is None else operator.index(max_chunk)
    except TypeError:
        raise ValueError("open_resample_streams: slots, orig_freq, new_freq and max_chunk must be integers") from None
    if slots < 1 or slots > 65535 or max_chunk < 1 or max_chunk > MAX_CAPACITY * datas.MAX_RATIO:
        raise ValueError(f"open_resample_streams: slots = {slots} (1 .. 65535), max_chunk = {max_chunk} (at least 1)")
    if orig_freq == new_freq:
        raise ValueError(f"open_resample_streams: {orig_freq} -> {new_freq} is no resampling (datas.resample hands such input back as it is)")
    datas.resample_plan(orig_freq, new_freq)  # ValueError for a ratio the kernel does not take
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return ResampleStreamPool(slots, orig_freq, new_freq, max_chunk, device)


class RateStreamPool(_Pool):
    """A ``StreamPool`` or ``CameraStreamPool`` whose audio arrives at the microphone's rate.  Built by ``open_streams`` /
    ``open_camera_streams`` with ``sample_rate`` other than 16000; same ``push`` / ``flush`` / ``reset`` / ``counters`` surface.

    A ``ResampleStreamPool`` brings each tick's audio chunks (float32 or int16 PCM at ``sample_rate``, at most ``max_chunk_in`` =
    floor(max_chunk o / n) samples) to 16 kHz and its output blocks go straight on, without a copy, as the inner pool's audio chunks;
    the concatenated outputs equal ``separate_long(datas.resample(wav, sample_rate), ...)`` / ``System.separate_recording(wav,
    sample_rate, rois)`` of the whole recording.  ``window``, ``hop`` and ``max_chunk`` stay in 16 kHz samples.  A chunk of m samples
    gives at most floor(m n / o) + 1 outputs, so the inner pool is opened with ``max_chunk + 640``, and a push is refused unless the
    resampler's flush tail (at most ceil(n width / o) + 1 samples) still fits the inner ring behind it: the tail of a ``flush`` is
    then never refused.  ``datas.normalize_mixture`` is NOT applied and cannot be: it needs the deviation of the whole recording, which
    a stream does not have (``separate_recording``'s ``normalize_audio`` is off by default as well)."""

    def __init__(self, resampler, inner, max_chunk):
        self.resampler, self.inner, self.max_chunk = resampler, inner, max_chunk
        self.camera = isinstance(inner, CameraStreamPool)
        self.audio = inner.audio if self.camera else inner
        self.slots, self.device, self.n_src = inner.slots, inner.device, inner.n_src
        self.sample_rate, self.max_chunk_in = resampler.orig_freq, resampler.max_chunk
        self.tail = -(-resampler.n * resampler.width // resampler.o) + 1
        self.max_frames = max_chunk // SPF  # per push; in camera frames where the lip pool runs at the camera's own frame rate
        rate = getattr(inner.lips, "frame_rate", None) if self.camera else None
        if rate is not None:
            self.max_frames = max(1, self.max_frames * rate.numerator // (25 * rate.denominator))

    def counters(self, slot):
        """((a, g) of the resampler, the inner pool's counters)."""
        return self.resampler.counters(slot), self.inner.counters(slot)

    def _no_video(self, R):
        if not self.camera:
            return [_lib.empty(512, 0, device=self.device)] * R
        hw = self.inner.lips.roi_hw
        return [_lib.empty(0, CROP, CROP, device=self.device) if hw is None else _lib.empty(0, *hw, device=self.device, dtype=torch.uint8)] * R

    def _plan_inner(self, ids, ks, nf):
        """The inner pool's dry run of a push of ks 16 kHz samples and nf frames; refuses a push behind which the flush tail would not
        fit.  -> the inner audio pool's new counters."""
        new = self.inner._plan_push(ids, ks, nf)[0]
        for r, s in enumerate(ids):
            a, _, e, _ = new[4 * r:4 * r + 4]
            if a + self.tail - e * self.audio.hop > self.audio.capacity:
                raise ValueError(f"RateStreamPool.push: refused ({_REASONS[5]}) at slot {s}; no slot was changed")
        return new

    def push(self, slot_ids, audio_chunks, video_chunks):
        """As the inner pool's ``push``, with audio chunks at ``sample_rate``: (m)|(1,m) float32 or int16 PCM, 0 <= m <= max_chunk_in.
        All pools plan first - the resampler's plan gives the 16 kHz sizes the inner plan takes - so a ValueError from any of them comes
        before any launch with all state unchanged."""
        ids, ms, wavs, i16, rplan = self.resampler._check_chunks(slot_ids, audio_chunks)
        if self.camera:
            _, nf, rois, u8 = self.inner.lips._check_chunks(ids, video_chunks)
            if any(f > self.max_frames for f in nf):
                raise ValueError(f"RateStreamPool.push: a chunk of {max(nf)} frames; at most {self.max_frames} (max_chunk // {SPF} model frames)")
        else:
            _, _, nf, _, _ = self.audio._check_chunks(ids, [_lib.empty(0, device=self.device)] * len(ids), video_chunks)
        if not ids:
            return []
        self._plan_inner(ids, rplan[1][4 * len(ids):5 * len(ids)], nf)
        if self.audio.model.training:
            raise RuntimeError("RateStreamPool is inference only: call .eval() on the model")
        blocks = self.resampler._tick(ids, ms, wavs, i16, flush=False, plan=rplan)
        if self.camera:  # CameraStreamPool.push behind its checks, which have all been made
            video_chunks = self.inner.lips._tick(ids, nf, rois, u8, flush=False)
        return self.audio.push(ids, blocks, video_chunks)

    def flush(self, slot_ids):
        """End the named streams: the resampler's flush, its tail pushed with empty video, then the inner flush.  Returns the remaining
        samples per slot (those the middle step made final in front of the flush's own)."""
        ids = self._check_ids(slot_ids)
        if not ids:
            return []
        R = len(ids)
        _, rtab, _ = self.resampler._plan(ids, None, True)
        new = self.inner._plan_push(ids, rtab[4 * R:5 * R], [0] * R)[0]
        with _counters_as(self.audio, ids, new, 4):  # the inner flush is planned on the counters the tail leaves
            self.inner._plan_flush(ids)
        if self.audio.model.training:
            raise RuntimeError("RateStreamPool is inference only: call .eval() on the model")
        mid = self.inner.push(ids, self.resampler.flush(ids), self._no_video(R))
        return _join(mid, self.inner.flush(ids))

    def _drop(self, ids):
        self.resampler.reset(ids)
        self.inner.reset(ids)


def _open_at_rate(open_inner, sample_rate, max_chunk):
    """The pool ``open_inner(640)`` returns (one more frame of room: a chunk may resample to max_chunk + 1 samples) behind a resampler
    from ``sample_rate``."""
    from . import datas
    try:
        max_chunk = operator.index(max_chunk)
    except TypeError:
        raise ValueError("open_streams: max_chunk must be an integer") from None
    o, n, width, _ = datas.resample_plan(sample_rate, FS)
    if max_chunk < SPF or max_chunk % SPF:
        raise ValueError(f"open_streams: max_chunk = {max_chunk} must be a positive multiple of {SPF}")
    tail = -(-n * width // o) + 1
    if tail > max_chunk:
        raise ValueError(f"open_streams: at {sample_rate} Hz a flush leaves up to {tail} samples, more than max_chunk = {max_chunk}")
    inner = open_inner(SPF)
    return RateStreamPool(open_resample_streams(inner.slots, sample_rate, FS, max_chunk=max(1, max_chunk * o // n), device=inner.device),
                          inner, max_chunk)
