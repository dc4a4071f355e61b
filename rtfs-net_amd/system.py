"""Mirror of the reference's ``System`` (``src/system/core.py:50-123``) and its on-disk formats (SURVEY 8f rank 4 + the start of
rank 1): ``forward(wav, mouth)`` chains the video front-end and the separator; ``validation_step`` / ``training_step`` add the PIT
loss, all on the HIP path.  ``optimization_step`` is what Lightning does around ``training_step`` in the reference (``train.py:135-148``:
backward, gradient all-reduce over the data-parallel ranks, ``gradient_clip_val`` 5.0, optimizer step) written out, because Lightning is
not a dependency here; the gradient exchange is ONE all-reduce of one flattened buffer (RCCL when the process group is ``nccl``).
Training covers what ``AVNet.forward_train`` covers (frozen BatchNorm statistics, frozen video-side VP block).
``load_lightning_checkpoint`` reads a Lightning ``.ckpt`` (``state_dict`` with ``audio_model.`` / ``video_model.`` prefixes,
``core.py:178-181``) and ``load_best_model`` the ``best_model.pth`` that ``train.py:156-160`` writes, both with non-executing loaders.
"""
from __future__ import annotations

import torch
import torch.nn as nn


class System(nn.Module):
    """core.py:53-92: audio_model (AVNet), optional video_model (FRCNNVideoModel), optional loss_func {"val": PITLossWrapper}."""

    default_monitor: str = "val_loss"

    def __init__(self, audio_model=None, video_model=None, optimizer=None, loss_func=None, train_loader=None, val_loader=None,
                 scheduler=None, config=None, train_video_model=False):
        super().__init__()
        if train_video_model:
            raise ValueError("MI355X System: the video front-end is inference-only (the reference freezes it too: yaml videonet)")
        self.audio_model, self.video_model, self.loss_func = audio_model, video_model, loss_func
        self.optimizer, self.scheduler = optimizer, scheduler
        self.train_loader, self.val_loader = train_loader, val_loader
        self.config = {} if config is None else config

    def forward(self, wav, mouth=None):
        """core.py:78-92."""
        if self.video_model is None:
            return self.audio_model(wav)
        with torch.no_grad():
            mouth_emb = self.video_model(mouth.type_as(wav))
        return self.audio_model(wav, mouth_emb)

    def separate_speakers(self, wav, mouths, counts=None):
        """Every target speaker of each mixture with one audio pass (inference): wav (B,L), mouths (B,K,1,Tv,88,88) -> (B,K,L).  The video
        front-end runs on the B*K mouth tracks (no_grad, as in ``forward``), then ``AVNet.separate_speakers``.  Without a video model the
        mouth slot holds lip embeddings (B,K,512,Tv).

        ``counts`` (B ints): mixture b has counts[b] faces; mouths is (N,1,Tv,88,88), N = sum(counts), mixture-major, and the result (N,L).
        The video front-end runs ONCE on the N tracks.  Without a video model the mouth slot holds lip embeddings (N,512,Tv)."""
        if counts is not None:
            if self.video_model is None:
                return self.audio_model.separate_speakers(wav, mouths, counts=counts)
            from .models import mixture_counts
            B = 1 if wav.ndim == 1 else int(wav.shape[0])
            counts = mixture_counts(counts, B, int(mouths.shape[0]), "System.separate_speakers")  # before the video model's launches
            with torch.no_grad():
                emb = self.video_model(mouths.type_as(wav))
            return self.audio_model.separate_speakers(wav, emb, counts=counts)
        if mouths.ndim < 3:
            raise ValueError(f"System.separate_speakers: mouths must be (B,K,...); got {tuple(mouths.shape)}")
        B, K = int(mouths.shape[0]), int(mouths.shape[1])
        if self.video_model is None:
            return self.audio_model.separate_speakers(wav, mouths)
        with torch.no_grad():
            emb = self.video_model(mouths.reshape(B * K, *mouths.shape[2:]).type_as(wav))
        return self.audio_model.separate_speakers(wav, emb.reshape(B, K, *emb.shape[1:]))

    def separate_long(self, wav, mouth, **kw):
        """A recording of any length in overlapping windows on the fused separator (inference): wav (L)|(B,L)|(B,1,L), mouth
        (B,1,Tv,88,88) at 25 fps -> (B,n_src,L).  The video front-end runs ONCE on the whole mouth track (no_grad, as in ``forward``), so
        its temporal context stays continuous across window boundaries; the embedding and ``**kw`` (window, hop, max_batch) go to
        ``AVNet.separate_long``.  Without a video model the mouth slot holds lip embeddings (B,512,Tv).  This is what the reference's
        ``infer_any_video.py:63-86`` call (whole track, one ``forward``) maps onto for recordings past the fused length."""
        if self.video_model is None:
            return self.audio_model.separate_long(wav, mouth, **kw)
        with torch.no_grad():
            emb = self.video_model(mouth.type_as(wav))
        return self.audio_model.separate_long(wav, emb, **kw)

    def separate_long_speakers(self, wav, mouths, **kw):
        """Every face of a long recording with one audio pass per window (inference): wav (L)|(B,L)|(B,1,L), mouths (B,K,1,Tv,88,88) at
        25 fps -> (B,K,L).  The video front-end runs ONCE on the B*K whole tracks (no_grad), then ``AVNet.separate_long_speakers(**kw)``.
        Without a video model the mouth slot holds lip embeddings (B,K,512,Tv)."""
        if self.video_model is None:
            return self.audio_model.separate_long_speakers(wav, mouths, **kw)
        if mouths.ndim != 6:
            raise ValueError(f"System.separate_long_speakers: mouths must be (B,K,1,Tv,88,88); got {tuple(mouths.shape)}")
        B, K = int(mouths.shape[0]), int(mouths.shape[1])
        with torch.no_grad():
            emb = self.video_model(mouths.reshape(B * K, *mouths.shape[2:]).type_as(wav))
        return self.audio_model.separate_long_speakers(wav, emb.reshape(B, K, *emb.shape[1:]), **kw)

    def separate_recording(self, wav, sample_rate, mouth_rois, normalize_audio=False, frame_rate=25, timestamps=None, timebase=None, until=None,
                           **kw):
        """A raw recording end to end on the device (inference), the whole of ``infer_any_video.py:63-86``: wav (L) | (B,L) at
        ``sample_rate`` Hz, mouth_rois uint8 (Tv,H,W) | (B,Tv,H,W) at 25 fps -> (B, n_src, L at 16 kHz).  ``datas.resample`` to 16 kHz, the
        ``"val"`` pipeline on the ROIs (one launch), the video model once on the whole track, then ``separate_long(**kw)``.  Without a
        video model the mouth slot holds lip embeddings (B,512,Tv), as in ``separate_long``; a floating mouth slot is taken as prepared
        lips.  ``normalize_audio`` (``datas.normalize_mixture`` on the resampled mixture) is off by default: the reference's script computes
        the mixture's deviation and never applies it.

        ``frame_rate`` other than 25 (DESIGN.md "Live streams at the camera's frame rate"): the uint8 ROIs are the camera's frames at that
        rate and the ``"val"`` launch selects the frames ``datas.frame_rate_map`` names, where the reference converts the file with
        ``ffmpeg -r 25`` first.  Prepared lips and embeddings are model frames already: ValueError with another rate.

        ``timestamps`` with ``timebase`` (DESIGN.md "Live streams with per-frame timestamps"): the capture time of every frame of
        ``mouth_rois`` in ticks of 1 / timebase s, for a camera that dropped frames or changed rate.  The frames
        ``datas.timestamp_map(timestamps, timebase, until)`` names are selected on the device (``index_select``), then the 25 fps path
        runs as above.  ValueError with another ``frame_rate``, or with one of the two missing."""
        from . import datas
        rate = datas.frame_rate_of(frame_rate)
        if timestamps is not None or timebase is not None or until is not None:
            if timestamps is None or timebase is None or rate != 25:
                raise ValueError("System.separate_recording: timestamps and timebase go together, without a frame_rate")
            idx = datas.timestamp_map(timestamps, timebase, until)
            if len(idx) == 0 or mouth_rois.shape[-3] != len(timestamps):
                raise ValueError(f"System.separate_recording: {len(timestamps)} timestamp(s) for {mouth_rois.shape[-3]} frame(s); need one per "
                                 f"frame, at least 1")
            mouth_rois = mouth_rois.index_select(mouth_rois.ndim - 3, torch.tensor(idx, dtype=torch.int64, device=mouth_rois.device))
        wav = datas.resample(wav, sample_rate, 16000)
        if normalize_audio:
            wav = datas.normalize_mixture(wav)
        if self.video_model is not None and mouth_rois.dtype == torch.uint8:
            val = datas.get_preprocessing_pipelines()["val"]
            mouth_rois = val(mouth_rois) if rate == 25 else val(mouth_rois, frame_rate=rate)
        elif rate != 25:
            raise ValueError(f"System.separate_recording: frame_rate = {rate} needs uint8 mouth ROIs and a video model")
        return self.separate_long(wav, mouth_rois, **kw)

    def separate_video(self, wav, sample_rate, frames, eyes, lips, order="bgr", **kw):
        """A raw recording from whole camera frames (inference; DESIGN.md "Mouth ROIs from camera frames"): ``infer_any_video.py:63-86``
        including its line 76, the landmark-aligned mouth crop.  wav (L) at ``sample_rate`` Hz, frames uint8 (Tv,H,W,3) in ``order``
        "bgr" | "rgb" or a grey plane (Tv,H,W) on the device, eyes (Tv,2,2) and lips (Tv,4,2) host landmarks as ``datas.mouth_affine``
        takes them (the detector stays the caller's).  ``datas.mouth_rois`` cuts the (Tv,96,96) ROIs in one launch, then
        ``separate_recording(wav, sample_rate, rois, **kw)``: ``frame_rate``, ``timestamps``, ``timebase``, ``until``,
        ``normalize_audio``, ``window`` ... pass through untouched, and at another ``frame_rate`` every camera frame is cropped before
        the ``"val"`` launch selects.  A batch: wav (B,L) with frames a sequence of B tensors of equal Tv (any resolutions), eyes and
        lips sequences; still one crop launch."""
        from . import datas
        rois = datas.mouth_rois(frames, eyes, lips, order=order)
        if not isinstance(rois, torch.Tensor):
            if len({tuple(r.shape) for r in rois}) != 1 or any(r.ndim != 3 for r in rois):
                raise ValueError(f"System.separate_video: the frame tensors of a batch must hold the same number of frames, one face "
                                 f"each; got ROIs {[tuple(r.shape) for r in rois]}")
            rois = torch.stack(list(rois))
        elif rois.ndim != 3:
            raise ValueError("System.separate_video: one face per recording (eyes (Tv,2,2), lips (Tv,4,2)); separate_long_speakers takes several")
        return self.separate_recording(wav, sample_rate, rois, **kw)

    def separate_many(self, wavs, mouths, **kw):
        """Many recordings of different lengths in one pooled pass (inference): wavs = R tensors (L_r)|(1,L_r), mouths = R lip tracks
        (1,Tv_r,88,88) at 25 fps -> a list of R tensors (n_src,L_r).  The video front-end runs under no_grad ONCE PER GROUP of tracks with
        equal Tv_r, the tracks of a group stacked as a batch; a track is never joined to another along time, because the stem's temporal
        padding belongs to each track.  The embeddings and ``**kw`` (window, hop, max_batch) go to ``AVNet.separate_many``.  Without a
        video model the mouth slot holds lip embeddings (512,Tv_r)."""
        wavs, mouths = list(wavs), list(mouths)
        if self.video_model is None:
            return self.audio_model.separate_many(wavs, mouths, **kw)
        if len(wavs) < 1 or len(mouths) != len(wavs):
            raise ValueError(f"System.separate_many: {len(wavs)} recording(s) and {len(mouths)} lip track(s); need the same number, at least 1")
        groups = {}
        for r, m in enumerate(mouths):
            if not isinstance(m, torch.Tensor) or m.ndim != 4 or m.shape[0] != 1 or m.shape[1] < 1:
                raise ValueError(f"System.separate_many: lip track {r} must be (1,Tv,88,88) with Tv >= 1; "
                                 f"got {tuple(m.shape) if isinstance(m, torch.Tensor) else type(m).__name__}")
            groups.setdefault(int(m.shape[1]), []).append(r)
        embs = [None] * len(mouths)
        with torch.no_grad():
            for rs in groups.values():
                emb = self.video_model(torch.stack([mouths[r] for r in rs]).type_as(wavs[rs[0]]))  # (G,1,Tv,88,88) -> (G,512,Tv)
                for g, r in enumerate(rs):
                    embs[r] = emb[g]
        return self.audio_model.separate_many(wavs, embs, **kw)

    def evaluate_many(self, wavs, cleans, mouths, keys, tracker, **kw):
        """The reference's test loop (``test.py:51-62``) for a pool: ``separate_many(wavs, mouths, **kw)``, then
        ``tracker.update_many(wavs, cleans, estimates, keys)`` (an ``ALLMetricsTracker``; cleans = R tensors (n_src,L_r)) scores the R
        estimates in one pooled pass.  Returns the estimates, the list ``separate_many`` returns."""
        wavs = list(wavs)
        estimates = self.separate_many(wavs, mouths, **kw)
        tracker.update_many(wavs, cleans, estimates, keys)
        return estimates

    def separate_many_speakers(self, wavs, mouths, **kw):
        """Many recordings, each with its own number of faces, in one pooled pass (inference): wavs = R tensors (L_r)|(1,L_r), mouths = R
        tensors (K_r,1,Tv_r,88,88) at 25 fps -> a list of R tensors (K_r,L_r).  The video front-end runs under no_grad ONCE PER GROUP of
        recordings with equal Tv_r, all tracks of the group as one batch, as in ``separate_many``; the embeddings and ``**kw`` go to
        ``AVNet.separate_many_speakers``.  Without a video model the mouth slot holds lip embeddings (K_r,512,Tv_r)."""
        wavs, mouths = list(wavs), list(mouths)
        if self.video_model is None:
            return self.audio_model.separate_many_speakers(wavs, mouths, **kw)
        if len(wavs) < 1 or len(mouths) != len(wavs):
            raise ValueError(f"System.separate_many_speakers: {len(wavs)} recording(s) and {len(mouths)} lip tensor(s); need the same "
                             f"number, at least 1")
        groups = {}
        for r, m in enumerate(mouths):
            if not isinstance(m, torch.Tensor) or m.ndim != 5 or m.shape[0] < 1 or m.shape[1] != 1 or m.shape[2] < 1:
                raise ValueError(f"System.separate_many_speakers: lip tracks {r} must be (K,1,Tv,88,88) with K, Tv >= 1; "
                                 f"got {tuple(m.shape) if isinstance(m, torch.Tensor) else type(m).__name__}")
            groups.setdefault(int(m.shape[2]), []).append(r)
        embs = [None] * len(mouths)
        with torch.no_grad():
            for rs in groups.values():
                emb = self.video_model(torch.cat([mouths[r] for r in rs]).type_as(wavs[rs[0]]))  # (sum K,1,Tv,88,88) -> (sum K,512,Tv)
                for r, e in zip(rs, emb.split([int(mouths[r].shape[0]) for r in rs])):
                    embs[r] = e
        return self.audio_model.separate_many_speakers(wavs, embs, **kw)

    def open_streams(self, sample_rate=16000, **kw):
        """Live streams chunk by chunk (inference): ``AVNet.open_streams(**kw)`` of the audio model.  The caller pushes lip EMBEDDINGS
        (512,m): the video stem is a 3-D convolution with temporal context, so frames embedded chunk by chunk are not the whole-track
        embedding without look-ahead state.  ``open_camera_streams`` is the entry that takes the camera's frames and keeps that state.
        ``sample_rate``: the rate of the audio chunks, as ``AVNet.open_streams`` takes it.  ``speakers=K`` (in ``**kw``): K lip tracks per
        slot -> ``streaming.SpeakerStreamPool``; ``max_speakers=Kmax``: faces that come and go -> ``streaming.FaceStreamPool``, both as
        ``AVNet.open_streams`` describes."""
        return self.audio_model.open_streams(sample_rate=sample_rate, **kw)

    def open_camera_streams(self, slots, window=32000, hop=None, max_chunk=None, max_batch=32, roi_hw=(96, 96), sample_rate=16000, speakers=1,
                            max_speakers=None, frame_rate=25, timebase=None):
        """Live streams from microphone samples and camera frames (inference; DESIGN.md "Live streams from camera frames") ->
        ``streaming.CameraStreamPool``.  ``pool.push(slot_ids, audio_chunks, roi_chunks)`` takes 16 kHz audio chunks of at most
        ``max_chunk`` samples (default ``window``) and uint8 mouth ROIs (m,H,W) with (H,W) == ``roi_hw`` at 25 fps (or float32 prepared lips
        (m,88,88)), and returns the (n_src,k) newly final samples; ``pool.flush`` / ``pool.reset`` end streams.  The frames are embedded
        chunk by chunk with two frames (80 ms) of look-ahead and pushed straight on into the audio ``StreamPool``; for any chunking the
        concatenated outputs equal ``separate_recording(wav, sample_rate, rois, window=..., hop=...)``.

        ``sample_rate`` other than 16000 (DESIGN.md "Live streams at the microphone's rate") -> ``streaming.RateStreamPool``: the audio
        chunks are at that rate, float32 or int16 PCM, at most floor(max_chunk o / n) samples, and are resampled on the device chunk by
        chunk, bit-equal to ``datas.resample`` of the whole recording; ``window``, ``hop`` and ``max_chunk`` stay in 16 kHz samples.
        ``normalize_audio`` has no streamed form: it needs the whole recording's deviation.

        ``speakers`` = K > 1 (DESIGN.md "Every face of a stream") -> ``streaming.SpeakerCameraStreamPool``: the ROI chunk of a slot is
        (K,m,H,W) uint8 or (K,m,88,88) float32, the results are (K,k), and output k of a slot equals ``separate_recording(wav, 16000,
        rois[k])``; 16 kHz audio only (ValueError with another ``sample_rate``).

        ``max_speakers`` = Kmax (DESIGN.md "Faces that come and go") -> ``streaming.FaceCameraStreamPool``: up to Kmax faces per slot,
        declared with ``pool.add_face`` on an idle slot and ended with ``pool.drop_face`` at any time; the ROI chunk of a slot holds one
        block per active face and the results are dicts face id -> samples.  Excludes ``speakers``; 16 kHz audio only.

        ``frame_rate`` other than 25 (an int, a ``Fraction``, (num, den) or a float; DESIGN.md "Live streams at the camera's frame rate"),
        with any of the above: the ROI chunks hold the camera's frames at that rate, at most floor(max_chunk / 640 * frame_rate / 25) per
        push, and the frames the model sees are selected inside the ingest launch (``datas.frame_rate_map``); for any chunking the
        outputs equal ``separate_recording(..., frame_rate=frame_rate)``.  The lip pool is a ``streaming.RateLipStreamPool`` whose
        ``counters`` report camera frames received; ``window``, ``hop`` and ``max_chunk`` stay in 16 kHz samples.

        ``timebase`` = ticks per second (DESIGN.md "Live streams with per-frame timestamps"): for cameras that drop frames or change
        rate.  ``pool.push(slot_ids, audio_chunks, roi_chunks, timestamps=None, until=None)`` takes the capture time of every frame
        (stamp 0 is audio sample 0) and ``until``, the promise that no frame before that instant is still coming, which keeps a stream
        moving through a camera dropout; ``pool.flush(slot_ids, until=None)``.  The lip pool is a ``streaming.StampLipStreamPool`` and
        for any chunking the outputs equal ``separate_recording(..., timestamps=, timebase=, until=)``.  One face per slot, 16 kHz
        audio, no ``frame_rate``: ValueError with ``speakers``, ``max_speakers``, another ``sample_rate`` or another ``frame_rate``."""
        from . import streaming
        if timebase is not None:
            return streaming.open_camera_streams(self, slots, window=window, hop=hop, max_chunk=max_chunk, max_batch=max_batch, roi_hw=roi_hw,
                                                 sample_rate=sample_rate, speakers=speakers, max_speakers=max_speakers, frame_rate=frame_rate,
                                                 timebase=timebase)
        if frame_rate == 25:
            return streaming.open_camera_streams(self, slots, window=window, hop=hop, max_chunk=max_chunk, max_batch=max_batch, roi_hw=roi_hw,
                                                 sample_rate=sample_rate, speakers=speakers, max_speakers=max_speakers)
        return streaming.open_camera_streams(self, slots, window=window, hop=hop, max_chunk=max_chunk, max_batch=max_batch, roi_hw=roi_hw,
                                             sample_rate=sample_rate, speakers=speakers, max_speakers=max_speakers, frame_rate=frame_rate)

    def separate_recordings(self, wavs, sample_rates, mouth_rois, normalize_audio=False, frame_rates=None, **kw):
        """The list form of ``separate_recording``: wavs = R raw recordings (L_r) at ``sample_rates[r]`` Hz, mouth_rois = R uint8
        tracks (Tv_r,H,W) at 25 fps -> a list of R tensors (n_src, L_r at 16 kHz).  Per recording ``datas.resample`` to 16 kHz and the ``"val"`` pipeline on the ROIs, then ``separate_many(**kw)``.  Without a video model the mouth
        slot holds lip embeddings (512,Tv_r); a floating mouth slot is taken as prepared lips (1,Tv_r,88,88).  ``frame_rates``: one camera
        frame rate per recording, as ``separate_recording`` takes it (None: all 25)."""
        from . import datas
        wavs, mouth_rois = list(wavs), list(mouth_rois)
        rates = list(sample_rates)
        if len(wavs) < 1 or len(rates) != len(wavs) or len(mouth_rois) != len(wavs):
            raise ValueError(f"System.separate_recordings: {len(wavs)} recording(s), {len(rates)} sample rate(s), {len(mouth_rois)} mouth track(s)")
        fps = [25] * len(wavs) if frame_rates is None else [datas.frame_rate_of(f) for f in frame_rates]
        if len(fps) != len(wavs):
            raise ValueError(f"System.separate_recordings: {len(wavs)} recording(s) and {len(fps)} frame rate(s)")
        val = datas.get_preprocessing_pipelines()["val"]
        prepared, mouths = [], []
        for w, fs, roi, fr in zip(wavs, rates, mouth_rois, fps):
            if not isinstance(w, torch.Tensor) or w.ndim not in (1, 2) or (w.ndim == 2 and w.shape[0] != 1):
                raise ValueError("System.separate_recordings: every recording must be a tensor (L) or (1,L)")
            w = datas.resample(w.reshape(-1), fs, 16000)
            prepared.append(datas.normalize_mixture(w) if normalize_audio else w)
            if self.video_model is not None and roi.dtype == torch.uint8:
                if roi.ndim != 3:
                    raise ValueError(f"System.separate_recordings: uint8 mouth ROIs must be (Tv,H,W) per recording; got {tuple(roi.shape)}")
                roi = (val(roi) if fr == 25 else val(roi, frame_rate=fr))[0]  # (1,Tv,88,88)
            elif fr != 25:
                raise ValueError(f"System.separate_recordings: frame rate {fr} needs uint8 mouth ROIs and a video model")
            mouths.append(roi)
        return self.separate_many(prepared, mouths, **kw)

    def prepare_batch(self, batch, train=True, normalize_audio=False, rng=None):
        """A reference-shaped batch (inputs, targets, target_mouths, ...) whose mouth slot may hold uint8 ROIs, (B,Tv,H,W) or (B,K,Tv,H,W):
        returns the batch with that slot replaced by float lips, (B,1,Tv,88,88) or (B,K,1,Tv,88,88) (the layout ``separate_speakers``
        takes), prepared by the ``"train"`` (random crop and flip per track, drawn from ``rng`` or ``random``) or ``"val"`` pipeline in one
        launch.  A slot that is not uint8 is handed back as the same object.  ``normalize_audio`` also replaces inputs and targets by
        ``datas.normalize_mixture`` of the two (``avspeech_dataset.py:145-148``).  ``common_step`` and ``forward`` take the result as is."""
        from . import datas
        out = list(batch)
        if len(out) >= 3 and isinstance(out[2], torch.Tensor) and out[2].dtype == torch.uint8:
            m = out[2]
            if m.ndim not in (4, 5):
                raise ValueError(f"System.prepare_batch: uint8 mouth ROIs must be (B,Tv,H,W) or (B,K,Tv,H,W); got {tuple(m.shape)}")
            lips = datas.get_preprocessing_pipelines()["train" if train else "val"](m.reshape(-1, *m.shape[-3:]), rng=rng)
            out[2] = lips.reshape(*m.shape[:-3], 1, *lips.shape[2:])
        if normalize_audio:
            inputs, targets = out[0], out[1]
            if targets is None:
                out[0] = datas.normalize_mixture(inputs)
            else:
                t = targets.unsqueeze(-2) if targets.ndim == inputs.ndim else targets
                out[0], t = datas.normalize_mixture(inputs, t)
                out[1] = t.reshape(targets.shape)
        return type(batch)(out) if isinstance(batch, (list, tuple)) else out

    @staticmethod
    def online_mixing_collate(batch, perms=None, generator=None):
        """core.py:183-202 on the device: batch = (inputs, targets (B,n_src,L)) -> (inputs, targets).  For every source index i in the
        order 0 .. n_src - 1 a permutation p_i of the batch is taken from ``perms[i]`` or drawn with ``torch.randperm(B,
        generator=generator)`` on the CPU - the reference's call and order, so the same ``torch.manual_seed`` gives the same
        permutations.  New source i of row b is ``targets[p_i[b], i]`` scaled to the energy of ``targets[b, i]`` (no eps: a silent
        source gives inf / NaN, as there), the new input their sum.  ONE ``datas.mix_batch`` call: the segments are rows of ``targets``
        addressed where they lie, the references the rows they replace.  n_src <= 4, L <= 2^20, float32 on the device (ValueError)."""
        from . import datas
        _, targets = batch
        if not isinstance(targets, torch.Tensor) or targets.ndim != 3 or not targets.is_cuda or targets.dtype != torch.float32:
            raise ValueError("System.online_mixing_collate: targets must be a float32 device tensor (B,n_src,L); there is no CPU fallback")
        B, n_src, L = (int(v) for v in targets.shape)
        if perms is not None and len(perms) != n_src:
            raise ValueError(f"System.online_mixing_collate: {len(perms)} permutation(s) for {n_src} source(s)")
        src, ref = [], []
        for i in range(n_src):
            p = [int(v) for v in (torch.randperm(B, generator=generator) if perms is None else perms[i])]
            if sorted(p) != list(range(B)):
                raise ValueError(f"System.online_mixing_collate: perms[{i}] is no permutation of 0 .. {B - 1}")
            src.append([(q * n_src + i) * L for q in p])
            ref.append([(b * n_src + i) * L for b in range(B)])
        zeros = [[0] * n_src for _ in range(B)]
        recipe = datas.MixRecipe(zeros, [list(r) for r in zip(*src)], [[1.0] * n_src for _ in range(B)], zeros, [list(r) for r in zip(*ref)])
        return datas.mix_batch([targets.contiguous().reshape(-1)], recipe, L, n_out=n_src)

    def mix_batch(self, sources, mouth_rois, length=32000, n_src=2, snr_db=(-5.0, 5.0), normalize_audio=False, train=True, rng=None,
                  recipe=None, rirs=None, rir_prob=1.0, loudness=None, utter_lufs=None):
        """A fresh target-speaker training batch from a pool of utterances, formed on the device: sources = R 1-D device tensors
        (float32 or int16 PCM at 16 kHz), mouth_rois = their R uint8 ROI tracks (Tv_r,H,W) at 25 fps -> the reference-shaped batch
        (inputs (B,L), targets (B,L), target_mouths (B,1,Tv,88,88), keys) that ``common_step`` and ``optimization_step`` take as is.
        ``recipe``: a ``datas.MixRecipe``, or None to draw one (``datas.draw_mix_recipe(..., align=640)``, so every start lies on a video
        frame) from ``rng`` or ``random``: ``config["training"]["batch_size"]`` rows (default 4), per row a target and ``n_src - 1``
        interferers at SNRs uniform in ``snr_db``.  Mixture and target come from ONE ``datas.mix_batch`` (``n_out`` 1;
        ``normalize_audio``: the dataset's joint normalisation in the same two
        launches).  The target's ROI track is sliced at start / 640 for length // 640 frames (ValueError if it is too short), the
        slices are stacked and prepared by the ``"train"`` / ``"val"`` pipeline with the same ``rng``.  ``keys``: the target indices.
        ``rirs``: device room impulse responses (``datas.load_rirs``) for reverberant mixtures (DESIGN.md "Reverberant mixtures"): a
        drawn recipe gives every slot an RIR with probability ``rir_prob`` (offset 0: the room's delay stays in the audio), a given
        ``recipe`` carries its own indices; the SNR holds between the images and the target returned is the target's image scaled as
        slot 0, as in the dry call.  One more launch in front of the two.
        ``loudness`` = (low, high) with ``utter_lufs`` (the integrated loudness of every whole utterance, measured once per dataset with
        ``datas.loudness_many``; a host sequence): a drawn recipe sets every slot to a target in LUFS uniform in ``loudness`` with the
        fixed gain 10^((target - utter_lufs) / 20) instead of an SNR (``datas.MixRecipe.lufs``; DESIGN.md "Loudness"); with RIRs the
        level is that of the dry utterance.  Without the two arguments the call draws and returns what it always did."""
        from . import datas
        sources, mouth_rois = list(sources), list(mouth_rois)
        if len(mouth_rois) != len(sources):
            raise ValueError(f"System.mix_batch: {len(sources)} utterance(s) and {len(mouth_rois)} ROI track(s)")
        if recipe is None:
            B = int(self.config.get("training", {}).get("batch_size", 4))  # the yaml's training.batch_size
            recipe = datas.draw_mix_recipe([int(s.shape[0]) for s in sources], B, length, n_src=n_src, snr_db=snr_db, align=640, rng=rng,
                                           n_rirs=None if rirs is None else len(rirs), rir_prob=rir_prob, loudness=loudness,
                                           utter_lufs=utter_lufs)
        Tv = int(length) // 640
        keys = [int(t) for t in recipe.src[:, 0]]
        if Tv < 1:
            raise ValueError(f"System.mix_batch: length {length} holds no video frame")
        tracks = []
        for b, t in enumerate(keys):
            if t < 0:
                raise ValueError(f"System.mix_batch: row {b} has no target in slot 0")
            roi, f0 = mouth_rois[t], int(recipe.start[b, 0]) // 640
            if not isinstance(roi, torch.Tensor) or roi.dtype != torch.uint8 or roi.ndim != 3 or roi.shape[0] < f0 + Tv:
                raise ValueError(f"System.mix_batch: ROI track {t} must be uint8 (Tv,H,W) with at least {f0 + Tv} frames for a segment "
                                 f"that starts at sample {int(recipe.start[b, 0])}; got "
                                 f"{(tuple(roi.shape), roi.dtype) if isinstance(roi, torch.Tensor) else type(roi).__name__}")
            tracks.append(roi[f0:f0 + Tv])
        inputs, targets = datas.mix_batch(sources, recipe, length, n_out=1, normalize=normalize_audio, rirs=rirs)
        lips = datas.get_preprocessing_pipelines()["train" if train else "val"](torch.stack(tracks), rng=rng)
        return inputs, targets[:, 0], lips, keys

    def forward_grouped(self, wav, mouth=None):
        """``forward`` for a batch that may list each mixture once per target speaker, as the reference's test batches do (test.py:128-140,
        avspeech_dataset.py:81-84: n_src 1, no shuffling, the entries of one mixture side by side).  wav (N,L) or (N,1,L) -> (N,1,L) in
        input order.  Runs of bit-identical consecutive mixture rows are found with one device reduction and one host read; if every run has
        the same length K > 1, the batch goes through ``separate_speakers`` (the audio prefix once per mixture); runs of different lengths
        (at most 16, at least one of 2 or more) go through ``separate_speakers`` with the run lengths as ``counts``; a batch without a
        repeated mixture goes through ``forward``.  Not capturable in a HIP graph: the routing reads the batch's contents back to the host."""
        if mouth is None or wav.ndim not in (2, 3) or wav.shape[0] < 2 or wav.dtype != torch.float32:
            return self(wav, mouth)
        N = int(wav.shape[0])
        bits = wav.reshape(N, -1).contiguous().view(torch.int32)
        same = (bits[1:] == bits[:-1]).all(dim=1).tolist()  # row i + 1 repeats row i
        starts = [0] + [i + 1 for i, s in enumerate(same) if not s] + [N]
        counts = [b - a for a, b in zip(starts[:-1], starts[1:])]
        runs = set(counts)
        L = bits.shape[1]
        if max(runs) < 2 or (len(runs) != 1 and max(runs) > 16):
            return self(wav, mouth)
        if len(runs) != 1:  # a different number of targets per mixture: the first row of every run, the lips as they lie
            return self.separate_speakers(wav.reshape(N, L)[starts[:-1]].contiguous(), mouth, counts=counts).reshape(N, 1, L)
        K = runs.pop()
        out = self.separate_speakers(wav.reshape(N, L)[::K].contiguous(), mouth.reshape(N // K, K, *mouth.shape[1:]))
        return out.reshape(N, 1, L)

    def common_step(self, batch, batch_nb, is_train=True):
        """core.py:94-118."""
        if self.video_model is None and len(batch) == 4:  # extension: pre-computed lip embeddings in the mouth slot
            inputs, targets, mouth_emb, _ = batch
            est_targets = self.audio_model(inputs, mouth_emb)
        elif self.video_model is None:
            inputs, targets, _ = batch
            if self.config.get("training", {}).get("online_mix"):  # core.py:96-97
                inputs, targets = self.online_mixing_collate((batch[0], batch[1]))
            est_targets = self(inputs)
        else:
            inputs, targets, target_mouths, _ = batch
            est_targets = self(inputs, target_mouths)
        if targets.ndim == 2:
            targets = targets.unsqueeze(1)
        return self.loss_func["train" if is_train else "val"](est_targets, targets)

    def training_step(self, batch, batch_nb):
        """core.py:119-123: the loss tensor carries the HIP backward graph (AVNet.forward_train + the PIT loss gradient kernel)."""
        return {"loss": self.common_step(batch, batch_nb, is_train=True)}

    def validation_step(self, batch, batch_nb):
        with torch.no_grad():
            return {"val_loss": self.common_step(batch, batch_nb, is_train=False)}

    # ---------------------------------------------------------------- what Lightning does around training_step (train.py:135-148)
    def convert_sync_batchnorm(self):
        """What Lightning's ``sync_batchnorm=True`` (train.py:145) does: BatchNorm layers become nn.SyncBatchNorm, which the training
        kernels synchronise with two small all-reduces per layer (batch statistics forward, dgamma / dbeta sums backward)."""
        self.audio_model = nn.SyncBatchNorm.convert_sync_batchnorm(self.audio_model)
        return self

    def trainable_parameters(self):
        return [p for p in self.audio_model.parameters() if p.requires_grad]

    def allreduce_gradients(self):
        """Average the gradients over the data-parallel ranks with ONE collective on one flattened buffer (739,952 floats for
        RTFS-Net; backend nccl = RCCL over xGMI on the GPU box, gloo in the CPU tests).  No-op without a process group."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return 0
        params = [p for p in self.trainable_parameters()]
        if not params:
            return 0
        flat = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in params])
        dist.all_reduce(flat, op=dist.ReduceOp.SUM)
        flat.div_(dist.get_world_size())
        off = 0
        for p in params:
            n = p.numel()
            p.grad = flat[off:off + n].view_as(p).clone()
            off += n
        return flat.numel()

    def broadcast_parameters(self, src=0):
        """What DistributedDataParallel does at construction (train.py:135-146 runs under Lightning's DDP strategy): every rank starts
        from rank `src`'s parameters AND buffers (BatchNorm running statistics), so ranks that were seeded differently cannot drift apart
        silently.  One broadcast of one flattened float buffer (+ one for the integer buffers).  No-op without a process group."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return 0
        tensors = [t for t in list(self.audio_model.parameters()) + list(self.audio_model.buffers())]
        done = 0
        for is_float in (True, False):
            group = [t for t in tensors if t.is_floating_point() == is_float]
            if not group:
                continue
            flat = torch.cat([t.detach().reshape(-1).to(torch.float32 if is_float else torch.int64) for t in group])
            dist.broadcast(flat, src=src)
            off = 0
            with torch.no_grad():
                for t in group:
                    n = t.numel()
                    t.copy_(flat[off:off + n].view_as(t).to(t.dtype))  # in place through the tensor itself: bumps _version (pack caches)
                    off += n
            done += flat.numel()
        self._params_broadcast = True
        return done

    def optimization_step(self, batch, batch_nb=0, gradient_clip_val=5.0):
        """zero_grad -> training_step -> backward -> gradient all-reduce -> clip (train.py:142 gradient_clip_val 5.0) -> optimizer step.
        The first step of a multi-rank job broadcasts rank 0's parameters and buffers first (DDP's construction-time broadcast).

        With the package's own ``optimizers.AdamW`` (``make_optimizer(..., optimizer="adamw")``) everything after backward runs on the
        device in two launches: one gathers the gradients into the optimizer's flat buffer, a multi-rank job all-reduces THAT buffer once
        (no cat, no per-parameter copies, the 1 / world folded into the update), one clips and updates.  The total gradient norm stays on
        the device in ``self.last_grad_norm`` (the optimizer's buffer: the next step overwrites it).  On this route ``p.grad`` is left as
        backward wrote it - local, unscaled, unclipped - whereas the stock route below leaves the averaged, clipped gradients there; the
        clip covers the optimizer's parameters.  Any other optimizer takes the stock route."""
        if self.optimizer is None:
            raise RuntimeError("System.optimization_step needs an optimizer")
        if not getattr(self, "_params_broadcast", False):
            self.broadcast_parameters()
            self._params_broadcast = True
        self.optimizer.zero_grad(set_to_none=True)
        loss = self.training_step(batch, batch_nb)["loss"]
        loss.backward()
        from .optimizers import AdamW
        if isinstance(self.optimizer, AdamW):
            import torch.distributed as dist
            world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
            flat = self.optimizer.gather_grads(zero_missing=world > 1)
            if world > 1:
                dist.all_reduce(flat, op=dist.ReduceOp.SUM)
            self.last_grad_norm = self.optimizer.step(max_norm=gradient_clip_val, grad_scale=1.0 / world)
            return loss.detach()
        self.allreduce_gradients()
        if gradient_clip_val:
            torch.nn.utils.clip_grad_norm_(self.trainable_parameters(), gradient_clip_val)
        self.optimizer.step()
        return loss.detach()

    # ---------------------------------------------------------------- on-disk formats
    def load_lightning_checkpoint(self, path, strict=True):
        """Lightning ``.ckpt``: {"state_dict": {"audio_model.*", "video_model.*"}, "training_config": ...}."""
        ckpt = torch.load(path, map_location="cpu", weights_only=True) if isinstance(path, str) else path
        sd = ckpt["state_dict"]
        audio = {k[len("audio_model."):]: v for k, v in sd.items() if k.startswith("audio_model.")}
        video = {k[len("video_model."):]: v for k, v in sd.items() if k.startswith("video_model.")}
        self.audio_model.load_state_dict(audio, strict=strict)
        if self.video_model is not None and video:
            self.video_model.load_state_dict(video, strict=strict)
        return ckpt.get("training_config")


def load_best_model(path, **audionet_kwargs):
    """``best_model.pth`` (train.py:156-160 -> BaseAVModel.serialize) -> AVNet, as test.py:38-39 does."""
    from .models import AVNet
    return AVNet.from_pretrain(path, **audionet_kwargs)
