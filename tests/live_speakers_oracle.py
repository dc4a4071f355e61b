"""Numpy restatement (float64) of live streaming with K faces per stream (AVNet.open_streams(speakers=K) / SpeakerStreamPool,
rtfs_live_ingest_frame_speakers_f32), a thin layer on tests/live_oracle.py from the rules of DESIGN.md "Every face of a stream".
Nothing here imports the package under test.

A slot has one audio track and K lip tracks that are pushed together, so the counters, readiness, the capacity rule and the output
ranges are those of ONE stream: ``tick`` is live_oracle.tick with n_src := K.  The framed video of a tick is live_oracle.frame_rows per
track, stacked so that target row r K + k holds window r of track k, and the overlap-add is live_oracle.OverlapAdd with K sources."""
import numpy as np

from tests import live_oracle as VO
from tests import longform_oracle as LO

SPF = VO.SPF


def tick(counters, slot_ids, na, nf, window, hop, max_chunk, K, flush=False):
    return VO.tick(counters, slot_ids, na, nf, window, hop, max_chunk, K, flush)


def frame_rows(rows, hist, limits, window, hop, K):
    """hist: slot -> (x (a',), v (K, 512, f')); limits: slot -> (L, Tv).  -> xw (rows, window), written once per window, and
    vw (rows * K, 512, window / 640), row r K + k = window r of track k."""
    per = []
    for k in range(K):
        xw, vw = VO.frame_rows(rows, {s: (x, v[k]) for s, (x, v) in hist.items()}, limits, window, hop)
        per.append(vw)
    return xw, np.stack(per, axis=1).reshape(len(rows) * K, 512, window // SPF)


def OverlapAdd(window, hop, K):
    return VO.OverlapAdd(window, hop, K)


def frame_long(x, v, window, hop):
    """rtfs_longform_frame_speakers_f32: x (B,L), v (B,K,512,Tv) -> xw (B*N, window), vw (B*N*K, 512, Wv), target row (b N + n) K + k:
    longform_oracle.frame per track."""
    B, K = v.shape[:2]
    per = []
    for k in range(K):
        xw, vw = LO.frame(x, np.ascontiguousarray(v[:, k]), window, hop)
        per.append(vw)
    return xw, np.stack(per, axis=1).reshape(-1, 512, window // SPF)
