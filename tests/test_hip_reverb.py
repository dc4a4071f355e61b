"""Reverberant images on the device (rtfs-net_amd/datas.py reverberate, csrc/k_reverb.hip) against tests/reverb_oracle.py, within the
oracle's derived per-sample bound, at the edges where the kernel can go wrong (T = REVERB_TILE and C = REVERB_TAP_CHUNK read from the
package).  Every source is a view at an odd sample offset into a larger buffer, every RIR a view at an odd 4-byte offset into one
allocation; everything an image must not touch is poison: NaN (float32) or +-32767 (int16) in front of and behind the view AND inside
the utterance outside [p + o - N + 1, p + o + L), NaN between the RIRs.  Outputs are compared whole.

1. taps x lengths: N in {1, 2, 3, 4, 5, C-1, C, C+1, 2C+3} x L in {1, 2, 5, T-1, T, T+1, 2T+3}, float32 and int16, three jobs a call;
2. start x offset: p in {0, 1, 3, N-2, N-1, N, N+1} x o in {0, 1, N-1}, the history crossing the utterance's first sample at every
   phase, and segments that end on the source's last sample with o > 0 (zeros past the end);
3. exact cases (==): h = [1], a shifted impulse, the offset that undoes the shift;
4. determinism: a job alone and inside a call of 7 with mixed N gives the same bits; one RIR shared by several jobs;
5. one case at training size against the np.convolve oracle;
6. refusals raise ValueError before any launch;
7. cases 1 - 4 again in child processes on poisoned memory (RTFS_POISON_WS = nan, big)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import reverb_oracle as RO

pytestmark = pytest.mark.gpu

POISONED = os.environ.get("RTFS_POISON_WS", "") not in ("", "0")


def D():
    from rtfs_net_amd import datas
    return datas


def TC():
    return D().REVERB_TILE, D().REVERB_TAP_CHUNK


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


class Jobs:
    """The jobs of one ``reverberate`` call.  add() builds a source of n_x samples whose only real samples are the ones the job's image
    touches; rir() packs an RIR at an odd 4-byte offset of the one RIR allocation."""

    def __init__(self, L, seed):
        self.L, self.rng = L, np.random.RandomState(seed)
        self.src_host, self.src_dev, self.rir_host, self.jobs = [], [], [], []

    def rir(self, h):
        self.rir_host.append(np.asarray(h, np.float32))
        return len(self.rir_host) - 1

    def random_rir(self, N):
        return self.rir((self.rng.randn(N) * np.exp(-3.0 * np.arange(N) / N)).astype(np.float32))

    def add(self, kind, p, o, r, n_x=None, off=1, data=None):
        L, N = self.L, self.rir_host[r].shape[0]
        n_x = p + L + 5 if n_x is None else n_x
        lo, hi = max(p + o - N + 1, 0), min(p + o + L, n_x)
        if kind == "f32":
            buf = np.full(off + n_x + 3, np.nan, np.float32)
            buf[off + lo:off + hi] = self.rng.randn(hi - lo).astype(np.float32) if data is None else data[lo:hi]
        else:
            buf = np.where(np.arange(off + n_x + 3) % 2 == 0, 32767, -32767).astype(np.int16)
            buf[off + lo:off + hi] = self.rng.randint(-20000, 20001, hi - lo).astype(np.int16)
        self.src_host.append(buf[off:off + n_x])
        self.src_dev.append(torch.from_numpy(buf).cuda()[off:off + n_x])
        self.jobs.append((len(self.src_host) - 1, p, r, o))
        return len(self.jobs) - 1

    def device_rirs(self):
        at, spans = 1, []
        for h in self.rir_host:
            spans.append(at)
            at += h.shape[0] + (1 if h.shape[0] % 2 else 2)  # the next one starts at an odd offset again
        flat = np.full(at + 1, np.nan, np.float32)
        for a, h in zip(spans, self.rir_host):
            flat[a:a + h.shape[0]] = h
        dev = torch.from_numpy(flat).cuda()
        views = [dev[a:a + h.shape[0]] for a, h in zip(spans, self.rir_host)]
        assert all((v.data_ptr() // 4) % 2 == 1 for v in views)
        return views

    def run(self):
        s, p, r, o = (np.array(v) for v in zip(*self.jobs))
        got = D().reverberate(self.src_dev, self.device_rirs(), s, p, r, self.L, offset=o)
        assert tuple(got.shape) == (len(self.jobs), self.L) and got.dtype == torch.float32
        return host(got)

    def oracle(self, i, exact=None):
        s, p, r, o = self.jobs[i]
        return RO.image64(self.src_host[s], p, self.rir_host[r], o, self.L, exact), RO.bound(self.src_host[s], p, self.rir_host[r], o, self.L, exact)

    def check(self, got, what, exact=None):
        worst = 0.0
        for i in range(len(self.jobs)):
            want, bar = self.oracle(i, exact)
            err = np.abs(got[i].astype(np.float64) - want)
            assert np.isfinite(got[i]).all(), f"{what} job {i} {self.jobs[i]}: not finite"
            ratio = float((err / np.maximum(bar, 1e-300)).max())
            worst = max(worst, ratio)
            assert (err <= bar).all(), f"{what} job {i} {self.jobs[i]}: error / bound {ratio:.3f} at t = {int((err / np.maximum(bar, 1e-300)).argmax())}"
        return worst


def tap_counts():
    T, C = TC()
    return [1, 2, 3, 4, 5, C - 1, C, C + 1, 2 * C + 3]


def lengths():
    T, C = TC()
    return [1, 2, 5, T - 1, T, T + 1, 2 * T + 3]


# ---------------------------------------------------------------- 1. taps x lengths
@pytest.mark.parametrize("n", range(9))
def test_sweep_taps_and_lengths(n):
    N = tap_counts()[n]
    for L in lengths():
        j = Jobs(L, seed=1000 * n + L)
        h = j.random_rir(N)
        j.add("f32", p=0, o=0, r=h, off=1)                                  # all history in front of the utterance
        j.add("i16", p=N + 1, o=min(1, N - 1), r=h, off=3)                  # all history inside it
        j.add("f32", p=1, o=N - 1, r=h, n_x=1 + L, off=2)                   # ends on the last sample; o > 0 reads past it
        worst = j.check(j.run(), f"N {N} L {L}")
        print(f"[reverb] N {N} L {L}: worst error / bound {worst:.3f}")


# ---------------------------------------------------------------- 2. start x offset
@pytest.mark.parametrize("N", [5, "C+1"])
@pytest.mark.parametrize("L", [37, "T+1"])
def test_sweep_start_and_offset(N, L):
    T, C = TC()
    N, L = (C + 1 if N == "C+1" else N), (T + 1 if L == "T+1" else L)
    j = Jobs(L, seed=N + L)
    h = j.random_rir(N)
    for i, p in enumerate([0, 1, 3, N - 2, N - 1, N, N + 1]):
        for o in (0, 1, N - 1):
            kind = "i16" if (i + o) % 3 == 1 else "f32"
            j.add(kind, p=p, o=o, r=h, n_x=p + L if o else None, off=1 + 2 * (i % 3))  # o > 0: the segment ends on the last sample
    assert len(j.jobs) == 21
    j.check(j.run(), f"start/offset N {N} L {L}")


# ---------------------------------------------------------------- 3. exact cases
@pytest.mark.parametrize("L", ["5", "T-1", "2T+3"])
def test_exact_impulses(L):
    T, C = TC()
    L = {"5": 5, "T-1": T - 1, "2T+3": 2 * T + 3}[L]
    for d in (1, 4, C, C + 2):
        j = Jobs(L, seed=L + d)
        one, delta = j.rir([1.0]), j.rir(np.eye(1, d + 3, d, dtype=np.float32)[0])
        x = j.rng.randn(L + d + 20).astype(np.float32)
        x[::7] = 0.0
        x[3::14] = -0.0
        p = 3
        j.add("f32", p=p, o=0, r=one, n_x=x.shape[0], data=x)       # the segment itself
        j.add("f32", p=p, o=0, r=delta, n_x=x.shape[0], data=x)     # shifted by d, zeros shifted in (p < d) or history (p >= d)
        j.add("f32", p=p, o=d, r=delta, n_x=x.shape[0], data=x)     # the offset undoes the shift
        j.add("f32", p=d + 2, o=0, r=delta, n_x=x.shape[0], data=x)
        j.add("i16", p=p, o=0, r=one)
        got = j.run()
        seg = x[p:p + L]
        shifted = np.concatenate([np.zeros(max(d - p, 0), np.float32), x[max(p - d, 0):]])[:L]
        assert (got[0] == seg).all() and (got[2] == seg).all(), (L, d)
        assert (got[1] == shifted).all() and (got[3] == x[2:2 + L]).all(), (L, d)
        pcm = j.src_host[4][p:p + L]
        assert (got[4] == pcm.astype(np.float32) / np.float32(32768)).all()


# ---------------------------------------------------------------- 4. determinism, shared RIRs, S = 1 and S = 7
def test_one_job_alone_and_among_seven_with_mixed_taps():
    T, C = TC()
    L = T + 5
    j = Jobs(L, seed=77)
    hs = [j.random_rir(N) for N in (C + 1, 3, 2 * C + 3, 1)]
    picks = [(0, "f32", 5, 2), (1, "i16", 0, 1), (0, "f32", C, 0), (2, "f32", 9, 2 * C + 2), (3, "i16", 4, 0), (0, "i16", 1, C), (2, "f32", 0, 0)]
    for r, kind, p, o in picks:
        j.add(kind, p=p, o=o, r=hs[r], n_x=p + L + (0 if o else 4))
    got = j.run()
    j.check(got, "seven jobs")
    views = j.device_rirs()
    for i, (s, p, r, o) in enumerate(j.jobs):  # S = 1: the same job on the same memory
        alone = host(D().reverberate([j.src_dev[s]], [views[r]], [0], [p], [0], L, offset=[o]))
        assert alone.shape == (1, L) and np.array_equal(alone[0].view(np.int32), got[i].view(np.int32)), f"job {i}"
    again = j.run()
    assert np.array_equal(again.view(np.int32), got.view(np.int32))


# ---------------------------------------------------------------- 5. training size
def test_training_size_against_convolve():
    L, N = 32000, 4096
    j = Jobs(L, seed=5)
    rng = np.random.RandomState(6)
    h0 = j.rir(D().synthetic_rir(N, 0.4, delay=40, rng=rng))
    h1 = j.rir(D().synthetic_rir(N, 0.25, delay=12, drr_db=5.0, rng=rng))
    j.add("f32", p=6400, o=40, r=h0, n_x=6400 + L + 640)
    j.add("i16", p=1280, o=12, r=h1, n_x=1280 + L)  # the history crosses the first sample; ends on the last one
    worst = j.check(j.run(), "training size", exact=False)
    print(f"[reverb] S 2 L {L} N {N}: worst error / bound {worst:.3f} (np.convolve oracle)")


# ---------------------------------------------------------------- 6. refusals
def test_refusals_raise_before_any_launch():
    from rtfs_net_amd import _lib
    M = D()
    x, y = torch.zeros(100, device="cuda"), torch.zeros(100, dtype=torch.int16, device="cuda")
    h = torch.ones(8, device="cuda")
    before = _lib.load().rtfs_debug_launch_count()
    bad = [lambda: M.reverberate([x], [h], [0], [51], [0], 50),                       # a segment past its source
           lambda: M.reverberate([x], [h], [0], [-1], [0], 50),
           lambda: M.reverberate([x], [h], [0], [0], [0], 50, offset=[8]),            # offset = taps
           lambda: M.reverberate([x], [h], [0], [0], [0], 50, offset=[-1]),
           lambda: M.reverberate([x], [h], [0], [0], [1], 50),                        # an RIR that is not there
           lambda: M.reverberate([x], [h], [1], [0], [0], 50),                        # a source that is not there
           lambda: M.reverberate([x], [h], [-1], [0], [0], 50),
           lambda: M.reverberate([x], [h], [0], [0], [0], 0),
           lambda: M.reverberate([x], [h], [0, 0], [0], [0], 50),                     # arrays of different lengths
           lambda: M.reverberate([x], [h], [], [], [], 50),
           lambda: M.reverberate([x], [torch.ones(16385, device="cuda")], [0], [0], [0], 50),
           lambda: M.reverberate([x], [h[:0]], [0], [0], [0], 50),                    # no taps
           lambda: M.reverberate([x], [h.double()], [0], [0], [0], 50),
           lambda: M.reverberate([x], [h.cpu()], [0], [0], [0], 50),
           lambda: M.reverberate([x], [h[::2]], [0], [0], [0], 50),
           lambda: M.reverberate([x.cpu()], [h], [0], [0], [0], 50),
           lambda: M.reverberate([x.double()], [h], [0], [0], [0], 50),
           lambda: M.mix_batch([x], M.MixRecipe([[0]], [[0]], [[1.0]], rir=[[1]]), 50, rirs=[h]),
           lambda: M.mix_batch([x], M.MixRecipe([[0]], [[0]], [[1.0]], rir=[[0]]), 50),                        # indices without RIRs
           lambda: M.mix_batch([x], M.MixRecipe([[0]], [[0]], [[1.0]], rir=[[0]], rir_offset=[[8]]), 50, rirs=[h]),
           lambda: M.mix_batch([x, y], M.MixRecipe([[0, 1]], [[0, 0]], [[1.0, 1.0]], [[-1, 0]], [[0, 51]], rir=[[0, 0]]), 50, rirs=[h])]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    assert _lib.load().rtfs_debug_launch_count() == before
    r = M.reverberate([x, y], [h], [0, 1], [50, 50], [0, 0], 50, offset=[7, 0])  # the last 50 samples of both: accepted, one launch
    assert _lib.load().rtfs_debug_launch_count() == before + 1 and float(r.abs().max()) == 0.0


# ---------------------------------------------------------------- 7. poisoned memory
FORWARD_CASES = "test_sweep or test_exact or test_one_job"
ABNORMAL = (124, 134, 137, 139)


@pytest.mark.skipif(POISONED, reason="already inside a poisoned run")
def test_poisoned():
    """Cases 1 - 4 in a fresh child process per pattern, with every output a C call fills poisoned (tests/test_hip_mix.py's discipline:
    a time limit per child, and no second child after one that did not exit cleanly)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for pattern in ("nan", "big"):
        env = dict(os.environ, RTFS_POISON_WS=pattern)
        try:
            pr = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_hip_reverb.py"), "-m", "gpu", "-q", "-p",
                                 "no:cacheprovider", "-k", FORWARD_CASES], cwd=root, env=env, capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired:
            pytest.fail(f"RTFS_POISON_WS={pattern}: timed out after 300 s; no further child started")
        if pr.returncode < 0 or pr.returncode in ABNORMAL:
            pytest.fail(f"RTFS_POISON_WS={pattern}: abnormal exit status {pr.returncode}; no further child started\n{pr.stdout[-3000:]}")
        assert pr.returncode == 0, f"RTFS_POISON_WS={pattern}: exit status {pr.returncode}\n{pr.stdout[-3000:]}\n{pr.stderr[-2000:]}"
