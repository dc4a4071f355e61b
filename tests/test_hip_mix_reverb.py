"""Reverberant training mixtures on the device (rtfs-net_amd/datas.py mix_batch(rirs=...), csrc/k_reverb.hip in front of csrc/k_mix.hip;
System.mix_batch(rirs=...)) against tests/reverb_oracle.py and tests/mix_oracle.py.  Sources are views at odd offsets into buffers that
are NaN / +-32767 outside the view; inside, every sample is real, because an image reads its history from the utterance.

1. without RIRs nothing changes: ``rirs=None`` is the dry call (bit-equal to the oracle's exact tier), a recipe whose RIR indices are
   all -1 next to a list of RIRs is bit-equal to it, stats included; all-impulse RIRs (h = [1]) are bit-equal to the dry call;
2. general recipes, B 1 / 3, J 1 .. 4, dry and reverberant slots in one row, int16 next to float32, n_out 0 .. J (every value at
   L = 5, one per recipe above that), with and without ``normalize``, L in {5, T + 1, 8195}:
   (a) the image tensor against the oracle's images within the oracle's bound, one row per distinct (source, start, RIR, offset);
   (b) outputs BIT-equal to ``mix_oracle.mix_given_stats`` fed the device's own images and stats;
   (c) outputs against ``reverb_oracle.mix`` from the samples alone at the project's bar, 1e-4 max-rel / 1e-5 l2-rel;
   (d) the SNR between the target's and each interferer's scaled image, from float64 energies of the returned images and the gains in
       stats, equals the drawn value to 1e-9 relative;
   normalised cases keep mix_oracle.max_abs_corr <= 0.9 and kappa < 1e5 on the oracle's images, checked on the CPU first;
3. ``System.mix_batch(rirs=...)``: the batch is the ``datas.mix_batch`` one, and ``optimization_step`` takes it."""
import random

import numpy as np
import pytest
import torch

from tests import mix_oracle as MO
from tests import reverb_oracle as RO
from tests.test_hip_mix import check_rows, same_bits

pytestmark = pytest.mark.gpu

J = 4
MAX_CORR, MAX_KAPPA = 0.9, 1e5  # tests/test_hip_mix.py
DBS = [-5.0, 2.5, 4.0]


def D():
    from rtfs_net_amd import datas
    return datas


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


class Pool:
    """Six float32 and three int16 utterances of n samples, each a view at an odd offset; three RIRs in one allocation."""

    def __init__(self, n, seed, taps=(7, 24, 64)):
        rng = np.random.RandomState(seed)
        self.host, self.dev = [], []
        for i in range(9):
            off = 1 + 2 * (i % 3)
            if i < 6:
                buf = np.full(off + n + 2, np.nan, np.float32)
                buf[off:off + n] = (0.3 + 0.2 * i) * rng.randn(n)
            else:
                buf = np.where(np.arange(off + n + 2) % 2 == 0, 32767, -32767).astype(np.int16)
                buf[off:off + n] = np.clip(np.rint(6000.0 * rng.randn(n)), -32000, 32000)
            self.host.append(buf[off:off + n])
            self.dev.append(torch.from_numpy(buf).cuda()[off:off + n])
        self.rirs = [D().synthetic_rir(N, 0.002 * N / 16.0 + 0.001, delay=min(3, N - 1), drr_db=2.0, rng=rng) for N in taps]
        self.dev_rirs, self.offsets = D().load_rirs(self.rirs)
        self.cache = {}

    def images_for(self, rec, L):
        """The oracle's images of a recipe, each computed once per pool: reverb_oracle.as_dry with the cache filled for this recipe."""
        src, start, _, ref_src, ref_start, rir, ref_rir, off, ref_off = (np.asarray(v) for v in rec)
        for s, p, r, o in list(zip(src.ravel(), start.ravel(), rir.ravel(), off.ravel())) + \
                list(zip(ref_src.ravel(), ref_start.ravel(), ref_rir.ravel(), ref_off.ravel())):
            key = (int(s), int(p), int(r), int(o))
            if s >= 0 and r >= 0 and (key, L) not in self.cache:
                self.cache[(key, L)] = (RO.image64(self.host[key[0]], key[1], self.rirs[key[2]], key[3], L),
                                        RO.bound(self.host[key[0]], key[1], self.rirs[key[2]], key[3], L))
        return {k: v[0].astype(np.float32) for (k, l), v in self.cache.items() if l == L}


def recipe_arrays(r):
    return (r.src, r.start, r.a, r.ref_src, r.ref_start, r.rir, r.ref_rir, r.rir_offset, r.ref_offset)


def snr_recipe(pool, B, Jr, L, seed):
    """B rows of a target and Jr - 1 interferers at DBS; per slot an RIR or none (row 0 reverberates everything, the others mix dry and
    reverberant slots, one of them with a dry target), offsets 0 or the RIR's direct path, starts that cut into the history."""
    rng = random.Random(seed)
    n = pool.host[0].shape[0]
    t, k, s, rr, oo = [], [], [], [], []
    for b in range(B):
        row = rng.sample(range(9), Jr)
        t.append(row[0])
        k.append(row[1:])
        s.append([rng.choice([0, 1, 5, 64, n - L]) for _ in row])
        if b == 0:
            picks = [rng.randrange(3) for _ in row]
        else:
            picks = [rng.choice([-1, 0, 1, 2]) for _ in row]
            picks[0] = -1 if b == 1 else rng.randrange(3)
            if Jr > 1 and b == 1:
                picks[1] = 2
        rr.append(picks)
        oo.append([0 if i < 0 else rng.choice([0, pool.offsets[i]]) for i in picks])
    return D().MixRecipe.snr(t, k, s, [DBS[:Jr - 1]] * B if Jr > 1 else 0.0, rirs=rr, offsets=oo)


# ---------------------------------------------------------------- 1. without RIRs nothing changes
@pytest.mark.parametrize("L", [5, "T+1"])
def test_without_rirs_the_call_is_the_dry_call(L):
    L = D().REVERB_TILE + 1 if L == "T+1" else L
    pool = Pool(L + 200, seed=L)
    rows = np.array([[0, 6, 1, 2], [3, -1, 7, -1], [8, 4, 0, -1]])
    start = np.array([[5, 0, 64, 1], [200, 0, 3, 0], [7, 9, 11, 0]])
    a = np.where(rows >= 0, np.array([[1.0, 0.5, -0.25, 3.0]] * 3), 0.0)
    dry = D().MixRecipe(rows, start, a)
    want_m, want_s, _ = MO.mix(pool.host, (dry.src, dry.start, dry.a, dry.ref_src, dry.ref_start), L, J)
    m0, s0, st0 = D().mix_batch(pool.dev, dry, L, n_out=J, return_stats=True)
    assert same_bits(host(m0), want_m) and same_bits(host(s0), want_s)  # the exact tier of tests/test_hip_mix.py
    res = D().mix_batch(pool.dev, dry, L, n_out=J, return_stats=True, rirs=None, return_images=True)
    assert len(res) == 5 and tuple(res[3].shape) == (0, L) and (res[4] == -1).all() and res[4].shape == (3, 4)
    m1, s1, st1, im, imap = D().mix_batch(pool.dev, dry, L, n_out=J, return_stats=True, rirs=pool.dev_rirs, return_images=True)  # indices all -1
    assert tuple(im.shape) == (0, L) and (imap == -1).all()
    for u, v in ((m0, m1), (s0, s1), (st0, st1), (m0, res[0]), (s0, res[1]), (st0, res[2])):
        assert same_bits(host(u), host(v))
    # the energy rule and normalisation too, and all-impulse RIRs: the image of h = [1] is the segment
    one = [torch.ones(1, device="cuda")]
    for normalize in (False, True):
        snr = snr_recipe(pool, 3, 3, L, seed=L)
        plain = D().MixRecipe(snr.src, snr.start, snr.a, snr.ref_src, snr.ref_start)
        m0, s0, st0 = D().mix_batch(pool.dev, plain, L, normalize=normalize, return_stats=True)
        m1, s1, st1 = D().mix_batch(pool.dev, plain, L, normalize=normalize, return_stats=True, rirs=pool.dev_rirs)
        imp = D().MixRecipe(snr.src, snr.start, snr.a, snr.ref_src, snr.ref_start, rir=np.where(snr.src >= 0, 0, -1),
                            ref_rir=np.where(snr.ref_src >= 0, 0, -1))
        m2, s2, st2, im, imap = D().mix_batch(pool.dev, imp, L, normalize=normalize, return_stats=True, rirs=one, return_images=True)
        assert (imap >= 0).all() and tuple(im.shape) == (int(imap.max()) + 1, L)
        for u, v in ((m0, m1), (s0, s1), (st0, st1), (m0, m2), (s0, s2), (st0, st2)):
            assert same_bits(host(u), host(v)), normalize
        for b in range(3):
            for j in range(3):
                seg = MO.segment(pool.host, imp.src[b, j], imp.start[b, j], L).astype(np.float32)
                assert (host(im)[imap[b, j]] == seg).all()


# ---------------------------------------------------------------- 2. general recipes
def check_general(pool, r, L, n_out, normalize, what):
    rec = recipe_arrays(r)
    B, Jr = r.shape
    cache = pool.images_for(rec, L)
    opool, dry, oimages, omap = RO.as_dry(pool.host, pool.rirs, rec, L, images=cache)
    if normalize:  # on the CPU, before the device is asked: no mixture that cancels
        assert L < 31 or MO.max_abs_corr(opool, dry, L) <= MAX_CORR, what
        assert MO.moment_bounds(opool, dry, L)[2].max() < MAX_KAPPA, what
    m, s, st, im, imap = D().mix_batch(pool.dev, r, L, n_out=n_out, normalize=normalize, return_stats=True, rirs=pool.dev_rirs, return_images=True)
    assert tuple(m.shape) == (B, L) and tuple(s.shape) == (B, n_out, L) and tuple(st.shape) == (B, J + 2) and st.dtype == torch.float64
    m, s, st, im = host(m), host(s), host(st), host(im)
    # (a) one row per distinct image, in the oracle's order, each within the bound
    assert np.array_equal(imap, omap) and im.shape == (len(oimages), L) and imap.dtype == np.int64
    keys = {}
    for b in range(B):
        for j in range(Jr):
            if imap[b, j] >= 0:
                keys[int(imap[b, j])] = (int(r.src[b, j]), int(r.start[b, j]), int(r.rir[b, j]), int(r.rir_offset[b, j]))
    for row, key in keys.items():
        want, bar = pool.cache[(key, L)]
        assert (np.abs(im[row].astype(np.float64) - want) <= bar).all(), f"{what}: (a) image {row} {key}"
    # (b) bit-equal to the documented float64 formulas on the device's own images and stats
    given = {key: im[row] for row, key in keys.items()}
    for key in cache:  # a reference's image that no slot holds: the oracle's
        given.setdefault(key, cache[key])
    dpool, ddry, _, _ = RO.as_dry(pool.host, pool.rirs, rec, L, images=given)
    exp_m, exp_s = MO.mix_given_stats(dpool, ddry, L, n_out, st, normalize=normalize)
    assert same_bits(m, exp_m), f"{what}: (b) mixture"
    assert same_bits(s, exp_s), f"{what}: (b) sources"
    # (c) from the samples alone
    want_m, want_s, want_st = MO.mix(opool, dry, L, n_out, normalize=normalize)
    check_rows(m, want_m, f"{what}: (c) mixture")
    if n_out:
        check_rows(s, want_s, f"{what}: (c) sources")
    # (d) the drawn SNR holds between the scaled images
    for b in range(B):
        sig = [im[imap[b, j]].astype(np.float64) if imap[b, j] >= 0 else MO.segment(pool.host, r.src[b, j], r.start[b, j], L) for j in range(Jr)]
        e = [float(x @ x) for x in sig]
        for j in range(1, Jr):
            if r.ref_rir[b, j] != r.rir[b, 0]:
                continue
            db = 10.0 * np.log10(st[b, 0] ** 2 * e[0] / (st[b, j] ** 2 * e[j]))
            assert abs(db - DBS[j - 1]) <= 1e-9 * abs(DBS[j - 1]), f"{what}: (d) row {b} slot {j}: {db} dB, drawn {DBS[j - 1]}"


@pytest.mark.parametrize("L", [5, "T+1", 8195])
@pytest.mark.parametrize("B", [1, 3])
def test_general_recipes(B, L):
    L = D().REVERB_TILE + 1 if L == "T+1" else L
    pool = Pool(L + 150, seed=10 * B + L)
    for Jr in (1, 2, 3, 4):
        r = snr_recipe(pool, B, Jr, L, seed=100 * B + 10 * Jr + L)
        assert r.reverberant
        for normalize in (False, True):
            if normalize and L < 31:
                continue  # five samples: tests/test_hip_mix.py's moment conditions say nothing there
            for n_out in (range(J + 1) if L == 5 else [(Jr + normalize) % (J + 1)]):
                check_general(pool, r, L, n_out, normalize, f"B {B} J {Jr} L {L} n_out {n_out} normalize {normalize}")


# ---------------------------------------------------------------- 3. System.mix_batch
def test_system_mix_batch_with_rirs_and_one_optimization_step():
    from tests.test_hip_mix import small_system, utterance_pool
    s, length, B = small_system(), 4096, 2
    lengths, wavs, rois = utterance_pool(length, seed=31)
    dw, dr = [torch.from_numpy(w).cuda() for w in wavs], [torch.from_numpy(r).cuda() for r in rois]
    rng = np.random.RandomState(3)
    rirs, offsets = D().load_rirs([D().synthetic_rir(N, 0.05, delay=d, rng=rng) for N, d in ((800, 5), (300, 0), (1500, 20))])
    batch = s.mix_batch(dw, dr, length=length, n_src=3, snr_db=(-3.0, 3.0), normalize_audio=True, rng=random.Random(21), rirs=rirs, rir_prob=0.7)
    rec = D().draw_mix_recipe(lengths, B, length, n_src=3, snr_db=(-3.0, 3.0), align=640, rng=random.Random(21), n_rirs=3, rir_prob=0.7)
    assert rec.reverberant and batch[3] == rec.src[:, 0].tolist()
    wm, ws, images, imap = D().mix_batch(dw, rec, length, n_out=1, normalize=True, rirs=rirs, return_images=True)
    assert torch.equal(batch[0], wm) and torch.equal(batch[1], ws[:, 0]) and tuple(batch[2].shape) == (B, 1, length // 640, 88, 88)
    # the target returned is the target's image, scaled as slot 0: collinear with the image row
    for b in range(B):
        if imap[b, 0] >= 0:
            tgt, img = host(batch[1])[b].astype(np.float64), host(images)[imap[b, 0]].astype(np.float64)
            img = img - img.mean()
            assert abs(tgt @ img) / np.sqrt((tgt @ tgt) * (img @ img)) > 1 - 1e-6
    value = s.optimization_step(batch, 0)
    torch.cuda.synchronize()
    assert np.isfinite(float(value))
