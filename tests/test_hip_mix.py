"""Training mixtures on the device (rtfs-net_amd/datas.py mix_batch, csrc/k_mix.hip; System.online_mixing_collate / System.mix_batch)
against tests/mix_oracle.py.  Every source is a view into a larger buffer in which everything but the one segment the recipes name is
NaN (float32) or +-32767 (int16), so a read outside a segment that enters a sum shows; outputs are compared whole.

1. exact tier: fixed gains, no normalisation: BIT-equal to the oracle's ``mix`` (nothing the device computes enters but one multiply
   and the ordered adds); J = 1 with a = 1 returns the segment itself;
2. energy rule (SNR recipes): (a) the gains in ``stats`` within (L + 16) 2^-53 relative of the oracle's exactly summed ones (squares are
   exact in double, any-order summation of L non-negative terms is within (L - 1) 2^-53, the ratio doubles and the root halves it);
   (b) outputs BIT-equal to ``mix_given_stats`` with the device's own stats; (c) outputs against ``mix`` at the project's bar;
3. the same with ``normalize=True``, a DC offset of 100 x the amplitude, amplitudes 1e-4 and 1e3, L = 1 -> NaN, and against
   ``normalize_mixture`` of the unnormalised call;
4. silence: the oracle's inf / NaN pattern in the same positions;
5. ``System.online_mixing_collate`` and the ``online_mix`` switch of ``common_step``;
6. ``System.mix_batch`` and one ``optimization_step`` on its batch;
7. refusals raise ValueError before any launch;
8. cases 1 - 3 again in child processes on poisoned memory (RTFS_POISON_WS = nan, big)."""
import copy
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mix_oracle as MO
from tests import prep_oracle as PO
from tests.util import l2_rel, rel_err

pytestmark = pytest.mark.gpu

POISONED = os.environ.get("RTFS_POISON_WS", "") not in ("", "0")
MAX_REL, L2_REL = 1e-4, 1e-5  # the project's bar for prepared audio (tests/test_hip_prep.py)
CHUNK, J = 4096, 4
LENGTHS = [1, 2, 3, 4, 5, 31, 32, 33, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3]
FACTORS = [1.0, 0.5, -0.25, 3.0]
MAX_CORR = 0.9     # |correlation| of any two scaled slots of a normalised case, from L = 31 on (below that a correlation says nothing)
MAX_KAPPA = 1e5    # mix_oracle.moment_bounds: the deviation from moments is then within (L + 16) 2^-53 1e5 < 4e-7 relative up to L = 32000


def D():
    from rtfs_net_amd import datas
    return datas


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def same_bits(a, b):
    """Bit-equal where the oracle is not NaN; NaN in exactly the same positions (a NaN's payload is not part of the definition)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    view = np.int32 if a.dtype == np.float32 else np.int64
    return np.array_equal(na, nb) and np.array_equal(a.view(view)[~na], b.view(view)[~nb])


class Pool:
    """Sources with ONE named segment each.  add() -> index; the source handed to the device is the view [off, off + start + L + tail)
    of its own buffer, poison everywhere outside [start, start + L): the allocation's samples in front of the view, the view's samples
    around the segment, and, with tail = 0, a segment that ends on the allocation's last sample."""

    def __init__(self, L, seed):
        self.L, self.rng, self.host, self.dev, self.start = L, np.random.RandomState(seed), [], [], []

    def add(self, kind="f32", off=0, start=0, tail=0, scale=1.0, dc=0.0, silent=False):
        L = self.L
        n = off + start + L + tail
        x = np.zeros(L) if silent else dc + scale * self.rng.randn(L)
        if kind == "f32":
            buf = np.full(n, np.nan, np.float32)
            buf[off + start:off + start + L] = x.astype(np.float32)
        else:
            buf = np.where(np.arange(n) % 2 == 0, 32767, -32767).astype(np.int16)
            full = abs(dc) + 4.0 * scale  # PCM has one scale: 4 deviations (+ the offset) at 30000
            buf[off + start:off + start + L] = np.clip(np.rint(x / full * 30000.0), -32000, 32000).astype(np.int16)
        self.host.append(buf[off:])
        self.dev.append(torch.from_numpy(buf).cuda()[off:])
        self.start.append(start)
        return len(self.host) - 1

    def recipe(self, rows, refs=None):
        """rows: per row a list of (source index or None, a); refs: per row a list of source index or None -> the five (B, Jr) arrays."""
        B, Jr = len(rows), max(len(r) for r in rows)
        src, start, a = np.full((B, Jr), -1, np.int64), np.zeros((B, Jr), np.int64), np.zeros((B, Jr))
        ref_src, ref_start = np.full((B, Jr), -1, np.int64), np.zeros((B, Jr), np.int64)
        for b, row in enumerate(rows):
            for j, (s, f) in enumerate(row):
                if s is None:
                    continue
                src[b, j], start[b, j], a[b, j] = s, self.start[s], f
                r = None if refs is None else refs[b][j]
                if r is not None:
                    ref_src[b, j], ref_start[b, j] = r, self.start[r]
        return src, start, a, ref_src, ref_start


def run(pool, rec, n_out, normalize=False):
    m, s, st = D().mix_batch(pool.dev, D().MixRecipe(*rec), pool.L, n_out=n_out, normalize=normalize, return_stats=True)
    assert tuple(m.shape) == (rec[0].shape[0], pool.L) and tuple(s.shape) == (rec[0].shape[0], n_out, pool.L) and m.dtype == s.dtype == torch.float32
    assert tuple(st.shape) == (rec[0].shape[0], J + 2) and st.dtype == torch.float64
    return host(m), host(s), host(st)


def check_rows(got, want, what):
    got, want = got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1])
    worst = (0.0, 0.0)
    for r in range(want.shape[0]):
        if not np.abs(want[r]).max() > 0:  # the source row of an empty slot
            assert np.array_equal(got[r], want[r]), f"{what} row {r}"
            continue
        e, l2 = rel_err(got[r], want[r]), l2_rel(got[r], want[r])
        worst = (max(worst[0], e), max(worst[1], l2))
        assert np.isfinite(got[r]).all() and e <= MAX_REL and l2 <= L2_REL, f"{what} row {r}: max-rel {e:.3e}, l2-rel {l2:.3e}"
    return worst


# ---------------------------------------------------------------- 1. exact tier
def exact_pool(L, seed):
    """Six float32 and four int16 sources at different phases against the 16-byte grid."""
    p = Pool(L, seed)
    for i in range(6):
        p.add("f32", off=i % 4, start=(3 * i + 1) % 7, tail=0 if i % 2 else 5)
    for i in range(4):
        p.add("i16", off=(3 * i) % 8, start=(5 * i + 2) % 9, tail=0 if i % 2 else 3)
    return p


@pytest.mark.parametrize("L", LENGTHS)
def test_exact_fixed_gains_are_bit_equal(L):
    p = exact_pool(L, seed=L)
    f = FACTORS
    rows = [[(0, f[0]), (6, f[1]), (1, f[2]), (2, f[3])],       # J = 4, int16 and float32 in one row
            [(3, f[0]), (None, 0.0), (7, f[2]), (None, 0.0)],  # empty slots in the middle and at the end
            [(8, f[0]), (4, f[1]), (0, f[2])],                  # J = 3, a source of row 0 again
            [(None, 0.0), (5, f[1]), (9, f[2])],                # an empty slot in front
            [(1, f[0]), (1, f[1])]]                             # J = 2, the same segment twice
    rec = p.recipe(rows)
    want_m, want_s, want_st = MO.mix(p.host, rec, L, J)
    got_m, got_s, got_st = run(p, rec, J)
    assert same_bits(got_m, want_m) and same_bits(got_s, want_s), f"L {L}"
    assert np.array_equal(got_st[:, :J], want_st[:, :J])  # fixed gains: a itself, 0 for an empty slot
    if L > 1:  # mean and 1 / (std + eps) come from the moments: within the bound the oracle derives from the samples
        dm, di, _ = MO.moment_bounds(p.host, rec, L)
        assert (np.abs(got_st[:, J] - want_st[:, J]) <= dm).all(), (got_st[:, J], want_st[:, J], dm)
        assert (np.abs(got_st[:, J + 1] / want_st[:, J + 1] - 1) <= di + 1e-15).all(), (got_st[:, J + 1], want_st[:, J + 1], di)


@pytest.mark.parametrize("L", LENGTHS)
def test_exact_one_slot_with_unit_gain_is_the_segment(L):
    p = Pool(L, seed=100 + L)
    for i in range(4):
        p.add("f32", off=i, start=2 * i + 1, tail=0)
    rec = p.recipe([[(i, 1.0)] for i in range(4)])
    got_m, got_s, _ = run(p, rec, 1)
    want = np.stack([p.host[i][p.start[i]:p.start[i] + L] for i in range(4)])
    assert same_bits(got_m, want) and same_bits(got_s[:, 0], want)


def test_exact_every_phase_of_slot_0_against_another_phase_in_slot_1():
    L = 33 + 2 * 256 * 4  # head, more than one round of 16-byte stores per thread, tail
    p = Pool(L, seed=7)
    rows = []
    for ph in range(4):
        a, b = p.add("f32", off=ph, start=4), p.add("f32", off=(ph + 1) % 4, start=8 + (ph % 2))
        rows.append([(a, 1.0), (b, 0.5)])
    for ph in range(8):
        a, b = p.add("i16", off=ph, start=8), p.add("i16" if ph % 2 else "f32", off=(ph + 3) % 8, start=16)
        rows.append([(a, 1.0), (b, -0.25)])
    rec = p.recipe(rows)
    for t in p.dev:
        assert t.data_ptr() % (4 if t.dtype == torch.float32 else 2) == 0
    assert len({(t.data_ptr() // 4) % 4 for t in p.dev[:8:2]}) == 4 and len({(t.data_ptr() // 2) % 8 for t in p.dev[8::2]}) == 8
    want_m, want_s, _ = MO.mix(p.host, rec, L, 2)
    got_m, got_s, _ = run(p, rec, 2)
    assert same_bits(got_m, want_m) and same_bits(got_s, want_s)


@pytest.mark.parametrize("B", [1, 3])
def test_exact_every_n_out_and_slot_count(B):
    L = 37  # odd: the rows of mixture and sources start at every phase of the 16-byte grid
    p = exact_pool(L, seed=B)
    for Jr in (1, 2, 3, 4):
        rows = [[((3 * b + j) % 10, FACTORS[j]) for j in range(Jr)] for b in range(B)]
        rec = p.recipe(rows)
        for n_out in range(J + 1):
            want_m, want_s, _ = MO.mix(p.host, rec, L, n_out)
            got_m, got_s, _ = run(p, rec, n_out)
            assert same_bits(got_m, want_m) and same_bits(got_s, want_s), (B, Jr, n_out)
    m, s = D().mix_batch(p.dev, D().MixRecipe(*p.recipe([[(0, 1.0), (1, 1.0), (2, 1.0)]] * B)), L)  # n_out defaults to the recipe's J
    assert tuple(s.shape) == (B, 3, L)


# ---------------------------------------------------------------- 2. / 3. energy rule, normalisation
def snr_case(L, seed, scale=(1.0, 1.0, 1.0), dc=(0.0, 0.0, 0.0)):
    """Three rows: J = 2 at -5 dB; J = 3 at 0 dB whose first interferer is row 0's target; J = 4 at +5 dB with the same segment in two
    slots.  float32 and int16 sources.  scale / dc: per row."""
    p = Pool(L, seed)
    t0 = p.add("f32", off=1, start=3, scale=scale[0], dc=dc[0])
    i0 = p.add("i16", off=3, start=2, scale=scale[0], dc=dc[0])
    t1 = p.add("f32", off=2, start=0, tail=4, scale=scale[1], dc=dc[1])
    i1 = p.add("f32", off=3, start=5, scale=3.0 * scale[1], dc=dc[1])
    t2 = p.add("i16", off=5, start=1, scale=scale[2], dc=dc[2])
    i2 = p.add("f32", off=0, start=6, scale=0.1 * scale[2], dc=dc[2])
    i3 = p.add("f32", off=2, start=2, tail=1, scale=scale[2], dc=dc[2])
    D_ = D()
    r = D_.MixRecipe.snr([t0, t1, t2], [[i0, -1, -1], [t0, i1, -1], [i2, i3, i2]], [[p.start[t0], p.start[i0], 0, 0],
                                                                                    [p.start[t1], p.start[t0], p.start[i1], 0],
                                                                                    [p.start[t2], p.start[i2], p.start[i3], p.start[i2]]],
                         [-5.0, 0.0, 5.0])
    return p, (r.src, r.start, r.a, r.ref_src, r.ref_start)


def check_energy_case(p, rec, normalize, what):
    L = p.L
    if normalize:  # on the CPU, before the device is asked: no mixture that cancels
        assert L < 31 or MO.max_abs_corr(p.host, rec, L) <= MAX_CORR, what
        assert L == 1 or MO.moment_bounds(p.host, rec, L)[2].max() <= MAX_KAPPA, what
    want_m, want_s, want_st = MO.mix(p.host, rec, L, J, normalize=normalize)
    got_m, got_s, got_st = run(p, rec, J, normalize=normalize)
    used = rec[0] >= 0
    g, w = got_st[:, :rec[0].shape[1]][used], want_st[:, :rec[0].shape[1]][used]
    gain_err = float(np.abs(g / w - 1).max())
    print(f"[mix] {what}: gains max-rel {gain_err:.2e} (bound {(L + 16) * 2.0 ** -53:.2e})")
    assert gain_err <= (L + 16) * 2.0 ** -53, f"{what}: (a) gains {gain_err:.3e}"
    assert (got_st[:, :J][np.pad(~used, ((0, 0), (0, J - used.shape[1])), constant_values=True)] == 0).all()
    exp_m, exp_s = MO.mix_given_stats(p.host, rec, L, J, got_st, normalize=normalize)
    assert same_bits(got_m, exp_m), f"{what}: (b) mixture"
    assert same_bits(got_s, exp_s), f"{what}: (b) sources"
    if normalize and L == 1:
        assert np.isnan(got_m).all() and np.isnan(want_m).all() and np.isnan(got_s).all()  # as torch.std
        return
    wm = check_rows(got_m, want_m, f"{what}: (c) mixture")
    ws = check_rows(got_s, want_s, f"{what}: (c) sources")
    print(f"[mix] {what}: mixture max-rel {wm[0]:.2e} l2 {wm[1]:.2e}; sources max-rel {ws[0]:.2e} l2 {ws[1]:.2e}")


@pytest.mark.parametrize("L", LENGTHS)
def test_energy_rule_snr_recipes(L):
    p, rec = snr_case(L, seed=200 + L)
    check_energy_case(p, rec, False, f"snr L {L}")


@pytest.mark.parametrize("L", LENGTHS)
def test_norm_snr_recipes(L):
    p, rec = snr_case(L, seed=300 + L)
    check_energy_case(p, rec, True, f"norm L {L}")


@pytest.mark.parametrize("L", [33, CHUNK + 1, 32000])
def test_norm_dc_offset_and_amplitudes(L):
    """Row 0: a DC offset of 100 x the amplitude in every source (the case raw moments lose digits on); rows 1, 2: amplitudes 1e-4, 1e3."""
    p, rec = snr_case(L, seed=400 + L, scale=(0.01, 1e-4, 1e3), dc=(1.0, 0.0, 0.0))
    for normalize in (False, True):
        check_energy_case(p, rec, normalize, f"dc/amplitude L {L} normalize {normalize}")


def test_norm_equals_normalize_mixture_of_the_plain_call():
    L = 2 * CHUNK + 3
    p, rec = snr_case(L, seed=500)
    r = D().MixRecipe(*rec)
    m0, s0 = D().mix_batch(p.dev, r, L, n_out=3)
    wm, ws = D().normalize_mixture(m0, s0)
    m1, s1 = D().mix_batch(p.dev, r, L, n_out=3, normalize=True)
    check_rows(host(m1), host(wm), "mixture vs normalize_mixture")
    check_rows(host(s1)[:, :2], host(ws)[:, :2], "sources vs normalize_mixture")


# ---------------------------------------------------------------- 4. silence
@pytest.mark.parametrize("normalize", [False, True])
def test_silent_segments_give_the_oracles_inf_nan_pattern(normalize):
    L = 100
    p = Pool(L, seed=9)
    t, quiet, other, quiet2 = p.add("f32", off=1), p.add("f32", off=2, silent=True), p.add("i16", off=1), p.add("i16", silent=True)
    rows = [[(t, 1.0), (quiet, 0.5)],        # a silent interferer scaled to a reference: sqrt(E / 0) = inf, inf * 0 = NaN
            [(quiet, 1.0), (other, 0.5)],    # a silent reference: gain 0
            [(quiet, 1.0), (quiet2, 1.0)],   # both silent: 0 / 0
            [(t, 1.0), (other, 2.0)]]        # an ordinary row next to them
    refs = [[None, t], [None, quiet], [None, quiet], [None, t]]
    rec = p.recipe(rows, refs)
    want_m, want_s, want_st = MO.mix(p.host, rec, L, 2, normalize=normalize)
    got_m, got_s, got_st = run(p, rec, 2, normalize=normalize)
    assert np.isinf(want_st[0, 1]) and want_st[1, 1] == 0 and np.isnan(want_st[2, 1]) and np.isfinite(want_st[3]).all()
    assert np.array_equal(np.isnan(got_st[:, :J]), np.isnan(want_st[:, :J])) and np.array_equal(np.isinf(got_st[:, :J]), np.isinf(want_st[:, :J]))
    for got, want in ((got_m, want_m), (got_s, want_s)):
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    assert np.isnan(got_m[0]).all() and np.isnan(got_m[2]).all() and np.isfinite(got_m[3]).all()
    exp_m, exp_s = MO.mix_given_stats(p.host, rec, L, 2, got_st, normalize=normalize)
    assert same_bits(got_m, exp_m) and same_bits(got_s, exp_s)
    if not normalize:
        assert same_bits(got_m[1], want_m[1]) and same_bits(got_s[0, 0], want_s[0, 0])


# ---------------------------------------------------------------- 5. collate
def collate_case(B, n_src, L, seed):
    rng = np.random.RandomState(seed)
    return (rng.randn(B, n_src, L) * rng.uniform(0.05, 5.0, (B, n_src, 1))).astype(np.float32)


@pytest.mark.parametrize("L", [33, 32000])
@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("n_src", [1, 2, 4])
def test_collate_against_the_oracle(n_src, B, L):
    import rtfs_net_amd as R
    t = collate_case(B, n_src, L, seed=B + 10 * n_src + L)
    rng = random.Random(B * n_src + L)
    perms = [rng.sample(range(B), B) for _ in range(n_src)]
    want_in, want_t = MO.collate(t, perms)
    dt = torch.from_numpy(t).cuda()
    marker = object()
    got_in, got_t = R.System.online_mixing_collate((marker, dt), perms=perms)
    assert tuple(got_in.shape) == (B, L) and tuple(got_t.shape) == (B, n_src, L)
    gi, gt = host(got_in), host(got_t)
    check_rows(gi, want_in, f"collate inputs n_src {n_src} B {B} L {L}")
    check_rows(gt, want_t, f"collate targets n_src {n_src} B {B} L {L}")
    e_old, e_new = (t.astype(np.float64) ** 2).sum(-1), (gt.astype(np.float64) ** 2).sum(-1)
    assert np.abs(e_new / e_old - 1).max() <= 1e-5  # every new source has the energy of the one it replaces
    assert np.array_equal(host(dt), t)              # the batch itself is not written


def test_collate_draws_the_references_permutations():
    import rtfs_net_amd as R
    B, n_src, L = 5, 3, 64
    t = collate_case(B, n_src, L, seed=1)
    dt = torch.from_numpy(t).cuda()
    g = torch.Generator().manual_seed(77)
    perms = [torch.randperm(B, generator=g).tolist() for _ in range(n_src)]
    want = R.System.online_mixing_collate((None, dt), perms=perms)
    got = R.System.online_mixing_collate((None, dt), generator=torch.Generator().manual_seed(77))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    torch.manual_seed(78)  # without a generator: the global CPU generator, the reference's torch.randperm(batch)
    perms = [torch.randperm(B).tolist() for _ in range(n_src)]
    want = R.System.online_mixing_collate((None, dt), perms=perms)
    torch.manual_seed(78)
    got = R.System.online_mixing_collate((None, dt))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    check_rows(host(got[1]), MO.collate(t, perms)[1], "collate under manual_seed")
    for bad in (dt.cpu(), dt.double(), dt[0]):
        with pytest.raises(ValueError):
            R.System.online_mixing_collate((None, bad))
    with pytest.raises(ValueError):
        R.System.online_mixing_collate((None, dt), perms=[[0, 0, 1, 2, 3]] * n_src)


class Echo(torch.nn.Module):
    """An audio model that returns its input as (B, 1, L)."""

    def forward(self, wav):
        return wav.unsqueeze(1)


def test_common_step_applies_the_collate_when_the_config_says_so():
    import rtfs_net_amd as R
    B, L = 4, 640
    t = collate_case(B, 1, L, seed=3)
    inputs, targets = torch.from_numpy(t.sum(1)).cuda(), torch.from_numpy(t).cuda()
    loss = R.losses.PITLossWrapper(R.losses.PairwiseNegSDR("snr"), pit_from="pw_mtx")
    batch = (inputs, targets, None)
    plain = R.System(audio_model=Echo(), loss_func={"train": loss, "val": loss})
    mixing = R.System(audio_model=Echo(), loss_func={"train": loss, "val": loss}, config={"training": {"online_mix": True}})
    off = R.System(audio_model=Echo(), loss_func={"train": loss, "val": loss}, config={"training": {"online_mix": False}})
    by_hand = float(loss(inputs.unsqueeze(1), targets))
    for system in (plain, off):  # without the key, or with it false, every path is unchanged
        assert abs(float(system.common_step(batch, 0)) - by_hand) <= 1e-6 * max(1.0, abs(by_hand))
    torch.manual_seed(11)
    got = float(mixing.common_step(batch, 0))
    torch.manual_seed(11)
    new_in, new_t = R.System.online_mixing_collate((inputs, targets))
    want = float(loss(new_in.unsqueeze(1), new_t))
    assert np.isfinite(got) and abs(got - want) <= 1e-6 * max(1.0, abs(want)), (got, want)
    torch.manual_seed(11)
    perm = torch.randperm(B).tolist()
    assert perm != list(range(B))  # the comparison is not vacuous: this seed moves rows
    ref_in, ref_t = MO.collate(t, [perm])
    check_rows(host(new_in), ref_in, "common_step collate")


# ---------------------------------------------------------------- 6. System.mix_batch
_CACHE = {}


def small_system():
    import rtfs_net_amd as R
    from oracle import video_oracle as V
    from rtfs_net_amd.configs import RTFS4_AUDIONET
    if "system" not in _CACHE:
        conf = copy.deepcopy(RTFS4_AUDIONET)
        conf["audio_params"]["repeats"] = 2
        torch.manual_seed(0)
        m = R.AVNet(print_macs=False, **conf).cuda().train()
        v = R.FRCNNVideoModel(print_macs=False)
        v.load_state_dict({k: torch.from_numpy(np.asarray(w)) for k, w in V.make_video_state_dict(0).items()})
        loss = R.losses.PITLossWrapper(R.losses.PairwiseNegSDR("snr"), pit_from="pw_mtx")
        opt = R.make_optimizer([q for q in m.parameters() if q.requires_grad], optimizer="adamw", lr=1e-3, weight_decay=0.1)
        _CACHE["system"] = R.System(audio_model=m, video_model=v.cuda().eval(), optimizer=opt, loss_func={"train": loss, "val": loss},
                                    config={"training": {"batch_size": 2}})
    return _CACHE["system"]


def utterance_pool(length, seed):
    rng = np.random.RandomState(seed)
    lengths = [length, length + 640 * 3, length + 1999, length - 1, length + 640 * 7 + 5]
    wavs = [(0.05 * rng.randn(n)).astype(np.float32) for n in lengths]
    wavs[2] = np.clip(np.rint(wavs[2] * 32768 * 4), -32000, 32000).astype(np.int16)  # one utterance as PCM
    rois = [rng.randint(0, 256, (max(n // 640, 1), 96, 100)).astype(np.uint8) for n in lengths]
    return lengths, wavs, rois


def test_system_mix_batch_shapes_keys_lips_and_audio():
    s, length, B = small_system(), 4096, 2
    lengths, wavs, rois = utterance_pool(length, seed=21)
    dw, dr = [torch.from_numpy(w).cuda() for w in wavs], [torch.from_numpy(r).cuda() for r in rois]
    for train in (True, False):
        got = s.mix_batch(dw, dr, length=length, n_src=3, snr_db=(-3.0, 3.0), normalize_audio=True, train=train, rng=random.Random(5))
        rng = random.Random(5)
        rec = D().draw_mix_recipe(lengths, B, length, n_src=3, snr_db=(-3.0, 3.0), align=640, rng=rng)
        inputs, targets, lips, keys = got
        Tv = length // 640
        assert tuple(inputs.shape) == (B, length) and tuple(targets.shape) == (B, length) and tuple(lips.shape) == (B, 1, Tv, 88, 88)
        assert keys == rec.src[:, 0].tolist() and 3 not in rec.src  # the short utterance is never drawn
        slices = np.stack([rois[k][st // 640:st // 640 + Tv] for k, st in zip(keys, rec.start[:, 0].tolist())])
        table = [PO.draw_offsets(96, 100, rng=rng) for _ in range(B)] if train else [PO.center_offsets(96, 100) + (0,)] * B
        want_lips = PO.lips_prepare(slices, table)
        assert same_bits(host(lips), want_lips), f"train {train}"
        wm, ws = D().mix_batch(dw, rec, length, n_out=1, normalize=True)
        assert torch.equal(inputs, wm) and torch.equal(targets, ws[:, 0])
        again = s.mix_batch(dw, dr, length=length, train=train, normalize_audio=True, recipe=rec, rng=random.Random(5))
        assert torch.equal(again[0], inputs) and again[3] == keys
    with pytest.raises(ValueError):  # a track too short for its slice
        s.mix_batch(dw, [r[:2] for r in dr], length=length, rng=random.Random(5))
    with pytest.raises(ValueError):
        s.mix_batch(dw, dr[:3], length=length)


def test_optimization_step_on_a_mixed_batch():
    s, length = small_system(), 4096
    lengths, wavs, rois = utterance_pool(length, seed=22)
    dw, dr = [torch.from_numpy(w).cuda() for w in wavs], [torch.from_numpy(r).cuda() for r in rois]
    batch = s.mix_batch(dw, dr, length=length, rng=random.Random(6))
    assert tuple(batch[0].shape) == (2, length)
    value = s.optimization_step(batch, 0)
    torch.cuda.synchronize()
    assert np.isfinite(float(value))


# ---------------------------------------------------------------- 7. refusals
def test_refusals_raise_before_any_launch():
    from rtfs_net_amd import _lib
    M = D()
    L = 50
    x, y = torch.zeros(100, device="cuda"), torch.zeros(100, dtype=torch.int16, device="cuda")
    before = _lib.load().rtfs_debug_launch_count()
    bad = [lambda: M.mix_batch([x], M.MixRecipe([[0]], [[51]], [[1.0]]), L),                            # a segment past its source
           lambda: M.mix_batch([x, y], M.MixRecipe([[0, 1]], [[0, 0]], [[1.0, 1.0]], [[-1, 0]], [[0, 51]]), L),  # a reference past its source
           lambda: M.mix_batch([x.cpu()], M.MixRecipe([[0]], [[0]], [[1.0]]), L),                      # CPU tensors
           lambda: M.mix_batch([x.double()], M.MixRecipe([[0]], [[0]], [[1.0]]), L),                   # a float64 source
           lambda: M.mix_batch([x], M.MixRecipe([[0]], [[0]], [[1.0]]), L, n_out=J + 1),               # n_out > J
           lambda: M.mix_batch([x], M.MixRecipe([[0] * 5], [[0] * 5], [[1.0] * 5]), L),                # five slots
           lambda: M.mix_batch([x], M.MixRecipe([[0], [-1]], [[0], [0]], [[1.0], [1.0]]), L),          # a row without a slot
           lambda: M.mix_batch([x], M.MixRecipe([[1]], [[0]], [[1.0]]), L),                            # a source that is not there
           lambda: M.mix_batch([x], M.MixRecipe([[0]], [[0]], [[1.0]]), 0),
           lambda: M.mix_batch([x.view(10, 10)], M.MixRecipe([[0]], [[0]], [[1.0]]), 5),
           lambda: M.mix_batch([x[::2]], M.MixRecipe([[0]], [[0]], [[1.0]]), 5)]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
    assert _lib.load().rtfs_debug_launch_count() == before
    m, s = M.mix_batch([x, y], M.MixRecipe([[0, 1]], [[50, 50]], [[1.0, 1.0]]), L)  # the last 50 samples of both: accepted, two launches
    assert _lib.load().rtfs_debug_launch_count() == before + 2 and float(m.abs().max()) == 0.0


# ---------------------------------------------------------------- 8. poisoned memory
FORWARD_CASES = "test_exact or test_energy or test_norm"
ABNORMAL = (124, 134, 137, 139)


@pytest.mark.skipif(POISONED, reason="already inside a poisoned run")
def test_poisoned():
    """Cases 1 - 3 in a fresh child process per pattern, with every workspace and output a C call fills poisoned (tests/test_hip_prep.py's
    discipline: a time limit per child, and no second child after one that did not exit cleanly)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for pattern in ("nan", "big"):
        env = dict(os.environ, RTFS_POISON_WS=pattern)
        try:
            pr = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_hip_mix.py"), "-m", "gpu", "-q", "-p",
                                 "no:cacheprovider", "-k", FORWARD_CASES], cwd=root, env=env, capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired:
            pytest.fail(f"RTFS_POISON_WS={pattern}: timed out after 300 s; no further child started")
        if pr.returncode < 0 or pr.returncode in ABNORMAL:
            pytest.fail(f"RTFS_POISON_WS={pattern}: abnormal exit status {pr.returncode}; no further child started\n{pr.stdout[-3000:]}")
        assert pr.returncode == 0, f"RTFS_POISON_WS={pattern}: exit status {pr.returncode}\n{pr.stdout[-3000:]}\n{pr.stderr[-2000:]}"
