"""Loudness on the device (rtfs-net_amd/datas.py loudness / loudness_many / loudness_normalize, csrc/k_loudness.hip;
System.mix_batch(loudness=...)) against tests/loudness_oracle.py.  Every recording is a view at an odd element offset into a larger
buffer in which everything outside the whole hops [0, floor(L / H) H) - the allocation around the view and the recording's own tail
behind its last whole hop - is NaN (float32) or +-32767 (int16), so a read that the definition does not make shows.

The reference is ``truth`` (the plain recurrence in 80-bit), computed once per process for all cases; block energies z are held to
``BAR`` relative, lufs to ``LUFS_BAR`` absolute, kept exactly (tests/test_loudness_host.py asserts that no block of any case lies within
1e-6 of a gate, so a flip is an error and not a rounding).  Every figure is printed before it is asserted."""
import math
import random

import numpy as np
import pytest
import torch

from tests import loudness_oracle as LO

pytestmark = pytest.mark.gpu

ROUNDING = 10.0 / math.log(10.0) * 2.0 ** -23   # float32 rounding of scaled samples: 2^-23 relative on energy, in dB


def D():
    from rtfs_net_amd import datas
    return datas


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def same_bits(a, b):
    """Bit-equal, NaN in the same positions (a NaN's payload is not part of the definition)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def place(x, H, off, poison_tail=True):
    """The recording as the device gets it: a view at element offset ``off`` of its own buffer, poison outside the whole hops."""
    L = len(x)
    keep = (L // H) * H if poison_tail else L
    n = off + L + 3
    if x.dtype == np.float32:
        buf = np.full(n, np.nan, np.float32)
    else:
        buf = np.where(np.arange(n) % 2 == 0, 32767, -32767).astype(np.int16)
    buf[off:off + keep] = x[:keep]
    return torch.from_numpy(buf).cuda()[off:off + L]


_POOLS = {}


def pool(fs):
    """(names, device views, host arrays) of the cases at one rate; built once."""
    if fs not in _POOLS:
        named = [(n, x) for n, f, x in LO.gpu_cases() if f == fs]
        _POOLS[fs] = ([n for n, _ in named], [place(x, fs // 10, 2 * i + 1) for i, (_, x) in enumerate(named)], [x for _, x in named])
    return _POOLS[fs]


def measured(fs):
    names, dev, _ = pool(fs)
    lufs, kept, z = D().loudness_many(dev, fs, return_kept=True, return_blocks=True)
    return names, host(lufs), host(kept), [host(v) for v in z]


# ---------------------------------------------------------------- against the 80-bit run
@pytest.mark.parametrize("fs", LO.rates())
def test_pool_against_truth(fs):
    assert fs in (8000, 16000, 44100, 48000)
    names, lufs, kept, z = measured(fs)
    tr = LO.truth_of_cases()
    assert lufs.dtype == np.float64 and kept.dtype == np.int64
    worst, worst_db, failed = 0.0, 0.0, []
    for i, n in enumerate(names):
        zt = tr[n][1]
        want_lufs, want_kept = LO.gate(zt)
        dev = LO.rel_dev(z[i], zt) if z[i].shape == zt.shape else float("inf")
        ddb = 0.0 if lufs[i] == want_lufs else abs(lufs[i] - want_lufs)
        print(f"fs {fs} {n}: blocks {len(zt)} z dev {dev:.3g} lufs {lufs[i]:.12f} want {want_lufs:.12f} diff {ddb:.3g} kept {kept[i]} want {want_kept}")
        worst, worst_db = max(worst, dev), max(worst_db, ddb)
        if not (dev <= LO.BAR and ddb <= LO.LUFS_BAR and kept[i] == want_kept):
            failed.append(n)
    print(f"fs {fs}: worst z dev {worst:.3g} (bar {LO.BAR:.3g}), worst lufs diff {worst_db:.3g} (bar {LO.LUFS_BAR:.3g})")
    assert not failed, failed


def test_both_gates_are_at_work_on_the_device():
    names, lufs, kept, z = measured(16000)
    i, j, k = names.index("zeros"), names.index("quiet40"), names.index("under70")
    assert z[i][12] < LO.ABS_GATE and 0 < kept[i] < len(z[i])
    assert (z[j] > LO.ABS_GATE).all() and 0 < kept[j] < len(z[j])
    assert lufs[k] == float("-inf") and kept[k] == 0 and (z[k] > 0).all()


def test_known_answers_and_non_finite_samples():
    fs = 48000
    sine = np.sin(2 * np.pi * 997.0 * np.arange(fs) / fs).astype(np.float32)
    silent = np.zeros(4 * 4800 + 17, np.float32)
    rng = np.random.RandomState(4)
    nan = (0.1 * rng.randn(6 * 4800)).astype(np.float32)
    nan[2 * 4800 + 11] = np.nan
    inf = nan.copy()
    inf[2 * 4800 + 11] = np.inf
    last = (0.1 * rng.randn(4 * 4800 + 9)).astype(np.float32)
    last[4 * 4800 - 1] = np.nan                          # the last sample of the last whole hop
    fine = last.copy()
    fine[4 * 4800 - 1] = 0.0
    fine[4 * 4800] = np.nan                              # the first sample behind it is not read
    dev = [place(x, 4800, 2 * i + 1, poison_tail=False) for i, x in enumerate((sine, silent, nan, inf, last, fine))]
    lufs, kept, z = D().loudness_many(dev, fs, return_kept=True, return_blocks=True)
    lufs, kept = host(lufs), host(kept)
    print("sine", lufs[0], "silent", lufs[1], kept[1], "nan", lufs[2:5], "fine", lufs[5])
    assert abs(lufs[0] - (-3.01)) <= 0.01 and kept[0] == 7
    assert lufs[1] == float("-inf") and kept[1] == 0 and (host(z[1]) == 0).all()
    assert np.isnan(lufs[2:5]).all() and (kept[2:5] == 0).all()
    assert np.isfinite(lufs[5]) and kept[5] == 1


# ---------------------------------------------------------------- determinism
def test_a_recording_alone_and_in_a_pool_and_twice_gives_the_same_bits():
    fs = 8000
    names, dev, _ = pool(fs)
    _, lufs, kept, z = measured(fs)
    _, lufs2, kept2, z2 = measured(fs)
    assert same_bits(lufs, lufs2) and np.array_equal(kept, kept2) and all(same_bits(a, b) for a, b in zip(z, z2))
    assert len(names) >= 8
    for n in ("hops257", "hops64", "len3201"):           # float32 and int16, the longest
        i = names.index(n)
        a, k, zz = D().loudness_many([dev[i]], fs, return_kept=True, return_blocks=True)
        assert same_bits(host(a), lufs[i:i + 1]) and host(k)[0] == kept[i] and same_bits(host(zz[0]), z[i]), n
    # the same samples at another alignment, and the tensor entry
    _, _, xs = pool(16000)
    x = xs[0]
    a = host(D().loudness(torch.from_numpy(x).cuda(), 16000))
    b = host(D().loudness(torch.from_numpy(np.concatenate([np.zeros(2, np.float32), x])).cuda()[2:], 16000))
    rows = torch.from_numpy(np.stack([x, 0.5 * x, x])).cuda()
    c = host(D().loudness(rows, 16000))
    assert a.shape == (1,) and c.shape == (3,) and same_bits(a, b) and same_bits(c[[0, 2]], np.repeat(a, 2))
    assert abs((c[0] - c[1]) - 20 * math.log10(2.0)) <= 2 * LO.LUFS_BAR


def test_poisoned_outputs_stats_and_workspace(monkeypatch):
    """Everything a loudness call allocates goes through _lib.empty / _lib.workspace: with the poison fill on, the same bits come back
    and the guard band behind the workspace is intact (_lib.check raises otherwise)."""
    from rtfs_net_amd import _lib
    fs = 16000
    names, dev, xs = pool(fs)
    _, lufs, kept, z = measured(fs)
    rows = [torch.from_numpy(x).cuda() for x in xs[:6]]
    out, (l0, g0) = D().loudness_normalize(rows, fs, return_stats=True)
    out, g0 = [host(o) for o in out], host(g0)
    for byte in (0xFF, 0x7F):
        monkeypatch.setattr(_lib, "_POISON", byte)
        _, lufs2, kept2, z2 = measured(fs)
        assert same_bits(lufs, lufs2) and np.array_equal(kept, kept2) and all(same_bits(a, b) for a, b in zip(z, z2)), hex(byte)
        out2, (_, g2) = D().loudness_normalize(rows, fs, return_stats=True)
        assert same_bits(g0, host(g2)) and all(same_bits(a, host(b)) for a, b in zip(out, out2)), hex(byte)
        monkeypatch.setattr(_lib, "_POISON", None)


# ---------------------------------------------------------------- loudness_normalize
def test_normalize_scales_by_the_devices_own_gain():
    fs, H, target = 16000, 1600, -23.0
    rng = np.random.RandomState(12)
    xs = [(0.03 * rng.randn(7 * H + 5)).astype(np.float32), LO._pcm(0.2 * rng.randn(4 * H)), np.zeros(5 * H + 1, np.float32),
          (0.5 * rng.randn(9 * H + 1599)).astype(np.float32), LO._pcm(0.01 * rng.randn(6 * H + 3) + 0.1)]
    dev = [place(x, H, 2 * i + 1, poison_tail=False) for i, x in enumerate(xs)]
    out, (lufs, g) = D().loudness_normalize(dev, fs, target=target, return_stats=True)
    lufs, g = host(lufs), host(g)
    assert same_bits(lufs, host(D().loudness_many(dev, fs)))
    assert lufs[2] == float("-inf") and g[2] == 1.0 and same_bits(host(out[2]), xs[2])      # a silent row is copied
    for i, x in enumerate(xs):
        assert out[i].dtype == torch.float32 and tuple(out[i].shape) == x.shape
        assert same_bits(host(out[i]), (LO.samples(x) * g[i]).astype(np.float32)), i        # (float)(x g) with the device's own g
        if i == 2:
            continue
        want = 10.0 ** ((target - lufs[i]) / 20.0)
        rel = abs(g[i] - want) / want
        print(f"row {i}: lufs {lufs[i]:.9f} g {g[i]:.17g} numpy {want:.17g} rel {rel:.3g}")
        assert rel <= 2.0 ** -47
    again = host(D().loudness_many(out, fs))
    print("re-measured", again, "tolerance", LO.LUFS_BAR + ROUNDING)
    for i in (0, 1, 3, 4):
        assert abs(again[i] - target) <= LO.LUFS_BAR + ROUNDING, (i, again[i])
    # the tensor entries: (L) and (B, L), another target
    rows = torch.from_numpy(np.stack([xs[0], 0.25 * xs[0]])).cuda()
    o2 = D().loudness_normalize(rows, fs, target=-30.0)
    o1 = D().loudness_normalize(rows[0], fs, target=-30.0)
    assert tuple(o2.shape) == tuple(rows.shape) and tuple(o1.shape) == tuple(rows[0].shape) and torch.equal(o2[0], o1)
    both = host(D().loudness(o2, fs))
    assert (np.abs(both + 30.0) <= LO.LUFS_BAR + ROUNDING).all(), both
    # a non-finite loudness: copied with g = 1, NaN and all
    bad = xs[0].copy()
    bad[100] = np.nan
    ob, (lb, gb) = D().loudness_normalize(torch.from_numpy(bad).cuda(), fs, return_stats=True)
    assert np.isnan(host(lb)[0]) and host(gb)[0] == 1.0 and same_bits(host(ob), bad)


# ---------------------------------------------------------------- System.mix_batch(loudness=...)
class Echo(torch.nn.Module):
    def forward(self, wav):
        return wav.unsqueeze(1)


def parents_recipe(lengths, batch, length, n_src, snr_db, rng):
    """System.mix_batch's draw before it knew loudness, restated (align 640)."""
    pool_ = [i for i, n in enumerate(lengths) if n >= length]
    rows, starts, dbs = [], [], []
    for _ in range(batch):
        row = rng.sample(pool_, n_src)
        rows.append(row)
        starts.append([640 * rng.randint(0, (lengths[i] - length) // 640) for i in row])
        dbs.append([rng.uniform(snr_db[0], snr_db[1]) for _ in row[1:]])
    return D().MixRecipe.snr([r[0] for r in rows], [r[1:] for r in rows], starts, dbs)


def test_system_mix_batch_levels_by_loudness():
    import rtfs_net_amd as R
    fs, length, B = 16000, 7040, 3
    rng = np.random.RandomState(31)
    lengths = [length + 640 * 5, length + 1999, length, length + 640 * 9 + 5, length - 1]
    sig = [0.05, 0.2, 0.01, 0.1, 0.05]
    wavs = [(s * rng.randn(n) * (1.0 + 0.8 * np.sin(np.arange(n) / 900.0))).astype(np.float32) for s, n in zip(sig, lengths)]
    wavs[1] = LO._pcm(wavs[1])
    rois = [rng.randint(0, 256, (max(n // 640, 1), 96, 100)).astype(np.uint8) for n in lengths]
    dw, dr = [torch.from_numpy(w).cuda() for w in wavs], [torch.from_numpy(r).cuda() for r in rois]
    loss = R.losses.PITLossWrapper(R.losses.PairwiseNegSDR("snr"), pit_from="pw_mtx")
    s = R.System(audio_model=Echo(), loss_func={"train": loss, "val": loss}, config={"training": {"batch_size": B}})
    utter = host(D().loudness_many(dw, fs)).tolist()     # the one readback, once per dataset
    assert np.isfinite(utter).all()
    for z in LO.truth(wavs, fs)[1]:
        LO.assert_gate_margin(z)                         # scaling and float32 rounding cannot move a block across a gate
    inputs, targets, lips, keys = s.mix_batch(dw, dr, length=length, n_src=2, rng=random.Random(5), loudness=(-33.0, -25.0), utter_lufs=utter)
    rec = D().draw_mix_recipe(lengths, B, length, n_src=2, align=640, rng=random.Random(5), loudness=(-33.0, -25.0), utter_lufs=utter)
    assert keys == rec.src[:, 0].tolist() and (rec.ref_src == -1).all() and tuple(lips.shape) == (B, 1, length // 640, 88, 88)
    wm, ws = D().mix_batch(dw, rec, length, n_out=2, return_stats=False)
    assert torch.equal(inputs, wm) and torch.equal(targets, ws[:, 0])
    seen = 0
    for b in range(B):
        for j in range(2):
            k, a, st = int(rec.src[b, j]), float(rec.a[b, j]), int(rec.start[b, j])
            drawn = utter[k] + 20.0 * math.log10(a)
            assert -33.0 - 1e-9 <= drawn <= -25.0 + 1e-9
            assert same_bits(host(ws[b, j]), (LO.samples(wavs[k])[st:st + length] * a).astype(np.float32))  # the slot is the crop times a
            whole = torch.from_numpy((LO.samples(wavs[k]) * a).astype(np.float32)).cuda()
            got = float(host(D().loudness(whole, fs))[0])
            print(f"row {b} slot {j}: utterance {k} at {utter[k]:.6f} LUFS, a {a:.6g}, drawn {drawn:.9f}, re-measured {got:.9f}")
            assert abs(got - drawn) <= 2 * LO.LUFS_BAR + ROUNDING
            seen += 1
    assert seen == 2 * B
    # without the arguments: the draws and the bits of the call as it was
    got = s.mix_batch(dw, dr, length=length, n_src=3, snr_db=(-3.0, 3.0), rng=random.Random(6))
    old = parents_recipe(lengths, B, length, 3, (-3.0, 3.0), random.Random(6))
    wm, ws = D().mix_batch(dw, old, length, n_out=1)
    assert got[3] == old.src[:, 0].tolist() and torch.equal(got[0], wm) and torch.equal(got[1], ws[:, 0])
    with pytest.raises(ValueError):
        s.mix_batch(dw, dr, length=length, loudness=(-30.0, -20.0))
    with pytest.raises(ValueError, match="source 2"):
        D().MixRecipe.lufs([[2]], [[0]], -23.0, [0.0, 0.0, float("-inf")])


# ---------------------------------------------------------------- refusals and launches
def test_refusals_raise_before_any_launch_and_a_call_is_four_launches():
    from rtfs_net_amd import _lib
    M = D()
    x, y = torch.zeros(8000, device="cuda"), torch.zeros(8000, dtype=torch.int16, device="cuda")
    before = _lib.load().rtfs_debug_launch_count()
    bad = [lambda: M.loudness_many([x[:6399]], 16000),            # L = 4 H - 1
           lambda: M.loudness_many([x, y[:100]], 16000),
           lambda: M.loudness_many([x], 11025),
           lambda: M.loudness_many([x], 7990),
           lambda: M.loudness_many([x], 192010),
           lambda: M.loudness_many([x.cpu()], 16000),
           lambda: M.loudness_many([x.double()], 16000),
           lambda: M.loudness_many([x[::2]], 16000),
           lambda: M.loudness_many([], 16000),
           lambda: M.loudness(x.view(2, 2, 2000), 8000),
           lambda: M.loudness_normalize([x[:100]], 16000)]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    assert _lib.load().rtfs_debug_launch_count() == before
    M.loudness_many([x, y, x[1:6401]], 16000)
    assert _lib.load().rtfs_debug_launch_count() == before + 4
    M.loudness_normalize([x, y], 16000)
    assert _lib.load().rtfs_debug_launch_count() == before + 9
