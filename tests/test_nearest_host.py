"""CPU: the nearest up-sampling index rule.  The reference calls F.interpolate(mode="nearest") on float32 tensors, and stock torch then
reads source min(int(floorf(dst * (float(n_in) / float(n_out)))), n_in - 1) - quotient and product rounded to float32 - which is not
floor(dst * n_in / n_out).  oracle.rtfs_oracle.nearest_index is that closed form in numpy; the kernels' nearest_src (csrc/common.h) is
the same on the device (tests/test_hip_nearest.py).  Here: the closed form against stock torch, where the two rules differ, and which
shape families - every committed fixture among them - are untouched by the difference."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import rtfs_oracle as O
from oracle.rtfs_oracle import nearest_index, nearest_index_integer
from tests import nearest_cases as NC
from tests.util import rel_err, spec_R4


def torch_index_1d(n_in, n_out, dtype=torch.float32):
    ramp = torch.arange(n_in, dtype=dtype).view(1, 1, n_in)
    return F.interpolate(ramp, size=n_out, mode="nearest").view(-1).to(torch.int64).numpy()


def torch_index_2d_leading(n_in, n_out):
    """Index along H of a 2-D call that also up-samples W (2 -> 3)."""
    x = torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in, 1).expand(1, 1, n_in, 2)
    y = F.interpolate(x, size=(n_out, 3), mode="nearest")
    assert bool((y[0, 0, :, :1] == y[0, 0]).all())
    return y[0, 0, :, 0].to(torch.int64).numpy()


def test_departing_set_is_not_empty_and_holds_the_model_lengths():
    dep = set(NC.departing_pairs())
    assert len(dep) == 5987  # n_in <= 256, n_out <= 1030
    for pair in [(16, 82), (32, 164), (40, 205), (16, 122), (26, 44), (14, 46), (36, 284)]:
        assert pair in dep, pair
    assert min(n_out for _, n_out in dep) == 44 and (26, 44) in dep
    # the vectorised scan and the per-pair closed forms are the same statement
    for n_in, n_out in list(dep)[::97] + NC.stride_sample()[::31]:
        assert NC.departs(n_in, n_out) == ((n_in, n_out) in dep), (n_in, n_out)
    # where they differ, and by how much: the float32 product lands just below an integer the exact product reaches
    assert np.flatnonzero(nearest_index(16, 82) != nearest_index_integer(16, 82)).tolist() == [41]
    assert np.flatnonzero(nearest_index(32, 164) != nearest_index_integer(32, 164)).tolist() == [41, 82]
    assert np.flatnonzero(nearest_index(40, 205) != nearest_index_integer(40, 205)).tolist() == [41, 82, 164]
    assert np.flatnonzero(nearest_index(16, 122) != nearest_index_integer(16, 122)).tolist() == [61]
    assert nearest_index(16, 82)[41] == 7 and nearest_index_integer(16, 82)[41] == 8
    # the VP block at Tv = 122 (pyramid 122, 61, 31, 16): three output frames of its last level see another global frame through the
    # chain 16 -> 122 (frame 61) and the depthwise k = 3 taps around it
    assert NC.vp_lengths(122) == [122, 61, 31, 16] and (16, 122) in NC.vp_pairs(122)
    assert [p for p in NC.vp_pairs(284) if p in dep] == [(36, 284)]


def test_closed_form_is_stock_torch_float32():
    """nearest_index == F.interpolate(mode="nearest") on float32 CPU tensors, 1-D and on the leading axis of a 2-D call: every departing
    pair, the stride sample, and every pair the existing tests and goldens use."""
    pairs = list(NC.departing_pairs()) + NC.stride_sample() + NC.used_pairs()
    assert len(pairs) > 8000
    for n_in, n_out in pairs:
        want = nearest_index(n_in, n_out)
        assert want.shape == (n_out,) and want[0] == 0 and want[-1] <= n_in - 1
        assert np.array_equal(torch_index_1d(n_in, n_out), want), (n_in, n_out)
    for n_in, n_out in pairs[::3] + [(16, 82), (32, 164), (40, 205), (16, 122), (14, 46), (26, 44)]:
        assert np.array_equal(torch_index_2d_leading(n_in, n_out), nearest_index(n_in, n_out)), (n_in, n_out)


def test_float64_interpolate_takes_the_integer_rule():
    """Why oracle/grad_oracle.py gathers explicitly: on a float64 tensor torch computes the index in float64, which gives
    floor(dst * n_in / n_out) - not what the reference's float32 run reads."""
    got = torch_index_1d(32, 164, torch.float64)
    assert np.array_equal(got, nearest_index_integer(32, 164))
    assert not np.array_equal(got, nearest_index(32, 164))
    # ... and the float64 oracle's up-sampling follows the float32 indices for any dtype, forward and backward
    from oracle.grad_oracle import nearest_up_torch
    x = torch.arange(32, dtype=torch.float64).view(1, 1, 32).requires_grad_()
    y = nearest_up_torch(x, 164)
    assert np.array_equal(y.detach().view(-1).numpy().astype(np.int64), nearest_index(32, 164))
    y.sum().backward()
    assert np.array_equal(x.grad.view(-1).numpy().astype(np.int64), np.bincount(nearest_index(32, 164), minlength=32))
    x2 = torch.zeros(1, 1, 14, 26, dtype=torch.float64)
    assert tuple(nearest_up_torch(x2, (46, 44)).shape) == (1, 1, 46, 44)


def test_unaffected_families_agree_under_both_rules():
    """No existing fixture changes: the audio block's T // 2 -> T (T <= 2100), 64 -> 129, whole-window pairs (k, 5k + 1) - long-form and
    live windows of a multiple of 640 samples - and every (Tv, T) of the committed end-to-end / gradient goldens, with the VP pyramid
    pairs of their Tv."""
    fam = [(t // 2, t) for t in range(4, 2101)] + [(64, 129)] + [(k, 5 * k + 1) for k in range(1, 257)] + NC.E2E_TV_T + NC.GOLDEN_TV_T
    for tv, _ in NC.GOLDEN_TV_T:
        fam += NC.vp_pairs(tv)
    for n_in, n_out in fam + NC.SURVEY_PAIRS:
        assert np.array_equal(nearest_index(n_in, n_out), nearest_index_integer(n_in, n_out)), (n_in, n_out)
    # the golden files' lengths are what the list says: T = L // 128 + 1
    for L, tv in [(4096, 7), (5000, 8), (8000, 13), (32000, 50), (64000, 100), (85000, 133), (131072, 205)]:
        assert (tv, L // 128 + 1) in NC.E2E_TV_T


@pytest.mark.parametrize("B,T,Fq,Tv", [(1, 82, 3, 16), (1, 164, 3, 32)])
def test_float64_caf_oracle_follows_the_float32_indices(B, T, Fq, Tv):
    """grad_oracle.caf_torch (float64 torch ops) == rtfs_oracle.caf (numpy, float32 between layers) at departing (Tv, T).  The two differ
    by float32 rounding of a chain of ~6 operations (conv, gLN / BatchNorm fold, softmax, product, sum): bar 2e-6 of the tensor's scale;
    with F.interpolate on the float64 tensors the difference was of order 1."""
    from oracle import grad_oracle as G
    from oracle.params import make_state_dict
    cell = O._sub(make_state_dict(spec_R4(), 0), "refinement_module.crossmodal_fusion.fusion_module.audio_lstm")
    rs = np.random.RandomState(300 + T)
    a, v = rs.randn(B, 256, T, Fq).astype(np.float32), rs.randn(B, 512, Tv).astype(np.float32)
    ref = O.caf(a, v, cell)
    got = G.caf_torch(torch.tensor(a, dtype=torch.float64), torch.tensor(v, dtype=torch.float64),
                      {k: torch.tensor(x, dtype=torch.float64) for k, x in cell.items()}).numpy()
    e = rel_err(ref, got)
    worst_t = float((np.abs(ref - got).max((0, 1, 3)) / np.abs(got).max((0, 1, 3))).max())
    print(f"caf_torch (float64) vs rtfs_oracle.caf at (T, Tv) = ({T}, {Tv}): max-rel {e:.3e}, worst time frame {worst_t:.3e}")
    assert e <= 2e-6 and worst_t <= 2e-6, (e, worst_t)
