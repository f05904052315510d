"""tests/_stereo_ref64.py must be trusted before it judges a kernel: the float64 restatement of the DepthNet cost volume against the
reference model's own stored output, against the float32 oracle in log space on every case of tests/test_gpu_stereo_ref64.py
(which yields the float32 floor each GPU bound is built from), on two poses with a known answer, and every input condition a GPU
case relies on -- which kernel branch its geometry reaches, that no probability underflows -- proven on the reference alone.
No GPU."""
import numpy as np
import pytest
import torch

import _stereo_ref64 as R
from oracle import oracle as O
from preworld_amd import synth as S


def _probs(ref):
    return ref.log_softmax.exp().numpy()


@pytest.mark.parametrize('bias', [0.0, 5.0])
def test_reference_model_fixture(golden, bias):
    """tests/golden/stereo_small.npz is DepthNet.calculate_cost_volumn's own float32 output.  A float32 softmax of costs of about 8
    with 8 channels x 4 corners of rounded products carries a relative error of some 1e-5 (measured: 1.8e-5 relative, 2e-6
    absolute); bounded at 1e-4 relative + 2^-18 absolute, the fixture's float32 rounding with the headroom of the 32 summed terms."""
    g = golden('stereo_small.npz')
    prev, curr, k2s, K, pr, pt, fr = S.stereo_inputs(int(g['seed']))
    ref = R.stereo_ref64(prev, curr, fr, k2s, K, pr, pt, bias=bias)
    want = g['cv_bias%d' % int(bias)].astype(np.float64)
    got = _probs(ref)
    err = np.abs(got - want)
    print('[parity] stereo ref64 vs reference fixture bias %g: max abs %.2e, max rel %.2e' % (
        bias, err.max(), (err / np.maximum(want, 1e-30))[want > 1e-4].max()))
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=2.0 ** -18)
    np.testing.assert_allclose(got.sum(1), 1.0, rtol=1e-12)


@pytest.mark.parametrize('name', [n for n in R.CASES if R.CASES[n]['kind'] != 'uniform'])
def test_oracle_floor(name):
    """The float32 oracle against the float64 reference in log space, outside the fragile mask: the case's float32 floor.
    FLOORS holds the measurement rounded up; the oracle must stay under it (and not far under: a table entry ten times the
    measurement would be a bound nobody measured)."""
    prev, curr, k2s, K, pr, pt, fr = R.case_inputs(name)
    worst = 0.0
    for bias in R.CASES[name]['biases']:
        out = O.stereo_cost_volume(prev, curr, fr, k2s, K, pr, pt, bias=bias)
        worst = max(worst, R.log_error(name, out, bias, report='oracle32'))
    assert worst <= R.FLOORS[name], (name, worst, R.FLOORS[name])
    assert worst >= 0.5 * R.FLOORS[name], (name, 'the table entry is not this measurement', worst, R.FLOORS[name])


@pytest.mark.parametrize('name', ['identity', 'sideways'])
def test_analytic_uniform(name):
    """identity pose: every bin of a pixel samples the same place -> equal costs -> exactly 1/D; 500 m sideways: every point is out
    of view -> the cost is sum |curr| (+ bias) in every bin -> exactly 1/D.  The float32 oracle is within UNIFORM_ATOL / 3 or so."""
    prev, curr, k2s, K, pr, pt, fr = R.case_inputs(name)
    D, (H, W) = fr.shape[0], curr.shape[2:]
    for bias in (0.0, 5.0):
        ref, frag = R.case_ref(name, bias)
        assert float((ref.log_softmax.exp() - 1.0 / D).abs().max()) <= 1e-12
        assert not bool(frag.any())
        out = O.stereo_cost_volume(prev, curr, fr, k2s, K, pr, pt, bias=bias)
        err = float(np.abs(out.astype(np.float64) - 1.0 / D).max())
        print('[parity] stereo %-10s bias %g oracle32 max|p - 1/D| %.2e (GPU bound %.1e)' % (name, bias, err, R.UNIFORM_ATOL))
        assert err <= R.UNIFORM_ATOL / 2
    inside = (ref.ix > -1) & (ref.ix < W) & (ref.iy > -1) & (ref.iy < H)
    if name == 'identity':
        # the sample point is the pixel itself: ix = w, iy = h
        assert float((ref.ix - torch.arange(W, dtype=torch.float64)).abs().max()) < 1e-9
        assert float((ref.iy - torch.arange(H, dtype=torch.float64)[:, None]).abs().max()) < 1e-9
        assert bool(inside.all())
    else:
        assert not bool(inside.any()) and bool((ref.first == 0).all())


@pytest.mark.parametrize('name', list(R.CASES))
def test_case_conditions(name):
    """What the GPU test takes for granted about a case's inputs, on the reference alone."""
    c = R.CASES[name]
    H, W = c['shape']['H'], c['shape']['W']
    for bias in c['biases']:
        ref, frag = R.case_ref(name, bias)
        share = float(frag.double().mean())
        pmin = float(ref.log_softmax.max(1).values.min().exp()), float(ref.log_softmax.min().exp())
        empty, staged, direct = R.tile_plan_stats(ref.ix, ref.iy, H, W)
        behind = float((ref.z < 1e-3).double().mean())
        inside = (ref.ix > -1) & (ref.ix < W) & (ref.iy > -1) & (ref.iy < H)
        biased_inside = float(((ref.first == 0) & inside).double().mean())
        print('[parity] stereo %-16s bias %g fragile %.4f %%  min p %.2e  empty / staged / direct %.3f / %.3f / %.3f  behind %.3f  '
              'biased in view %.3f' % (name, bias, 100 * share, pmin[1], empty, staged, direct, behind, biased_inside))
        assert bool(torch.isfinite(ref.log_softmax).all())
        assert share <= 0.01
        if c['kind'] != 'unit':
            assert pmin[1] >= 1e-5
        else:
            assert pmin[1] < 1e-20 and float((ref.log_softmax >= np.log(R.UNIT_PMIN)).double().mean()) == 1.0
        if c['kind'] == 'zoom':
            assert direct >= 0.05 and empty >= 0.20 and staged >= 0.20
        if name == 'zoom_out':
            assert staged >= 0.99                               # every bin staged, in runs that span whole geometry chunks
        if c['kind'] == 'behind':
            assert behind >= 0.30
        if c['kind'] == 'zero_rect':
            assert biased_inside >= 0.05
            assert float(((ref.first == 0) & ~inside).double().mean()) > 0          # and the ordinary out-of-view kind too


def test_tile_plan_stats_by_hand():
    """one 8 x 8 tile, three bins: all points outside; a 2 x 2 pixel footprint; a footprint over the whole map"""
    H = W = 8
    ix = np.zeros((1, 3, H, W))
    iy = np.zeros((1, 3, H, W))
    ix[0, 0], iy[0, 0] = -5.0, 3.0
    ix[0, 1], iy[0, 1] = 3.5, 2.5
    ix[0, 2], iy[0, 2] = np.meshgrid(np.linspace(-0.5, 7.5, W), np.linspace(-0.5, 7.5, H))
    assert R.tile_plan_stats(ix, iy, H, W, cap=63) == (1 / 3, 1 / 3, 1 / 3)
    assert R.tile_plan_stats(ix, iy, H, W, cap=64) == (1 / 3, 2 / 3, 0.0)
    assert R.tile_plan_stats(ix, iy, H, W, cap=3) == (1 / 3, 0.0, 2 / 3)


def test_fragile_mask_rules():
    """each of the four rules fires on a hand-made point and nothing else does"""
    H, W = 6, 11
    z = torch.full((1, 1, 1, 8), 5.0, dtype=torch.float64)
    ix, iy, first = torch.full_like(z, 3.3), torch.full_like(z, 2.2), torch.full_like(z, 0.7)
    ix[..., 1], ix[..., 2] = -1.0 + 5e-4, W - 5e-4
    iy[..., 3], iy[..., 4] = -1.0 - 5e-4, H + 5e-4
    z[..., 5] = 1e-3 + 5e-6
    first[..., 6] = 1e-7
    first[..., 7] = 0.0                                        # exactly zero is a decision both precisions share
    ref = R.StereoRef(None, None, ix, iy, z, first)
    assert R.fragile_mask(ref, 1.0, H, W).reshape(-1).tolist() == [False, True, True, True, True, True, True, False]
