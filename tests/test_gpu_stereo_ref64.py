"""GPU: pw_stereo_cost_volume (csrc/pw_stereo.hip behind ops.stereo_cost_volume) on every kernel path -- the point-per-lane kernels
k_stereo_cost_volume<false> / <true> and the LDS-tiled k_stereo_cost_volume_tile<128> / <0> with their staged, direct-gather and
empty branches -- against the float64 restatement of tests/_stereo_ref64.py.

Every case compares log(out) with the reference log_softmax element by element outside the fragile mask: with the features scaled
so that no probability underflows this sees every bin's cost.  The bound is 4 x the case's float32 floor (FLOORS, measured on the
CPU from the float32 oracle, never from a kernel); test_stereo_ref64_cpu.py proves on the reference alone that each case's inputs
reach the branch it is here for, and the [parity] lines repeat those shares.  Each run also asserts the dispatched kernel,
sum over D = 1, finiteness and bit-identical repetition.

The library reports both tiled instantiations as 'k_stereo_cost_volume_tile'; which one ran follows from C (== 128: <128>), so
the labels below carry the template argument and the assertion compares the reported name without it."""
import numpy as np
import pytest
import torch

import _stereo_ref64 as R
from preworld_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NCHW, TRUE = 'k_stereo_cost_volume<false>', 'k_stereo_cost_volume<true>'
TILE128, TILE0 = 'k_stereo_cost_volume_tile<128>', 'k_stereo_cost_volume_tile<0>'


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dense(t):
    return T(t)


def channels_last(t):
    return T(t).contiguous(memory_format=torch.channels_last)


def cl_kernel(name):
    C = R.CASES[name]['shape']['C']
    return TILE128 if C == 128 else TILE0 if C < 128 else TRUE


def reported(label):
    return label[:label.index('_tile') + 5] if '_tile' in label else label


def run_case(name, place, kernel, tag):
    """one case in one feature placement: place(numpy (BN, C, H, W)) -> a (BN, C, H, W) device tensor of any strides"""
    prev, curr, k2s, K, pr, pt, fr = R.case_inputs(name)
    c = R.CASES[name]
    D, H, W = c['shape']['D'], c['shape']['H'], c['shape']['W']
    tp, tc = place(prev), place(curr)
    assert tuple(tp.shape) == prev.shape and tp.stride() == tc.stride()
    args = (T(fr), T(k2s), T(K), T(pr), T(pt))
    for bias in c['biases'] if c['kind'] != 'uniform' else (0.0, 5.0):
        out = ops.stereo_cost_volume(tp, tc, *args, bias=bias)
        ran = _lib.lib().pw_last_kernel().decode()
        again = ops.stereo_cost_volume(tp, tc, *args, bias=bias)
        ref, _ = R.case_ref(name, bias)
        shares = R.tile_plan_stats(ref.ix, ref.iy, H, W)
        label = '%s %s' % (tag, kernel[len('k_stereo_cost_volume'):])
        if c['kind'] == 'uniform':
            err = float((out.double() - 1.0 / D).abs().max())
            print('[parity] stereo %-16s bias %g %-34s max|p - 1/D| %.3e (bound %.1e)' % (name, bias, label, err, R.UNIFORM_ATOL))
            bound = R.UNIFORM_ATOL
        else:
            err = R.log_error(name, out, bias, report=label)
            bound = R.FACTOR * R.FLOORS[name]
        print('[parity] stereo %-16s tile plan of these inputs: empty %.3f  staged %.3f  direct %.3f; ran %s' % ((name,) + shares + (ran,)))
        assert ran == reported(kernel), (name, tag, ran, kernel)
        assert bool(torch.isfinite(out).all()), (name, tag, 'not finite')
        assert float(out.double().sum(1).sub(1).abs().max()) <= 1e-5, (name, tag)
        assert torch.equal(out, again), (name, tag, 'a second call differs')
        assert err <= bound, (name, tag, bias, err, bound)


LAYOUTS = [pytest.param(dense, id='nchw'), pytest.param(channels_last, id='channels_last')]


def both(name, place):
    run_case(name, place, NCHW if place is dense else cl_kernel(name), 'nchw' if place is dense else 'channels-last')


@pytest.mark.parametrize('place', LAYOUTS)
def test_reference_width(place):
    """C = 128, D = 88 at the default pose: 704 threads per block in <false>, both softmax registers in tile<128>"""
    both('ref_width', place)


def test_direct_gather_reference_width():
    """strong parallax at near bins 0.25 m apart: 7 % of the (tile, bin) entries exceed the staging buffer, 26 % are empty"""
    both('direct128', channels_last)


@pytest.mark.parametrize('place', LAYOUTS)
def test_direct_gather_generic_channels(place):
    both('direct16', place)


@pytest.mark.parametrize('D', [2, 63, 64, 65, 128])
@pytest.mark.parametrize('place', LAYOUTS)
def test_softmax_halves(place, D):
    """D around the 64 lanes of the tiled softmax's first register, and at both ends of what the ABI accepts"""
    both('softmax_D%d' % D, place)


def test_long_staged_runs():
    """zoom-out: every bin's footprint is small, runs span whole geometry chunks"""
    both('zoom_out', channels_last)


@pytest.mark.parametrize('C', [4, 124])
@pytest.mark.parametrize('HW', [(2, 2), (2, 9), (8, 8), (9, 8), (7, 16)], ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('place', LAYOUTS)
def test_tile_edges(place, HW, C):
    """one channel group and 31 of the 32 lanes' groups; maps below, at and one past the 8-pixel tile"""
    both('edge_C%d_%dx%d' % ((C,) + HW), place)


def test_channels_last_point_per_lane_kernel():
    """C = 132 > 128 channels-last: the float4 point-per-lane kernel no other test reaches"""
    assert cl_kernel('c132') == TRUE
    both('c132', channels_last)


@pytest.mark.parametrize('place', LAYOUTS)
def test_behind_the_camera(place):
    both('behind', place)


@pytest.mark.parametrize('place', LAYOUTS)
def test_bias_rule_inside_the_view(place):
    """a rectangle of zeros in channel C - 4 of prev: 12 % of the points take the bias while every corner is inside the map"""
    both('zero_rect', place)


@pytest.mark.parametrize('name', ['identity', 'sideways'])
@pytest.mark.parametrize('place', LAYOUTS)
def test_analytic_uniform(place, name):
    both(name, place)


def test_unit_amplitude():
    """N(0, 1) features at C = 128: probabilities down to 4e-28, compared in log space wherever the reference is >= 1e-30"""
    both('unit_amp', channels_last)


# ------------------------------------------------------------------------------------------------ strided views
def _nan(*shape):
    return torch.full(shape, float('nan'), device=DEV)


def channel_slice(c0, c_buf):
    """the features as channels [c0, c0 + C) of a channels-last (BN, H, W, c_buf) buffer full of NaN"""
    def place(a):
        BN, C, H, W = a.shape
        buf = _nan(BN, H, W, c_buf)
        v = buf[..., c0:c0 + C]
        v.copy_(T(a).permute(0, 2, 3, 1))
        return v.permute(0, 3, 1, 2)
    return place


def spatial_crop(a):
    BN, C, H, W = a.shape
    buf = _nan(BN, H + 3, W + 5, C)
    v = buf[:, 1:1 + H, 2:2 + W]
    v.copy_(T(a).permute(0, 2, 3, 1))
    return v.permute(0, 3, 1, 2)


def every_second_camera(a):
    BN, C, H, W = a.shape
    buf = _nan(2 * BN, H, W, C)
    v = buf[::2]
    v.copy_(T(a).permute(0, 2, 3, 1))
    return v.permute(0, 3, 1, 2)


def test_view_machinery():
    """the views are what the cases below say they are"""
    a = np.zeros((2, 16, 3, 5), np.float32)
    v = channel_slice(4, 24)(a)
    assert v.stride() == (3 * 5 * 24, 1, 5 * 24, 24) and v.data_ptr() % 16 == 0
    v = channel_slice(2, 24)(a)
    assert v.stride()[3] == 24 and v.data_ptr() % 16 == 8
    v = channel_slice(0, 18)(a)
    assert v.stride()[3] == 18 and v.data_ptr() % 16 == 0
    v = spatial_crop(a)
    assert v.stride() == ((3 + 3) * (5 + 5) * 16, 1, (5 + 5) * 16, 16) and v.data_ptr() % 16 == 0
    v = every_second_camera(a)
    assert v.stride() == (2 * 3 * 5 * 16, 1, 5 * 16, 16)
    assert bool((v == 0).all())                                 # the view holds the data, the NaN is all around it


@pytest.mark.parametrize('place, kernel, name', [
    pytest.param(channel_slice(4, 24), TILE0, 'direct16', id='a-aligned-channel-slice'),
    pytest.param(channel_slice(2, 24), NCHW, 'direct16', id='b-unaligned-base'),
    pytest.param(channel_slice(0, 18), NCHW, 'direct16', id='c-pixel-stride-18'),
    pytest.param(spatial_crop, TILE0, 'direct16', id='d-spatial-crop'),
    pytest.param(every_second_camera, TILE0, 'direct16_2cam', id='e-every-second-camera'),
])
def test_strided_views(place, kernel, name):
    """the 16-channel direct-gather case read through views of larger NaN-filled buffers: a read outside the view poisons the
    result.  Aligned views with a pixel stride of any multiple of 4 keep the tiled kernel; an unaligned base or a pixel stride
    that is no multiple of 4 must fall back to the strided point-per-lane kernel."""
    run_case(name, place, kernel, 'view')
