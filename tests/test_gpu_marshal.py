"""_lib.call's argument converters on the device: a tensor that does not match the header's declaration is refused in Python -- the C
function is never entered (pw_last_error() stays as it was), so no bad pointer ever reaches a kernel.  Rejections only, plus the one
positive case of the `strided` marker.  B = 1, a 4x8x8 grid with 32 channels, 18 x 4x4x2 logits, 8 ranks."""
import pytest
import torch

from preworld_amd import _lib, losses, ops, train

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _refused(fn, *args, **kw):
    l = _lib.lib()
    torch.cuda.synchronize()
    before = l.pw_last_error()
    with pytest.raises(_lib.PreworldHipError) as e:
        fn(*args, **kw)
    assert l.pw_last_error() == before
    return str(e.value)


@pytest.fixture(scope='module')
def grid():
    gen = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn(1, 4, 8, 8, 32, device=DEV, generator=gen)
    w = torch.randn(32, 32, 3, 3, 3, device=DEV, generator=gen) * 0.05
    return x, w


def test_conv3d_ndhwc_float64_scale(grid):
    x, w = grid
    msg = _refused(ops.conv3d_ndhwc, x, ops.pack_conv_weight(w), scale=torch.ones(32, device=DEV, dtype=torch.float64))
    assert msg == 'pw_conv3d_ndhwc: scale must be torch.float32, got torch.float64', msg


def test_conv3d_h2_strided_bias(grid):
    x, w = grid
    wpk, inv = ops.pack_conv_weight_h2(w)
    msg = _refused(ops.conv3d_h2, ops.f32_to_h2(x), wpk, inv, bias=torch.zeros(64, device=DEV)[::2])
    assert msg == 'pw_conv3d_h2: bias must be contiguous', msg


def test_f32_to_h2_int32_input(grid):
    msg = _refused(ops.f32_to_h2, torch.zeros(1, 4, 8, 8, 32, device=DEV, dtype=torch.int32))
    assert msg == 'pw_f32_to_h2: x must be torch.float32, got torch.int32', msg


def test_losses_move_a_host_target():
    """losses._args moves target / camera_mask / class_weights to the logits' device where it converts them"""
    gen = torch.Generator().manual_seed(1)
    pred = (torch.randn(1, 18, 4, 4, 2, generator=gen) * 2).to(DEV)
    target = torch.randint(0, 18, (1, 4, 4, 2), generator=gen)
    cam = torch.rand(1, 4, 4, 2, generator=gen) < 0.8
    cw = torch.rand(18, generator=gen) + 0.1
    want = losses.voxel_losses(pred, target.to(DEV), cw.to(DEV), 255, 17, cam.to(DEV))
    got = losses.voxel_losses(pred, target, cw, 255, 17, cam)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_bn_apply_host_mean(grid):
    x, _ = grid
    one = torch.ones(32, device=DEV)
    msg = _refused(train.bn_apply, x, torch.zeros(32), one, one, one)
    assert msg == 'pw_bn_apply: mean must be a CUDA(HIP) tensor', msg


def test_raw_bev_pool_int64_ranks():
    depth, feat, out = torch.zeros(8, device=DEV), torch.zeros(8, 32, device=DEV), torch.zeros(8, 32, device=DEV)
    r = torch.arange(8, device=DEV, dtype=torch.int32)
    one = torch.ones(8, device=DEV, dtype=torch.int32)
    msg = _refused(_lib.call, 'pw_bev_pool_v2_forward', depth, feat, out, r.long(), r, r, one, r, 32, 8, _lib.STREAM)
    assert msg == 'pw_bev_pool_v2_forward: ranks_depth must be torch.int32, got torch.int64', msg


def test_channel_slice_needs_the_marker(grid):
    x, _ = grid
    wide = torch.cat([x, -x], dim=-1)                      # (1,4,8,8,64): x is its channel slice [..., :32], row stride 64
    sl, n = wide[..., :32], x.numel() // 32
    assert not sl.is_contiguous()
    slot = torch.zeros(ops.RNG_ROW, dtype=torch.int32, device=DEV)
    out = torch.empty_like(x)
    msg = _refused(_lib.call, 'pw_f32_to_h2', sl, out, n, 32, 64, 32, slot, 0, _lib.STREAM)
    assert msg == 'pw_f32_to_h2: x must be contiguous', msg
    # with the marker the same call runs, and gives the bits of the dense tensor
    _lib.call('pw_f32_to_h2', _lib.strided(sl), out, n, 32, 64, 32, slot, 0, _lib.STREAM)
    dense = torch.empty_like(x)
    _lib.call('pw_f32_to_h2', x, dense, n, 32, 32, 32, torch.zeros_like(slot), 0, _lib.STREAM)
    assert torch.equal(out.view(torch.int32), dense.view(torch.int32))
    # the marker skips the contiguity check only
    assert 'must be torch.float32' in _refused(_lib.call, 'pw_f32_to_h2', _lib.strided(sl.int()), out, n, 32, 64, 32, slot, 0, _lib.STREAM)
    assert 'must be a CUDA(HIP) tensor' in _refused(_lib.call, 'pw_f32_to_h2', _lib.strided(sl.cpu()), out, n, 32, 64, 32, slot, 0, _lib.STREAM)
