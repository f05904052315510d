"""The fine-tune step's voxel-loss kernels (csrc/pw_loss.hip, csrc/pw_loss2.hip) at the training grid, (B, 18, 200, 200, 16) with
B = 1 and the reference's training batch B = 2, in both layouts the logits arrive in (ncxyz, and the channels-last OccHead buffer
viewed as (B, C, X, Y, Z)), against the float64 restatement of tests/_loss_ref64.py on the device: the values and the WHOLE gradient
tensor.  At this size the multi-block paths run that the small fixtures (1 440 voxels) barely reach: 512 statistics blocks, and
the Lovasz scan's cross-block prefix over ~1 250 blocks of LV_BLOCK = 1 024 sorted elements per class.

The Lovasz kernel sorts on a 27-bit key (lv_key, pw_loss2.hip): errors that agree to ~2^-20 are ties, kept in walk order, so its
per-element gradient inside a run of equal keys depends on that order.  The test groups each class's valid voxels by the key,
recomputed here from lv_key's definition: a group of one is compared element by element; for a tied group the sum of
gradient x sign (-1 foreground, +1 background) -- the sum of lovasz_grad over the run, which depends only on how many foreground and
background voxels it holds -- is compared with the float64 reference's sum over the same voxels (keys are monotone in the error,
so the group is a contiguous run of the exact order too)."""
import numpy as np
import pytest
import torch

import _loss_ref64 as R
from _parity import check_close
from oracle import oracle as O
from preworld_amd import losses as L

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GRID = (200, 200, 16)
LV_KEY_ZERO = (1 << 27) - 2                 # pw_loss2.hip: the key of a zero error; LV_KEY_INVALID = LV_KEY_ZERO + 1
REL = 1e-5                                  # gradients: max |err| <= REL * max |ref|


def _inputs(seed, B, layout, X=200, Y=200, Z=16, scale=2.0):
    """logits (B, 18, X, Y, Z) ~ N(0, scale^2), labels with 10 % 255 and 40 % 17, camera mask 80 % -- synth.voxel_loss_inputs' mix,
    drawn on the device"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    pred = torch.randn((B, 18, X, Y, Z), generator=g, device=DEV) * scale
    target = torch.randint(0, 18, (B, X, Y, Z), generator=g, device=DEV)
    target[torch.rand((B, X, Y, Z), generator=g, device=DEV) < 0.1] = 255
    target[torch.rand((B, X, Y, Z), generator=g, device=DEV) < 0.4] = 17
    cam = torch.rand((B, X, Y, Z), generator=g, device=DEV) < 0.8
    return _layout(pred, layout), target, cam


def _layout(pred, layout):
    if layout == 'channels_last':                   # the OccHead logits buffer (B, Z, Y, X, C) viewed as (B, C, X, Y, Z)
        pred = pred.permute(0, 4, 3, 2, 1).contiguous().permute(0, 4, 3, 2, 1)
        assert not pred.is_contiguous()
    return pred.contiguous() if layout == 'ncxyz' else pred


def _class_weights():
    g = torch.Generator(device=DEV).manual_seed(11)
    return torch.cat([torch.rand(17, generator=g, device=DEV) * 0.05 + 0.05, torch.zeros(1, device=DEV)])


def _value(name, got, want, rtol):
    got, want = float(torch.as_tensor(got).detach()), float(torch.as_tensor(want).detach())
    print('[parity] %-44s got %.9g  ref %.9g  rel %.2e (bound %.1e)' % (name, got, want, abs(got - want) / abs(want), rtol))
    assert abs(got - want) <= rtol * abs(want), (name, got, want)


# ------------------------------------------------------------------------------------------------- CE + sem_scal + geo_scal
def _check_voxel_losses(name, pred, target, cam, cw):
    pred = pred.detach().requires_grad_(True)
    ce, sem, geo = L.voxel_losses(pred, target, cw, 255, 17, cam)
    (1.0 * ce + 0.7 * sem + 1.3 * geo).backward()
    p64 = pred.detach().double().requires_grad_(True)
    rce, rsem, rgeo = R.voxel_losses(p64, target, cw.double(), 255, 17, cam)
    (1.0 * rce + 0.7 * rsem + 1.3 * rgeo).backward()
    for tag, got, want in (('ce', ce, rce), ('sem', sem, rsem), ('geo', geo, rgeo)):
        _value('%s %s' % (name, tag), got, want, 3e-6)
    assert torch.isfinite(pred.grad).all()
    check_close('%s grad (whole tensor)' % name, pred.grad, p64.grad, REL)


@pytest.mark.parametrize('layout', ['ncxyz', 'channels_last'])
@pytest.mark.parametrize('B', [1, 2])
def test_ce_sem_geo_whole_gradient_at_the_training_grid(B, layout):
    """pw_voxel_loss_stats / _finish / _coef / _grad: the three values to 3e-6 relative, the whole gradient of
    1.0 ce + 0.7 sem + 1.3 geo to 1e-5 of its largest entry.  (0.02 s per case on an MI355X; 1.3 s for the first, which warms up)"""
    pred, target, cam = _inputs(21 + B, B, layout)
    _check_voxel_losses('ce+sem+geo B=%d %s' % (B, layout), pred, target, cam, _class_weights())


def test_ce_sem_geo_saturated_softmax_and_clamped_logs():
    """Logits to +-60 (the softmax saturates, many probabilities underflow in float32), one class present in a single voxel whose
    logit is -60 while another class's is +60 (its recall and precision underflow to 0: the BCE log clamp at -100 is reached), one
    class absent.  The reference's gradient there is finite -- F.binary_cross_entropy's backward divides by max(x (1 - x), 1e-12)
    -- and so must the kernel's be.  (0.1 s on an MI355X)"""
    g = torch.Generator(device=DEV).manual_seed(31)
    B = 2
    pred = (torch.randn((B, 18) + GRID, generator=g, device=DEV) * 20).clamp(-60, 60)
    target = torch.randint(0, 18, (B,) + GRID, generator=g, device=DEV)
    target[target == 5] = 6                                        # class 5: only in the one voxel below
    target[target == 9] = 10                                       # class 9: absent
    target[torch.rand((B,) + GRID, generator=g, device=DEV) < 0.1] = 255
    cam = torch.rand((B,) + GRID, generator=g, device=DEV) < 0.8
    v = (1, 120, 37, 9)
    target[v] = 5
    cam[v] = True
    pred[(v[0], slice(None)) + v[1:]] = -60.0
    pred[(v[0], 3) + v[1:]] = 60.0
    assert int((target == 5).sum()) == 1 and int((target == 9).sum()) == 0
    _check_voxel_losses('ce+sem+geo saturated', _layout(pred, 'channels_last'), target, cam, _class_weights())


# ------------------------------------------------------------------------------------------------- focal
@pytest.mark.parametrize('layout', ['ncxyz', 'channels_last'])
@pytest.mark.parametrize('B', [1, 2])
def test_focal_whole_gradient_at_the_training_grid(B, layout):
    """pw_focal_loss_stats / _finish / _grad (CustomFocalLoss, radial map of the 200 x 200 grid): the value to 3e-6 relative and
    every gradient element -- not a [::97] sample -- to 1e-5 of the largest.  (0.01-0.24 s per case on an MI355X)"""
    pred, target, cam = _inputs(41 + B, B, layout)
    cw = _class_weights()
    pred = pred.detach().requires_grad_(True)
    loss = L.CustomFocalLoss()(pred, target, cw, None, 255, camera_mask=cam)
    (2.5 * loss).backward()
    p64 = pred.detach().double().requires_grad_(True)
    ref = R.focal_loss(p64, target, cw.double(), 255, cam)
    (2.5 * ref).backward()
    _value('focal B=%d %s' % (B, layout), loss, ref, 3e-6)
    check_close('focal B=%d %s grad (whole tensor)' % (B, layout), pred.grad, p64.grad, REL)


# ------------------------------------------------------------------------------------------------- Lovasz
def lv_key(err32):
    """lv_key of pw_loss2.hip: the complement of the float32 error's bit pattern without its top two bits and its 3 lowest mantissa
    bits, clamped to LV_KEY_ZERO (ascending key = descending error)"""
    bits = err32.contiguous().view(torch.int32).long() & 0xFFFFFFFF
    return (((~bits) & 0x3FFFFFFF) >> 3).clamp_(max=LV_KEY_ZERO)


def _check_lovasz(name, probas, labels, ignore=17, cam=None):
    """kernel value and dL/dprobas against the float64 restatement, tie-order independent (module docstring); -> voxels in ties"""
    pk = probas.detach().requires_grad_(True)
    loss = L.lovasz_softmax(pk, labels, ignore=ignore, camera_mask=cam)
    loss.backward()
    p64 = probas.detach().double().requires_grad_(True)
    ref = R.lovasz_softmax(p64, labels, ignore, cam)
    ref.backward()
    if float(ref.detach()) == 0.0:
        assert float(loss.detach()) == 0.0 and float(pk.grad.abs().max()) == 0.0, name
        print('[parity] %-44s value 0 and gradient 0, as the reference' % name)
        return 0
    _value(name, loss, ref, 2e-6)
    B, C = probas.shape[:2]
    valid, vp, vl = R.lovasz_classes(probas.detach(), labels, ignore, cam)
    gk = pk.grad.reshape(B, C, -1).movedim(1, 2).reshape(-1, C)
    gr = p64.grad.reshape(B, C, -1).movedim(1, 2).reshape(-1, C)
    if bool((~valid).any()):
        assert float(gk[~valid].abs().max()) == 0.0, name                                 # ignored / masked voxels get nothing
    gk, gr = gk[valid].double(), gr[valid]
    scale = float(gr.abs().max())
    err_one, err_run, n_tied, n_runs = 0.0, 0.0, 0, 0
    for c in range(C):
        fg = vl == c
        if not bool(fg.any()):
            assert float(gk[:, c].abs().max()) == 0.0, (name, 'absent class', c)
            continue
        e64 = (fg.double() - vp[:, c].double()).abs()
        key = lv_key((fg.float() - vp[:, c]).abs().clamp_(max=1.0))
        order = torch.sort(e64, descending=True, stable=True).indices
        ks = key[order]
        assert bool((ks[1:] >= ks[:-1]).all()), 'keys are not monotone in the exact error'
        start = torch.ones_like(ks, dtype=torch.bool)
        start[1:] = ks[1:] != ks[:-1]
        gid = start.long().cumsum(0) - 1
        cnt = torch.bincount(gid)
        a, b = gk[order, c], gr[order, c]
        one = cnt[gid] == 1
        if bool(one.any()):
            err_one = max(err_one, float((a - b)[one].abs().max()))
        sgn = torch.where(fg[order], -1.0, 1.0).double()
        sa = torch.zeros(cnt.numel(), dtype=torch.float64, device=DEV).index_add_(0, gid, a * sgn)
        sb = torch.zeros(cnt.numel(), dtype=torch.float64, device=DEV).index_add_(0, gid, b * sgn)
        run = cnt > 1
        if bool(run.any()):
            err_run = max(err_run, float((sa - sb)[run].abs().max()))
            n_tied += int(cnt[run].sum())
            n_runs += int(run.sum())
    print('[parity] %-44s max|ref| %.3e; singletons max|err| %.3e rel %.2e; tied runs (%d voxel-classes in %d runs) max|err of '
          'sum| %.3e rel %.2e (bound %.1e)' % (name + ' grad', scale, err_one, err_one / scale, n_tied, n_runs, err_run,
                                               err_run / scale, REL))
    assert err_one <= REL * scale and err_run <= REL * scale, (name, err_one, err_run, scale)
    return n_tied


@pytest.mark.parametrize('layout', ['ncxyz', 'channels_last'])
@pytest.mark.parametrize('B', [1, 2])
def test_lovasz_gradient_at_the_training_grid(B, layout):
    """pw_lovasz_softmax on softmax probabilities of the training grid (~1 250 blocks of 1 024 sorted elements per class): the value
    to 2e-6 relative, the gradient by key groups to 1e-5 of its largest entry.  (0.02-0.26 s per case on an MI355X)"""
    pred, target, cam = _inputs(61 + B, B, layout)
    _check_lovasz('lovasz B=%d %s' % (B, layout), L._softmax_classes(pred), target, 17, cam)


def test_lovasz_dense_near_ties():
    """Probabilities on a 2^-18 grid plus noise below the key's bucket width: every class has runs of equal keys holding foreground
    and background voxels together (exact ties and ties of the 27-bit key).  (0.03 s on an MI355X)"""
    g = torch.Generator(device=DEV).manual_seed(71)
    B = 2
    k = torch.randint(0, 1 << 18, (B, 18) + GRID, generator=g, device=DEV).double()
    noise = torch.rand((B, 18) + GRID, generator=g, device=DEV).double() * 2.0 ** -24
    probas = ((k * 2.0 ** -18 + noise).clamp(0, 1)).float()
    _, target, cam = _inputs(72, B, 'ncxyz')
    n_tied = _check_lovasz('lovasz dense near-ties', probas, target, 17, cam)
    assert n_tied > 1_000_000


def test_lovasz_cross_block_prefix_below_the_chunked_scan():
    """A grid of 12 800 voxels, ~5 500 of them valid: six blocks of 1 024 sorted elements per class, each block its own chunk of
    k_lovasz_scan (fewer than 256 blocks; the training grid has ~1 250, five per chunk).  (0.02 s on an MI355X)"""
    pred, target, cam = _inputs(81, 2, 'ncxyz', X=40, Y=40, Z=4)
    valid = (target != 17) & cam
    assert int(valid.sum()) > 4 * 1024
    _check_lovasz('lovasz 12 800 voxels', L._softmax_classes(pred), target, 17, cam)


def test_lovasz_degenerate_inputs_as_the_oracle():
    """Every voxel ignored, camera mask all false: value 0, gradient 0.  A class present only in masked voxels is not present.
    (0.07 s on an MI355X)"""
    pred, target, cam = _inputs(91, 1, 'ncxyz', X=20, Y=20, Z=4)
    probas = L._softmax_classes(pred)
    _check_lovasz('lovasz all ignored', probas, torch.full_like(target, 17), 17, cam)
    _check_lovasz('lovasz camera mask all false', probas, target, 17, torch.zeros_like(cam))
    t2, cam2 = target.clone(), cam.clone()
    cam2[t2 == 4] = False                                          # class 4 only where the camera mask is false
    _check_lovasz('lovasz class only in masked voxels', probas, t2, 17, cam2)
    pk = probas.detach().requires_grad_(True)
    loss = L.lovasz_softmax(pk, t2, ignore=17, camera_mask=cam2)
    loss.backward()
    assert float(pk.grad[:, 4].abs().max()) == 0.0
    np.testing.assert_allclose(float(loss.detach()), O.lovasz_softmax(probas.cpu().numpy(), t2.cpu().numpy(), 17, cam2.cpu().numpy()),
                               rtol=2e-6)
