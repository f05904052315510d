"""The float64 restatement of the voxel losses (tests/_loss_ref64.py), which the GPU tests of the loss kernels at the training grid
measure against, pinned on the CPU before anything relies on it: it reproduces the values and gradients the imported reference
recorded (tests/golden/voxel_losses.npz, voxel_losses2.npz; float32 torch on the CPU) to their float32 precision, and it agrees
with the numpy oracle (oracle.voxel_losses, focal_loss_voxel, lovasz_softmax)."""
import numpy as np
import pytest
import torch

import _loss_ref64 as R
from _parity import check_close
from oracle import oracle as O
from preworld_amd import synth as S


def D(a):
    return torch.from_numpy(np.asarray(a)).double()


@pytest.mark.parametrize('tag', ['cam', 'nocam'])
def test_ce_sem_geo_reproduce_the_reference_fixture(golden, tag):
    g = golden('voxel_losses.npz')
    pred_np, target_np, cam_np = S.voxel_loss_inputs(int(g['seed']))
    pred = D(pred_np).requires_grad_(True)
    cam = torch.from_numpy(cam_np) if tag == 'cam' else None
    ce, sem, geo = R.voxel_losses(pred, torch.from_numpy(target_np), D(g['class_weights']), 255, 17, cam)
    for got, key in ((ce, 'ce_'), (sem, 'sem_'), (geo, 'geo_')):
        check_close('ref64 %s%s vs reference' % (key, tag), np.array([got.item()]), np.array([float(g[key + tag])]), 1e-6)
    (1.0 * ce + 0.7 * sem + 1.3 * geo).backward()
    check_close('ref64 ce+sem+geo grad %s vs reference' % tag, pred.grad, g['grad_' + tag], 1e-6)
    oce, osem, ogeo = O.voxel_losses(pred_np, target_np, g['class_weights'], 255, 17, cam_np if tag == 'cam' else None)
    np.testing.assert_allclose([ce.item(), sem.item(), geo.item()], [oce, osem, ogeo], rtol=1e-12)


@pytest.mark.parametrize('tag', ['cam', 'nocam'])
def test_focal_reproduces_the_reference_fixture_and_the_oracle(golden, tag):
    g = golden('voxel_losses2.npz')
    cw = golden('voxel_losses.npz')['class_weights']
    pred_np, target_np, cam_np = S.voxel_loss_inputs(int(g['seed_focal']), shape=(1, 18, 200, 200, 2))
    cam_np = cam_np if tag == 'cam' else None
    pred = D(pred_np).requires_grad_(True)
    loss = R.focal_loss(pred, torch.from_numpy(target_np), D(cw), 255, None if cam_np is None else torch.from_numpy(cam_np))
    check_close('ref64 focal %s vs reference' % tag, np.array([loss.item()]), np.array([float(g['focal_' + tag])]), 1e-6)
    loss.backward()
    grad = pred.grad.numpy()
    check_close('ref64 focal grad[::97] %s vs reference' % tag, grad.reshape(-1)[::97], g['focal_grad_' + tag], 1e-6)
    ov, og = O.focal_loss_voxel(pred_np, target_np, cw, 255, cam_np, want_grad=True)
    np.testing.assert_allclose(loss.item(), ov, rtol=1e-12)
    check_close('ref64 focal grad %s vs oracle' % tag, grad, og, 1e-6)     # the oracle's gradient is stored in float32


@pytest.mark.parametrize('tag', ['cam', 'nocam'])
def test_lovasz_reproduces_the_reference_fixture_and_the_oracle(golden, tag):
    g = golden('voxel_losses2.npz')
    pred_np, target_np, cam_np = S.voxel_loss_inputs(int(g['seed_lovasz']))
    cam = torch.from_numpy(cam_np) if tag == 'cam' else None
    target = torch.from_numpy(target_np)
    pred = D(pred_np).requires_grad_(True)
    loss = R.lovasz_softmax(torch.softmax(pred, dim=1), target, 17, cam)
    check_close('ref64 lovasz %s vs reference' % tag, np.array([loss.item()]), np.array([float(g['lovasz_' + tag])]), 1e-6)
    loss.backward()
    # the reference (and the oracle) take lovasz_grad as differences of float32 Jaccard values, each within an ulp of 1: 2-3e-6 of
    # the largest gradient here; the restatement forms them in float64
    check_close('ref64 lovasz grad (logits) %s vs reference' % tag, pred.grad, g['lovasz_grad_' + tag], 1e-5)
    # the oracle takes float32 probabilities and forms lovasz_grad from float32 cumulative sums, as the reference does: the
    # restatement is fed the same float32 probabilities, so both sort the same errors
    pr32 = torch.softmax(torch.from_numpy(pred_np), dim=1)
    pr = pr32.double().requires_grad_(True)
    loss = R.lovasz_softmax(pr, target, 17, cam)
    ov, og = O.lovasz_softmax(pr32.numpy(), target_np, 17, cam_np if tag == 'cam' else None, want_grad=True)
    np.testing.assert_allclose(loss.item(), ov, rtol=1e-6)
    loss.backward()
    check_close('ref64 lovasz grad (probas) %s vs oracle' % tag, pr.grad, og, 1e-5)


def test_lovasz_degenerate_inputs_are_zero():
    """nothing valid, camera mask all false, and a class present only in masked voxels (it does not count as present)"""
    rs = np.random.RandomState(2)
    pr = torch.softmax(D(rs.standard_normal((1, 5, 4, 3, 2))), dim=1).requires_grad_(True)
    lab = torch.from_numpy(rs.randint(0, 5, (1, 4, 3, 2)))
    assert R.lovasz_softmax(pr, torch.full_like(lab, 4), ignore=4).item() == 0.0
    assert R.lovasz_softmax(pr, lab, ignore=None, camera_mask=torch.zeros_like(lab, dtype=torch.bool)).item() == 0.0
    cam = lab != 3
    lab2 = lab.clone()
    lab2[0, 0, 0, 0] = 3
    cam[0, 0, 0, 0] = False
    got = R.lovasz_softmax(pr, lab2, ignore=None, camera_mask=cam).item()
    assert got > 0
    np.testing.assert_allclose(got, O.lovasz_softmax(pr.detach().float().numpy(), lab2.numpy(), None, cam.numpy()), rtol=1e-6)
