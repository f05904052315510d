"""The float64 restatement of the bias-free Conv3d (tests/_conv_ref64.py), which the GPU tests of the training-side convolution
kernels at the training grid measure against, pinned on the CPU before anything relies on it: its forward, data gradient and weight
gradient are F.conv3d's under float64 autograd (channels-first, padding k // 2, none for k = 2) for every kernel size and stride the
training step uses, at B = 2 with odd extents and channel counts that are not multiples of 32; slabbing over the output depth
changes nothing; and its forward agrees with the numpy oracle's conv3d (oracle.conv3d, float32)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _conv_ref64 as C
from _parity import check_close
from oracle import oracle as O

CASES = [  # (B, D, H, W), Cin, Cout, k, stride
    ((2, 5, 7, 9), 13, 21, 3, 1),
    ((2, 7, 6, 5), 19, 11, 3, 2),
    ((2, 6, 5, 8), 17, 40, 3, 2),
    ((2, 5, 9, 7), 35, 9, 1, 1),
    ((2, 7, 5, 6), 10, 6, 1, 2),
    ((2, 7, 9, 5), 12, 33, 2, 2),
    ((2, 8, 6, 10), 33, 18, 2, 2),
    ((2, 1, 1, 3), 7, 5, 3, 1),
]
IDS = ['k%d-s%d-%dx%dx%dx%d-%d-%d' % (k, s, *shape, ci, co) for shape, ci, co, k, s in CASES]


def cl(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


def ncdhw(t):
    return t.permute(0, 4, 1, 2, 3)


def _torch64(x_cl, w, g_cl, stride):
    """y, dX, dW of F.conv3d under float64 autograd, channels-last"""
    x = ncdhw(x_cl).detach().clone().requires_grad_(True)
    wt = w.detach().clone().requires_grad_(True)
    y = F.conv3d(x, wt, stride=stride, padding=C.conv_pad(w.shape[2]))
    y.backward(ncdhw(g_cl))
    return cl(y.detach()), cl(x.grad), wt.grad


@pytest.mark.parametrize('shape,cin,cout,k,stride', CASES, ids=IDS)
def test_ref64_matches_float64_autograd_of_conv3d(shape, cin, cout, k, stride):
    B, D, H, W = shape
    gen = torch.Generator().manual_seed(cin * 97 + cout * 7 + k * 3 + stride)
    x = torch.randn((B, D, H, W, cin), generator=gen, dtype=torch.float64)
    w = torch.randn((cout, cin, k, k, k), generator=gen, dtype=torch.float64)
    Do, Ho, Wo = (C.out_extent(n, k, stride) for n in (D, H, W))
    g = torch.randn((B, Do, Ho, Wo, cout), generator=gen, dtype=torch.float64)
    y_t, dx_t, dw_t = _torch64(x, w, g, stride)
    y = C.conv3d(x, w, stride)
    dx = C.conv3d_dx(g, w, x.shape, stride)
    dw = C.conv3d_dw(x, g, k, stride)
    assert y.dtype == dx.dtype == dw.dtype == torch.float64
    check_close('ref64 y  k%d s%d %s' % (k, stride, shape), y, y_t, 1e-13)
    check_close('ref64 dX k%d s%d %s' % (k, stride, shape), dx, dx_t, 1e-13)
    check_close('ref64 dW k%d s%d %s' % (k, stride, shape), dw, dw_t, 1e-13)
    # the adjoint identity <conv(x), g> = <x, dX(g)> = <w, dW(x, g)>, independent of autograd
    ip = float((y * g).sum())
    assert abs(ip - float((x * dx).sum())) <= 1e-12 * max(abs(ip), 1.0)
    assert abs(ip - float((w * dw).sum())) <= 1e-12 * max(abs(ip), 1.0)
    # slabs over the output depth give the same sums in another grouping
    for slab in (1, 2):
        check_close('ref64 y  slab %d' % slab, C.conv3d(x, w, stride, slab=slab), y, 1e-14)
        check_close('ref64 dX slab %d' % slab, C.conv3d_dx(g, w, x.shape, stride, slab=slab), dx, 1e-14)
        check_close('ref64 dW slab %d' % slab, C.conv3d_dw(x, g, k, stride, slab=slab), dw, 1e-14)


@pytest.mark.parametrize('shape,cin,cout,k,stride', CASES, ids=IDS)
def test_ref64_forward_matches_the_oracle(shape, cin, cout, k, stride):
    B, D, H, W = shape
    rs = np.random.RandomState(cin + 5 * cout + k + stride)
    x = rs.standard_normal((B, cin, D, H, W)).astype(np.float32)
    w = (rs.standard_normal((cout, cin, k, k, k)) * 0.2).astype(np.float32)
    want = O.conv3d(x, w, stride=stride, pad=C.conv_pad(k))
    got = C.conv3d(cl(torch.from_numpy(x)), torch.from_numpy(w), stride)
    check_close('ref64 vs oracle k%d s%d %s' % (k, stride, shape), ncdhw(got).numpy(), want, 1e-6)


def test_ref64_does_not_accept_what_training_does_not_run():
    x = torch.zeros(1, 4, 4, 4, 8, dtype=torch.float64)
    with pytest.raises(AssertionError):
        C.conv3d(x, torch.zeros(8, 8, 2, 2, 2, dtype=torch.float64), 1)         # 2x2x2 is stride 2 only
    with pytest.raises(AssertionError):
        C.conv3d(x, torch.zeros(8, 7, 3, 3, 3, dtype=torch.float64), 1)         # channel mismatch
