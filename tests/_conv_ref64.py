"""A bias-free Conv3d restated in float64 torch -- the yardstick the training-side convolution kernels (csrc/pw_train.hip,
pw_train_h2.hip, pw_dgrad_s2_h2.hip, pw_conv3d_wino.hip behind preworld_amd/train.py) answer to at the training grid.

Channels-last tensors (B, D, H, W, C), torch's weight layout (Cout, Cin, k, k, k); padding k // 2 for k = 1 and 3, none for the
2x2x2 stride-2 convs of the trajectory branch; stride 1 or 2.  Every function is a sum over the k^3 taps of one GEMM each over a
shifted (stride 1) or strided (stride 2) slice of the padded tensor, so the peak stays near the size of the operands on any device
(F.conv3d in float64 falls back to im2col where MIOpen does not serve float64: ~9 GB per sample of the 200x200x16 grid at 64
channels).  `slab` bounds the peak further: the output depth planes are taken that many at a time.  Nothing here calls a project
kernel."""
import torch
import torch.nn.functional as F

_f64 = torch.float64


def conv_pad(k):
    return 0 if k == 2 else k // 2


def out_extent(n, k, stride):
    return (n + 2 * conv_pad(k) - k) // stride + 1


def _check(x, w, stride):
    k = w.shape[2]
    assert w.dim() == 5 and w.shape[2] == w.shape[3] == w.shape[4] and k in (1, 2, 3), tuple(w.shape)
    assert stride in (1, 2) and (k != 2 or stride == 2), (k, stride)
    assert x.dim() == 5 and x.shape[-1] == w.shape[1], (tuple(x.shape), tuple(w.shape))
    return k, conv_pad(k)


def _padded(x, p):
    x = x.to(_f64)
    return F.pad(x, (0, 0, p, p, p, p, p, p)) if p else x


def _taps(k):
    return [(a, b, c) for a in range(k) for b in range(k) for c in range(k)]


def _window(xp, a, b, c, d0, d1, Ho, Wo, s):
    """the input voxels tap (a, b, c) meets for the output planes d0 .. d1 - 1: (B, d1 - d0, Ho, Wo, C), a view of xp"""
    return xp[:, a + s * d0:a + s * (d1 - 1) + 1:s, b:b + s * (Ho - 1) + 1:s, c:c + s * (Wo - 1) + 1:s, :]


def _slabs(Do, slab):
    step = Do if not slab else max(1, int(slab))
    return [(d0, min(Do, d0 + step)) for d0 in range(0, Do, step)]


def conv3d(x, w, stride=1, slab=None):
    """y (B, Do, Ho, Wo, Cout) = conv3d(x (B, D, H, W, Cin), w (Cout, Cin, k, k, k)) in float64"""
    k, p = _check(x, w, stride)
    B, D, H, W, Cin = x.shape
    Cout = w.shape[0]
    Do, Ho, Wo = out_extent(D, k, stride), out_extent(H, k, stride), out_extent(W, k, stride)
    xp, w = _padded(x, p), w.to(device=x.device, dtype=_f64)
    y = torch.zeros(B, Do, Ho, Wo, Cout, dtype=_f64, device=x.device)
    for d0, d1 in _slabs(Do, slab):
        ys = y[:, d0:d1].reshape(-1, Cout)
        for a, b, c in _taps(k):
            win = _window(xp, a, b, c, d0, d1, Ho, Wo, stride).reshape(-1, Cin)
            ys.addmm_(win, w[:, :, a, b, c].t())
        y[:, d0:d1] = ys.view(B, d1 - d0, Ho, Wo, Cout)
    return y


def conv3d_dx(dy, w, x_shape, stride=1, slab=None):
    """d <dy, conv3d(x, w)> / d x: the adjoint, each tap's dy @ w scattered back onto the voxels it read, padding cropped"""
    B, D, H, W, Cin = x_shape
    k, p = _check(torch.empty((1, 1, 1, 1, Cin), device='meta'), w, stride)
    Do, Ho, Wo = out_extent(D, k, stride), out_extent(H, k, stride), out_extent(W, k, stride)
    Cout = w.shape[0]
    assert tuple(dy.shape) == (B, Do, Ho, Wo, Cout), (tuple(dy.shape), (B, Do, Ho, Wo, Cout))
    w = w.to(device=dy.device, dtype=_f64)
    dxp = torch.zeros(B, D + 2 * p, H + 2 * p, W + 2 * p, Cin, dtype=_f64, device=dy.device)
    for d0, d1 in _slabs(Do, slab):
        g = dy[:, d0:d1].to(_f64).reshape(-1, Cout)
        for a, b, c in _taps(k):
            _window(dxp, a, b, c, d0, d1, Ho, Wo, stride).add_((g @ w[:, :, a, b, c]).view(B, d1 - d0, Ho, Wo, Cin))
    return dxp[:, p:p + D, p:p + H, p:p + W].contiguous() if p else dxp


def conv3d_dw(x, dy, k, stride=1, slab=None):
    """d <dy, conv3d(x, w)> / d w (Cout, Cin, k, k, k): per tap dy^T @ the slice of x it read, summed over the voxels"""
    B, D, H, W, Cin = x.shape
    Cout = dy.shape[-1]
    _check(x, torch.empty((Cout, Cin, k, k, k), device='meta'), stride)
    p = conv_pad(k)
    Do, Ho, Wo = out_extent(D, k, stride), out_extent(H, k, stride), out_extent(W, k, stride)
    assert tuple(dy.shape) == (B, Do, Ho, Wo, Cout), (tuple(dy.shape), (B, Do, Ho, Wo, Cout))
    xp = _padded(x, p)
    dw = torch.zeros(Cout, Cin, k, k, k, dtype=_f64, device=x.device)
    for d0, d1 in _slabs(Do, slab):
        g = dy[:, d0:d1].to(_f64).reshape(-1, Cout).t()
        for a, b, c in _taps(k):
            dw[:, :, a, b, c] += g @ _window(xp, a, b, c, d0, d1, Ho, Wo, stride).reshape(-1, Cin)
    return dw
