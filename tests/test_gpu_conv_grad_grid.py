"""Every convolution of the voxel side's training step at the training batch, B = 2 on the 200x200x16 grid and the encoder's
coarser levels, against the float64 restatement of tests/_conv_ref64.py on the device: the forward y, the data gradient dX and
every weight gradient dW, each to 1e-5 of its largest reference entry (the per-layer bar of test_gpu_train's
test_conv3d_grads_vs_torch), and dX / dW bit-identical on a second pass.

Grids (D, H, W): G0 = (16, 200, 200), G1 = (8, 100, 100), G2 = (4, 50, 50), G3 = (2, 25, 25).  Each row drives the autograd
Function training uses (train.Conv3dCL, ConvPairCL, LinearRowsCL, linear_cl) with the real weight layouts -- the OccHead's and the
trajectory branch's permuted taps, the neck's slices of its 224-column weight -- and asserts which library entry points it reached
(a spy on train._lib.call), so that a change of dispatch (_use_wino, _pairable, _DGRAD_S2, _WGRAD) fails the row instead of
quietly testing another kernel.  At these sizes the size-chosen paths run that the small fixtures barely reach: 800 chunk
partials in k_wgrad_reduce (1x1x1 layers at G0), the unrolled main loop and the tail of k_wgrad_h2_reduce (256 / 224 / 48 chunks),
wg_plan's row splits and strips, the persistent Winograd tiles on flipped / transposed weights with the pair's `accumulate`
epilogue, the parity-class kernel on the pair's concatenated dY, pw_linear_rows over 1.28 M rows, and the sample boundary.

Operand regimes:
  normal  x, dY ~ N(0, 1);
  train   x >= 0 with about half zeros (post-ReLU); dY with random signs, magnitudes log-uniform over 2^-12 .. 1, times 2^-20 (the size
          of a loss gradient): the per-tensor power-of-two pre-scales of the split-fp16 kernels at full size;
  bn      (rows b and d) x from a BatchNormCL forward (ReLU), dY from BatchNormCL backwards fed the `train` draw: the maxima the
          BatchNorm kernels recorded feed the weight gradient (no pw_absmax2 pass), each one checked against a fresh pass
          (train._AMAX_CHECK)."""
import contextlib
import types

import pytest
import torch

import _conv_ref64 as R
from _parity import check_close
from preworld_amd import train

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
B = 2
G0, G1, G2, G3 = (16, 200, 200), (8, 100, 100), (4, 50, 50), (2, 25, 25)
REL = 1e-5                                        # max |err| <= REL * max |ref| for y, dX and every dW


# ------------------------------------------------------------------------------------------------- operands
def _x(gen, grid, C, regime):
    x = torch.randn((B,) + grid + (C,), generator=gen, device=DEV)
    return x.clamp_min_(0.0) if regime != 'normal' else x


def _dy(gen, shape, regime):
    if regime == 'normal':
        return torch.randn(shape, generator=gen, device=DEV)
    sign = torch.randint(0, 2, shape, generator=gen, device=DEV).float().mul_(2.0).sub_(1.0)
    mag = torch.exp2(torch.rand(shape, generator=gen, device=DEV) * -12.0)
    return sign * mag * 2.0 ** -20


def _w(gen, shape):
    fan_in = shape[1] * (shape[2] * shape[3] * shape[4] if len(shape) == 5 else 1)
    return (torch.randn(shape, generator=gen, device=DEV) / fan_in ** 0.5).requires_grad_(True)


# ------------------------------------------------------------------------------------------------- dispatch spy
@contextlib.contextmanager
def _spy():
    """every library entry point called inside, with the kernel it noted last (pw_last_kernel) and its arguments"""
    calls, real, lib = [], train._lib.call, train._lib.lib()

    def spy(name, *a):
        real(name, *a)
        calls.append((name, lib.pw_last_kernel().decode(), a))
    train._lib.call = spy
    try:
        yield calls
    finally:
        train._lib.call = real


def _names(calls, name):
    return [c for c in calls if c[0] == name]


# ------------------------------------------------------------------------------------------------- the rows
# A row: inputs [(grid, C)], parameters {name: shape}, convolutions [(input index, parameter, effective torch-layout weight of the
# parameter, stride)], and run(xs, ps) -> one output per convolution, through the Functions training uses.
def _perm(w):                                     # the (Z,Y,X) buffer convolved with the reference's (X,Y,Z) taps
    return w.permute(0, 1, 4, 3, 2)


def _ident(w):
    return w


def _lin(w):
    return w.reshape(w.shape[0], w.shape[1], 1, 1, 1)


def _single(stride=1):
    return lambda xs, ps: (train.Conv3dCL.apply(xs[0], ps['w'], stride),)


def _pair(stride):
    return lambda xs, ps: train.ConvPairCL.apply(xs[0], ps['w1'], ps['w2'], stride)


def _neck(xs, ps):                                # train.fpn_forward's three per-level slices of the 224-column weight
    w, c8, c16 = ps['w'], xs[0].shape[-1], xs[1].shape[-1]
    return (train.Conv3dCL.apply(xs[0], w[:, :c8], 1), train.Conv3dCL.apply(xs[1], w[:, c8:c8 + c16], 1),
            train.Conv3dCL.apply(xs[2], w[:, c8 + c16:], 1))


def _occ_conv(xs, ps):                            # train.occ_head_forward's first conv
    return (train.Conv3dCL.apply(xs[0], _perm(ps['w']).contiguous(), 1),)


def _occ_1x1(xs, ps):                             # occ_pred_conv's two bias-free 1x1x1 convs (train._conv1x1_cl)
    return tuple(train.LinearRowsCL.apply(x, ps[k].reshape(ps[k].shape[0], -1)) for x, k in zip(xs, ('w0', 'w1')))


def _downscale(xs, ps):                           # train.downscale_forward's three convs (bias in a separate pass)
    return tuple(train.Conv3dCL.apply(x, _perm(ps[k]).contiguous(), 2) for x, k in zip(xs, ('w1', 'w2', 'w3')))


def _attr_mlps(xs, ps):                           # train.linear_cl on the attribute MLPs' Linear layers (bias in a separate pass)
    return tuple(train.linear_cl(x, types.SimpleNamespace(weight=ps[k], bias=None))
                 for x, k in zip((xs[0], xs[1], xs[1], xs[1]), ('l0', 'd', 's', 'c')))


ROWS = {
    # pre_process / encoder conv2 / final_conv
    'a': dict(inputs=[(G0, 32)], params={'w': (32, 32, 3, 3, 3)}, convs=[(0, 'w', _ident, 1)], run=_single(),
              expect=[('pw_conv3d_wino', None, 2), ('pw_conv3d_wgrad_h2', 'k_conv3d_wgrad_h2<1, 1>', 1)],
              forbid=['pw_conv3d_ndhwc', 'pw_conv3d_wgrad']),
    # encoder layer 0: conv1 + downsample as one pair, 64 -> 32 + 32
    'b': dict(inputs=[(G0, 64)], params={'w1': (32, 64, 3, 3, 3), 'w2': (32, 64, 3, 3, 3)},
              convs=[(0, 'w1', _ident, 1), (0, 'w2', _ident, 1)], run=_pair(1),
              expect=[('pw_conv3d_wino', None, 3), ('pw_conv3d_wgrad_h2', 'k_conv3d_wgrad_h2<1, 2>', 2)],
              forbid=['pw_conv3d_ndhwc', 'pw_conv3d_wgrad']),
    # encoder layer 1 pair, stride 2: 32 -> 64 + 64
    'c': dict(inputs=[(G0, 32)], params={'w1': (64, 32, 3, 3, 3), 'w2': (64, 32, 3, 3, 3)},
              convs=[(0, 'w1', _ident, 2), (0, 'w2', _ident, 2)], run=_pair(2),
              expect=[('pw_conv3d_ndhwc', None, 1), ('pw_conv3d_dgrad_s2_h2', None, 1), ('pw_conv3d_wgrad', 'k_conv3d_wgrad', 2)],
              forbid=['pw_conv3d_wino', 'pw_conv3d_dgrad_s2', 'pw_conv3d_wgrad_h2']),
    # encoder layer 1 convs
    'd': dict(inputs=[(G1, 64)], params={'w': (64, 64, 3, 3, 3)}, convs=[(0, 'w', _ident, 1)], run=_single(),
              expect=[('pw_conv3d_wino', None, 2), ('pw_conv3d_wgrad_h2', 'k_conv3d_wgrad_h2<2, 2>', 1)],
              forbid=['pw_conv3d_ndhwc', 'pw_conv3d_wgrad']),
    # encoder layer 2 pair, stride 2: 64 -> 128 + 128
    'e': dict(inputs=[(G1, 64)], params={'w1': (128, 64, 3, 3, 3), 'w2': (128, 64, 3, 3, 3)},
              convs=[(0, 'w1', _ident, 2), (0, 'w2', _ident, 2)], run=_pair(2),
              expect=[('pw_conv3d_ndhwc', None, 1), ('pw_conv3d_dgrad_s2_h2', None, 1), ('pw_conv3d_wgrad', 'k_conv3d_wgrad', 2)],
              forbid=['pw_conv3d_wino', 'pw_conv3d_dgrad_s2', 'pw_conv3d_wgrad_h2']),
    # encoder layer 2 convs
    'f': dict(inputs=[(G2, 128)], params={'w': (128, 128, 3, 3, 3)}, convs=[(0, 'w', _ident, 1)], run=_single(),
              expect=[('pw_conv3d_wino', None, 2), ('pw_conv3d_wgrad_h2', 'k_conv3d_wgrad_h2<2, 2>', 1)],
              forbid=['pw_conv3d_ndhwc', 'pw_conv3d_wgrad']),
    # LSSFPN3D's 1x1x1 conv, per level
    'g': dict(inputs=[(G0, 32), (G1, 64), (G2, 128)], params={'w': (32, 224, 1, 1, 1)},
              convs=[(0, 'w', lambda w: w[:, :32], 1), (1, 'w', lambda w: w[:, 32:96], 1), (2, 'w', lambda w: w[:, 96:], 1)], run=_neck,
              expect=[('pw_conv3d_ndhwc', None, 6), ('pw_conv3d_wgrad', 'k_conv3d_wgrad', 3)],
              forbid=['pw_conv3d_wino', 'pw_conv3d_wgrad_h2']),
    # OccHead's 3x3x3 conv, 32 -> 16, transposed taps
    'h': dict(inputs=[(G0, 32)], params={'w': (16, 32, 3, 3, 3)}, convs=[(0, 'w', _perm, 1)], run=_occ_conv,
              expect=[('pw_conv3d_wino', None, 2), ('pw_conv3d_wgrad_h2', 'k_conv3d_wgrad_h2<1, 1>', 1)],
              forbid=['pw_conv3d_ndhwc', 'pw_conv3d_wgrad']),
    # OccHead's per-voxel 16 -> 8 -> 18
    'i': dict(inputs=[(G0, 16), (G0, 8)], params={'w0': (8, 16, 1, 1, 1), 'w1': (18, 8, 1, 1, 1)},
              convs=[(0, 'w0', _ident, 1), (1, 'w1', _ident, 1)], run=_occ_1x1,
              expect=[('pw_linear_rows', None, 4), ('pw_conv3d_wgrad', 'k_conv3d_wgrad', 2)],
              forbid=['pw_conv3d_ndhwc', 'pw_conv3d_wino']),
    # trajectory branch, DownScaleModule3DCustom: 2x2x2 stride 2, permuted taps
    'j': dict(inputs=[(G0, 32), (G1, 64), (G2, 128)],
              params={'w1': (64, 32, 2, 2, 2), 'w2': (128, 64, 2, 2, 2), 'w3': (128, 128, 2, 2, 2)},
              convs=[(0, 'w1', _perm, 2), (1, 'w2', _perm, 2), (2, 'w3', _perm, 2)], run=_downscale,
              expect=[('pw_conv3d_ndhwc', None, 3), ('pw_conv3d_dgrad_k2s2', 'k_conv3d_dgrad_k2s2', 3), ('pw_conv3d_wgrad', 'k_conv3d_wgrad', 3)],
              forbid=['pw_conv3d_wino', 'pw_conv3d_dgrad_s2', 'pw_conv3d_dgrad_s2_h2']),
    # attribute MLPs (pre-train): 32 -> 64, 64 -> {2, 17, 3}
    'k': dict(inputs=[(G0, 32), (G0, 64)], params={'l0': (64, 32), 'd': (2, 64), 's': (17, 64), 'c': (3, 64)},
              convs=[(0, 'l0', _lin, 1), (1, 'd', _lin, 1), (1, 's', _lin, 1), (1, 'c', _lin, 1)], run=_attr_mlps,
              expect=[('pw_conv3d_ndhwc', None, 8), ('pw_conv3d_wgrad', 'k_conv3d_wgrad', 4)],
              forbid=['pw_conv3d_wino', 'pw_linear_rows']),
}
CASES = [(r, g) for r in sorted(ROWS) for g in ('normal', 'train')] + [('b', 'bn'), ('d', 'bn')]


def _bn_params(gen, C):
    return torch.rand(C, generator=gen, device=DEV) + 0.5, torch.randn(C, generator=gen, device=DEV) * 0.1


def _train_pass(row, regime, seed):
    """one forward + backward through the training Functions -> (xs, dys, ys, dxs, grads, calls); xs / dys: the conv operands"""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    ps = {k: _w(gen, s) for k, s in row['params'].items()}
    xs, leaves = [], []
    for grid, C in row['inputs']:
        if regime == 'bn':
            src = torch.randn((B,) + grid + (C,), generator=gen, device=DEV).requires_grad_(True)
            x = train.BatchNormCL.apply(src, *_bn_params(gen, C), None, 1e-5, True)[0]
            x.retain_grad()
        else:
            x = _x(gen, grid, C, regime).requires_grad_(True)
        xs.append(x)
    checked0 = train._AMAX_STATS['checked']
    with _spy() as calls:
        ys = row['run'](xs, ps)
        assert len(ys) == len(row['convs'])
        if regime == 'bn':
            for y in ys:
                y.retain_grad()
            tops = [train.BatchNormCL.apply(y, *_bn_params(gen, y.shape[-1]), None, 1e-5, True)[0] for y in ys]
            torch.autograd.backward(tops, [_dy(gen, tuple(t.shape), 'train') for t in tops])
            dys = [y.grad for y in ys]
        else:
            dys = [_dy(gen, tuple(y.shape), regime) for y in ys]
            torch.autograd.backward(list(ys), dys)
    grads = {k: p.grad for k, p in ps.items()}
    n_checked = train._AMAX_STATS['checked'] - checked0
    return ([x.detach() for x in xs], [d.detach() for d in dys], [y.detach() for y in ys], [x.grad for x in xs], grads,
            {k: p.detach() for k, p in ps.items()}, calls, n_checked)


def _reference(row, xs, dys, ps):
    """float64: y per conv, dX per input (summed over the convs that read it), dW per parameter (through the parameter's
    slice / permutation / reshape by float64 autograd)"""
    ys, dxs = [], [None] * len(xs)
    p64 = {k: p.double().requires_grad_(True) for k, p in ps.items()}
    effs, dws = [], []
    for (i, k, eff, s), dy in zip(row['convs'], dys):
        w = eff(p64[k])
        ys.append(R.conv3d(xs[i], w.detach(), s))
        dx = R.conv3d_dx(dy, w.detach(), tuple(xs[i].shape), s)
        dxs[i] = dx if dxs[i] is None else dxs[i] + dx
        effs.append(w)
        dws.append(R.conv3d_dw(xs[i], dy, w.shape[2], s))
    torch.autograd.backward(effs, dws)
    return ys, dxs, {k: p.grad for k, p in p64.items()}


@pytest.mark.parametrize('row,regime', CASES, ids=['%s-%s' % c for c in CASES])
def test_conv_grads_at_the_training_grid_vs_float64(row, regime):
    spec = ROWS[row]
    seed = 1000 + ord(row) * 7 + ('normal', 'train', 'bn').index(regime)
    old = train._AMAX_CHECK
    train._AMAX_CHECK = True
    try:
        xs, dys, ys, dxs, grads, ps, calls, n_checked = _train_pass(spec, regime, seed)
        xs2, dys2, ys2, dxs2, grads2, _, _, _ = _train_pass(spec, regime, seed)
    finally:
        train._AMAX_CHECK = old
    # the kernels this row is meant to reach
    for name, kernel, n in spec['expect']:
        got = _names(calls, name)
        assert len(got) == n, (row, name, len(got), [c[:2] for c in calls])
        assert kernel is None or all(c[1] == kernel for c in got), (row, name, kernel, [c[1] for c in got])
    for name in spec['forbid']:
        assert not _names(calls, name), (row, name, [c[:2] for c in calls])
    if row in ('b',):                                     # the Winograd data gradient of w1 is the accumulate operand of w2's
        assert sum(c[2][4] is not None for c in _names(calls, 'pw_conv3d_wino')) == 1, row
    if row in ('c', 'e'):                                 # the parity-class kernel on the concatenated dY of the pair
        assert [c[2][11] for c in _names(calls, 'pw_conv3d_dgrad_s2_h2')] == [2 * spec['params']['w1'][0]], row
    absmax = _names(calls, 'pw_absmax2')
    if regime == 'bn':                                    # every maximum was recorded by a BatchNorm kernel; each one was checked
        assert n_checked > 0 and len(absmax) == n_checked, (row, n_checked, len(absmax))
    elif row == 'b':                                      # one pass over x serves both weight gradients
        assert sum(c[2][1] > 0 for c in absmax) == 1, (row, [c[2][1] for c in absmax])
    # float64 reference on the device
    rys, rdxs, rdws = _reference(spec, xs, dys, ps)
    tag = '%s %s' % (row, regime)
    for i, (y, r) in enumerate(zip(ys, rys)):
        check_close('%s y%d %s' % (tag, i, tuple(r.shape[1:])), y, r, REL)
    for i, (dx, r) in enumerate(zip(dxs, rdxs)):
        check_close('%s dX%d %s' % (tag, i, tuple(r.shape[1:])), dx, r, REL)
    for k, r in rdws.items():
        check_close('%s dW %s %s' % (tag, k, tuple(r.shape)), grads[k], r, REL)
    # deterministic: the same operands give the same bits
    for a, b in zip(xs + dys + ys + dxs, xs2 + dys2 + ys2 + dxs2):
        assert torch.equal(a, b), row
    for k in grads:
        assert torch.equal(grads[k], grads2[k]), (row, k)
