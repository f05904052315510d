"""The inference convolutions restated in float64 torch -- the yardstick pw_conv3d_h2 (tiled, gather and stride-2 kernels),
pw_occ_head_h2, pw_fpn3d_fuse and the fp32 kernels behind PW_PRECISION=f32 answer to on every kernel path.

Built on tests/_conv_ref64.conv3d; nothing here calls a project kernel, and the h2 storage format is decoded by this file's own
reading of the slot formula in csrc/pw_h2.h (h2_decode), so the library's h2_to_f32 is not its own judge.

THE UNIT.  Every operation returns its value and a per-element normaliser
    n = conv3d(|x|, |w|) * |scale| + |bias| + |residual|
(propagated through OccHead's two 1x1 layers with |w|).  The unit of error at an element is u = 2^-24 * n and every comparison is
q = |got - ref| / u per element: a column whose folded BatchNorm scale is 2^-10 of the largest, or a corner voxel where 8 taps meet
instead of 27, is judged on its own magnitude, not on the tensor's largest.

THE OPERANDS are exactly representable in BOTH fp32 and split-fp16: activations are drawn in fp32 and replaced by (hi + lo) * 2^e
of their own split (quant_x), weights by (hi + lo) / S of the packers' per-column power-of-two pre-scale (quant_w).  Kernels and
reference then see the same numbers, the same rows serve the fp32 kernels, and what is measured is the arithmetic alone.

THE BOUND.  Per row, max q <= 2 * Q32[row] + 1: Q32 is the same operation done with torch float32 ops on the same operands, scored
in the same units on the CPU (test_infer_ref64_cpu.py measures and asserts the table); two correct float32 summation orders differ
by about that.  An h2 output adds the storage term of test_h2_round_trip_and_slices, 2^-21 |y| + 2^-37 amax.  Rows whose path
exceeds this for a reason that lies in the format carry an a-priori term in FORMAT_TERM (derivations: profiles/infer_conv_pin.md).
"""
import collections
import functools
import math

import numpy as np
import torch

import _conv_ref64 as C64

U = 2.0 ** -24
_f64 = torch.float64


# ------------------------------------------------------------------------------------------------ the h2 layout, restated
# csrc/pw_h2.h: every 32-channel chunk of a voxel is 128 bytes = 8 slots of 16 bytes; slot(half, ks, p) = 4 half + 2 ks + p holds
# plane p (0 = hi, 1 = lo) of channels 16 ks + 8 half + 0..7 as eight fp16.  In units of fp16 inside the chunk:
def _plane_index(p):
    c = np.arange(32)
    half, ks = (c >> 3) & 1, c >> 4
    return (4 * half + 2 * ks + p) * 8 + (c & 7)


HI_IDX, LO_IDX = _plane_index(0), _plane_index(1)


def ideal_exp(amax):
    """the exponent that puts the largest magnitude in [2^12, 2^13) stored units (pw_h2.h "Range"); 0 for zero / non-finite"""
    if not (amax > 0.0) or math.isinf(amax) or math.isnan(amax):
        return 0
    return max(-100, min(100, math.frexp(float(amax))[1] - 1 - 12))


def h2_decode(buf, e):
    """float32-typed array (.., C) holding h2 bytes, exponent e -> float64 numpy (hi + lo) * 2^e of the same shape"""
    buf = np.ascontiguousarray(buf, dtype=np.float32)
    C = buf.shape[-1]
    assert C % 32 == 0, C
    h = buf.view(np.float16).reshape(buf.shape[:-1] + (C // 32, 64)).astype(np.float64)
    v = (h[..., HI_IDX] + h[..., LO_IDX]) * 2.0 ** int(e)
    return v.reshape(buf.shape)


def h2_encode(x, e):
    """fp32 array (.., C) -> float32-typed array of the same shape holding the split of x / 2^e (hi = fp16(s), lo = fp16(s - hi))"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    C = x.shape[-1]
    assert C % 32 == 0, C
    s = x.astype(np.float64) * 2.0 ** -int(e)
    hi = s.astype(np.float16)
    lo = (s - hi.astype(np.float64)).astype(np.float16)
    out = np.zeros(x.shape[:-1] + (C // 32, 64), np.float16)
    out[..., HI_IDX] = hi.reshape(x.shape[:-1] + (C // 32, 32))
    out[..., LO_IDX] = lo.reshape(x.shape[:-1] + (C // 32, 32))
    return out.reshape(x.shape[:-1] + (2 * C,)).view(np.float32).reshape(x.shape)


def quant_x(x, e=None):
    """-> (xq fp32 exactly equal to its own h2 encoding under e, the encoded float32-typed buffer, e)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if e is None:
        e = ideal_exp(float(np.abs(x).max()))
    buf = h2_encode(x, e)
    xq = h2_decode(buf, e)
    assert (xq.astype(np.float32).astype(np.float64) == xq).all()
    return xq.astype(np.float32), buf, e


def quant_w(w, per_column=True):
    """weight (Cout, ...) -> fp32 weight that the split-fp16 packers (ops.pack_conv_weight_h2, pack_occ_weight_h2: one power of two
    per output column; pack_occ_tail_h2: one per matrix) represent exactly: (hi + lo) / S with max |S w| in [512, 1024)"""
    w = np.asarray(w, np.float32).astype(np.float64)            # an fp32 weight first: hi + lo of its split then fits fp32 again
    f = w.reshape(w.shape[0], -1)
    amax = np.maximum(np.abs(f).max(1, keepdims=True) if per_column else np.abs(f).max(), 1e-30)
    S = np.exp2(np.floor(np.log2(1023.0 / amax)))
    s = f * S
    hi = s.astype(np.float16).astype(np.float64)
    lo = (s - hi).astype(np.float16).astype(np.float64)
    q = ((hi + lo) / S).reshape(w.shape)
    assert (q.astype(np.float32).astype(np.float64) == q).all()
    return q.astype(np.float32)


# ------------------------------------------------------------------------------------------------ the operations
class one_thread:
    """torch's float32 conv and GEMM pick their blocking by the thread count: the float32 restatements run on one thread, so that
    the floor table is the same measurement wherever the suite runs"""

    def __enter__(self):
        self.n = torch.get_num_threads()
        torch.set_num_threads(1)

    def __exit__(self, *exc):
        torch.set_num_threads(self.n)


def _t(a):
    return a.detach().cpu().to(_f64) if torch.is_tensor(a) else torch.from_numpy(np.asarray(a, np.float64))


def conv_bn_act(x, w, scale=None, bias=None, residual=None, relu=False, stride=1, core=None):
    """x (B, D, H, W, Cin), w (Cout, Cin, k, k, k), scale / bias (Cout,), residual like the output -> (value, n), float64 torch.
    core: an already computed (conv3d(x, w), conv3d(|x|, |w|)) pair."""
    if core is None:
        x, w = _t(x), _t(w)
        core = C64.conv3d(x, w, stride), C64.conv3d(x.abs(), w.abs(), stride)
    c, a = core
    if scale is not None:
        c, a = c * _t(scale), a * _t(scale).abs()
    if bias is not None:
        c, a = c + _t(bias), a + _t(bias).abs()
    if residual is not None:
        c, a = c + _t(residual), a + _t(residual).abs()
    return (torch.relu(c) if relu else c), a


OccRef = collections.namedtuple('OccRef', 'logits n occ geo margin dead')


def occ_head(x, w0, s0, b0, w1, s1, b1, w2, empty_idx=17, dtype=_f64):
    """OccHead: conv3x3x3 32 -> 16, BN, ReLU, 16 -> 8, BN, ReLU, 8 -> 18.  x (B, D, H, W, 32) -> OccRef: logits and their
    normaliser (B, D, H, W, 18), first-maximum argmax and geo (uint8), the top-2 margin per voxel, and the voxels whose hidden
    layer is entirely clamped.  dtype=torch.float32 is the float32 restatement of the same chain."""
    cv = lambda a: torch.as_tensor(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a)).to(dtype)
    x, w0, s0, b0, w1, s1, b1, w2 = [cv(a) for a in (x, w0, s0, b0, w1, s1, b1, w2)]
    if dtype == _f64:
        c, a = C64.conv3d(x, w0), C64.conv3d(x.abs(), w0.abs())
    else:
        c = torch.nn.functional.conv3d(x.permute(0, 4, 1, 2, 3), w0, padding=1).permute(0, 2, 3, 4, 1)
        a = torch.zeros_like(c)
    mid, n_mid = torch.relu(c * s0 + b0), a * s0.abs() + b0.abs()
    hid, n_hid = torch.relu(mid @ w1.t() * s1 + b1), n_mid @ w1.abs().t() * s1.abs() + b1.abs()
    logits, n = hid @ w2.t(), n_hid @ w2.abs().t()
    occ = np.argmax(logits.numpy(), -1).astype(np.uint8)                # numpy: the first maximum
    geo = np.where(occ != empty_idx, 0, empty_idx).astype(np.uint8)
    top = torch.topk(logits, 2, -1).values
    return OccRef(logits, n, occ, geo, top[..., 0] - top[..., 1], (hid == 0).all(-1))


def _lerp_axis(y, n_out, axis):
    """linear interpolation along one axis with align_corners=True: out[i] reads src = i * (n_in - 1) / (n_out - 1)"""
    n_in = y.shape[axis]
    if n_in == n_out:
        return y
    src = torch.arange(n_out, dtype=_f64) * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
    i0 = src.floor().clamp(0, n_in - 1).long()
    i1 = (i0 + 1).clamp(max=n_in - 1)
    f = (src - i0.to(_f64)).view([-1 if d == axis else 1 for d in range(y.dim())])
    return y.index_select(axis, i0) * (1.0 - f) + y.index_select(axis, i1) * f


def upsample(y, size):
    """channels-last (B, d, h, w, C) float64 -> (B, D, H, W, C): trilinear, align_corners=True (what LSSFPN3D uses)"""
    for axis, n in zip((1, 2, 3), size):
        y = _lerp_axis(y, n, axis)
    return y


def neck(x8, w8, y16, y32, scale, bias, relu=True, w16=None, w32=None):
    """ReLU(BN(W8 x8 + up2(y16) + up4(y32))) -> (value, n).  x8 (B, D, H, W, C8), w8 (32, C8[, 1, 1, 1]); y16 / y32 are the
    lateral outputs (.., 32) on the coarse grids, or -- with w16 / w32 -- the coarse features the 1x1 laterals are applied to here,
    in float64."""
    x8, y16, y32 = _t(x8), _t(y16), _t(y32)
    lat = lambda x, w: (x @ _t(w).reshape(w.shape[0], -1).t(), x.abs() @ _t(w).reshape(w.shape[0], -1).abs().t())
    size = x8.shape[1:4]
    v, n = lat(x8, w8)
    for y, w in ((y16, w16), (y32, w32)):
        yv, yn = lat(y, w) if w is not None else (y, y.abs())
        v, n = v + upsample(yv, size), n + upsample(yn, size)
    v, n = v * _t(scale) + _t(bias), n * _t(scale).abs() + _t(bias).abs()
    return (torch.relu(v) if relu else v), n


def q_of(got, ref, n, storage=None):
    """per-element q = max(|got - ref| - storage, 0) / (2^-24 n); an element with n == 0 must be reproduced exactly"""
    got, ref, n = _t(got), _t(ref), _t(n)
    assert tuple(got.shape) == tuple(ref.shape), (tuple(got.shape), tuple(ref.shape))
    err = (got - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float('inf')), err)
    if storage is not None:
        err = (err - storage).clamp_min(0.0)
    return torch.where(n > 0, err / (U * n.clamp_min(1e-300)), torch.where(err > 0, torch.full_like(err, float('inf')), err))


def storage_term(ref):
    """what storing a tensor in h2 under its ideal exponent may add per element (test_h2_round_trip_and_slices)"""
    ref = _t(ref)
    return ref.abs() * 2.0 ** -21 + float(ref.abs().max()) * 2.0 ** -37


# ------------------------------------------------------------------------------------------------ dispatch thresholds, restated
BD, BH, BW = 4, 8, 8                       # the 4 x 8 x 8 output tile of the stride-1 kernels (pw_conv3d_common.h)
S2_TILE = (2, 4, 8)                        # the stride-2 tiled kernel's output tile (pw_conv3d_h2_s2.hip)
CUS = 256                                  # the table below is laid out for this CU count


def cdiv(a, b):
    return -(-a // b)


def n_tiles(B, D, H, W, tile=(BD, BH, BW)):
    return B * cdiv(D, tile[0]) * cdiv(H, tile[1]) * cdiv(W, tile[2])


def out_grid(o):
    return tuple(C64.out_extent(v, o['k'], o['stride']) for v in (o['D'], o['H'], o['W']))


def h2_nt(nblk, ntiles, cus=CUS):
    """pw_conv3d_h2: two N-tiles per wave when that still leaves every CU two or more work items"""
    return 2 if ntiles % 2 == 0 and nblk * (ntiles // 2) >= 2 * cus else 1


def gather_mt(n_out, ngroups):
    """split-fp16 3x3x3 stride-2 gather: two voxel tiles per wave while the launch has few blocks"""
    return 2 if cdiv(n_out, 128) * ngroups < 512 else 1


def f32_nt(nblk, ntiles):
    """pw_conv3d_ndhwc, 3x3x3 stride 1 tiled: NT = 2 only when it fills 512 resident slots"""
    return 2 if ntiles % 2 == 0 and nblk * (ntiles // 2) >= 512 else 1


def wino_ng(nblk, cout_total, cus=CUS):
    return 2 if cout_total % 64 == 0 and nblk * (cout_total // 64) >= 2 * (cus // 8 * 8) else 1


def nt2_batch(cus=CUS):
    """samples of the (13, 29, 31) grid (64 tiles) at 256 output columns that reach NT = 2: nblk * 4 >= 2 * CUs"""
    return cdiv(2 * cus, 64 * 4)


# ------------------------------------------------------------------------------------------------ operand sets
# regime: 'normal' N(0, 1); 'relu' non-negative, about half zeros; 'wide' |x| log-uniform over 2^-14 .. 1 with folded BN scales
# 2^k, k in -10 .. 2 per column (the per-tensor metric is blind to this one)
def _opset(B, grid, cin, cout, k=3, stride=1, regime='normal', seed=0):
    return dict(B=B, D=grid[0], H=grid[1], W=grid[2], cin=cin, cout=cout, k=k, stride=stride, regime=regime, seed=seed)


G_BIG = (13, 29, 31)                       # 4 x 4 x 4 = 64 tiles per sample, cut in every axis
OPSETS = collections.OrderedDict()
OPSETS['A'] = _opset(nt2_batch(), G_BIG, 32, 256, regime='normal', seed=101)       # NT = 2 at its smallest grid
OPSETS['B'] = _opset(2, (5, 11, 13), 64, 96, regime='relu', seed=102)              # NT = 1, not resident, odd tile count
OPSETS['C'] = _opset(1, G_BIG, 32, 32, regime='wide', seed=103)                    # resident, 64 items on 256 blocks
OPSETS['D'] = _opset(5, G_BIG, 32, 32, regime='normal', seed=104)                  # resident, 320 items: one and two trips
OPSETS['G1'] = _opset(2, (5, 11, 13), 64, 32, k=1, regime='normal', seed=111)      # the neck's laterals
OPSETS['G2'] = _opset(1, (4, 6, 10), 128, 32, k=1, regime='wide', seed=112)
OPSETS['G3'] = _opset(2, (5, 11, 13), 32, 64, regime='relu', seed=113)
OPSETS['G4'] = _opset(1, (4, 6, 10), 128, 64, regime='normal', seed=114)
OPSETS['G5'] = _opset(2, (7, 11, 13), 32, 32, stride=2, regime='normal', seed=115)
OPSETS['G6'] = _opset(2, (7, 11, 13), 32, 64, stride=2, regime='wide', seed=116)
OPSETS['G7'] = _opset(2, (7, 11, 13), 32, 96, stride=2, regime='relu', seed=117)
OPSETS['G8'] = _opset(1, (27, 79, 81), 32, 96, stride=2, regime='normal', seed=118)  # 22 960 outputs: MT = 1
OPSETS['T1'] = _opset(2, (5, 11, 13), 32, 128, stride=2, regime='normal', seed=121)  # 8 tiles of 2 x 4 x 8
OPSETS['T2'] = _opset(3, (9, 17, 13), 64, 256, stride=2, regime='relu', seed=122)    # 27 tiles
OPSETS['T3'] = _opset(2, (5, 11, 13), 32, 128, stride=2, regime='wide', seed=123)
OPSETS['K2'] = _opset(2, (6, 10, 9), 32, 64, k=2, stride=2, regime='normal', seed=131)  # the trajectory branch's 2x2x2 convs


def _draw_x(rs, shape, regime):
    if regime == 'normal':
        return rs.standard_normal(shape)
    if regime == 'relu':
        return np.maximum(rs.standard_normal(shape), 0.0)
    assert regime == 'wide', regime
    return np.exp2(rs.uniform(-14.0, 0.0, shape)) * rs.choice([-1.0, 1.0], shape)


def _draw_scale_bias(rs, cout, regime):
    if regime == 'wide':
        scale = np.exp2(rs.randint(-10, 3, cout).astype(np.float64))
        return scale.astype(np.float32), (scale * 0.05 * rs.standard_normal(cout)).astype(np.float32)
    return rs.uniform(0.5, 1.5, cout).astype(np.float32), rs.standard_normal(cout).astype(np.float32)


Operands = collections.namedtuple('Operands', 'x xbuf ex w scale bias res conv64 abs64 conv32')


@functools.lru_cache(maxsize=None)
def operands(name):
    """the operand set's tensors and the three convolutions every row on it shares (float64, float64 of the magnitudes, and
    torch's float32 conv); treat as read-only.  res: an unquantised residual draw (B, Do, Ho, Wo, cout) the rows quantise."""
    o = OPSETS[name]
    rs = np.random.RandomState(o['seed'])
    x, xbuf, ex = quant_x(_draw_x(rs, (o['B'], o['D'], o['H'], o['W'], o['cin']), o['regime']).astype(np.float32))
    k = o['k']
    w = quant_w(rs.standard_normal((o['cout'], o['cin'], k, k, k)) * np.sqrt(2.0 / (o['cin'] * k ** 3)))
    scale, bias = _draw_scale_bias(rs, o['cout'], o['regime'])
    res = rs.standard_normal((o['B'],) + out_grid(o) + (o['cout'],))
    res = (res * (scale if o['regime'] == 'wide' else 1.0) * (0.3 if o['regime'] == 'wide' else 1.0)).astype(np.float32)
    xt, wt = torch.from_numpy(x), torch.from_numpy(w)
    c64, a64 = C64.conv3d(xt, wt, o['stride']), C64.conv3d(xt.abs(), wt.abs(), o['stride'])
    with one_thread():
        c32 = torch.nn.functional.conv3d(xt.permute(0, 4, 1, 2, 3), wt, stride=o['stride'], padding=C64.conv_pad(k)).permute(0, 2, 3, 4, 1)
    return Operands(x, xbuf, ex, w, scale, bias, res, c64, a64, c32.contiguous())


# ------------------------------------------------------------------------------------------------ the conv rows
# api: 'h2' ops.conv3d_h2, 'f32' ops.conv3d_ndhwc, 'wino' ops.conv3d_wino.  fmt: storage of (y0, y1), 1 = h2.  res: None, 'h2',
# 'f32'.  inplace: also run with out0 as the residual (BasicBlock3D's form); the two must be bit-equal.  zero_bias: bias 0, for
# the scaling-invariance check.  checks: 'slice' (destination = a channel slice of a NaN-filled buffer), 'scale' (2^+-20 x).
def _row(ops_, kernel, api='h2', cout1=0, fmt=(1, 1), res=None, inplace=False, relu=(True, False), algo=0, zero_bias=False,
         checks=(), family='k_conv3d_h2'):
    return dict(kind='conv', ops=ops_, kernel=kernel, api=api, cout1=cout1, fmt=tuple(fmt), res=res, inplace=inplace,
                relu=tuple(relu), algo=algo, zero_bias=zero_bias, checks=tuple(checks), family=family)


H2 = 'k_conv3d_h2<%d, %d, %s>'
GA = 'k_conv3d_gather<%d, %d, %d, %d, %d, true, %s>'
ROWS = collections.OrderedDict()
# k_conv3d_h2: all eleven instantiations.  EPI 1 h2 outputs without a residual; 2 one h2 output + h2 residual; 3 fp32 outputs
# without a residual; 0 everything else (the (h2, fp32) pair, an fp32 residual into an h2 output)
for _s, _nt, _c1 in (('A', 2, 128), ('B', 1, 32)):
    ROWS['h2_%s_epi1_pair' % _s] = _row(_s, H2 % (_nt, 1, 'false'), cout1=_c1, checks=('slice',) if _s == 'B' else ())
    ROWS['h2_%s_epi2_res' % _s] = _row(_s, H2 % (_nt, 2, 'false'), res='h2', inplace=True)
    ROWS['h2_%s_epi3_f32' % _s] = _row(_s, H2 % (_nt, 3, 'false'), fmt=(0, 0), relu=(False, False))
    ROWS['h2_%s_epi0_pair' % _s] = _row(_s, H2 % (_nt, 0, 'false'), cout1=_c1, fmt=(1, 0))
    ROWS['h2_%s_epi0_res32' % _s] = _row(_s, H2 % (_nt, 0, 'false'), res='f32')
for _s in ('C', 'D'):
    ROWS['h2_%s_wr_epi1' % _s] = _row(_s, H2 % (1, 1, 'true'))
    ROWS['h2_%s_wr_epi2' % _s] = _row(_s, H2 % (1, 2, 'true'), res='h2', inplace=True)
    ROWS['h2_%s_wr_epi3' % _s] = _row(_s, H2 % (1, 3, 'true'), fmt=(0, 0), relu=(False, False), zero_bias=True, checks=('scale',))
ROWS['h2_C_epi0_res32'] = _row('C', H2 % (1, 0, 'false'), res='f32')                 # one 32 -> 32 tile, but EPI 0 is not resident
# split-fp16 gather: <NT, ksize, stride, MT, ksplit, true, h2 epilogue>
_g = dict(family='k_conv3d_gather(f16)')
ROWS['ga_k1_64'] = _row('G1', GA % (1, 1, 1, 1, 1, 'false'), fmt=(0, 0), relu=(False, False), **_g)
ROWS['ga_k1_128'] = _row('G2', GA % (1, 1, 1, 1, 1, 'false'), fmt=(0, 0), relu=(False, False), **_g)
ROWS['ga_k3_algo2'] = _row('G3', GA % (2, 3, 1, 1, 1, 'true'), algo=2, checks=('slice',), **_g)
ROWS['ga_k3_algo3_ks2'] = _row('B', GA % (1, 3, 1, 1, 2, 'false'), algo=3, fmt=(0, 0), res='f32', **_g)
ROWS['ga_k3_algo3_ks4'] = _row('G4', GA % (2, 3, 1, 1, 4, 'true'), algo=3, **_g)
ROWS['ga_s2_32_h2'] = _row('G5', GA % (1, 3, 2, 2, 1, 'true'), **_g)
ROWS['ga_s2_64_f32'] = _row('G6', GA % (2, 3, 2, 2, 1, 'false'), fmt=(0, 0), relu=(False, False), zero_bias=True, checks=('scale',), **_g)
ROWS['ga_s2_64_h2'] = _row('G6', GA % (2, 3, 2, 2, 1, 'true'), **_g)
ROWS['ga_s2_96_f32'] = _row('G7', GA % (1, 3, 2, 2, 1, 'false'), fmt=(0, 0), **_g)
ROWS['ga_s2_96_mt1'] = _row('G8', GA % (1, 3, 2, 1, 1, 'true'), **_g)
# LDS-tiled stride 2 in the conv1 + downsample form: 128 and 256 packed columns
_t2 = dict(family='k_conv3d_h2_s2')
ROWS['s2_128'] = _row('T1', 'k_conv3d_h2_s2<1>', cout1=64, checks=('slice',), **_t2)
ROWS['s2_256'] = _row('T2', 'k_conv3d_h2_s2<2>', cout1=128, **_t2)
ROWS['s2_128_wide'] = _row('T3', 'k_conv3d_h2_s2<1>', cout1=64, **_t2)
# the fp32 kernels under PW_PRECISION=f32
_f = dict(api='f32', fmt=(0, 0), family='fp32')
ROWS['f32_tiled_nt2'] = _row('A', 'k_conv3d_k3s1<2, 1>', algo=1, res='f32', **_f)
ROWS['f32_tiled_nt1'] = _row('C', 'k_conv3d_k3s1<1, 1>', algo=1, checks=('slice',), **_f)
ROWS['f32_pipe_nt2'] = _row('A', 'k_conv3d_k3s1_pipe<2>', algo=4, **_f)
ROWS['f32_pipe_nt1'] = _row('D', 'k_conv3d_k3s1_pipe<1>', algo=4, relu=(False, False), zero_bias=True, checks=('scale',), **_f)
ROWS['f32_pipe_relu'] = _row('G3', 'k_conv3d_k3s1_pipe<1>', algo=4, res='f32', **_f)
ROWS['f32_gather_k2s2'] = _row('K2', 'k_conv3d_gather<2, 2, 2, 1, 1>', relu=(False, False), **_f)
_w = dict(api='wino', fmt=(0, 0), family='fp32')
ROWS['f32_wino_ng2'] = _row('A', 'k_conv3d_wino_ws<2>', res='f32', **_w)
ROWS['f32_wino_ng1'] = _row('C', 'k_conv3d_wino_ws<1>', **_w)

# instantiations no row reaches, and why (profiles/infer_conv_pin.md repeats this list)
UNREACHED = {
    'k_conv3d_gather<2, 3, 2, 1, *, true, *>': 'stride 2 with MT = 1 needs cdiv(n_out, 128) * groups >= 512; at an even tile count the '
    'tiled kernel declines (64 outputs) that is 32 768 output voxels from a 33 MB input -- the NT = 1 form is pinned at 96 outputs',
    'k_conv3d_gather<2, 1, 1, 1, *, true, *> and the channel-split 1x1x1 forms': 'no caller in the model: the laterals are 64 -> 32 '
    'and 128 -> 32 without a channel split',
}


def row_split(name):
    r = ROWS[name]
    o = OPSETS[r['ops']]
    return o['cout'] - r['cout1'], r['cout1']


ConvRef = collections.namedtuple('ConvRef', 'y n y32 bias res resbuf e')
# y / n / y32: tuples over (y0, y1) -- float64 value, normaliser, and the float32 restatement; bias: the fp32 bias the kernels get;
# res: the quantised fp32 residual (or None) with its h2 encoding resbuf; e: exponents of (y0, y1) for h2 destinations


@functools.lru_cache(maxsize=None)
def conv_ref(name):
    r = ROWS[name]
    o, P = OPSETS[r['ops']], operands(r['ops'])
    c0, c1 = row_split(name)
    bias = np.zeros_like(P.bias) if r['zero_bias'] else P.bias
    sc, bi = torch.from_numpy(P.scale), torch.from_numpy(bias)

    def parts(res):
        ys, ns, y32 = [], [], []
        for lo, hi, relu, rr in ((0, c0, r['relu'][0], res), (c0, c0 + c1, r['relu'][1], None)):
            if hi == lo:
                continue
            y, n = conv_bn_act(None, None, sc[lo:hi], bi[lo:hi], rr, relu, core=(P.conv64[..., lo:hi], P.abs64[..., lo:hi]))
            f = P.conv32[..., lo:hi] * sc[lo:hi] + bi[lo:hi]
            if rr is not None:
                f = f + torch.from_numpy(rr)
            ys.append(y); ns.append(n); y32.append(torch.relu(f) if relu else f)
        return tuple(ys), tuple(ns), tuple(y32)

    res = resbuf = None
    if r['res'] is not None:
        res = np.ascontiguousarray(P.res[..., :c0])
        if r['res'] == 'h2':
            # the residual shares y0's range slot when the conv adds onto it in place: encode it under y0's exponent (two passes:
            # the exponent follows the reference's largest magnitude, which the quantised residual is part of)
            e = ideal_exp(float(parts(res)[0][0].abs().max()))
            for _ in range(2):
                rq, resbuf, _e = quant_x(np.ascontiguousarray(P.res[..., :c0]), e)
                e = ideal_exp(float(parts(rq)[0][0].abs().max()))
            res = rq
    ys, ns, y32 = parts(res)
    e = tuple(ideal_exp(float(y.abs().max())) for y in ys)
    return ConvRef(ys, ns, y32, bias, res, resbuf, e)


def conv_q32(name):
    """max and mean q of the float32 restatement over the row's outputs"""
    ref = conv_ref(name)
    qs = torch.cat([q_of(a, b, n).reshape(-1) for a, b, n in zip(ref.y32, ref.y, ref.n)])
    return float(qs.max()), float(qs.mean())


# ------------------------------------------------------------------------------------------------ the OccHead rows
def _occ(shape, kernel, regime='normal', strided=False, api='h2', family='k_occ_head_h2'):
    return dict(kind='occ', shape=shape, kernel=kernel, regime=regime, strided=strided, api=api, family=family)


for _shape, _reg in (((2, 5, 19, 27), 'relu'), ((3, 2, 9, 7), 'normal'), ((1, 4, 8, 8), 'wide')):
    _n = 'x'.join(str(v) for v in _shape)
    ROWS['occ_%s_logits' % _n] = _occ(_shape, 'k_occ_head_h2<true>', _reg)
    ROWS['occ_%s_strided' % _n] = _occ(_shape, 'k_occ_head_h2<false>', _reg, strided=True)
ROWS['occ_f32_direct'] = _occ((2, 5, 19, 27), 'k_occ_head16<1>', api='f32', family='fp32')
ROWS['occ_f32_wino'] = _occ((2, 5, 19, 27), 'k_occ_head_wino', api='wino', family='fp32')

OccOperands = collections.namedtuple('OccOperands', 'x xbuf ex w0 s0 b0 w1 s1 b1 w2')


@functools.lru_cache(maxsize=None)
def occ_operands(shape, regime):
    """the draw order and seed of test_occ_head_h2_matches_direct_and_oracle, then quantised"""
    rs = np.random.RandomState(23)
    B, D, H, W = shape
    x = rs.standard_normal((B, D, H, W, 32))
    if regime == 'relu':
        x = np.maximum(x, 0.0)
    elif regime == 'wide':
        x = np.exp2(-14.0 * rs.uniform(0.0, 1.0, x.shape)) * np.sign(x)
    x, xbuf, ex = quant_x(x.astype(np.float32))
    w0 = quant_w(rs.standard_normal((16, 32, 3, 3, 3)) * np.sqrt(2.0 / (32 * 27)))
    s0 = rs.uniform(0.5, 1.5, 16).astype(np.float32); b0 = (rs.standard_normal(16) * 0.3).astype(np.float32)
    w1 = quant_w(rs.standard_normal((8, 16)) * 0.4, per_column=False)
    s1 = rs.uniform(0.5, 1.5, 8).astype(np.float32); b1 = (rs.standard_normal(8) * 0.3).astype(np.float32)
    w2 = quant_w(rs.standard_normal((18, 8)) * 0.5, per_column=False)
    if regime == 'wide':                                    # the conv's columns at scales 2^k; x is small, so is the bias
        s0 = np.exp2(rs.randint(-2, 11, 16).astype(np.float64)).astype(np.float32)
        b0 = (b0 * 0.05 * s0 * 2.0 ** -4).astype(np.float32)
    return OccOperands(x, xbuf, ex, w0, s0, b0, w1, s1, b1, w2)


@functools.lru_cache(maxsize=None)
def occ_ref(shape, regime):
    P = occ_operands(shape, regime)
    args = (P.x, P.w0, P.s0, P.b0, P.w1, P.s1, P.b1, P.w2)
    with one_thread():
        r32 = occ_head(*args, dtype=torch.float32)
    return occ_head(*args), r32


def occ_q32(name):
    r = ROWS[name]
    ref, r32 = occ_ref(r['shape'], r['regime'])
    qs = q_of(r32.logits, ref.logits, ref.n)
    return float(qs.max()), float(qs.mean())


def near_tie(ref, bound):
    """(B, D, H, W) bool: voxels whose float64 top-2 margin is at most twice the asserted bound times the largest unit there"""
    return ref.margin <= 2.0 * bound * U * ref.n.max(-1).values


# ------------------------------------------------------------------------------------------------ the neck rows
def _fpn(shape, lv16, lv32, kernel, h2, regime):
    return dict(kind='fpn', shape=shape, lv16=lv16, lv32=lv32, kernel=kernel, h2=h2, regime=regime, family='k_fpn3d_fuse')


# fine grids that are not exactly 2x and 4x the coarse ones are what the stride-2 stages produce from odd extents: (n + 1) // 2
ROWS['fpn_tile_h2'] = _fpn((1, 4, 12, 36), (2, 6, 18), (1, 3, 9), 'k_fpn3d_fuse<true>', True, 'normal')
ROWS['fpn_tile_f32_odd'] = _fpn((2, 5, 19, 37), (3, 10, 19), (2, 5, 10), 'k_fpn3d_fuse<true>', False, 'wide')
ROWS['fpn_row_h2_odd'] = _fpn((2, 5, 19, 27), (3, 10, 14), (2, 5, 7), 'k_fpn3d_fuse<false>', True, 'relu')
ROWS['fpn_row_f32'] = _fpn((1, 4, 12, 20), (2, 6, 10), (1, 3, 5), 'k_fpn3d_fuse<false>', False, 'normal')

FpnRef = collections.namedtuple('FpnRef', 'x xbuf ex w8 y16 y32 scale bias y n y32f e')


@functools.lru_cache(maxsize=None)
def fpn_ref(name):
    r = ROWS[name]
    rs = np.random.RandomState(300 + list(ROWS).index(name))
    B, D, H, W = r['shape']
    x, xbuf, ex = quant_x(_draw_x(rs, (B, D, H, W, 32), r['regime']).astype(np.float32))
    y16 = _draw_x(rs, (B,) + r['lv16'] + (32,), r['regime']).astype(np.float32)
    y32 = _draw_x(rs, (B,) + r['lv32'] + (32,), r['regime']).astype(np.float32)
    w8 = quant_w(rs.standard_normal((32, 32, 1, 1, 1)) * np.sqrt(2.0 / 32))
    scale, bias = _draw_scale_bias(rs, 32, r['regime'])
    y, n = neck(x, w8, y16, y32, scale, bias)
    t = torch.from_numpy
    up = lambda a: torch.nn.functional.interpolate(t(a).permute(0, 4, 1, 2, 3), size=(D, H, W), mode='trilinear',
                                                   align_corners=True).permute(0, 2, 3, 4, 1)
    with one_thread():
        f = torch.relu((t(x) @ t(w8).view(32, 32).t() + up(y16) + up(y32)) * t(scale) + t(bias))
    return FpnRef(x, xbuf, ex, w8, y16, y32, scale, bias, y, n, f, ideal_exp(float(y.abs().max())))


def fpn_q32(name):
    ref = fpn_ref(name)
    qs = q_of(ref.y32f, ref.y, ref.n)
    return float(qs.max()), float(qs.mean())


def q32(name):
    """(max, mean) q of the float32 restatement of a row, measured on the CPU"""
    return {'conv': conv_q32, 'occ': occ_q32, 'fpn': fpn_q32}[ROWS[name]['kind']](name)


# max q of the float32 restatement per row, measured by test_infer_ref64_cpu.py (which asserts that the restatement stays under
# each entry and above half of it) and rounded up to two digits; the mean is printed there
Q32 = {
    'h2_A_epi1_pair':          3.5,     # measured 3.483 (mean 0.178)
    'h2_A_epi2_res':           3.2,     # measured 3.121 (mean 0.115)
    'h2_A_epi3_f32':           3.5,     # measured 3.483 (mean 0.242)
    'h2_A_epi0_pair':          3.5,     # measured 3.483 (mean 0.178)
    'h2_A_epi0_res32':         3.2,     # measured 3.121 (mean 0.115)
    'h2_B_epi1_pair':          4.8,     # measured 4.737 (mean 0.199)
    'h2_B_epi2_res':           4.8,     # measured 4.726 (mean 0.143)
    'h2_B_epi3_f32':           4.8,     # measured 4.737 (mean 0.310)
    'h2_B_epi0_pair':          4.8,     # measured 4.737 (mean 0.199)
    'h2_B_epi0_res32':         4.8,     # measured 4.726 (mean 0.143)
    'h2_C_wr_epi1':            3.9,     # measured 3.826 (mean 0.184)
    'h2_C_wr_epi2':            3.7,     # measured 3.679 (mean 0.172)
    'h2_C_wr_epi3':            4.4,     # measured 4.353 (mean 0.374)
    'h2_D_wr_epi1':            3.1,     # measured 3.019 (mean 0.133)
    'h2_D_wr_epi2':            3,       # measured 2.928 (mean 0.128)
    'h2_D_wr_epi3':            3.3,     # measured 3.268 (mean 0.250)
    'h2_C_epi0_res32':         3.7,     # measured 3.679 (mean 0.172)
    'ga_k1_64':                3.8,     # measured 3.794 (mean 0.313)
    'ga_k1_128':               4.8,     # measured 4.773 (mean 0.568)
    'ga_k3_algo2':             2.3,     # measured 2.218 (mean 0.107)
    'ga_k3_algo3_ks2':         4.8,     # measured 4.726 (mean 0.143)
    'ga_k3_algo3_ks4':         0.72,    # measured 0.715 (mean 0.063)
    'ga_s2_32_h2':             1.8,     # measured 1.762 (mean 0.117)
    'ga_s2_64_f32':            3.7,     # measured 3.662 (mean 0.434)
    'ga_s2_64_h2':             3.7,     # measured 3.692 (mean 0.215)
    'ga_s2_96_f32':            1.8,     # measured 1.797 (mean 0.119)
    'ga_s2_96_mt1':            3.2,     # measured 3.179 (mean 0.118)
    's2_128':                  2.1,     # measured 2.044 (mean 0.184)
    's2_256':                  4.4,     # measured 4.397 (mean 0.238)
    's2_128_wide':             4,       # measured 3.937 (mean 0.318)
    'f32_tiled_nt2':           3.2,     # measured 3.121 (mean 0.115)
    'f32_tiled_nt1':           3.9,     # measured 3.826 (mean 0.184)
    'f32_pipe_nt2':            3.5,     # measured 3.483 (mean 0.118)
    'f32_pipe_nt1':            3.3,     # measured 3.268 (mean 0.250)
    'f32_pipe_relu':           2,       # measured 1.930 (mean 0.104)
    'f32_gather_k2s2':         1.8,     # measured 1.710 (mean 0.241)
    'f32_wino_ng2':            3.2,     # measured 3.121 (mean 0.115)
    'f32_wino_ng1':            3.9,     # measured 3.826 (mean 0.184)
    'occ_2x5x19x27_logits':    0.18,    # measured 0.177 (mean 0.014)
    'occ_2x5x19x27_strided':   0.18,    # measured 0.177 (mean 0.014)
    'occ_3x2x9x7_logits':      0.13,    # measured 0.127 (mean 0.017)
    'occ_3x2x9x7_strided':     0.13,    # measured 0.127 (mean 0.017)
    'occ_1x4x8x8_logits':      0.4,     # measured 0.394 (mean 0.028)
    'occ_1x4x8x8_strided':     0.4,     # measured 0.394 (mean 0.028)
    'occ_f32_direct':          0.24,    # measured 0.231 (mean 0.015)
    'occ_f32_wino':            0.24,    # measured 0.231 (mean 0.015)
    'fpn_tile_h2':             6.5,     # measured 6.478 (mean 0.235)
    'fpn_tile_f32_odd':        7.5,     # measured 7.485 (mean 0.256)
    'fpn_row_h2_odd':          3.8,     # measured 3.765 (mean 0.285)
    'fpn_row_f32':             3.9,     # measured 3.871 (mean 0.213)
}

# a-priori terms, in units of u, added to single rows for reasons that lie in the format (profiles/infer_conv_pin.md)
FORMAT_TERM = {
}


def bound(name):
    return 2.0 * Q32[name] + 1.0 + FORMAT_TERM.get(name, 0.0)
