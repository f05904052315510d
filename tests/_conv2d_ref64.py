"""The stride-1 convolutions of the reference's FPN_LSS (mmdet3d/models/necks/lss_fpn.py:13-110) and DepthNet
(mmdet3d/models/necks/view_transformer.py:322-638) with the eval-mode BatchNorm, bias, ReLU and residual addition behind them,
restated in float64 torch -- the yardstick pw_conv2d (csrc/pw_conv2d.hip, behind ops.conv2d and conv_impl='hip') answers to.

A plain composition: F.conv2d in double with zero padding dilation (k - 1) / 2; (y - mean) / sqrt(var + eps) * gamma + beta from the
raw statistics; + residual; max(., 0).  Nothing is folded, scaled, split or laid out channels-last here, and nothing above the
harness line calls project code.

THE CASES are the smallest shapes at which the kernel can still go wrong (see CASES).  The kernel has four tile variants
(tile_variant below mirrors its dispatch rule: a 64 x 64 tile, and where ceil(M / 128) x ceil(Cout / 128) >= 128 a 128 x 128 one;
with more than 1024 packed k -- taps x Cin rounded up to 32 -- the sum is taken in blocks of 1024 and the large tile is 128 x 64).
The table's shapes reach only the two small variants, so `big_1x1` and `big_3x3` run the two large ones, each with a row tail
(M = 5440 = 42.5 tiles), a column tail (Cout = 272) and a Cin tail (144), and `big_deep_small_tile` gives the small blocked-sum
variant a column tail as well.  Inputs are seeded.

THE BOUND.  Per case 4 x FLOORS[case], relative to max |out64|, no element excluded: the floor is max |out_torch - out64| /
max |out64| of the EXISTING torch modules on the CPU in float32 -- F.conv2d, F.batch_norm in eval mode, the addition and ReLU --
measured by tests/test_conv2d_cpu.py, which asserts that the torch path stays under each entry (rounded up to two digits) and
reaches at least half of it: never taken from the kernel.  The factor covers a different summation order and the matrix-core
products, as for the Linears (tests/_swin_linear_ref64.py).

THE UNIT.  That figure divides by the tensor's largest element, so an error in a dim image, a small channel or a corner pixel
vanishes in it (tests/test_conv2d_cpu.py::test_the_unit_sees_what_the_tensor_maximum_hides).  Every case is therefore ALSO scored per
element, as tests/_infer_ref64.py scores the voxel side:
    q = |out - out64| / (2^-24 n),      n = conv2d(|x|, |w|) |scale| + |shift| + |residual|
with scale = gamma / sqrt(var + eps) and shift = beta + (bias - mean) scale, the folded BatchNorm and bias in float64 (fold64; a
ReLU passes n through unchanged; an element with n == 0 must be reproduced exactly).  The bound is max q <= 2 Q32[case] + 1 +
FORMAT_TERM.get(case, 0): Q32 is the worst q of the same float32 torch path on one CPU thread, rounded up to two digits and asserted
by tests/test_conv2d_cpu.py like FLOORS; FORMAT_TERM holds a-priori terms only (profiles/image_gemm_units.md).  Four cases aim at
the exponents -- the kernel takes ONE power of two for all of x and one per weight row: dim_image (the second image x 2^-14, no
BatchNorm or bias, so its outputs are judged at their own size), dim_corner (the rows h < 6 x 2^-14 under dilation 6), w_rows_span
(weight row n x 2^((n % 25) - 12), Cout = 88: the n tail) and bn_scale_span (gamma and beta of channel c x 2^-(c % 11))."""
import collections
import contextlib
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

Case = collections.namedtuple('Case', 'B H W Cin Cout k dil epi seed bn bias special x_scale')
# epi: 'none', 'relu' or 'residual_relu'; bn: an eval-mode BatchNorm behind the convolution; bias: the convolution has one


def _c(B, H, W, Cin, Cout, k, dil, epi, seed, bn=True, bias=False, special=None, x_scale=1.0):
    return Case(B, H, W, Cin, Cout, k, dil, epi, seed, bn, bias, special, x_scale)


CASES = collections.OrderedDict([
    ('toy_3x3', _c(2, 2, 3, 16, 16, 3, 1, 'relu', 1)),                               # the map is smaller than any tile
    ('far_taps', _c(2, 2, 3, 16, 8, 3, 18, 'relu', 2)),                              # every off-centre tap is outside (the golden ASPP)
    ('dil6_edges', _c(1, 20, 15, 32, 16, 3, 6, 'relu', 3)),                          # taps partly inside; W above the dilation
    ('dil12_edges', _c(1, 20, 15, 32, 16, 3, 12, 'relu', 4)),                        # ... and W - 1 = 14 barely above it, H above
    ('image_seam', _c(3, 5, 7, 32, 32, 3, 1, 'none', 5)),                            # an M tile spans images and many row ends
    ('cin_tail', _c(1, 9, 11, 28, 16, 3, 1, 'relu', 6)),                             # k tail: 28 of 32
    ('cin_600', _c(1, 8, 12, 600, 64, 3, 1, 'relu', 7)),                             # k tail: 600 of 608, blocked sum
    ('cout_88_1x1', _c(1, 9, 11, 32, 88, 1, 1, 'none', 8, bn=False, bias=True)),     # n tail, one tap, plain bias
    ('neck_deep', _c(1, 6, 10, 1536, 64, 3, 1, 'relu', 9)),                          # K = 13 824
    ('res_relu', _c(2, 7, 9, 64, 64, 3, 1, 'residual_relu', 10, special='neg')),     # some channels mostly negative before the ReLU
    ('bn_fold', _c(1, 9, 11, 32, 32, 3, 1, 'relu', 11, bias=True, special='bn_fold')),      # large mean, tiny variance, conv bias
    ('outlier_channel', _c(1, 9, 11, 32, 32, 3, 1, 'relu', 12, special='outlier')),  # one input channel 2^10 x the rest
    ('range_2m12', _c(2, 7, 9, 64, 64, 3, 1, 'residual_relu', 13, bias=True, x_scale=2.0 ** -12)),      # x, shift, residual x 2^-12 / 2^8
    ('range_2p8', _c(2, 7, 9, 64, 64, 3, 1, 'residual_relu', 13, bias=True, x_scale=2.0 ** 8)),
    ('zero_image', _c(1, 5, 7, 16, 16, 3, 1, 'relu', 14, special='zero')),           # out = epi(shift)
    ('big_deep_small_tile', _c(1, 9, 11, 144, 88, 3, 1, 'residual_relu', 15)),          # 64 x 64 blocked sum with row, column and Cin tails
    ('big_1x1', _c(2, 32, 85, 144, 272, 1, 1, 'none', 16, bn=False, bias=True)),     # 128 x 128 tile
    ('big_3x3', _c(2, 32, 85, 144, 272, 3, 1, 'relu', 17)),                          # 128 x 64 tile, blocked sum
    # the exponents (see THE UNIT): what one power of two for all of x, and one per weight row, do to the small values
    ('dim_image', _c(2, 7, 9, 64, 64, 3, 1, 'none', 18, bn=False, special='dim_image')),      # the second image x 2^-14, no shift
    ('dim_corner', _c(1, 20, 15, 32, 16, 3, 6, 'relu', 19, special='dim_corner')),   # the rows h < 6 x 2^-14 under dilation 6
    ('w_rows_span', _c(1, 9, 11, 32, 88, 3, 1, 'none', 20, bn=False, special='w_rows_span')),      # weight row n x 2^((n % 25) - 12), n tail
    ('bn_scale_span', _c(1, 9, 11, 32, 32, 3, 1, 'relu', 21, special='bn_scale_span')),      # folded scale and shift of channel c x 2^-(c % 11)
])
EPS = 1e-5
OUTLIER_CHANNEL = 5
DIM = 2.0 ** -14
U = 2.0 ** -24

# max |out_torch - out64| / max |out64| of the torch path on the CPU in float32 (see the module docstring), rounded up to two digits
FLOORS = {
    'toy_3x3': 4.4e-07,                      # measured 4.342e-07
    'far_taps': 9.2e-08,                     # measured 9.162e-08
    'dil6_edges': 4.3e-07,                   # measured 4.201e-07
    'dil12_edges': 2.3e-07,                  # measured 2.239e-07
    'image_seam': 2.5e-07,                   # measured 2.402e-07
    'cin_tail': 4.0e-07,                     # measured 3.915e-07
    'cin_600': 2.2e-07,                      # measured 2.105e-07
    'cout_88_1x1': 2.0e-07,                  # measured 1.981e-07
    'neck_deep': 3.8e-07,                    # measured 3.773e-07
    'res_relu': 2.4e-07,                     # measured 2.355e-07
    'bn_fold': 7.4e-07,                      # measured 7.393e-07
    'outlier_channel': 9.2e-07,              # measured 9.139e-07
    'range_2m12': 3.2e-07,                   # measured 3.109e-07
    'range_2p8': 3.2e-07,                    # measured 3.109e-07
    'zero_image': 4.4e-08,                   # measured 4.346e-08
    'big_deep_small_tile': 3.7e-07,          # measured 3.654e-07
    'big_1x1': 4.2e-07,                      # measured 4.132e-07
    'big_3x3': 3.1e-07,                      # measured 3.044e-07
    'dim_image': 2.9e-07,                    # measured 2.852e-07
    'dim_corner': 6.8e-07,                   # measured 6.720e-07
    'w_rows_span': 4.0e-07,                  # measured 3.972e-07
    'bn_scale_span': 2.8e-07,                # measured 2.759e-07
}

# worst q of the same torch path in the units of THE UNIT (2^-24 n), rounded up to two digits
Q32 = {
    'toy_3x3': 1.5,                          # measured 1.442, mean 0.139
    'far_taps': 1.5,                         # measured 1.426, mean 0.152
    'dil6_edges': 2.4,                       # measured 2.333, mean 0.162
    'dil12_edges': 3,                        # measured 2.991, mean 0.173
    'image_seam': 1.8,                       # measured 1.744, mean 0.257
    'cin_tail': 2.4,                         # measured 2.343, mean 0.171
    'cin_600': 0.58,                         # measured 0.5735, mean 0.037
    'cout_88_1x1': 3.7,                      # measured 3.655, mean 0.334
    'neck_deep': 0.36,                       # measured 0.3541, mean 0.026
    'res_relu': 1.5,                         # measured 1.448, mean 0.073
    'bn_fold': 4.8,                          # measured 4.79, mean 0.308
    'outlier_channel': 16,                   # measured 15.11, mean 0.988
    'range_2m12': 1.3,                       # measured 1.296, mean 0.094
    'range_2p8': 1.3,                        # measured 1.296, mean 0.094
    'zero_image': 1.8,                       # measured 1.764, mean 0.409
    'big_deep_small_tile': 1.6,              # measured 1.546, mean 0.090
    'big_1x1': 5.5,                          # measured 5.41, mean 0.330
    'big_3x3': 1.1,                          # measured 1.038, mean 0.065
    'dim_image': 1.3,                        # measured 1.265, mean 0.187
    'dim_corner': 4,                         # measured 3.995, mean 0.200
    'w_rows_span': 3.5,                      # measured 3.467, mean 0.332
    'bn_scale_span': 3.6,                    # measured 3.533, mean 0.169
}
# a-priori terms of the format, in units of 2^-24 n (profiles/image_gemm_units.md); never fitted to a measured q
FORMAT_TERM = {}

# the two modules at real width (build_neck / build_depthnet below): the torch module in float32 on the CPU against the same module
# in float64, rounded up to two digits
MODULE_FLOORS = {
    'neck': 4.8e-07,                         # measured 4.708e-07
    'depthnet': 6.5e-07,                     # measured 6.495e-07
}


def tile_variant(c):
    """(TM, TN, deep) of the k_conv2d instantiation pw_conv2d launches for a case: a Python mirror of its dispatch rule"""
    M, Kp = c.B * c.H * c.W, c.k * c.k * (-(-c.Cin // 32) * 32)
    large, deep = -(-M // 128) * -(-c.Cout // 128) >= 128, Kp > 1024
    return (2 if large else 1, 2 if large and not deep else 1, deep)


TILE_VARIANTS = {(1, 1, False), (1, 1, True), (2, 2, False), (2, 1, True)}


def _randn(rs, *shape):
    return torch.from_numpy(rs.standard_normal(shape).astype(np.float32))


def _uniform(rs, lo, hi, *shape):
    return torch.from_numpy(rs.uniform(lo, hi, shape).astype(np.float32))


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict(x (B, Cin, H, W), weight (Cout, Cin, k, k), bias (Cout) or None, bn = (gamma, beta, mean, var) or None, residual
    (B, Cout, H, W) or None): float32 CPU tensors in the default (NCHW) layout"""
    c = CASES[name]
    rs = np.random.RandomState(3000 + c.seed)
    x = _randn(rs, c.B, c.Cin, c.H, c.W)
    w = _randn(rs, c.Cout, c.Cin, c.k, c.k) / math.sqrt(c.Cin * c.k * c.k)
    b = 0.1 * _randn(rs, c.Cout) if c.bias else None
    bn = None
    if c.bn:
        bn = [_uniform(rs, 0.5, 1.5, c.Cout), 0.1 * _randn(rs, c.Cout), 0.1 * _randn(rs, c.Cout), _uniform(rs, 0.5, 1.5, c.Cout)]
    res = _randn(rs, c.B, c.Cout, c.H, c.W) if c.epi == 'residual_relu' else None
    if c.special == 'neg':                                 # every fourth channel sits about two sigma below zero
        bn[1][::4] -= 2.0
    if c.special == 'bn_fold':                             # every third channel: |mean| ~ 30 x the conv's output, var ~ 1e-4
        bn[2][::3] = 30.0 + _randn(rs, len(bn[2][::3]))
        b[::3] += 30.0                                     # ... which the conv bias meets, so the normalised value stays O(100)
        bn[3][::3] = 1e-4 * _uniform(rs, 0.5, 1.5, len(bn[3][::3]))
    if c.special == 'outlier':
        x[:, OUTLIER_CHANNEL] *= 2.0 ** 10
    if c.special == 'zero':
        x = torch.zeros_like(x)
    if c.special == 'dim_image':
        x[1] *= DIM
    if c.special == 'dim_corner':
        x[:, :, :c.dil] *= DIM
    if c.special == 'w_rows_span':
        w = w * torch.pow(2.0, (torch.arange(c.Cout) % 25 - 12).float()).view(-1, 1, 1, 1)
    if c.special == 'bn_scale_span':                       # gamma and beta: the channel's whole output is scaled
        f = torch.pow(2.0, -(torch.arange(c.Cout) % 11).float())
        bn[0], bn[1] = bn[0] * f, bn[1] * f
    if c.x_scale != 1.0:                                   # x, residual and everything that enters the shift
        x, res, b = x * c.x_scale, res * c.x_scale, b * c.x_scale
        bn[1], bn[2] = bn[1] * c.x_scale, bn[2] * c.x_scale
    return dict(x=x, weight=w, bias=b, bn=None if bn is None else tuple(bn), residual=res)


def padding(c):
    return c.dil * (c.k - 1) // 2


@functools.lru_cache(maxsize=None)
def reference(name):
    """the float64 yardstick of a case, (B, Cout, H, W)"""
    c, i = CASES[name], inputs(name)
    d = lambda t: None if t is None else t.double()
    y = F.conv2d(d(i['x']), d(i['weight']), d(i['bias']), stride=1, padding=padding(c), dilation=c.dil)
    if i['bn'] is not None:
        g, beta, mean, var = (d(t).view(1, -1, 1, 1) for t in i['bn'])
        y = (y - mean) / torch.sqrt(var + EPS) * g + beta
    if i['residual'] is not None:
        y = y + d(i['residual'])
    return y if c.epi == 'none' else y.clamp_min(0.0)


def torch_path(name, dtype=torch.float32):
    """what the torch modules compute for a case: F.conv2d, F.batch_norm in eval mode, the addition, ReLU"""
    c, i = CASES[name], inputs(name)
    d = lambda t: None if t is None else t.to(dtype)
    y = F.conv2d(d(i['x']), d(i['weight']), d(i['bias']), stride=1, padding=padding(c), dilation=c.dil)
    if i['bn'] is not None:
        g, beta, mean, var = (d(t) for t in i['bn'])
        y = F.batch_norm(y, mean, var, g, beta, False, 0.1, EPS)
    if i['residual'] is not None:
        y = y + d(i['residual'])
    return y if c.epi == 'none' else F.relu(y)


def rel_err(out, ref):
    return float((out.double() - ref.double()).abs().max() / ref.double().abs().max())


# ------------------------------------------------------------------------------------------------------- the unit, per element
def fold64(name):
    """(scale, shift) (Cout,) of the eval-mode BatchNorm and the bias behind a case's convolution, in float64:
    y = conv(x, w) scale + shift"""
    c, i = CASES[name], inputs(name)
    bias = torch.zeros(c.Cout, dtype=torch.float64) if i['bias'] is None else i['bias'].double()
    if i['bn'] is None:
        return torch.ones(c.Cout, dtype=torch.float64), bias
    g, beta, mean, var = (t.double() for t in i['bn'])
    scale = g / torch.sqrt(var + EPS)
    return scale, beta + (bias - mean) * scale


@functools.lru_cache(maxsize=None)
def normaliser(name):
    """n = conv2d(|x|, |w|) |scale| + |shift| + |residual| in float64, (B, Cout, H, W); a ReLU passes it through unchanged.  Computed
    once and shared (do not modify)"""
    c, i = CASES[name], inputs(name)
    scale, shift = fold64(name)
    n = F.conv2d(i['x'].double().abs(), i['weight'].double().abs(), None, stride=1, padding=padding(c), dilation=c.dil)
    n = n * scale.abs().view(1, -1, 1, 1) + shift.abs().view(1, -1, 1, 1)
    return n if i['residual'] is None else n + i['residual'].double().abs()


@contextlib.contextmanager
def one_thread():
    """a CPU measurement that gives the same figure on every machine: torch picks a GEMM's blocking, and so the order of its sums, by
    the thread count"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(threads)


def q_of(got, ref, n):
    """per-element q = |got - ref| / (2^-24 n) in double; where n == 0 the element must be reproduced exactly (q = inf otherwise); a
    NaN counts as inf"""
    err = (got.double() - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float('inf')), err)
    return torch.where(n > 0, err / (U * n.clamp_min(1e-300)), torch.where(err > 0, torch.full_like(err, float('inf')), err))


def bound(name):
    return 2.0 * Q32[name] + 1.0 + FORMAT_TERM.get(name, 0.0)


def check_units(name, out, say):
    """a case's output in per-element units against bound(name); prints the figures before it asserts; returns (worst, mean) q"""
    q = q_of(out.cpu(), reference(name), normaliser(name))
    worst, mean = float(q.max()), float(q.mean())
    print('%s: %s worst q %.3f, mean q %.3f, Q32 %.2f, bound %.2f, variant %s' % (name, say, worst, mean, Q32[name], bound(name),
                                                                                 tile_variant(CASES[name])))
    assert worst <= bound(name), (name, worst, bound(name))
    return worst, mean


# ------------------------------------------------------------------------------------------------------------ harness (project code)
def conv_modules(name, device='cpu'):
    """(nn.Conv2d, nn.BatchNorm2d in eval mode or None) holding a case's parameters: what ops.conv2d_pack takes"""
    c, i = CASES[name], inputs(name)
    conv = torch.nn.Conv2d(c.Cin, c.Cout, c.k, stride=1, padding=padding(c), dilation=c.dil, bias=c.bias)
    bn = None
    with torch.no_grad():
        conv.weight.copy_(i['weight'])
        if c.bias:
            conv.bias.copy_(i['bias'])
        if c.bn:
            bn = torch.nn.BatchNorm2d(c.Cout, eps=EPS).eval()
            for t, v in zip((bn.weight, bn.bias, bn.running_mean, bn.running_var), i['bn']):
                t.copy_(v)
    return conv.to(device), None if bn is None else bn.to(device)


def build_neck(conv_impl='torch', dtype=torch.float32):
    """FPN_LSS at the real width (1536 -> 512) on the smallest pair of maps: (module in eval mode, [x2 (1, 512, 4, 6), x1 (1, 1024, 2, 3)])"""
    from preworld_amd import image_encoder as IE, synth as S
    neck = IE.FPN_LSS(in_channels=512 + 1024, out_channels=512, extra_upsample=None, input_feature_index=(0, 1), scale_factor=2,
                      conv_impl=conv_impl).eval()
    neck.load_state_dict(S.seeded_module_state(neck, 61))
    rs = np.random.RandomState(62)
    feats = [_randn(rs, 1, 512, 4, 6).to(dtype), _randn(rs, 1, 1024, 2, 3).to(dtype)]
    return neck.to(dtype), feats


def build_depthnet(conv_impl='torch', dtype=torch.float32):
    """DepthNet at the real width (512 channels, 88 depth bins, 96-wide ASPP, stereo) on an 8 x 12 map with no previous stereo feature
    (a zero cost volume through cost_volumn_net): (module in eval mode, x (1, 512, 8, 12), mlp_input (1, 1, 27), stereo_metas)"""
    from preworld_amd import image_encoder as IE, synth as S
    dn = IE.DepthNet(512, 512, 32, 88, use_dcn=False, aspp_mid_channels=96, stereo=True, bias=5.0, conv_impl=conv_impl).eval()
    dn.load_state_dict(S.seeded_module_state(dn, 63))
    rs = np.random.RandomState(64)
    x, mlp = _randn(rs, 1, 512, 8, 12).to(dtype), _randn(rs, 1, 1, 27).to(dtype)
    return dn.to(dtype), x, mlp, dict(cv_feat_list=[None, None], downsample=16, cv_downsample=4)
