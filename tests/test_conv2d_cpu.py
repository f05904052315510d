"""The FPN_LSS / DepthNet convolutions (pw_conv2d*, ops.conv2d, conv_impl='hip') on the CPU side: the float64 yardstick of
tests/_conv2d_ref64.py against F.conv2d + F.batch_norm in double, the FLOORS and Q32 tables against the torch path (met, and not loose), the per-element unit against the tensor maximum on a
spoilt reference, the
header's ABI rules, refusals before any HIP call, and the module plumbing."""
import ctypes
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _conv2d_ref64 as R
import _swin_linear_ref64 as L
from preworld_amd import _lib, image_encoder as IE, ops

NAMES = list(R.CASES)
FNS = {'pw_conv2d_packed_bytes', 'pw_conv2d_pack', 'pw_conv2d_workspace_bytes', 'pw_conv2d'}
SIZE_FNS = {'pw_conv2d_packed_bytes', 'pw_conv2d_workspace_bytes'}


# ------------------------------------------------------------------------------------------------------------ yardstick, floors
@pytest.mark.parametrize('name', NAMES)
def test_yardstick_agrees_with_torch_in_float64(name):
    ref = R.reference(name)
    out = R.torch_path(name, torch.float64)
    assert out.dtype == torch.float64 and R.rel_err(out, ref) < 1e-12, R.rel_err(out, ref)


@pytest.mark.parametrize('name', NAMES)
def test_floor_of_the_torch_path(name):
    """FLOORS[name] bounds the float32 torch path on the CPU from above, and by less than a factor of two"""
    out = R.torch_path(name)
    assert out.dtype == torch.float32
    err = R.rel_err(out, R.reference(name))
    print('%s: torch path %.3e, floor %.1e' % (name, err, R.FLOORS[name]))
    assert 0.5 * R.FLOORS[name] <= err <= R.FLOORS[name], (name, err)
    assert set(R.FLOORS) == set(R.CASES)


@pytest.mark.parametrize('name', NAMES)
def test_q32_of_the_torch_path(name):
    """Q32[name] bounds the worst per-element q of the float32 torch path from above, by less than a factor of two; the normaliser is
    at least |out64| everywhere, as a sum of absolute values must be"""
    ref, n = R.reference(name), R.normaliser(name)
    assert n.dtype == torch.float64 and tuple(n.shape) == tuple(ref.shape) and bool((n >= ref.abs() * (1 - 1e-12)).all())
    with R.one_thread():
        q = R.q_of(R.torch_path(name), ref, n)
    worst = float(q.max())
    print('%s: torch path worst q %.4g, mean q %.3f, Q32 %.2f, bound %.2f, variant %s' % (name, worst, float(q.mean()), R.Q32[name],
                                                                                     R.bound(name), R.tile_variant(R.CASES[name])))
    assert 0.5 * R.Q32[name] <= worst <= R.Q32[name], (name, worst)
    assert set(R.Q32) == set(R.CASES) and set(R.FORMAT_TERM) <= set(R.CASES)


def test_the_fold_of_the_normaliser_is_the_yardsticks():
    """fold64 restates the BatchNorm and bias as scale and shift: conv(x, w) scale + shift (+ residual, ReLU) is the yardstick"""
    for name in ('bn_fold', 'res_relu', 'cout_88_1x1', 'bn_scale_span', 'dim_image'):
        c, i = R.CASES[name], R.inputs(name)
        scale, shift = R.fold64(name)
        y = F.conv2d(i['x'].double(), i['weight'].double(), None, padding=R.padding(c), dilation=c.dil)
        y = y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
        y = y if i['residual'] is None else y + i['residual'].double()
        y = y if c.epi == 'none' else y.clamp_min(0.0)
        assert R.rel_err(y, R.reference(name)) < 1e-12, name


def test_exponent_cases_are_what_they_claim():
    C, i = R.CASES, R.inputs
    c, x = C['dim_image'], i('dim_image')['x']
    assert (c.B, c.H, c.W, c.Cin, c.Cout, c.k, c.dil) == (2, 7, 9, 64, 64, 3, 1) and not c.bn and not c.bias and c.epi == 'none'
    assert 2.0 ** -14.5 < float(x[1].abs().max() / x[0].abs().max()) < 2.0 ** -13.5
    n = R.normaliser('dim_image')
    assert float(n[0].min() / n[1].max()) > 2.0 ** 10                # the whole second image lies far below the first
    c, x = C['dim_corner'], i('dim_corner')['x']
    assert (c.B, c.H, c.W, c.Cin, c.Cout, c.k, c.dil) == (1, 20, 15, 32, 16, 3, 6)
    assert float(x[:, :, :6].abs().max()) < 2.0 ** -11 and float(x[:, :, 6:].abs().max()) > 2.0
    c, w = C['w_rows_span'], i('w_rows_span')['weight']
    assert (c.H, c.W, c.Cin, c.Cout, c.k) == (9, 11, 32, 88, 3) and c.Cout % 64 and not c.bn and not c.bias
    amax = w.abs().amax((1, 2, 3))
    assert 2.0 ** 11.5 < float(amax[12] / amax[0]) < 2.0 ** 12.5 and float(amax.max() / amax.min()) > 2.0 ** 22
    c = C['bn_scale_span']
    assert (c.H, c.W, c.Cin, c.Cout, c.k) == (9, 11, 32, 32, 3) and c.bn
    scale, shift = R.fold64('bn_scale_span')
    assert 2.0 ** 9 < float(scale.abs().max() / scale.abs().min()) < 2.0 ** 12 and float(scale.abs().max()) < 2.5
    assert float((shift.abs() / scale.abs()).max() / (shift.abs() / scale.abs()).min()) < 2.0 ** 9      # the shift follows the scale


@pytest.mark.parametrize('name', ['dim_image', 'w_rows_span'])
def test_the_unit_sees_what_the_tensor_maximum_hides(name):
    """the yardstick against itself: the float64 output spoilt where it is small stays under the tensor-maximum bound 4 x FLOORS and
    is far over the per-element bound, which the clean float32 torch path meets.  w_rows_span: the output channels whose weight scale
    is <= 2^-9 lose the whole sum, or have their weights rounded to 11 significant bits (a lost lo plane).  dim_image: the second
    image's input is rounded to 11 significant bits; the tensor maximum does see that whole image vanish (2^-14 of the largest
    element against a bound near 2^-20; printed), so the sum is dropped from those of its elements that lie below 2^-20 of the
    largest -- which it cannot see either"""
    c, i, ref, n = R.CASES[name], R.inputs(name), R.reference(name), R.normaliser(name)
    x, w = i['x'].double(), i['weight'].double()
    dropped = ref.clone()
    if name == 'dim_image':
        whole = ref.clone()
        whole[1] = 0.0
        print('%s, the whole second image dropped: tensor-max %.3e (bound %.3e)' % (name, R.rel_err(whole, ref), 4 * R.FLOORS[name]))
        low = ref.abs() <= 2.0 ** -20 * ref.abs().max()
        low[0] = False
        assert 20 <= int(low.sum()) and R.rel_err(whole, ref) > 4 * R.FLOORS[name]
        dropped[low] = 0.0
        x = x.clone()
        x[1] = L.round11(x[1])
        where = '%d elements of the second image' % int(low.sum())
    else:
        low = torch.pow(2.0, (torch.arange(c.Cout) % 25 - 12).float()) <= L.LOW_SCALE
        assert 0 < int(low.sum()) < c.Cout // 2
        dropped[:, low] = 0.0
        w = torch.where(low.view(-1, 1, 1, 1), L.round11(w), w)
        where = '%d low channels' % int(low.sum())
    rounded = F.conv2d(x, w, None, padding=R.padding(c), dilation=c.dil)
    for what, out in (('the sum dropped in ' + where, dropped), ('11 significant bits', rounded)):
        old, q = R.rel_err(out, ref), float(R.q_of(out, ref, n).max())
        print('%s, %s: tensor-max %.3e (bound %.3e), worst q %.4g (bound %.2f)' % (name, what, old, 4 * R.FLOORS[name], q, R.bound(name)))
        assert 0.0 < old <= 4 * R.FLOORS[name], (name, what, old)
        assert q > 10 * R.bound(name), (name, what, q)
    with R.one_thread():
        clean = float(R.q_of(R.torch_path(name), ref, n).max())
    assert clean <= R.bound(name), (name, clean)


def test_module_floors():
    """the real-width neck and DepthNet of the GPU test: the torch module in float32 against the same module in float64"""
    with torch.no_grad():
        neck, feats = R.build_neck()
        neck64, feats64 = R.build_neck(dtype=torch.float64)
        err = R.rel_err(neck(feats), neck64(feats64))
        print('neck: torch path %.3e, floor %.1e' % (err, R.MODULE_FLOORS['neck']))
        assert 0.5 * R.MODULE_FLOORS['neck'] <= err <= R.MODULE_FLOORS['neck']
        dn, x, mlp, metas = R.build_depthnet()
        dn64, x64, mlp64, _ = R.build_depthnet(dtype=torch.float64)
        err = R.rel_err(dn(x, mlp, metas), dn64(x64, mlp64, metas))
        print('depthnet: torch path %.3e, floor %.1e' % (err, R.MODULE_FLOORS['depthnet']))
        assert 0.5 * R.MODULE_FLOORS['depthnet'] <= err <= R.MODULE_FLOORS['depthnet']


def test_cases_are_what_they_claim():
    C, i = R.CASES, R.inputs
    # every epilogue, both kernel sizes, a plain bias, a BatchNorm with a conv bias
    assert {c.epi for c in C.values()} == {'none', 'relu', 'residual_relu'} and {c.k for c in C.values()} == {1, 3}
    assert any(not c.bn and c.bias for c in C.values()) and any(c.bn and c.bias for c in C.values())
    # every tile variant, each with a row tail (against its own tile height) and a column tail
    seen = {}
    for name, c in C.items():
        tm, tn, deep = R.tile_variant(c)
        tails = ((c.B * c.H * c.W) % (64 * tm) != 0, c.Cout % (64 * tn) != 0)
        old = seen.get((tm, tn, deep), (False, False))
        seen[(tm, tn, deep)] = (old[0] or tails[0], old[1] or tails[1])
    assert set(seen) == R.TILE_VARIANTS and all(v == (True, True) for v in seen.values()), seen
    for name in ('big_1x1', 'big_3x3', 'big_deep_small_tile'):
        c = C[name]
        assert c.B <= 6 and c.H <= 32 and c.W <= 88 and c.Cin <= 144 and c.Cout <= 272, name
    assert R.tile_variant(C['neck_deep'])[2] and R.tile_variant(C['cin_600'])[2] and C['neck_deep'].k ** 2 * C['neck_deep'].Cin == 13824
    # far_taps: every off-centre tap is outside the map; the dilated edge cases: some inside, some outside
    c = C['far_taps']
    assert c.dil >= c.H and c.dil >= c.W
    for name in ('dil6_edges', 'dil12_edges'):
        c = C[name]
        assert c.dil < c.W and c.dil < c.H and c.W % 64 and (c.H * c.W) % 64
    # an M tile of image_seam spans two images; the k tails; the n tail
    c = C['image_seam']
    assert c.H * c.W < 64 < c.B * c.H * c.W and c.epi == 'none'
    assert C['cin_tail'].Cin % 32 and C['cin_600'].Cin % 32 and C['cout_88_1x1'].Cout % 64 and C['cout_88_1x1'].k == 1
    # exact power-of-two multiples of one draw
    a, b = i('range_2m12'), i('range_2p8')
    f = 2.0 ** 20
    assert torch.equal(a['x'] * f, b['x']) and torch.equal(a['residual'] * f, b['residual']) and torch.equal(a['bias'] * f, b['bias'])
    assert torch.equal(a['weight'], b['weight']) and torch.equal(a['bn'][0], b['bn'][0]) and torch.equal(a['bn'][3], b['bn'][3])
    assert torch.equal(a['bn'][1] * f, b['bn'][1]) and torch.equal(a['bn'][2] * f, b['bn'][2])
    assert torch.equal(R.torch_path('range_2m12', torch.float64) * f, R.torch_path('range_2p8', torch.float64))
    x = i('outlier_channel')['x']
    assert float(x[:, R.OUTLIER_CHANNEL].abs().median() / x[:, R.OUTLIER_CHANNEL + 1].abs().median()) > 500
    assert float(i('zero_image')['x'].abs().max()) == 0.0 and float(R.reference('zero_image').abs().max()) > 0.0
    g, beta, mean, var = i('bn_fold')['bn']
    assert float(mean.abs().max()) > 25.0 and float(var.min()) < 2e-4 and i('bn_fold')['bias'] is not None
    # res_relu: channels whose pre-activation is negative for most pixels, and the ReLU is live in every case that has one
    c, d = C['res_relu'], i('res_relu')
    pre = R.torch_path('res_relu', torch.float64)          # after the ReLU: zero where the pre-activation was negative
    assert float((pre[:, ::4] == 0).double().mean()) > 0.5 > float((pre[:, 1::4] == 0).double().mean())


# ------------------------------------------------------------------------------------------------------------ ABI
def test_conv2d_header_parses_like_the_main_header():
    """include/preworld_hip_conv2d.h (included by preworld_hip.h) under the rules tests/test_swin_linear_cpu.py holds the Linears' header
    to: every pw_*( parses, every pointer parameter has a converter, the library exports every name, stream comes last"""
    text = open(_lib.CONV2D_HEADER_PATH).read()
    protos = _lib.parse_header(_lib.CONV2D_HEADER_PATH)
    code = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    declared = set(re.findall(r'\b(pw_\w+)\s*\(', code))
    assert declared == set(protos) == FNS
    assert '#include "preworld_hip_conv2d.h"' in open(_lib.HEADER_PATH).read()
    assert _lib.PW_CONV2D == dict(PW_CONV2D_EPI_NONE=0, PW_CONV2D_EPI_RELU=1, PW_CONV2D_EPI_RESIDUAL_RELU=2, PW_CONV2D_MIN_DIM=4,
                                  PW_CONV2D_MAX_DIM=4096)
    l = _lib.lib()
    for fn, (restype, argtypes, argnames) in protos.items():
        assert hasattr(l, fn) and fn in _lib.protos()
        params = re.search(r'\b%s\s*\(([^;{]*?)\)\s*;' % fn, code).group(1).split(',')
        assert len(params) == len(argtypes) == len(argnames), fn
        for ptext, a, name in zip(params, argtypes, argnames):
            assert ('*' in ptext) == isinstance(a, _lib._PtrArg), (fn, name)
            if '*' in ptext:
                assert not a.table and not a.host, (fn, name)
        assert ctypes.c_void_p not in _lib._fns[fn].argtypes, fn
        if fn in SIZE_FNS:                                            # a size formula: host only, no stream
            assert restype is ctypes.c_size_t and 'stream' not in argnames, fn
        else:
            assert argnames[-1] == 'stream' and restype is ctypes.c_int, fn
    # every entry point cites the reference
    for fn in FNS:
        comment = text[:text.index(fn + '(')].rsplit('/*', 1)[1]
        assert 'lss_fpn.py:' in comment and 'view_transformer.py:' in comment, fn
    assert 'mmdet3d/models/necks/lss_fpn.py:13-110' in text and 'mmdet3d/models/necks/view_transformer.py:322-638' in text
    from preworld_amd import build
    assert 'preworld_hip_conv2d.h' in build.ABI_HEADERS and 'pw_conv2d.hip' in build.sources()


def test_size_formulas():
    l = _lib.lib()
    f = l.pw_conv2d_packed_bytes
    f.restype, f.argtypes = ctypes.c_size_t, [ctypes.c_int] * 3
    up = lambda v, m: -(-v // m) * m
    for Cin, Cout, k in ((4, 4, 1), (16, 16, 3), (28, 24, 3), (600, 512, 3), (512, 88, 1), (1536, 512, 3), (4096, 4096, 3), (12, 8, 1)):
        assert f(Cin, Cout, k) == 64 + 12 * up(Cout, 64) + 4 * up(Cout, 64) * k * k * up(Cin, 32), (Cin, Cout, k)
    for Cin, Cout, k in ((2, 16, 3), (16, 6, 3), (0, 16, 1), (16, -4, 1), (4100, 16, 3), (16, 4100, 3), (16, 16, 2), (16, 16, 5), (16, 16, 0)):
        assert f(Cin, Cout, k) == 0 and b'pw_conv2d_packed_bytes' in l.pw_last_error(), (Cin, Cout, k)
    w = l.pw_conv2d_workspace_bytes
    w.restype, w.argtypes = ctypes.c_size_t, [ctypes.c_int] * 3
    assert w(1, 1, 1) == w(6, 32, 88) == w(1000, 1000, 1000) == 1024 and w(0, 4, 4) == w(4, 0, 4) == w(4, 4, -1) == 0


def test_c_side_refuses_before_any_hip_call():
    """bad sizes, null pointers and a residual that does not go with epi never reach a HIP call: the addresses are never touched
    (there is no device here)"""
    l = _lib.lib()
    x, y = ctypes.c_void_p(1 << 30), ctypes.c_void_p(1 << 31)
    pack = l.pw_conv2d_pack
    pack.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_float, ctypes.c_void_p] + [ctypes.c_int] * 3 + [ctypes.c_void_p]
    conv = l.pw_conv2d
    conv.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_size_t] + [ctypes.c_int] * 8 + [ctypes.c_void_p]

    def call_pack(weight=x, bias=x, g=x, b=x, mean=x, var=x, eps=1e-5, packed=x, Cin=32, Cout=16, k=3):
        rc = pack(weight, bias, g, b, mean, var, eps, packed, Cin, Cout, k, None)
        msg = l.pw_last_error()
        assert rc < 0 and b'pw_conv2d_pack:' in msg, (rc, msg)
        return rc

    def call(xp=x, packed=x, res=None, out=y, wsp=x, nbytes=1 << 20, B=2, H=5, W=7, Cin=32, Cout=16, k=3, dil=1, epi=1):
        rc = conv(xp, packed, res, out, wsp, nbytes, B, H, W, Cin, Cout, k, dil, epi, None)
        msg = l.pw_last_error()
        assert rc < 0 and b'pw_conv2d:' in msg, (rc, msg)
        return rc, msg
    EUNSUP, EINVAL = _lib.PW['PW_EUNSUP'], _lib.PW['PW_EINVAL']
    for kw in (dict(Cin=2), dict(Cin=30), dict(Cin=4100), dict(Cout=2), dict(Cout=18), dict(Cout=4100), dict(Cin=0), dict(Cout=-16), dict(k=2),
               dict(k=5), dict(k=0)):
        assert call(**kw)[0] == EUNSUP and call_pack(**kw) == EUNSUP, kw
    assert b'Cin = 30' in call(Cin=30)[1]
    off = lambda n: ctypes.c_void_p((1 << 30) + n)
    for kw in (dict(xp=None), dict(packed=None), dict(out=None), dict(B=0), dict(H=0), dict(W=-3), dict(epi=3), dict(epi=-1), dict(dil=0),
               dict(dil=-2), dict(dil=5000), dict(epi=2), dict(res=x), dict(res=x, epi=0), dict(xp=off(4)), dict(out=off(8)),
               dict(packed=off(8)), dict(res=off(4), epi=2), dict(wsp=None), dict(nbytes=1023), dict(wsp=off(2)), dict(out=x),
               dict(B=1 << 15, H=1 << 15, W=4), dict(B=1 << 10, H=1 << 10, W=1 << 9, Cin=4096)):
        assert call(**kw)[0] == EINVAL, kw
    for kw in (dict(weight=None), dict(packed=None), dict(g=None), dict(var=None), dict(g=None, b=None, mean=None), dict(eps=float('nan')),
               dict(eps=-1.0), dict(packed=off(4)), dict(weight=off(2))):
        assert call_pack(**kw) == EINVAL, kw


def test_python_side_refuses():
    E = _lib.PreworldHipError
    S = ops.conv2d_supported
    assert S(512, 512, 3, 1, 1, 1, 1) is None and S(600, 512, (3, 3), (1, 1), (1, 1), (1, 1), 1) is None and S(512, 88, 1, 1, 1, 0, 1) is None
    assert S(512, 96, 3, 1, 18, 18, 1) is None and S(28, 24, 3, 1, 1, 1, 1) is None and S(4096, 4, 1) is None
    assert 'stride (2, 2)' in S(88, 88, 3, 2, 1, 1, 1) and 'groups 2' in S(64, 64, 3, 1, 1, 1, 2) and 'kernel_size (5, 5)' in S(64, 64, 5, 1, 1, 2, 1)
    assert 'kernel_size (1, 3)' in S(64, 64, (1, 3), 1, 1, (0, 1), 1) and 'padding (0, 0)' in S(64, 64, 3, 1, 1, 0, 1)
    assert 'padding (6, 6)' in S(64, 64, 3, 1, 12, 6, 1) and 'dilation (1, 2)' in S(64, 64, 3, 1, (1, 2), 1, 1)
    assert 'in_channels 3 ' in S(3, 64, 3, 1, 1, 1, 1) and 'out_channels 8192' in S(64, 8192, 1, 1, 1, 0, 1) and 'out_channels 6 ' in S(64, 6, 1)
    with pytest.raises(E, match='stride'):
        ops.conv2d_pack(nn.Conv2d(16, 16, 3, stride=2, padding=1))
    with pytest.raises(E, match='padding_mode'):
        ops.conv2d_pack(nn.Conv2d(16, 16, 3, padding=1, padding_mode='reflect'))
    with pytest.raises(E, match='BatchNorm2d over 16 channels'):
        ops.conv2d_pack(nn.Conv2d(16, 16, 3, padding=1), nn.BatchNorm2d(8))
    with pytest.raises(E, match='weight must be a contiguous float32'):
        ops.conv2d_pack(nn.Conv2d(16, 16, 3, padding=1).double())
    with pytest.raises(E, match='must be a CUDA'):                     # a host tensor is refused, never given a fallback
        ops.conv2d_pack(nn.Conv2d(16, 16, 3, padding=1), nn.BatchNorm2d(16))
    p = ops.Conv2dPacked(torch.zeros(16, dtype=torch.uint8), 16, 8, 3)
    cl = lambda *shape: torch.zeros(*shape).contiguous(memory_format=torch.channels_last)
    with pytest.raises(E, match='conv2d_pack'):
        ops.conv2d(cl(2, 16, 5, 7), torch.zeros(16, dtype=torch.uint8))
    with pytest.raises(E, match='x must be'):
        ops.conv2d(cl(2, 12, 5, 7), p)
    with pytest.raises(E, match='x must be a float32'):
        ops.conv2d(cl(2, 16, 5, 7).double(), p)
    with pytest.raises(E, match='x must be in torch.channels_last storage'):
        ops.conv2d(torch.zeros(2, 16, 5, 7), p)
    with pytest.raises(E, match='residual needs relu'):
        ops.conv2d(cl(2, 16, 5, 7), p, residual=cl(2, 8, 5, 7))
    with pytest.raises(E, match='residual must be a float32'):
        ops.conv2d(cl(2, 16, 5, 7), p, relu=True, residual=cl(2, 16, 5, 7))
    with pytest.raises(E, match='residual must be in torch.channels_last storage'):
        ops.conv2d(cl(2, 16, 5, 7), p, relu=True, residual=torch.zeros(2, 8, 5, 7))
    with pytest.raises(E, match='dilation must be'):
        ops.conv2d(cl(2, 16, 5, 7), p, dilation=0)
    with pytest.raises(E, match='must be a CUDA'):
        ops.conv2d(cl(2, 16, 5, 7), p, relu=True, residual=cl(2, 8, 5, 7))


# ------------------------------------------------------------------------------------------------------------ modules
def _fused(net):
    return [m for m in net.modules() if isinstance(m, IE._FusedConvs)]


def _toy_neck(**kw):
    return IE.FPN_LSS(in_channels=64 + 128, out_channels=24, extra_upsample=None, input_feature_index=(0, 1), scale_factor=2, **kw)


def _toy_depthnet(**kw):
    return IE.DepthNet(16, 16, 4, 12, use_dcn=False, aspp_mid_channels=8, stereo=True, bias=5.0, **kw)


def test_conv_impl_plumbing(golden):
    g = golden('image_branch_small.npz')
    for build in (_toy_neck, _toy_depthnet, lambda **kw: IE.BasicBlock2d(16, 16, **kw), lambda **kw: IE.ASPP(16, 8, **kw),
                  lambda **kw: IE._ASPPModule(16, 8, 3, 6, 6, **kw)):
        with pytest.raises(ValueError, match='conv_impl must be one of'):
            build(conv_impl='triton')
        assert build().conv_impl == 'torch' and build(conv_impl='hip').conv_impl == 'hip'
    # a layer the kernel does not take is refused where the module is built
    with pytest.raises(ValueError, match='conv1: stride'):
        IE.BasicBlock2d(16, 16, stride=2, conv_impl='hip')
    with pytest.raises(ValueError, match='downsample: groups 2'):
        IE.BasicBlock2d(16, 16, downsample=nn.Conv2d(16, 16, 1, groups=2), conv_impl='hip')
    with pytest.raises(ValueError, match='downsample: a Sequential is not an nn.Conv2d'):
        IE.BasicBlock2d(16, 16, downsample=nn.Sequential(nn.Conv2d(16, 16, 1)), conv_impl='hip')
    with pytest.raises(ValueError, match='in_channels 18'):
        IE.DepthNet(16, 16, 4, 2, use_dcn=False, aspp_mid_channels=8, stereo=True, conv_impl='hip')       # 16 + 2 input channels
    with pytest.raises(ValueError, match='out_channels 6 '):
        IE.FPN_LSS(in_channels=64, out_channels=6, extra_upsample=None, conv_impl='hip')
    assert IE.BasicBlock2d(16, 16, stride=2).conv_impl == 'torch'                                           # 'torch' takes anything
    # parameters, buffers and state-dict keys do not depend on conv_impl
    for build, keys in ((_toy_neck, 'neck_keys'), (_toy_depthnet, 'depthnet_keys')):
        hip, ref = build(conv_impl='hip'), build()
        assert sorted(hip.state_dict().keys()) == sorted(ref.state_dict().keys()) == list(g[keys])
        assert [n for n, _ in hip.named_buffers()] == [n for n, _ in ref.named_buffers()]
        assert all(m.conv_impl == 'hip' for m in _fused(hip)) and all(m.conv_impl == 'torch' for m in _fused(ref))
        ref.set_conv_impl('hip')
        assert all(m.conv_impl == 'hip' for m in _fused(ref))
        ref.set_conv_impl('torch')
        assert all(m.conv_impl == 'torch' for m in _fused(ref))
        with pytest.raises(ValueError, match='conv_impl must be one of'):
            ref.set_conv_impl('cuda')
    assert len(_fused(_toy_depthnet())) == 9                           # DepthNet, 3 BasicBlock2d, ASPP and its 4 branches
    # every fused layer of the DepthNet is listed once; cost_volumn_net and the SE convolutions are not
    names = [n for n, _ in _toy_depthnet()._fused_convs()]
    assert len(names) == len(set(names)) == 3 + 7 + 1 + 4 and not any('cost_volumn' in n or '_se' in n for n in names)
    assert 'reduce_conv.0' in names and 'depth_conv.0.downsample' in names and 'depth_conv.3.aspp4.atrous_conv' in names
    # config plumbing
    from preworld_amd import builder
    neck = builder.build(dict(type='FPN_LSS', in_channels=64 + 128, out_channels=24, extra_upsample=None, input_feature_index=(0, 1),
                              scale_factor=2, conv_impl='hip'))
    assert neck.conv_impl == 'hip'


def _toy_branch(**kw):
    from preworld_amd import synth as S
    cfg = IE.preworld_image_cfg()
    cfg['backbone_cfg'] = dict(S.small_swin_cfg(), window_size=4)
    cfg['neck_cfg'] = dict(in_channels=64 + 128, out_channels=48, extra_upsample=None, input_feature_index=(0, 1), scale_factor=2)
    cfg['in_channels'] = 48
    cfg['input_size'] = (64, 96)
    cfg.update(kw)
    return IE.ImageBranch(**cfg)


def test_image_branch_conv_impl():
    a, b = _toy_branch(), _toy_branch(conv_impl='hip')
    assert a.conv_impl == 'torch' and b.conv_impl == 'hip' and sorted(a.state_dict()) == sorted(b.state_dict())
    assert b.img_neck.conv_impl == 'hip' and all(m.conv_impl == 'hip' for m in _fused(b.img_view_transformer.depth_net))
    c = _toy_branch(depthnet_cfg=dict(use_dcn=False, aspp_mid_channels=96, stereo=True, bias=5., conv_impl='hip'))
    assert c.conv_impl == 'mixed' and c.img_neck.conv_impl == 'torch'
    c.set_conv_impl('hip')
    assert c.conv_impl == 'hip'
    c.set_conv_impl('torch')
    assert c.conv_impl == 'torch' and all(m.conv_impl == 'torch' for m in _fused(c))
    with pytest.raises(ValueError, match='conv_impl must be one of'):
        _toy_branch(conv_impl='cuda')


def test_set_conv_impl_switches_nothing_when_one_layer_is_unsupported():
    dn = _toy_depthnet()
    dn.depth_conv[1].conv2 = nn.Conv2d(16, 16, 3, padding=1, groups=4, bias=False)      # one grouped layer deep inside
    with pytest.raises(ValueError, match='depth_conv.1.conv2: groups 4'):
        dn.set_conv_impl('hip')
    assert all(m.conv_impl == 'torch' for m in _fused(dn))
    br = _toy_branch()
    br.img_view_transformer.depth_net.depth_conv[3].aspp3.atrous_conv = nn.Conv2d(48, 96, 3, padding=12, dilation=12, stride=2, bias=False)
    with pytest.raises(ValueError, match='depth_conv.3.aspp3.atrous_conv: stride'):
        br.set_conv_impl('hip')
    assert br.conv_impl == 'torch' and all(m.conv_impl == 'torch' for m in _fused(br))      # the neck, checked first, was not switched


def test_hip_in_training_mode_or_with_grad_is_the_torch_path_and_otherwise_has_no_fallback():
    from preworld_amd import synth as S
    rs_x = torch.randn(2, 16, 2, 3, generator=torch.Generator().manual_seed(0))
    mlp = torch.randn(1, 2, 27, generator=torch.Generator().manual_seed(1))
    metas = dict(cv_feat_list=[None, None], downsample=16, cv_downsample=4)
    a, b = _toy_depthnet().eval(), _toy_depthnet(conv_impl='hip').eval()
    sd = S.seeded_module_state(a, 54)
    a.load_state_dict(sd)
    b.load_state_dict(sd)
    # eval mode with grad enabled: autograd needs a backward
    ya, yb = a(rs_x, mlp, metas), b(rs_x, mlp, metas)
    assert yb.grad_fn is not None and torch.equal(ya, yb) and all(m._derived is None for m in _fused(b))
    ya.square().sum().backward()
    yb.square().sum().backward()
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p.grad, q.grad), n
    # training mode without grad: BatchNorm batch statistics
    a.train()
    b.train()
    with torch.no_grad():
        outs = []
        for net in (a, b):
            torch.manual_seed(3)                           # the ASPP's Dropout draws
            outs.append(net(rs_x, mlp, metas))
        assert torch.equal(*outs)
    for (n, p), q in zip(a.named_buffers(), b.buffers()):
        assert torch.equal(p, q), n
    # autocast
    a.eval()
    b.eval()
    with torch.no_grad(), torch.autocast('cpu', torch.bfloat16):
        assert torch.equal(a(rs_x, mlp, metas), b(rs_x, mlp, metas))
    # eval mode, no grad, no autocast: the fused path, which refuses a host tensor
    with torch.no_grad(), pytest.raises(_lib.PreworldHipError, match='must be a CUDA'):
        b(rs_x, mlp, metas)
    neck = _toy_neck(conv_impl='hip').eval()
    feats = [torch.randn(1, 64, 4, 6), torch.randn(1, 128, 2, 3)]
    assert neck(feats).grad_fn is not None
    with torch.no_grad(), pytest.raises(_lib.PreworldHipError, match='must be a CUDA'):
        neck(feats)
