"""CPU side of the fused Swin Linears' backward: the float64 yardstick of tests/_swin_linear_bwd_ref64.py against the torch modules in
double, the float32 floors of the torch path it sets for the kernels (tensor maximum and per element), the per-element unit
against the tensor maximum on a spoilt reference, the case census, the C ABI of
include/preworld_hip_swin_linear_bwd.h (parsing, refusals before any HIP call) and the linear_impl='hip_grad' plumbing."""
import ctypes
import re

import pytest
import torch

import _swin_linear_bwd_ref64 as G
import _swin_linear_ref64 as R
from preworld_amd import _lib, image_encoder as IE, ops, synth as S

FNS = {'pw_swin_linear_backward_packed_bytes', 'pw_swin_linear_backward_pack', 'pw_swin_linear_backward_rows_workspace_bytes',
       'pw_swin_linear_backward_data', 'pw_swin_linear_backward_gelu', 'pw_swin_linear_backward_weight_workspace_bytes',
       'pw_swin_linear_backward_weight', 'pw_swin_layernorm_backward_workspace_bytes', 'pw_swin_layernorm_backward'}
SIZE_FNS = {f for f in FNS if f.endswith('_bytes')}


# ------------------------------------------------------------------------------------------------------------ yardstick and floors
@pytest.mark.parametrize('name', list(G.CASES))
def test_yardstick_agrees_with_the_torch_modules_in_float64(name):
    errs = G.errors(name, G.torch_path_grads(name, torch.float64))
    assert errs and max(errs.values()) <= 1e-12, errs


@pytest.mark.parametrize('name', list(G.CASES))
def test_floor_of_the_torch_path(name):
    """the float32 backward of the torch modules meets every entry of BWD_FLOORS and the table is not loose; no gradient is zero"""
    got = G.torch_path_grads(name)
    errs = G.errors(name, got)
    ref = G.reference(name)
    assert set(errs) - {'dresidual'} == set(G.BWD_FLOORS[name])
    for k, err in errs.items():
        assert float(ref[k].abs().max()) > 0.0, (name, k)
        if k == 'dresidual':
            assert torch.equal(got[k], G.cotangent(name)), name
            continue
        floor = G.BWD_FLOORS[name][k]
        print('%s %s: torch float32 %.3e, floor %.1e' % (name, k, err, floor))
        assert 0.5 * floor <= err <= floor, (name, k, err, floor)


@pytest.mark.parametrize('name', list(G.CASES))
def test_q32_of_the_torch_path(name):
    """Q32[name][gradient] bounds the worst per-element q of the torch modules' float32 backward from above, by less than a factor of
    two; every normaliser is at least |gradient| everywhere, as a sum of absolute values must be"""
    got, ref, n = G.torch_path_grads(name), G.reference(name), G.normaliser(name)
    qs = G.q_errors(name, got)
    assert set(qs) == set(G.Q32[name]) == set(G.BWD_FLOORS[name]) and set(G.Q32) == set(G.CASES)
    for k, q in qs.items():
        assert n[k].dtype == torch.float64 and tuple(n[k].shape) == tuple(ref[k].shape), (name, k)
        assert bool((n[k] >= ref[k].abs() * (1 - 1e-12)).all()), (name, k)
        worst = float(q.max())
        print('%s %s: torch float32 worst q %.4g, mean q %.3f, Q32 %.2f, bound %.2f' % (name, k, worst, float(q.mean()), G.Q32[name][k],
                                                                                    G.bound(name, k)))
        assert 0.5 * G.Q32[name][k] <= worst <= G.Q32[name][k], (name, k, worst)
    G.check_units(name, got, 'torch float32')             # and dresidual is exactly the cotangent
    if name == 'cot_zero_rows':                           # a zero normaliser: the row must be, and is, exactly zero
        assert float(n['dx'][G.ZERO_ROW].max()) == 0.0 and float(n['dx'].min()) == 0.0 and float(qs['dx'][G.ZERO_ROW].max()) == 0.0


def test_the_unit_sees_what_the_tensor_maximum_hides():
    """the yardstick against itself on cot_rows_span's data gradient: the float64 dx with the rows whose cotangent scale is <= 2^-9
    spoilt -- g W dropped there, or the cotangent rounded to 11 significant bits there, a lost lo plane -- stays under the
    tensor-maximum bound 4 x BWD_FLOORS and is far over the per-element bound, which the clean float32 torch backward meets"""
    name = 'cot_rows_span'
    c, ref, n = G.CASES[name], G.reference(name)['dx'], G.normaliser(name)['dx']
    g, W = G.cotangent(name).double(), G.inputs(name)['weight'].double()
    low = R.span(c.M) <= R.LOW_SCALE
    assert int(low.sum()) == 16
    dropped = ref.clone()
    dropped[low] = 0.0
    rounded = torch.where(low.view(-1, 1), R.round11(g), g) @ W
    for what, out in (('g W dropped', dropped), ('11 significant bits', rounded)):
        old, q = G.rel_err(out, ref), float(R.q_of(out, ref, n).max())
        print('%s dx, %s in 16 low rows: tensor-max %.3e (bound %.3e), worst q %.4g (bound %.2f)' % (
            name, what, old, 4 * G.BWD_FLOORS[name]['dx'], q, G.bound(name, 'dx')))
        assert 0.0 < old <= 4 * G.BWD_FLOORS[name]['dx'], (what, old)
        assert q > 10 * G.bound(name, 'dx'), (what, q)
    clean = float(G.q_errors(name, G.torch_path_grads(name))['dx'].max())
    assert clean <= G.bound(name, 'dx'), clean


@pytest.mark.parametrize('name', list(R.BLOCK_CASES))
def test_block_yardstick_and_floor(name):
    errs64 = G.block_errors(name, G.block_grads(name, dtype=torch.float64)[2])
    assert max(errs64.values()) <= 1e-11, errs64
    errs = G.block_errors(name, G.block_grads(name)[2])
    assert set(errs) == set(G.BLOCK_BWD_FLOORS[name]) and len(errs) == 14
    for k, err in errs.items():
        floor = G.BLOCK_BWD_FLOORS[name][k]
        print('%s %s: torch float32 %.3e, floor %.1e' % (name, k, err, floor))
        assert 0.5 * floor <= err <= floor, (name, k, err, floor)


def test_cases_are_what_they_claim():
    C = G.CASES
    assert [k for k in R.CASES if R.CASES[k].dtype == 'f32'] + list(G.NEW_CASES) == list(C) and len(C) == 30
    assert {'w_rows_span', 'w_rows_span_ln_gelu', 'x_and_w_span'} <= set(C)          # the forward's exponent cases
    for name, dim in (('x_rows_span_wgrad', 0), ('x_cols_span_wgrad', 1)):
        c, x = C[name], G.inputs(name)['x']
        assert (c.role, c.M, c.K, c.N) == ('res', 96, 256, 256)
        amax = x.abs().amax(1 - dim)
        assert 2.0 ** 11.5 < float(amax[12] / amax[0]) < 2.0 ** 12.5 and float(amax.max() / amax.min()) > 2.0 ** 22, name
        g = G.cotangent(name).abs().amax(1)
        assert float(g.max() / g.min()) < 2.0, name                                  # a plain cotangent
    dw = G.reference('x_cols_span_wgrad')['dweight'].abs().amax(0)                   # small columns of dweight
    assert float(dw.max() / dw.min()) > 2.0 ** 22
    assert all(c.dtype == 'f32' for c in C.values())
    assert {c.role for c in C.values()} == {'ln', 'ln_gelu', 'res'}
    big = lambda M, N: -(-M // 128) * -(-N // 128) >= 128                    # the forward's tile rule, for both GEMMs it serves
    assert {big(c.M, c.N) for c in C.values()} == {False, True}              # the GELU gradient
    assert {big(c.M, c.K) for c in C.values()} == {False, True}              # the data gradient: N and K exchanged
    assert any(c.K > 1024 for c in C.values()) and any(c.N > 1024 for c in C.values())      # blocked accumulation of dx: N > 1024
    assert {c.K >= 128 and c.N >= 128 for c in C.values()} == {False, True}  # both tiles of the weight gradient
    split = _lib.PW_SWIN_LINEAR_BWD['PW_SWIN_LINEAR_BWD_SPLIT_ROWS']
    assert any(c.M > 2 * split and c.M % split for c in C.values()) and any(c.M < 64 for c in C.values())
    c = C['long_m']
    assert (c.role, c.M, c.K, c.N) == ('ln', 20011, 16, 48)
    c = C['cot_rows_span']
    g = G.cotangent('cot_rows_span')
    assert (c.role, c.M, c.K, c.N) == ('res', 96, 256, 256)
    ratio = g.abs().amax(1)[12] / g.abs().amax(1)[0]
    assert 2.0 ** 10 < float(ratio) < 2.0 ** 14
    c = C['cot_outlier_column']
    g = G.cotangent('cot_outlier_column')
    assert (c.role, c.M, c.K, c.N) == ('ln', 96, 512, 512)
    assert float(g[:, G.OUTLIER_COLUMN].abs().max()) > 200 * float(g[:, G.OUTLIER_COLUMN + 1].abs().max())
    c = C['cot_zero_rows']
    g = G.cotangent('cot_zero_rows')
    assert (c.role, c.M, c.K, c.N) == ('ln_gelu', 64, 128, 512)
    assert float(g[G.ZERO_ROW].abs().max()) == 0.0 and float(g[G.ZERO_ROW + 1].abs().max()) > 0.0
    assert float(G.reference('cot_zero_rows')['dx'][G.ZERO_ROW].abs().max()) == 0.0
    assert G.reference('no_ln_bias_zero')['dbias'] is None and G.reference('qkv_tile')['dresidual'] is None


# ------------------------------------------------------------------------------------------------------------ ABI
def test_swin_linear_bwd_header_parses_like_the_main_header():
    """include/preworld_hip_swin_linear_bwd.h (included by preworld_hip.h) under the rules of
    test_swin_linear_header_parses_like_the_main_header: every pw_*( parses, every pointer parameter has a converter, the library
    exports every name, stream comes last, every entry point cites the reference"""
    text = open(_lib.SWIN_LINEAR_BWD_HEADER_PATH).read()
    protos = _lib.parse_header(_lib.SWIN_LINEAR_BWD_HEADER_PATH)
    code = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    declared = set(re.findall(r'\b(pw_\w+)\s*\(', code))
    assert declared == set(protos) == FNS
    assert '#include "preworld_hip_swin_linear_bwd.h"' in open(_lib.HEADER_PATH).read()
    assert _lib.PW_SWIN_LINEAR_BWD == dict(PW_SWIN_LINEAR_BWD_SPLIT_ROWS=1024, PW_SWIN_LINEAR_BWD_COL_ROWS=512)
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
            assert restype is ctypes.c_size_t, fn
        else:
            assert argnames[-1] == 'stream' and restype is ctypes.c_int, fn
    for fn in FNS:
        comment = text[:text.index(fn + '(')].rsplit('/*', 1)[1]
        assert 'swin.py:' in comment or 'top of this file' in comment, fn
    assert 'mmdet3d/models/backbones/swin.py' in text and 'FFN' in text
    from preworld_amd import build
    assert 'preworld_hip_swin_linear_bwd.h' in build.ABI_HEADERS and 'pw_swin_linear_bwd.hip' in build.sources()


def _size_fn(l, name, argtypes):
    f = getattr(l, name)
    f.restype, f.argtypes = ctypes.c_size_t, argtypes
    return f


def test_size_formulas():
    l = _lib.lib()
    i, i64 = ctypes.c_int, ctypes.c_int64
    pb = _size_fn(l, 'pw_swin_linear_backward_packed_bytes', [i, i])
    fwd = _size_fn(l, 'pw_swin_linear_packed_bytes', [i, i, i])
    for K, N in ((16, 48), (128, 384), (4096, 1024)):
        assert pb(K, N) == fwd(N, K, 0) == 64 + 8 * K + 8 * N + 4 * N * K
    assert pb(24, 48) == 0 and b'pw_swin_linear_backward_packed_bytes' in l.pw_last_error()
    rows = _size_fn(l, 'pw_swin_linear_backward_rows_workspace_bytes', [i64])
    assert rows(70) == 560 and rows(0) == 0
    ww = _size_fn(l, 'pw_swin_linear_backward_weight_workspace_bytes', [i64, i, i, i])
    M, K, N = 20011, 16, 48
    rb, s = -(-M // 512), -(-M // 1024)
    assert ww(M, K, N, 0) == 16 * rb * N + 8 * rb * K + 8 * N + 8 * K + 4 * s * N * K
    assert ww(M, K, N, 1) == (8 * M + 15) // 16 * 16 + 16 * rb * N + 8 * N + 4 * s * N * K
    assert ww(M, 24, N, 0) == 0 and ww(0, K, N, 0) == 0 and ww(65536 * 1024, K, N, 0) == 0
    lw = _size_fn(l, 'pw_swin_layernorm_backward_workspace_bytes', [i64, i])
    assert lw(M, K) == (8 * M + 15) // 16 * 16 + 16 * rb * K and lw(M, 8) == 0 and lw(-1, K) == 0


def test_c_side_refuses_before_any_hip_call():
    """bad sizes, null or misaligned pointers and short workspaces never reach a HIP call: the addresses are never touched (there is
    no device here)"""
    l = _lib.lib()
    P, i, i64, f, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_size_t
    x = P(1 << 30)
    odd = P((1 << 30) + 4)
    EUNSUP, EINVAL = _lib.PW['PW_EUNSUP'], _lib.PW['PW_EINVAL']
    l.pw_swin_linear_backward_pack.argtypes = [P, P, i, i, P]
    l.pw_swin_linear_backward_data.argtypes = [P, P, P, P, sz, i64, i, i, P]
    l.pw_swin_linear_backward_gelu.argtypes = [P, P, P, P, P, sz, i64, i, i, f, P]
    l.pw_swin_linear_backward_weight.argtypes = [P, P, P, P, P, P, sz, i64, i, i, i, f, P]
    l.pw_swin_layernorm_backward.argtypes = [P, P, P, P, P, P, P, P, sz, i64, i, f, P]
    big = 1 << 44

    def refused(fn, rc_want, *args):
        rc = getattr(l, fn)(*args)
        msg = l.pw_last_error()
        assert rc == rc_want and fn.encode() + b':' in msg, (fn, args, rc, msg)

    def pack(w=x, p=x, K=128, N=384):
        return ('pw_swin_linear_backward_pack', w, p, K, N, None)

    def data(g=x, p=x, dx=x, ws=x, nb=big, M=70, K=128, N=384):
        return ('pw_swin_linear_backward_data', g, p, dx, ws, nb, M, K, N, None)

    def gelu(xp=x, p=x, dh=x, dz=x, ws=x, nb=big, M=70, K=128, N=384, eps=1e-5):
        return ('pw_swin_linear_backward_gelu', xp, p, dh, dz, ws, nb, M, K, N, eps, None)

    def weight(g=x, xp=x, p=x, dw=x, db=x, ws=x, nb=big, M=70, K=128, N=384, ln=1, eps=1e-5):
        return ('pw_swin_linear_backward_weight', g, xp, p, dw, db, ws, nb, M, K, N, ln, eps, None)

    def lnb(dxn=x, xp=x, g=x, dres=None, dx=x, dg=x, db=x, ws=x, nb=big, M=70, K=128, eps=1e-5):
        return ('pw_swin_layernorm_backward', dxn, xp, g, dres, dx, dg, db, ws, nb, M, K, eps, None)

    for call in (pack, data, gelu, weight):
        for kw in (dict(K=8), dict(K=24), dict(K=4112), dict(N=40), dict(N=4112), dict(K=0), dict(N=-16)):
            a = call(**kw)
            refused(a[0], EUNSUP, *a[1:])
    for kw in (dict(K=8), dict(K=24), dict(K=4112), dict(K=0)):
        a = lnb(**kw)
        refused(a[0], EUNSUP, *a[1:])
    need_w = 8 * 70 + 16 * 384 + 8 * 384 + 4 * 384 * 128 + 8
    assert need_w - 8 == _size_fn(l, 'pw_swin_linear_backward_weight_workspace_bytes', [i64, i, i, i])(70, 128, 384, 1)
    einval = [pack(w=None), pack(p=None), pack(p=odd), pack(w=P((1 << 30) + 2)),
              data(g=None), data(p=None), data(dx=None), data(ws=None), data(nb=559), data(M=0), data(M=-3), data(M=1 << 40), data(g=odd),
              data(dx=odd), data(p=odd), data(ws=odd),
              gelu(xp=None), gelu(p=None), gelu(dh=None), gelu(dz=None), gelu(ws=None), gelu(nb=559), gelu(M=0), gelu(M=1 << 40),
              gelu(eps=float('nan')), gelu(eps=-1.0), gelu(dh=odd), gelu(dz=odd), gelu(xp=odd),
              weight(g=None), weight(ws=None), weight(dw=None, db=None), weight(xp=None), weight(p=None), weight(M=0), weight(M=-1),
              weight(M=65536 * 1024), weight(nb=need_w - 9), weight(ws=odd), weight(g=odd), weight(dw=odd), weight(db=P((1 << 30) + 2)),
              weight(eps=float('inf')),
              lnb(dxn=None), lnb(xp=None), lnb(g=None), lnb(ws=None), lnb(dx=None, dg=None, db=None), lnb(dg=None), lnb(db=None), lnb(M=0),
              lnb(M=1 << 40), lnb(nb=8 * 70 + 16 * 128 - 1), lnb(eps=-1.0), lnb(dxn=odd), lnb(dx=odd), lnb(dres=odd), lnb(ws=odd)]
    for a in einval:
        refused(a[0], EINVAL, *a[1:])


def test_python_side_refuses():
    E = _lib.PreworldHipError
    p = ops.SwinLinearPacked(torch.zeros(16, dtype=torch.uint8), 16, 48, torch.float32)
    pt = ops.SwinLinearPacked(torch.zeros(16, dtype=torch.uint8), 48, 16, torch.float32)
    pbf = ops.SwinLinearPacked(torch.zeros(16, dtype=torch.uint8), 16, 48, torch.bfloat16)
    g, x, gamma = torch.zeros(5, 48), torch.zeros(5, 16), torch.ones(16)
    with pytest.raises(E, match='in_features 24'):
        ops.swin_linear_pack_transposed(torch.zeros(48, 24))
    with pytest.raises(E, match='must be a CUDA'):                     # a host tensor is refused, never given a fallback
        ops.swin_linear_pack_transposed(torch.zeros(48, 16))
    with pytest.raises(E, match='float32 only'):
        ops.swin_linear_backward_data(g, pbf)
    with pytest.raises(E, match='g must be'):
        ops.swin_linear_backward_data(torch.zeros(5, 32), pt)
    with pytest.raises(E, match='contiguous float32'):
        ops.swin_linear_backward_data(g.double(), pt)
    with pytest.raises(E, match='must be a CUDA'):
        ops.swin_linear_backward_data(g, pt)
    with pytest.raises(E, match='dh must be'):
        ops.swin_linear_backward_gelu(x, p, torch.zeros(5, 47))
    with pytest.raises(E, match='must be a CUDA'):
        ops.swin_linear_backward_gelu(x, p, g)
    with pytest.raises(E, match='leading dimensions'):
        ops.swin_linear_backward_weight(g, torch.zeros(4, 16))
    with pytest.raises(E, match='out_features 40'):
        ops.swin_linear_backward_weight(torch.zeros(5, 40), x)
    with pytest.raises(E, match='packed is a'):
        ops.swin_linear_backward_weight(torch.zeros(5, 64), x, p, ln=True)
    with pytest.raises(E, match='must be a CUDA'):
        ops.swin_linear_backward_weight(g, x)
    assert ops.swin_linear_backward_weight(g, x, need_weight=False, need_bias=False) == (None, None)
    with pytest.raises(E, match='gamma must be'):
        ops.swin_layernorm_backward(x, x, torch.ones(8))
    with pytest.raises(E, match='shape of x'):
        ops.swin_layernorm_backward(torch.zeros(5, 32), x, gamma)
    with pytest.raises(E, match='must be a CUDA'):
        ops.swin_layernorm_backward(x, x, gamma)
    assert ops.swin_layernorm_backward(x, x, gamma, need_x=False, need_affine=False) == (None, None, None)
    with pytest.raises(E, match='role must be'):
        ops.swin_linear_backward('gelu', g, x, p, pt)
    with pytest.raises(E, match='need packed_t'):
        ops.swin_linear_backward('res', g, x, p)
    with pytest.raises(E, match='needs gamma'):
        ops.swin_linear_backward('ln', g, x, p, pt)
    assert ops.swin_linear_backward('res', g, x, p, need_x=False, need_weight=False, need_bias=False) == (None,) * 5


# ------------------------------------------------------------------------------------------------------------ modules
def _blocks(net):
    return [m for m in net.modules() if isinstance(m, IE.SwinBlock)]


def test_linear_impl_hip_grad_plumbing():
    assert IE.LINEAR_IMPLS == ('torch', 'hip', 'hip_grad')
    for attn in ('hip', 'torch'):
        with pytest.raises(ValueError, match="needs attn_impl"):
            IE.SwinBlock(16, 2, 64, 4, False, attn_impl=attn, linear_impl='hip_grad')
        with pytest.raises(ValueError, match="needs attn_impl"):
            IE.SwinTransformer(**S.small_swin_cfg(), attn_impl=attn, linear_impl='hip_grad')
    with pytest.raises(ValueError, match='in_features 8'):
        IE.SwinBlock(8, 2, 32, 4, False, attn_impl='hip_grad', linear_impl='hip_grad')
    blk = IE.SwinBlock(16, 2, 64, 4, False, attn_impl='hip_grad', linear_impl='hip_grad')
    assert blk.linear_impl == 'hip_grad'
    seq = IE.SwinBlockSequence(16, 2, 64, 2, 4, None, attn_impl='hip_grad', linear_impl='hip_grad')
    assert all(b.linear_impl == 'hip_grad' for b in seq.blocks)
    net = IE.SwinTransformer(**S.small_swin_cfg(), attn_impl='hip_grad', linear_impl='hip_grad')
    ref = IE.SwinTransformer(**S.small_swin_cfg())
    assert sorted(net.state_dict().keys()) == sorted(ref.state_dict().keys())
    assert net.linear_impl == 'hip_grad' and all(b.linear_impl == 'hip_grad' for b in _blocks(net)) and len(_blocks(net)) == 8
    net = IE.SwinTransformer(**S.small_swin_cfg(), attn_impl='hip_grad')
    for impl in ('hip_grad', 'hip', 'torch', 'hip_grad'):
        net.set_linear_impl(impl)
        assert net.linear_impl == impl and all(b.linear_impl == impl for b in _blocks(net))
    net = IE.SwinTransformer(**S.small_swin_cfg(), attn_impl='hip')
    with pytest.raises(ValueError, match="needs attn_impl 'hip_grad'"):
        net.set_linear_impl('hip_grad')
    assert net.linear_impl == 'torch' and all(b.linear_impl == 'torch' for b in _blocks(net))
    from preworld_amd import builder
    net = builder.build_backbone(dict(type='SwinTransformer', **S.small_swin_cfg(), attn_impl='hip_grad', linear_impl='hip_grad'))
    assert net.linear_impl == 'hip_grad'


def test_set_linear_impl_switches_nothing_when_one_block_is_unsupported():
    net = IE.SwinTransformer(**S.small_swin_cfg(), attn_impl='hip_grad')
    _blocks(net)[-1].attn.set_attn_impl('hip')                         # one block whose attention has no backward
    with pytest.raises(ValueError, match='needs attn_impl'):
        net.set_linear_impl('hip_grad')
    assert net.linear_impl == 'torch' and all(b.linear_impl == 'torch' for b in _blocks(net))


def test_hip_grad_with_grad_has_no_fallback_and_hip_keeps_its_own():
    """with grad in float32 'hip_grad' goes to the kernels (a host tensor is refused, the torch path does not run); 'hip' still runs
    the torch path under grad"""
    b, x, hw = R.build_block('toy_s2', 'hip_grad', 'hip_grad')
    with pytest.raises(_lib.PreworldHipError, match='must be a CUDA'):
        b(x, hw)
    with torch.no_grad(), pytest.raises(_lib.PreworldHipError, match='must be a CUDA'):
        b(x, hw)
    a, _, _ = R.build_block('toy_s2', 'hip', 'hip')
    assert a(x, hw).grad_fn is not None and a._derived is None
