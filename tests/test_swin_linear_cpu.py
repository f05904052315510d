"""The Swin blocks' fused Linears (pw_swin_linear*, ops.swin_linear, linear_impl='hip') on the CPU side: the float64 yardstick of
tests/_swin_linear_ref64.py against the torch modules in double, the FLOORS and Q32 tables against the torch path (met, and not loose), the per-element unit against the tensor maximum on a
spoilt reference, the
header's ABI rules, refusals before any HIP call, and the module plumbing."""
import ctypes
import re

import pytest
import torch
import torch.nn.functional as F

import _swin_linear_ref64 as R
from preworld_amd import _lib, image_encoder as IE, ops, synth as S

NAMES = list(R.CASES)
FNS = {'pw_swin_linear_packed_bytes', 'pw_swin_linear_pack', 'pw_swin_linear_workspace_bytes', 'pw_swin_linear'}
SIZE_FNS = {'pw_swin_linear_packed_bytes', 'pw_swin_linear_workspace_bytes'}


# ------------------------------------------------------------------------------------------------------------ yardstick, floors
@pytest.mark.parametrize('name', NAMES)
def test_yardstick_agrees_with_the_torch_modules_in_float64(name):
    ref = R.reference(name)
    out = R.torch_path(name, torch.float64)
    assert out.dtype == torch.float64 and R.rel_err(out, ref) < 1e-12, R.rel_err(out, ref)


@pytest.mark.parametrize('name', NAMES)
def test_floor_of_the_torch_path(name):
    """FLOORS[name] bounds the float32 (autocast bf16) torch modules on the CPU from above, and by less than a factor of two"""
    out = R.torch_path(name)
    assert out.dtype == R.out_dtype(R.CASES[name])
    err = R.rel_err(out, R.reference(name))
    print('%s: torch path %.3e, floor %.1e' % (name, err, R.FLOORS[name]))
    assert 0.5 * R.FLOORS[name] <= err <= R.FLOORS[name], (name, err)
    assert set(R.FLOORS) == set(R.CASES)


@pytest.mark.parametrize('name', NAMES)
def test_q32_of_the_torch_path(name):
    """Q32[name] (and Q32_SUM for a 'ln_gelu' case) bounds the worst per-element q of the same torch path from above, by less than a
    factor of two; the normaliser is at least |out64| everywhere, as a sum of absolute values must be"""
    ref, n = R.reference(name), R.normaliser(name)
    assert n.dtype == torch.float64 and tuple(n.shape) == tuple(ref.shape) and bool((n >= ref.abs() * (1 - 1e-12)).all())
    with R.one_thread():
        out = R.torch_path(name)
    q = R.q_of(out, ref, n, R.unit(name))
    worst = float(q.max())
    print('%s: torch path worst q %.4g, mean q %.3f, Q32 %.2f, bound %.2f' % (name, worst, float(q.mean()), R.Q32[name], R.bound(name)))
    assert 0.5 * R.Q32[name] <= worst <= R.Q32[name], (name, worst)
    if R.CASES[name].role == 'ln_gelu':
        ns = R.normaliser_sum(name)
        assert bool((ns >= n * (1 - 1e-12)).all())
        worst = float(R.q_of(out, ref, ns, R.unit(name)).max())
        print('%s: torch path against n_sum worst q %.4g, Q32_SUM %.2f' % (name, worst, R.Q32_SUM[name]))
        assert 0.5 * R.Q32_SUM[name] <= worst <= R.Q32_SUM[name], (name, worst)
    assert set(R.Q32) == set(R.CASES) and set(R.Q32_SUM) == {k for k, c in R.CASES.items() if c.role == 'ln_gelu'}
    assert set(R.FORMAT_TERM) <= set(R.CASES) and R.unit(name) == (2.0 ** -9 if name.startswith('bf16_') else 2.0 ** -24)


def test_q_of_asks_for_an_exact_zero_where_the_normaliser_is_zero():
    ref, n = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64), torch.tensor([0.0, 0.0, 2.0], dtype=torch.float64)
    q = R.q_of(torch.tensor([0.0, 1e-30, 1.0 + 2.0 ** -22]), ref, n)
    assert float(q[0]) == 0.0 and float(q[1]) == float('inf') and float(q[2]) == 2.0
    assert float(R.q_of(torch.tensor([float('nan')]), ref[2:], n[2:])) == float('inf')


@pytest.mark.parametrize('name,axis', [('rows_span', 'x'), ('w_rows_span', 'weight')])
def test_the_unit_sees_what_the_tensor_maximum_hides(name, axis):
    """the yardstick against itself: the float64 output with the rows of x (the columns of the output, for the weight) whose scale is
    <= 2^-9 spoilt -- x W^T dropped there, or the operand rounded to 11 significant bits there, a lost lo plane -- stays under the
    tensor-maximum bound 4 x FLOORS and is far over the per-element bound, which the clean float32 torch path meets"""
    c, ref, n = R.CASES[name], R.reference(name), R.normaliser(name)
    d = {k: None if v is None else v.double() for k, v in R.inputs(name).items()}
    low = R.span(c.M if axis == 'x' else c.N) <= R.LOW_SCALE
    assert 0 < int(low.sum()) < len(low) // 2
    rest = d['residual'] + d['bias']
    dropped = ref.clone()
    if axis == 'x':
        dropped[low] = rest[low]
    else:
        dropped[:, low] = rest[:, low]
    d[axis] = torch.where(low.view(-1, 1), R.round11(d[axis]), d[axis])
    rounded = R.linear_ref64(c.role, **d)
    for what, out in (('x W^T dropped', dropped), ('11 significant bits', rounded)):
        old, q = R.rel_err(out, ref), float(R.q_of(out, ref, n).max())
        print('%s, %s in %d low %s: tensor-max %.3e (bound %.3e), worst q %.4g (bound %.2f)' % (
            name, what, int(low.sum()), 'rows' if axis == 'x' else 'columns', old, 4 * R.FLOORS[name], q, R.bound(name)))
        assert 0.0 < old <= 4 * R.FLOORS[name], (name, what, old)
        assert q > 10 * R.bound(name), (name, what, q)
    with R.one_thread():
        clean = float(R.q_of(R.torch_path(name), ref, n).max())
    assert clean <= R.bound(name), (name, clean)


@pytest.mark.parametrize('name', list(R.BLOCK_CASES))
def test_block_yardstick_and_floor(name):
    c = R.BLOCK_CASES[name]
    blk, x, hw = R.build_block(name)
    ref = R.block_ref64(x, hw, blk.state_dict(), c.heads, c.ws, c.ws // 2 if c.shift else 0)
    b64, x64, _ = R.build_block(name, dtype=torch.float64)
    with torch.no_grad():
        assert R.rel_err(b64(x64, hw), ref) < 1e-12
        err = R.rel_err(blk(x, hw), ref)
        print('block %s: torch path %.3e, floor %.1e' % (name, err, R.BLOCK_FLOORS[name]))
        assert 0.5 * R.BLOCK_FLOORS[name] <= err <= R.BLOCK_FLOORS[name], (name, err)
        if name in R.BLOCK_FLOORS_BF16:
            with torch.autocast('cpu', torch.bfloat16):
                err = R.rel_err(blk(x, hw), ref)
            print('block %s under autocast: torch path %.3e, floor %.1e' % (name, err, R.BLOCK_FLOORS_BF16[name]))
            assert 0.5 * R.BLOCK_FLOORS_BF16[name] <= err <= R.BLOCK_FLOORS_BF16[name], (name, err)
    assert set(R.BLOCK_FLOORS) == set(R.BLOCK_CASES)


def test_model_floor_under_autocast():
    """the real-width model of the GPU test under CPU autocast against float64: the floor of the fused bf16 model's bound"""
    net, x = R.build_model('torch')
    net64, x64 = R.build_model('torch', dtype=torch.float64)
    with torch.no_grad():
        o64 = net64(x64)
        with torch.autocast('cpu', torch.bfloat16):
            o = net(x)
    assert len(o) == len(R.MODEL_FLOORS_BF16) == 4
    for a, b, f in zip(o, o64, R.MODEL_FLOORS_BF16):
        print('model output %s: %.3e, floor %.1e' % (tuple(a.shape), R.rel_err(a, b), f))
        assert 0.5 * f <= R.rel_err(a, b) <= f


def test_cases_are_what_they_claim():
    i = R.inputs
    # exact power-of-two multiples of one draw
    for name, f in (('range_2m12', 2.0 ** -12), ('range_2p8', 2.0 ** 8)):
        base = {k: v for k, v in i(name).items()}
        other = i('range_2p8' if name == 'range_2m12' else 'range_2m12')
        g = f / (2.0 ** 8 if name == 'range_2m12' else 2.0 ** -12)
        assert torch.equal(base['x'], other['x'] * g) and torch.equal(base['residual'], other['residual'] * g)
        assert torch.equal(base['weight'], other['weight'])
    x = i('rows_span')['x']
    amax = x.abs().amax(1)
    assert float(amax.max() / amax.min()) > 2.0 ** 22
    x = i('outlier_channel_ln')['x']
    assert float(x[:, 7].abs().median() / x[:, 8].abs().median()) > 500
    assert float(i('degenerate_rows_ln')['x'][R.DEGENERATE_ROW].var()) == 0.0
    assert float(i('degenerate_rows_res')['x'][R.DEGENERATE_ROW].abs().max()) == 0.0
    assert bool(torch.isfinite(R.reference('degenerate_rows_ln')).all()) and bool(torch.isfinite(R.reference('degenerate_rows_res')).all())
    assert i('no_ln_bias_zero')['bias'] is None
    # the pre-activations of gelu_tails reach about +-8
    g = i('gelu_tails')
    pre = F.linear(F.layer_norm(g['x'], (128,), g['gamma'], g['beta'], R.EPS), g['weight'], g['bias'])
    assert 7.0 < float(pre.max()) < 12.0 and -12.0 < float(pre.min()) < -7.0
    # what the kernel reads as bf16 is bf16
    for name, c in R.CASES.items():
        if c.dtype == 'bf16' and c.role == 'res':
            assert torch.equal(i(name)['x'].bfloat16().float(), i(name)['x'])
    # both tile shapes, the blocked sum with both, every role in both modes
    big = lambda c: -(-c.M // 128) * -(-c.N // 128) >= 128
    for bf in (False, True):
        for role in ('ln', 'ln_gelu', 'res'):
            assert any((c.dtype == 'bf16') == bf and c.role == role for c in R.CASES.values()), (bf, role)
        assert {big(c) for c in R.CASES.values() if (c.dtype == 'bf16') == bf} == {False, True}
    assert {big(c) for c in R.CASES.values() if c.dtype == 'f32' and c.K > 1024} == {False, True}
    assert any(c.K == 16 for c in R.CASES.values()) and any(c.K == 4096 for c in R.CASES.values()) and any(c.N == 4096 for c in R.CASES.values())


def test_span_cases_are_what_they_claim():
    i, sp = R.inputs, R.span(256)
    assert float(sp.max() / sp.min()) == 2.0 ** 24 and torch.equal(sp[:25], torch.pow(2.0, torch.arange(-12.0, 13.0)))
    for name, (role, M, K, N) in (('w_rows_span', ('res', 96, 256, 256)), ('w_rows_span_ln_gelu', ('ln_gelu', 64, 128, 512)),
                                  ('x_and_w_span', ('res', 96, 256, 256))):
        c = R.CASES[name]
        assert (c.role, c.M, c.K, c.N, c.dtype) == (role, M, K, N, 'f32'), name
        amax = i(name)['weight'].abs().amax(1)
        assert 2.0 ** 11.5 < float(amax[12] / amax[0]) < 2.0 ** 12.5 and float(amax.max() / amax.min()) > 2.0 ** 22, name
    amax = i('w_rows_span')['x'].abs().amax(1)
    assert float(amax.max() / amax.min()) < 2.0                      # only the weight is spanned there
    d = i('x_and_w_span')
    amax = d['x'].abs().amax(1)
    assert float(amax.max() / amax.min()) > 2.0 ** 22 and d['bias'] is None
    # every element of x_and_w_span is judged at its own size: the normaliser follows the product of the two scales over 2^48 ...
    n = R.normaliser('x_and_w_span')
    scale = (R.span(96).view(-1, 1) * R.span(256).view(1, -1)).double()
    assert float(n.max() / n.min()) > 2.0 ** 44 and float((n / scale).max() / (n / scale).min()) < 64.0
    # ... while the tensor's largest element is the only size the tensor-maximum figure knows
    assert float(R.reference('x_and_w_span').abs().max() / n.min()) > 2.0 ** 40


# ------------------------------------------------------------------------------------------------------------ ABI
def test_swin_linear_header_parses_like_the_main_header():
    """include/preworld_hip_swin_linear.h (included by preworld_hip.h) under the rules tests/test_swin_attn_cpu.py holds the attention
    header to: every pw_*( parses, every pointer parameter has a converter, the library exports every name, stream comes last"""
    text = open(_lib.SWIN_LINEAR_HEADER_PATH).read()
    protos = _lib.parse_header(_lib.SWIN_LINEAR_HEADER_PATH)
    code = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    declared = set(re.findall(r'\b(pw_\w+)\s*\(', code))
    assert declared == set(protos) == FNS
    assert '#include "preworld_hip_swin_linear.h"' in open(_lib.HEADER_PATH).read()
    assert _lib.PW_SWIN_LINEAR == dict(PW_SWIN_LINEAR_EPI_BIAS=0, PW_SWIN_LINEAR_EPI_GELU=1, PW_SWIN_LINEAR_EPI_RESIDUAL=2,
                                       PW_SWIN_LINEAR_MIN_DIM=16, PW_SWIN_LINEAR_MAX_DIM=4096)
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
    # every entry point cites the reference
    for fn in FNS:
        comment = text[:text.index(fn + '(')].rsplit('/*', 1)[1]
        assert 'swin.py:' in comment or 'top of this file' in comment, fn
    assert 'mmdet3d/models/backbones/swin.py' in text and 'FFN' in text
    from preworld_amd import build
    assert 'preworld_hip_swin_linear.h' in build.ABI_HEADERS and 'pw_swin_linear.hip' in build.sources()


def test_packed_size_formula():
    l = _lib.lib()
    f = l.pw_swin_linear_packed_bytes
    f.restype, f.argtypes = ctypes.c_size_t, [ctypes.c_int] * 3
    for K, N in ((16, 16), (128, 384), (4096, 1024), (1024, 4096)):
        assert f(K, N, 0) == 64 + 8 * N + 8 * K + 4 * N * K and f(K, N, 1) == 64 + 8 * N + 8 * K + 2 * N * K
    for K, N, dt in ((8, 16, 0), (16, 24, 0), (4112, 16, 0), (16, 4112, 1), (0, 16, 0), (128, 128, 2)):
        assert f(K, N, dt) == 0 and b'pw_swin_linear_packed_bytes' in l.pw_last_error()
    w = l.pw_swin_linear_workspace_bytes
    w.restype, w.argtypes = ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int, ctypes.c_int]
    assert w(70, 1, 0) == w(70, 0, 0) == w(70, 1, 1) == 560 and w(70, 0, 1) == 0 and w(0, 1, 0) == 0 and w(1 << 33, 1, 0) == 1 << 36


def test_c_side_refuses_before_any_hip_call():
    """bad sizes and null pointers never reach a HIP call: the addresses are never touched (there is no device here)"""
    l = _lib.lib()
    x = ctypes.c_void_p(1 << 30)
    pack = l.pw_swin_linear_pack
    pack.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int] * 3 + [ctypes.c_void_p]
    gemm = l.pw_swin_linear
    gemm.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_size_t, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int, ctypes.c_int,
                     ctypes.c_void_p]

    def call_pack(weight=x, bias=x, g=x, b=x, packed=x, K=128, N=384, dtype=0):
        rc = pack(weight, bias, g, b, packed, K, N, dtype, None)
        msg = l.pw_last_error()
        assert rc < 0 and b'pw_swin_linear_pack:' in msg, (rc, msg)
        return rc

    def call(xp=x, packed=x, res=None, out=x, wsp=x, nbytes=1 << 44, M=70, K=128, N=384, ln=1, eps=1e-5, epi=0, dtype=0):
        rc = gemm(xp, packed, res, out, wsp, nbytes, M, K, N, ln, eps, epi, dtype, None)
        msg = l.pw_last_error()
        assert rc < 0 and b'pw_swin_linear:' in msg, (rc, msg)
        return rc, msg
    EUNSUP, EINVAL = _lib.PW['PW_EUNSUP'], _lib.PW['PW_EINVAL']
    for kw in (dict(K=8), dict(K=24), dict(K=4112), dict(N=8), dict(N=40), dict(N=4112), dict(K=0), dict(N=-16)):
        assert call(**kw)[0] == EUNSUP and call_pack(**kw) == EUNSUP, kw
    assert b'K = 24' in call(K=24)[1]
    for kw in (dict(xp=None), dict(packed=None), dict(out=None), dict(M=0), dict(M=-5), dict(epi=3), dict(epi=-1), dict(dtype=2),
               dict(epi=2), dict(res=x), dict(res=x, epi=1), dict(eps=float('nan')), dict(eps=-1.0),
               dict(xp=ctypes.c_void_p((1 << 30) + 4)), dict(out=ctypes.c_void_p((1 << 30) + 8)), dict(packed=ctypes.c_void_p((1 << 30) + 8)),
               dict(xp=ctypes.c_void_p((1 << 30) + 2), dtype=1, ln=0), dict(M=1 << 40), dict(wsp=None), dict(nbytes=8 * 70 - 1),
               dict(wsp=ctypes.c_void_p((1 << 30) + 4)), dict(wsp=None, nbytes=0, ln=0)):
        assert call(**kw)[0] == EINVAL, kw
    for kw in (dict(weight=None), dict(packed=None), dict(g=None), dict(b=None), dict(dtype=3), dict(packed=ctypes.c_void_p((1 << 30) + 4)),
               dict(weight=ctypes.c_void_p((1 << 30) + 2))):
        assert call_pack(**kw) == EINVAL, kw


def test_python_side_refuses():
    E = _lib.PreworldHipError
    assert ops.swin_linear_supported(128, 384) is None and ops.swin_linear_supported(4096, 1024) is None
    assert 'in_features 24' in ops.swin_linear_supported(24, 128) and 'out_features 8192' in ops.swin_linear_supported(128, 8192)
    w, b, g = torch.zeros(48, 16), torch.zeros(48), torch.ones(16)
    with pytest.raises(E, match='in_features 24'):
        ops.swin_linear_pack(torch.zeros(48, 24), b)
    with pytest.raises(E, match='dtype must be'):
        ops.swin_linear_pack(w, b, dtype=torch.float16)
    with pytest.raises(E, match='come together'):
        ops.swin_linear_pack(w, b, g, None)
    with pytest.raises(E, match='bias must be'):
        ops.swin_linear_pack(w, torch.zeros(47))
    with pytest.raises(E, match='weight must be a contiguous float32'):
        ops.swin_linear_pack(w.double(), b)
    with pytest.raises(E, match='ln_weight must be'):
        ops.swin_linear_pack(w, b, g.bfloat16(), g)
    with pytest.raises(E, match='must be a CUDA'):                     # a host tensor is refused, never given a fallback
        ops.swin_linear_pack(w, b, g, g)
    for dt in (torch.float32, torch.bfloat16):
        p = ops.SwinLinearPacked(torch.zeros(16, dtype=torch.uint8), 16, 48, dt)
        xln = torch.zeros(5, 16)
        xin = xln.to(dt)
        with pytest.raises(E, match='x must be'):
            ops.swin_linear(torch.zeros(5, 32), p, ln=True)
        with pytest.raises(E, match='x must be torch.float32'):
            ops.swin_linear(xln.double() if dt == torch.float32 else xln.bfloat16(), p, ln=True)
        with pytest.raises(E, match='contiguous'):
            ops.swin_linear(torch.zeros(5, 32, dtype=dt)[:, ::2], p)
        with pytest.raises(E, match="act must be"):
            ops.swin_linear(xin, p, act='tanh')
        with pytest.raises(E, match='exclude'):
            ops.swin_linear(xin, p, act='gelu', residual=torch.zeros(5, 48))
        with pytest.raises(E, match='residual must be'):
            ops.swin_linear(xin, p, residual=torch.zeros(5, 47))
        with pytest.raises(E, match='residual must be'):
            ops.swin_linear(xin, p, residual=torch.zeros(5, 48).bfloat16())
        with pytest.raises(E, match='must be a CUDA'):
            ops.swin_linear(xin, p, residual=torch.zeros(5, 48))
    with pytest.raises(E, match='x must be torch.bfloat16'):
        ops.swin_linear(torch.zeros(5, 16), ops.SwinLinearPacked(torch.zeros(16, dtype=torch.uint8), 16, 48, torch.bfloat16))
    with pytest.raises(E, match='swin_linear_pack'):
        ops.swin_linear(torch.zeros(5, 16), torch.zeros(16, dtype=torch.uint8))


# ------------------------------------------------------------------------------------------------------------ modules
def _blocks(net):
    return [m for m in net.modules() if isinstance(m, IE.SwinBlock)]


def test_linear_impl_plumbing(golden):
    g = golden('image_branch_small.npz')
    with pytest.raises(ValueError, match='linear_impl'):
        IE.SwinTransformer(**S.small_swin_cfg(), attn_impl='hip', linear_impl='triton')
    with pytest.raises(ValueError, match="needs attn_impl 'hip' or 'hip_grad'"):
        IE.SwinTransformer(**S.small_swin_cfg(), linear_impl='hip')
    with pytest.raises(ValueError, match="needs attn_impl"):
        IE.SwinBlock(16, 2, 64, 4, False, attn_impl='torch', linear_impl='hip')
    with pytest.raises(ValueError, match='in_features 8'):
        IE.SwinBlock(8, 2, 32, 4, False, attn_impl='hip', linear_impl='hip')
    with pytest.raises(ValueError, match='out_features 40'):
        IE.SwinBlock(16, 2, 40, 4, False, attn_impl='hip', linear_impl='hip')
    hip = IE.SwinTransformer(**S.small_swin_cfg(), attn_impl='hip', linear_impl='hip')
    ref = IE.SwinTransformer(**S.small_swin_cfg())
    assert sorted(hip.state_dict().keys()) == sorted(ref.state_dict().keys()) == list(g['swin_keys'])
    assert [n for n, _ in hip.named_buffers()] == [n for n, _ in ref.named_buffers()]
    assert hip.linear_impl == 'hip' and all(b.linear_impl == 'hip' for b in _blocks(hip)) and len(_blocks(hip)) == 8
    assert ref.linear_impl == 'torch' and all(b.linear_impl == 'torch' for b in _blocks(ref))
    for impl in ('hip_grad', 'hip'):
        net = IE.SwinTransformer(**S.small_swin_cfg(), attn_impl=impl)
        net.set_linear_impl('hip')
        assert net.linear_impl == 'hip' and all(b.linear_impl == 'hip' for b in _blocks(net))
        net.set_linear_impl('torch')
        assert net.linear_impl == 'torch' and all(b.linear_impl == 'torch' for b in _blocks(net))
    with pytest.raises(ValueError, match='linear_impl'):
        net.set_linear_impl('cuda')
    from preworld_amd import builder
    net = builder.build_backbone(dict(type='SwinTransformer', **S.small_swin_cfg(), attn_impl='hip', linear_impl='hip'))
    assert net.linear_impl == 'hip'


def test_set_linear_impl_switches_nothing_when_one_block_is_unsupported():
    net = IE.SwinTransformer(**S.small_swin_cfg(), attn_impl='hip')
    _blocks(net)[-1].attn.set_attn_impl('torch')                       # one block whose attention is not fused
    with pytest.raises(ValueError, match='needs attn_impl'):
        net.set_linear_impl('hip')
    assert net.linear_impl == 'torch' and all(b.linear_impl == 'torch' for b in _blocks(net))
    # ... or whose width the kernel does not take: embed_dims 24 -> stage widths 24, 48, 96, 192
    net = IE.SwinTransformer(**dict(S.small_swin_cfg(), embed_dims=24, num_heads=[2, 2, 4, 8]), attn_impl='hip')
    with pytest.raises(ValueError, match='in_features 24'):
        net.set_linear_impl('hip')
    assert net.linear_impl == 'torch' and all(b.linear_impl == 'torch' for b in _blocks(net))


def test_hip_with_grad_is_the_torch_path_and_without_grad_has_no_fallback():
    a, x, hw = R.build_block('toy_s2', 'hip', 'torch')
    b, _, _ = R.build_block('toy_s2', 'hip', 'hip')
    ya, yb = a(x, hw), b(x, hw)
    assert yb.grad_fn is not None and torch.equal(ya, yb) and b._derived is None
    ya.square().sum().backward()
    yb.square().sum().backward()
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p.grad, q.grad), n
    with torch.no_grad(), pytest.raises(_lib.PreworldHipError, match='must be a CUDA'):
        b(x, hw)
    with torch.no_grad(), pytest.raises(_lib.PreworldHipError, match='float32'):
        b.bfloat16()(x.bfloat16(), hw)
