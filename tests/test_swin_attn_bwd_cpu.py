"""The backward of the fused Swin window attention (pw_swin_window_attention_backward, ops.swin_window_attention_backward,
attn_impl='hip_grad') on the CPU side: the float64 autograd yardstick of tests/_swin_attn_bwd_ref64.py against the torch module, the
floor tables, what the cases cover, that the padded tokens' gradient cannot be dropped, the header's ABI rules, refusals of the C and
the Python side, and the module plumbing."""
import ctypes
import re

import pytest
import torch

import _swin_attn_bwd_ref64 as G
import _swin_attn_ref64 as R
from preworld_amd import _lib, image_encoder as IE, ops, synth as S

FN = 'pw_swin_window_attention_backward'


@pytest.mark.parametrize('name', G.NAMES)
def test_yardstick_agrees_with_the_torch_module_in_float64(name):
    ref, got = G.reference(name), G.torch_path_grads(name, dtype=torch.float64)
    for k in G.GRADS:
        if ref[k] is None:
            continue
        assert got[k].dtype == torch.float64
        if float(ref[k].abs().max()) == 0.0:
            assert float(got[k].abs().max()) == 0.0, (name, k)
        else:
            assert G.rel_err(got[k], ref[k]) < 1e-12, (name, k, G.rel_err(got[k], ref[k]))


@pytest.mark.parametrize('name', G.NAMES)
def test_floor_of_the_torch_path_backward(name):
    """BWD_FLOORS[name] bounds the float32 (bf16) torch path's backward on the CPU from above, per gradient"""
    c = R.CASES[name]
    ref, got = G.reference(name), G.torch_path_grads(name)
    assert set(G.BWD_FLOORS) == set(G.NAMES) and set(G.NAMES) <= set(R.CASES)
    assert set(G.BWD_FLOORS[name]) == {k for k in G.GRADS if ref[k] is not None}
    for k, floor in G.BWD_FLOORS[name].items():
        assert got[k].dtype == R.torch_dtype(c)
        err = G.rel_err(got[k], ref[k])
        print('%s %s: torch path %.3e, floor %s' % (name, k, err, floor))
        if floor is None:
            assert float(ref[k].abs().max()) == 0.0 and err == 0.0, (name, k)
        else:
            assert err <= floor, (name, k, err)


def test_cases_and_the_yardstick_are_what_they_claim():
    cases = [R.CASES[n] for n in G.NAMES]
    # every window / head-width path of the kernel, and the NULL pad vector
    assert {(c.ws * c.ws + 15) // 16 for c in cases} == {1, 4, 9}
    assert {c.d for c in cases} == {8, 16, 32} and any(not c.bias_pad for c in cases)
    assert {c.dtype for c in cases} == {'f32', 'bf16'} and {c.shift > 0 for c in cases} == {True, False}
    for name, c in zip(G.NAMES, cases):
        ref, C = G.reference(name), c.heads * c.d
        dout = G.cotangent(name)
        assert tuple(dout.shape) == (c.B, c.H, c.W, C)
        if c.dtype == 'bf16':
            assert torch.equal(dout.bfloat16().float(), dout)
        assert (ref['dpad'] is None) == (not c.bias_pad)
        if ref['dpad'] is not None:
            assert float(ref['dpad'][:C].abs().max()) == 0.0                        # a padded query has no output
            assert (float(ref['dpad'][C:].abs().max()) > 0.0) == G.padded(c)         # exactly zero without padding
        # every table bin receives gradient.  range_2p8: the logits span 2^16, so exp underflows to exactly 0 in float64 for some
        # pairs; there every head still has non-zero bins, and a bin it leaves at zero is non-zero in tile_pad_s6, the same draw
        # unscaled on the same map -- underflow, not a pair that is missing
        if name != 'range_2p8':
            assert bool((ref['dtable'] != 0).all()), name
        else:
            nz = ref['dtable'] != 0
            assert bool(nz.any(0).all()) and bool((G.reference('tile_pad_s6')['dtable'] != 0)[~nz].all())
            print('range_2p8: %d of %d table bins are non-zero in float64' % (int(nz.sum()), nz.numel()))
    # the pad gradient is no small term
    for name in ('tile_pad_s6', 'range_2m12'):
        ref = G.reference(name)
        assert float(ref['dpad'].abs().max()) > 5 * float(ref['dqkv'].abs().max()), name


def test_padded_tokens_gradient_cannot_be_dropped():
    """on the reference alone: without the padded positions' dk and dv, dpad (then zero) and the gradient of a qkv bias (sum of
    dqkv over the tokens + dpad) move by more than 50 bounds -- a kernel that drops the term cannot pass"""
    for name in ('padded_keys_matter', 'tile_pad_s6'):
        ref = G.reference(name)
        bound = 4 * G.BWD_FLOORS[name]['dpad']
        moved_dpad = G.rel_err(torch.zeros_like(ref['dpad']), ref['dpad'])
        dbias = ref['dqkv'].sum((0, 1, 2)) + ref['dpad']
        moved_bias = G.rel_err(ref['dqkv'].sum((0, 1, 2)), dbias)
        print('%s: dropping the padded tokens moves dpad by %.3f (%.0f bounds), d(qkv.bias) by %.3f (%.0f bounds)'
              % (name, moved_dpad, moved_dpad / bound, moved_bias, moved_bias / bound))
        assert moved_dpad > 50 * bound and moved_bias > 50 * bound, (name, moved_dpad, moved_bias)


def test_module_and_toy_floors():
    """the floors of the two whole-module GPU tests: float32 against float64 of the torch path on the CPU"""
    ref = G.module_reference()
    _, _, got = G.module_grads('torch')
    assert set(G.MODULE_FLOORS) == set(G.MODULE_GRADS) == set(got)
    for k in G.MODULE_GRADS:
        err = G.rel_err(got[k], ref[k])
        print('module %s: %.3e, floor %.1e' % (k, err, G.MODULE_FLOORS[k]))
        assert err <= G.MODULE_FLOORS[k], (k, err)
    _, g64 = G.toy_grads('torch', torch.float64)
    _, g32 = G.toy_grads('torch')
    assert set(g32) == set(g64) and len(g64) > 100
    worst = max((G.rel_err(g32[k], g64[k]), k) for k in g64)
    print('toy Swin: worst parameter %s %.3e, floor %.1e' % (worst[1], worst[0], G.TOY_FLOOR))
    assert worst[0] <= G.TOY_FLOOR, worst


# ------------------------------------------------------------------------------------------------------------ ABI
def test_bwd_header_parses_like_the_main_header():
    text = open(_lib.SWIN_BWD_HEADER_PATH).read()
    protos = _lib.parse_header(_lib.SWIN_BWD_HEADER_PATH)
    code = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    declared = set(re.findall(r'\b(pw_\w+)\s*\(', code))
    assert declared == set(protos) == {FN}
    assert '#include "preworld_hip_swin_bwd.h"' in open(_lib.HEADER_PATH).read()
    assert _lib.PW_SWIN_BWD == dict(PW_SWIN_BWD_PAD_SLOTS=64)
    l = _lib.lib()
    for fn, (_, argtypes, argnames) in protos.items():
        assert hasattr(l, fn) and fn in _lib.protos()
        params = re.search(r'\b%s\s*\(([^;{]*?)\)\s*;' % fn, code).group(1).split(',')
        assert len(params) == len(argtypes) == len(argnames) == 20, fn
        for ptext, a, name in zip(params, argtypes, argnames):
            assert ('*' in ptext) == isinstance(a, _lib._PtrArg), (fn, name)
            if '*' in ptext:
                assert not a.table and not a.host, (fn, name)
        assert ctypes.c_void_p not in _lib._fns[fn].argtypes and argnames[-1] == 'stream', fn
    from preworld_amd import build
    assert 'preworld_hip_swin_bwd.h' in build.ABI_HEADERS and 'pw_swin_attn_bwd.hip' in build.sources()
    # the forward header is still its one entry point and its constants
    assert set(_lib.parse_header(_lib.SWIN_HEADER_PATH)) == {'pw_swin_window_attention'}
    assert _lib.PW_SWIN == dict(PW_SWIN_F32=0, PW_SWIN_BF16=1, PW_SWIN_MAX_WS=12, PW_SWIN_MAX_HEAD_DIM=32)


def test_workspace_formula():
    assert ops.swin_backward_workspace_bytes(2, 13, 25, 4, 12) == 4 * 2 * 2 * 3 * 4 * (529 + 64)
    assert ops.swin_backward_workspace_bytes(12, 128, 352, 4, 12) == 4 * 12 * 11 * 30 * 4 * 593      # stage 0 of the real model: 37.6 MB


def test_c_side_refuses_before_any_hip_call():
    """bad arguments never reach a HIP call: the addresses are never touched (there is no device here)"""
    l = _lib.lib()
    f = getattr(l, FN)
    f.argtypes = [ctypes.c_void_p] * 9 + [ctypes.c_int64] + [ctypes.c_int] * 7 + [ctypes.c_float, ctypes.c_int, ctypes.c_void_p]
    x = ctypes.c_void_p(1 << 30)
    big = 1 << 40

    def call(qkv=x, pad=x, table=x, out=x, dout=x, dqkv=x, dpad=x, dtab=x, wsp=x, nbytes=big, B=1, H=12, W=12, C=128, heads=4, ws=12,
             shift=6, scale=1.0, dtype=0):
        rc = f(qkv, pad, table, out, dout, dqkv, dpad, dtab, wsp, nbytes, B, H, W, C, heads, ws, shift, scale, dtype, None)
        msg = l.pw_last_error()
        assert rc < 0 and FN.encode() in msg, (rc, msg)
        return rc, msg
    assert call(ws=13)[0] == _lib.PW['PW_EUNSUP'] and b'window 13' in call(ws=13)[1]
    assert call(ws=1)[0] == _lib.PW['PW_EUNSUP']
    assert call(C=160, heads=4)[0] == _lib.PW['PW_EUNSUP'] and b'head width 40' in call(C=160, heads=4)[1]
    assert call(C=24, heads=4)[0] == _lib.PW['PW_EUNSUP']                   # head width 6
    assert b'dtype' in call(dtype=2)[1]
    for k in ('qkv', 'table', 'out', 'dout', 'dqkv'):
        assert call(**{k: None})[0] == _lib.PW['PW_EINVAL'], k
    call(B=0), call(H=0), call(C=130, heads=4), call(shift=12), call(shift=-1)
    for k in ('qkv', 'out', 'dout', 'dqkv', 'pad'):                         # float32 rows are read and written 16 bytes at a time
        assert b'aligned' in call(**{k: ctypes.c_void_p((1 << 30) + 4)})[1], k
    assert b'aligned' in call(dout=ctypes.c_void_p((1 << 30) + 2), dtype=1)[1]
    for k in ('dpad', 'dtab', 'wsp'):
        assert b'aligned' in call(**{k: ctypes.c_void_p((1 << 30) + 2)})[1], k
    need = ops.swin_backward_workspace_bytes(1, 12, 12, 4, 12)
    assert b'workspace' in call(nbytes=need - 1)[1] and b'workspace' in call(wsp=None)[1]
    assert b'workspace' in call(nbytes=need - 1, dpad=None)[1] and b'workspace' in call(nbytes=need - 1, dtab=None, wsp=None)[1]
    assert b'pad_qkv is NULL' in call(pad=None)[1]                           # dpad_qkv given with pad_qkv NULL


def _args(B=1, H=5, W=9, heads=2, d=8, ws=4, dtype=torch.float32):
    C = heads * d
    return [torch.zeros(B, H * W, 3 * C, dtype=dtype), torch.zeros(3 * C, dtype=dtype), torch.zeros((2 * ws - 1) ** 2, heads),
            torch.zeros(B, H * W, C, dtype=dtype), torch.zeros(B, H * W, C, dtype=dtype), H, W, heads, ws, 0, 1.0]


def test_python_side_refuses():
    f = ops.swin_window_attention_backward
    with pytest.raises(_lib.PreworldHipError, match='window 13'):
        f(*_args(ws=13))
    with pytest.raises(_lib.PreworldHipError, match='head width 40'):
        f(*_args(d=40))
    with pytest.raises(_lib.PreworldHipError, match='float32 or bfloat16'):
        f(*_args(dtype=torch.float16))
    a = _args()
    a[0] = torch.zeros(1, 45, 96)[:, :, ::2]
    with pytest.raises(_lib.PreworldHipError, match='contiguous'):
        f(*a)
    a = _args()
    a[1] = a[1].bfloat16()
    with pytest.raises(_lib.PreworldHipError, match='pad_qkv'):
        f(*a)
    a = _args()
    a[2] = a[2].double()
    with pytest.raises(_lib.PreworldHipError, match='bias_table'):
        f(*a)
    a = _args()
    a[3] = a[3].bfloat16()
    with pytest.raises(_lib.PreworldHipError, match='out must be'):
        f(*a)
    a = _args()
    a[4] = torch.zeros(1, 45, 32)[:, :, ::2]
    with pytest.raises(_lib.PreworldHipError, match='dout must be'):
        f(*a)
    a = _args()
    a[5] = 6
    with pytest.raises(_lib.PreworldHipError, match='qkv must be'):
        f(*a)
    # everything in order but the device: _lib.call refuses host tensors before the C function is entered -- no fallback
    with pytest.raises(_lib.PreworldHipError, match='must be a CUDA'):
        f(*_args())
    with pytest.raises(_lib.PreworldHipError, match='must be a CUDA'):
        f(*_args(), need_pad=False, need_table=False)


# ------------------------------------------------------------------------------------------------------------ modules
def test_hip_grad_is_accepted_everywhere_and_keeps_the_state_dict_keys(golden):
    assert IE.ATTN_IMPLS == ('torch', 'hip', 'hip_grad')
    g = golden('image_branch_small.npz')
    assert IE.WindowMSA(16, 2, (4, 4), attn_impl='hip_grad').attn_impl == 'hip_grad'
    assert IE.ShiftWindowMSA(16, 2, 4, 2, attn_impl='hip_grad').attn_impl == 'hip_grad'
    assert IE.SwinBlock(16, 2, 64, 4, True, attn_impl='hip_grad').attn.attn_impl == 'hip_grad'
    assert IE.SwinBlockSequence(16, 2, 64, 2, 4, None, attn_impl='hip_grad').blocks[1].attn.w_msa.attn_impl == 'hip_grad'
    net = IE.SwinTransformer(**S.small_swin_cfg(), attn_impl='hip_grad')
    assert net.attn_impl == 'hip_grad' and sorted(net.state_dict().keys()) == list(g['swin_keys'])
    blocks = [m for m in net.modules() if isinstance(m, IE.ShiftWindowMSA)]
    assert blocks and all(m.attn_impl == 'hip_grad' and m.w_msa.attn_impl == 'hip_grad' for m in blocks)
    for impl in ('torch', 'hip_grad', 'hip', 'hip_grad'):
        net.set_attn_impl(impl)
        assert net.attn_impl == impl and all(m.attn_impl == impl and m.w_msa.attn_impl == impl for m in blocks)


def test_hip_grad_through_the_registry():
    from preworld_amd import builder
    net = builder.build_backbone(dict(type='SwinTransformer', **S.small_swin_cfg(), attn_impl='hip_grad'))
    assert isinstance(net, IE.SwinTransformer) and net.attn_impl == 'hip_grad'
    cfg = IE.preworld_image_cfg()
    cfg['backbone_cfg'] = dict(S.small_swin_cfg(), attn_impl='hip_grad')
    cfg['neck_cfg'] = dict(in_channels=64 + 128, out_channels=24, extra_upsample=None, input_feature_index=(0, 1), scale_factor=2)
    cfg.update(in_channels=24, input_size=(64, 96))
    assert IE.ImageBranch(**cfg).img_backbone.attn_impl == 'hip_grad'


def test_unsupported_config_raises_at_construction():
    with pytest.raises(ValueError, match='window 14'):
        IE.SwinTransformer(**dict(S.small_swin_cfg(), window_size=14), attn_impl='hip_grad')
    with pytest.raises(ValueError, match="attn_impl='hip_grad'.*head width 48"):
        IE.ShiftWindowMSA(96, 2, 7, attn_impl='hip_grad')
    with pytest.raises(ValueError, match='head width 6'):
        IE.SwinBlock(12, 2, 48, 4, False, attn_impl='hip_grad')
    net = IE.SwinTransformer(**dict(S.small_swin_cfg(), window_size=14))
    with pytest.raises(ValueError, match='window 14'):
        net.set_attn_impl('hip_grad')
    assert all(m.attn_impl == 'torch' for m in net.modules() if isinstance(m, IE.ShiftWindowMSA))      # nothing was switched


def test_hip_grad_has_no_fallback_with_or_without_grad():
    """with grad enabled on host tensors 'hip_grad' is refused ('hip' still runs the torch path there); without grad it is 'hip'"""
    torch.manual_seed(3)
    a = IE.ShiftWindowMSA(16, 2, 4, 2, attn_impl='torch')
    b = IE.ShiftWindowMSA(16, 2, 4, 2, attn_impl='hip')
    c = IE.ShiftWindowMSA(16, 2, 4, 2, attn_impl='hip_grad')
    b.load_state_dict(a.state_dict())
    c.load_state_dict(a.state_dict())
    x = torch.randn(2, 5 * 9, 16)
    assert torch.equal(a(x, (5, 9)), b(x, (5, 9)))
    with pytest.raises(_lib.PreworldHipError, match='must be a CUDA'):
        c(x, (5, 9))
    with torch.no_grad(), pytest.raises(_lib.PreworldHipError, match='must be a CUDA'):
        c(x, (5, 9))
    assert c._mask_cache == {} and len(b._mask_cache) == 1
