"""The fused Swin window attention (pw_swin_window_attention, ops.swin_window_attention, attn_impl='hip') on the CPU side: the float64
yardstick of tests/_swin_attn_ref64.py against the existing torch module, the per-token statements of include/preworld_hip_swin.h
against the reference's own constructions, the FLOORS table, the header's ABI rules, refusals, and the module plumbing."""
import ctypes
import re

import pytest
import torch

import _swin_attn_ref64 as R
from preworld_amd import _lib, image_encoder as IE, ops, synth as S

NAMES = list(R.CASES)


@pytest.mark.parametrize('name', NAMES)
def test_yardstick_agrees_with_the_torch_module_in_float64(name):
    ref = R.reference(name)
    m, x, hw = R.attention_module(name, 'torch', dtype=torch.float64)
    with torch.no_grad():
        out = m(x, hw).view(ref.shape)
    assert out.dtype == torch.float64 and R.rel_err(out, ref) < 1e-13, R.rel_err(out, ref)


@pytest.mark.parametrize('name', NAMES)
def test_floor_of_the_torch_path(name):
    """FLOORS[name] bounds the float32 (bf16) torch path on the CPU from above"""
    ref = R.reference(name)
    m, x, hw = R.attention_module(name, 'torch')
    with torch.no_grad():
        out = m(x, hw).view(ref.shape)
    assert out.dtype == R.torch_dtype(R.CASES[name])
    err = R.rel_err(out, ref)
    print('%s: torch path %.3e, floor %.1e' % (name, err, R.FLOORS[name]))
    assert err <= R.FLOORS[name], (name, err)
    assert set(R.FLOORS) == set(R.CASES)


def test_relative_position_index_is_the_header_formula():
    """table[(r_a - r_b + ws - 1)(2 ws - 1) + (c_a - c_b + ws - 1)] == table[relative_position_index] for every window the kernel
    takes; the module's registered buffer and the yardstick's construction are the reference's"""
    for ws in range(2, ops.SWIN_MAX_WS + 1):
        n = torch.arange(ws * ws)
        r, c = n // ws, n % ws
        formula = (r[:, None] - r[None, :] + ws - 1) * (2 * ws - 1) + (c[:, None] - c[None, :] + ws - 1)
        assert torch.equal(formula, R.relative_position_index(ws)), ws
        assert torch.equal(formula, IE.WindowMSA(4, 1, (ws, ws)).relative_position_index), ws
        assert int(formula.min()) == 0 and int(formula.max()) == (2 * ws - 1) ** 2 - 1


def test_region_formula_is_the_img_mask_of_the_slice_loops():
    for ws, shift, Hp, Wp in ((12, 6, 24, 36), (12, 6, 12, 12), (7, 3, 7, 14), (4, 2, 8, 12), (4, 1, 4, 4), (5, 4, 10, 5)):
        img_mask = torch.zeros(Hp, Wp)
        cnt = 0
        for h in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            for w in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
                img_mask[h, w] = cnt
                cnt += 1
        i, j = torch.arange(Hp)[:, None], torch.arange(Wp)[None, :]
        region = 3 * ((i >= Hp - ws).long() + (i >= Hp - shift).long()) + (j >= Wp - ws).long() + (j >= Wp - shift).long()
        assert torch.equal(region, img_mask.long()), (ws, shift, Hp, Wp)


def test_cases_are_what_they_claim():
    # the peaked case reaches +-60 and stays clear of the -100 offset
    c = R.CASES['peaked_s6']
    qkv, pad, table, scale = R.inputs('peaked_s6')
    _, logits = R.swin_attn_ref64(qkv, pad, table, c.heads, c.ws, c.shift, scale, return_logits=True)
    same = logits[logits > -45]
    assert 55 < float(same.max()) < 75 and float(same.min()) < -35, (float(same.max()), float(same.min()))
    # the dynamic-range cases are exact power-of-two multiples of one draw
    base = R.inputs('tile_pad_s6')
    for name, f in (('range_2m12', 2.0 ** -12), ('range_2p8', 2.0 ** 8)):
        got = R.inputs(name)
        assert torch.equal(got[0], base[0] * f) and torch.equal(got[1], base[1] * f) and torch.equal(got[2], base[2])
    # bf16 inputs are bf16 values
    for name, c in R.CASES.items():
        if c.dtype == 'bf16':
            assert torch.equal(R.inputs(name)[0].bfloat16().float(), R.inputs(name)[0])
    # every window / head-width path of the kernel is covered: key tiles 1, 4 and 9, head widths 8, 16, 32, NULL pad vector
    assert {(c.ws * c.ws + 15) // 16 for c in R.CASES.values()} == {1, 4, 9}
    assert {c.d for c in R.CASES.values()} == {8, 16, 32} and any(not c.bias_pad for c in R.CASES.values())


def test_padded_keys_matter_on_the_reference_alone():
    """padded tokens take part as keys and values (the reference masks regions, not padding): removing them from the softmax moves
    the output by the size of the output itself (50 bounds and more), so a kernel that drops them cannot pass"""
    for name in ('padded_keys_matter', 'tile_pad_s0', 'bf16_tile_pad_s6'):
        c = R.CASES[name]
        qkv, pad, table, scale = R.inputs(name)
        dropped = R.swin_attn_ref64(qkv, pad, table, c.heads, c.ws, c.shift, scale, drop_padded_keys=True)
        moved = R.rel_err(dropped, R.reference(name))
        print('%s: dropping padded keys moves the output by %.3f of max |out| = %.0f bounds' % (name, moved, moved / (4 * R.FLOORS[name])))
        assert moved > 50 * 4 * R.FLOORS[name], (name, moved)
    assert R.rel_err(dropped, R.reference(name)) > 0.1


def test_model_floor():
    """the real-width model of the GPU test: float32 against float64 on the CPU, the floor of the 'hip' against 'torch' bound"""
    net, x = R.build_model('torch')
    net64, x64 = R.build_model('torch', torch.float64)
    with torch.no_grad():
        o32, o64 = net(x), net64(x64)
    assert len(o32) == len(R.MODEL_FLOORS) == 4
    for a, b, f in zip(o32, o64, R.MODEL_FLOORS):
        print('model output %s: %.3e, floor %.1e' % (tuple(a.shape), R.rel_err(a, b), f))
        assert R.rel_err(a, b) <= f


# ------------------------------------------------------------------------------------------------------------ ABI
def test_swin_header_parses_like_the_main_header():
    """include/preworld_hip_swin.h (included by preworld_hip.h) under the rules tests/test_abi.py and tests/test_marshal_cpu.py hold
    the main header to: every pw_*( parses, every pointer parameter has a converter, the library exports every name"""
    text = open(_lib.SWIN_HEADER_PATH).read()
    protos = _lib.parse_header(_lib.SWIN_HEADER_PATH)
    code = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    declared = set(re.findall(r'\b(pw_\w+)\s*\(', code))
    assert declared == set(protos) == {'pw_swin_window_attention'}
    assert '#include "preworld_hip_swin.h"' in open(_lib.HEADER_PATH).read()
    assert _lib.PW_SWIN == dict(PW_SWIN_F32=0, PW_SWIN_BF16=1, PW_SWIN_MAX_WS=12, PW_SWIN_MAX_HEAD_DIM=32)
    l = _lib.lib()
    for fn, (_, argtypes, argnames) in protos.items():
        assert hasattr(l, fn) and fn in _lib.protos()
        params = re.search(r'\b%s\s*\(([^;{]*?)\)\s*;' % fn, code).group(1).split(',')
        assert len(params) == len(argtypes) == len(argnames), fn
        for ptext, a, name in zip(params, argtypes, argnames):
            assert ('*' in ptext) == isinstance(a, _lib._PtrArg), (fn, name)
            if '*' in ptext:
                assert not a.table and not a.host, (fn, name)
        assert ctypes.c_void_p not in _lib._fns[fn].argtypes and argnames[-1] == 'stream', fn
    from preworld_amd import build
    assert 'preworld_hip_swin.h' in build.ABI_HEADERS and 'pw_swin_attn.hip' in build.sources()


def test_c_side_refuses_before_any_hip_call():
    """bad sizes never reach a HIP call: the addresses are never touched (there is no device here)"""
    l = _lib.lib()
    f = l.pw_swin_window_attention
    f.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 7 + [ctypes.c_float, ctypes.c_int, ctypes.c_void_p]
    x = ctypes.c_void_p(1 << 30)

    def call(qkv=x, pad=None, table=x, out=x, B=1, H=12, W=12, C=128, heads=4, ws=12, shift=6, scale=1.0, dtype=0):
        rc = f(qkv, pad, table, out, B, H, W, C, heads, ws, shift, scale, dtype, None)
        msg = l.pw_last_error()
        assert rc < 0 and b'pw_swin_window_attention' in msg, (rc, msg)
        return rc, msg
    assert call(ws=13)[0] == _lib.PW['PW_EUNSUP'] and b'window 13' in call(ws=13)[1]
    assert call(ws=1)[0] == _lib.PW['PW_EUNSUP']
    assert call(C=160, heads=4)[0] == _lib.PW['PW_EUNSUP'] and b'head width 40' in call(C=160, heads=4)[1]
    assert call(C=24, heads=4)[0] == _lib.PW['PW_EUNSUP']                   # head width 6
    assert b'dtype' in call(dtype=2)[1]
    call(qkv=None), call(table=None), call(out=None)
    call(B=0), call(H=0), call(C=130, heads=4), call(shift=12), call(shift=-1)
    call(qkv=ctypes.c_void_p((1 << 30) + 4))                                # float32 rows are read 16 bytes at a time
    call(pad=ctypes.c_void_p((1 << 30) + 2), dtype=1)


def _args(B=1, H=5, W=9, heads=2, d=8, ws=4, dtype=torch.float32):
    C = heads * d
    return [torch.zeros(B, H * W, 3 * C, dtype=dtype), torch.zeros(3 * C, dtype=dtype), torch.zeros((2 * ws - 1) ** 2, heads), H, W,
            heads, ws, 0, 1.0]


def test_python_side_refuses():
    with pytest.raises(_lib.PreworldHipError, match='window 13'):
        ops.swin_window_attention(*_args(ws=13))
    with pytest.raises(_lib.PreworldHipError, match='head width 40'):
        ops.swin_window_attention(*_args(d=40))
    with pytest.raises(_lib.PreworldHipError, match='float32 or bfloat16'):
        ops.swin_window_attention(*_args(dtype=torch.float16))
    a = _args()
    a[0] = torch.zeros(1, 45, 96)[:, :, ::2]
    with pytest.raises(_lib.PreworldHipError, match='contiguous'):
        ops.swin_window_attention(*a)
    a = _args()
    a[1] = a[1].bfloat16()
    with pytest.raises(_lib.PreworldHipError, match='pad_qkv'):
        ops.swin_window_attention(*a)
    a = _args()
    a[2] = a[2].double()
    with pytest.raises(_lib.PreworldHipError, match='bias_table'):
        ops.swin_window_attention(*a)
    a = _args()
    a[3] = 6
    with pytest.raises(_lib.PreworldHipError, match='qkv must be'):
        ops.swin_window_attention(*a)
    # everything in order but the device: _lib.call refuses host tensors before the C function is entered -- no fallback
    with pytest.raises(_lib.PreworldHipError, match='must be a CUDA'):
        ops.swin_window_attention(*_args())


# ------------------------------------------------------------------------------------------------------------ modules
def test_hip_model_keeps_the_state_dict_keys(golden):
    g = golden('image_branch_small.npz')
    net = IE.SwinTransformer(**S.small_swin_cfg(), attn_impl='hip')
    assert sorted(net.state_dict().keys()) == list(g['swin_keys'])
    assert all(m.attn_impl == 'hip' and m.w_msa.attn_impl == 'hip' for m in net.modules() if isinstance(m, IE.ShiftWindowMSA))
    assert all(hasattr(m, 'relative_position_index') for m in net.modules() if isinstance(m, IE.WindowMSA))
    torch_net = IE.SwinTransformer(**S.small_swin_cfg())
    assert torch_net.attn_impl == 'torch' and all(m.attn_impl == 'torch' for m in torch_net.modules() if isinstance(m, IE.ShiftWindowMSA))
    torch_net.set_attn_impl('hip')
    assert all(m.attn_impl == 'hip' for m in torch_net.modules() if isinstance(m, IE.ShiftWindowMSA))
    torch_net.set_attn_impl('torch')
    assert all(m.attn_impl == 'torch' for m in torch_net.modules() if isinstance(m, IE.ShiftWindowMSA))


def test_hip_through_the_registry():
    from preworld_amd import builder
    net = builder.build_backbone(dict(type='SwinTransformer', **S.small_swin_cfg(), attn_impl='hip'))
    assert isinstance(net, IE.SwinTransformer) and net.attn_impl == 'hip'
    cfg = IE.preworld_image_cfg()
    cfg['backbone_cfg'] = dict(S.small_swin_cfg(), attn_impl='hip')
    cfg['neck_cfg'] = dict(in_channels=64 + 128, out_channels=24, extra_upsample=None, input_feature_index=(0, 1), scale_factor=2)
    cfg.update(in_channels=24, input_size=(64, 96))
    assert IE.ImageBranch(**cfg).img_backbone.attn_impl == 'hip'


def test_unsupported_config_raises_at_construction():
    with pytest.raises(ValueError, match='window 14'):
        IE.SwinTransformer(**dict(S.small_swin_cfg(), window_size=14), attn_impl='hip')
    with pytest.raises(ValueError, match='head width 48'):
        IE.ShiftWindowMSA(96, 2, 7, attn_impl='hip')
    with pytest.raises(ValueError, match='head width 6'):
        IE.SwinBlock(12, 2, 48, 4, False, attn_impl='hip')
    with pytest.raises(ValueError, match='attn_impl'):
        IE.SwinTransformer(**S.small_swin_cfg(), attn_impl='triton')
    IE.SwinTransformer(**dict(S.small_swin_cfg(), window_size=14))              # the torch path takes it
    net = IE.SwinTransformer(**dict(S.small_swin_cfg(), window_size=14))
    with pytest.raises(ValueError, match='window 14'):
        net.set_attn_impl('hip')
    assert all(m.attn_impl == 'torch' for m in net.modules() if isinstance(m, IE.ShiftWindowMSA))      # nothing was switched


def test_hip_with_grad_is_the_torch_path_and_without_grad_has_no_fallback():
    """forward only: where autograd needs a backward 'hip' runs the torch path (same bits, same gradients, also without a device);
    where it does not, a host tensor is refused -- never a silent fallback"""
    torch.manual_seed(3)
    a = IE.ShiftWindowMSA(16, 2, 4, 2, attn_impl='torch')
    b = IE.ShiftWindowMSA(16, 2, 4, 2, attn_impl='hip')
    with torch.no_grad():
        a.w_msa.relative_position_bias_table.normal_(std=0.5)
    b.load_state_dict(a.state_dict())
    x = torch.randn(2, 5 * 9, 16)
    ya, yb = a(x, (5, 9)), b(x, (5, 9))
    assert torch.equal(ya, yb)
    ya.square().sum().backward()
    yb.square().sum().backward()
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p.grad, q.grad), n
    with torch.no_grad(), pytest.raises(_lib.PreworldHipError, match='must be a CUDA'):
        b(x, (5, 9))
