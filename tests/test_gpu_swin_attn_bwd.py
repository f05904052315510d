"""The backward of the fused Swin window attention on the device: pw_swin_window_attention_backward through
ops.swin_window_attention_backward and through ShiftWindowMSA(attn_impl='hip_grad') against the float64 autograd yardstick of
tests/_swin_attn_bwd_ref64.py under 4 x the torch path's own CPU floors, a module with real Linears and the toy Swin against the torch
path, the forward's bits, same bits twice, graph capture and the need_* switches."""
import pytest
import torch

import _swin_attn_bwd_ref64 as G
import _swin_attn_ref64 as R
from preworld_amd import image_encoder as IE, ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _dev_inputs(name):
    c = R.CASES[name]
    qkv, pad, table, scale = R.inputs(name)
    dt = R.torch_dtype(c)
    return c, qkv.to(DEV, dt), None if pad is None else pad.to(DEV, dt), table.to(DEV), scale, G.cotangent(name).to(DEV, dt)


def _ops_backward(name, **kw):
    c, qkv, pad, table, scale, dout = _dev_inputs(name)
    out = ops.swin_window_attention(qkv, pad, table, c.H, c.W, c.heads, c.ws, c.shift, scale)
    dqkv, dpad, dtable = ops.swin_window_attention_backward(qkv, pad, table, out, dout, c.H, c.W, c.heads, c.ws, c.shift, scale, **kw)
    return dict(dqkv=dqkv, dpad=dpad, dtable=dtable)


@pytest.mark.parametrize('name', G.NAMES)
def test_ops_backward_against_the_yardstick(name):
    c = R.CASES[name]
    got = _ops_backward(name)
    assert got['dqkv'].dtype == R.torch_dtype(c) and got['dtable'].dtype == torch.float32
    assert got['dpad'] is None or got['dpad'].dtype == torch.float32
    G.check(name, got, say='kernel')


@pytest.mark.parametrize('name', G.NAMES)
def test_module_hip_grad_against_the_yardstick(name):
    c = R.CASES[name]
    m, x, hw = R.attention_module(name, 'hip_grad', device=DEV)
    m.w_msa.relative_position_bias_table.data = R.inputs(name)[2].to(DEV)      # float32 as stored (the harness rounds it in the bf16 cases)
    if c.bias_pad:
        m.w_msa.qkv.bias.requires_grad_(True)
    m.w_msa.qkv.rows.requires_grad_(True)
    out = m(x, hw)
    (out.view(c.B, c.H, c.W, -1) * G.cotangent(name).to(DEV, out.dtype)).sum().backward()
    assert m._mask_cache == {}                                    # the torch path did not run
    with torch.no_grad():                                         # under grad the forward is the same launch as 'hip' without
        assert torch.equal(out, m(x, hw))
    rows = m.w_msa.qkv.rows.grad
    assert float(rows[0].abs().max()) == 0.0                      # the fused path reads no zero token: the pad vector is qkv.bias
    got = dict(dqkv=rows[1:].view(c.B, c.H, c.W, -1), dtable=m.w_msa.relative_position_bias_table.grad,
               dpad=m.w_msa.qkv.bias.grad.float() if c.bias_pad else None)
    G.check(name, got, say='module')


def test_module_with_real_linears_against_float64():
    """ShiftWindowMSA(128, 4, 12, 6) on a 13 x 25 map: the input gradient and every parameter gradient of 'hip_grad' on the device
    against 'torch' in float64 on the CPU, each under 4 x the float32 torch module's own error (G.MODULE_FLOORS)"""
    ref = G.module_reference()
    m, y, got = G.module_grads('hip_grad', device=DEV)
    assert m._mask_cache == {}
    mh, xh, hw, _ = G.module_case('hip', device=DEV)
    with torch.no_grad():
        assert torch.equal(y, mh(xh, hw))                         # the forward under grad is 'hip' without grad, bit for bit
    assert set(got) == set(G.MODULE_GRADS)
    for k in G.MODULE_GRADS:
        err = G.rel_err(got[k].cpu(), ref[k])
        print('module %s: hip_grad %.3e, bound %.3e' % (k, err, 4 * G.MODULE_FLOORS[k]))
        assert err <= 4 * G.MODULE_FLOORS[k], (k, err)


def test_two_backward_calls_give_the_same_bits():
    for name in ('tile_pad_s6', 'bf16_tile_pad_s6', 'narrow_d8_s2'):
        a, b = _ops_backward(name), _ops_backward(name)
        for k in G.GRADS:
            assert torch.equal(a[k], b[k]), (name, k)


def test_need_switches_return_none_and_the_same_dqkv():
    for name in ('tile_pad_s6', 'bf16_tile_pad_s6'):
        full = _ops_backward(name)
        for kw in (dict(need_pad=False), dict(need_table=False), dict(need_pad=False, need_table=False)):
            got = _ops_backward(name, **kw)
            assert torch.equal(got['dqkv'], full['dqkv']), (name, kw)
            for key, k in (('need_pad', 'dpad'), ('need_table', 'dtable')):
                if key in kw:
                    assert got[k] is None, (name, kw)
                else:
                    assert torch.equal(got[k], full[k]), (name, kw)


def test_graph_capture_replays_to_the_eager_result():
    for name in ('tile_pad_s6', 'bf16_tile_nopad_s0'):
        c, qkv, pad, table, scale, dout = _dev_inputs(name)
        out = ops.swin_window_attention(qkv, pad, table, c.H, c.W, c.heads, c.ws, c.shift, scale)
        eager = ops.swin_window_attention_backward(qkv, pad, table, out, dout, c.H, c.W, c.heads, c.ws, c.shift, scale)
        static = torch.zeros_like(dout)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                     # one stream: no parallel branches
            got = ops.swin_window_attention_backward(qkv, pad, table, out, static, c.H, c.W, c.heads, c.ws, c.shift, scale)
        static.copy_(dout)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(got, eager):
            assert (a is None and b is None) or torch.equal(a, b), name


def test_toy_swin_parameter_gradients_against_torch():
    """the toy Swin, loss = sum of squares of the outputs: every parameter gradient of 'hip_grad' against 'torch' on the device,
    within 4 x the float32-against-float64 floor of the torch model's gradients on the CPU (G.TOY_FLOOR)"""
    net, want = G.toy_grads('torch', device=DEV)
    nh, got = G.toy_grads('hip_grad', device=DEV)
    assert set(got) == set(want) and len(got) > 100
    assert all(m._mask_cache == {} for m in nh.modules() if isinstance(m, IE.ShiftWindowMSA))
    worst = max((G.rel_err(got[k].cpu(), want[k].double().cpu()), k) for k in want)
    print('toy Swin: worst parameter %s %.3e, bound %.3e' % (worst[1], worst[0], 4 * G.TOY_FLOOR))
    assert worst[0] <= 4 * G.TOY_FLOOR, worst
    assert any(not torch.equal(got[k], want[k]) for k in want)    # another code path ran
