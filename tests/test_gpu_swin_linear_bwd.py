"""The backward of the fused Swin Linears on the device: include/preworld_hip_swin_linear_bwd.h through ops.SwinLinear /
ops.swin_linear_backward and through SwinBlock(attn_impl='hip_grad', linear_impl='hip_grad') against the float64 autograd yardstick of
tests/_swin_linear_bwd_ref64.py under 4 x the torch path's own CPU floors and, per element in units of 2^-24 n, under 2 Q32 + 1; the
forward's bits, same bits twice, the need_* switches,
graph capture, an in-place weight update, the toy Swin against the torch path and bf16 autocast."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _swin_linear_bwd_ref64 as G
import _swin_linear_ref64 as R
from preworld_amd import image_encoder as IE, ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _dev_inputs(name):
    i = {k: None if v is None else v.to(DEV) for k, v in G.inputs(name).items()}
    packed = ops.swin_linear_pack(i['weight'], i['bias'], i['gamma'], i['beta'])
    return G.CASES[name], i, packed, ops.swin_linear_pack_transposed(i['weight']), G.cotangent(name).to(DEV)


def _function_grads(name, dres=None):
    """every gradient of a case through ops.SwinLinear (forward and backward on the device); also returns the forward's output"""
    c, i, packed, packed_t, cot = _dev_inputs(name)
    lv = {k: None if v is None else v.clone().requires_grad_(True) for k, v in i.items()}
    out = ops.SwinLinear.apply(lv['x'], lv['weight'], lv['bias'], lv['gamma'], lv['beta'], lv['residual'], packed, packed_t, c.role, R.EPS)
    if c.role != 'res':
        out, xr = out
        assert xr.data_ptr() == lv['x'].data_ptr()
        if dres is not None:
            torch.autograd.backward([out, xr], [cot, dres])
        else:
            out.backward(cot)
    else:
        out.backward(cot)
    return out.detach(), {g: None if lv[l] is None else lv[l].grad for g, l in G.LEAVES.items()}


def _ops_backward(name, **kw):
    c, i, packed, packed_t, cot = _dev_inputs(name)
    return ops.swin_linear_backward(c.role, cot, i['x'], packed, packed_t, gamma=i['gamma'], eps=R.EPS, **kw)


@pytest.mark.parametrize('name', list(G.CASES))
def test_gradients_against_the_yardstick(name):
    c, i, packed, _, _ = _dev_inputs(name)
    out, got = _function_grads(name)
    want = ops.swin_linear(i['x'], packed, ln=c.role != 'res', eps=R.EPS, act='gelu' if c.role == 'ln_gelu' else None, residual=i['residual'])
    assert torch.equal(out, want)                                   # the forward under grad is the forward: same bits
    G.check(name, got, say='kernel')
    if name == 'cot_zero_rows':
        assert float(got['dx'][G.ZERO_ROW].abs().max()) == 0.0      # an all-zero cotangent row: exact zeros


@pytest.mark.parametrize('name', list(G.CASES))
def test_gradients_per_element_units(name):
    """every element of every gradient against its own magnitude: q = |g - g64| / (2^-24 n) under 2 Q32 + 1 + FORMAT_TERM (THE UNIT in
    tests/_swin_linear_bwd_ref64.py); dresidual is exactly the cotangent, a zero normaliser asks for an exact zero"""
    _, got = _function_grads(name)
    G.check_units(name, got, 'kernel')


@pytest.mark.parametrize('name', ['qkv_tile', 'm_tail', 'wide_n_gelu'])
def test_residual_gradient_is_folded_into_the_layernorm_gradient(name):
    """dx = dres + LayerNorm'(..): the yardstick's dx plus dres in float64.  The bound is the case's own (4 x floor of max |dx64|) for
    the LayerNorm term plus one float32 rounding (2^-24) of the sum, relative to max |dx64 + dres|"""
    c = G.CASES[name]
    dres = torch.from_numpy(np.random.RandomState(c.seed).standard_normal((c.M, c.K)).astype(np.float32))
    _, got = _function_grads(name, dres=dres.to(DEV))
    dx64 = G.reference(name)['dx']
    want = dx64 + dres.double()
    err = float((got['dx'].cpu().double() - want).abs().max())
    bound = 4 * G.BWD_FLOORS[name]['dx'] * float(dx64.abs().max()) + 2.0 ** -24 * float(want.abs().max())
    print('%s dx with dres: kernel %.3e absolute, bound %.3e' % (name, err, bound))
    assert err <= bound
    _, plain = _function_grads(name)
    for k in ('dweight', 'dbias', 'dgamma', 'dbeta'):
        assert torch.equal(got[k], plain[k]), k


@pytest.mark.parametrize('name', ['long_m', 'big_ln_gelu', 'big_deep_res', 'cot_rows_span'])
def test_two_backward_calls_give_the_same_bits(name):
    a, b = _ops_backward(name), _ops_backward(name)
    for u, v in zip(a, b):
        assert (u is None and v is None) or torch.equal(u, v), name


def test_need_switches_return_none_and_leave_the_rest_unchanged():
    for name in ('m_tail', 'toy_narrow_fc2', 'qkv_tile'):
        full = _ops_backward(name)
        ln = G.CASES[name].role != 'res'
        for kw, gone in ((dict(need_x=False), {0}), (dict(need_weight=False), {1}), (dict(need_bias=False), {2}), (dict(need_ln=False), {3, 4}),
                         (dict(need_x=False, need_ln=False), {0, 3, 4}), (dict(need_weight=False, need_bias=False), {1, 2})):
            got = _ops_backward(name, **kw)
            for j, (u, v) in enumerate(zip(got, full)):
                if j in gone or (j in (3, 4) and not ln):
                    assert u is None, (name, kw, j)
                else:
                    assert torch.equal(u, v), (name, kw, j)
        assert _ops_backward(name, need_x=False, need_weight=False, need_bias=False, need_ln=False) == (None,) * 5


def test_gelu_gradient_may_overwrite_the_hidden_gradient():
    c, i, packed, _, cot = _dev_inputs('m_tail')
    want = ops.swin_linear_backward_gelu(i['x'], packed, cot, R.EPS)
    buf = cot.clone()
    got = ops.swin_linear_backward_gelu(i['x'], packed, buf, R.EPS, out=buf)
    assert got is buf and torch.equal(got, want) and not torch.equal(want, cot)


def test_graph_capture_replays_to_the_eager_result():
    for name in ('m_tail', 'big_res', 'long_m'):
        c, i, packed, packed_t, cot = _dev_inputs(name)
        eager = ops.swin_linear_backward(c.role, cot, i['x'], packed, packed_t, gamma=i['gamma'], eps=R.EPS)
        static = torch.zeros_like(cot)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                     # one stream: no parallel branches
            got = ops.swin_linear_backward(c.role, static, i['x'], packed, packed_t, gamma=i['gamma'], eps=R.EPS)
        static.copy_(cot)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(got, eager):
            assert (a is None and b is None) or torch.equal(a, b), name


# ------------------------------------------------------------------------------------------------------------ the block
def _no_torch_path(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError('the torch Linear / LayerNorm / GELU ran')
    for fn in ('linear', 'layer_norm', 'gelu'):
        monkeypatch.setattr(F, fn, refuse)


@pytest.mark.parametrize('name', list(R.BLOCK_CASES))
def test_block_gradients_against_the_yardstick(name, monkeypatch):
    hip, x, hw = R.build_block(name, 'hip_grad', 'hip')
    with torch.no_grad():
        want = hip.to(DEV)(x.to(DEV), hw)
    _no_torch_path(monkeypatch)
    blk, y, grads = G.block_grads(name, 'hip_grad', 'hip_grad', device=DEV)
    monkeypatch.undo()
    assert torch.equal(y, want)                           # the forward under grad equals the 'hip' forward bit for bit
    errs = G.block_errors(name, grads)
    for k, err in sorted(errs.items()):
        floor = G.BLOCK_BWD_FLOORS[name][k]
        print('%s %s: kernel %.3e, bound %.3e (4 x floor %.1e)' % (name, k, err, 4 * floor, floor))
    for k, err in errs.items():
        assert err <= 4 * G.BLOCK_BWD_FLOORS[name][k], (name, k, err)
    with torch.no_grad():
        assert torch.equal(blk(x.to(DEV), hw), want)      # without grad 'hip_grad' is 'hip'


def test_frozen_parameters_and_an_input_without_grad():
    blk, x, hw = R.build_block('toy_s2', 'hip_grad', 'hip_grad')
    blk, x = blk.to(DEV), x.to(DEV)
    full = G.block_grads('toy_s2', 'hip_grad', 'hip_grad', device=DEV)[2]
    for p in (blk.norm1.weight, blk.attn.w_msa.proj.weight, blk.ffn.layers[1].bias):
        p.requires_grad_(False)
    (blk(x, hw) * G.block_cotangent('toy_s2').to(DEV)).sum().backward()      # x does not require grad
    frozen = {'norm1.weight', 'attn.w_msa.proj.weight', 'ffn.layers.1.bias'}
    for n, p in blk.named_parameters():
        if n in frozen:
            assert p.grad is None, n
        else:
            assert torch.equal(p.grad, full[n]), n


def test_gradients_follow_an_in_place_weight_update():
    name = 'tile_s6'
    blk, x, hw = R.build_block(name, 'hip_grad', 'hip_grad')
    blk, x, cot = blk.to(DEV), x.to(DEV).requires_grad_(True), G.block_cotangent(name).to(DEV)
    (blk(x, hw) * cot).sum().backward()
    first = {n: p.grad.clone() for n, p in blk.named_parameters()}
    with torch.no_grad():
        for n, p in blk.named_parameters():
            if n.endswith('weight'):
                p.mul_(1.25)                              # what an optimizer step does: same storage, new version
    blk.zero_grad(set_to_none=True)
    x.grad = None
    (blk(x, hw) * cot).sum().backward()
    fresh, _, _ = R.build_block(name, 'hip_grad', 'hip_grad')
    fresh = fresh.to(DEV)
    fresh.load_state_dict(blk.state_dict())
    x2 = x.detach().clone().requires_grad_(True)
    (fresh(x2, hw) * cot).sum().backward()
    assert torch.equal(x.grad, x2.grad)
    for (n, p), q in zip(blk.named_parameters(), fresh.parameters()):
        assert torch.equal(p.grad, q.grad), n
    assert not torch.equal(first['ffn.layers.1.weight'], blk.ffn.layers[1].weight.grad)


def test_toy_swin_parameter_gradients_against_torch():
    """the toy Swin, loss = sum of squares of the outputs: every parameter gradient of linear_impl='hip_grad' against the torch Linears
    (both with attn_impl='hip_grad') on the device, within 4 x the float32-against-float64 floor of the torch model's gradients on the
    CPU (G.TOY_FLOOR)"""
    _, want = G.toy_grads('hip_grad', 'torch', DEV)
    _, got = G.toy_grads('hip_grad', 'hip_grad', DEV)
    assert set(got) == set(want) and len(got) > 100
    worst = max((G.rel_err(got[k].cpu(), want[k].double().cpu()), k) for k in want)
    print('toy Swin: worst parameter %s %.3e, bound %.3e' % (worst[1], worst[0], 4 * G.TOY_FLOOR))
    assert worst[0] <= 4 * G.TOY_FLOOR, worst
    assert any(not torch.equal(got[k], want[k]) for k in want)    # another code path ran


def test_bf16_autocast_with_grad_is_the_torch_path():
    name = 'tile_s6'
    res = []
    for impl in ('hip_grad', 'torch'):
        blk, x, hw = R.build_block(name, 'hip_grad', impl)
        blk, x = blk.to(DEV), x.to(DEV).requires_grad_(True)
        with torch.autocast('cuda', torch.bfloat16):
            y = blk(x, hw)
        (y.float() * G.block_cotangent(name).to(DEV)).sum().backward()
        res.append((y.detach(), x.grad, [p.grad for p in blk.parameters()]))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    for a, b in zip(res[0][2], res[1][2]):
        assert torch.equal(a, b)
