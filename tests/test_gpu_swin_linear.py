"""The Swin blocks' fused Linears on the device: pw_swin_linear through ops.swin_linear against the float64 yardstick of
tests/_swin_linear_ref64.py under 4 x the torch modules' own CPU floor and, per element in units of 2^-24 n, under 2 Q32 + 1, SwinBlock(linear_impl='hip') against the float64 block, whole
models against the golden outputs and against 'torch' Linears, same bits twice, graph capture, the Derived cache after an in-place
update, the torch path under grad, and a NaN that stays in its row."""
import numpy as np
import pytest
import torch

import _swin_attn_ref64 as A
import _swin_linear_ref64 as R
from preworld_amd import image_encoder as IE, ops, synth as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAMES = list(R.CASES)


def _dev(t, dtype=None):
    return None if t is None else t.to(DEV, dtype)


def _operands(name):
    """a case's inputs on the device, x in the dtype the kernel reads it in"""
    c = R.CASES[name]
    d = {k: _dev(v) for k, v in R.inputs(name).items()}
    if c.dtype == 'bf16' and c.role == 'res':
        d['x'] = d['x'].bfloat16()
    return d


def _run(name, x=None, d=None):
    """(out, packed) of a case through ops.swin_linear_pack / ops.swin_linear"""
    c = R.CASES[name]
    d = _operands(name) if d is None else d
    packed = ops.swin_linear_pack(d['weight'], d['bias'], d['gamma'], d['beta'], dtype=R.torch_dtype(c))
    out = ops.swin_linear(d['x'] if x is None else x, packed, ln=c.role != 'res', eps=R.EPS, act='gelu' if c.role == 'ln_gelu' else None,
                          residual=d['residual'])
    return out, packed


@pytest.mark.parametrize('name', NAMES)
def test_ops_against_the_yardstick(name):
    c = R.CASES[name]
    ref = R.reference(name)
    out, _ = _run(name)
    assert out.dtype == R.out_dtype(c) and tuple(out.shape) == tuple(ref.shape)
    err = R.rel_err(out.cpu(), ref)
    print('%s: kernel %.3e, bound %.3e (4 x floor %.1e)' % (name, err, 4 * R.FLOORS[name], R.FLOORS[name]))
    assert bool(torch.isfinite(out).all())
    assert err <= 4 * R.FLOORS[name], (name, err)
    if c.special in ('const_row', 'zero_row'):             # the degenerate row itself, against its own magnitude
        r = R.DEGENERATE_ROW
        row_err = float((out[r].double().cpu() - ref[r]).abs().max() / ref.abs().max())
        print('%s: degenerate row %.3e' % (name, row_err))
        assert row_err <= 4 * R.FLOORS[name]


@pytest.mark.parametrize('name', NAMES)
def test_ops_per_element_units(name):
    """every element against its own magnitude: q = |out - out64| / (U n) under 2 Q32 + 1 + FORMAT_TERM (THE UNIT in
    tests/_swin_linear_ref64.py); an element whose normaliser is zero must be exact"""
    out, _ = _run(name)
    assert out.dtype == R.out_dtype(R.CASES[name]) and bool(torch.isfinite(out).all())
    R.check_units(name, out, 'kernel')


def test_range_cases_scale_exactly():
    """x, bias and residual times a power of two: the per-row exponent absorbs it, so the output bits are the same bits scaled"""
    a, b = _run('range_2m12')[0], _run('range_2p8')[0]
    assert torch.equal(a * 2.0 ** 20, b)


@pytest.mark.parametrize('name', list(R.BLOCK_CASES))
def test_block_against_the_float64_block(name):
    c = R.BLOCK_CASES[name]
    blk, x, hw = R.build_block(name, 'hip', 'hip')
    ref = R.block_ref64(x, hw, blk.state_dict(), c.heads, c.ws, c.ws // 2 if c.shift else 0)
    blk, x = blk.to(DEV), x.to(DEV)
    with torch.no_grad():
        out = blk(x, hw)
    assert blk.attn._mask_cache == {} and out.dtype == torch.float32              # the torch path did not run
    err = R.rel_err(out.cpu(), ref)
    print('block %s: fused %.3e, bound %.3e (4 x floor %.1e)' % (name, err, 4 * R.BLOCK_FLOORS[name], R.BLOCK_FLOORS[name]))
    assert err <= 4 * R.BLOCK_FLOORS[name], (name, err)


def test_block_under_autocast_runs_the_bf16_mode():
    """bf16 against the float64 block under 4 x the floor of the torch block under CPU autocast; a .bfloat16() block is refused"""
    name = 'tile_s6'
    c = R.BLOCK_CASES[name]
    blk, x, hw = R.build_block(name, 'hip', 'hip')
    ref = R.block_ref64(x, hw, blk.state_dict(), c.heads, c.ws, c.ws // 2)
    blk, x = blk.to(DEV), x.to(DEV)
    with torch.no_grad(), torch.autocast('cuda', torch.bfloat16):
        out = blk(x, hw)
    assert out.dtype == torch.float32 and blk.attn._mask_cache == {}
    err = R.rel_err(out.cpu(), ref)
    bound = 4 * R.BLOCK_FLOORS_BF16[name]
    print('block %s under autocast: %.3e, bound %.3e' % (name, err, bound))
    assert err <= bound
    with torch.no_grad(), pytest.raises(RuntimeError, match='float32'):
        blk.bfloat16()(x.bfloat16(), hw)


def test_toy_swin_hip_linears_match_the_golden_outputs(golden):
    g = golden('image_branch_small.npz')
    net = IE.SwinTransformer(**S.small_swin_cfg(), attn_impl='hip', linear_impl='hip').eval()
    net.load_state_dict(S.seeded_module_state(net, 51), strict=False)
    net = net.to(DEV)
    x = torch.from_numpy(np.random.RandomState(52).standard_normal((2, 3, 64, 96)).astype(np.float32)).to(DEV)
    with torch.no_grad():
        outs = net(x)
        ref0 = net.stereo_ref_feat(x)
    for o, k in zip(outs, ('swin_stereo', 'swin_s2', 'swin_s3')):
        np.testing.assert_allclose(o.cpu().numpy(), g[k], rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(ref0.cpu().numpy(), g['swin_ref0'], rtol=2e-4, atol=2e-5)
    assert all(m._mask_cache == {} for m in net.modules() if isinstance(m, IE.ShiftWindowMSA))
    assert all(m._derived is not None for m in net.modules() if isinstance(m, IE.SwinBlock))            # the fused path ran


def test_real_width_model_hip_linears_against_torch_linears():
    """embed_dims 128 .. 1024, hidden up to 4096: linear_impl 'hip' against 'torch' (both with attn_impl='hip') on the same device in
    float32, per output map within 4 x the float32-against-float64 difference of the torch model on the CPU
    (tests/test_swin_attn_cpu.py::test_model_floor)"""
    net, x = R.build_model('hip')
    net, x = net.to(DEV), x.to(DEV)
    with torch.no_grad():
        want = net(x)
        net.set_linear_impl('hip')
        got = net(x)
        net.set_linear_impl('torch')
        again = net(x)
    for a, b, c, f in zip(got, want, again, A.MODEL_FLOORS):
        err = R.rel_err(a.cpu(), b.double().cpu())
        print('model output %s: hip Linears against torch Linears %.3e, bound %.3e' % (tuple(a.shape), err, 4 * f))
        assert err <= 4 * f and not torch.equal(a, b)
        assert torch.equal(b, c)


def test_real_width_model_under_autocast_against_float64():
    """the fp32 model under torch.autocast(bfloat16) with fused Linears: stages 1 .. 3 receive a bf16 map from PatchMerging, which their
    first block lifts; per output map within 4 x the error of the torch model under CPU autocast, both against the float64 model"""
    net, x = R.build_model('hip', 'hip')
    net64, x64 = R.build_model('torch', dtype=torch.float64)
    with torch.no_grad():
        want = net64(x64)
        net, x = net.to(DEV), x.to(DEV)
        with torch.autocast('cuda', torch.bfloat16):
            got = net(x)
    assert all(m._mask_cache == {} for m in net.modules() if isinstance(m, IE.ShiftWindowMSA))
    assert all(m._derived is not None for m in net.modules() if isinstance(m, IE.SwinBlock))
    for a, b, f in zip(got, want, R.MODEL_FLOORS_BF16):
        err = R.rel_err(a.cpu(), b)
        print('model output %s under autocast: fused %.3e, bound %.3e' % (tuple(a.shape), err, 4 * f))
        assert err <= 4 * f


def test_two_calls_give_the_same_bits():
    for name in ('m_tail', 'toy_narrow_fc2', 'big_res', 'bf16_qkv_tile', 'bf16_big_res'):
        (a, pa), (b, pb) = _run(name), _run(name)
        assert torch.equal(a, b) and torch.equal(pa.buf, pb.buf), name


def test_graph_capture_replays_to_the_eager_result():
    for name in ('qkv_tile', 'rows_span', 'bf16_k_deep_res'):
        d = _operands(name)
        eager, _ = _run(name, d=d)
        static = torch.zeros_like(d['x'])
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                     # one stream: no parallel branches; the pack is captured too
            out, _ = _run(name, static, d)
        static.copy_(d['x'])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager), name


def test_an_in_place_weight_update_is_seen_by_the_next_forward():
    blk, x, hw = R.build_block('toy_s2', 'hip', 'hip')
    blk, x = blk.to(DEV), x.to(DEV)
    fc2 = blk.ffn.layers[1]
    with torch.no_grad():
        before = blk(x, hw)
        v = fc2.weight._version
        fc2.weight.mul_(0.5)
        blk.norm1.bias.add_(0.25)
        assert fc2.weight._version > v
        after = blk(x, hw)
        fresh, _, _ = R.build_block('toy_s2', 'hip', 'hip')
        fresh = fresh.to(DEV)
        fresh.load_state_dict(blk.state_dict())
        want = fresh(x, hw)
    assert not torch.equal(before, after) and torch.equal(after, want)


def test_with_grad_the_torch_path_runs():
    a, x, hw = R.build_block('tile_s6', 'hip', 'torch')
    b, _, _ = R.build_block('tile_s6', 'hip', 'hip')
    a, b, x = a.to(DEV), b.to(DEV), x.to(DEV)
    ya, yb = a(x, hw), b(x, hw)
    assert yb.grad_fn is not None and torch.equal(ya, yb) and b._derived is None
    with torch.no_grad():
        yk = b(x, hw)
    assert yk.grad_fn is None and not torch.equal(yk, ya) and b._derived is not None


def test_a_nan_stays_in_its_row():
    for name, row in (('qkv_tile', 37), ('rows_span', 5), ('big_res', 2000), ('bf16_qkv_tile', 100), ('bf16_big_res', 4132)):
        c, d = R.CASES[name], _operands(name)
        clean, _ = _run(name, d=d)
        x = d['x'].clone()
        x[row, 11] = float('nan')
        out, _ = _run(name, x, d)
        bad = ~torch.isfinite(out).all(dim=1)
        assert bool(bad[row]) and int(bad.sum()) == 1 and not bool(torch.isfinite(out[row]).any()), name
        keep = torch.arange(c.M, device=DEV) != row
        assert torch.equal(out[keep], clean[keep]), name
    # an Inf likewise (float32, per-row exponent path)
    d = _operands('rows_span')
    x = d['x'].clone()
    x[7, 0] = float('inf')
    out, _ = _run('rows_span', x, d)
    bad = ~torch.isfinite(out).all(dim=1)
    assert bool(bad[7]) and int(bad.sum()) == 1
