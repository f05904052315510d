"""GPU: the gradient of the Lift-Splat-Shoot voxel pooling (pw_bev_pool_v2_backward behind ops.QuickCumsumCuda.backward) and the
training forward (pw_bev_pool_v2_forward) at every kernel width, against the float64 restatement of tests/_pool_ref64.py.

Every output element is compared.  The tolerance is the derived one stated in _pool_ref64.py, |got - ref64| <= 2 (n + 2) 2^-24 S
with n the number of summed products and S the sum of their absolute values; an element without a term must be exactly 0.0.  The
[parity] lines print the worst err / bound of each comparison: a record, not a threshold."""
import ctypes

import numpy as np
import pytest
import torch

import _pool_ref64 as R
from preworld_amd import _lib, modules as M, ops, synth as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -777216.5                 # exact in fp32; no sum of the test data comes near it


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.to(dtype) if dtype is not None else t


def offset_view(t, fill=None):
    """t's contents (or `fill`) in a contiguous view that starts 4 bytes into a larger buffer: not 16-byte aligned"""
    big = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    v = big[1:].view(t.shape)
    if fill is None:
        v.copy_(t)
    else:
        v.fill_(fill)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def make_inputs(seed, ranks, C):
    rs = np.random.RandomState(seed)
    depth = rs.random_sample(ranks.BN * ranks.D * ranks.HW).astype(np.float32)       # (B*N*D*H*W,)
    feat = rs.standard_normal((ranks.BN * ranks.HW, C)).astype(np.float32)           # (B*N*H*W, C)
    og = rs.standard_normal((ranks.n_vox, C)).astype(np.float32)                     # (n_vox, C)
    return depth, feat, og


def run_abi(ranks, depth, feat, og, misalign=()):
    """forward and backward through the C ABI (ops.bev_pool_v2_forward / _backward), the backward intervals from the numpy
    restatement of the host side.  Every output buffer is pre-filled with a sentinel.  misalign: names among 'feat',
    'out_grad', 'feat_grad', 'out' to hand over as 4-byte-offset views.  Returns numpy (out, depth_grad, feat_grad)."""
    C = feat.shape[-1]
    d, f, g = T(depth), T(feat), T(og)
    if 'feat' in misalign:
        f = offset_view(f)
    if 'out_grad' in misalign:
        g = offset_view(g)
    out = torch.full((ranks.n_vox, C), SENTINEL, device=DEV)
    if 'out' in misalign:
        out = offset_view(out, SENTINEL)
    ops.bev_pool_v2_forward(d, f, out, T(ranks.ranks_depth), T(ranks.ranks_feat), T(ranks.ranks_bev), T(ranks.interval_lengths),
                            T(ranks.interval_starts))
    rd, rf, rb, st, ln = R.backward_intervals(ranks.ranks_depth, ranks.ranks_feat, ranks.ranks_bev)
    dg = torch.full_like(d, SENTINEL)
    fg = torch.full((feat.shape[0], C), SENTINEL, device=DEV)
    if 'feat_grad' in misalign:
        fg = offset_view(fg, SENTINEL)
    ops.bev_pool_v2_backward(g, dg, fg, d, f, T(rd), T(rf), T(rb), T(ln), T(st))
    torch.cuda.synchronize()
    return out.cpu().numpy(), dg.cpu().numpy(), fg.cpu().numpy()


def run_autograd(ranks, depth, feat, og):
    """ops.bev_pool_v2 (QuickCumsumCuda): the gradient handed over in the (B, C, Z, Y, X) view, i.e. permuted against the
    channels-last buffer, so the wrapper's .contiguous() works.  Returns numpy (out (n_vox, C), depth_grad, feat_grad)."""
    C = feat.shape[-1]
    d, f = T(depth).requires_grad_(), T(feat).requires_grad_()
    bev = ops.bev_pool_v2(d, f, T(ranks.ranks_depth), T(ranks.ranks_feat), T(ranks.ranks_bev), (1, 1, 1, ranks.n_vox, C),
                          T(ranks.interval_starts), T(ranks.interval_lengths))
    assert tuple(bev.shape) == (1, C, 1, 1, ranks.n_vox)
    g = T(np.ascontiguousarray(og.T)).view(1, C, 1, 1, ranks.n_vox)
    bev.backward(g)
    torch.cuda.synchronize()
    return bev.detach().permute(0, 2, 3, 4, 1).reshape(-1, C).cpu().numpy(), d.grad.cpu().numpy(), f.grad.cpu().numpy()


def check_abi_writes(name, got, ref):
    """the raw ABI writes exactly where it belongs: positions (rows) without a term still hold the sentinel, the others are
    within the bound"""
    for key, g in zip(('out', 'depth_grad', 'feat_grad'), got):
        r, n, s = getattr(ref, key), ref.n[key], ref.S[key]
        untouched = np.asarray(n).reshape(r.shape) == 0
        assert np.all(g.reshape(r.shape)[untouched] == np.float32(SENTINEL)), (name, key, 'a write where no point names one')
        assert not np.any(g.reshape(r.shape)[~untouched] == np.float32(SENTINEL)), (name, key, 'a named position was not written')
        k = ~untouched
        R.assert_within_bound('%s abi %s' % (name, key), g.reshape(r.shape)[k], r[k], np.asarray(n).reshape(r.shape)[k], s[k])


def check_autograd(name, got, ref):
    for key, g in zip(('out', 'depth_grad', 'feat_grad'), got):
        R.assert_within_bound('%s autograd %s' % (name, key), g, getattr(ref, key), ref.n[key], ref.S[key])


def check_both(name, ranks, depth, feat, og, ref):
    abi = run_abi(ranks, depth, feat, og)
    check_abi_writes(name, abi, ref)
    auto = run_autograd(ranks, depth, feat, og)
    check_autograd(name, auto, ref)
    # the wrapper's device sort and zero-filled gradients feed the same kernel the same intervals: same bits where written
    for key, a, b in zip(('out', 'depth_grad', 'feat_grad'), abi, auto):
        k = np.asarray(ref.n[key]).reshape(a.shape) > 0
        assert np.array_equal(a[k], b[k]), (name, key, 'ABI and autograd wrapper disagree')
    return abi, auto


# ------------------------------------------------------------------------------------------ every dispatch target
def _dispatch_ranks():
    """4 cameras x 83 pixels x 16 bins: ~300 backward intervals (an odd number: partial last wave at every width, several
    blocks from L = 1 on), 61 voxels with ~40 points each (forward intervals longer than the 8-point unroll)"""
    D, BN, HW = 16, 4, 83
    rs = np.random.RandomState(41)
    ln = rs.randint(1, D + 1, (BN, HW))
    ln[rs.random_sample((BN, HW)) < 0.1] = 0
    if np.count_nonzero(ln) % 2 == 0:
        ln[0, np.flatnonzero(ln[0])[0]] = 0
    return R.build_ranks(ln, D, 61, seed=42)


TEMPLATE_C = [4, 8, 16, 32, 64, 128, 256]        # k_pool_bwd<L> / k_pool_intervals<L>, L = C / 4 = 1 .. 64
GENERIC_C = [1, 12, 80, 512]                    # not a multiple of 4; a multiple of 4 with an unsupported L (3, 20); C > 256


@pytest.mark.parametrize('C', TEMPLATE_C + GENERIC_C)
def test_every_dispatch_target(C):
    ranks = _dispatch_ranks()
    n_int = len(np.unique(ranks.ranks_feat))
    assert n_int % 2 == 1 and n_int > 256 and len(ranks.interval_starts) == 61
    depth, feat, og = make_inputs(C, ranks, C)
    ref = R.pool_ref64(depth, feat, og, ranks.ranks_depth, ranks.ranks_feat, ranks.ranks_bev)
    kind = 'k_pool_bwd<%d>' % (C // 4) if C in TEMPLATE_C else 'k_pool_bwd_generic'
    check_both('C=%d %s' % (C, kind), ranks, depth, feat, og, ref)


@pytest.mark.parametrize('which', ['feat', 'out_grad', 'feat_grad', 'out'])
def test_alignment_fallback_equals_the_aligned_run(which):
    """C = 32 with one operand 4 bytes off a 16-byte boundary: the float4 kernels cannot run, the scalar ones take over --
    silently, so the result must not depend on it: equal to the aligned run to the bit ('out' misaligns the forward)."""
    ranks = _dispatch_ranks()
    depth, feat, og = make_inputs(32, ranks, 32)
    ref = R.pool_ref64(depth, feat, og, ranks.ranks_depth, ranks.ranks_feat, ranks.ranks_bev)
    want = run_abi(ranks, depth, feat, og)
    got = run_abi(ranks, depth, feat, og, misalign=(which,))
    check_abi_writes('C=32 misaligned %s' % which, got, ref)
    for key, a, b in zip(('out', 'depth_grad', 'feat_grad'), got, want):
        assert np.array_equal(a, b), 'misaligned %s: %s differs from the aligned run in %d elements' % (which, key, int((a != b).sum()))


# ------------------------------------------------------------------------------------------ interval shapes inside one wave
D88 = 88


def _shape_profile(kind):
    """per-pixel interval lengths for 3 cameras x 19 pixels of 88 depth bins"""
    BN, HW = 3, 19
    n = BN * HW
    if kind == 'long_next_to_short':
        ln = np.where(np.arange(n) % 2 == 0, 88, 1)
    elif kind == 'equal_runs':
        ln = np.repeat([5, 17, 88, 1, 40, 8, 9, 64], 8)[:n]
    elif kind == 'one_long_among_ones':
        ln = np.ones(n, np.int64)
        ln[13] = 88
    elif kind == 'holes':
        rs = np.random.RandomState(8)
        ln = rs.randint(1, 89, n)
        ln[::3] = 0                                   # first pixel empty ...
        ln[-1] = 0                                    # ... and the last one
        ln[[4, 5]] = (88, 1)
    else:
        assert kind == 'single'
        ln = np.zeros(n, np.int64)
        ln[31] = 41
    return ln.reshape(BN, HW)


@pytest.mark.parametrize('C', [32, 128])
@pytest.mark.parametrize('kind', ['long_next_to_short', 'equal_runs', 'one_long_among_ones', 'holes', 'single'])
def test_interval_shapes_inside_one_wave(kind, C, monkeypatch):
    """C = 32 (the training width: 8 intervals share a wave) and C = 128 (two): a wave iterates to its longest interval, lanes
    past their own length add nothing, one store per point; the last wave and the last block are partial"""
    lens = _shape_profile(kind)
    n_int = int(np.count_nonzero(lens))
    L = C // 4
    assert n_int == 1 or ((n_int * L) % 64 != 0 and (n_int * L) % 256 != 0)
    ranks = R.build_ranks(lens, D88, 50, seed=len(kind))
    depth, feat, og = make_inputs(3, ranks, C)
    ref = R.pool_ref64(depth, feat, og, ranks.ranks_depth, ranks.ranks_feat, ranks.ranks_bev)
    seen = []
    launch = ops.bev_pool_v2_backward

    def spy(out_grad, depth_grad, feat_grad, d, f, rd, rf, rb, interval_lengths, interval_starts):
        seen.append((interval_lengths.cpu().numpy(), interval_starts.cpu().numpy(), rf.cpu().numpy()))
        return launch(out_grad, depth_grad, feat_grad, d, f, rd, rf, rb, interval_lengths, interval_starts)
    monkeypatch.setattr(ops, 'bev_pool_v2_backward', spy)
    _, auto = check_both('%s C=%d' % (kind, C), ranks, depth, feat, og, ref)
    # the wrapper's device sort handed the kernel what the numpy restatement of the host side handed it through the ABI ...
    assert len(seen) == 2 and all(np.array_equal(a, b) for a, b in zip(*seen))
    # ... one interval per pixel WITH a point, in pixel order, and none for the others
    ln, st, rf = seen[1]
    flat = lens.reshape(-1)
    np.testing.assert_array_equal(ln, flat[flat > 0])
    np.testing.assert_array_equal(rf[st], np.flatnonzero(flat > 0))
    # pixels without a point: gradient row exactly zero; frustum points outside the grid: depth gradient exactly zero
    assert np.all(auto[2][flat == 0] == 0.0)
    named = np.zeros(len(depth), bool)
    named[ranks.ranks_depth] = True
    assert np.all(auto[1][~named] == 0.0) and (~named).sum() == len(depth) - flat.sum()


def test_backward_is_deterministic():
    ranks = R.build_ranks(_shape_profile('holes'), D88, 50, seed=1)
    depth, feat, og = make_inputs(4, ranks, 32)
    a, b = run_autograd(ranks, depth, feat, og), run_autograd(ranks, depth, feat, og)
    c, d = run_abi(ranks, depth, feat, og), run_abi(ranks, depth, feat, og)
    for x, y in zip(a + c, b + d):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------------------------------ real geometry through the module
GEO = dict(B=2, N=2, C=32, H=8, W=22, input_size=(128, 352), downsample=16)


def _geo_rig():
    """two samples x two cameras of synth.synthetic_rig (the second sample's ego moved), the image augmentation of a 4x smaller
    input (resize 0.22 +- 5 %, a small rotation, the crop offset) and a rotated + scaled / sheared bda per sample"""
    r0, r1 = S.synthetic_rig(2), S.synthetic_rig(2, dx=-2.5)
    rig = {k: np.concatenate([r0[k], r1[k]], 0) for k in r0}
    for b in range(2):
        for n in range(2):
            a, sc = 0.04 * (2 * b + n - 1), 0.22 * (1.0 + 0.05 * n)
            rig['post_rot'][b, n, :2, :2] = sc * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
            rig['post_tran'][b, n, :2] = [2.0 * n - 3.0, -70.0 + 4.0 * b]
    a = 0.06
    rig['bda'][0] = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) * np.array([1.03, 1.03, 1.0])[None, :]
    rig['bda'][1] = np.array([[0.99, 0.1, 0], [-0.1, 0.99, 0], [0, 0, 1.0]], np.float32)
    return rig


@pytest.fixture(scope='module')
def geo():
    """the view transformer at the training width and depth range on a reduced input, its ranks, random inputs and the float64
    reference -- built once, read by every test below"""
    g = dict(GEO)
    B, N, C, H, W = (g[k] for k in 'BNCHW')
    vt = M.LSSViewTransformer(grid_config=S.GRID_CONFIG_C1, input_size=g['input_size'], downsample=g['downsample'], in_channels=8,
                              out_channels=C, collapse_z=False).to(DEV)
    assert vt.D == D88 and tuple(vt.frustum.shape[:3]) == (D88, H, W)
    rig = _geo_rig()
    cams = [T(rig[k]) for k in ('sensor2ego', 'intrin', 'post_rot', 'post_tran', 'bda')]
    inp = [torch.empty(B, N, 8, H, W, device=DEV), cams[0], None] + cams[1:]
    rb, rd, rf, st, ln = vt.voxel_pooling_prepare_v2(*cams)
    _, _, size = vt._grid()
    n_vox = B * size[0] * size[1] * size[2]
    total = B * N * D88 * H * W
    kept = rb.numel()
    print('[parity] module geometry: %d of %d frustum points inside the grid, %d voxels hit, longest segment %d' % (
        kept, total, st.numel(), int(ln.max())))
    assert 0.3 * total < kept < 0.9 * total and int(ln.max()) > ops.LONG_SEGMENT          # see _geo_rig
    depth, feat = S.lift_inputs(21, B=B, N=N, D=D88, H=H, W=W, C=C)
    depth, feat = depth.reshape(B * N, D88, H, W), feat.reshape(B * N, C, H, W)
    og = np.random.RandomState(22).standard_normal((B, C, size[2], size[1], size[0])).astype(np.float32)
    featc = np.ascontiguousarray(feat.transpose(0, 2, 3, 1))
    ranks = tuple(r.cpu().numpy() for r in (rd, rf, rb))
    ref = R.pool_ref64(depth, featc, og.transpose(0, 2, 3, 4, 1).reshape(-1, C), *ranks)
    g.update(vt=vt, inp=inp, cams=cams, size=size, n_vox=n_vox, depth=depth, feat=feat, featc=featc, og=og, ref=ref, ranks=ranks,
             dev_ranks=(rd, rf, rb, st, ln))
    return g


@pytest.mark.parametrize('collapse_z', [False, True])
@pytest.mark.parametrize('form', ['nchw', 'channels_last'])
def test_module_view_transform_core_grads(geo, form, collapse_z):
    """LSSViewTransformer.view_transform_core in training, both input forms and both output forms, B = 2: forward, depth.grad
    and tran_feat.grad against the float64 reference fed the module's own ranks"""
    vt, C, size, ref = geo['vt'], geo['C'], geo['size'], geo['ref']
    B = geo['B']
    depth = T(geo['depth']).requires_grad_()
    if form == 'nchw':
        tran_feat = T(geo['feat']).requires_grad_()                     # (B*N, C, H, W): permuted by the module
    else:
        tran_feat = T(geo['featc']).requires_grad_()                    # (B*N, H, W, C) as ops.depthnet_tail returns it
        tran_feat._pw_channels_last = True
    og = T(geo['og'])                                                   # contiguous as (B, C, Z, Y, X)
    vt.collapse_z = collapse_z
    try:
        bev, dep_out = vt.view_transform_core(geo['inp'], depth, tran_feat)
    finally:
        vt.collapse_z = False
    assert dep_out is depth
    if collapse_z:
        assert tuple(bev.shape) == (B, C * size[2], size[1], size[0])
        bev.backward(torch.cat(og.unbind(dim=2), 1))
        out = bev.detach().view(B, size[2], C, size[1], size[0]).permute(0, 1, 3, 4, 2)
    else:
        assert tuple(bev.shape) == (B, C, size[2], size[1], size[0])
        assert not og.permute(0, 2, 3, 4, 1).is_contiguous()
        bev.backward(og)
        out = bev.detach().permute(0, 2, 3, 4, 1)
    name = 'module %s%s' % (form, ' collapse_z' if collapse_z else '')
    fg = tran_feat.grad if form == 'channels_last' else tran_feat.grad.permute(0, 2, 3, 1)
    check_autograd(name, (out.reshape(-1, C).cpu().numpy(), depth.grad.cpu().numpy(), fg.reshape(-1, C).cpu().numpy()), ref)


def test_training_forward_equals_the_inference_path(geo):
    """C = 32: the training forward (bev_pool_v2 from ranks, k_pool_intervals<8>) equals bev_pool_dense (k_pool_dense<8>, with
    its long-segment blocks) on the same sort to the bit, and the no-grad module path (ops.lss_lift_pool) as well"""
    vt, C = geo['vt'], geo['C']
    B, N, H, W = (geo[k] for k in 'BNHW')
    rd, rf, rb, st, ln = geo['dev_ranks']
    size = geo['size']
    d, f = T(geo['depth']).view(B, N, D88, H, W), T(geo['featc']).view(B, N, H, W, C)
    train = ops.bev_pool_v2(d, f, rd, rf, rb, (B, size[2], size[1], size[0], C), st, ln)
    vs = vt._sort(*geo['cams'])
    assert int(vs.n_long) > 0
    dense = ops.bev_pool_dense(d, f, vs)
    assert _lib.lib().pw_last_kernel().decode() == 'k_pool_dense<8>'
    assert torch.equal(dense.view(B, size[2], size[1], size[0], C).permute(0, 4, 1, 2, 3), train)
    with torch.no_grad():
        infer, _ = vt.view_transform_core(geo['inp'], T(geo['depth']), T(geo['feat']))
    assert torch.equal(infer, train)
    R.assert_within_bound('module dense forward', dense.cpu().numpy(), geo['ref'].out, geo['ref'].n['out'], geo['ref'].S['out'])


class _PassThrough(torch.nn.Module):
    def forward(self, x, mlp_input=None, stereo_metas=None):
        return x


def test_softmax_link_through_the_bevdepth_forward(geo):
    """LSSViewTransformerBEVDepth.forward with a pass-through DepthNet: the gradient with respect to the DepthNet output x (88
    depth logits + 32 context channels) -- torch's fp32 softmax backward on top of the pooling gradient -- against float64 torch
    autograd of softmax -> reference pooling -> <., out_grad> on the CPU.  Bound: the same gamma with n = 88 + the pooling's n
    and S the absolute sum of the fully expanded terms (_pool_ref64.softmax_link_bound)."""
    B, N, C, H, W = (geo[k] for k in 'BNCHW')
    size, n_vox = geo['size'], geo['n_vox']
    vt = M.LSSViewTransformerBEVDepth(grid_config=S.GRID_CONFIG_C1, input_size=geo['input_size'], downsample=geo['downsample'],
                                      in_channels=D88 + C, out_channels=C, collapse_z=False,
                                      depthnet_cfg=dict(use_dcn=False, aspp_mid_channels=8)).to(DEV)
    vt.depth_net = _PassThrough()
    rs = np.random.RandomState(33)
    x = (rs.standard_normal((B, N, D88 + C, H, W)) * 2).astype(np.float32)
    x[0, 0, :D88, 0, 0] = 5.0 * rs.standard_normal(D88)                 # a peaked pixel (probabilities down to ~1e-13: normal fp32)
    xt = T(x).requires_grad_()
    bev, dep = vt([xt] + geo['inp'][1:] + [None])
    assert tuple(bev.shape) == (B, C, size[2], size[1], size[0]) and tuple(dep.shape) == (B * N, D88, H, W)
    bev.backward(T(geo['og']))
    # float64 on the CPU
    rd, rf, rb = geo['ranks']
    x64 = torch.from_numpy(x).double().view(B * N, D88 + C, H, W).requires_grad_()
    depth64 = x64[:, :D88].softmax(dim=1)
    feat64 = x64[:, D88:].permute(0, 2, 3, 1).reshape(-1, C)
    og2 = geo['og'].transpose(0, 2, 3, 4, 1).reshape(-1, C)
    out64 = R.pool_torch64(depth64.reshape(-1), feat64, rd, rf, rb, n_vox)
    (out64 * torch.from_numpy(og2).double()).sum().backward()
    ref = R.pool_ref64(depth64.detach().numpy(), feat64.detach().numpy(), og2, rd, rf, rb)
    n, S_ = R.softmax_link_bound(x64.detach().numpy()[:, :D88], ref, D88)
    R.assert_within_bound('softmax link forward', bev.detach().permute(0, 2, 3, 4, 1).reshape(-1, C).cpu().numpy(),
                          out64.detach().numpy(), ref.n['out'] + D88, ref.S['out'])
    R.assert_within_bound('softmax link d/dx (logits + context)', xt.grad.view(B * N, D88 + C, H, W).cpu().numpy(),
                          x64.grad.numpy(), n, S_)


# ------------------------------------------------------------------------------------------ argument errors launch nothing
def test_argument_errors_launch_nothing():
    ranks = R.build_ranks(_shape_profile('holes'), D88, 50, seed=1)
    C = 32
    depth, feat, og = make_inputs(5, ranks, C)
    d, f, g = T(depth), T(feat), T(og)
    rd, rf, rb, st, ln = (T(a) for a in R.backward_intervals(ranks.ranks_depth, ranks.ranks_feat, ranks.ranks_bev))
    out = torch.full((ranks.n_vox, C), SENTINEL, device=DEV)
    dg, fg = torch.full_like(d, SENTINEL), torch.full_like(f, SENTINEL)
    empty = torch.empty(0, device=DEV, dtype=torch.int32)

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == SENTINEL).all()) for t in (out, dg, fg))
    # n_intervals == 0 returns
    ops.bev_pool_v2_backward(g, dg, fg, d, f, rd, rf, rb, empty, empty)
    ops.bev_pool_v2_forward(d, f, out, T(ranks.ranks_depth), T(ranks.ranks_feat), T(ranks.ranks_bev), empty, empty)
    assert untouched()
    st_ = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n_int = int(ln.numel())
    bwd = [g, dg, fg, d, f, rd, rf, rb, ln, st]
    fwd = [d, f, out, rd, rf, rb, ln, st]
    for i in range(len(bwd)):                                            # a null pointer in any position
        args = list(bwd)
        args[i] = None
        with pytest.raises(_lib.PreworldHipError, match='null pointer'):
            _lib.call('pw_bev_pool_v2_backward', *args, C, n_int, st_)
    for i in range(len(fwd)):
        args = list(fwd)
        args[i] = None
        with pytest.raises(_lib.PreworldHipError, match='null pointer'):
            _lib.call('pw_bev_pool_v2_forward', *args, C, n_int, st_)
    for c, n in ((0, n_int), (-4, n_int), (C, -1)):
        with pytest.raises(_lib.PreworldHipError, match='bad sizes'):
            _lib.call('pw_bev_pool_v2_backward', *bwd, c, n, st_)
        with pytest.raises(_lib.PreworldHipError, match='bad sizes'):
            _lib.call('pw_bev_pool_v2_forward', *fwd, c, n, st_)
    # the Python wrappers refuse host tensors and wrong dtypes before anything is launched
    with pytest.raises(_lib.PreworldHipError):
        ops.bev_pool_v2_backward(g.cpu(), dg, fg, d, f, rd, rf, rb, ln, st)
    with pytest.raises(_lib.PreworldHipError):
        ops.bev_pool_v2_backward(g, dg, fg, d, f, rd.long(), rf, rb, ln, st)
    assert untouched()
