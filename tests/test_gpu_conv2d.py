"""The FPN_LSS / DepthNet convolutions on the device: pw_conv2d through ops.conv2d against the float64 yardstick of
tests/_conv2d_ref64.py under 4 x the torch path's own CPU floor and, per element in units of 2^-24 n, under 2 Q32 + 1, exact scaling of the range cases, same bits twice, graph capture, a
refused layout, FPN_LSS / DepthNet(conv_impl='hip') against the golden outputs and, at real width, against the float64 modules, the
Derived cache after new BatchNorm statistics, and the image branch with fused convolutions against the torch branch."""
import numpy as np
import pytest
import torch

import _conv2d_ref64 as R
from preworld_amd import _lib, image_encoder as IE, ops, synth as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAMES = list(R.CASES)
CL = torch.channels_last


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _operands(name):
    """a case's maps on the device in channels-last storage, and its layers"""
    i = R.inputs(name)
    conv, bn = R.conv_modules(name, DEV)
    res = None if i['residual'] is None else i['residual'].to(DEV).contiguous(memory_format=CL)
    return dict(x=i['x'].to(DEV).contiguous(memory_format=CL), residual=res, conv=conv, bn=bn)


def _run(name, x=None, d=None):
    """(out, packed) of a case through ops.conv2d_pack / ops.conv2d"""
    c = R.CASES[name]
    d = _operands(name) if d is None else d
    packed = ops.conv2d_pack(d['conv'], d['bn'])
    out = ops.conv2d(d['x'] if x is None else x, packed, dilation=c.dil, relu=c.epi != 'none', residual=d['residual'])
    return out, packed


@pytest.mark.parametrize('name', NAMES)
def test_ops_against_the_yardstick(name):
    ref = R.reference(name)
    out, _ = _run(name)
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(ref.shape) and out.permute(0, 2, 3, 1).is_contiguous()
    err = R.rel_err(out.cpu(), ref)
    print('%s: kernel %.3e, bound %.3e (4 x floor %.1e), variant %s' % (name, err, 4 * R.FLOORS[name], R.FLOORS[name],
                                                                        R.tile_variant(R.CASES[name])))
    assert bool(torch.isfinite(out).all())
    assert err <= 4 * R.FLOORS[name], (name, err)


@pytest.mark.parametrize('name', NAMES)
def test_ops_per_element_units(name):
    """every element against its own magnitude: q = |out - out64| / (2^-24 n) under 2 Q32 + 1 + FORMAT_TERM (THE UNIT in
    tests/_conv2d_ref64.py); an element whose normaliser is zero must be exact"""
    out, _ = _run(name)
    assert out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    R.check_units(name, out, 'kernel')


def test_range_cases_scale_exactly():
    """x, shift and residual times a power of two: the tensor's exponent absorbs it, so the output bits are the same bits scaled"""
    a, b = _run('range_2m12')[0], _run('range_2p8')[0]
    assert torch.equal(a * 2.0 ** 20, b) and float(b.abs().max()) > 0


def test_two_calls_give_the_same_bits():
    for name in ('image_seam', 'cin_600', 'big_1x1', 'big_3x3'):
        (a, pa), (b, pb) = _run(name), _run(name)
        assert torch.equal(a, b) and torch.equal(pa.buf, pb.buf), name


def test_graph_capture_replays_to_the_eager_result():
    name = 'dil6_edges'
    d = _operands(name)
    eager, _ = _run(name, d=d)
    static = torch.zeros_like(d['x'])
    assert static.permute(0, 2, 3, 1).is_contiguous()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                         # one stream: no parallel branches; the pack is captured too
        out, _ = _run(name, static, d)
    static.copy_(d['x'])
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_a_layout_that_is_not_channels_last_is_refused():
    d = _operands('image_seam')
    packed = ops.conv2d_pack(d['conv'], d['bn'])
    with pytest.raises(_lib.PreworldHipError, match='x must be in torch.channels_last storage'):
        ops.conv2d(d['x'].contiguous(), packed)
    d = _operands('res_relu')
    packed = ops.conv2d_pack(d['conv'], d['bn'])
    with pytest.raises(_lib.PreworldHipError, match='residual must be in torch.channels_last storage'):
        ops.conv2d(d['x'], packed, relu=True, residual=d['residual'].contiguous())


def _ran_fused(net):
    return all(m._derived is not None for m in net.modules() if isinstance(m, IE._FusedConvs))


def test_toy_neck_and_depthnet_match_the_golden_outputs(golden):
    g = golden('image_branch_small.npz')
    neck = IE.FPN_LSS(in_channels=64 + 128, out_channels=24, extra_upsample=None, input_feature_index=(0, 1), scale_factor=2,
                      conv_impl='hip').eval()
    neck.load_state_dict(S.seeded_module_state(neck, 53))
    neck = neck.to(DEV)
    with torch.no_grad():
        out = neck([T(g['swin_s2']), T(g['swin_s3'])])
    assert tuple(out.shape) == g['neck'].shape and _ran_fused(neck)
    np.testing.assert_allclose(out.cpu().numpy(), g['neck'], rtol=3e-4, atol=3e-5)
    dn = IE.DepthNet(16, 16, 4, 12, use_dcn=False, aspp_mid_channels=8, stereo=True, bias=5.0, conv_impl='hip').eval()
    dn.load_state_dict(S.seeded_module_state(dn, 54))
    dn = dn.to(DEV)
    prev, curr, k2s, K, post_rot, post_tran, frustum = S.stereo_inputs(55, C=8, H=8, W=12, D=12, n_cams=2)
    rs = np.random.RandomState(56)
    xin = T(rs.standard_normal((2, 16, 2, 3)).astype(np.float32))
    mlp = T(rs.standard_normal((1, 2, 27)).astype(np.float32))
    metas = dict(k2s_sensor=T(k2s), intrins=T(K), post_rots=T(post_rot), post_trans=T(post_tran), frustum=T(frustum),
                 cv_downsample=4, downsample=16, cv_feat_list=[T(prev), T(curr)])
    with torch.no_grad():
        out = dn(xin, mlp, metas)
        metas['cv_feat_list'] = [None, T(curr)]
        out0 = dn(xin, mlp, metas)
    assert _ran_fused(dn)
    np.testing.assert_allclose(out.cpu().numpy(), g['depthnet_stereo'], rtol=3e-4, atol=3e-5)
    np.testing.assert_allclose(out0.cpu().numpy(), g['depthnet_nostereo'], rtol=3e-4, atol=3e-5)


def test_real_width_neck_and_depthnet_against_the_float64_modules():
    """FPN_LSS 1536 -> 512 and the 512-wide stereo DepthNet with fused convolutions against the same modules in float64 on the CPU,
    within 4 x the float32 torch module's own CPU floor (tests/test_conv2d_cpu.py::test_module_floors)"""
    with torch.no_grad():
        neck, feats = R.build_neck('hip')
        neck64, feats64 = R.build_neck(dtype=torch.float64)
        want = neck64(feats64)
        got = neck.to(DEV)([f.to(DEV) for f in feats])
        err = R.rel_err(got.cpu(), want)
        print('neck: fused %.3e, bound %.3e' % (err, 4 * R.MODULE_FLOORS['neck']))
        assert _ran_fused(neck) and err <= 4 * R.MODULE_FLOORS['neck']
        dn, x, mlp, metas = R.build_depthnet('hip')
        dn64, x64, mlp64, _ = R.build_depthnet(dtype=torch.float64)
        want = dn64(x64, mlp64, metas)
        got = dn.to(DEV)(x.to(DEV), mlp.to(DEV), metas)
        err = R.rel_err(got.cpu(), want)
        print('depthnet: fused %.3e, bound %.3e' % (err, 4 * R.MODULE_FLOORS['depthnet']))
        assert _ran_fused(dn) and err <= 4 * R.MODULE_FLOORS['depthnet']


def test_new_batchnorm_statistics_are_seen_by_the_next_forward():
    """load_state_dict copies into the running-statistic buffers in place: the Derived key holds them, so the packs are rebuilt"""
    neck = IE.FPN_LSS(in_channels=64 + 128, out_channels=24, extra_upsample=None, input_feature_index=(0, 1), scale_factor=2,
                      conv_impl='hip').eval()
    neck.load_state_dict(S.seeded_module_state(neck, 53))
    neck = neck.to(DEV)
    rs = np.random.RandomState(57)
    feats = [T(rs.standard_normal((1, 64, 4, 6)).astype(np.float32)), T(rs.standard_normal((1, 128, 2, 3)).astype(np.float32))]
    with torch.no_grad():
        before = neck(feats)
        sd = {k: v.clone() for k, v in neck.state_dict().items()}
        sd['conv.1.running_mean'] += 0.5
        sd['conv.4.running_var'] *= 2.0
        neck.load_state_dict(sd)
        after = neck(feats)
        fresh = IE.FPN_LSS(in_channels=64 + 128, out_channels=24, extra_upsample=None, input_feature_index=(0, 1), scale_factor=2,
                           conv_impl='hip').eval().to(DEV)
        fresh.load_state_dict(sd)
        want = fresh(feats)
        fresh.set_conv_impl('torch')
        torch_out = fresh(feats)
    assert not torch.equal(before, after) and torch.equal(after, want)
    np.testing.assert_allclose(after.cpu().numpy(), torch_out.cpu().numpy(), rtol=3e-4, atol=3e-5)


def test_image_branch_with_fused_convs_against_the_torch_branch():
    """ImageBranch.frames_from_images on the toy-width config of tests/test_gpu_image_branch.py::test_images_to_occupancy_wiring
    (real 512 x 1408 input, a 32 x 88 map): conv_impl='hip' against 'torch' on the same device, to that test's rtol plus the golden
    comparison's atol"""
    cfg = IE.preworld_image_cfg()
    cfg['backbone_cfg'] = dict(S.small_swin_cfg(), window_size=4)
    cfg['neck_cfg'] = dict(in_channels=64 + 128, out_channels=48, extra_upsample=None, input_feature_index=(0, 1), scale_factor=2)
    cfg['in_channels'] = 48
    torch.manual_seed(0)
    branch = IE.ImageBranch(**cfg).to(DEV).eval()
    n_cams = 1
    rigs = [S.synthetic_rig(n_cams, dx=-2.5 * f) for f in range(3)]
    imgs = [torch.randn(1, n_cams, 3, 512, 1408, device=DEV) for _ in range(3)]
    s2k = [T(r['sensor2ego']) for r in rigs]
    e2g = [torch.eye(4, device=DEV).view(1, 1, 4, 4).repeat(1, n_cams, 1, 1) for _ in range(3)]
    intr, prot, ptran = [T(r['intrin']) for r in rigs], [T(r['post_rot']) for r in rigs], [T(r['post_tran']) for r in rigs]
    k2s = torch.eye(4, device=DEV).view(1, 1, 4, 4).repeat(1, n_cams, 1, 1)
    k2s[..., 0, 3] = 0.3
    args = (imgs, s2k, e2g, intr, prot, ptran, T(rigs[0]['bda']), [k2s, k2s, None])
    want = branch.frames_from_images(*args)
    assert not _ran_fused(branch.img_neck)
    branch.set_conv_impl('hip')
    got = branch.frames_from_images(*args)
    assert branch.conv_impl == 'hip' and _ran_fused(branch.img_neck) and _ran_fused(branch.img_view_transformer.depth_net)
    assert len(got) == len(want) == 2
    for f, w in zip(got, want):
        assert tuple(f['depth'].shape) == (n_cams, 88, 32, 88) and tuple(f['tran_feat'].shape) == (n_cams, 32, 88, 32)
        np.testing.assert_allclose(f['depth'].sum(1).cpu().numpy(), 1.0, rtol=1e-4)
        for k in ('depth', 'tran_feat'):
            err = float((f[k] - w[k]).abs().max())
            print('%s: max |hip - torch| %.3e of max %.3e' % (k, err, float(w[k].abs().max())))
            np.testing.assert_allclose(f[k].cpu().numpy(), w[k].cpu().numpy(), rtol=1e-4, atol=3e-5)
