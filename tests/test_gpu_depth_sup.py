"""Depth supervision from the sweep on the GPU (csrc/pw_depth_sup.hip; ops.lidar_depth_maps / lidar_depth_labels /
depth_map_labels / DepthBCE): against the reference fixture under the accounting rule of tests/test_depth_sup_cpu.py (same
functions, same caps), against the numpy restatement at the training size, against the existing PyTorch path, through
forward_train, and inside one captured graph.  Bounds for the loss terms are the project's fine-tune bounds: loss 1e-6 relative,
gradient 4e-5 of its max-norm."""
import numpy as np
import pytest
import torch

import _depth_np as DN
import _e2e_stub as E
from preworld_amd import harness, modules, ops, synth as S, transforms

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CAP = 0.05
DEPTH = [1.0, 45.0, 0.5]
D = 88


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope='module')
def fx(golden):
    return golden('depth_sup_small.npz')


def _vt(input_size, weight=0.05):
    return modules.LSSViewTransformerBEVStereo(grid_config=S.GRID_CONFIG_FULL, input_size=input_size, in_channels=16, out_channels=8,
                                               sid=False, collapse_z=False, loss_depth_weight=weight, downsample=16,
                                               depthnet_cfg=dict(use_dcn=False, aspp_mid_channels=8, stereo=True, bias=5.0)).to(DEV)


def _check_maps(tag, got, ref_np, R, H, W, ds=1):
    """got: device maps (V,h,w) under the rule against the restatement R; ref_np (or None): the reference's maps"""
    got = got.cpu().numpy()
    for v, a in enumerate(DN.account_maps(got, R, H // ds, W // ds, ds, DEPTH[0], DEPTH[1])):
        share = a['n_excused'] / max(1, a['n_hit'])
        print('%s view %d: %d hit, %d excused (%.2f %%), differs from the restatement in %d pixels' %
              (tag, v, a['n_hit'], a['n_excused'], 100 * share, int((got[v].view(np.uint32) != R['maps'][v].view(np.uint32)).sum())))
        assert share <= CAP
        assert (a['bad_single'], a['bad_multi'], a['bad_empty'], a['not_candidate']) == (0, 0, 0, 0), a
        if ref_np is not None:                        # the kernel against the reference itself: same rule
            exc = a['excused']
            assert np.array_equal(got[v][~exc].view(np.uint32), ref_np[v][~exc].view(np.uint32))
    return got


def test_maps_and_labels_vs_reference_fixture(fx):
    H, W = [int(v) for v in fx['hw']]
    ds = int(fx['ds_loss'])
    pts = [T(fx['points_%d' % b]) for b in range(2)]
    l2i = T(np.stack([fx['lidar2img_%d' % b] for b in range(2)]))
    pr, pt = T(np.stack([fx['post_rots_%d' % b] for b in range(2)])), T(np.stack([fx['post_trans_%d' % b] for b in range(2)]))
    maps = ops.lidar_depth_maps(pts, l2i, pr, pt, (H, W), DEPTH[:2])                       # B = 2 in one launch
    labels = ops.lidar_depth_labels(pts, l2i, pr, pt, (H, W), DEPTH, ds).cpu().numpy()
    assert maps.shape == (2, 6, H, W) and labels.shape == (12, H // ds, W // ds) and labels.dtype == np.int32
    n_lab = n_exc = 0
    for b in range(2):
        R = DN.depth_maps(fx['points_%d' % b], fx['lidar2img_%d' % b], fx['post_rots_%d' % b], fx['post_trans_%d' % b], H, W, 1, *DEPTH[:2])
        got = _check_maps('fixture sample %d' % b, maps[b], fx['gt_depth'][b], R, H, W)
        one = ops.lidar_depth_maps(pts[b], l2i[b:b + 1], pr[b:b + 1], pt[b:b + 1], (H, W), DEPTH[:2])      # B = 1, no offsets: same bits
        assert torch.equal(one[0], maps[b])
        assert np.array_equal(labels[6 * b:6 * b + 6], DN.map_labels(got, ds, DEPTH[0], DEPTH[2], D))      # labels = binning of the maps
        acc = DN.account_maps(got, R, H, W, 1, DEPTH[0], DEPTH[1])
        for v in range(6):
            exc = DN.excused_cells(acc[v]['excused'], ds)
            want = fx['labels'][6 * b + v]
            assert np.array_equal(labels[6 * b + v][~exc], want[~exc])
            n_lab += int((want >= 0).sum())
            n_exc += int(exc.sum())
    print('labelled cells %d, excused cells %d' % (n_lab, n_exc))
    assert n_exc <= CAP * n_lab
    # the transform end to end: poses -> lidar2img on the host -> kernel
    Rs = DN.synthetic_results(int(fx['seed']), H, W, float(fx['resize']), n_az=int(fx['n_az']))
    res = dict(points=torch.from_numpy(Rs['points']), cam_names=Rs['cam_names'], curr=Rs['curr'],
               img_inputs=(torch.zeros(6, 3, H, W), None, None, torch.from_numpy(Rs['intrins']), torch.from_numpy(Rs['post_rots']),
                           torch.from_numpy(Rs['post_trans']), None))
    out = transforms.PointToMultiViewDepth(S.GRID_CONFIG_FULL, downsample=1, device=DEV)(res)
    l2i_here = transforms.compose_lidar2img(Rs['curr'], Rs['cam_names'], Rs['intrins']).numpy()
    if np.array_equal(l2i_here, fx['lidar2img_0']):
        assert torch.equal(out['gt_depth'], maps[0])
    else:                        # another host's LAPACK: same rule against the restatement with this host's matrices
        _check_maps('transform', out['gt_depth'], None, DN.depth_maps(Rs['points'], l2i_here, Rs['post_rots'], Rs['post_trans'], H, W, 1, *DEPTH[:2]), H, W)
    lab = transforms.PointToMultiViewDepth(S.GRID_CONFIG_FULL, downsample=1, labels_downsample=ds, device=DEV)(dict(res))['gt_depth_labels']
    assert lab.shape == (6, H // ds, W // ds) and lab.dtype == torch.int32


def _full_inputs(seed, n_az=1000):
    H, W = 512, 1408
    R = DN.synthetic_results(seed, H, W, 0.48, n_az=n_az, n_boxes=30, pts_per_box=100)
    l2i = transforms.compose_lidar2img(R['curr'], R['cam_names'], R['intrins']).numpy()
    return R, l2i, H, W


def test_maps_and_labels_vs_restatement_full_size():
    """about 35 k points per sample, 6 views, 512 x 1408, D = 88, B = 2"""
    Rs = [_full_inputs(13), _full_inputs(21)]          # sweeps whose excused share stays under the cap in all 12 views
    H, W = Rs[0][2:]
    pts = [T(r[0]['points']) for r in Rs]
    assert all(30000 < p.shape[0] < 40000 for p in pts)
    l2i, pr, pt = T(np.stack([r[1] for r in Rs])), T(np.stack([r[0]['post_rots'] for r in Rs])), T(np.stack([r[0]['post_trans'] for r in Rs]))
    maps = ops.lidar_depth_maps(pts, l2i, pr, pt, (H, W), DEPTH[:2])
    labels = ops.lidar_depth_labels(pts, l2i, pr, pt, (H, W), DEPTH, 16)
    assert torch.equal(labels, ops.depth_map_labels(maps, 16, DEPTH, D))                  # with and without the dense maps: same labels
    again = ops.lidar_depth_labels(pts, l2i, pr, pt, (H, W), DEPTH, 16)
    assert torch.equal(labels, again) and torch.equal(maps, ops.lidar_depth_maps(pts, l2i, pr, pt, (H, W), DEPTH[:2]))
    labels = labels.cpu().numpy()
    for b, (R, l2, _, _) in enumerate(Rs):
        Rn = DN.depth_maps(R['points'], l2, R['post_rots'], R['post_trans'], H, W, 1, *DEPTH[:2])
        got = _check_maps('full sample %d' % b, maps[b], None, Rn, H, W)
        acc = DN.account_maps(got, Rn, H, W, 1, DEPTH[0], DEPTH[1])
        want = DN.map_labels(Rn['maps'], 16, DEPTH[0], DEPTH[2], D)
        for v in range(6):
            exc = DN.excused_cells(acc[v]['excused'], 16)
            assert np.array_equal(labels[6 * b + v][~exc], want[v][~exc])
        assert (want >= 0).sum() > 2000
    # a coarser map (downsample 4) against the restatement too.  16 x fewer pixels and ranks under 2^16 make float32-key ties
    # (rule b) common at the full sweep's density -- the excused share is 6.5 to 9 % there -- so this case runs on every fourth point
    R = Rs[0][0]
    thin = np.ascontiguousarray(R['points'][::4])
    m4 = ops.lidar_depth_maps(T(thin), l2i[:1], pr[:1], pt[:1], (H, W), DEPTH[:2], downsample=4)
    _check_maps('full ds 4', m4[0], None, DN.depth_maps(thin, Rs[0][1], R['post_rots'], R['post_trans'], H, W, 4, *DEPTH[:2]), H, W, ds=4)


def _dense_gt(seed, B=2, N=6, H=512, W=1408):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(B, N, H, W, generator=g) * 60.0
    gt[torch.rand(B, N, H, W, generator=g) < 0.995] = 0.0
    gt[0, 3] = 0.0                                     # an all-zero camera
    gt[1, 2, 32:48, 64:80] = 0.0
    gt[1, 2, 40, 70] = 60.0                            # a patch whose only depth lies beyond the grid
    gt[1, 2, 48:64, 64:80] = 0.0
    gt[1, 2, 50, 66] = 0.3                             # ... and one under it (bin 0 of the reference: no label)
    return gt.to(DEV)


def test_depth_map_labels_equal_get_downsampled_gt_depth():
    vt = _vt((512, 1408))
    gt = _dense_gt(3)
    onehot = vt.get_downsampled_gt_depth(gt)
    fg = onehot.max(1).values > 0
    want = torch.where(fg, onehot.argmax(1), torch.full_like(onehot.argmax(1), -1)).view(12, 32, 88)
    got = vt.get_depth_labels(gt_depth=gt)
    assert got.dtype == torch.int32 and torch.equal(got.long(), want)
    assert int((got[3] >= 0).sum()) == 0 and int(got[8, 2, 4]) == -1 and int(got[8, 3, 4]) == -1
    assert 0.3 < float(fg.float().mean()) < 0.9


def _softmax_pred(seed, BN=12, h=32, w=88):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(BN, D, h, w, generator=g) * 2.0).softmax(1).to(DEV)


def _check_loss(pred, labels, weight, loss, grad):
    want_l, want_g, n_fg = DN.bce(pred.cpu().numpy(), labels.cpu().numpy(), weight)
    err_l = abs(float(loss) - want_l) / max(abs(want_l), 1e-30)
    err_g = float(np.abs(grad.cpu().numpy() - want_g).max() / max(np.abs(want_g).max(), 1e-30))
    print('loss %.9g (float64 %.9g, rel err %.2e), gradient max err / max %.2e, n_fg %d' % (float(loss), want_l, err_l, err_g, n_fg))
    assert err_l <= 1e-6 and err_g <= 4e-5


def test_loss_and_gradient_vs_fixture_and_float64(fx):
    weight = float(fx['weight'])
    vt = _vt((int(fx['hw'][0]), int(fx['hw'][1])), weight)
    pred = T(fx['pred_q16'].astype(np.float32) / np.float32(65536.0)).requires_grad_(True)
    labels = T(fx['labels'])
    loss = vt.get_depth_loss_from_labels(labels, pred)
    loss.backward()
    assert abs(float(loss) - float(fx['loss'])) <= 1e-6 * abs(float(fx['loss']))
    g = pred.grad[list(fx['grad_views'])].cpu().numpy()
    assert np.abs(g - fx['grad']).max() <= 4e-5 * np.abs(fx['grad']).max()
    _check_loss(pred.detach(), labels, weight, loss, pred.grad)
    # from the reference's dense maps through depth_map_labels: the same labels, the same bits
    lab2 = vt.get_depth_labels(gt_depth=T(fx['gt_depth']))
    assert torch.equal(lab2, labels)
    # the existing PyTorch path on the same inputs
    p2 = pred.detach().clone().requires_grad_(True)
    old = vt.get_depth_loss(T(fx['gt_depth']), p2)
    old.backward()
    assert abs(float(old) - float(loss)) <= 1e-6 * abs(float(old))
    assert float((p2.grad - pred.grad).abs().max()) <= 4e-5 * float(p2.grad.abs().max())


def test_loss_full_size_clamps_empty_and_reproducible():
    vt = _vt((512, 1408), 3.0)
    labels = vt.get_depth_labels(gt_depth=_dense_gt(4))
    pred = _softmax_pred(6)
    p0 = pred.clone().requires_grad_(True)                       # the plain case at the training size first
    l0 = ops.depth_bce(p0, labels, 3.0)
    l0.backward()
    _check_loss(p0.detach(), labels, 3.0, l0, p0.grad)
    # exact 0 and 1, on and off the target bin, to reach both clamps (log >= -100) and the 1e-12 floor of the gradient
    lab = labels.clone()
    lab[0, 0, :4] = torch.tensor([5, 5, 7, 7], dtype=torch.int32, device=DEV)
    pred[0, :, 0, 0] = 0.0
    pred[0, 5, 0, 0] = 1.0                 # target exactly 1, the rest exactly 0: contributes 0
    pred[0, :, 0, 1] = 0.0
    pred[0, 9, 0, 1] = 1.0                 # target exactly 0 and another bin exactly 1: two clamped logs
    pred[0, 7, 0, 2] = 0.0
    pred[0, 3, 0, 3] = 1.0
    pred.requires_grad_(True)
    loss = ops.depth_bce(pred, lab, 3.0)
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(pred.grad).all()
    _check_loss(pred.detach(), lab, 3.0, loss, pred.grad)
    assert float(pred.grad[lab.unsqueeze(1).expand_as(pred) < 0].abs().max()) == 0.0            # zeros on background cells
    g1 = pred.grad.clone()
    pred.grad = None
    loss2 = ops.depth_bce(pred, lab, 3.0)
    loss2.backward()
    assert torch.equal(loss, loss2) and torch.equal(g1, pred.grad)                              # bit-identical runs
    # no foreground cell at all
    p = _softmax_pred(7).requires_grad_(True)
    none = ops.depth_bce(p, torch.full_like(lab, -1), 3.0)
    none.backward()
    assert float(none) == 0.0 and float(p.grad.abs().max()) == 0.0


class _GradDepthNet(E.SeededDepthNet):
    """the seeded stand-in, with outputs that are autograd leaves: d loss / d depth logits can be read off them"""

    def forward(self, x, mlp_input, stereo_metas=None):
        out = super().forward(x, mlp_input, stereo_metas).requires_grad_(True)
        self.outs = getattr(self, 'outs', []) + [out]
        return out


def test_forward_train_points_vs_dense_gt_depth():
    B = 2
    cfg = E.model_cfg('PreWorld', True, True)
    cfg.update(E.TRAIN_CFG)
    cfg['use_lss_depth_loss'] = True
    inputs = tuple(t.to(DEV) for t in E.img_inputs(0, batch=B))
    H, W = E.INPUT_SIZE
    N = len(E.VARIANTS['small']['cams'])
    # lidar frame = key ego frame: lidar2img = K inverse(sensor2ego) of the key frame's cameras
    s2e, K = inputs[1].view(B, 3, N, 4, 4)[:, 0].double(), inputs[3].view(B, 3, N, 3, 3)[:, 0].double()
    K4 = torch.eye(4, dtype=torch.float64, device=DEV).repeat(B, N, 1, 1)
    K4[..., :3, :3] = K
    lidar2img = (K4 @ torch.inverse(s2e)).float()
    pts = [T(DN.synthetic_sweep(21 + b, n_az=300)) for b in range(B)]
    pr, pt = inputs[4].view(B, 3, N, 3, 3)[:, 0].contiguous(), inputs[5].view(B, 3, N, 3)[:, 0].contiguous()
    gt_depth = ops.lidar_depth_maps(pts, lidar2img, pr, pt, (H, W), DEPTH[:2])
    assert int((gt_depth > 0).sum()) > 500
    runs = []
    for kw in (dict(gt_depth=gt_depth), dict(points=pts, lidar2img=lidar2img),
               dict(gt_depth_labels=ops.depth_map_labels(gt_depth, 16, DEPTH, D))):
        net = harness.build_model(cfg, S.synth_state_dict(0), DEV).train()
        E.install_image_side(net, seed=0)
        dn = net.img_view_transformer.depth_net = _GradDepthNet(0)
        kw.update(E.train_kwargs(0, 'PreWorld', DEV, batch=B))
        losses = net(return_loss=True, img_inputs=inputs, img_metas=[dict()] * B, **kw)
        key = dn.outs[-1]                                       # the key frame runs last
        g, = torch.autograd.grad(losses['loss_lss_depth'], key, retain_graph=False)
        runs.append(({k: v.detach().clone() for k, v in losses.items()}, g[:, :D]))
    (l0, g0) = runs[0]
    assert float(l0['loss_lss_depth']) > 0 and float(g0.abs().max()) > 0
    for l1, g1 in runs[1:]:
        assert sorted(l0) == sorted(l1)
        for k in l0:
            if k == 'loss_lss_depth':
                err = abs(float(l0[k]) - float(l1[k])) / abs(float(l0[k]))
                print('loss_lss_depth dense %.9g, new path %.9g (rel %.2e)' % (float(l0[k]), float(l1[k]), err))
                assert err <= 1e-6
            else:
                assert torch.equal(l0[k], l1[k]), k
        gerr = float((g0 - g1).abs().max() / g0.abs().max())
        print('d loss_lss_depth / d depth logits: max err / max %.2e' % gerr)
        assert gerr <= 4e-5


def test_labels_loss_backward_in_one_captured_graph():
    """get_depth_labels -> get_depth_loss_from_labels -> backward as ONE captured chain; replayed on a second sweep copied into
    the static buffers it equals eager on that sweep: nothing in the path synchronises or reads a size back."""
    vt = _vt((512, 1408), 3.0)
    Rs = [_full_inputs(31), _full_inputs(32, 960), _full_inputs(33, 1040), _full_inputs(34, 900)]   # 32 n_az + 3104 points each
    cap = 2 * 40000

    def pack(a, b):
        pa, pb = a[0]['points'], b[0]['points']
        buf = np.zeros((cap, 5), np.float32)
        buf[:pa.shape[0]], buf[pa.shape[0]:pa.shape[0] + pb.shape[0]] = pa, pb
        off = np.array([0, pa.shape[0], pa.shape[0] + pb.shape[0]], np.int32)
        return [T(buf), T(off), T(np.stack([a[1], b[1]])), T(np.stack([a[0]['post_rots'], b[0]['post_rots']])),
                T(np.stack([a[0]['post_trans'], b[0]['post_trans']]))]
    first, second = pack(Rs[0], Rs[1]), pack(Rs[2], Rs[3])
    assert int(first[1][2]) != int(second[1][2])                    # sweeps of different lengths
    static = [t.clone() for t in first]
    logits = (torch.randn(12, D, 32, 88, generator=torch.Generator().manual_seed(8)) * 2.0).to(DEV).requires_grad_(True)

    def step(bufs):
        labels = vt.get_depth_labels(points=bufs[0], offsets=bufs[1], lidar2img=bufs[2], post_rots=bufs[3], post_trans=bufs[4])
        loss = vt.get_depth_loss_from_labels(labels, logits.softmax(1))
        g, = torch.autograd.grad(loss, logits)
        return loss, g
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(static)                                                # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_c, grad_c = step(static)
    for bufs in (second, first):
        for d, src in zip(static, bufs):
            d.copy_(src)
        graph.replay()
        loss_e, grad_e = step(bufs)
        assert float(loss_e) > 0 and torch.equal(loss_c, loss_e) and torch.equal(grad_c, grad_e)
