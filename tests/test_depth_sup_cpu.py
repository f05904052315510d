"""Depth supervision from the sweep, the part that needs no GPU: the numpy restatement (tests/_depth_np.py) against the reference
fixture (tests/golden/depth_sup_small.npz, tools/gen_golden_depth.py) under the accounting rule, the transform's host side and
the argument validation of the new entry points.

THE ACCOUNTING RULE (used here and, unchanged, by tests/test_gpu_depth_sup.py).  A pixel is excused only if
  (a) a point touching it or one of its 8 neighbours lies, in float64, within 1e-3 px of a rounding threshold (the image border
      is one) or within 1e-4 relative of d0 / d1, or
  (b) it is a multi-hit pixel whose two smallest candidate depths have equal float32 sort keys rank + depth / 100 -- the
      reference's unstable argsort may keep either ("Depth supervision from the sweep").
Everywhere else single-hit pixels are bit-equal, multi-hit pixels equal the float32 minimum, empty pixels are 0; in EVERY pixel
the reference's value is one of the candidates.  A cell is excused iff it contains an excused pixel; all other labels are equal.
Caps (conditions, not measurements): per camera the excused pixels -- all of them, the empty ones in the 3 x 3 neighbourhood of a
near-threshold point included -- are at most 5 % of the hit pixels; over the fixture the excused cells, labelled or not, are at
most 5 % of the labelled cells.  Rule (a) alone excuses about 9 pixels for each of the 0.4 % of the points that lie within
1e-3 px of a threshold, 3.6 % of the hit pixels on average; the fixture's sweep was chosen (tools/gen_golden_depth.py) so that
every camera stays under the cap."""
import numpy as np
import pytest

import _depth_np as DN
from preworld_amd import _lib, transforms

CAP = 0.05


@pytest.fixture(scope='module')
def fx(golden):
    return golden('depth_sup_small.npz')


def _sample(fx, b):
    H, W = [int(v) for v in fx['hw']]
    d0, d1, dstep = [float(v) for v in fx['depth_cfg']]
    R = DN.depth_maps(fx['points_%d' % b], fx['lidar2img_%d' % b], fx['post_rots_%d' % b], fx['post_trans_%d' % b], H, W, 1, d0, d1)
    return R, H, W, d0, d1, dstep


def test_restatement_vs_reference_maps(fx):
    for b in range(2):
        R, H, W, d0, d1, _ = _sample(fx, b)
        for v, a in enumerate(DN.account_maps(fx['gt_depth'][b], R, H, W, 1, d0, d1)):
            share = a['n_excused'] / max(1, a['n_hit'])
            print('sample %d view %d: %d hit pixels, %d excused pixels (%.2f %%)' % (b, v, a['n_hit'], a['n_excused'], 100 * share))
            assert a['n_hit'] > 200
            assert share <= CAP
            assert (a['bad_single'], a['bad_multi'], a['bad_empty'], a['not_candidate']) == (0, 0, 0, 0), a


def test_restatement_vs_reference_labels(fx):
    ds = int(fx['ds_loss'])
    n_lab = n_exc = 0
    for b in range(2):
        R, H, W, d0, d1, dstep = _sample(fx, b)
        D = int(round((d1 - d0) / dstep))
        acc = DN.account_maps(fx['gt_depth'][b], R, H, W, 1, d0, d1)
        got = DN.map_labels(R['maps'], ds, d0, dstep, D)
        want = fx['labels'][6 * b:6 * b + 6]
        # the reference's own labels are its binning of its own maps
        assert np.array_equal(DN.map_labels(fx['gt_depth'][b], ds, d0, dstep, D), want)
        for v in range(6):
            exc = DN.excused_cells(acc[v]['excused'], ds)
            assert np.array_equal(got[v][~exc], want[v][~exc])
            n_lab += int((want[v] >= 0).sum())
            n_exc += int(exc.sum())
    print('labelled cells %d, excused cells %d (%.2f %%)' % (n_lab, n_exc, 100.0 * n_exc / n_lab))
    assert n_lab > 1000 and n_exc <= CAP * n_lab


def test_sweep_has_the_awkward_points(fx):
    """some behind the cameras, some beyond 45 m, some under 1 m"""
    R, H, W, d0, d1, _ = _sample(fx, 0)
    d = R['uvd64'][1][:, 2]                      # front camera
    assert (d < 0).sum() > 100 and (d >= d1).sum() > 10 and ((d > 0) & (d < d0)).sum() > 3


def test_bce_restatement_vs_reference(fx):
    pred = fx['pred_q16'].astype(np.float32) / np.float32(65536.0)
    loss, grad, n_fg = DN.bce(pred, fx['labels'], float(fx['weight']))
    assert n_fg == int((fx['labels'] >= 0).sum())
    assert abs(loss - float(fx['loss'])) <= 1e-6 * abs(loss)
    g = grad[list(fx['grad_views'])]
    assert np.abs(g - fx['grad']).max() <= 4e-5 * np.abs(g).max()


def test_lidar2img_composition(fx):
    """transforms.compose_lidar2img against the recorded float32 composition and an independent float64 one.  Bound: the chain
    is three 4x4 float32 products and one inverse of a rotation-translation matrix whose translation (~1.2e3 m) cancels in the
    product; each step loses a few eps32 of the largest intermediate, ~1.2e3 * 1266 px/m: 64 eps32 of that.  That bound (about
    12 on entries of order 1e3) catches a missing inverse or a swapped pose, not a subtle change of order or precision: the
    sharp check of the composition is test_restatement_vs_reference_maps, where the reference composes its own matrices from
    the poses and every non-excused single-hit pixel of its gt_depth is bit-equal to the restatement run on the matrices
    recorded from compose_lidar2img -- one ulp of difference in a matrix entry moves depths."""
    for b in range(2):
        R = DN.synthetic_results(int(fx['seed']) + 7 * b, int(fx['hw'][0]), int(fx['hw'][1]), float(fx['resize']), n_az=int(fx['n_az']))
        assert np.array_equal(R['points'], fx['points_%d' % b]) and np.array_equal(R['post_rots'], fx['post_rots_%d' % b])
        got = transforms.compose_lidar2img(R['curr'], R['cam_names'], R['intrins']).numpy()
        bound = 64 * np.finfo(np.float32).eps * 1.2e3 * 1266.4
        assert got.dtype == np.float32 and got.shape == (6, 4, 4)
        assert np.abs(got - fx['lidar2img_%d' % b]).max() <= bound
        assert np.abs(got - fx['lidar2img_f64_%d' % b]).max() <= bound


def test_quaternion_round_trip():
    rs = np.random.RandomState(0)
    for _ in range(20):
        q = rs.standard_normal(4)
        Rm = transforms.quaternion_rotation_matrix(q)
        assert np.allclose(Rm @ Rm.T, np.eye(3), atol=1e-12) and abs(np.linalg.det(Rm) - 1) < 1e-12
        q2 = np.array(DN.rot_to_quat(Rm))
        qn = q / np.linalg.norm(q)
        assert min(np.abs(q2 - qn).max(), np.abs(q2 + qn).max()) < 1e-12


def test_transform_call_contract(fx, monkeypatch):
    """__call__ reads points / img_inputs / cam_names / curr, hands the kernel wrapper the composed lidar2img and the first N
    post_rots / post_trans, and writes gt_depth -- or gt_depth_labels when labels_downsample is set.  The wrappers are replaced:
    no GPU here."""
    import torch
    calls = []

    def fake_maps(points, lidar2img, post_rots, post_trans, image_hw, depth_range, downsample=1, offsets=None):
        calls.append(('maps', points, lidar2img, post_rots, post_trans, tuple(image_hw), tuple(depth_range), downsample))
        return torch.zeros(1, lidar2img.shape[1], image_hw[0] // downsample, image_hw[1] // downsample)

    def fake_labels(points, lidar2img, post_rots, post_trans, image_hw, depth_cfg, loss_downsample, D=None, downsample=1, offsets=None):
        calls.append(('labels', points, lidar2img, post_rots, post_trans, tuple(image_hw), tuple(depth_cfg), loss_downsample, downsample))
        return torch.zeros(lidar2img.shape[1], image_hw[0] // downsample // loss_downsample, image_hw[1] // downsample // loss_downsample,
                           dtype=torch.int32)
    monkeypatch.setattr(transforms.ops, 'lidar_depth_maps', fake_maps)
    monkeypatch.setattr(transforms.ops, 'lidar_depth_labels', fake_labels)
    H, W = [int(v) for v in fx['hw']]
    R = DN.synthetic_results(int(fx['seed']), H, W, float(fx['resize']), n_az=int(fx['n_az']))

    class Pts:
        tensor = torch.from_numpy(R['points'])
    results = dict(points=Pts(), cam_names=R['cam_names'], curr=R['curr'],
                   img_inputs=(torch.zeros(12, 3, H, W), None, None, torch.from_numpy(R['intrins']),
                               torch.from_numpy(np.concatenate([R['post_rots']] * 2)), torch.from_numpy(np.concatenate([R['post_trans']] * 2)), None))
    gc = {'depth': [1.0, 45.0, 0.5]}
    t = transforms.PointToMultiViewDepth(gc, downsample=2, device='cpu')
    assert (t.downsample, t.grid_config, t.labels_downsample) == (2, gc, None)
    out = t(results)
    assert out is results and out['gt_depth'].shape == (6, H // 2, W // 2) and 'gt_depth_labels' not in out
    kind, pts, l2i, pr, pt, hw, rng, ds = calls[-1]
    assert kind == 'maps' and hw == (H, W) and rng == (1.0, 45.0) and ds == 2 and pts.shape == R['points'].shape
    assert l2i.shape == (1, 6, 4, 4) and pr.shape == (1, 6, 3, 3) and pt.shape == (1, 6, 3)
    assert np.array_equal(l2i[0].numpy(), transforms.compose_lidar2img(R['curr'], R['cam_names'], R['intrins']).numpy())
    assert np.array_equal(pr[0].numpy(), R['post_rots'])
    out = transforms.PointToMultiViewDepth(gc, downsample=1, labels_downsample=16, device='cpu')(dict(results))
    assert out['gt_depth_labels'].shape == (6, H // 16, W // 16) and out['gt_depth_labels'].dtype == torch.int32
    assert calls[-1][0] == 'labels' and calls[-1][6:] == ((1.0, 45.0, 0.5), 16, 1)

    class Reg:
        def __init__(self):
            self.d = {}

        def register_module(self, name=None, force=False, module=None):
            assert force
            self.d[name] = module
    reg = Reg()
    assert transforms.register_pipelines(reg) == ['PointToMultiViewDepth'] and reg.d['PointToMultiViewDepth'] is transforms.PointToMultiViewDepth


def test_new_entry_points_validate_before_any_hip_call():
    l = _lib.lib()
    one = 0x1000                                     # a non-null address that is never dereferenced: validation fails first
    cases = [
        ('pw_lidar_depth_maps', (None, 10, 5, None, 1, 6, one, one, one, 512, 1408, 1, 1.0, 45.0, one, None)),           # null points
        ('pw_lidar_depth_maps', (one, 10, 2, None, 1, 6, one, one, one, 512, 1408, 1, 1.0, 45.0, one, None)),            # stride < 3
        ('pw_lidar_depth_maps', (one, 10, 5, None, 2, 6, one, one, one, 512, 1408, 1, 1.0, 45.0, one, None)),            # B > 1, no offsets
        ('pw_lidar_depth_maps', (one, 10, 5, None, 1, 6, one, one, one, 512, 1408, 1, 0.0, 45.0, one, None)),            # d0 <= 0
        ('pw_lidar_depth_labels', (one, 10, 5, None, 1, 6, one, one, one, 512, 1408, 1, 15, 1.0, 45.0, 0.5, 88, one, None)),   # 15 does not divide
        ('pw_lidar_depth_labels', (one, 10, 5, None, 1, 6, one, one, one, 512, 1408, 1, 16, 1.0, 45.0, 0.0, 88, one, None)),   # dstep 0
        ('pw_depth_map_labels', (one, 12, 512, 1408, 15, 1.0, 0.5, 88, one, None)),
        ('pw_depth_map_labels', (None, 12, 512, 1408, 16, 1.0, 0.5, 88, one, None)),
        ('pw_depth_bce_fwd', (one, one, 12, 88, 2816, 3.0, None, one, one, None)),                                        # no workspace
        ('pw_depth_bce_fwd', (one, one, 0, 88, 2816, 3.0, one, one, one, None)),
        ('pw_depth_bce_bwd', (one, one, None, one, 12, 88, 2816, 3.0, one, None)),
    ]
    for name, args in cases:
        rc = getattr(l, name)(*args)
        assert rc == -1, (name, rc)
        assert name.encode() in l.pw_last_error(), (name, l.pw_last_error())
    assert l.pw_depth_bce_ws_bytes(12 * 2816) == (12 * 2816 // 64) * 12 and l.pw_depth_bce_ws_bytes(0) == 0
