"""Generate tests/golden/depth_sup_small.npz: the reference's PointToMultiViewDepth (mmdet3d/datasets/pipelines/loading.py),
get_downsampled_gt_depth and get_depth_loss (mmdet3d/models/necks/view_transformer.py) on a synthetic sweep.

Like tools/gen_golden.py this runs only where the reference checkout exists, loads its Python files through the same shim (plus
stand-ins for the packages loading.py imports; `Quaternion` is transforms.quaternion_rotation_matrix behind pyquaternion's
interface) and records inputs -> outputs as data; it contains no reference source and the .npz holds arrays only.

    python tools/gen_golden_depth.py [seed]

Inputs come from tests/_depth_np.py (synthetic_results: ground rings + box faces + near and far returns under the 6-camera rig
of preworld_amd.synth; resize, crop, flip and rotation in post_rots / post_trans) at a reduced 128 x 352 image with the loss
downsample 16, B = 2 sweeps.  The generator also runs the accounting of tests/test_depth_sup_cpu.py and refuses a sweep whose
excused share passes 5 % -- choose another sweep then, the cap stays.  Rule (a) alone excuses the 9 pixels round each of the
0.4 % of the points that lie within 1e-3 px of a rounding threshold, 3.6 % of the hit pixels on average, so whether a camera
with a few hundred hit pixels stays under the cap is a matter of two or three points: the default seed and N_AZ were picked
by running the accounting over seeds (numpy only, no reference needed) and keeping one where all 12 views stay under it."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'tests'))
import _depth_np as DN  # noqa: E402
from preworld_amd import synth as S, transforms as T  # noqa: E402

H, W, RESIZE, DS_LOSS = 128, 352, 0.22, 16
N_AZ = 240                   # azimuth steps per beam of the synthetic sweep: 8504 points per sample
DEPTH = S.GRID_CONFIG_FULL['depth']
WEIGHT = 0.05
PRED_SEED = 5
GRAD_VIEWS = (0, 7)


class _Quaternion:
    def __init__(self, q):
        self.q = q

    @property
    def rotation_matrix(self):
        return T.quaternion_rotation_matrix(self.q)


class _Points:
    def __init__(self, t):
        self.tensor = t


def load_reference():
    G.install_shim()
    base = type('Base', (), {})
    G._mod('numba')
    G._mod('PIL', Image=None)
    G._mod('pyquaternion', Quaternion=_Quaternion)
    G._mod('mmdet3d.core')
    G._mod('mmdet3d.core.points', BasePoints=base, get_points_type=None)
    G._mod('mmdet3d.core.bbox', LiDARInstance3DBoxes=base)
    G._mod('mmdet.datasets')
    G._mod('mmdet.datasets.pipelines', LoadAnnotations=base, LoadImageFromFile=base)
    G._mod('mmdet3d.datasets')
    G._mod('mmdet3d.datasets.builder', PIPELINES=G._Registry())
    G._mod('mmdet3d.datasets.pipelines')
    loading = G.load_ref('mmdet3d.datasets.pipelines.loading', 'mmdet3d/datasets/pipelines/loading.py')
    G.load_ref('mmdet3d.ops.bev_pool_v2.bev_pool', 'mmdet3d/ops/bev_pool_v2/bev_pool.py')
    vtm = G.load_ref('mmdet3d.models.necks.view_transformer', 'mmdet3d/models/necks/view_transformer.py')
    return loading, vtm


def lidar2img_f64(R):
    """the same composition in float64 numpy, independently of transforms.compose_lidar2img"""
    def pose(rot, tr):
        m = np.eye(4)
        m[:3, :3] = T.quaternion_rotation_matrix(rot)
        m[:3, 3] = tr
        return m
    c = R['curr']
    l2g = pose(c['ego2global_rotation'], c['ego2global_translation']) @ pose(c['lidar2ego_rotation'], c['lidar2ego_translation'])
    out = []
    for i, name in enumerate(R['cam_names']):
        cam = c['cams'][name]
        c2g = pose(cam['ego2global_rotation'], cam['ego2global_translation']) @ pose(cam['sensor2ego_rotation'], cam['sensor2ego_translation'])
        K = np.eye(4)
        K[:3, :3] = R['intrins'][i].astype(np.float64)
        out.append(K @ np.linalg.inv(c2g) @ l2g)
    return np.stack(out)


def fixture_pred(BN, D, h, w):
    """a seeded softmax, quantised to k / 65536 with 1 <= k <= 65535 so that it is stored exactly in 16 bits"""
    g = torch.Generator().manual_seed(PRED_SEED)
    p = (torch.randn(BN, D, h, w, generator=g) * 2.0).softmax(1)
    return (p * 65536.0).round().clamp(1, 65535).to(torch.int32).numpy().astype(np.uint16)


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    loading, vtm = load_reference()
    ref = loading.PointToMultiViewDepth(grid_config=dict(S.GRID_CONFIG_FULL), downsample=1)
    out = dict(seed=np.int64(seed), hw=np.array([H, W], np.int64), resize=np.float64(RESIZE), ds_loss=np.int64(DS_LOSS),
               depth_cfg=np.array(DEPTH, np.float64), weight=np.float64(WEIGHT), n_az=np.int64(N_AZ))
    gts = []
    for b in range(2):
        R = DN.synthetic_results(seed + 7 * b, H, W, RESIZE, n_az=N_AZ)
        results = dict(points=_Points(torch.from_numpy(R['points'])), cam_names=R['cam_names'], curr=R['curr'],
                       img_inputs=(torch.zeros(6, 3, H, W), None, None, torch.from_numpy(R['intrins']), torch.from_numpy(R['post_rots']),
                                   torch.from_numpy(R['post_trans']), None))
        gt = ref(results)['gt_depth'].numpy()
        l2i = T.compose_lidar2img(R['curr'], R['cam_names'], R['intrins']).numpy()
        acc = DN.account_maps(gt, DN.depth_maps(R['points'], l2i, R['post_rots'], R['post_trans'], H, W, 1, DEPTH[0], DEPTH[1]),
                              H, W, 1, DEPTH[0], DEPTH[1])
        for v, a in enumerate(acc):
            print('  sample %d view %d: %5d hit pixels, %4d excused pixels (%.2f %%), bad single / multi / empty %d / %d / %d, not a candidate %d'
                  % (b, v, a['n_hit'], a['n_excused'], 100.0 * a['n_excused'] / max(1, a['n_hit']), a['bad_single'], a['bad_multi'],
                     a['bad_empty'], a['not_candidate']))
            assert a['n_excused'] <= 0.05 * a['n_hit'], 'excused share over the cap: choose another sweep'
        gts.append(gt)
        out.update({'points_%d' % b: R['points'], 'intrins_%d' % b: R['intrins'], 'post_rots_%d' % b: R['post_rots'],
                    'post_trans_%d' % b: R['post_trans'], 'lidar2img_%d' % b: l2i, 'lidar2img_f64_%d' % b: lidar2img_f64(R)})
    gt = torch.from_numpy(np.stack(gts))                                     # (2, 6, H, W)
    vtm.BasicBlock = G._RefBasicBlock
    vt = vtm.LSSViewTransformerBEVStereo(grid_config=dict(S.GRID_CONFIG_FULL), input_size=(H, W), in_channels=16, out_channels=8,
                                         sid=False, collapse_z=False, loss_depth_weight=WEIGHT, downsample=DS_LOSS,
                                         depthnet_cfg=dict(use_dcn=False, aspp_mid_channels=8, stereo=True, bias=5.0))
    onehot = vt.get_downsampled_gt_depth(gt)                                 # (2 6 h w, D)
    h, w = H // DS_LOSS, W // DS_LOSS
    labels = torch.where(onehot.max(1).values > 0, onehot.argmax(1), torch.full((onehot.shape[0],), -1)).view(12, h, w)
    q = fixture_pred(12, vt.D, h, w)
    pred = torch.from_numpy(q.astype(np.float32) / np.float32(65536.0)).requires_grad_(True)
    loss = vt.get_depth_loss(gt, pred)
    loss.backward()
    print('  labelled cells %d of %d, loss %.9g' % (int((labels >= 0).sum()), labels.numel(), float(loss)))
    out.update(gt_depth=gt.numpy(), labels=labels.numpy().astype(np.int32), pred_q16=q, loss=np.float32(loss.item()),
               grad_views=np.array(GRAD_VIEWS, np.int64), grad=pred.grad.numpy()[list(GRAD_VIEWS)])
    G.save('depth_sup_small.npz', **out)


if __name__ == '__main__':
    main()
