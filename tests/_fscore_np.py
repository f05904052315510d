"""A numpy restatement of Metric_FScore (mmdet3d/datasets/occ_metrics.py:322-410) on the voxel lattice: the reference's two
KDTree nearest-neighbour queries become an OR of shifted occupancy grids over the offsets that ops.fscore_offsets admits.
Shared by tests/test_fscore_cpu.py and tests/test_gpu_fscore.py."""
import numpy as np

from preworld_amd import ops


def occupied(grid, mask, void):
    """voxel2points' selection (:352-356) after add_batch's masking (:372-378): masked voxels read as 255"""
    g = np.asarray(grid)
    if mask is not None:
        g = np.where(np.asarray(mask).astype(bool), g, 255)
    return ~np.isin(g, np.asarray(void))


def near(occ, m):
    """bool grid: some voxel of `occ` lies at an admissible offset (|dz| <= m[dx + rx, dy + ry]); outside the grid is empty"""
    rx, ry = (m.shape[0] - 1) // 2, (m.shape[1] - 1) // 2
    X, Y, Z = occ.shape
    rz = int(max(0, m.max()))
    pad = np.zeros((X + 2 * rx, Y + 2 * ry, Z + 2 * rz), bool)
    pad[rx:rx + X, ry:ry + Y, rz:rz + Z] = occ
    out = np.zeros_like(occ)
    for i in range(2 * rx + 1):
        for j in range(2 * ry + 1):
            for dz in range(-int(m[i, j]), int(m[i, j]) + 1):
                out |= pad[i:i + X, j:j + Y, rz + dz:rz + dz + Z]
    return out


def counts(pred, gt, mask=None, void=(17, 255), voxel_size=(0.4, 0.4, 0.4), thr_acc=0.6, thr_cmpl=0.6):
    """{n_pred, n_pred_hit, n_gt, n_gt_hit} of one sample, as pw_occ_fscore adds them"""
    P, G = occupied(pred, mask, void), occupied(gt, mask, void)
    ma, mc = ops.fscore_offsets(thr_acc, voxel_size), ops.fscore_offsets(thr_cmpl, voxel_size)
    return np.array([P.sum(), (P & near(G, ma)).sum(), G.sum(), (G & near(P, mc)).sum()], np.int64)


def scores(c, eps=1e-8):
    """(acc, cmpl, f) of one count row with the reference's float64 arithmetic (:380-397); empty gt -> (0, 0, 0)"""
    n_pred, hit_p, n_gt, hit_g = (int(v) for v in c)
    if n_pred == 0 or n_gt == 0:
        return 0.0, 0.0, 0.0
    acc = np.float64(hit_p) / np.float64(n_pred)
    cmpl = np.float64(hit_g) / np.float64(n_gt)
    return float(acc), float(cmpl), float(2.0 / (1 / (acc + eps) + 1 / (cmpl + eps)))


def fixture_case(z, name):
    """(metric kwargs, [(pred, gt, mask_lidar, mask_camera)], per-sample (n, 3), totals (3,)) of one case of fscore.npz"""
    p = name + '_'
    lid, cam = (bool(v) for v in z[p + 'masks'])
    kw = dict(threshold_acc=float(z[p + 'thresholds'][0]), threshold_complete=float(z[p + 'thresholds'][1]),
              voxel_size=[float(v) for v in z[p + 'voxel_size']], void=[int(v) for v in z[p + 'void']],
              use_lidar_mask=lid, use_image_mask=cam)
    n = z[p + 'pred'].shape[0]
    samples = [(z[p + 'pred'][i], z[p + 'gt'][i], z[p + 'mask_lidar'][i] if lid else None,
                z[p + 'mask_camera'][i] if cam else None) for i in range(n)]
    return kw, samples, z[p + 'per_sample'], z[p + 'totals']


def case_counts(kw, sample):
    pred, gt, lid, cam = sample
    mask = cam if kw['use_image_mask'] else (lid if kw['use_lidar_mask'] else None)
    return counts(pred, gt, mask, kw['void'], kw['voxel_size'], kw['threshold_acc'], kw['threshold_complete'])
