"""Dataloader-side drop-in for the fine-tune depth supervision: mmdet3d/datasets/pipelines/loading.py:761-844,
`PointToMultiViewDepth`, with the projection and the per-pixel minimum on the device (ops.lidar_depth_maps /
ops.lidar_depth_labels, csrc/pw_depth_sup.hip).

    from preworld_amd import transforms
    transforms.register_pipelines(PIPELINES)          # mmdet's pipeline registry; replaces the reference class (force=True)

The reference builds six dense (H, W) maps on the CPU and the training step ships them to the GPU (17.3 MB per sample at
512 x 1408); here the sweep (about 0.7 MB) goes to the device and either the same `gt_depth` stays there, or -- with
`labels_downsample=` -- only the (6, 32, 88) int32 labels the loss consumes are made (`results['gt_depth_labels']`, which the
detectors' forward_train takes as `gt_depth_labels=`).  Per pixel the EXACT minimum depth wins; the reference's float32 sort key
cannot always separate two depths of one pixel ("Depth supervision from the sweep")."""
import numpy as np
import torch

from . import ops


def quaternion_rotation_matrix(q):
    """Rotation matrix of the quaternion (w, x, y, z) as pyquaternion's `Quaternion(q).rotation_matrix` computes it (float64):
    normalise unless already unit to 1e-14, then the lower-right 3x3 of Q(q) . Qbar(q)^T."""
    w, x, y, z = [float(v) for v in q]
    n = np.sqrt(np.dot([w, x, y, z], [w, x, y, z]))
    if abs(1.0 - n) > 1e-14 and n > 0:
        w, x, y, z = w / n, x / n, y / n, z / n
    Q = np.array([[w, -x, -y, -z], [x, w, -z, y], [y, z, w, -x], [z, -y, x, w]])
    Qb = np.array([[w, -x, -y, -z], [x, w, z, -y], [y, -z, w, x], [z, y, -x, w]])
    return np.dot(Q, Qb.conj().transpose())[1:][:, 1:]


def _pose(rotation, translation):
    m = np.eye(4, dtype=np.float32)
    m[:3, :3] = quaternion_rotation_matrix(rotation)
    m[:3, 3] = translation
    return torch.from_numpy(m)


def compose_lidar2img(curr, cam_names, intrins):
    """loading.py:794-830: per camera, lidar2img = K @ inverse(G_cam @ E_cam) @ (G_lidar @ E_lidar) -- E the sensor's mount on
    its ego frame, G that ego frame's pose in the world at the sensor's timestamp, K the intrinsics padded to 4x4 -- as 4x4
    float32 products on the host, grouped as the reference groups them.  curr: the sample's info dict (lidar2ego_*, ego2global_*,
    cams[name][sensor2ego_* / ego2global_*]); intrins (N,3,3).  Returns (N,4,4) float32."""
    lidar2global = _pose(curr['ego2global_rotation'], curr['ego2global_translation']) @ \
        _pose(curr['lidar2ego_rotation'], curr['lidar2ego_translation'])
    out = []
    for i, name in enumerate(cam_names):
        info = curr['cams'][name]
        cam2global = _pose(info['ego2global_rotation'], info['ego2global_translation']) @ \
            _pose(info['sensor2ego_rotation'], info['sensor2ego_translation'])
        K = torch.eye(4, dtype=torch.float32)
        K[:3, :3] = torch.as_tensor(intrins[i], dtype=torch.float32).cpu()
        out.append(K @ (torch.inverse(cam2global) @ lidar2global))
    return torch.stack(out)


class PointToMultiViewDepth(object):
    """Constructor kwargs and __call__(results) contract of the reference class.  Reads results['points'] (a tensor or an object
    with `.tensor`, x y z first), results['img_inputs'] = (imgs, rots, trans, intrins, post_rots, post_trans, bda),
    results['cam_names'] and results['curr']; writes results['gt_depth'] (N, H // downsample, W // downsample) float32 ON THE
    DEVICE, or -- labels_downsample set (the view transformer's `downsample`, 16) -- results['gt_depth_labels']
    (N, H // downsample // labels_downsample, ...) int32 instead.  grid_config['depth'] = [d0, d1, dstep].

    The call launches kernels, so it belongs in a process that may own the GPU: the training process itself (a loader with
    no worker processes), or workers started with `spawn` -- never a forked worker, where HIP cannot initialise, and every
    worker that does run it is one more process with the GPU open.  With worker processes, leave the points in the batch and
    pass them to forward_train(points=..., lidar2img=...) instead."""

    def __init__(self, grid_config, downsample=1, labels_downsample=None, device='cuda'):
        self.downsample = downsample
        self.grid_config = grid_config
        self.labels_downsample = labels_downsample
        self.device = device

    def __call__(self, results):
        points = results['points']
        points = points.tensor if hasattr(points, 'tensor') else points
        inputs = results['img_inputs']                  # (imgs, rots, trans, intrins, post_rots, post_trans, bda)
        imgs, intrins, post_rots, post_trans = inputs[0], inputs[3], inputs[4], inputs[5]
        n = len(results['cam_names'])
        dev = torch.device(self.device)
        lidar2img = compose_lidar2img(results['curr'], results['cam_names'], intrins).to(dev)[None]
        args = (points.to(dev), lidar2img, post_rots[:n].to(dev)[None], post_trans[:n].to(dev)[None], imgs.shape[2:4])
        if self.labels_downsample:
            results['gt_depth_labels'] = ops.lidar_depth_labels(*args, self.grid_config['depth'], self.labels_downsample,
                                                                downsample=self.downsample)
        else:
            results['gt_depth'] = ops.lidar_depth_maps(*args, self.grid_config['depth'][:2], downsample=self.downsample)[0]
        return results

    def __repr__(self):
        return '%s(grid_config=%r, downsample=%r, labels_downsample=%r)' % (type(self).__name__, self.grid_config, self.downsample,
                                                                             self.labels_downsample)


def register_pipelines(registry):
    """Put PointToMultiViewDepth into an mmcv-style pipeline registry (`register_module(name=None, force=False, module=None)`)
    under the reference's name, replacing the reference class.  Returns the registered names."""
    registry.register_module(name='PointToMultiViewDepth', force=True, module=PointToMultiViewDepth)
    return ['PointToMultiViewDepth']
