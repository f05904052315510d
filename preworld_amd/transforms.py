"""Dataloader-side drop-in for the fine-tune depth supervision: mmdet3d/datasets/pipelines/loading.py:761-844,
`PointToMultiViewDepth`, with the projection and the per-pixel minimum on the device (ops.lidar_depth_maps /
ops.lidar_depth_labels, csrc/pw_depth_sup.hip).

    from preworld_amd import transforms
    transforms.register_pipelines(PIPELINES)          # mmdet's pipeline registry; replaces the reference class (force=True)

The reference builds six dense (H, W) maps on the CPU and the training step ships them to the GPU (17.3 MB per sample at
512 x 1408); here the sweep (about 0.7 MB) goes to the device and either the same `gt_depth` stays there, or -- with
`labels_downsample=` -- only the (6, 32, 88) int32 labels the loss consumes are made (`results['gt_depth_labels']`, which the
detectors' forward_train takes as `gt_depth_labels=`).  Per pixel the EXACT minimum depth wins; the reference's float32 sort key
cannot always separate two depths of one pixel ("Depth supervision from the sweep").

`PrepareImageInputs` / `PrepareImageInputs4DTraj` (loading.py:902-1140, loading_traj_temporal.py:230-577) are here too: camera
frames -> the network's `img_inputs`, with resize / crop / flip / rotate / normalise on the device (ops.prepare_images,
csrc/pw_image_prep.hip); `transforms.register_image_pipelines(PIPELINES)` ("Camera frames to network input").

`SweepsToRays` is the pre-train twin of PointToMultiViewDepth: sweeps with their lidarseg bytes + the staged frames -> the ray
table of the reference's `get_rays` (ops.ray_table, csrc/pw_ray_labels.hip); `transforms.register_ray_pipelines(PIPELINES)`
("Ray supervision from the sweep")."""
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


def compose_view_poses(infos, cam_names):
    """Stage A's poses (tools/gen_data/gen_depth_gt.py:17-52, map_pointcloud_to_image) for every sweep of `infos` and every
    camera of that sweep's own sample: (T N, 57) float64 rows R1 t1 (lidar->ego), R2 t2 (ego->global), -t3 R3^T (global->camera
    ego), -t4 R4^T (camera ego->camera), K -- rotations from the quaternions in float64, nothing rounded here (the kernel
    rounds the translations to float32 as the devkit's float32 cloud does).  View v = t N + camera."""
    rows = []
    for info in infos:
        for name in cam_names:
            cam = info['cams'][name]
            rows.append(np.concatenate([
                quaternion_rotation_matrix(info['lidar2ego_rotation']).ravel(), np.asarray(info['lidar2ego_translation'], np.float64),
                quaternion_rotation_matrix(info['ego2global_rotation']).ravel(), np.asarray(info['ego2global_translation'], np.float64),
                -np.asarray(cam['ego2global_translation'], np.float64), quaternion_rotation_matrix(cam['ego2global_rotation']).T.ravel(),
                -np.asarray(cam['sensor2ego_translation'], np.float64), quaternion_rotation_matrix(cam['sensor2ego_rotation']).T.ravel(),
                np.asarray(cam['cam_intrinsic'], np.float64).ravel()]))
    return torch.from_numpy(np.stack(rows))


def compose_sensor2keyegos(infos, cam_names):
    """nuscenes_dataset_occ.py:248-259: sensor2keyego = inverse(keyego2global) @ ego2global @ sensor2ego per view, the float32
    poses multiplied in float64 and rounded to float32; keyego2global is the same camera's ego pose in the first (key) frame.
    infos: the frames in [0] + aux_frames order.  Returns (T N, 4, 4) float32 on the host."""
    s2e = torch.stack([_pose(info['cams'][n]['sensor2ego_rotation'], info['cams'][n]['sensor2ego_translation'])
                       for info in infos for n in cam_names]).view(len(infos), len(cam_names), 4, 4)
    e2g = torch.stack([_pose(info['cams'][n]['ego2global_rotation'], info['cams'][n]['ego2global_translation'])
                       for info in infos for n in cam_names]).view(len(infos), len(cam_names), 4, 4)
    global2keyego = torch.inverse(e2g[0:1].double())
    return (global2keyego @ e2g.double() @ s2e.double()).float().view(-1, 4, 4)


class SweepsToRays(object):
    """The ray supervision of the pre-train dataloader (nuscenes_dataset_occ.py:197-270, get_rays) as a pipeline step, from what
    a training run already has on the device: no gen_depth_gt / gen_seg_gt_from_lidarseg directories, no per-camera loop
    (ops.ray_table, csrc/pw_ray_labels.hip).  Sits beside PointToMultiViewDepth.

    Reads results['curr'] (the key sample's info dict: scene_token, lidar2ego_*, ego2global_*, cams) and results['ray_frames'],
    {frame id: dict(info=..., points=(P, >= 3) tensor or object with .tensor, point_labels=uint8 (P) lidarseg bytes, frames=
    uint8 (N, H, W, 3) tensor)} for frame ids [0] + aux_frames; or, with results['ray_staged'] = the staged uint8 (M, H, W, 3)
    buffer of PrepareImageInputs4DTraj, frame_index=[N indices into it] in place of frames= (nothing is copied then).  Frames are picked
    as get_rays picks them: a neighbour that is missing or belongs to another scene falls back to the key sample (entry 0).
    Writes results['rays']: (R, 16), or (max_ray_nums, 16) drawn by weight when R is larger; with capacity= set,
    (table, weights, n_rows) without synchronising (rays.generate_rays_from_sweeps).

    label_lut (256 entries, lidarseg byte -> class), dynamic_class (the classes weighted by weight_dyn in the auxiliary frames; None:
    none, as in rays.generate_rays) and class_nums (the dataset-level ray counts per class, from which the
    balance weights exp(0.005 (max / n - 1)) are made; None or wrs_use_batch: the batch's own counts) are the caller's.
    The process rules of PointToMultiViewDepth hold: no forked workers."""

    def __init__(self, aux_frames=(-1, 1), max_ray_nums=0, wrs_use_batch=False, class_nums=None, dynamic_class=None,
                 label_lut=None, weight_adj=0.3, weight_dyn=0.0, capacity=None, device='cuda'):
        self.aux_frames = list(aux_frames)
        self.max_ray_nums = max_ray_nums
        self.balance_weight = None
        if not wrs_use_batch and class_nums is not None:
            n = torch.as_tensor(class_nums, dtype=torch.float32)
            self.balance_weight = torch.exp(0.005 * (n.max() / n - 1))
        self.dynamic_class = None if dynamic_class is None else torch.tensor(list(dynamic_class), dtype=torch.int32)
        self.label_lut = label_lut
        self.weight_adj, self.weight_dyn, self.capacity, self.device = weight_adj, weight_dyn, capacity, device

    def pick_frames(self, results):
        """-> ([frame ids], [the entry used for each]) in [0] + aux_frames order"""
        key = results['ray_frames'][0]
        scene = results['curr']['scene_token']
        ids, picked = [0] + self.aux_frames, []
        for time_id in ids:
            entry = results['ray_frames'].get(time_id)
            if entry is None or entry['info']['scene_token'] != scene:
                entry = key                                # out of sequence
            picked.append(entry)
        return ids, picked

    def __call__(self, results):
        from . import rays
        dev = torch.device(self.device)
        ids, picked = self.pick_frames(results)
        cam_names = list(picked[0]['info']['cams'].keys())
        infos = [e['info'] for e in picked]
        N = len(cam_names)
        points = [(e['points'].tensor if hasattr(e['points'], 'tensor') else e['points']).to(dev) for e in picked]
        labels = [torch.as_tensor(e['point_labels']).to(dev) for e in picked]
        if 'ray_staged' in results:                        # the staged buffer of PrepareImageInputs4DTraj + indices into it: no copy
            frames = results['ray_staged'].to(dev)
            view_frame = [int(i) for e in picked for i in e['frame_index']]
        else:                                              # one (N,H,W,3) tensor per frame: each distinct one once
            uniq = []
            for e in picked:
                if not any(e is u for u in uniq):
                    uniq.append(e)
            frames = uniq[0]['frames'].to(dev) if len(uniq) == 1 else torch.cat([u['frames'].to(dev) for u in uniq], 0)
            view_frame = [[e is u for u in uniq].index(True) * N + c for e in picked for c in range(N)]
        intrins = torch.tensor([info['cams'][n]['cam_intrinsic'] for info in infos for n in cam_names], dtype=torch.float32)
        time_ids = {t: list(range(k * N, (k + 1) * N)) for k, t in enumerate(ids)}
        results['rays'] = rays.generate_rays_from_sweeps(
            points, labels, frames, compose_view_poses(infos, cam_names), compose_sensor2keyegos(infos, cam_names), intrins,
            max_ray_nums=self.max_ray_nums, time_ids=time_ids, dynamic_class=self.dynamic_class, balance_weight=self.balance_weight,
            weight_adj=self.weight_adj, weight_dyn=self.weight_dyn, label_lut=self.label_lut, capacity=self.capacity,
            view_frame=view_frame)
        return results

    def __repr__(self):
        return '%s(aux_frames=%r, max_ray_nums=%r, capacity=%r)' % (type(self).__name__, self.aux_frames, self.max_ray_nums, self.capacity)


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


def _pil_loader(path):
    from PIL import Image                    # only needed when the frames are not handed in
    return np.asarray(Image.open(path).convert('RGB'))


def _frame_u8(f):
    f = f.cpu().numpy() if isinstance(f, torch.Tensor) else np.asarray(f)
    if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3:
        raise ValueError('a frame must be a uint8 (H, W, 3) RGB array, got %s %s' % (f.dtype, f.shape))
    return f


class PrepareImageInputs(object):
    """Drop-in for mmdet3d/datasets/pipelines/loading.py:902-1140 with the pixel work on the device (ops.prepare_images,
    csrc/pw_image_prep.hip): PIL's antialiased bicubic resize, crop with zero fill, flip, nearest rotation and mmlabNormalize for
    all frames of the sample in one call.  Constructor kwargs and __call__(results) contract of the reference class;
    data_config = dict(cams, Ncams, input_size, resize, rot, flip, crop_h[, resize_test]).

    Reads results['curr'] (and ['adjacent'] when sequential).  Pixels: results['frames'], one uint8 (H, W, 3) RGB array or
    tensor per image in the order the reference opens files (camera by camera, the key frame then its adjacent frames) --
    else `loader(data_path)`, by default PIL.  JPEG decoding stays on the host; the frames of a call go to the device as one
    uint8 copy from pinned memory.  Writes results['img_inputs'] = (imgs (N F, 3, fH, fW) float32 ON THE DEVICE, camera-major /
    frame-minor; sensor2egos, ego2globals, intrins, post_rots, post_trans on the host, frame-major, as the reference has
    them), results['canvas'] (the key frames' uint8 images, bit-equal to PIL's), results['gt_depths'] (zeros(1) per camera)
    and results['cam_names'].  Augmentations are drawn from np.random in the reference's order: the same seed gives the same
    sample.  Channel 0 of imgs is the BLUE plane: the reference applies to_rgb to an array that is already RGB.

    load_depth=True is not implemented (no released config sets it; PointToMultiViewDepth / get_depth_labels cover the need).

    The call launches kernels, so it belongs in a process that may own the GPU: the training process itself (a loader with
    no worker processes), or workers started with `spawn` -- never a forked worker, where HIP cannot initialise, and every
    worker that does run it is one more process with the GPU open."""

    def __init__(self, data_config, is_train=False, sequential=False, load_depth=False, depth_gt_path=None, loader=None,
                 device='cuda'):
        if load_depth:
            raise NotImplementedError('load_depth=True is not supported: use PointToMultiViewDepth or get_depth_labels')
        self.is_train = is_train
        self.data_config = data_config
        self.sequential = sequential
        self.load_depth = load_depth
        self.depth_gt_path = depth_gt_path
        self.loader = loader or _pil_loader
        self.device = device
        self._plans = {}
        self._pinned = None

    # ---- sampling: np.random is consumed in the reference's order (scale, kept height, left edge, mirror, angle), so one seed
    # gives one sample on both sides
    def choose_cams(self):
        """the cameras of this sample: all of data_config['cams'], or, in training with Ncams below that, Ncams of them drawn
        without replacement"""
        names, wanted = self.data_config['cams'], self.data_config['Ncams']
        if not self.is_train or wanted >= len(names):
            return names
        return np.random.choice(names, wanted, replace=False)

    def _window(self, H, W, scale_delta, drop_bottom, left_edge):
        """scale = fW / W + scale_delta; the resized size truncates; the crop keeps fH rows ending `drop_bottom` (a fraction
        of the resized height) above the bottom edge and fW columns from left_edge(spare columns).  -> scale, dims, box"""
        fH, fW = self.data_config['input_size']
        scale = float(fW) / float(W) + scale_delta
        dims = (int(W * scale), int(H * scale))
        top = int((1 - drop_bottom(dims[1])) * dims[1]) - fH
        left = left_edge(max(0, dims[0] - fW))
        return scale, dims, (left, top, left + fW, top + fH)

    def _fixed_augmentation(self, H, W, flip, scale):
        """test time: the centred window, no rotation; `scale` overrides data_config['resize_test']"""
        cfg = self.data_config
        delta = cfg.get('resize_test', 0.0) if scale is None else scale
        geo = self._window(H, W, delta, lambda _: np.mean(cfg['crop_h']), lambda spare: int(spare / 2))
        return geo + (False if flip is None else flip, 0)

    def sample_augmentation(self, H, W, flip=None, scale=None):
        """-> (resize, resize_dims, crop, flip, rotate) as loading.py:975-1001 returns them"""
        if not self.is_train:
            return self._fixed_augmentation(H, W, flip, scale)
        cfg, rnd = self.data_config, np.random
        geo = self._window(H, W, rnd.uniform(*cfg['resize']), lambda _: rnd.uniform(*cfg['crop_h']),
                           lambda spare: int(rnd.uniform(0, spare)))
        mirrored = cfg['flip'] and rnd.choice([0, 1])          # no draw when the config switches the flip off
        return geo + (mirrored, rnd.uniform(*cfg['rot']))

    # ---- bookkeeping: float32 torch products in the reference's order (loading.py:940-951), so post_rots / post_trans are
    # bit-equal to its tensors
    @staticmethod
    def _after(lin, shift, rot, tran):
        """x -> lin x + shift applied after x -> rot x + tran"""
        return torch.matmul(lin, rot), torch.matmul(lin, tran) + shift

    def img_transform(self, resize, crop, flip, rotate):
        """the 2 x 2 / 2-vector pixel map of one augmentation: scale, move to the crop origin, mirror about the window, turn
        about its centre"""
        f32 = torch.float32
        x0, y0, x1, y1 = crop
        size = torch.tensor([x1 - x0, y1 - y0], dtype=f32)
        rot, tran = torch.eye(2) * resize, torch.zeros(2) - torch.tensor([x0, y0], dtype=f32)
        if flip:
            rot, tran = self._after(torch.tensor([[-1.0, 0.0], [0.0, 1.0]]), size * torch.tensor([1.0, 0.0]), rot, tran)
        h = rotate / 180 * np.pi
        turn = torch.tensor([[np.cos(h), np.sin(h)], [-np.sin(h), np.cos(h)]], dtype=f32)
        centre = size / 2
        return self._after(turn, torch.matmul(turn, -centre) + centre, rot, tran)

    def get_sensor_transforms(self, cam_info, cam_name):
        """(sensor2ego, ego2global) 4 x 4 float32 of one camera of an info dict"""
        cam = cam_info['cams'][cam_name]
        return tuple(_pose(cam[k + '_rotation'], cam[k + '_translation']) for k in ('sensor2ego', 'ego2global'))

    # ---- one pass over an info dict: bookkeeping now, pixels later
    def _collect(self, info, cam_names, frames, job, sampler, flip=None, scale=None):
        """Walks the cameras of info['curr'] (and, when sequential, of each info['adjacent'] frame) in the order the reference
        opens files, appends (frame, aug) to `job` camera-major / frame-minor and returns (n_images, (sensor2egos, ego2globals,
        intrins, post_rots, post_trans) frame-major, positions of the key frames in the job).  One augmentation per camera,
        shared by its adjacent frames; the flip handed to the sampler is the previous camera's, as in the reference."""
        older = list(info['adjacent']) if self.sequential else []
        n0, keys, per_cam = len(job), [], []
        for name in cam_names:
            cam = info['curr']['cams'][name]
            key_frame = frames(cam['data_path'])
            resize, dims, crop, flip, rotate = sampler(H=key_frame.shape[0], W=key_frame.shape[1], flip=flip, scale=scale)
            rot3, tran3 = torch.eye(3), torch.zeros(3)
            rot3[:2, :2], tran3[:2] = self.img_transform(resize, crop, flip, rotate)
            per_cam.append((torch.tensor(cam['cam_intrinsic'], dtype=torch.float32), rot3, tran3))
            keys.append(len(job))
            job.append((key_frame, (dims, crop, flip, rotate)))
            job.extend((frames(past['cams'][name]['data_path']), (dims, crop, flip, rotate)) for past in older)
        poses = [self.get_sensor_transforms(frame_info, name) for frame_info in [info['curr']] + older for name in cam_names]
        n_frames = 1 + len(older)
        small = [torch.stack([p[i] for p in poses]) for i in (0, 1)] + \
                [torch.stack([c[i] for c in per_cam] * n_frames) for i in (0, 1, 2)]
        return len(job) - n0, tuple(small), keys

    def _frame_source(self, results):
        if 'frames' in results:
            it = iter(results['frames'])
            return lambda path: _frame_u8(next(it))
        return lambda path: _frame_u8(self.loader(path))

    def _run(self, job):
        """all frames of the call: one pinned uint8 staging buffer, one copy, one ops.prepare_images"""
        M = len(job)
        H, W = job[0][0].shape[:2]
        fH, fW = self.data_config['input_size']
        if any(f.shape[:2] != (H, W) for f, _ in job):
            raise ValueError('all frames of a call must have one size')
        key = (H, W, fH, fW, tuple((tuple(a[0]), tuple(a[1]), bool(a[2]), float(a[3])) for _, a in job))
        plan = self._plans.get(key)
        if plan is None:
            if len(self._plans) >= 8:            # training draws a new augmentation every call: keep the few that repeat
                self._plans.clear()
            plan = self._plans[key] = ops.image_prep_plan((H, W), (fH, fW), [a for _, a in job], device=self.device)
        dev = torch.device(self.device)
        if self._pinned is None or self._pinned.shape != (M, H, W, 3):
            self._pinned = torch.empty((M, H, W, 3), dtype=torch.uint8, pin_memory=dev.type == 'cuda')
        else:
            torch.cuda.current_stream(dev).synchronize()     # the previous call's copy has to be out of the staging buffer
        stage = self._pinned.numpy()
        for i, (f, _) in enumerate(job):
            stage[i] = f
        src = self._pinned.to(dev, non_blocking=True)
        canvas = torch.empty((M, fH, fW, 3), dtype=torch.uint8, device=dev)
        return ops.prepare_images(src, plan, canvas=canvas), canvas

    def get_inputs(self, results, job, frames, flip=None, scale=None):
        cam_names = self.choose_cams()
        results['cam_names'] = cam_names
        return self._collect(results, cam_names, frames, job, self.sample_augmentation, flip, scale)

    def __call__(self, results):
        job = []
        n, small, keys = self.get_inputs(results, job, self._frame_source(results))
        imgs, canvas = self._run(job)
        results['img_inputs'] = (imgs[:n],) + small
        results['gt_depths'] = torch.stack([torch.zeros(1) for _ in keys])
        results['canvas'] = [c for c in canvas[keys].cpu().numpy()]
        return results

    def __repr__(self):
        return '%s(is_train=%r, sequential=%r, input_size=%r)' % (type(self).__name__, self.is_train, self.sequential,
                                                                   self.data_config.get('input_size'))


class PrepareImageInputs4DTraj(PrepareImageInputs):
    """Drop-in for mmdet3d/datasets/pipelines/loading_traj_temporal.py:230-577: PrepareImageInputs plus
    results['temporal_img_inputs'][1..6], the same six-tuple for each of results['temporal_ann_infos'][k] = {curr, adjacent},
    always at the test-time augmentation (sample_augmentation_temporal, :464-478).  All 7 groups of frames go through ONE
    ops.prepare_images call; results['frames'], when given, lists them group by group.  The process rules of
    PrepareImageInputs hold: no forked workers."""

    def sample_augmentation_temporal(self, H, W, flip=None, scale=None):
        """the future groups are always taken at the test-time augmentation (loading_traj_temporal.py:464-478)"""
        return self._fixed_augmentation(H, W, flip, scale)

    def __call__(self, results):
        job = []
        frames = self._frame_source(results)
        n, small, keys = self.get_inputs(results, job, frames)
        groups = []
        for interval in [1, 2, 3, 4, 5, 6]:
            cam_names = self.choose_cams()
            groups.append(self._collect(results['temporal_ann_infos'][interval], cam_names, frames, job,
                                        self.sample_augmentation_temporal))
        imgs, canvas = self._run(job)
        results['img_inputs'] = (imgs[:n],) + small
        results['gt_depths'] = torch.stack([torch.zeros(1) for _ in keys])
        results['canvas'] = [c for c in canvas[keys].cpu().numpy()]
        results['temporal_img_inputs'] = {}
        at = n
        for interval, (m, sm, _) in zip([1, 2, 3, 4, 5, 6], groups):
            results['temporal_img_inputs'][interval] = (imgs[at:at + m],) + sm
            at += m
        return results


def register_pipelines(registry):
    """Put PointToMultiViewDepth into an mmcv-style pipeline registry (`register_module(name=None, force=False, module=None)`)
    under the reference's name, replacing the reference class.  Returns the registered names."""
    registry.register_module(name='PointToMultiViewDepth', force=True, module=PointToMultiViewDepth)
    return ['PointToMultiViewDepth']


def register_ray_pipelines(registry):
    """Put SweepsToRays into an mmcv-style pipeline registry.  The reference has no pipeline class of this name (its dataset
    builds the rays in get_rays), so nothing is replaced.  Returns the registered names."""
    registry.register_module(name='SweepsToRays', force=True, module=SweepsToRays)
    return ['SweepsToRays']


def register_image_pipelines(registry):
    """Put PrepareImageInputs and PrepareImageInputs4DTraj into an mmcv-style pipeline registry under the reference's names,
    replacing the reference classes.  Returns the registered names."""
    registry.register_module(name='PrepareImageInputs', force=True, module=PrepareImageInputs)
    registry.register_module(name='PrepareImageInputs4DTraj', force=True, module=PrepareImageInputs4DTraj)
    return ['PrepareImageInputs', 'PrepareImageInputs4DTraj']
