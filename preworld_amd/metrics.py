"""Occupancy metrics -- drop-ins for mmdet3d/datasets/occ_metrics.py:52-185 (Metric_mIoU), :322-410 (Metric_FScore) and
:413-594 (Metric_mIoU_Temporal): same constructor flags, add_batch / count_miou / count_fscore semantics.  The
18x18 confusion matrix is accumulated on the GPU (pw_confusion_hist, exact integer work); the
final per-class IoU / nanmean is the reference's numpy arithmetic.  The F-score's neighbour counts are a lattice stencil
on the GPU (pw_occ_fscore) and its float64 totals are folded there with the reference's arithmetic."""
import numpy as np
import torch

from . import ops

CLASS_NAMES = ['others', 'barrier', 'bicycle', 'bus', 'car', 'construction_vehicle', 'motorcycle',
               'pedestrian', 'traffic_cone', 'trailer', 'truck', 'driveable_surface', 'other_flat',
               'sidewalk', 'terrain', 'manmade', 'vegetation', 'free']


def _dev(a, device):
    t = torch.as_tensor(a)
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    return t.to(device)


class Metric_mIoU:
    def __init__(self, save_dir='.', num_classes=18, use_lidar_mask=False, use_image_mask=False,
                 device='cuda:0'):
        self.class_names = CLASS_NAMES
        self.num_classes = num_classes
        self.use_lidar_mask, self.use_image_mask = use_lidar_mask, use_image_mask
        self.device = device
        self._hist = torch.zeros(num_classes, num_classes, dtype=torch.int64, device=device)
        self._occ_hist = torch.zeros(2, 2, dtype=torch.int64, device=device)
        self.cnt = 0

    @property
    def hist(self):
        return self._hist.cpu().numpy().astype(np.float64)

    @property
    def occ_hist(self):
        return self._occ_hist.cpu().numpy().astype(np.float64)

    def add_batch(self, semantics_pred, semantics_gt, mask_lidar, mask_camera):
        self.cnt += 1
        mask = mask_camera if self.use_image_mask else (mask_lidar if self.use_lidar_mask else None)
        p = _dev(semantics_pred, self.device).to(torch.uint8)
        g = _dev(semantics_gt, self.device).to(torch.uint8)
        m = _dev(mask, self.device) if mask is not None else None
        ops.confusion_hist(p, g, m, self.num_classes, self._hist)
        # binary occupied/free histogram (occ_metrics.py:137-141)
        free = self.num_classes - 1
        ops.confusion_hist((p != free).to(torch.uint8), (g != free).to(torch.uint8), m, 2, self._occ_hist)

    def add_counts(self, counts, n=1):
        """add_batch's effect from a device table of n samples' scores: counts (n_cl*n_cl + 4,) or (1, n_cl*n_cl + 4) int64, the
        confusion matrix then the binary 2x2 histogram (ops.occ_score / pw_occ_score).  hist, occ_hist and cnt then equal what
        add_batch gives on the same grids.  Device-side adds on the current stream: no host sync."""
        nb = self.num_classes * self.num_classes
        c = counts.reshape(-1)
        if c.numel() != nb + 4 or c.dtype != torch.int64:
            raise ValueError('add_counts: expected %d int64 entries, got %d %s' % (nb + 4, c.numel(), c.dtype))
        torch._foreach_add_([self._hist.view(-1), self._occ_hist.view(-1)], [c[:nb], c[nb:]])
        self.cnt += int(n)

    @staticmethod
    def per_class_iu(hist):
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.diag(hist) / (hist.sum(1) + hist.sum(0) - np.diag(hist))

    def count_miou(self, verbose=False):
        mIoU = self.per_class_iu(self.hist)
        res = round(np.nanmean(mIoU[:self.num_classes - 1]) * 100, 2)
        if verbose:
            for i in range(self.num_classes):
                print('===> %s - IoU = %s' % (self.class_names[i], round(mIoU[i] * 100, 2)))
            print('===> mIoU of %d samples: %s' % (self.cnt, res))
        return self.class_names, mIoU, self.cnt, res

    def count_iou(self):
        IoU = self.per_class_iu(self.occ_hist)
        return ['free', 'occupied'], IoU, self.cnt, round(IoU[-1] * 100, 2)


class Metric_mIoU_Temporal:
    """Drop-in for occ_metrics.py:413-594, same call signatures and return values:

    * add_batch(semantics_pred, semantics_gt_temp, mask_lidar_temp, mask_camera_temp): `semantics_pred` is the stack of
      states {0,2,4,6} (apis/test.py:218-223); the three dicts are keyed by the ground-truth index idx in {0,2,4,6}
      (keyframes at 2 Hz = 0/1/2/3 s) and idx is scored against semantics_pred[idx // 2] (:505-510);
    * count_miou() -> (per-class IoU at 1 s, [mIoU 1 s, 2 s, 3 s]) (:548-575); count_iou() -> [IoU 1 s, 2 s, 3 s] (:577-594);
    * attributes cnt, hist_{0..3}s, occ_hist_{0..3}s.
    add_idx(...) scores one horizon (what the harness's per-horizon report uses); report() returns every horizon
    incl. 0 s, which the reference accumulates (:533-535) but never prints."""

    def __init__(self, save_dir='.', num_classes=18, use_lidar_mask=False, use_image_mask=False, device='cuda:0'):
        self.class_names = CLASS_NAMES
        self.save_dir, self.num_classes = save_dir, num_classes
        self.use_lidar_mask, self.use_image_mask = use_lidar_mask, use_image_mask
        self.occ_names = ['free', 'occupied']
        self.horizons = (0, 2, 4, 6)
        self.metrics = {h: Metric_mIoU(num_classes=num_classes, use_lidar_mask=use_lidar_mask,
                                       use_image_mask=use_image_mask, device=device)
                        for h in self.horizons}
        self.cnt = 0

    def __getattr__(self, name):
        # hist_0s .. hist_3s / occ_hist_0s .. occ_hist_3s as float arrays, like the reference's numpy accumulators
        for prefix, attr in (('occ_hist_', 'occ_hist'), ('hist_', 'hist')):
            if name.startswith(prefix) and name.endswith('s') and name[len(prefix):-1].isdigit():
                sec = int(name[len(prefix):-1])
                if 2 * sec in self.__dict__.get('metrics', {}):
                    return getattr(self.metrics[2 * sec], attr)
        raise AttributeError(name)

    def add_idx(self, semantics_pred_stack, semantics_gt, mask_lidar, mask_camera, idx):
        assert idx in self.metrics
        self.metrics[idx].add_batch(semantics_pred_stack[idx // 2], semantics_gt, mask_lidar, mask_camera)

    def add_batch(self, semantics_pred, semantics_gt_temp, mask_lidar_temp, mask_camera_temp):
        self.cnt += 1
        for idx in semantics_gt_temp.keys():
            self.add_idx(semantics_pred, semantics_gt_temp[idx],
                         mask_lidar_temp[idx] if mask_lidar_temp is not None else None,
                         mask_camera_temp[idx] if mask_camera_temp is not None else None, idx)

    def add_counts(self, counts, n=1, horizons=None):
        """add_batch's effect from a device table (len(horizons), n_cl*n_cl + 4) int64 of n samples' scores (ops.occ_score; row j
        scores ground-truth index horizons[j], default (0, 2, 4, 6)): hist_*s, occ_hist_*s, cnt, count_miou(), count_iou() and
        report() then equal what add_batch gives on the same stacks."""
        horizons = self.horizons if horizons is None else tuple(horizons)
        if counts.shape[0] != len(horizons) or any(h not in self.metrics for h in horizons):
            raise ValueError('add_counts: one row per horizon of %s, got %s rows for %s' % (self.horizons, counts.shape[0], horizons))
        nb = self.num_classes * self.num_classes
        if counts.dtype != torch.int64 or counts.reshape(len(horizons), -1).shape[1] != nb + 4:
            raise ValueError('add_counts: expected (%d, %d) int64, got %s %s' % (len(horizons), nb + 4, tuple(counts.shape), counts.dtype))
        dst, src = [], []
        for j, h in enumerate(horizons):                  # one multi-tensor add for every horizon's two histograms
            m = self.metrics[h]
            dst += [m._hist.view(-1), m._occ_hist.view(-1)]
            src += [counts[j].reshape(-1)[:nb], counts[j].reshape(-1)[nb:]]
            m.cnt += int(n)
        torch._foreach_add_(dst, src)
        self.cnt += int(n)

    def _miou(self, h):
        iu = Metric_mIoU.per_class_iu(self.metrics[h].hist)
        return iu, round(np.nanmean(iu[:self.num_classes - 1]) * 100, 2)

    def count_miou(self, verbose=False):
        res = []
        for sec in (1, 2, 3):
            iu, m = self._miou(2 * sec)
            if verbose:
                print('===> mIoU of %d samples at %ds: %s' % (self.cnt, sec, m))
            res.append(m)
        return self._miou(2)[0], res

    def count_iou(self):
        res = []
        for sec in (1, 2, 3):
            iu = Metric_mIoU.per_class_iu(self.metrics[2 * sec].occ_hist)
            res.append(round(iu[-1] * 100, 2))
        return res

    def report(self):
        out = {h: self._miou(h)[1] for h in self.horizons}
        out['avg_future'] = round(float(np.mean([out[h] for h in self.horizons if h != 0])), 2)
        return out


class Metric_FScore:
    """Drop-in for occ_metrics.py:322-410 (the Occ3D geometry F-score): same constructor kwargs -- leaf_size is accepted and
    ignored (there is no tree), range only places the reference's points and cannot change a distance -- plus device=.

    * add_batch(semantics_pred, semantics_gt, mask_lidar, mask_camera): one (X, Y, Z) sample, numpy or device arrays.  The
      counts come from one pw_occ_fscore launch (the KDTree queries of :383-397 restated exactly on the voxel lattice, see
      ops.fscore_offsets) and one pw_occ_fscore_accumulate launch folds them into float64 device totals with the reference's
      arithmetic, so tot_acc / tot_cmpl / tot_f1_mean are the same float64 sums.  Unlike the reference (:372-378), the
      caller's arrays are NOT modified when a mask is used.
    * add_counts(table): the same from a device count table (ops.occ_fscore), one row (4,) per sample.
    * count_fscore() prints the reference's line and also returns the value.
    * cnt, tot_acc, tot_cmpl, tot_f1_mean as in the reference (the totals are read from the device: a sync).
    Deviation: a sample with an occupied prediction and an empty ground truth makes the reference raise inside KDTree; here it
    adds (0, 0, 0) and is counted in n_empty_gt."""

    def __init__(self, leaf_size=10, threshold_acc=0.6, threshold_complete=0.6, voxel_size=[0.4, 0.4, 0.4],
                 range=[-40, -40, -1, 40, 40, 5.4], void=[17, 255], use_lidar_mask=False, use_image_mask=False,
                 device='cuda:0', _totals=None, _empty=None):
        self.leaf_size = leaf_size
        self.threshold_acc = threshold_acc
        self.threshold_complete = threshold_complete
        self.voxel_size = voxel_size
        self.range = range
        self.void = void
        self.use_lidar_mask = use_lidar_mask
        self.use_image_mask = use_image_mask
        self.device = device
        self.cnt = 0
        self.eps = 1e-8
        ops.fscore_offsets(threshold_acc, voxel_size)             # a threshold that ties a lattice distance fails here
        ops.fscore_offsets(threshold_complete, voxel_size)
        self._totals = _totals if _totals is not None else torch.zeros(1, 3, dtype=torch.float64, device=device)
        self._empty = _empty if _empty is not None else torch.zeros(1, dtype=torch.int64, device=device)
        self._table = torch.zeros(1, 4, dtype=torch.int64, device=device)

    @classmethod
    def _group(cls, n, **kw):
        """n metrics whose totals are the rows of one (n, 3) tensor: one pw_occ_fscore_accumulate launch adds a sample's
        (n, 4) table to all of them (SampleStream).  Returns (metrics, totals, n_empty_gt)."""
        dev = kw.get('device', 'cuda:0')
        totals = torch.zeros(n, 3, dtype=torch.float64, device=dev)
        empty = torch.zeros(n, dtype=torch.int64, device=dev)
        return [cls(_totals=totals[j:j + 1], _empty=empty[j:j + 1], **kw) for j in range(n)], totals, empty

    def kernel_args(self):
        """the keyword arguments of ops.occ_fscore this metric scores with"""
        return dict(void=tuple(self.void), voxel_size=tuple(self.voxel_size), thr_acc=self.threshold_acc,
                    thr_cmpl=self.threshold_complete)

    @property
    def tot_acc(self):
        return float(self._totals[0, 0].item())

    @property
    def tot_cmpl(self):
        return float(self._totals[0, 1].item())

    @property
    def tot_f1_mean(self):
        return float(self._totals[0, 2].item())

    @property
    def n_empty_gt(self):
        """samples with an occupied prediction and no occupied ground truth (the reference raises on them)"""
        return int(self._empty[0].item())

    def add_batch(self, semantics_pred, semantics_gt, mask_lidar, mask_camera):
        mask = mask_camera if self.use_image_mask else (mask_lidar if self.use_lidar_mask else None)
        p = _dev(semantics_pred, self.device).to(torch.uint8).contiguous()
        g = _dev(semantics_gt, self.device).to(torch.uint8).contiguous()
        m = _dev(mask, self.device).to(torch.uint8).contiguous() if mask is not None else None
        if p.dim() != 3:
            raise ValueError('Metric_FScore.add_batch: expected one (X, Y, Z) grid, got %s' % (tuple(p.shape),))
        self._table.zero_()
        ops.occ_fscore([p], [g], [m] if m is not None else None, self._table, **self.kernel_args())
        ops.occ_fscore_accumulate(self._table, self._totals, self._empty)
        self.cnt += 1

    def add_counts(self, table):
        """add_batch's effect from a device count table of n samples (ops.occ_fscore rows {n_pred, n_pred_hit, n_gt, n_gt_hit}):
        (4,), (1, 4), (n, 4) or (n, 1, 4) int64, one row per sample, folded in row order.  No host sync."""
        if table.dtype != torch.int64 or table.numel() % 4 or table.shape[-1] != 4:
            raise ValueError('add_counts: expected (n, 4) int64 rows, got %s %s' % (tuple(table.shape), table.dtype))
        t = table.reshape(-1, 1, 4)
        ops.occ_fscore_accumulate(t, self._totals, self._empty)
        self.cnt += t.shape[0]

    def count_fscore(self):
        value = self.tot_f1_mean / self.cnt
        line = '\n######## F score: {} #######'.format(value)
        try:
            from termcolor import colored
            line = colored(line, 'red', attrs=['bold', 'dark'])
        except ImportError:
            pass
        print(line)
        return value
