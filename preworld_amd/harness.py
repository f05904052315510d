"""Row H of SURVEY.md 8a: what replaces tools/test_temporal.py + mmdet3d/apis/test.py for the hot
path -- build the detector from a restated config dict, load a state dict by the reference's key
names, feed lifted inputs, collect `semantic_occ_{k}s`, stack states 0/2/4/6
(mmdet3d/apis/test.py:218-223) and score them with Metric_mIoU_Temporal
(mmdet3d/datasets/occ_metrics.py:413-594).  GPU only: every op goes through libpreworld_hip.so."""
import collections
import collections.abc
import os
import time

import numpy as np
import torch

from . import builder, metrics, synth


def model_cfg(grid_config=None, with_prev=True, if_post_finetune=True, detector='PreWorld4DTraj'):
    """The `model = dict(...)` section of configs/preworld/**.py restricted to the hot path
    (bevstereo-occ.py:62-131 + preworld-7frame-finetune[-traj].py), as a plain dict; the image side
    (img_backbone / img_neck) is left out: benches and parity tests start from the lifted inputs."""
    gc = grid_config or synth.GRID_CONFIG_FULL
    sx = int(round((gc['x'][1] - gc['x'][0]) / gc['x'][2]))
    sy = int(round((gc['y'][1] - gc['y'][0]) / gc['y'][2]))
    sz = int(round((gc['z'][1] - gc['z'][0]) / gc['z'][2]))
    return dict(
        type=detector,
        img_view_transformer=dict(type='LSSViewTransformerBEVStereo', grid_config=gc,
                                  input_size=synth.INPUT_SIZE, in_channels=512, out_channels=32, sid=False,
                                  collapse_z=False, loss_depth_weight=0.05,
                                  depthnet_cfg=dict(use_dcn=False, aspp_mid_channels=96, stereo=True, bias=5.0),
                                  downsample=16),
        img_bev_encoder_backbone=dict(type='CustomResNet3D', numC_input=64, num_layer=[1, 2, 4], with_cp=False,
                                      num_channels=[32, 64, 128], stride=[1, 2, 2], backbone_output_ids=[0, 1, 2]),
        img_bev_encoder_neck=dict(type='LSSFPN3D', in_channels=224, out_channels=32),
        pre_process=dict(type='CustomResNet3D', numC_input=32, with_cp=False, num_layer=[1], num_channels=[32],
                         stride=[1], backbone_output_ids=[0]),
        occupancy_head=dict(type='OccHead', with_cp=False, use_deblock=False,
                            norm_cfg=dict(type='SyncBN', requires_grad=True), soft_weights=True,
                            final_occ_size=[sx, sy, sz], empty_idx=17, num_level=1, in_channels=[32],
                            out_channel=18, point_cloud_range=[gc['x'][0], gc['y'][0], gc['z'][0],
                                                               gc['x'][1], gc['y'][1], gc['z'][1]]),
        if_post_finetune=if_post_finetune, with_prev=with_prev)


def build_model(cfg, state_dict, device='cuda:0'):
    """cfg: model_cfg(...) or the reference's own `model` dict (type PreWorld / PreWorld4DTraj / BEVStereo4DOCC);
    state_dict: numpy or torch tensors under the reference's key names.  Hot-path keys must all be present; image-side
    keys (img_backbone / img_neck / depth_net) may be absent when only lifted inputs are fed."""
    net = builder.build(cfg, 'PreWorld4DTraj')
    sd = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in state_dict.items()}
    missing, _ = net.load_state_dict(sd, strict=False)
    # (nerf_head.*: five registered buffers the constructor recomputes from the config, nerf_head.py:134-144)
    image_side = ('depth_net', 'img_backbone', 'img_neck', 'num_batches_tracked', 'nerf_head.')
    bad = [k for k in missing if not any(t in k for t in image_side)]
    if bad:
        raise KeyError('state dict lacks hot-path keys: %s' % bad[:8])
    return net.to(device).eval()


def lifted_frames(seed, grid_cams, device='cuda:0', n_frames=2):
    """Synthetic (depth, context, camera) inputs of SURVEY.md 8d for `n_frames` frames (key first)."""
    def T(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(device)
    frames = []
    for f in range(n_frames):
        rig = synth.synthetic_rig(grid_cams, dx=-2.5 * f)
        depth, feat = synth.lift_inputs(seed * 16 + f, N=grid_cams)
        frames.append(dict(depth=T(depth).view(grid_cams, 88, 32, 88), tran_feat=T(feat).view(grid_cams, 32, 32, 88),
                           sensor2keyego=T(rig['sensor2ego']), intrin=T(rig['intrin']),
                           post_rot=T(rig['post_rot']), post_tran=T(rig['post_tran']), bda=T(rig['bda'])))
    return frames


def stack_states(result, horizons=(0, 2, 4, 6)):
    """apis/test.py:218-223: [np.stack([semantic_occ_0s, _2s, _4s, _6s])] of sample 0."""
    return np.stack([result['semantic_occ_%ds' % h][0].cpu().numpy() for h in horizons], axis=0)


@torch.no_grad()
def evaluate(net, samples, device='cuda:0', use_image_mask=True, fscore=None):
    """samples: iterable of dict(frames, ego, gt {idx: (X,Y,Z) uint8}, mask_camera (X,Y,Z) bool).
    Scores the stacked states {0,2,4,6} like tools/test_temporal.py -> dataset.evaluate
    (nuscenes_dataset_occ_trajectory.py:478-526).  Returns (Metric_mIoU_Temporal.report() dict incl. the 0 s horizon and
    'avg_future', list of stacked predictions); the reference's own return values are metric.count_miou() /
    count_iou() of the same object (third return value).
    fscore: None, or a dict of Metric_FScore keyword arguments plus mask=None | 'camera' | 'lidar' (the sample entry it reads):
    every horizon is also scored by a Metric_FScore (occ_metrics.py:322-410), report['fscore'] = {idx: tot_f1_mean / cnt} and
    metric.fscore = {idx: Metric_FScore}."""
    metric = metrics.Metric_mIoU_Temporal(num_classes=18, use_image_mask=use_image_mask, device=device)
    fs = _fscore_metrics(fscore, metric.horizons, device) if fscore is not None else None
    stacks = []
    for s in samples:
        res = net.simple_test_from_lift(s['frames'], s['ego'], n_steps=6)
        st = stack_states(res)
        stacks.append(st)
        mc = s.get('mask_camera')
        metric.add_batch(st, s['gt'], None, {h: mc for h in s['gt']} if mc is not None else None)
        if fs is not None:
            for h, f in fs.items():
                ml, mc_ = s.get('mask_lidar'), s.get('mask_camera')
                f.add_batch(st[h // 2], s['gt'][h], ml[h] if isinstance(ml, dict) else ml, mc_[h] if isinstance(mc_, dict) else mc_)
    report = metric.report()
    if fs is not None:
        metric.fscore = fs
        report['fscore'] = {h: f.tot_f1_mean / f.cnt for h, f in fs.items()}
    return report, stacks, metric


def _fscore_metrics(fscore, horizons, device):
    kw = dict(fscore)
    mask = kw.pop('mask', None)
    if mask not in ('camera', 'lidar', None):
        raise ValueError("fscore['mask'] must be 'camera', 'lidar' or None, got %r" % (mask,))
    return {h: metrics.Metric_FScore(use_image_mask=mask == 'camera', use_lidar_mask=mask == 'lidar', device=device, **kw)
            for h in horizons}


@torch.no_grad()
def simple_test_sharded(net, frames, ego, n_steps=6, group=None, gather_on_host=False, timings=None):
    """The latency mode of DESIGN.md section 7 wired to the real modules (one process per GPU, torch.distributed
    initialised): frame f is lifted + pre-processed on rank f % W and all ranks receive every frame's (B,Z,Y,X,32)
    feature through ONE all_gather (parallel.lift_frames_sharded), every rank runs the encoder, state k is forecast +
    decoded on rank k % W, one all_gather of the uint8 grids assembles all states on every rank.
    Returns {'semantic_occ_%ds': [(X,Y,Z) uint8]} like simple_test_from_lift.  `with_prev=False` drops the adjacent
    frames: their channel slice is zeros (bevdet_occ.py:243-258), exactly as in extract_bev_feat_cl.
    gather_on_host=True moves the 0.64 MB grids through host memory (for process groups that cannot all_gather device
    tensors: gloo in the tests; RCCL takes device tensors).
    timings: a dict that receives the milliseconds of the LAST pass's phases on this rank -- lift (LSS + pre_process of this rank's
    frames), gather_frames (the 81.92 MB per frame all_gather), encoder (cat + bev_encoder + final_conv), decode (this rank's
    share of the recursion + OccHead), gather_states (the uint8 all_gather) -- from HIP events on the current stream (synchronises) --
    and the payload bytes of the two exchanges on this rank (frames_bytes_received / _sent, states_bytes_received)."""
    from . import ops, parallel
    from .modules import precision
    vt = net.img_view_transformer
    _, _, size = vt._grid()
    f0 = frames[0]
    B, C = f0['sensor2keyego'].shape[0], vt.out_channels
    n = net.num_adj + 1
    use = frames[:n] if net.with_prev else frames[:1]
    # The exchanged features are fp32 values: an h2 buffer is only meaningful together with the exponent of its range slot,
    # which every rank calibrates for itself (ops.RangeCtx).  On the split-fp16 path a frame is lifted in h2, expanded
    # (hi + lo) * 2^e -- exact -- for the all_gather, and the concatenated buffer is split again under ONE exponent derived
    # from its own maximum, which is the same number on every rank.
    h2 = precision() == 'h2' and C % 32 == 0
    from .modules import as_f32

    def lift(fr):
        return as_f32(net.lift_frame_cl(out_h2=h2, **fr))

    def decode(f):
        occ = net.occupancy_head.decode_cl(f, transposed=True)
        occ = occ.permute(0, 3, 2, 1)[0].contiguous()                          # batch element 0, (X,Y,Z) (:306)
        return occ.cpu() if gather_on_host else occ

    events = []

    def mark(name):
        if timings is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            events.append((name, e))

    def one_pass():
        del events[:]
        mark('start')
        lifted = parallel.lift_frames_sharded(use, lift, (B, size[2], size[1], size[0], C), torch.float32, f0['depth'].device,
                                              group, via_host=gather_on_host, mark=mark, stats=timings)
        x = torch.cat(lifted[1:][::-1] + lifted[:1], dim=-1)                   # [adjacent ..., key] (bevdet_occ.py:266)
        if len(lifted) < n:
            x = torch.cat([x.new_zeros(x.shape[:-1] + ((n - len(lifted)) * C,)), x], dim=-1)
        # final_conv -> forecast -> OccHead keep h2 storage like simple_test_from_lift (post-finetune decode)
        v0 = net.final_conv.forward_cl(net.bev_encoder_cl(ops.f32_to_h2(x) if h2 else x, out_h2=h2), out_h2=h2)
        mark('encoder')
        return parallel.decode_states_sharded(v0, lambda v, k: net.forecast_cl(v, ego, k, out_h2=h2)[0], decode,
                                              n_steps + 1, group, mark=mark, stats=timings,
                                              grid_like=((int(size[0]), int(size[1]), int(size[2])), torch.uint8,
                                                         'cpu' if gather_on_host else f0['depth'].device))

    if h2:
        # ranks own different tensors, so they must agree on whether another calibration pass runs (the passes contain
        # collectives): one tiny MIN all-reduce per pass
        ctx = net.__dict__.get('_range_ctx_sharded')
        if ctx is None or ctx.device != f0['depth'].device:
            ctx = net.__dict__['_range_ctx_sharded'] = ops.RangeCtx(f0['depth'].device)
        grids = ops.ranged(one_pass, ctx, agree=lambda ok: parallel.all_agree(ok, f0['depth'].device, group, gather_on_host))
    else:
        grids = one_pass()
    if timings is not None:
        torch.cuda.synchronize()
        for (_, a), (name, b) in zip(events[:-1], events[1:]):
            timings[name] = a.elapsed_time(b)
    return {'semantic_occ_%ds' % k: [g] for k, g in enumerate(grids)}


@torch.no_grad()
def evaluate_stream(net, samples, in_flight=2, use_image_mask=True, keep_stacks=False, fscore=None, distributed=False, group=None,
                    dump_dir=None, stats=None):
    """harness.evaluate through pipeline.SampleStream: `in_flight` captured samples on their own HIP streams, every replay
    range-checked, each sample scored on the device by one pw_occ_score launch inside its graph (no per-sample D2H copy).
    samples: a list or iterable of the same dicts as evaluate (the first one fixes the shapes the graphs are captured for).
    Returns what evaluate returns: (report, stacks or None, metric) -- stacks (the {0,2,4,6} stack per sample, numpy) only when
    keep_stacks=True, which turns the payload copy on.
    fscore: as for evaluate -- one more launch inside each sample's graph (pw_occ_fscore) and one fold per finished sample
    (pw_occ_fscore_accumulate); then report['fscore'] = {idx: tot_f1_mean / cnt} and metric.fscore = {idx: Metric_FScore}.
    dump_dir: the reference's --dump_dir (apis/test.py:225-232): each sample's stack is written to
    <dump_dir>/<scene_name>/<sample_idx>.npy as np.save(path, [stack]) -- a (1, 4, X, Y, Z) uint8 array -- with scene_name and
    sample_idx read from the sample dict (ValueError without them).  Turns the payload copy on.
    distributed=True: evaluate one split across the ranks of an initialised torch.distributed group (`group`, or the default
    group), one process per GPU; see _evaluate_stream_distributed.  Every rank returns the whole split's (report, None, metric).
    stats (dict): receives this process's 'samples', 'replays', 'recalibrations', 'recaptures' and the seconds of 'capture_s'
    (the slots' capture), 'stream_s' (first sample enqueued to the stream drained) and 'reduce_s' (drained to the final report)."""
    if distributed:
        return _evaluate_stream_distributed(net, samples, in_flight, use_image_mask, keep_stacks, fscore, group, dump_dir, stats)
    from .pipeline import SampleStream
    it = iter(samples)
    first = next(it, None)
    if first is None:
        raise ValueError('evaluate_stream: no samples')
    if dump_dir is not None:
        _dump_path(dump_dir, first)
    horizons = (0, 2, 4, 6)
    score = dict(horizons=horizons, n_cl=18, mask='camera' if use_image_mask else None)
    if fscore is not None:
        score['fscore'] = dict(fscore)
    t0 = time.perf_counter()
    stream = SampleStream(net, first['frames'], first['ego'], in_flight=in_flight, n_steps=6,
                          payload=keep_stacks or dump_dir is not None, score=score)
    t1 = time.perf_counter()
    stacks = [] if keep_stacks else None
    try:
        n = _drain(stream, _chain(first, it), False, horizons, stacks, dump_dir)
    finally:
        stream.close()
    t2 = time.perf_counter()
    report = stream.metric.report()
    if fscore is not None:
        stream.metric.fscore = stream.fscore
        report['fscore'] = {h: f.tot_f1_mean / f.cnt for h, f in stream.fscore.items()}
    if stats is not None:
        stats.update(samples=n, replays=stream.replays, recalibrations=stream.recalibrations, recaptures=stream.recaptures,
                     capture_s=t1 - t0, stream_s=t2 - t1, reduce_s=time.perf_counter() - t2)
    return report, stacks, stream.metric


def _dump_path(dump_dir, sample):
    """<dump_dir>/<scene_name>/<sample_idx>.npy (apis/test.py:226-232)"""
    if 'scene_name' not in sample or 'sample_idx' not in sample:
        raise ValueError('evaluate_stream: dump_dir needs scene_name and sample_idx in every sample')
    return os.path.join(dump_dir, str(sample['scene_name']), '%s.npy' % (sample['sample_idx'],))


def _drain(stream, items, indexed, horizons, stacks, dump_dir):
    """run the stream over `items` to the end; stacks (a list) receives every stack, dump_dir every file.  Returns the count."""
    paths = collections.deque()

    def feed():
        for item in items:
            if dump_dir is not None:
                paths.append(_dump_path(dump_dir, item[1] if indexed else item))
            yield item
    n = 0
    for res in stream.run(feed(), indexed=indexed):
        n += 1
        if stacks is not None or dump_dir is not None:
            st = np.stack([res['semantic_occ_%ds' % h][0] for h in horizons], axis=0)
            if stacks is not None:
                stacks.append(st)
            if dump_dir is not None:
                path = paths.popleft()
                os.makedirs(os.path.dirname(path), exist_ok=True)
                np.save(path, [st])
    torch.cuda.current_stream().synchronize()
    return n


def _is_sequence(samples):
    return hasattr(samples, '__len__') and hasattr(samples, '__getitem__') and not isinstance(samples, collections.abc.Mapping)


def _evaluate_stream_distributed(net, samples, in_flight, use_image_mask, keep_stacks, fscore, group, dump_dir, stats):
    """evaluate_stream(distributed=True): what tools/dist_test_temporal.sh -> multi_gpu_test_temporal -> dataset.evaluate does
    (apis/test.py:198-256, nuscenes_dataset_occ_trajectory.py:478-526), without moving a prediction between processes.

    * Rank r of W evaluates the global samples i with i % W == r (parallel.eval_shard: DistributedSampler(shuffle=False) without
      its padding).  samples: a sequence (len + indexing; a rank reads its own items and item 0 only) or an iterable (every rank
      walks ALL of it and skips the other ranks' items: its items should be cheap handles, e.g. loading their tensors lazily).
    * Every rank captures its slots on global sample 0, so sample i replays under the activation ranges the single-process stream
      uses; a range miss still recalibrates that rank's slot locally.  A rank with no sample (W > N) captures nothing.
    * Once the rank's stream has drained: parallel.all_agree on "finished without error" (any failure -> PreworldHipError on
      EVERY rank, chained to the local error where there is one), then parallel.reduce_eval_counts: SUM of every horizon's
      confusion matrix and binary histogram and the counts.  With fscore, sample i's (H, 4) counts were written to row i of an
      (n, H, 4) int64 table during the stream (nothing folded); N, the split's size, is a MAX all-reduce of the rows each rank
      has seen (len(samples), or the items walked), the tables are SUM-reduced and ONE pw_occ_fscore_accumulate folds all N
      rows in index order -- the single-process stream's input order, so the float64 totals and n_empty_gt are identical.
      The same collectives run on every rank whatever its sample count.  RCCL ('nccl') reduces device tensors; any other
      backend (gloo) gets them through host memory.
    keep_stacks raises ValueError (predictions stay where they were made: use dump_dir, each rank writes its own samples)."""
    import torch.distributed as dist
    from . import ops, parallel
    from .pipeline import SampleStream
    if keep_stacks:
        raise ValueError('evaluate_stream(distributed=True): predictions stay on the rank that made them -- use dump_dir')
    if not (dist.is_available() and dist.is_initialized()):
        raise ValueError('evaluate_stream(distributed=True) needs an initialised torch.distributed process group')
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    via_host = dist.get_backend(group) != 'nccl'
    seen = [0]
    if _is_sequence(samples):
        seen[0] = len(samples)
        if not seen[0]:
            raise ValueError('evaluate_stream: no samples')
        first = samples[0]
        own = ((i, samples[i]) for i in parallel.eval_shard(seen[0], rank, world))
    else:
        it = iter(samples)
        first = next(it, None)
        if first is None:
            raise ValueError('evaluate_stream: no samples')

        def walk():
            seen[0] = 1
            if rank == 0:
                yield 0, first
            for i, s in enumerate(it, 1):
                seen[0] = i + 1
                if i % world == rank:
                    yield i, s
        own = walk()
    if dump_dir is not None:
        _dump_path(dump_dir, first)
    horizons = (0, 2, 4, 6)
    dev = first['ego'].device
    score = dict(horizons=horizons, n_cl=18, mask='camera' if use_image_mask else None)
    if fscore is not None:
        score['fscore'] = dict(fscore)
    stream, err, n = None, None, 0
    t0 = t1 = time.perf_counter()
    try:
        head = next(own, None)
        if head is not None:
            stream = SampleStream(net, first['frames'], first['ego'], in_flight=in_flight, n_steps=6,
                                  payload=dump_dir is not None, score=score)
            t1 = time.perf_counter()
            n = _drain(stream, _chain(head, own), True, horizons, None, dump_dir)
    except Exception as e:                  # every rank must still reach the agreement below
        err = e
    t2 = time.perf_counter()
    try:
        if not parallel.all_agree(err is None, dev, group, via_host):
            raise ops._lib.PreworldHipError('evaluate_stream(distributed=True): rank %d of %d: %s' % (
                rank, world, 'failed: %r' % (err,) if err is not None else 'another rank failed')) from err
        if stream is not None:
            metric, fs, totals, empty, rows = stream.metric, stream.fscore, stream.fs_totals, stream.fs_empty, stream.fs_rows
        else:
            metric = metrics.Metric_mIoU_Temporal(num_classes=18, use_image_mask=use_image_mask, device=dev)
            fs = totals = empty = rows = None
            if fscore is not None:
                kw = dict(fscore)
                fmask = kw.pop('mask', None)
                group_fs, totals, empty = metrics.Metric_FScore._group(
                    len(horizons), use_image_mask=fmask == 'camera', use_lidar_mask=fmask == 'lidar', device=dev, **kw)
                fs = dict(zip(horizons, group_fs))
        if fs is not None and rows is None:
            rows = torch.zeros((0, len(horizons), 4), dtype=torch.int64, device=dev)
        mine = [n] + ([stream.replays, stream.recalibrations, stream.recaptures] if stream is not None else [0, 0, 0])
        summed, rows = parallel.reduce_eval_counts(metric, rows if fs is not None else None, seen[0], mine, group, via_host)
        N = seen[0] if rows is None else rows.shape[0]
        if summed[0] != N or metric.cnt != N:
            raise ops._lib.PreworldHipError('evaluate_stream(distributed=True): %d samples scored across the ranks for a split of %d'
                                            % (summed[0], N))
        report = metric.report()
        if fs is not None:
            ops.occ_fscore_accumulate(rows, totals, empty)         # all N rows in index order: the single-process fold
            for m in fs.values():
                m.cnt = N
            metric.fscore = fs
            report['fscore'] = {h: f.tot_f1_mean / f.cnt for h, f in fs.items()}
    finally:
        if stream is not None:
            stream.close()
    if stats is not None:
        stats.update(world=world, rank=rank, n_samples=N, samples=n, replays=mine[1], recalibrations=mine[2], recaptures=mine[3],
                     all=dict(replays=summed[1], recalibrations=summed[2], recaptures=summed[3]),
                     capture_s=t1 - t0, stream_s=t2 - t1, reduce_s=time.perf_counter() - t2)
    return report, None, metric


def _chain(first, rest):
    yield first
    yield from rest
