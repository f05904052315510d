"""Serving-side composition of the hot path: synthetic or real lifted inputs in HBM -> LSS voxel
pooling -> voxel encoder -> forecast decode -> occupancy heads, mirroring the call order of
PreWorld4DTraj.simple_test (mmdet3d/models/detectors/preworld_temporal_traj.py:212-370).

`CapturedSample` records one sample's ~60 kernel launches into a hipGraph (torch.cuda.CUDAGraph) over
static input/output buffers: a replay has no launch gaps (kernel time == wall time in
profiles/r01_bench_kernel_stats_v5.md) and no per-launch host work, which is what the C3 step needs
once the kernels themselves run in 10-1000 us."""
import collections

import numpy as np
import torch

from . import ops


def clone_frame(f):
    """static copy of one frame's inputs.  depthnet_tail hands the context over channels-last and says so through an attribute of the
    tensor object (modules.LSSViewTransformer.depthnet_tail): a clone must keep it, or the lift reads the buffer channel-first"""
    out = {}
    for k, v in f.items():
        out[k] = v.clone()
        if getattr(v, '_pw_channels_last', False):
            out[k]._pw_channels_last = True
    return out


def to_dev(a, dev='cuda:0'):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class CapturedSample:
    """net: modules.PreWorld4DTraj (eval).  frames / ego: example inputs defining the shapes (list of
    dicts as for simple_test_from_lift, (B,1,21) ego states).  run(frames, ego) copies new inputs into
    the static buffers, replays the graph and returns the (static) result dict: consume or clone the
    outputs before the next run()."""

    fused_input_copy = True          # run(): one pw_copy_many launch for the inputs (False: one torch copy per tensor; A/B)

    def __init__(self, net, frames, ego, n_steps=6, d2h=False):
        """d2h=True: the replay also delivers the reference's host payload (preworld_temporal_traj.py:311-366: every
        semantic_occ / geo_occ grid as a contiguous uint8 (X,Y,Z) host array) -- one device-side gather of the (X,Y,Z)
        views into a (n_grids, X, Y, Z) buffer and ONE async copy into pinned host memory (`self.host`, rows in the
        order of `self.host_keys`) instead of the reference's 14 synchronous .cpu() calls per sample."""
        self.net, self.n_steps, self.d2h = net, n_steps, d2h
        self.host = self.host_keys = None
        self.frames = [clone_frame(f) for f in frames]
        self.ego = ego.clone()
        # Activation ranges of the split-fp16 path (ops.RangeCtx): this sample's own table of per-tensor exponents.  The
        # warm-up calibrates it (repeats the pass until every h2 tensor's maximum sits in the window); the captured kernels
        # read the exponents from the table, clear and re-record the maxima on every replay, and the table travels to pinned
        # host memory with the results: ranges_ok() is the per-replay check, recalibrate() the (rare) repair.
        self.rctx = ops.RangeCtx(self.ego.device)
        self.host_rng = torch.zeros(tuple(self.rctx.compact.shape), dtype=torch.int32, pin_memory=True)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():        # warm-up off the capture stream: fills the packed-weight
            ops.ranged(self._step, self.rctx)                  # caches, sets the kernels' LDS attributes, calibrates the ranges
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        # thread_local: a HIP call from another thread of the process (the RCCL watchdog of a multi-GPU run polls
        # events) must not invalidate this thread's capture
        with torch.cuda.graph(self.graph, capture_error_mode='thread_local'), torch.no_grad(), ops.use_range(self.rctx):
            self.rctx.begin()
            self.out = self._step()
            self.rctx.fold()
            self.rctx.audit()                                   # sticky device counters: EVERY replay is range-checked (bad_replays())
            self.host_rng.copy_(self.rctx.compact, non_blocking=True)

    def _step(self):
        kw = dict(n_steps=self.n_steps) if hasattr(self.net, 'forecast_cl') else {}
        args = (self.frames, self.ego) if hasattr(self.net, 'forecast_cl') else (self.frames,)
        out = self.net.simple_test_from_lift(*args, **kw)
        if self.d2h:
            keys = [k for k in out if k.startswith(('semantic_occ', 'geo_occ'))]
            g = out.get('grids')
            if g is not None and g.numel() == len(keys) * out[keys[0]][0].numel() and all(
                    out[k][0].data_ptr() == g.data_ptr() + i * out[k][0].numel() for i, k in enumerate(keys)):
                dev = g.view((len(keys),) + tuple(out[keys[0]][0].shape))  # the kernels wrote the payload rows in place
            else:
                dev = torch.stack([out[k][0] for k in keys])              # (n_grids, X, Y, Z) contiguous uint8
            if self.host is None:
                self.host = torch.empty(dev.shape, dtype=torch.uint8, pin_memory=True)
                self.host_keys = keys
            self.host.copy_(dev, non_blocking=True)
        return out

    def replay(self):
        self.graph.replay()
        return self.out

    def eager(self):
        """the same pass as a replay -- same static buffers, same exponent table, same slot order -- launched eagerly on the
        current stream: results are bit-identical to replay() (all kernels are deterministic)"""
        with torch.no_grad(), ops.use_range(self.rctx):
            self.rctx.begin()
            out = self._step()
            self.rctx.fold()
            return out

    def ranges_ok(self):
        """after the replay has completed (stream / device synchronised): did every h2 tensor of it stay inside the
        representable window under the exponents it ran with?  False -> recalibrate() and replay that sample again."""
        return not self.rctx.check(self.host_rng)

    def bad_replays(self):
        """(replays that left their calibrated activation ranges, replays audited) since capture (synchronises): the device-side
        tally of pw_rng_audit, which every replay feeds -- unlike ranges_ok(), which only sees the LAST replay's table"""
        torch.cuda.synchronize()
        return self.rctx.audited()

    def recalibrate(self):
        """re-derive the exponents from the inputs currently in the static buffers (eager passes; the graph keeps reading
        the same table).  Waits for everything in flight first: a replay must not see the table change under it."""
        torch.cuda.synchronize()
        with torch.no_grad():
            ops.ranged(self._step, self.rctx)
        torch.cuda.synchronize()

    def run_checked(self, frames, ego):
        """run() + wait + range check, repaired and replayed once if the sample left the calibrated window"""
        out = self.run(frames, ego)
        torch.cuda.current_stream().synchronize()
        if not self.ranges_ok():
            self.recalibrate()
            out = self.replay()
            torch.cuda.current_stream().synchronize()
            if not self.ranges_ok():
                raise ops._lib.PreworldHipError('activation ranges still outside the window after recalibration: slots %s'
                                                % self.rctx.check(self.host_rng))
        return out

    def run(self, frames, ego):
        dsts, srcs = [self.ego], [ego]
        for dst, src in zip(self.frames, frames):
            for k, v in src.items():
                dsts.append(dst[k])
                srcs.append(v)
        if self.fused_input_copy and all(s.is_cuda and s.is_contiguous() and s.dtype == d.dtype and s.shape == d.shape for d, s in zip(dsts, srcs)):
            ops.copy_many(dsts, srcs)                      # one launch for the ~15 input tensors
        else:
            for d, s in zip(dsts, srcs):
                d.copy_(s, non_blocking=True)
        return self.replay()


class ShardedSample:
    """BASELINE.json configs[3] -- ONE sample across the ranks of a node (frames lifted on different ranks, RCCL exchange of the
    per-frame voxel features before the encoder, states forecast + decoded round-robin, all_gather of the uint8 grids; the reference's
    join point is bevdet_occ.py:266-267, its result gather apis/test.py:198-223) -- as three captured compute phases between the two
    collectives (round 6; harness.simple_test_sharded is the eager form: ~60 launches + a calibration all-reduce and a host sync per
    call):
        graph A   this rank's frames: LSS lift + pooling + pre_process -> fp32 features in static buffers   (nothing on other ranks)
        exchange  parallel.exchange_frames: all_gather_into_tensor (full rounds) / broadcasts from the owners (partial round)
        graph B   cat [adjacent ..., key] -> one h2 split -> CustomResNet3D -> LSSFPN3D -> final_conv
        graph C   ONE pass of the forecast recursion up to this rank's largest owned state, OccHead on its owned states -> uint8 slots
        gather    parallel.gather_states: one all_gather of the 0.64 MB slots
    Activation ranges: calibrated ONCE at construction (ops.ranged over eager passes; the ranks agree through a MIN all-reduce per
    calibration pass, as the passes contain collectives), then every replay re-records its maxima and the device-side audit tallies
    the replays that left the window (bad_replays(), like CapturedSample) -- no host sync and no collective for the ranges per sample.
    run(frames, ego) copies a sample's inputs (every rank holds all of them) into the static buffers and returns the reference's
    result dict; timings (dict) receives the phases' milliseconds from HIP events and the payload bytes."""

    def __init__(self, net, frames, ego, n_steps=6, group=None, gather_on_host=False):
        import torch.distributed as dist
        from . import parallel
        from .modules import as_f32, precision
        self.net, self.n_steps, self.group, self.via_host = net, n_steps, group, gather_on_host
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.collective = self.world > 1 or parallel.ALWAYS_COLLECTIVE
        vt = net.img_view_transformer
        _, _, size = vt._grid()
        self.size = [int(v) for v in size]
        n = net.num_adj + 1
        self.frames = [clone_frame(f) for f in (frames[:n] if net.with_prev else frames[:1])]
        self.ego = ego.clone()
        self.dev = self.ego.device
        self.F = len(self.frames)
        f0 = self.frames[0]
        self.B, self.C, self.n = f0['sensor2keyego'].shape[0], vt.out_channels, n
        self.h2 = precision() == 'h2' and self.C % 32 == 0
        self.n_states = n_steps + 1
        self.mine_f = list(range(self.rank, self.F, self.world))
        self.mine_s = parallel.owned_states(self.n_states, self.rank, self.world)
        self.shape = (self.B, self.size[2], self.size[1], self.size[0], self.C)
        self._as_f32, self._par = as_f32, parallel
        self.static = {}                                        # receive buffers of the frame exchange (fixed addresses)
        self.rctx = ops.RangeCtx(self.dev)
        self.host_rng = torch.zeros(tuple(self.rctx.compact.shape), dtype=torch.int32, pin_memory=True)
        slots = (self.n_states + self.world - 1) // self.world
        gdev = 'cpu' if gather_on_host else self.dev
        self.send = torch.zeros((slots, self.size[0], self.size[1], self.size[2]), dtype=torch.uint8, device=self.dev)
        self.send_x = self.send if not gather_on_host else torch.zeros(self.send.shape, dtype=torch.uint8, pin_memory=True)
        self.recv = [torch.empty(self.send.shape, dtype=torch.uint8, device=gdev) for _ in range(self.world)]
        self.lifted, self.v0, self.all_frames = {}, None, None
        # calibration: eager passes with the collectives inside, all ranks agree on whether another pass runs
        with torch.no_grad():
            ops.ranged(self._eager_pass, self.rctx,
                       agree=lambda ok: parallel.all_agree(ok, self.dev, group, gather_on_host))
        torch.cuda.synchronize()
        # capture: the same pass cut at the collectives; slots are handed out in call order, so A -> B -> C under ONE begin()
        self.gA, self.gB, self.gC = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        kw = dict(capture_error_mode='thread_local')
        with torch.no_grad(), ops.use_range(self.rctx):
            with torch.cuda.graph(self.gA, **kw):
                self.rctx.begin()
                self._phase_lift()
            pool = self.gA.pool()
            self.all_frames = self._exchange()                  # eager, now: graph B is captured on the buffers it delivers into
            with torch.cuda.graph(self.gB, pool=pool, **kw):
                self._phase_encoder()
            with torch.cuda.graph(self.gC, pool=pool, **kw):
                self._phase_decode()
                self.rctx.fold()
                self.rctx.audit()
                self.host_rng.copy_(self.rctx.compact, non_blocking=True)
        torch.cuda.synchronize()

    # ---- the three compute phases (shared by the eager calibration pass and the captures)
    def _phase_lift(self):
        for f in self.mine_f:
            # fp32 values travel: an h2 buffer means nothing without its rank-local exponent ((hi + lo) * 2^e is exact)
            self.lifted[f] = self._as_f32(self.net.lift_frame_cl(out_h2=self.h2, **self.frames[f])).contiguous()

    def _exchange(self, stats=None):
        if not self.collective:
            return [self.lifted[f] for f in range(self.F)]
        return self._par.exchange_frames(self.lifted, self.F, self.shape, torch.float32, self.dev, self.group, self.via_host, stats,
                                         static=self.static)

    def _phase_encoder(self):
        lifted, C, n = self.all_frames, self.C, self.n
        net, h2 = self.net, self.h2
        # [adjacent ..., key] (bevdet_occ.py:266): every frame goes straight into its channel slice of ONE buffer -- on the split-fp16
        # path as ONE h2 tensor under ONE range slot of this pass's table (the same data, hence the same exponent, on every rank)
        x = torch.empty(self.shape[:-1] + (n * C,), device=self.dev, dtype=torch.float32)
        slot = ops.new_slot(self.dev) if h2 else None
        for j in range(n):                                                      # frame j sits at channel block n - 1 - j
            lo, hi = (n - 1 - j) * C, (n - j) * C
            if j < len(lifted):
                if h2:
                    ops.f32_to_h2(lifted[j], out=ops.H2(x[..., lo:hi], slot))
                else:
                    x[..., lo:hi].copy_(lifted[j])
            else:
                x[..., lo:hi].zero_()                                           # with_prev=False: zeros (bevdet_occ.py:243-258)
        self.v0 = net.final_conv.forward_cl(net.bev_encoder_cl(ops.H2(x, slot) if h2 else x, out_h2=h2), out_h2=h2)

    def _phase_decode(self):
        net = self.net
        if not self.mine_s:
            return
        kmax = max(self.mine_s)
        states = net.forecast_cl(self.v0, self.ego, kmax, out_h2=self.h2)[0] if kmax > 0 else None
        inplace = self.h2 and self.B == 1       # the kernel writes a (Z,Y,X) result as the (X,Y,Z)-contiguous payload grid, in place
        i = 0
        while i < len(self.mine_s):
            k = self.mine_s[i]
            run = 1                              # consecutive owned forecast states decode in ONE launch (world 1: states 1 .. 6)
            while k > 0 and i + run < len(self.mine_s) and self.mine_s[i + run] == k + run:
                run += 1
            if k == 0:
                feats = self.v0
            elif run == 1:
                feats = states[k - 1]
            else:
                feats = states.view((states.shape[0] * self.B,) + tuple(self.v0.shape[1:]))[(k - 1) * self.B:(k - 1 + run) * self.B]
            dst = self.send[i:i + run]
            if inplace:
                net.occupancy_head.decode_cl(feats, transposed=True, occ_out=dst.permute(0, 3, 2, 1))
            else:
                occ = net.occupancy_head.decode_cl(feats, transposed=True)
                dst.copy_(occ.permute(0, 3, 2, 1).reshape(run, self.B, *dst.shape[1:])[:, 0])      # batch element 0 (:306)
            i += run

    def _gather(self, stats=None):
        if not self.collective:
            return [self.send[i] for i in range(self.n_states)]
        if self.via_host:
            self.send_x.copy_(self.send, non_blocking=True)
            torch.cuda.current_stream().synchronize()
        return self._par.gather_states(None, self.n_states, self.group, stats=stats, send=self.send_x, recv=self.recv)

    def _eager_pass(self):
        self._phase_lift()
        self.all_frames = self._exchange()
        self._phase_encoder()
        self._phase_decode()
        return self._gather()

    def run(self, frames=None, ego=None, timings=None):
        """one sample: optional new inputs into the static buffers, A -> exchange -> B -> C -> gather.  Returns
        {'semantic_occ_%ds': [(X,Y,Z) uint8]} (static buffers: consume before the next run)."""
        if frames is not None:
            dsts, srcs = [self.ego], [ego]
            for dst, src in zip(self.frames, frames):
                for k, v in src.items():
                    dsts.append(dst[k])
                    srcs.append(v)
            ops.copy_many(dsts, srcs)
        ev = []

        def mark(name):
            if timings is not None:
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                ev.append((name, e))
        mark('start')
        self.gA.replay()
        mark('lift')
        got = self._exchange(timings)
        assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got, self.all_frames)), 'frame exchange left its static buffers'
        mark('gather_frames')
        self.gB.replay()
        mark('encoder')
        self.gC.replay()
        mark('decode')
        grids = self._gather(timings)
        mark('gather_states')
        if timings is not None:
            torch.cuda.synchronize()
            for (_, a), (name, b) in zip(ev[:-1], ev[1:]):
                timings[name] = a.elapsed_time(b)
        return {'semantic_occ_%ds' % k: [g] for k, g in enumerate(grids)}

    def bad_replays(self):
        """(passes that left their calibrated activation ranges, passes audited) since capture (synchronises)"""
        torch.cuda.synchronize()
        return self.rctx.audited()


# ---------------------------------------------------------------------------------------------------------------------------------
# Streaming evaluation: M captured samples in flight, every replay range-checked, scored on the device, results in input order.
# ---------------------------------------------------------------------------------------------------------------------------------

class StreamScheduler:
    """The ordering / lag / repair / count logic of SampleStream over a list of slots (any objects with the methods below), so
    that it can be pinned without a GPU.  Sample i goes to slot i % M; before a slot takes a new sample the host waits for THAT
    slot's previous sample only, checks its ranges, repairs it if needed, commits its scores, enqueues the new sample and only
    then hands the finished result out -- so results come out in input order, M - 1 samples behind the enqueue.

    slot.stage(sample)   host-side preparation that does not touch the slot's device buffers (e.g. pinned staging of host GT)
    slot.load(sample)    enqueue the copies of the sample's inputs into the slot's static buffers
    slot.launch(buf)     enqueue one replay over the static buffers (+ the payload copy into host buffer `buf` of 2)
    slot.wait()          host waits for the slot's last launch
    slot.ranges_ok()     did the last replay stay inside its calibrated activation ranges?
    slot.recalibrate()   re-derive the ranges from the inputs in the static buffers
    slot.commit()        add the last replay's per-sample score table to the running totals
    slot.commit(index)   (run(..., indexed=True) only) the same for global sample `index` (deferred F-score rows)
    slot.result(buf)     what run() yields for the sample (valid at least until the next next())"""

    def __init__(self, slots):
        self.slots = list(slots)
        self.replays = 0
        self.recalibrations = 0

    def run(self, samples, indexed=False):
        """indexed=True: the items are (global index, sample) pairs and a finished sample is committed with commit(index)"""
        M = len(self.slots)
        pending = collections.deque()               # (slot, payload buffer, sample, index): the sample stays referenced until finished
        parity = [0] * M
        for i, item in enumerate(samples):
            index, sample = item if indexed else (None, item)
            s = i % M
            slot = self.slots[s]
            slot.stage(sample)
            done = self._finish(*pending.popleft()) if len(pending) == M else None      # the oldest in flight sits in slot s
            slot.load(sample)
            slot.launch(parity[s])
            self.replays += 1
            pending.append((slot, parity[s], sample, index))
            parity[s] ^= 1
            if done is not None:
                yield done
        while pending:
            yield self._finish(*pending.popleft())

    def _finish(self, slot, buf, sample, index=None):
        slot.wait()
        if not slot.ranges_ok():
            # a replay outside its window is never counted: repair, replay the same static inputs, check again (run_checked)
            self.recalibrations += 1
            slot.recalibrate()
            slot.launch(buf)
            self.replays += 1
            slot.wait()
            if not slot.ranges_ok():
                raise ops._lib.PreworldHipError('activation ranges still outside the window after recalibration')
        if index is None:
            slot.commit()
        else:
            slot.commit(index)
        return slot.result(buf)


class _ScoredCapture(CapturedSample):
    """CapturedSample whose graph also scores the sample: static GT / mask buffers (one row per scored horizon) and one
    pw_occ_score launch that zeroes, then fills the slot's per-sample table.  payload: the device rows of the host payload
    (the OccHead's in-place `grids` rows when the layout allows, else a gather inside the graph), copied out by the stream.
    fscore: None, or dict(kernel=ops.occ_fscore keyword arguments, own_mask=bool): one more pw_occ_fscore launch into
    `fs_table` over the same GT buffers -- and the mIoU mask buffers, or (own_mask) static mask buffers of its own."""

    def __init__(self, net, frames, ego, n_steps, pred_keys=None, n_cl=18, masked=False, payload=False, fscore=None):
        self.pred_keys, self.n_cl, self.masked, self.want_payload = pred_keys, n_cl, masked, payload
        self.fscore = fscore
        self.gt = self.mask = self.table = None
        self.fs_table = self.fs_mask = None
        self.payload_dev = self.payload_keys = None
        super().__init__(net, frames, ego, n_steps=n_steps, d2h=False)

    def _step(self):
        out = super()._step()
        capturing = torch.cuda.is_current_stream_capturing()
        if self.want_payload and capturing:
            keys = [k for k in out if k.startswith(('semantic_occ', 'geo_occ'))]
            g = out.get('grids')
            if g is not None and g.numel() == len(keys) * out[keys[0]][0].numel() and all(
                    out[k][0].data_ptr() == g.data_ptr() + i * out[k][0].numel() for i, k in enumerate(keys)):
                self.payload_dev = g.view((len(keys),) + tuple(out[keys[0]][0].shape))
            else:
                self.payload_dev = torch.stack([out[k][0] for k in keys])
            self.payload_keys = keys
        if self.pred_keys:
            preds = [out[k][0] if out[k][0].is_contiguous() else out[k][0].contiguous() for k in self.pred_keys]
            if self.gt is None:                       # first (eager, uncaptured) pass: the static buffers take the grid shape
                H, shape, dev = len(preds), tuple(preds[0].shape), preds[0].device
                self.gt = torch.zeros((H,) + shape, dtype=torch.uint8, device=dev)
                self.mask = torch.ones((H,) + shape, dtype=torch.uint8, device=dev) if self.masked else None
                self.table = torch.zeros((H, ops.occ_score_bins(self.n_cl)), dtype=torch.int64, device=dev)
                if self.fscore is not None:
                    self.fs_table = torch.zeros((H, 4), dtype=torch.int64, device=dev)
                    if self.fscore['own_mask']:
                        self.fs_mask = torch.ones((H,) + shape, dtype=torch.uint8, device=dev)
            self.table.zero_()
            ops.occ_score(preds, list(self.gt), list(self.mask) if self.mask is not None else None, self.n_cl, self.table)
            if self.fscore is not None:
                fm = self.fs_mask if self.fscore['own_mask'] else (self.mask if self.fscore['mask_key'] is not None else None)
                self.fs_table.zero_()
                ops.occ_fscore(preds, list(self.gt), list(fm) if fm is not None else None, self.fs_table, **self.fscore['kernel'])
        return out


def _grid_per_horizon(v, horizons):
    """a sample's gt / mask entry: {h: grid} or one grid for every horizon"""
    return [v[h] for h in horizons] if isinstance(v, dict) else [v] * len(horizons)


class _StreamSlot:
    """one slot of SampleStream: a _ScoredCapture on its own HIP stream, pinned staging for host GT, two pinned payload buffers"""

    def __init__(self, owner, cap):
        self.owner, self.cap = owner, cap
        self.stream = torch.cuda.Stream(device=cap.ego.device)
        self.done = torch.cuda.Event()
        self.staged = torch.cuda.Event()              # the H2D copies out of the staging buffers have been enqueued before this
        self.host = self.views = None
        if cap.payload_dev is not None:
            self.host = [torch.empty(tuple(cap.payload_dev.shape), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
            self.views = [{k: [h[i].numpy()] for i, k in enumerate(cap.payload_keys)} for h in self.host]
        self.staging = {}                             # kind -> pinned (H, X, Y, Z) staging of host grids
        self._host_rows = ()

    def _static(self, kind):
        return {'gt': self.cap.gt, 'mask': self.cap.mask, 'fs_mask': self.cap.fs_mask}[kind]

    def _grids(self, sample):
        """(kind, row, array) of the sample's GT (and masks) per scored horizon"""
        hz = self.owner.horizons
        out = [('gt', j, a) for j, a in enumerate(_grid_per_horizon(sample['gt'], hz))]
        for kind, key in (('mask', self.owner.mask_key), ('fs_mask', self.owner.fs_mask_key)):
            if self._static(kind) is not None:
                m = sample.get(key)
                if m is None:                         # no mask with this sample: every voxel counts (as add_batch with None)
                    m = np.ones(tuple(self.cap.gt.shape[1:]), dtype=np.uint8)
                out += [(kind, j, a) for j, a in enumerate(_grid_per_horizon(m, hz))]
        return out

    def stage(self, sample):
        """host GT / masks -> this slot's pinned staging, once the previous sample's H2D copies out of it have completed"""
        rows = []
        if self.cap.table is not None:
            for kind, j, a in self._grids(sample):
                if isinstance(a, torch.Tensor) and a.is_cuda:
                    continue
                if not rows:
                    self.staged.synchronize()
                if kind not in self.staging:
                    self.staging[kind] = torch.empty(tuple(self.cap.gt.shape), dtype=torch.uint8, pin_memory=True)
                dst = self.staging[kind][j]
                np.copyto(dst.numpy(), np.asarray(a).reshape(tuple(dst.shape)), casting='unsafe')
                rows.append((kind, j))
        self._host_rows = tuple(rows)

    def load(self, sample):
        cap, st = self.cap, self.stream
        st.wait_stream(torch.cuda.current_stream())   # the sample's device tensors were made on the caller's stream
        dsts, srcs = ([cap.ego], [sample['ego']]) if self.owner.temporal else ([], [])
        for dst, src in zip(cap.frames, sample['frames']):
            for k, v in src.items():
                dsts.append(dst[k])
                srcs.append(v)
        if cap.table is not None:
            for kind, j, a in self._grids(sample):
                if isinstance(a, torch.Tensor) and a.is_cuda:
                    dsts.append(self._static(kind)[j])
                    srcs.append(a.view(torch.uint8) if a.dtype == torch.bool else a)
        with torch.cuda.stream(st):
            # CapturedSample.run's guard: one pw_copy_many launch when every source qualifies, else one copy per tensor
            if cap.fused_input_copy and all(s_.is_cuda and s_.is_contiguous() and s_.dtype == d.dtype and s_.shape == d.shape
                                            for d, s_ in zip(dsts, srcs)):
                ops.copy_many(dsts, srcs)
            else:
                for d, s_ in zip(dsts, srcs):
                    d.copy_(s_, non_blocking=True)
            for kind, j in self._host_rows:
                self._static(kind)[j].copy_(self.staging[kind][j], non_blocking=True)
            if self._host_rows:
                self.staged.record(st)
        self._host_rows = ()

    def launch(self, buf):
        with torch.cuda.stream(self.stream):
            self.cap.replay()
            if self.host is not None:
                self.host[buf].copy_(self.cap.payload_dev, non_blocking=True)
            self.done.record(self.stream)

    def wait(self):
        self.done.synchronize()

    def ranges_ok(self):
        return self.cap.ranges_ok()

    def recalibrate(self):
        self.cap.recalibrate()

    def commit(self, index=None):
        if self.cap.table is None:
            return
        ms = self.owner.metric_stream
        with torch.cuda.stream(ms):
            if self.owner.temporal:
                self.owner.metric.add_counts(self.cap.table, 1, horizons=self.owner.horizons)
            else:
                self.owner.metric.add_counts(self.cap.table, 1)
            if self.cap.fs_table is not None and index is not None:
                self.owner._fs_row(index).copy_(self.cap.fs_table)       # deferred: folded later, in index order
            elif self.cap.fs_table is not None:       # every horizon's F-score totals: one pw_occ_fscore_accumulate launch
                ops.occ_fscore_accumulate(self.cap.fs_table, self.owner.fs_totals, self.owner.fs_empty)
                for m in self.owner.fscore.values():
                    m.cnt += 1
        self.stream.wait_stream(ms)                   # the next replay re-zeroes the tables: after the adds

    def result(self, buf):
        return dict(self.views[buf]) if self.views is not None else {}


class SampleStream:
    """Streaming inference + evaluation through the captured hot path: `in_flight` slots, each a hipGraph of one sample
    (CapturedSample over static buffers) on its own HIP stream.  run(samples) yields one result per sample, in input order:

    * payload=True: {'semantic_occ_{k}s' / 'geo_occ_{k}s' (PreWorld: 'semantic_occ' / 'geo_occ'): [numpy uint8 (X,Y,Z)]} -- views
      of pinned buffers, valid until the next next() (copy what you keep); payload=False: {} (no device-to-host copy at all);
    * score=dict(horizons=(0, 2, 4, 6), n_cl=18, mask='camera' | 'lidar' | None[, metric=...]): the graph also holds static GT /
      mask buffers and one pw_occ_score launch, and every finished sample's table is added to `self.metric` on the device
      (Metric_mIoU_Temporal for PreWorld4DTraj, Metric_mIoU with horizons (0,) for PreWorld) -- no per-sample result comes back to
      the host.  Samples then carry gt={h: (X,Y,Z) uint8} (or one grid) and mask_camera / mask_lidar (one grid or {h: grid}), numpy
      (through pinned staging) or device tensors.
      score['fscore'] = dict(threshold_acc=0.6, threshold_complete=0.6, voxel_size=[0.4, 0.4, 0.4], range=..., void=[17, 255],
      mask=None | 'camera' | 'lidar') (opt-in): one more launch in the graph, pw_occ_fscore over the same static GT buffers (and
      the mIoU mask buffers when the masks agree; another mask gets static buffers of its own, filled from the samples' entry), and
      every finished sample's counts are folded into `self.fscore` = {horizon: metrics.Metric_FScore} on the device.

    run(pairs, indexed=True) takes (global index, sample) pairs (a shard of a larger split, harness.evaluate_stream(distributed=True)):
    the mIoU tables are added as above, but the F-score counts are NOT folded -- sample i's (H, 4) row is copied into row i of
    `self.fs_rows`, an (n, H, 4) int64 device table that grows (zero-filled) as indices arrive, for the caller to fold in index order
    once every shard's rows are in it (ops.occ_fscore_accumulate).

    Every replay is range-checked before it counts (a miss: recalibrate, replay the same inputs, check again; still outside the
    window -> PreworldHipError).  Counters: `replays`, `recalibrations`, `recaptures`.
    Stale captures: a fingerprint -- precision() and modules.tensor_key of every parameter and buffer -- is taken at capture and
    compared at the start of every run(); a change (load_state_dict, an in-place update) re-captures.  In-place writes through
    `.data` bypass the version counter and are NOT seen: call recapture() after them.
    close() frees the graphs and static buffers (about 1.5 GB per full-size C3 slot)."""

    def __init__(self, net, example_frames, example_ego=None, in_flight=2, n_steps=6, payload=True, score=None):
        from . import metrics
        self.net, self.in_flight, self.payload = net, max(1, int(in_flight)), payload
        self.temporal = hasattr(net, 'forecast_cl')
        self.n_steps = n_steps if self.temporal else 0
        self.example = (example_frames, example_ego if self.temporal else example_frames[0]['bda'].new_zeros(1))
        if self.temporal and example_ego is None:
            raise ValueError('SampleStream: PreWorld4DTraj needs example ego states (B,1,21)')
        self.score = dict(score) if score is not None else None
        self.metric = None
        self.fscore = self.fs_totals = self.fs_empty = self.fs_rows = None
        self.horizons, self.mask_key, self.pred_keys, self.fs_mask_key = (), None, None, None
        self._fs_cap = None
        if self.score is not None:
            self.horizons = tuple(self.score.get('horizons', (0, 2, 4, 6) if self.temporal else (0,)))
            n_cl = self.score.setdefault('n_cl', 18)
            mask = self.score.get('mask', 'camera')
            self.mask_key = {'camera': 'mask_camera', 'lidar': 'mask_lidar', None: None}[mask]
            if self.temporal:
                self.pred_keys = ['semantic_occ_%ds' % h for h in self.horizons]
                if any(h > self.n_steps for h in self.horizons):
                    raise ValueError('SampleStream: horizons %s beyond n_steps %d' % (self.horizons, self.n_steps))
            else:
                if self.horizons != (0,):
                    raise ValueError('SampleStream: PreWorld predicts one state, horizons must be (0,)')
                self.pred_keys = ['semantic_occ']
            self.metric = self.score.get('metric')
            if self.metric is None:
                dev = self.example[1].device
                kw = dict(num_classes=n_cl, use_image_mask=mask == 'camera', use_lidar_mask=mask == 'lidar', device=dev)
                self.metric = metrics.Metric_mIoU_Temporal(**kw) if self.temporal else metrics.Metric_mIoU(**kw)
            fs = self.score.get('fscore')
            if fs is not None:
                fs = dict(fs)
                fmask = fs.pop('mask', None)
                if fmask not in ('camera', 'lidar', None):
                    raise ValueError("SampleStream: fscore['mask'] must be 'camera', 'lidar' or None, got %r" % (fmask,))
                fmask_key = {'camera': 'mask_camera', 'lidar': 'mask_lidar', None: None}[fmask]
                group, self.fs_totals, self.fs_empty = metrics.Metric_FScore._group(
                    len(self.horizons), use_image_mask=fmask == 'camera', use_lidar_mask=fmask == 'lidar',
                    device=self.example[1].device, **fs)
                self.fscore = dict(zip(self.horizons, group))
                own = fmask_key is not None and fmask_key != self.mask_key
                self.fs_mask_key = fmask_key if own else None
                self._fs_cap = dict(kernel=group[0].kernel_args(), own_mask=own, mask_key=fmask_key)
        self.replays = self.recalibrations = self.recaptures = 0
        self.slots = []
        self.metric_stream = None
        self._fp = None
        self._capture()

    def _fingerprint(self):
        from .modules import precision, tensor_key
        return (precision(),) + tensor_key(list(self.net.parameters()) + list(self.net.buffers()))      # the net keeps them alive

    def _capture(self):
        self.close()
        frames, ego = self.example
        kw = dict(pred_keys=self.pred_keys, n_cl=self.score['n_cl'] if self.score else 18, masked=self.mask_key is not None,
                  payload=self.payload, fscore=self._fs_cap)
        self.slots = [_StreamSlot(self, _ScoredCapture(self.net, frames, ego, self.n_steps, **kw)) for _ in range(self.in_flight)]
        self._fp = self._fingerprint()

    def recapture(self):
        """capture every slot again (what run() does by itself when the fingerprint changed)"""
        self._capture()
        self.recaptures += 1

    def _fs_row(self, index):
        """row `index` of the deferred F-score table (on the metric stream; grown by doubling, the new rows zero)"""
        rows = self.fs_rows
        if rows is None or index >= rows.shape[0]:
            n = max(index + 1, 16, 2 * rows.shape[0] if rows is not None else 0)
            grown = torch.zeros((n, len(self.horizons), 4), dtype=torch.int64, device=self.fs_totals.device)
            if rows is not None:
                grown[:rows.shape[0]].copy_(rows)
            self.fs_rows = rows = grown
        return rows[index]

    def run(self, samples, indexed=False):
        if not self.slots:
            raise RuntimeError('SampleStream: closed')
        if self._fingerprint() != self._fp:
            self.recapture()
        self.metric_stream = torch.cuda.current_stream() if self.metric is not None else None     # where the totals are added
        sched = StreamScheduler(self.slots)
        try:
            for r in sched.run(samples, indexed=indexed):
                yield r
        finally:
            self.replays += sched.replays
            self.recalibrations += sched.recalibrations

    def close(self):
        """free the graphs and the static buffers of every slot"""
        if self.slots:
            torch.cuda.synchronize()
            for sl in self.slots:
                sl.cap.graph.reset()
            self.slots = []
            torch.cuda.empty_cache()
