#!/usr/bin/env python
"""Headline benchmark: samples/s of PreWorld's camera->voxel occupancy hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config C3|C2|C5] [--mode replicas|sharded] [--no-graph] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \\
        --master-port P bench.py --gpus N --steps K --warmup W

One "step" = one sample through the whole hot path with every input already resident in HBM:
  C3 (default, BASELINE.json configs[2], the config north_star's target is quoted on):
     2 frames (key + adjacent) x [LSS geometry -> voxel sort -> voxel pooling -> pre_process],
     concat -> CustomResNet3D [1,2,4] -> LSSFPN3D -> final_conv -> 6-step state-conditioned
     forecast -> OccHead x 7 states -> 7 semantic + 7 geometric uint8 200x200x16 grids, delivered as the reference
     delivers them: contiguous (X,Y,Z) uint8 arrays in HOST memory (one async D2H copy per sample, inside the step).
  C2 (configs[1]): key frame only (with_prev=False), the PreWorld detector, 1 state.
Inputs are what LSSViewTransformerBEVDepth.forward hands to view_transform
(mmdet3d/models/necks/view_transformer.py:798-803): softmaxed depth (6,88,32,88) and context
features (6,32,32,88) per frame plus the camera tensors; the image backbone / DepthNet stay on
PyTorch and are outside the measured path.  Weights are random (seeded), data
synthetic -- there is no dataset or checkpoint in this environment.

--mode replicas (default; what the driver runs): N > 1 = one process per GPU, each rank runs its own sample stream
  (samples are independent: no data-path collective), barrier + synchronize on both sides, max over ranks -> weak scaling.
--mode sharded (BASELINE.json configs[3], the latency mode of DESIGN.md section 7): ONE sample per step for the whole
  job -- frames lifted on different ranks + RCCL all_gather of the voxel features, encoder on every rank, the 7 states
  forecast + decoded round-robin + RCCL all_gather of the uint8 grids (harness.simple_test_sharded) -> strong scaling.

A plain run sets up, warms up, times the K steps, writes --dump-outputs and prints the headline line; every figure that needs runs
of its own is measured only with --full, and then the JSON line also carries
  roofline     -- the kernel with the largest share of the step BY ROCPROF KERNEL NAME (plus the HBM-bound voxel-pooling
                  kernel under `also`): algorithmic work / HIP-event duration measured live on the launch stream
  cpu_baseline -- the same C3 sample at FULL size on the host cores (no extrapolation): the PyTorch-CPU composition
                  (median of 5 after a warm-up) and the OpenMP port (the reference has no CPU path for its native ops).
  extra        -- measured after the timed region: c2 (single frame, 1 state), c5 (render head forward / forward + backward, the
                  pre-train step), train (the voxel-side fine-tune step, forward + backward); --no-extra skips them.
and config.single_sample_latency_ms, config.replay_same_inputs, config.sharded_phase_ms_rank0 (--mode sharded); with --config C5,
the forward-only, bf16-grid, transparent-scene, 38 400 x 417 and pre-train figures and the roofline.  Without --full these are null.

--dump-outputs DIR writes the result of the last timed step (rank 0's) as DIR/<name>.npy (float32; arrays above 2^20 elements as a
seeded sample of 2^19; at most 64 MB in all) and lists them under `dump_outputs`: the same arguments give the same inputs on every
run, so two builds can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from preworld_amd import _lib  # noqa: E402
from preworld_amd import harness  # noqa: E402
from preworld_amd import ops  # noqa: E402
from preworld_amd import synth as S  # noqa: E402
from preworld_amd.modules import precision  # noqa: E402

# /opt/skills/guides/MI355X_MICROARCH.md: dense MFMA peaks and HBM3E
PEAK_TFLOPS = {'f32': 157.3, 'f16': 2500.0}
PEAK_HBM_GBPS = 8000.0


def build_net(dev, config):
    cfg = harness.model_cfg(S.GRID_CONFIG_FULL, with_prev=config == 'C3',
                            detector='PreWorld4DTraj' if config == 'C3' else 'PreWorld')
    sd = S.synth_state_dict(0)
    return harness.build_model(cfg, sd, dev), sd


def make_inputs(dev, seed, n_frames):
    frames = harness.lifted_frames(seed, 6, dev, n_frames=n_frames)
    ego = torch.from_numpy(S.ego_state(seed)).to(dev)
    return frames, ego


# ------------------------------------------------------------------------------ --dump-outputs
DUMP_MAX_BYTES = 64 * 10 ** 6      # one dump, all files together
DUMP_WHOLE_MAX = 1 << 20           # arrays of up to this many elements are written whole,
DUMP_SAMPLE = 1 << 19              # larger ones as this many elements at fixed positions (seed 0, sorted, drawn from the flat index)


def dump_outputs(out, path):
    """Writes the result dict of the last timed step to path/<name>.npy, float32 (float64 stays float64): every tensor a caller
    receives, one file each (a list entry of more than one tensor becomes <name>_<i>), h2 storage expanded exactly to fp32.
    'grids' is skipped: it holds the same bytes as the semantic_occ_* / geo_occ_* entries.  Inputs and sample positions depend
    only on the command line, so two builds can be compared file by file.  Returns {name: shape written}."""
    def host(t):
        if isinstance(t, ops.H2):
            t = ops.h2_to_f32(t)
        t = t.detach()
        t = t.double() if t.dtype == torch.float64 else t.float()
        if t.numel() > DUMP_WHOLE_MAX:
            idx = np.sort(np.random.RandomState(0).randint(0, t.numel(), DUMP_SAMPLE))
            t = t.reshape(-1)[torch.from_numpy(idx).to(t.device)]
        return t.cpu().numpy()
    arrays = {}
    for key, v in out.items():
        if key == 'grids' or v is None:
            continue
        if isinstance(v, (list, tuple)):
            for i, t in enumerate(v):
                arrays[key if len(v) == 1 else '%s_%d' % (key, i)] = host(t)
        else:
            arrays[key] = host(v)
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_MAX_BYTES:
        raise SystemExit('bench.py --dump-outputs: %d bytes, more than %d' % (total, DUMP_MAX_BYTES))
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + '.npy'), a)
    return {name: list(a.shape) for name, a in sorted(arrays.items())}


# ------------------------------------------------------------------------------ roofline probe
class KernelProbe:
    """Times every hot launch of one eager step with HIP events recorded on the launch stream (torch's current stream ==
    the stream passed through the C ABI) and asks the library which kernel it picked (pw_last_kernel)."""

    OPS = ('conv3d_ndhwc', 'conv3d_wino', 'conv3d_h2', 'occ_head_fused', 'occ_head_h2', 'forecast_steps', 'forecast_steps_h2', 'fpn3d_fuse', 'bev_pool_dense',
           'segment_sort', 'lss_voxel_index', 'lss_lift_pool', 'f32_to_h2', 'h2_to_f32')

    def __init__(self):
        self.records = []
        self._orig = {}

    def __enter__(self):
        for name in self.OPS:
            self._orig[name] = getattr(ops, name)
            setattr(ops, name, self._wrap(name, self._orig[name]))
        return self

    def __exit__(self, *a):
        for name, fn in self._orig.items():
            setattr(ops, name, fn)

    def _wrap(self, name, fn):
        def inner(*args, **kw):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = fn(*args, **kw)
            e.record()
            kernel = _lib.lib().pw_last_kernel().decode() or name
            self.records.append((self._work(name, args, kw, out), kernel, s, e))
            return out
        return inner

    @staticmethod
    def _work(name, args, kw, out):
        """label + algorithmic (direct-form) flops, flops the matrix pipe really executes, algorithmic HBM bytes, dtype of the
        MFMA operands, and how many 'units' (the reference's own launch granularity) the launch covers."""
        w = dict(label=name, flops=0.0, exec_flops=0.0, bytes=0.0, mfma='f32', units=1)
        if name == 'conv3d_ndhwc':
            x, wpk = args[0], args[1]
            B, D, H, W, Cin = x.shape
            taps, nt = wpk.shape[1], wpk.shape[2]
            ks, st = kw.get('ksize', 3), kw.get('stride', 1)
            nv = B * (D // st) * (H // st) * (W // st)
            cout = (kw.get('cout0') or nt * 32) + (kw.get('cout1') or 0)
            fl = 2.0 * nv * taps * Cin * cout
            w.update(label='conv3d k%d s%d %dx%dx%d %d->%d' % (ks, st, D, H, W, Cin, cout), flops=fl, exec_flops=fl,
                     bytes=4.0 * (x.numel() + nv * cout + wpk.numel()))
        elif name == 'conv3d_wino':
            # algorithmic work = the direct-form conv; Winograd F(2,3)^3 executes 64 transform-domain
            # products per 2x2x2 outputs instead of 8*27: x8/27 of these flops on the matrix pipe
            x, uw = args[0], args[1]
            B, D, H, W, Cin = x.shape
            cout = (kw.get('cout0') or uw.shape[2] * 16) + (kw.get('cout1') or 0)
            nv = B * D * H * W
            fl = 2.0 * nv * 27 * Cin * cout
            w.update(label='conv3d k3 s1 %dx%dx%d %d->%d' % (D, H, W, Cin, cout), flops=fl, exec_flops=fl * 8 / 27,
                     bytes=4.0 * (x.numel() + nv * cout + uw.numel()))
        elif name == 'conv3d_h2':
            # split-fp16 operands on the fp16 matrix cores: three MFMA products per direct-form multiply
            x, wpk = args[0].buf, args[1]
            B, D, H, W, Cin = x.shape
            taps, nt = wpk.shape[1], wpk.shape[2]
            ks, st = kw.get('ksize', 3), kw.get('stride', 1)
            nv = B * (D // st) * (H // st) * (W // st)
            cout = (kw.get('cout0') or nt * 32) + (kw.get('cout1') or 0)
            fl = 2.0 * nv * taps * Cin * cout
            w.update(label='conv3d k%d s%d %dx%dx%d %d->%d' % (ks, st, D, H, W, Cin, cout), flops=fl, exec_flops=3.0 * fl,
                     mfma='f16', bytes=4.0 * (x.numel() + nv * cout + wpk.numel()))
        elif name in ('f32_to_h2', 'h2_to_f32'):
            t = args[0].buf if hasattr(args[0], 'buf') else args[0]
            w.update(label=name, mfma=None, bytes=8.0 * t.numel())
        elif name == 'occ_head_fused':
            x = args[0]
            nv = x.numel() // x.shape[-1]
            wino = args[1].dim() == 5
            conv, tail = 2.0 * nv * 27 * 32 * 16, 2.0 * nv * (16 * 8 + 8 * 18)
            # the six forecast states are decoded by ONE launch over a batch of 6: counted as 6 units of one state each
            w.update(label='occ_head 32->16->8->18 + argmax', flops=conv + tail,
                     exec_flops=(conv * 8 / 27 if wino else conv) + tail, bytes=4.0 * x.numel() + 2.0 * nv,
                     units=int(x.shape[0]))
        elif name == 'occ_head_h2':
            x = args[0].buf
            nv = x.numel() // x.shape[-1]
            fl = 2.0 * nv * (27 * 32 * 16 + 16 * 8 + 8 * 18)
            w.update(label='occ_head 32->16->8->18 + argmax', flops=fl, exec_flops=3.0 * fl, mfma='f16',
                     bytes=4.0 * x.numel() + 2.0 * nv, units=int(x.shape[0]))
        elif name in ('forecast_steps', 'forecast_steps_h2'):
            v0, n_steps = args[0], (args[6] if name == 'forecast_steps' else args[5])
            v0 = v0.buf if hasattr(v0, 'buf') else v0
            nv = v0.numel() // 32
            fl = 2.0 * nv * n_steps * (32 * 128 + 128 * 32)
            h2 = name.endswith('h2')
            w.update(label='forecast %d steps' % n_steps, flops=fl, exec_flops=3.0 * fl if h2 else fl,
                     mfma='f16' if h2 else 'f32', bytes=4.0 * v0.numel() * (1 + n_steps))
        elif name == 'fpn3d_fuse':
            x = args[0].buf if hasattr(args[0], 'buf') else args[0]
            fl = 2.0 * (x.numel() // 32) * 32 * 32
            w.update(label='fpn3d_fuse', flops=fl, exec_flops=fl, bytes=8.0 * x.numel())
        elif name == 'bev_pool_dense':
            depth, feat, vs = args[0], args[1], args[2]
            kept = int(vs.seg_start[-1].item())                # points inside the grid (device value; eager probe only)
            C = feat.shape[-1]
            w.update(label='bev_pool_dense', flops=2.0 * C * kept, exec_flops=0.0, mfma=None,
                     bytes=4.0 * (vs.n_keys * C + depth.numel() + feat.numel() + (vs.n_keys + 1) + 2 * kept))
        elif name == 'lss_lift_pool':
            # one frame's whole lift (camera matrices, voxel ids, point lists, pooling: 5 launches, timed together).  Algorithmic
            # bytes = SURVEY 8(d)'s 90.0 MB per frame: the pooled grid written once (81.92), depth (5.95) and context (2.16) read
            # once; the frustum table (2.97 MB, shared by the cameras and L2-resident), the id slots and the lists are the
            # implementation's own traffic and are not counted
            fr, depth, feat = args[0], args[9], args[10]
            size = args[8]
            n_vox = int(args[1].shape[0]) * int(size[0]) * int(size[1]) * int(size[2])
            C = feat.shape[-1]
            w.update(label='lss_lift_pool (whole frame, 5 launches)', flops=2.0 * C * depth.numel(), exec_flops=0.0, mfma=None,
                     bytes=4.0 * (n_vox * C + depth.numel() + feat.numel()))
        elif name == 'segment_sort':
            keys, n_keys = args[0], args[1]
            w.update(label='segment_sort', mfma=None, bytes=4.0 * (3 * keys.numel() + 2 * n_keys))
        elif name == 'lss_voxel_index':
            fr = args[0]
            n = args[9] * args[10] * fr.shape[0] * fr.shape[1] * fr.shape[2]
            w.update(label='lss_voxel_index', mfma=None, bytes=16.0 * n)
        return w

    def summary(self):
        torch.cuda.synchronize()
        by_kernel = {}
        for w, kernel, s, e in self.records:
            a = by_kernel.setdefault(kernel, dict(launches=0, units=0, ms=0.0, flops=0.0, exec_flops=0.0, bytes=0.0,
                                                  mfma=w['mfma'], labels={}))
            dt = s.elapsed_time(e)
            a['launches'] += 1
            a['units'] += w['units']
            a['ms'] += dt
            for k in ('flops', 'exec_flops', 'bytes'):
                a[k] += w[k]
            lab = a['labels'].setdefault(w['label'], dict(launches=0, ms=0.0, flops=0.0, bytes=0.0))
            lab['launches'] += 1
            lab['ms'] += dt
            lab['flops'] += w['flops']
            lab['bytes'] += w['bytes']
        return by_kernel


_PMC_BUILD = [None]           # build id of the library the newest committed PMC passes were collected on


def lib_build_id():
    import ctypes
    fn = _lib.lib().pw_build_id
    fn.restype = ctypes.c_char_p
    return fn().decode()


def _pmc_traffic(kernel):
    """HBM bytes per launch from the committed rocprofv3 --pmc passes (PMC counters cannot be read from inside this
    process; profiles/*_pmc_traffic.json says how they were collected and corrected), newest round first."""
    prof = os.path.join(ROOT, 'profiles')
    for name in sorted((f for f in os.listdir(prof) if f.endswith('_pmc_traffic.json')), reverse=True):
        doc = json.load(open(os.path.join(prof, name)))
        by = doc.get('by_kernel', {})
        _PMC_BUILD[0] = doc.get('build_id')
        name = '%s, library build id %s' % (name, doc.get('build_id') or 'not recorded')
        if kernel == 'k_lss_pool_slots':
            # ops.lss_lift_pool is probed as ONE unit (5 launches, the library reports its last kernel): traffic of all five
            ents = [v for k, v in by.items() if k.startswith('k_lss_')]
            if ents:
                return int(sum(e['fetch_bytes'] + e['write_bytes'] for e in ents)), name
        ent = by.get(kernel)
        if ent is None and kernel == 'k_render_rays':                    # the forward instantiation of the literal 3 072 x 96 shape
            ent = by.get('k_render_rays<2, 0, false>')
        if ent:
            return int(ent['fetch_bytes'] + ent['write_bytes']), name
    return None, None


def roofline_object(agg, n_probe_steps):
    def entry(kernel, a):
        sec = a['ms'] * 1e-3
        traffic, src = _pmc_traffic(kernel)
        ent = dict(kernel=kernel if kernel != 'k_lss_pool_slots' else 'k_lss_prologue + k_lss_index_slots + k_lss_heavy_alloc + k_lss_ovf_scatter + k_lss_pool_slots',
                   launches_per_step=a['launches'] // n_probe_steps,
                   avg_launch_us=round(a['ms'] * 1e3 / a['launches'], 2), us_per_step=round(a['ms'] * 1e3 / n_probe_steps, 1),
                   algorithmic_bytes=int(a['bytes'] / a['launches']), traffic=traffic,
                   traffic_unit='HBM bytes per launch (PMC, %s)' % src if src else None,
                   # VERDICT r05 hygiene: is the PMC pass from THIS library?  (kernels whose source file did not change keep their traffic)
                   traffic_build_matches=(_PMC_BUILD[0] == lib_build_id()) if src else None,
                   timing='avg_launch_us / us_per_step: eager HIP-event pass on the launch stream inside this run (%d probe steps); the '
                          'rocprofv3 --kernel-trace --stats averages of the same command are in profiles/ (newest *_bench_kernel_stats.md) '
                          'and agree within the box-to-box spread (~4 %%)' % n_probe_steps)
        if a['mfma']:
            peak = PEAK_TFLOPS[a['mfma']]
            direct, execd = a['flops'] / sec / 1e12, a['exec_flops'] / sec / 1e12
            ent.update(bound='mfma', achieved=round(direct, 2), peak=peak, unit='TFLOP/s', frac=round(direct / peak, 4),
                       pipe_busy=round(execd / peak, 4), executed_tflops=round(execd, 2), mfma_operands=a['mfma'],
                       note='achieved = ALGORITHMIC (direct-form) FLOPs / time and frac = achieved / dense peak of the MFMA '
                            'operand type, as SURVEY 8(d) defines it; pipe_busy = FLOPs the matrix pipe actually executes / time '
                            '/ peak (split-fp16 executes 3 products per direct-form multiply, so its frac cannot exceed 1/3; '
                            'Winograd F(2,3)^3 executes 8/27, so its frac can exceed pipe_busy)')
        else:
            gbps = a['bytes'] / sec / 1e9
            ent.update(bound='hbm', achieved=round(gbps, 1), peak=PEAK_HBM_GBPS, unit='GB/s', frac=round(gbps / PEAK_HBM_GBPS, 4))
        ent['shapes'] = {k: dict(launches=v['launches'] // n_probe_steps, avg_us=round(v['ms'] * 1e3 / v['launches'], 1),
                                 tflops=round(v['flops'] / (v['ms'] * 1e-3) / 1e12, 1),
                                 alg_GBps=round(v['bytes'] / (v['ms'] * 1e-3) / 1e9, 1))
                         for k, v in sorted(a['labels'].items(), key=lambda kv: -kv[1]['ms'])}
        return ent
    order = sorted(agg.items(), key=lambda kv: -kv[1]['ms'])
    dom = entry(*order[0])
    dom['also'] = [entry(k, a) for k, a in order[1:] if k.startswith(('k_pool_dense', 'k_lss_pool'))]
    dom['step_gflop'] = round(sum(a['flops'] for _, a in order) / n_probe_steps / 1e9, 1)       # direct-form FLOPs of one sample, all kernels
    dom['all_kernels'] = {k: dict(us_per_step=round(a['ms'] * 1e3 / n_probe_steps, 1), launches=a['launches'] // n_probe_steps,
                                  tflops=round(a['flops'] / (a['ms'] * 1e-3) / 1e12, 2),
                                  alg_GBps=round(a['bytes'] / (a['ms'] * 1e-3) / 1e9, 1)) for k, a in order}
    return dom


# ------------------------------------------------------------------------------ CPU baseline
def host_cpu():
    """model string and logical CPU count of the box the baseline ran on (lscpu / nproc)"""
    import subprocess
    model = None
    try:
        for line in subprocess.run(['lscpu'], capture_output=True, text=True, timeout=10).stdout.splitlines():
            if line.startswith('Model name'):
                model = line.split(':', 1)[1].strip()
                break
    except Exception:                                                     # noqa: BLE001
        pass
    if model is None:
        try:
            model = next(l.split(':', 1)[1].strip() for l in open('/proc/cpuinfo') if l.startswith('model name'))
        except Exception:                                                 # noqa: BLE001
            model = 'unknown'
    return dict(model=model, nproc=os.cpu_count(), sockets_visible=len({l for l in open('/proc/cpuinfo') if l.startswith('physical id')}) or None)


def cpu_baseline(sd, seed=100, step_gflop=None):
    """The C3 sample at FULL size (6 cameras, 200x200x16, key + adjacent frame, 7 states) on the host cores, no
    extrapolation.  Two stand-ins, because the reference has NO CPU path for its native ops:
      * torch-cpu: the reference's nn.Modules are plain torch layers, so oracle/torch_ref.py runs the same composition on
        PyTorch-CPU (oneDNN convolutions, torch.set_num_threads(all cores));
      * openmp-port: oracle/pw_oracle.c (the parity checker);
    each leg: median of 5 runs after 1 warm-up.
    `value` is the faster of the two.  The voxel pooling of both comes from the C oracle and is inside the timed region."""
    from oracle import oracle as O
    from oracle import torch_ref as TR
    threads = O.num_threads()
    torch.set_num_threads(threads)
    gc = S.GRID_CONFIG_FULL
    ego = S.ego_state(seed)

    def torch_run():
        t0 = time.perf_counter()
        bevs = TR.lifted_bevs(seed, 6, gc)
        st = TR.c3_sample(bevs, ego, sd, n_steps=6)
        assert len(st) == 7 and st[0].shape == (200, 200, 16)
        return time.perf_counter() - t0

    def port_run():
        t0 = time.perf_counter()
        bevs = TR.lifted_bevs(seed, 6, gc)
        pre = [O.pre_process(b, sd) for b in bevs]
        vf = O.final_conv(O.encoder_forward(pre[1], pre[0], sd), sd)
        states, _ = O.preworld4d_decode(vf, ego, sd, n_steps=6, post_finetune=True)
        assert len(states) == 7 and states[0].shape == (200, 200, 16)
        return time.perf_counter() - t0

    RUNS = 5                                           # each leg: 1 warm-up + RUNS timed runs, median reported (>= 5)
    torch_run()
    tt = sorted(torch_run() for _ in range(RUNS))
    port_run()
    tp = sorted(port_run() for _ in range(RUNS))
    t_torch, t_port = tt[RUNS // 2], tp[RUNS // 2]
    best = min(t_torch, t_port)
    return dict(value=1.0 / best, unit='samples/s', cores=threads, kind='port', host=host_cpu(),
                # what the host leg reaches on the same direct-form FLOP count the GPU roofline uses (VERDICT r05 hygiene): a few per cent
                # of the host's own peak -- the GPU / CPU ratio says nothing about kernel quality, roofline.frac does
                host_gflops=dict(sample_gflop=step_gflop, openmp_port=round(step_gflop / t_port, 1), torch_cpu=round(step_gflop / t_torch, 1))
                if step_gflop else None,
                torch_cpu=dict(samples_per_s=round(1.0 / t_torch, 4), median_s=round(t_torch, 3), min_s=round(tt[0], 3),
                               max_s=round(tt[-1], 3), runs=RUNS, warmup=1, threads=threads),
                openmp_port=dict(samples_per_s=round(1.0 / t_port, 4), median_s=round(t_port, 3), min_s=round(tp[0], 3),
                                 max_s=round(tp[-1], 3), runs=RUNS, warmup=1, threads=threads),
                sample='full-size C3 sample (6 cams, 200x200x16, key+adjacent, 7 states), unscaled; both legs: median of %d runs '
                       'after 1 warm-up: PyTorch-CPU composition of the reference modules = %.2f s; OpenMP port '
                       '(oracle/pw_oracle.c) = %.2f s; %d host threads; value = the faster one; the reference itself has no CPU '
                       'path for bev_pool_v2 / render ops (CUDA only)' % (RUNS, t_torch, t_port, threads))


# ------------------------------------------------------------------------------ main
def bench_c5(args):
    print(json.dumps(c5_result(args)))


def c5_result(args, quick=False):
    """Extra, non-headline line (BASELINE.json configs[4]): the volume-rendering attribute head at the literal C5 shape
    -- 6 cameras x 512 rays x 96 uniform samples through the packed (200,200,16,24) sigma / semantic / colour grid -- forward
    (pw_render_rays) and forward + backward (pw_render_rays_backward_sorted), one GPU, on TWO scenes:
      'mixed'       S.render_grids_mixed / S.rays_mixed: ground slab + boxes with density ~U(10,22) (occupied <=> density > 8.5,
                    detectors/preworld.py:32,180) -- the rays that meet them TERMINATE at T < 1e-3 (render_utils_kernel.cu:591-603);
                    the fraction that does is measured on the device and reported (`terminated_frac`);
      'transparent' density 4.0 in a ground slab and a ring of blocks, -8 elsewhere: alpha ~3e-5 per sample, NO ray terminates
                    (every round-2..4 figure was of this kind).
    `value` = rays/s of forward + backward on the mixed scene; the reference's own 38 400 x 417 shape is in config for both.
    Without --full only that headline is measured: the transparent scene, the other figures and the roofline are null."""
    from preworld_amd import modules as M
    dev = 'cuda:0'
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                                   # noqa: E731
    head = M.NerfHead(point_cloud_range=[-40, -40, -1, 40, 40, 5.4], voxel_size=0.4, scene_center=[0, 0, 2.2], radius=39).to(dev)
    consts = head.consts(torch.eye(3))
    b = torch.linspace(0, 2, 97)
    t96 = ((b[1:] + b[:-1]) * 0.5).to(dev).contiguous()
    steps = 20 if quick else args.steps
    last = {}                                   # what the headline's last timed step (mixed scene, forward + backward) computed

    def timed(fn, steps, warmup):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps, out

    def scene(name):
        if name == 'mixed':
            dens, semantic, color = S.render_grids_mixed(41)
            ray_fn = S.rays_mixed
        else:
            _, semantic, color = S.render_grids(41)
            xs, ys, zs = np.meshgrid(np.arange(200), np.arange(200), np.arange(16), indexing='ij')
            rr = np.hypot(xs - 100, ys - 100)
            dens = np.where((zs < 2) | ((rr > 40) & (rr < 60) & ((xs // 8 + ys // 8) % 2 == 0)), 4.0, -8.0).astype(np.float32)
            ray_fn = S.rays
        grid = M.pack_attribute_grid(T(dens), T(semantic), T(color))
        g16 = grid.to(torch.bfloat16)

        def shape(R, t):
            o, d = ray_fn(7, R)
            ro, rd = T(o), T(d)
            g = torch.Generator(device=dev).manual_seed(0)
            gd, gs, gc, gl = (torch.randn(R, device=dev, generator=g), torch.randn(R, 17, device=dev, generator=g),
                              torch.randn(R, 3, device=dev, generator=g), torch.randn(R, device=dev, generator=g))
            gg = torch.zeros_like(grid)
            dbg = ops.render_rays(ro, rd, t, grid, consts, want_debug=True)
            stats = dict(terminated_frac=round(float((dbg['alphainv_last'] < 1e-3).float().mean()), 4),
                         kept_samples_per_ray=round(float(dbg['counts'][:, 2].float().mean()), 1))

            def fwd():
                ops.render_rays(ro, rd, t, grid, consts)

            def fwd_bwd():
                out = ops.render_rays(ro, rd, t, grid, consts)
                gg.zero_()
                ops.render_rays_backward(ro, rd, t, grid, consts, gd, gs, gc, gl, grad_grid=gg)
                return dict(out, grad_grid=gg)
            return fwd, fwd_bwd, (lambda: ops.render_rays(ro, rd, t, g16, consts)), stats
        fwd, fwd_bwd, fwd16, st = shape(3072, t96)
        t_end = time.perf_counter() + args.settle_s / 2
        while time.perf_counter() < t_end:
            fwd_bwd()
        t_fb, out = timed(fwd_bwd, steps, args.warmup)
        if name == 'mixed':
            last.update(out)
        fb = dict(st, fwd_bwd_ms=round(t_fb * 1e3, 4), rays_per_s_fwd_bwd=round(3072 / t_fb, 1),
                  fwd_bwd_samples_per_s=round(3072 * 96 / t_fb, 0))
        if not args.full:
            return fb, None
        t_f, t_f16 = timed(fwd, steps, args.warmup)[0], timed(fwd16, steps, args.warmup)[0]
        rf, rfb, _, st_ref = shape(38400, head.t_table(dev))
        t_rf, t_rfb = timed(rf, 10, 2)[0], timed(rfb, 5, 1)[0]
        return dict(fb, forward_ms=round(t_f * 1e3, 4), forward_bf16_grid_ms=round(t_f16 * 1e3, 4),
                    forward_samples_per_s=round(3072 * 96 / t_f, 0),
                    reference_shape_38400x417=dict(st_ref, forward_ms=round(t_rf * 1e3, 3), fwd_bwd_ms=round(t_rfb * 1e3, 3),
                                                   forward_samples_per_s=round(38400 * 417 / t_rf, 0))), grid.numel() * 4 / t_f
    mixed, fwd_bytes_per_s = scene('mixed')
    dumped = dump_outputs(last, args.dump_outputs) if args.dump_outputs and not quick else None
    last.clear()
    transparent = scene('transparent')[0] if args.full else None
    pretrain = pretrain_step_ms(dev, args) if args.full else None
    traffic, traffic_src = _pmc_traffic('k_render_rays') if args.full else (None, None)
    res = {
        'metric': 'rays/sec (render head forward + backward, 6 cams x 512 rays x 96 samples)', 'value': mixed['rays_per_s_fwd_bwd'],
        'unit': 'rays/s', 'n_gpus': 1, 'steps': steps, 'warmup': args.warmup, 'ms_per_step': mixed['fwd_bwd_ms'],
        'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
        'config': {
            'workload': 'C5: NerfHead render, 3072 rays x 96 uniform samples, packed (200,200,16,24) fp32 grid, mixed-opacity scene '
                        '(%.0f %% of the rays terminate at T < 1e-3); a step = forward + zero-fill of the gradient grid + backward'
                        % (100 * mixed['terminated_frac']),
            'terminated_frac': mixed['terminated_frac'], 'mixed': mixed, 'transparent': transparent,
            'forward_ms': mixed.get('forward_ms'), 'reference_shape_38400x417': mixed.get('reference_shape_38400x417'),
            'pretrain_step': pretrain,
            'backward': 'pw_render_rays_backward_sorted: entries sorted by voxel, 64-bit fixed-point segmented sums, no float atomics, '
                        'bit-reproducible',
            'note': 'extra, non-headline entry; the headline metric is --config C3'},
        'roofline': {'bound': 'hbm', 'kernel': 'k_render_rays', 'achieved': round(fwd_bytes_per_s / 1e9, 1), 'peak': PEAK_HBM_GBPS,
                     'unit': 'GB/s', 'frac': round(fwd_bytes_per_s / 1e9 / PEAK_HBM_GBPS, 4), 'traffic': traffic,
                     'traffic_unit': 'HBM bytes per forward launch at 3072 x 96 (PMC, %s)' % traffic_src if traffic_src else None,
                     'note': 'algorithmic bytes = the 61 MB packed grid read once per forward (SURVEY 8d); the kernel is bound by the '
                             'per-ray scan and gather latency, not by HBM (profiles/r02_render_c5.txt)'} if args.full else None,
    }
    if dumped is not None:
        res['dump_outputs'] = dict(dir=args.dump_outputs, arrays=dumped)
    return res


def _sub_json(cmd, env, pick, timeout=600):
    """run a bench command in its own process, take the last JSON line it prints, return pick(line) (or {'error': ...}: an extra figure
    must not take the headline line down)"""
    import subprocess
    try:
        out = subprocess.run(cmd, env=dict(os.environ, **env), capture_output=True, text=True, timeout=timeout)
        lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
        if out.returncode != 0 or not lines:
            return {'error': 'rc %d: %s' % (out.returncode, out.stderr[-300:])}
        return pick(json.loads(lines[-1]))
    except Exception as e:                                                # noqa: BLE001
        return {'error': repr(e)[:300]}


def extra_figures(args, dev):
    """compact C2, C5 and training-step figures for the driver's record, measured AFTER the headline's timed region (BASELINE.json configs[1], [4]):
    C2 = single frame, PreWorld detector, 1 state (captured step, two in flight, rotating inputs like the headline); C5 = the render
    head forward / forward + backward at the literal 3 072 x 96 shape and at the reference's 38 400 x 417, and the pre-train step."""
    ex = {}
    try:
        from preworld_amd.pipeline import CapturedSample
        net2, _ = build_net(dev, 'C2')
        caps = [CapturedSample(net2, *make_inputs(dev, seed=50 + k, n_frames=1), n_steps=0, d2h=not args.no_d2h) for k in range(2)]
        sets = [make_inputs(dev, seed=2000 + j, n_frames=1) for j in range(3)]
        streams = [torch.cuda.Stream() for _ in range(2)]

        def run(n):
            for i in range(n):
                with torch.cuda.stream(streams[i % 2]):
                    caps[i % 2].run(*sets[i % 3])
        run(10)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 60
        run(n)
        torch.cuda.synchronize()
        e = time.perf_counter() - t0
        bad = [c.bad_replays() for c in caps]
        ex['c2'] = dict(workload='C2: single frame (with_prev=False), 6 cams, 200x200x16, PreWorld detector, 1 state; captured step, 2 in '
                                 'flight, 3 rotating input sets', samples_per_s=round(n / e, 2), ms_per_step=round(e / n * 1e3, 4),
                        steps=n, recalibrations=int(sum(b[0] for b in bad)))
        del caps, net2
    except Exception as e:                                                # noqa: BLE001
        ex['c2'] = {'error': repr(e)[:300]}
    try:
        # the reference-API entry beside the captured figure (VERDICT r05 hygiene / weak 11): the drop-in's simple_test path from the lifted
        # inputs, EAGER -- per call: range calibration check (one 2 KB D2H + host sync, detectors._ranged), ~60 launches, the payload as 14
        # numpy arrays (_to_numpy) -- one sample at a time, nothing in flight
        net3, _ = build_net(dev, 'C3')
        sets3 = [make_inputs(dev, seed=3000 + j, n_frames=2) for j in range(3)]
        for j in range(3):
            net3._to_numpy(net3.simple_test_from_lift(*sets3[j], n_steps=6))
        torch.cuda.synchronize()
        n = 30
        t0 = time.perf_counter()
        for i in range(n):
            res3 = net3._to_numpy(net3.simple_test_from_lift(*sets3[i % 3], n_steps=6))
        e = time.perf_counter() - t0
        assert len(res3) == 14 and res3['semantic_occ_6s'][0].shape == (200, 200, 16)
        # ... and the same entry with net.capture_replay (PreWorld4DTraj.simple_test_captured): the module's own hipGraph of the hot path,
        # range-checked on the host after every call, the 14 grids copied out of the pinned buffer
        for j in range(3):
            net3.simple_test_captured(*sets3[j])
        t0 = time.perf_counter()
        for i in range(n):
            res4 = net3.simple_test_captured(*sets3[i % 3])
        e4 = time.perf_counter() - t0
        n_diff = int(sum(int((res4[k][0] != res3[k][0]).sum()) for k in res3))
        ex['dropin_simple_test'] = dict(
            workload='C3 through PreWorld4DTraj.simple_test_from_lift + _to_numpy (the drop-in module API downstream of the image side), eager, '
                     'one sample at a time, 3 rotating input sets, host payload = 14 numpy uint8 grids', ms_per_sample=round(e / n * 1e3, 4),
            samples_per_s=round(n / e, 2), steps=n,
            captured=dict(what='the same entry with net.capture_replay = True (simple_test_captured: the module replays its own hipGraph, host '
                               'range check + payload copy per call, one sample at a time)', ms_per_sample=round(e4 / n * 1e3, 4),
                          samples_per_s=round(n / e4, 2), voxels_differing_from_eager=n_diff))
        del net3, sets3
    except Exception as e:                                                # noqa: BLE001
        ex['dropin_simple_test'] = {'error': repr(e)[:300]}
    try:
        r = c5_result(args, quick=True)
        c = r['config']
        ex['c5'] = dict(workload='C5: NerfHead render 3072 rays x 96 samples (and the reference shape 38 400 x 417), one GPU',
                        rays_per_s_fwd_bwd=r['value'], fwd_bwd_ms=r['ms_per_step'], forward_ms=c['forward_ms'],
                        terminated_frac=c['terminated_frac'], mixed=c['mixed'], transparent=c['transparent'],
                        reference_shape_38400x417=c['reference_shape_38400x417'], pretrain_step=c['pretrain_step'],
                        roofline=r['roofline'])
    except Exception as e:                                                # noqa: BLE001
        ex['c5'] = {'error': repr(e)[:300]}
    try:
        ex['train'] = finetune_step(dev)
    except Exception as e:                                                # noqa: BLE001
        ex['train'] = {'error': repr(e)[:300]}
    torch.cuda.empty_cache()
    ex['f32_exact'] = _sub_json([sys.executable, os.path.abspath(__file__), '--steps', '10', '--warmup', '3', '--settle-s', '1', '--full',
                                 '--no-extra', '--no-cpu-baseline'], dict(PW_PRECISION='f32'),
                                lambda r: dict(workload='C3 under PW_PRECISION=f32: every product an exact-fp32 MFMA (Winograd / direct conv '
                                                        'kernels, k_occ_head_wino, k_forecast), same captured step, same rotating inputs',
                                               samples_per_s=r['value'], ms_per_step=r['ms_per_step'], steps=r['steps'], dtype=r['dtype'],
                                               roofline_kernel=r['roofline'].get('kernel'), roofline_frac=r['roofline'].get('frac'),
                                               roofline_executed_frac=r['roofline'].get('pipe_busy'),
                                               roofline_note='roofline_frac = DIRECT-FORM FLOP/s / 157.3 TF fp32-MFMA peak; the dominant kernel '
                                                             'is Winograd F(2,3)^3, which executes 8/27 of them, so frac can exceed 1; '
                                                             'roofline_executed_frac = FLOPs the matrix pipe executes / peak'))
    # BASELINE configs[3] at world 1 (its own process: it initialises a 1-rank RCCL group): pipeline.ShardedSample, three graphs per rank
    ex['sharded_w1'] = _sub_json([sys.executable, os.path.abspath(__file__), '--mode', 'sharded', '--steps', '30', '--warmup', '5', '--settle-s', '1',
                                  '--full', '--no-extra', '--no-cpu-baseline'], dict(MASTER_PORT=str(29600 + os.getpid() % 300)),
                                 lambda r: dict(workload='C3 sample in the sharded latency mode (frames / states owned round-robin, two collectives), '
                                                         'world 1: every phase on this GPU, collectives trivial', samples_per_s=r['value'],
                                                ms_per_step=r['ms_per_step'], steps=r['steps'], phase_ms_rank0=r['config']['sharded_phase_ms_rank0'],
                                                recalibrations=r['config']['recalibrations'], replays_audited=r['config']['replays_audited']))
    tool = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tools', 'bench_image_path.py')
    img = {}
    for amp in ('none', 'bf16'):
        img['image_side_' + ('f32' if amp == 'none' else 'bf16_autocast')] = _sub_json(
            [sys.executable, tool, '--steps', '5', '--amp', amp], {},
            lambda r: dict(samples_per_s=r['value'], ms_per_sample=r['ms_per_sample'], image_branch_ms=r['image_branch_ms'],
                           voxel_path_ms=r['voxel_path_ms']))
    img['what'] = ('image -> occupancy, serial, 1 GPU: 6 cams x 3 frames of 3x512x1408 through Swin-B + FPN_LSS + DepthNet with the stereo cost '
                   'volume (PyTorch-ROCm, preworld_amd/image_encoder.py; OUTSIDE the measured path, SURVEY 8a) + the captured hot path')
    ex['image_to_occ'] = img
    torch.cuda.empty_cache()
    return ex


def finetune_step(dev, n=10):
    """The voxel side of PreWorld.forward_train for the fine-tune configs at the C3 shape (preworld.py:229-309; the composition of
    tools/bench_train.py): pooling of the key frame under autograd and of the adjacent frame without, pre_process, CustomResNet3D,
    LSSFPN3D, final_conv, OccHead with batch-statistics BatchNorm, loss_voxel (CE + sem_scal + geo_scal + focal + Lovasz), backward
    through all of it on the HIP training kernels (preworld_amd/train.py).  Image side excluded."""
    from preworld_amd.modules import to_channels_last_3d
    cfg = harness.model_cfg(S.GRID_CONFIG_FULL, detector='PreWorld')
    cfg.update(if_render=False, if_post_finetune=True, use_lss_depth_loss=False, weight_voxel_ce=1.0, weight_voxel_sem_scal=1.0,
               weight_voxel_geo_scal=1.0, weight_voxel_lovasz=1.0)
    net = harness.build_model(cfg, S.synth_state_dict(0), dev).train()
    frames = harness.lifted_frames(0, 6, dev, n_frames=2)
    sem = torch.randint(0, 18, (1, 200, 200, 16), device=dev)
    vt = net.img_view_transformer

    def lift(fr, grad):
        d, f = fr['depth'].detach().requires_grad_(grad), fr['tran_feat'].detach().requires_grad_(grad)
        B, N = fr['sensor2keyego'].shape[:2]
        inp = [d.new_empty(B, N, 1, d.shape[-2], d.shape[-1]), fr['sensor2keyego'], None, fr['intrin'], fr['post_rot'], fr['post_tran'],
               fr['bda']]
        return net.pre_process_net.forward_cl(to_channels_last_3d(vt.view_transform(inp, d, f)[0]).float())[0]

    def step():
        net.zero_grad(set_to_none=True)
        key = lift(frames[0], True)
        with torch.no_grad():
            adj = lift(frames[1], False)
        losses = net.forward_train_from_feats(net.bev_encoder_cl(torch.cat([adj, key], -1)), voxel_semantics=sem)
        sum(losses.values()).backward()
        return losses
    for _ in range(3):
        out = step()
    torch.cuda.synchronize()
    per = []
    for _ in range(n):                                  # every step timed on its own: the figure is the MEDIAN (an eager step of ~560 launches
        t0 = time.perf_counter()                        # picks up allocator / host hiccups: 14.8 .. 16.8 ms seen for the same build)
        step()
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) * 1e3)
    ms = float(np.median(per))
    return dict(workload='voxel side of PreWorld.forward_train, fine-tune config, C3 shape (6 cams, key + adjacent, 200x200x16), forward + '
                         'backward, eager (no graph capture); median of the steps', ms_per_step=round(ms, 2), steps=n,
                ms_min=round(min(per), 2), ms_max=round(max(per), 2),
                losses={k: round(float(v), 4) for k, v in out.items() if 'sup' not in k})


def pretrain_step_ms(dev, args):
    """The self-supervised pre-train step end to end downstream of the encoder (preworld.py:229-309 with if_render=True, SURVEY 3.3;
    VERDICT r02 missing 4): final_conv -> OccHead (zero-weight loss_sup_voxel keeps its parameters in the graph) -> density /
    semantic / colour MLPs -> NerfHead on 38 400 rays x 417 samples (fused render forward, silog depth + weighted CE + L1 colour +
    last-alpha entropy + distortion losses) -> backward through all of it (sorted render backward, MLP / conv / BatchNorm
    backward on the HIP training kernels and library GEMMs), from a random (1,16,200,200,32) neck output."""
    try:
        cfg = harness.model_cfg(S.GRID_CONFIG_FULL, detector='PreWorld', if_post_finetune=False)
        cfg.update(if_render=True, if_pretrain=True, use_lss_depth_loss=False, use_focal_loss=False,
                   nerf_head=dict(type='NerfHead', point_cloud_range=[-40, -40, -1, 40, 40, 5.4], voxel_size=0.4, scene_center=[0, 0, 2.2],
                                  radius=39, use_depth_sup=True, weight_depth=0.1, weight_semantic=0.1, weight_color=0.1))
        R = 38400
        o, d = S.rays_mixed(9, R, n_special=0)
        rs = np.random.RandomState(10)
        rays = np.zeros((1, R, 16), np.float32)
        rays[0, :, 2] = rs.uniform(1, 50, R); rays[0, :, 3] = rs.randint(0, 17, R); rays[0, :, 4:7] = o; rays[0, :, 7:10] = d
        rays[0, :, 13:16] = rs.standard_normal((R, 3))
        rays_t = torch.from_numpy(rays).to(dev)
        feat = torch.randn(1, 16, 200, 200, 32, device=dev)
        sem = torch.randint(0, 18, (1, 200, 200, 16), device=dev)
        bda = torch.eye(3, device=dev)[None]
        # a scene on which rays TERMINATE.  The synthetic density_mlp stays far below |act_shift| = 13.8 (every sample
        # transparent, entropy / distortion terms 0): its output row is rescaled (gain, shift) until a good part of the rays end at T < 1e-3;
        # the fraction is measured on the device from the training step's own alphainv_last and reported.
        stats = {}
        real_apply = ops.RenderRays.apply

        def spy(*a):
            out = real_apply(*a)
            last = out[3].detach()
            stats.update(terminated_frac=round(float((last < 1e-3).float().mean()), 4),
                         partly_opaque_frac=round(float(((last >= 1e-3) & (last < 0.99)).float().mean()), 4), rays_rendered=int(last.numel()))
            return out
        net = None
        for gain, shift in ((1.0, 0.0), (8.0, 0.0), (16.0, -4.0), (24.0, -8.0), (40.0, -12.0), (80.0, -20.0)):
            sd = S.synth_state_dict(0)
            w, b = sd['density_mlp.2.weight'].copy(), sd['density_mlp.2.bias'].copy()
            w[0] *= gain
            b[0] = b[0] * gain + shift
            sd['density_mlp.2.weight'], sd['density_mlp.2.bias'] = w, b
            net = harness.build_model(cfg, sd, dev).train()
            ops.RenderRays.apply = staticmethod(spy)
            try:
                net.forward_train_from_feats(feat.clone().requires_grad_(), voxel_semantics=sem, rays=rays_t.clone(), bda=bda)
            finally:
                ops.RenderRays.apply = real_apply
            stats.update(density_gain=gain, density_shift=shift)
            if gain > 1.0 and 0.25 <= stats['terminated_frac'] <= 0.8:
                break
            if gain == 1.0:
                transparent_stats = dict(stats)

        def step():
            net.zero_grad(set_to_none=True)
            f = feat.clone().requires_grad_()
            losses = net.forward_train_from_feats(f, voxel_semantics=sem, rays=rays_t.clone(), bda=bda)
            sum(losses.values()).backward()
            return losses
        if args == 'step':                                            # tools/diag_train_ops.py: just the closure
            return step
        net_t = harness.build_model(cfg, S.synth_state_dict(0), dev).train()      # the unscaled (transparent) scene of rounds 2-5, for comparison

        def step_t():
            net_t.zero_grad(set_to_none=True)
            losses = net_t.forward_train_from_feats(feat.clone().requires_grad_(), voxel_semantics=sem, rays=rays_t.clone(), bda=bda)
            sum(losses.values()).backward()
        for _ in range(2):
            step_t()
        torch.cuda.synchronize()
        per_t = []
        for _ in range(5):
            t0 = time.perf_counter()
            step_t()
            torch.cuda.synchronize()
            per_t.append((time.perf_counter() - t0) * 1e3)
        del net_t
        for _ in range(2):
            losses = step()
        torch.cuda.synchronize()
        n, per = 7, []
        for _ in range(n):
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            per.append((time.perf_counter() - t0) * 1e3)
        return {'ms': round(float(np.median(per)), 2), 'ms_min': round(min(per), 2), 'ms_max': round(max(per), 2), 'rays': R, 'samples_per_ray': 417,
                'what': 'final_conv + OccHead + attribute MLPs + NerfHead losses, forward + backward, 1 sample, eager; density_mlp output '
                        'rescaled so that rays terminate (terminated_frac measured on the step itself)',
                'terminated_frac': stats.get('terminated_frac'), 'scene': stats,
                'unscaled_scene': dict(transparent_stats, ms=round(float(np.median(per_t)), 2),
                                       note='no ray terminates: every sample of every ray is kept and goes through the backward'),
                'losses': {k: round(float(v.detach()), 4) for k, v in losses.items() if 'sup' not in k}}
    except Exception as e:                                            # noqa: BLE001  (an extra figure must not take the bench line down)
        return {'error': repr(e)[:300]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--settle-s', type=float, default=1.0,
                    help='untimed run-in before the W warm-up steps: the GPU needs a few hundred ms of load to leave '
                         'its idle clock state (measured: 304 us vs 278 us for the same conv launch)')
    ap.add_argument('--in-flight', type=int, default=2,
                    help='independent samples in flight per GPU (one hipGraph + HIP stream each); 1 = strictly serial')
    ap.add_argument('--config', default='C3', choices=['C3', 'C2', 'C5'],
                    help='C3 (headline) / C2 = the occupancy forward pass; C5 = the pre-train render head (extra, non-headline line)')
    ap.add_argument('--mode', default='replicas', choices=['replicas', 'sharded'])
    ap.add_argument('--no-graph', action='store_true', help='eager launches instead of hipGraph replay')
    ap.add_argument('--no-d2h', action='store_true', help='leave the occupancy grids on the device (no host payload)')
    ap.add_argument('--full', action='store_true',
                    help='also measure what the headline does not need: roofline, sustained MFMA rate, latency, same-input replay, '
                         'sharded phase times, the extra figures and the CPU baseline (C5: the forward, bf16, transparent, '
                         'reference-shape and pre-train figures)')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='with --full: skip the CPU baseline')
    ap.add_argument('--no-extra', action='store_true', help='with --full: skip the compact C2 / C5 figures appended after the timed region')
    ap.add_argument('--dump-outputs', metavar='DIR',
                    help='after the timed steps, write what the last one computed to DIR/<name>.npy (rank 0; see dump_outputs)')
    args = ap.parse_args()
    if args.steps < 1:
        ap.error('--steps must be at least 1')
    if args.config == 'C5':
        return bench_c5(args)

    rank = int(os.environ.get('RANK', 0))
    local_rank = int(os.environ.get('LOCAL_RANK', 0))
    world = int(os.environ.get('WORLD_SIZE', 1))
    if args.gpus > 1 and world == 1:
        raise SystemExit('launch with torch.distributed.run --nproc-per-node %d' % args.gpus)
    dist = None
    n_dev = torch.cuda.device_count()
    # one rank per GPU over RCCL.  Which device is mine?  Either every rank sees all GPUs of the node (torch.distributed.run's
    # default: take LOCAL_RANK) or the launcher pinned one device per rank through *_VISIBLE_DEVICES (then it is device 0).
    # Fewer GPUs than ranks WITHOUT such pinning only happens when the launch contract is exercised on a 1-GPU development
    # box: ranks then share a device and rendezvous over gloo (RCCL refuses two ranks on one GPU); such a timing means nothing.
    local_world = int(os.environ.get('LOCAL_WORLD_SIZE', world))
    pinned = n_dev < local_world and any(os.environ.get(k) for k in ('HIP_VISIBLE_DEVICES', 'ROCR_VISIBLE_DEVICES', 'CUDA_VISIBLE_DEVICES'))
    oversubscribed = n_dev < local_world and not pinned
    if n_dev == 0:
        raise SystemExit('bench.py: no GPU visible to rank %d (HIP_VISIBLE_DEVICES=%r)' % (rank, os.environ.get('HIP_VISIBLE_DEVICES')))
    dev_index = 0 if pinned else local_rank % n_dev
    torch.cuda.set_device(dev_index)
    dev = 'cuda:%d' % dev_index
    backend = None
    if world > 1 or args.mode == 'sharded':
        import datetime
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29533')
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')       # dmabuf IPC: RCCL's P2P buffers need it on this driver
        backend = 'gloo' if oversubscribed else 'nccl'                  # 'nccl' == RCCL on ROCm
        try:
            dist.init_process_group(backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=300))
            # first collective now, on the device: a broken xGMI / IPC set-up fails here with a message instead of hanging
            # the timed region
            probe = torch.ones(1, device='cpu' if oversubscribed else dev)
            dist.all_reduce(probe)
            assert int(probe.item()) == world
        except Exception as e:                                           # noqa: BLE001
            raise SystemExit('bench.py: %s process group of %d ranks failed on rank %d (device %s, MASTER_ADDR=%s:%s, '
                             'HSA_ENABLE_IPC_MODE_LEGACY=%s): %r' % (backend, world, rank, dev, os.environ['MASTER_ADDR'],
                                                                     os.environ['MASTER_PORT'],
                                                                     os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY'), e))

    sharded = args.mode == 'sharded'
    n_frames, n_steps_fc = (2, 6) if args.config == 'C3' else (1, 0)
    net, sd = build_net(dev, args.config)
    # sharded mode: every rank works on the SAME sample; replicas: each rank has its own
    frames, ego = make_inputs(dev, seed=0 if sharded else rank, n_frames=n_frames)

    phase_ms, phase_bytes = {}, {}
    ss = None
    ss_i = [0]
    if sharded and not args.no_graph:
        # round 6: the three compute phases between the two collectives as hipGraphs, ranges calibrated once + audited on the device
        from preworld_amd.pipeline import ShardedSample
        ss = ShardedSample(net, frames, ego, n_steps=n_steps_fc, gather_on_host=oversubscribed)
        ss_sets = [make_inputs(dev, seed=4000 + j, n_frames=n_frames) for j in range(3)]        # the same 3 samples on every rank, rotating

    def step():
        if ss is not None:
            ss_i[0] += 1
            return ss.run(*ss_sets[ss_i[0] % 3])
        if sharded:
            return harness.simple_test_sharded(net, frames, ego, n_steps=n_steps_fc, gather_on_host=oversubscribed)
        if args.config == 'C3':
            return net.simple_test_from_lift(frames, ego, n_steps=n_steps_fc)
        return net.simple_test_from_lift(frames)

    # eager warmup (also fills the packed-weight caches and sets kernel attributes)
    for _ in range(max(1, min(args.warmup, 3))):
        out = step()
    torch.cuda.synchronize()

    # run-in: clocks settled before anything is measured
    t_settle = time.perf_counter() + args.settle_s
    while time.perf_counter() < t_settle:
        step()
        torch.cuda.synchronize()

    # live per-kernel timing for the roofline object (eager, HIP events on the launch stream)
    roofline = None
    if rank == 0 and args.full:
        n_probe = 3
        # one stream for this pass: with the adjacent frame's lift forked onto a side stream the events around a launch
        # would also span whatever the other branch is running
        lift_streams = os.environ.get('PW_LIFT_STREAMS')
        os.environ['PW_LIFT_STREAMS'] = '0'
        try:
            with KernelProbe() as probe:
                for _ in range(n_probe):
                    if ss is not None:                       # (the captured phases cannot be probed launch by launch: the eager form)
                        harness.simple_test_sharded(net, frames, ego, n_steps=n_steps_fc, gather_on_host=oversubscribed)
                    else:
                        step()
        finally:
            if lift_streams is None:
                os.environ.pop('PW_LIFT_STREAMS')
            else:
                os.environ['PW_LIFT_STREAMS'] = lift_streams
        roofline = roofline_object(probe.summary(), n_probe)

    graph = None
    latency_ms = None
    d2h = not args.no_d2h
    if not args.no_graph and not sharded:
        from preworld_amd.pipeline import CapturedSample
        # M independent samples in flight, each a hipGraph over its own static buffers on its own HIP
        # stream: while one sample sits in a stage that cannot fill 256 CUs (the 8x100x100 / 4x50x50
        # encoder levels, the last partial wave of tiles of every launch, the latency-bound sort), the other
        # one's kernels take the idle CUs.  A step is still one sample; steps alternate between the streams.
        M = max(1, args.in_flight)
        caps = [CapturedSample(net, *make_inputs(dev, seed=rank * 8 + k, n_frames=n_frames), n_steps=n_steps_fc, d2h=d2h)
                for k in range(M)]
        streams = [torch.cuda.Stream() for _ in range(M)]
        graph = caps[0]
        out = graph.out
        # the timed stream: N_SETS distinct samples (none of them a calibration sample), resident in HBM, rotated through the captured
        # steps -- every step copies its sample's inputs (16 MB device-to-device) into the graph's static buffers and replays; N_SETS is
        # odd so that every captured step sees every sample.  The activation ranges of EVERY replay are audited on the device
        # (pw_rng_audit inside the graph), read once after the timed region.
        N_SETS = 5
        sets = [make_inputs(dev, seed=1000 + rank * 16 + j, n_frames=n_frames) for j in range(N_SETS)]

        def run_steps(n, rotate=True):
            res = None
            for i in range(n):
                with torch.cuda.stream(streams[i % M]):
                    if rotate:
                        res = caps[i % M].run(*sets[i % N_SETS])
                    else:
                        res = caps[i % M].replay()
            return res
    else:
        M = 1

        def run_steps(n, rotate=True):
            res = None
            for _ in range(n):
                res = step()
            return res

    t_settle = time.perf_counter() + args.settle_s
    while time.perf_counter() < t_settle:
        run_steps(M)
        torch.cuda.synchronize()
    if graph is not None and M > 1 and rank == 0 and args.full:        # single-sample latency, beside the throughput
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            caps[0].replay()
        torch.cuda.synchronize()
        latency_ms = (time.perf_counter() - t0) / 20 * 1e3
    run_steps(args.warmup)
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    ss_i[0] = 0                     # the run-in above is timed by the clock: restart the rotation so every run times the same samples
    t0 = time.perf_counter()
    last = run_steps(args.steps)
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], device='cpu' if oversubscribed else dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    # before anything else runs: the captured steps' outputs are static buffers that the next replay overwrites
    dumped = dump_outputs(last, args.dump_outputs) if args.dump_outputs and rank == 0 else None
    del last

    replay_only = None
    audit = None
    if graph is not None:
        bad = [c.bad_replays() for c in caps]                    # (replays outside their calibrated ranges, replays audited) per captured step
        audit = dict(replays_audited=int(sum(b[1] for b in bad)), recalibrations=int(sum(b[0] for b in bad)))
        if rank == 0 and world == 1 and args.full:
            # the round-3 figure beside it: the same captured steps replayed on their own calibration samples, no input copies
            run_steps(args.warmup, rotate=False)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            run_steps(args.steps, rotate=False)
            torch.cuda.synchronize()
            e1 = time.perf_counter() - t1
            replay_only = dict(samples_per_s=round(args.steps / e1, 3), ms_per_step=round(e1 / args.steps * 1e3, 4))

    if roofline is not None and roofline.get('bound') == 'mfma':
        # what the 1400 W socket cap leaves of the matrix pipe on this box: a bare fp16 MFMA stream on random operands
        # (pw_probe_mfma_f16, ~0.5 s), run AFTER the timed region so that it cannot warm the chip for it.  `peak` / `frac` stay the
        # data-sheet figures SURVEY 8(d) asks for.
        import ctypes
        from preworld_amd import _lib as L
        tf = ctypes.c_double(0.0)
        L.call('pw_probe_mfma_f16', 0.5, ctypes.byref(tf))
        roofline['sustained_mfma'] = dict(
            tflops=round(tf.value, 1), frac_of_it=round(roofline['executed_tflops'] / tf.value, 4),
            how='bare v_mfma_f32_32x32x16_f16 stream, random fp16 operands in registers, no memory traffic, one wave per SIMD, '
                '0.5 s on this box right after the timed region; frac_of_it = executed_tflops / tflops '
                '(profiles/r03_power_wall.txt: with real data the socket sits at its power cap and the clock follows)')

    if sharded and args.full:
        # per-phase times of this mode (HIP events, a few passes AFTER the timed region; rank 0's own phases), so that a multi-GPU
        # run explains itself: which part is divided by N, which is not, what the two all_gathers cost
        acc = {}
        for _ in range(5):
            t = {}
            if ss is not None:
                ss.run(*ss_sets[0], timings=t)
            else:
                harness.simple_test_sharded(net, frames, ego, n_steps=n_steps_fc, gather_on_host=oversubscribed, timings=t)
            for k, v in t.items():
                acc[k] = acc.get(k, 0.0) + v / 5
        phase_ms = {k: round(v, 4) for k, v in acc.items() if 'bytes' not in k}
        phase_bytes = {k: int(round(v)) for k, v in acc.items() if 'bytes' in k}

    # every replay of the timed region stayed inside its calibrated activation ranges (pipeline.CapturedSample.ranges_ok: the
    # exponent table + recorded maxima the replays delivered to pinned host memory)
    if ss is not None:
        bad = ss.bad_replays()
        audit = dict(replays_audited=int(bad[1]), recalibrations=int(bad[0]))
    ranges_ok = (audit['recalibrations'] == 0) if audit is not None and precision() == 'h2' else None
    ablation = os.environ.get('PW_BENCH_ABLATION') == '1'          # tools/ablate_step.sh: variant libraries that skip kernels; the line says so
    assert ranges_ok is not False or ablation, 'replays left their calibrated activation ranges: %s' % audit

    # sanity on the produced states (cheap, outside the timed region)
    key0 = 'semantic_occ_0s' if args.config == 'C3' else 'semantic_occ'
    occ0 = out[key0][0]
    assert tuple(occ0.shape) == (200, 200, 16) and occ0.dtype == torch.uint8
    n_states = sum(1 for k in out if k.startswith('semantic_occ'))
    if graph is not None and d2h:
        host = graph.host.numpy()
        assert host.shape == (2 * n_states, 200, 200, 16) and np.array_equal(host[graph.host_keys.index(key0)], occ0.cpu().numpy())

    if rank == 0:
        samples = args.steps * (1 if sharded else world)       # replicas: one sample per step per rank
        workload = ('C3: 7-state temporal, 6 cams, key+adjacent frame, 200x200x16, '
                    'LSS pooling x2 + pre_process x2 + CustomResNet3D + LSSFPN3D + final_conv '
                    '+ 6-step forecast + OccHead x7 -> 7 semantic + 7 geometric uint8 occupancy grids'
                    if args.config == 'C3' else
                    'C2: single frame (with_prev=False), 6 cams, 200x200x16, PreWorld detector, OccHead decode, 1 state')
        res = {
            'metric': 'samples/sec (6-cam frame -> 200x200x16 occ)',
            'value': round(samples / elapsed, 3),
            'unit': 'samples/s',
            'n_gpus': world,
            'rccl_world': world if backend == 'nccl' else None,          # ranks in the RCCL process group (None: single process / gloo)
            'steps': args.steps,
            'warmup': args.warmup,
            'ms_per_step': round(elapsed / args.steps * 1e3, 4),
            'higher_is_better': True,
            'scaling': 'strong' if sharded else 'weak',
            'vs_baseline': None,
            'dtype': 'f32' if precision() == 'f32' else 'f32 as hi+lo f16 (3 MFMA per product block, f32 accumulate)',
            'data': 'synthetic',
            'config': {
                'workload': workload,
                'states_per_sample': n_states,
                'launch': ('hipGraph replay, %d independent sample(s) in flight on %d HIP stream(s); %d distinct input sets rotate through '
                           'the captured steps, each step copies its inputs (16 MB D2D) into the static buffers inside the timed region'
                           % (M, M, N_SETS))
                if graph is not None else
                ('three hipGraphs per rank (own frames\' lift | encoder | forecast + decode of the owned states) around the two collectives '
                 '(pipeline.ShardedSample); 3 input sets rotate, each step copies its inputs into the static buffers') if ss is not None else 'eager',
                'replay_same_inputs': replay_only,
                'recalibrations': audit['recalibrations'] if audit else None,
                'replays_audited': audit['replays_audited'] if audit else None,
                'outputs': ('host: %d contiguous (X,Y,Z) uint8 grids per sample in pinned memory, one async D2H copy inside '
                            'the step (the reference payload, preworld_temporal_traj.py:311-366)' % (2 * n_states))
                if graph is not None and d2h else 'device (uint8 grids stay in HBM)',
                'single_sample_latency_ms': round(latency_ms, 4) if latency_ms else None,
                'sharded_phase_ms_rank0': phase_ms or None,
                'sharded_payload_bytes_rank0': phase_bytes or None,
                'parallelism': ('frames + states sharded over %d rank(s): per-frame features by all_gather (full rounds) / broadcast from '
                                'the owners (2 frames on 8 ranks), uint8 states by one all_gather (harness.simple_test_sharded)' % world)
                if sharded else
                'replicas x%d (independent samples, no data-path collective)' % world,
                'note': (' OVERSUBSCRIBED development run, %d GPU(s): not a measurement' % n_dev if oversubscribed else
                         'ABLATION RUN (PW_BENCH_ABLATION=1: a variant library skips kernels, outputs are garbage): timing experiment, not a '
                         'measurement' if ablation else None),
                'excluded': 'image backbone + DepthNet (stay on PyTorch, SURVEY 8a)',
                'activation_ranges': ('per-tensor power-of-two exponents calibrated on each captured step\'s warm-up sample (ops.RangeCtx); '
                                      'every replay re-records each tensor\'s maximum and a kernel inside the graph tallies the replays '
                                      'whose maxima left [2^6, 65504] stored units (pw_rng_audit): none of the %d replays since '
                                      'capture did = %s' % (audit['replays_audited'], ranges_ok)) if ranges_ok is not None else None,
                'arithmetic': ('PW_PRECISION=%s: ' % precision()) + (
                    'every value is fp32; conv / forecast products run as exact-fp32 MFMA (Winograd / direct kernels)'
                    if precision() == 'f32' else
                    'activations and weights are fp32 values stored as fp16 hi + fp16 lo (same 4 bytes); each product block is '
                    'hi.hi + lo_w.hi_x + hi_w.lo_x on v_mfma_f32_32x32x16_f16 with fp32 accumulation (K = 1728 dot product: '
                    '5.8e-6 max error vs 5.6e-6 for an fp32 fma chain, profiles/r02_hw_probes.md); pooling, FPN interpolation, '
                    'OccHead, softplus, argmax in fp32; roofline priced against the fp16 dense peak'),
            },
            'roofline': roofline,
        }
        if dumped is not None:
            res['dump_outputs'] = dict(dir=args.dump_outputs, arrays=dumped)
        if args.full and world == 1 and not sharded and args.config == 'C3' and not args.no_extra:
            res['extra'] = extra_figures(args, dev)
        if args.full and not args.no_cpu_baseline and world == 1 and not sharded:
            res['cpu_baseline'] = cpu_baseline(sd, step_gflop=(roofline or {}).get('step_gflop'))
        print(json.dumps(res))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
