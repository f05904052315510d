"""Throughput of streaming evaluation (pipeline.SampleStream) at C3 against bench.py's raw captured loop, in one process.

    python tools/bench_stream.py [--in-flight 2] [--samples 600] [--warmup 20] [--eval-samples 100] [--fscore]

Prints one JSON line with samples/s for
  raw        bench.py's timed loop restated: M CapturedSamples (host payload in the graph, as bench.py's default), rotating
             resident input sets, each replayed on its own stream, nothing checked, nothing scored
  score      SampleStream(payload=False, score=...): every replay range-checked, scored in the graph, no D2H
  payload    SampleStream(payload=True, score=...): the same plus the 14-grid host payload per sample
  evaluate   harness.evaluate (eager, one sample at a time, host-side stacking) on the same samples
raw, score and payload alternate (twice each, about 1.5 s per window at C3) so drift shows; the ratios use the means.
--fscore measures instead, alternated three times each:
  score      as above
  fscore     the same stream with score['fscore'] (the camera mask): one more pw_occ_fscore launch in every graph and one
             pw_occ_fscore_accumulate per sample
and prints their ratio and the F-scores of the fscore stream.
--distributed runs under torch.distributed.run (one process per GPU, RCCL):

    python -m torch.distributed.run --nproc-per-node N tools/bench_stream.py --distributed [--in-flight 2] [--samples 600] [--fscore]

and times harness.evaluate_stream(distributed=True) over a split of --samples samples (rank r scores every W-th one), twice after
one warm-up call.  Rank 0 prints one JSON line: per rank its scored samples/s (its samples over its stream phase, the slots'
capture excluded), the aggregate (the split over the slowest rank's stream phase, and over the whole call incl. capture) and the
seconds from the rank's last sample to the reduced report.  --fscore adds the F-score (deferred rows, folded after the reduction).
Inputs, GT grids and masks are resident in HBM (N_SETS distinct samples from fixed seeds); evaluate gets the GT as numpy, as
its callers pass it."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from preworld_amd import harness  # noqa: E402
from preworld_amd.pipeline import CapturedSample, SampleStream  # noqa: E402

N_SETS = 5
HZ = (0, 2, 4, 6)


def make_samples(dev, n_frames):
    rs = np.random.RandomState(2024)
    out = []
    for j in range(N_SETS):
        frames, ego = bench.make_inputs(dev, seed=1000 + j, n_frames=n_frames)
        gt = {h: rs.randint(0, 18, size=(200, 200, 16)).astype(np.uint8) for h in HZ}
        mask = rs.rand(200, 200, 16) < 0.7
        out.append(dict(frames=frames, ego=ego, gt_np=gt, mask_np=mask,
                        gt={h: torch.from_numpy(g).to(dev) for h, g in gt.items()},
                        mask_camera=torch.from_numpy(mask).to(dev)))
    return out


def time_raw(caps, streams, sets, n):
    M = len(caps)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        with torch.cuda.stream(streams[i % M]):
            caps[i % M].run(sets[i % N_SETS]['frames'], sets[i % N_SETS]['ego'])
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def time_stream(st, sets, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    k = 0
    for _ in st.run(sets[i % N_SETS] for i in range(n)):
        k += 1
    torch.cuda.synchronize()
    assert k == n
    return n / (time.perf_counter() - t0)


def bench_fscore(net, sets, score, M, args):
    """score-only stream against the same stream with the F-score, alternated"""
    fs = dict(score, fscore=dict(threshold_acc=0.6, threshold_complete=0.6, voxel_size=[0.4, 0.4, 0.4], void=[17, 255],
                                 mask='camera'))
    st_b = SampleStream(net, sets[0]['frames'], sets[0]['ego'], in_flight=M, payload=False, score=score)
    st_f = SampleStream(net, sets[0]['frames'], sets[0]['ego'], in_flight=M, payload=False, score=fs)
    time_stream(st_b, sets, args.warmup)
    time_stream(st_f, sets, args.warmup)
    sc, sf = [], []
    for _ in range(3):
        sc.append(time_stream(st_b, sets, args.samples))
        sf.append(time_stream(st_f, sets, args.samples))
    b, f = float(np.mean(sc)), float(np.mean(sf))
    res = dict(config='C3', in_flight=M, samples_timed=args.samples, score_samples_per_s=[round(v, 1) for v in sc],
               fscore_samples_per_s=[round(v, 1) for v in sf], ratio_fscore_over_score=round(f / b, 4),
               fscore={h: round(m.tot_f1_mean / m.cnt, 6) for h, m in st_f.fscore.items()},
               fscore_cnt=st_f.fscore[HZ[0]].cnt, miou_cnt=st_f.metric.cnt,
               counters={name: dict(replays=st.replays, recalibrations=st.recalibrations) for name, st in (('score', st_b),
                                                                                                        ('fscore', st_f))},
               gt_resident=True, torch=torch.__version__, pw_precision=os.environ.get('PW_PRECISION', 'h2'))
    st_b.close()
    st_f.close()
    print(json.dumps(res), flush=True)


def bench_distributed(args):
    """harness.evaluate_stream(distributed=True) under torch.distributed.run"""
    import torch.distributed as dist
    local = int(os.environ.get('LOCAL_RANK', '0'))
    dev = 'cuda:%d' % local
    torch.cuda.set_device(local)
    dist.init_process_group('nccl', device_id=torch.device(dev))
    try:
        rank, world = dist.get_rank(), dist.get_world_size()
        net, _ = bench.build_net(dev, 'C3')
        sets = make_samples(dev, 2)
        fs = dict(mask='camera') if args.fscore else None

        def split(n):
            return [dict(frames=s['frames'], ego=s['ego'], gt=s['gt'], mask_camera=s['mask_camera'])
                    for s in (sets[i % N_SETS] for i in range(n))]
        harness.evaluate_stream(net, split(max(args.warmup, world)), in_flight=args.in_flight, fscore=fs, distributed=True)
        runs = []
        for _ in range(2):
            st = {}
            dist.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rep, _, metric = harness.evaluate_stream(net, split(args.samples), in_flight=args.in_flight, fscore=fs,
                                                     distributed=True, stats=st)
            st['call_s'] = time.perf_counter() - t0
            per = [None] * world
            dist.all_gather_object(per, st)
            runs.append(dict(
                per_rank_samples_per_s=[round(p['samples'] / p['stream_s'], 1) if p['samples'] else None for p in per],
                per_rank_samples=[p['samples'] for p in per],
                aggregate_samples_per_s=round(args.samples / max(p['stream_s'] for p in per), 1),
                aggregate_incl_capture_samples_per_s=round(args.samples / max(p['call_s'] for p in per), 1),
                last_sample_to_report_ms=[round(1e3 * p['reduce_s'], 2) for p in per],
                capture_s=[round(p['capture_s'], 3) for p in per],
                recalibrations=st['all']['recalibrations']))
        if rank == 0:
            res = dict(config='C3', mode='evaluate_stream(distributed=True)', world=world, backend='nccl', in_flight=args.in_flight,
                       samples=args.samples, fscore=bool(args.fscore), runs=runs, miou=rep, cnt=metric.cnt,
                       gt_resident=True, torch=torch.__version__, pw_precision=os.environ.get('PW_PRECISION', 'h2'))
            if fs is not None:
                res['fscore_values'] = {h: round(v, 6) for h, v in rep['fscore'].items()}
            print(json.dumps(res), flush=True)
    finally:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--in-flight', type=int, default=2)
    ap.add_argument('--samples', type=int, default=600)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--eval-samples', type=int, default=100)
    ap.add_argument('--fscore', action='store_true', help='score-only stream with and without the F-score (nothing else); '
                    'with --distributed: score the F-score too')
    ap.add_argument('--distributed', action='store_true', help='evaluate_stream(distributed=True), under torch.distributed.run')
    args = ap.parse_args()
    if args.distributed:
        bench_distributed(args)
        return
    dev = 'cuda:0'
    M = max(1, args.in_flight)
    net, _ = bench.build_net(dev, 'C3')
    n_frames = 2
    sets = make_samples(dev, n_frames)
    score = dict(horizons=HZ, n_cl=18, mask='camera')
    if args.fscore:
        bench_fscore(net, sets, score, M, args)
        return

    caps = [CapturedSample(net, *bench.make_inputs(dev, seed=k, n_frames=n_frames), n_steps=6, d2h=True) for k in range(M)]
    streams = [torch.cuda.Stream() for _ in range(M)]
    st_b = SampleStream(net, sets[0]['frames'], sets[0]['ego'], in_flight=M, payload=False, score=score)
    st_c = SampleStream(net, sets[0]['frames'], sets[0]['ego'], in_flight=M, payload=True, score=score)
    time_raw(caps, streams, sets, args.warmup)
    time_stream(st_b, sets, args.warmup)
    time_stream(st_c, sets, args.warmup)
    raw, sc, pay = [], [], []
    for _ in range(2):                                  # alternating, so that drift of the machine shows in both
        raw.append(time_raw(caps, streams, sets, args.samples))
        sc.append(time_stream(st_b, sets, args.samples))
        pay.append(time_stream(st_c, sets, args.samples))
    bad = [c.bad_replays() for c in caps]
    del caps
    res = dict(config='C3', in_flight=M, samples_timed=args.samples, raw_samples_per_s=[round(v, 1) for v in raw],
               score_samples_per_s=[round(v, 1) for v in sc], payload_samples_per_s=[round(v, 1) for v in pay])
    counters = {name: dict(replays=st.replays, recalibrations=st.recalibrations) for name, st in (('score', st_b), ('payload', st_c))}
    st_b.close()
    st_c.close()

    ev_samples = [dict(frames=s['frames'], ego=s['ego'], gt=s['gt_np'], mask_camera=s['mask_np'])
                  for s in (sets[i % N_SETS] for i in range(args.eval_samples))]
    harness.evaluate(net, ev_samples[:2], dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    harness.evaluate(net, ev_samples, dev)
    torch.cuda.synchronize()
    ev = args.eval_samples / (time.perf_counter() - t0)

    a, b, c = float(np.mean(raw)), float(np.mean(sc)), float(np.mean(pay))
    res.update(evaluate_samples_per_s=round(ev, 1), evaluate_samples_timed=args.eval_samples,
               ratio_score_over_raw=round(b / a, 4), ratio_payload_over_raw=round(c / a, 4),
               raw_bad_replays=[list(x) for x in bad], counters=counters,
               gt_resident=True, torch=torch.__version__, pw_precision=os.environ.get('PW_PRECISION', 'h2'))
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
