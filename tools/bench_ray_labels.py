"""The ray table of one pre-train sample (7 frames x 6 cameras of 900 x 1600, sweeps of ~34 720 points), two ways, in one process:

  (i)  the parent commit's means: stage A and the label gathers on the host (the numpy restatement tests/_ray_labels_np.py:
       projection of every sweep into its six cameras, seg map, colour gather), the per-camera lists uploaded, then
       rays.generate_rays -- one pw_pts2ray, one pw_class_count and one pw_wrs_weights launch per camera plus the concatenations;
  (ii) the new path: the sweeps and their lidarseg bytes uploaded from pinned memory (the frames are already on the device, as
       PrepareImageInputs4DTraj stages them), then ops.ray_table + ops.ray_table_weights at a fixed capacity: no host
       synchronisation inside a step.

Each leg is timed wall-clock around its back-to-back steps with a device synchronise at both ends; the legs alternate over
`--rounds` rounds and the median round is reported with the spread.  The tables of the two legs are compared first (columns 0-3
and 13-15 bit-equal, 4-12 to rtol 2e-6 / atol 1e-6).  Prints one JSON line: times, kernel launches per step, scratch bytes.

`--md PATH` also writes the figures as the note kept in profiles/ray_labels.md.

    python tools/bench_ray_labels.py [--iters 200] [--host-iters 2] [--rounds 5] [--md profiles/ray_labels.md]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import _ray_labels_np as RN  # noqa: E402
from preworld_amd import ops, rays  # noqa: E402

DYN = [0, 1, 3, 4, 5, 7, 9, 10]


def note(o):
    """the figures of one run as profiles/ray_labels.md"""
    new, par, host = o['new_ray_table'], o['parent_host_numpy_plus_generate_rays'], o['parent_host_part_alone']
    V = o['frames'] * o['cameras']
    row = '| %s | %.4f | %.4f | %.4f | %s | %s |\n'
    return ''.join([
        '# Ray supervision from the sweep: one pre-train sample\'s ray table two ways\n\n',
        '`python tools/bench_ray_labels.py --iters %d --host-iters %d --rounds %d --md profiles/ray_labels.md`, one MI355X, one process.\n' % (
            o['iters'], o['host_iters'], o['rounds']),
        '%d frames x %d cameras of %d x %d, synthetic sweeps of %d .. %d points with lidarseg bytes, %d rows in the table (capacity %d).\n' % (
            o['frames'], o['cameras'], o['image'][0], o['image'][1], min(o['points']), max(o['points']), o['rows'], o['capacity']),
        'Wall clock between two device synchronisations around the back-to-back steps of a leg, the legs alternating over the rounds;\n',
        'median round with min / max.  Before timing, the two tables were compared: columns 0-3 and 13-15 bit-equal, 4-12 within\n',
        'rtol 2e-6 / atol 1e-6, weights within rtol 1e-5.\n\n',
        '| leg | ms / sample (median) | min | max | kernel launches per sample | bytes host -> device |\n|---|---|---|---|---|---|\n',
        row % ('parent commit\'s means: numpy restatement of stage A + label gathers on the host, lists uploaded, `rays.generate_rays`',
               par['ms_median'], par['ms_min'], par['ms_max'], o['launches']['parent'], '{:,}'.format(o['h2d_bytes']['parent']).replace(',', ' ')),
        row % ('... its host part alone (no device work)', host['ms_median'], host['ms_min'], host['ms_max'], '0', '0'),
        row % ('new: sweeps + lidarseg bytes uploaded from pinned memory, `ops.ray_table` + `ops.ray_table_weights` at a fixed capacity '
               '(frames already on the device, no host synchronisation)', new['ms_median'], new['ms_min'], new['ms_max'],
               o['launches']['new_ray_table'], '{:,}'.format(o['h2d_bytes']['new_ray_table']).replace(',', ' ')),
        '\nThe new leg takes %.0f x less time than the parent\'s in the same run; %.1f %% of the parent\'s time is its host part.\n' % (
            par['ms_median'] / new['ms_median'], 100.0 * host['ms_median'] / par['ms_median']),
        'Each parent step ran %d times per round, each new step %d times.\n\n' % (o['host_iters'], o['iters']),
        '*Scratch.*  %s bytes of device scratch per sample (%d views, Pmax = %d): the owner table, 8 bytes x the power of two >= 2 V Pmax\n' % (
            '{:,}'.format(o['scratch_bytes']).replace(',', ' '), V, max(o['points'])),
        'entries, plus the block bases and view offsets.  A dense `int32[V][H][W]` owner table would take %s bytes, %.1f x as much.\n' % (
            '{:,}'.format(o['dense_owner_table_bytes']).replace(',', ' '), o['dense_owner_table_bytes'] / o['scratch_bytes']),
        'Stage A alone (`ops.sweep_pixel_labels`) allocates no owner table.\n\n',
        '*Not measured.*  Per-kernel times (no rocprofv3 run was made), the lists mode, and `bench.py --config C5`: its pre-train step\n',
        'starts from a prepared ray table and does not run this path.\n'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--host-iters', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--md', default=None)
    a = ap.parse_args()
    dev, T, N, H, W = 'cuda:0', 7, 6, 900, 1600
    lengths = [34720 - 37 * t for t in range(T)]
    S = RN.synthetic_sample(51, T=T, N=N, P=34720, H=H, W=W, focal=1266.0, lengths=lengths)
    V = T * N
    c2w_np, K_np = RN.camera_tables(S['infos'], S['cam_names'])
    frame_ids = [t for t in range(T) for _ in range(N)]
    time_ids = {t: list(range(t * N, (t + 1) * N)) for t in range(T)}
    frames = torch.from_numpy(S['frames']).to(dev)
    c2w, K = torch.from_numpy(c2w_np).to(dev), torch.from_numpy(K_np).to(dev)
    dyn = torch.tensor(DYN, dtype=torch.int32, device=dev)

    # ---- (i) the parent commit's means
    def host_lists():
        dl, sl = RN.stage_a(S['points'], S['labels'], RN.LUT, S['poses'], N, H, W)
        return [RN.view_labels(dl[v], sl[v], S['frames'][v], H, W, fancy=True) for v in range(V)]

    def parent():
        per_view = host_lists()
        cols = [[torch.from_numpy(np.ascontiguousarray(x[k])).to(dev, non_blocking=True) for x in per_view] for k in range(4)]
        return rays.generate_rays(cols[0], cols[1], cols[2], cols[3], c2w, K, max_ray_nums=0, time_ids=time_ids, dynamic_class=dyn,
                                  return_weights=True)[:2]

    # ---- (ii) the new path
    Pmax = max(lengths)
    pts_h = torch.zeros(T, Pmax, 5).pin_memory()
    lab_h = torch.zeros(T, Pmax, dtype=torch.uint8).pin_memory()
    for t in range(T):
        pts_h[t, :lengths[t]] = torch.from_numpy(S['points'][t])
        lab_h[t, :lengths[t]] = torch.from_numpy(S['labels'][t])
    n_h = torch.tensor(lengths, dtype=torch.int32).pin_memory()
    pose = torch.from_numpy(S['poses']).to(dev)
    lut = torch.from_numpy(RN.LUT).to(dev)
    fid = torch.tensor(frame_ids, dtype=torch.int32, device=dev)
    ref_table, ref_w = parent()
    R = int(ref_table.shape[0])
    cap = -(-R // 4096) * 4096 + 4096

    def new():
        sw = ops.RaySweeps(pts_h.to(dev, non_blocking=True), lab_h.to(dev, non_blocking=True), pose, lut, n_h.to(dev, non_blocking=True))
        table, view_off, counts = ops.ray_table(c2w, K, frames, sweeps=sw, capacity=cap)
        return table, ops.ray_table_weights(table, view_off, fid, dyn, counts=counts), view_off

    table, w, view_off = new()
    assert int(view_off[-1]) == R, (int(view_off[-1]), R)
    a_, b_ = table[:R].cpu().numpy(), ref_table.cpu().numpy()
    assert np.array_equal(a_[:, :4].view(np.uint32), b_[:, :4].view(np.uint32)) and np.array_equal(a_[:, 13:].view(np.uint32), b_[:, 13:].view(np.uint32))
    np.testing.assert_allclose(a_[:, 4:13], b_[:, 4:13], rtol=2e-6, atol=1e-6)
    np.testing.assert_allclose(w[:R].cpu().numpy(), ref_w.cpu().numpy(), rtol=1e-5)
    for _ in range(10):
        new()
    legs = [('parent_host_numpy_plus_generate_rays', parent, a.host_iters), ('new_ray_table', new, a.iters)]
    times = {name: [] for name, _, _ in legs}
    host_only = []
    for _ in range(a.rounds):
        for name, fn, iters in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / iters * 1e3)
        t0 = time.perf_counter()
        host_lists()
        host_only.append((time.perf_counter() - t0) * 1e3)
    out = dict(bench='ray_labels', frames=T, cameras=N, image=[H, W], points=lengths, rows=R, capacity=cap, iters=a.iters,
               host_iters=a.host_iters, rounds=a.rounds, scratch_bytes=ops.ray_scratch_bytes(T, N, Pmax),
               dense_owner_table_bytes=4 * V * H * W,
               launches=dict(new_ray_table='5 of this library (fill, project + count, scan, emit, weights) + 1 torch fill (class counts)',
                             parent='%d of this library (pw_pts2ray, pw_class_count, pw_wrs_weights per view) + 2 torch.cat + the balance-weight ops' % (3 * V)),
               h2d_bytes=dict(new_ray_table=pts_h.numel() * 4 + lab_h.numel() + n_h.numel() * 4, parent=R * (2 + 1 + 1 + 3) * 4))
    for name, _, _ in legs:
        t = sorted(times[name])
        out[name] = dict(ms_median=round(t[len(t) // 2], 4), ms_min=round(t[0], 4), ms_max=round(t[-1], 4))
    t = sorted(host_only)
    out['parent_host_part_alone'] = dict(ms_median=round(t[len(t) // 2], 4), ms_min=round(t[0], 4), ms_max=round(t[-1], 4))
    print(json.dumps(out), flush=True)
    if a.md:
        with open(a.md, 'w') as f:
            f.write(note(out))


if __name__ == '__main__':
    main()
