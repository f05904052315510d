"""How long does a dense camera view take?  pw_render_views against the sparse route to the same pixels -- ops.pts2ray for every
pixel + ops.render_rays without debug outputs + argmax, on one stream -- in one process on one GPU, for the mixed scene and for
synth.render_grids, at 6 x 450 x 800 (stride 2) and 6 x 900 x 1600.  Both routes must produce the same class map (up to near-ties
of the rendered sums) before a time is reported.  The two routes alternate run for run; median of `--repeats` timed runs each
after `--warmup` untimed ones, device events.

    python tools/bench_render_views.py [--repeats 5] [--warmup 2] [--sizes 2 1] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from preworld_amd import modules as M, ops, synth as S  # noqa: E402

DEV = 'cuda:0'
H, W = 900, 1600


def timed_ab(fa, fb, warmup, repeats):
    """A/B on one box: the two routes ALTERNATE, run for run, with the same number of untimed and timed runs each; device events
    around each run.  Returns (median a, runs a, last result a, median b, runs b, last result b)."""
    ms = ([], [])
    outs = [None, None]
    for r in range(warmup + repeats):
        for k, fn in enumerate((fa, fb)):
            outs[k] = None                                      # free the previous run's outputs outside the timed window
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            outs[k] = fn()
            b.record()
            b.synchronize()
            if r >= warmup:
                ms[k].append(a.elapsed_time(b))
    return float(np.median(ms[0])), ms[0], outs[0], float(np.median(ms[1])), ms[1], outs[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--sizes', type=int, nargs='+', default=[2, 1], help='strides over the 900 x 1600 images')
    ap.add_argument('--scenes', nargs='+', default=['mixed', 'soft'])
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)      # noqa: E731
    head = M.NerfHead(point_cloud_range=[-40, -40, -1, 40, 40, 5.4], voxel_size=0.4, scene_center=[0, 0, 2.2], radius=39).to(DEV)
    rig = S.synthetic_rig(6)
    K, c2w = T(rig['intrin'][0]), T(rig['sensor2ego'][0])
    consts, t = head.consts(torch.eye(3)), head.t_table(DEV)
    rows = []
    for scene in a.scenes:
        grids = S.render_grids_mixed(61) if scene == 'mixed' else S.render_grids(31)
        grid = M.pack_attribute_grid(*[T(g) for g in grids])
        for stride in a.sizes:
            h, w = -(-H // stride), -(-W // stride)
            jj, ii = torch.meshgrid(torch.arange(w, device=DEV), torch.arange(h, device=DEV), indexing='xy')
            coor = torch.stack([jj * stride, ii * stride], -1).reshape(-1, 2).float().contiguous()
            z1, z3 = torch.zeros(h * w, device=DEV), torch.zeros(h * w, 3, device=DEV)

            def dense():
                return ops.render_views(grid, K, c2w, (h, w), consts, t, stride=stride, outputs=('depth', 'cls', 'color'))

            def sparse():
                res = []                                        # per view: (cls, the sums the check below reads); nothing is copied here
                for v in range(6):
                    rays = ops.pts2ray(coor, z1, z1, z3, c2w[v], K[v])
                    out = ops.render_rays(rays[:, 4:7].contiguous(), rays[:, 7:10].contiguous(), t, grid, consts)
                    res.append((out['semantic'].argmax(-1), out['semantic']))
                return res

            d_ms, d_all, d_out, s_ms, s_all, s_out = timed_ab(dense, sparse, a.warmup, a.repeats)
            s_cls = torch.stack([r[0] for r in s_out]).view(6, h, w)
            s_sem = torch.stack([r[1] for r in s_out]).view(6, h, w, 17)
            last = ops.render_views(grid, K, c2w, (h, w), consts, t, stride=stride, outputs=('alphainv_last',))['alphainv_last']
            diff = d_out['cls'].long() != s_cls
            top2 = s_sem.topk(2, -1).values
            near = (top2[..., 0] - top2[..., 1]) <= 2 * (2e-4 * top2[..., 0].abs() + 2e-4)      # the sparse-vs-dense bound on both contenders
            bad = int((diff & ~near).sum())
            assert bad == 0, '%d pixels of the class maps differ away from a near-tie' % bad
            row = dict(scene=scene, stride=stride, pixels=6 * h * w, render_views_ms=d_ms, sparse_route_ms=s_ms, ratio=s_ms / d_ms,
                       render_views_runs=d_all, sparse_route_runs=s_all, cls_differ=int(diff.sum()), cls_differ_off_tie=bad,
                       terminated=float((last < 1e-3).float().mean()))
            rows.append(row)
            print('%-5s 6 x %4d x %4d: pw_render_views %8.2f ms   pts2ray + render_rays + argmax %9.2f ms   ratio %6.1fx   '
                  '(class maps: %d pixels differ, all near-ties; %.0f %% of the rays terminate)'
                  % (scene, h, w, d_ms, s_ms, s_ms / d_ms, int(diff.sum()), 100 * row['terminated']), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
