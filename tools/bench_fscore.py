"""pw_occ_fscore alone: one launch scoring 4 full-size (200, 200, 16) horizons with camera masks, repeated, for
`rocprofv3 --kernel-trace --stats -- python tools/bench_fscore.py` (kernel time) -- and timed with HIP events here (launch
included).  Prints one JSON line: microseconds per launch and the bytes the launch reads.

    python tools/bench_fscore.py [--iters 2000] [--horizons 4]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from preworld_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=2000)
    ap.add_argument('--horizons', type=int, default=4)
    a = ap.parse_args()
    dev, H, shape = 'cuda:0', a.horizons, (200, 200, 16)
    rs = np.random.RandomState(5)

    def grid():
        g = np.full(shape, 17, np.uint8)
        occ = rs.rand(*shape) < 0.3
        g[occ] = rs.randint(0, 17, int(occ.sum()))
        return torch.from_numpy(g).to(dev)
    preds = [grid() for _ in range(H)]
    gts = [grid() for _ in range(H)]
    masks = [torch.from_numpy(rs.rand(*shape) < 0.7).to(dev) for _ in range(H)]
    table = torch.zeros(H, 4, dtype=torch.int64, device=dev)
    for _ in range(20):
        ops.occ_fscore(preds, gts, masks, table)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        ops.occ_fscore(preds, gts, masks, table)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / a.iters
    nbytes = 3 * H * int(np.prod(shape))
    print(json.dumps(dict(kernel='pw_occ_fscore', horizons=H, shape=shape, masked=True, iters=a.iters,
                          us_per_launch_events=round(us, 2), bytes_read=nbytes,
                          gb_per_s_events=round(nbytes / us / 1e3, 1))), flush=True)


if __name__ == '__main__':
    main()
