"""Camera frames to network input at the real size (12 frames 900 x 1600 -> 512 x 1408: 6 cameras x key + adjacent), for the
test-time augmentation and for one drawn training augmentation (np.random.seed(--seed), the released ranges), three legs in
one process:

  (a) device path: the 12 uint8 frames copied from pinned host memory (51.8 MB) + pw_image_prep;
  (b) the kernel alone on frames already resident, with the bytes it has to move (source rows and columns the crop keeps are
      not counted apart: all of src once, out once, canvas once) per second beside the 8 TB/s HBM peak DESIGN.md uses;
  (c) host path, as the reference does it: PIL resize / crop / flip / rotate per frame, the normalise in numpy float32 (mmcv's
      imnormalize is not installable here), and the float32 result (103.8 MB) copied from pinned memory to the device.
      Skipped, and reported as null, where PIL does not import.
  (d) training column only: what a training step pays, where every sample draws a new augmentation -- the draw, a NEW
      ops.image_prep_plan (coefficient tables for the new sizes, parameters, two small copies to the device), then (a).  The
      table cache is left as the run fills it, as in training; legs (a) and (b) of that column re-use one plan.

Timed wall-clock around `--iters` back-to-back calls ((c): `--host-iters`), synchronised at both ends; the legs are interleaved
over `--rounds` rounds and the median round is reported with min / max.  Prints one JSON line.

    python tools/bench_image_prep.py [--iters 1000] [--host-iters 2] [--plan-iters 50] [--rounds 5] [--seed 0]"""
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
import _image_prep_np as IP  # noqa: E402
from preworld_amd import ops, transforms  # noqa: E402

HBM_PEAK = 8.0e12
DATA_CONFIG = dict(cams=IP.CAM_NAMES, Ncams=6, input_size=(512, 1408), resize=(-0.06, 0.11), rot=(-5.4, 5.4), flip=True,
                   crop_h=(0.0, 0.0), resize_test=0.00)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=1000)
    ap.add_argument('--host-iters', type=int, default=2)
    ap.add_argument('--plan-iters', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--seed', type=int, default=0)
    a = ap.parse_args()
    dev, H, W, (fH, fW) = 'cuda:0', 900, 1600, DATA_CONFIG['input_size']
    try:
        from PIL import Image
    except ImportError:
        Image = None
    frames = IP.synthetic_frames(4, 12, H, W)
    pinned = torch.from_numpy(np.stack(frames)).pin_memory()
    resident = pinned.to(dev)
    out = torch.empty(12, 3, fH, fW, device=dev)
    canvas = torch.empty(12, fH, fW, 3, dtype=torch.uint8, device=dev)
    host_out = torch.empty(12, 3, fH, fW).pin_memory()
    np.random.seed(a.seed)
    augs = {}
    for name, is_train in (('test_time', False), ('train_draw', True)):
        t = transforms.PrepareImageInputs(DATA_CONFIG, is_train=is_train, sequential=True)
        augs[name] = [t.sample_augmentation(H, W)[1:] for _ in range(6)]
    trainer = t
    result = dict(bench='image_prep', frames=12, src=[H, W], input_size=[fH, fW], iters=a.iters, host_iters=a.host_iters, plan_iters=a.plan_iters, rounds=a.rounds,
                  h2d_bytes=dict(device_path=pinned.numel(), host_path=host_out.numel() * 4), hbm_peak_bytes_per_s=HBM_PEAK,
                  pil=None if Image is None else __import__('PIL').__version__, host_cpus=len(os.sched_getaffinity(0)))
    for name, six in augs.items():
        per_image = [six[i // 2] for i in range(12)]
        plan = ops.image_prep_plan((H, W), (fH, fW), per_image, device=dev)

        def leg_a():
            ops.prepare_images(pinned.to(dev, non_blocking=True), plan, out=out, canvas=canvas)

        def leg_b():
            ops.prepare_images(resident, plan, out=out, canvas=canvas)

        def leg_c():
            o = host_out.numpy()
            for i, (f, (dims, crop, flip, rot)) in enumerate(zip(frames, per_image)):
                im = Image.fromarray(f).resize(dims).crop(crop)
                if flip:
                    im = im.transpose(method=Image.FLIP_LEFT_RIGHT)
                px = np.array(im.rotate(rot))
                o[i] = np.moveaxis((px[..., ::-1].astype(np.float32) - IP.MEAN32) * IP.STDINV32, -1, 0)
            return host_out.to(dev, non_blocking=True)
        def leg_d():
            drawn = [trainer.sample_augmentation(H, W)[1:] for _ in range(6)]
            fresh = ops.image_prep_plan((H, W), (fH, fW), [drawn[i // 2] for i in range(12)], device=dev)
            ops.prepare_images(pinned.to(dev, non_blocking=True), fresh, out=out, canvas=canvas)
        legs = [('a_copy_plus_kernel', leg_a, a.iters), ('b_kernel_alone', leg_b, a.iters)]
        if name == 'train_draw':
            legs.append(('d_draw_plan_copy_kernel', leg_d, a.plan_iters))
        if Image is not None:
            legs.insert(2, ('c_host_pil_numpy_copy', leg_c, a.host_iters))
            want = leg_c()
            leg_b()
            assert torch.equal(want, out), 'device and host paths differ'
        for _, fn, _ in legs[:2]:
            for _ in range(5):
                fn()
        times = {n: [] for n, _, _ in legs}
        for _ in range(a.rounds):
            for n, fn, iters in legs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(iters):
                    fn()
                torch.cuda.synchronize()
                times[n].append((time.perf_counter() - t0) / iters * 1e3)
        r = dict(launches=plan.launches, augs=[[list(x[0]), list(x[1]), int(x[2]), round(float(x[3]), 3)] for x in six])
        for n, _, _ in legs:
            t = sorted(times[n])
            r[n] = dict(ms_median=round(t[len(t) // 2], 4), ms_min=round(t[0], 4), ms_max=round(t[-1], 4))
        moved = resident.numel() + out.numel() * 4 + canvas.numel() + (2 * canvas.numel() if plan.any_rot else 0)
        r['b_kernel_alone'].update(bytes=moved, bytes_per_s=round(moved / (r['b_kernel_alone']['ms_median'] * 1e-3), 0),
                                   share_of_hbm_peak=round(moved / (r['b_kernel_alone']['ms_median'] * 1e-3) / HBM_PEAK, 4))
        if Image is None:
            r['c_host_pil_numpy_copy'] = None
        result[name] = r
    print(json.dumps(result), flush=True)


if __name__ == '__main__':
    main()
