"""Render one synthetic sample's seven predicted states into a six-camera rig and write one .npy per state and output.

    python tools/render_forecast.py [--out views] [--stride 4] [--pretrain] [--image 900 1600]

The model is the synthetic-weight PreWorld4DTraj of the benches (harness.model_cfg, synth.synth_state_dict) on the full
200 x 200 x 16 grid; --pretrain switches to the attribute-MLP branch (depth / cls / color through the soft renderer), the
default post-finetune model renders its uint8 grids in label mode (depth / cls).  Files: <out>/<output>_<k>s.npy, arrays
(6, h, w[, 3]).  No image library is needed: np.load the arrays and view them with whatever is at hand."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from preworld_amd import harness, synth as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='views')
    ap.add_argument('--stride', type=int, default=4)
    ap.add_argument('--pretrain', action='store_true')
    ap.add_argument('--image', type=int, nargs=2, default=[900, 1600])
    a = ap.parse_args()
    dev = 'cuda:0'
    net = harness.build_model(harness.model_cfg(if_post_finetune=not a.pretrain), S.synth_state_dict(0), dev)
    frames = harness.lifted_frames(1, 6, dev)
    ego = torch.from_numpy(S.ego_state(1)).to(dev)
    rig = S.synthetic_rig(6)
    K, c2w = torch.from_numpy(rig['intrin'][0]).to(dev), torch.from_numpy(rig['sensor2ego'][0]).to(dev)
    views = net.render_forecast(frames, ego, K, c2w, tuple(a.image), n_steps=6, stride=a.stride)
    os.makedirs(a.out, exist_ok=True)
    for k, v in views.items():
        np.save(os.path.join(a.out, k + '.npy'), v.cpu().numpy())
        print('%-12s %s %s' % (k, tuple(v.shape), v.dtype))


if __name__ == '__main__':
    main()
