"""Generate tests/golden/image_prep_small.npz: the reference's PrepareImageInputs4DTraj
(mmdet3d/datasets/pipelines/loading_traj_temporal.py:230-577) on synthetic frames.

Like tools/gen_golden_depth.py this runs only where the reference checkout exists, loads the reference file through the shim of
tools/gen_golden.py plus stand-ins for the packages it imports, and records inputs -> outputs as data; it contains no reference
source and the .npz holds arrays only.

    python tools/gen_golden_images.py

What is NOT the reference's own code: `mmcv.image.photometric.imnormalize` (mmcv and cv2 are not installable next to this
package) is bound to a float64 restatement, float32((float64(px[..., ::-1]) - mean) / std) -- the fixture says so
(normalize_restated = 1) -- and `Quaternion` is transforms.quaternion_rotation_matrix behind pyquaternion's interface.  The
canvas bytes come out of the installed Pillow (its version is recorded), the augmentations out of the reference's sampling
under np.random.seed(seed), post_rots / post_trans out of its float32 torch arithmetic.

Inputs: tests/_image_prep_np.py synthetic_sample (noise on gradients that saturate at 0 and 255; 45 x 80 frames to a 24 x 64
input, 6 cameras x (key + 1 adjacent) x (current + 6 future groups)).  Cases: `test` (is_train False) and `train<seed>` for
the recorded seeds, which between them draw down- and up-scaling, crops wider than the resized image, flips and both rotation
signs (asserted below)."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'tests'))
import _image_prep_np as IP  # noqa: E402
from preworld_amd import transforms as T  # noqa: E402

SEEDS = (0, 1, 2)
SAMPLE_SEED = 11


class _Quaternion:
    def __init__(self, *q):
        self.q = q

    @property
    def rotation_matrix(self):
        return T.quaternion_rotation_matrix(self.q)


def _imnormalize(img, mean, std, to_rgb=True):
    img = np.asarray(img).astype(np.float64)
    if to_rgb:
        img = img[..., ::-1]
    return ((img - mean.astype(np.float64)) / std.astype(np.float64)).astype(np.float32)


def load_reference():
    G.install_shim()
    base = type('Base', (), {})
    G._mod('numba')
    G._mod('mmcv.image')
    G._mod('mmcv.image.photometric', imnormalize=_imnormalize)
    G._mod('pyquaternion', Quaternion=_Quaternion)
    G._mod('mmdet3d.core')
    G._mod('mmdet3d.core.points', BasePoints=base, get_points_type=None)
    G._mod('mmdet3d.core.bbox', LiDARInstance3DBoxes=base)
    G._mod('mmdet.datasets')
    G._mod('mmdet.datasets.pipelines', LoadAnnotations=base, LoadImageFromFile=base)
    G._mod('mmdet3d.datasets')
    G._mod('mmdet3d.datasets.builder', PIPELINES=G._Registry())
    G._mod('mmdet3d.datasets.pipelines')
    return G.load_ref('mmdet3d.datasets.pipelines.loading_traj_temporal', 'mmdet3d/datasets/pipelines/loading_traj_temporal.py')


def run_case(mod, is_train, seed):
    import PIL.Image
    cfg = dict(IP.DATA_CONFIG)
    H, W = cfg['src_size']
    res = IP.synthetic_sample(SAMPLE_SEED, H, W, n_adj=1)
    files = res['files']
    mod.Image = types.SimpleNamespace(open=lambda p: PIL.Image.fromarray(files[p]), FLIP_LEFT_RIGHT=PIL.Image.FLIP_LEFT_RIGHT)
    ref = mod.PrepareImageInputs4DTraj(cfg, is_train=is_train, sequential=True)
    augs = []
    for name in ('sample_augmentation', 'sample_augmentation_temporal'):
        def wrap(*a, _f=getattr(ref, name), **k):
            r = _f(*a, **k)
            augs.append([r[0], r[1][0], r[1][1]] + list(r[2]) + [float(r[3]), r[4]])
            return r
        setattr(ref, name, wrap)
    np.random.seed(seed)
    out = ref({k: res[k] for k in ('curr', 'adjacent', 'temporal_ann_infos')})
    imgs, s2e, e2g, intr, pr, pt = out['img_inputs']
    d = dict(imgs=imgs.numpy(), sensor2egos=s2e.numpy(), ego2globals=e2g.numpy(), intrins=intr.numpy(), post_rots=pr.numpy(),
             post_trans=pt.numpy(), canvas=np.stack(out['canvas']), augs=np.array(augs, np.float64),
             gt_depths=out['gt_depths'].numpy())
    for k in range(1, 7):
        t = out['temporal_img_inputs'][k]
        d['t%d_post_rots' % k], d['t%d_post_trans' % k], d['t%d_ego2globals' % k] = t[4].numpy(), t[5].numpy(), t[2].numpy()
    d['t_imgs'] = np.stack([out['temporal_img_inputs'][k][0].numpy() for k in (1, 6)])
    return d


def main():
    import PIL
    mod = load_reference()
    cfg = IP.DATA_CONFIG
    out = dict(pil_version=np.array(PIL.__version__), normalize_restated=np.int64(1), seeds=np.array(SEEDS, np.int64),
               sample_seed=np.int64(SAMPLE_SEED), src_size=np.array(cfg['src_size'], np.int64),
               input_size=np.array(cfg['input_size'], np.int64))
    all_augs = []
    for name, is_train, seed in [('test', False, 0)] + [('train%d' % s, True, s) for s in SEEDS]:
        d = run_case(mod, is_train, seed)
        all_augs.append(d['augs'][:6])
        if name != 'train0':
            d.pop('t_imgs')
        out.update({'%s_%s' % (name, k): v for k, v in d.items()})
        print(name, 'augs:\n', np.round(d['augs'][:6], 3))
    a = np.concatenate(all_augs)
    fW = cfg['input_size'][1]
    assert (a[:, 1] < fW).any() and (a[:, 1] > fW).any() and (a[:, 7] == 1).any() and (a[:, 8] > 1).any() and (a[:, 8] < -1).any(), \
        'the recorded seeds must draw an over-wide crop, a flip and both rotation signs'
    G.save('image_prep_small.npz', **out)


if __name__ == '__main__':
    main()
