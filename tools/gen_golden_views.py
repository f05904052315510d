"""Generate tests/golden/render_views_small.npz: the reference's get_rays (mmdet3d/datasets/ray.py) and NerfHead
(render_one_scene -> render_depth / render_semantic / render_color) on every pixel of a small two-camera window.

Like tools/gen_golden.py this runs only where the reference checkout exists, loads its Python files through the same shim and
records inputs -> outputs as data; it contains no reference source and the .npz holds arrays only.

    python tools/gen_golden_views.py [seed_soft seed_mixed seed_clear]

The class-map test excuses pixels whose two largest rendered semantic sums are closer than 2 (1e-3 |top| + 1e-3) and allows at
most 1e-3 of the pixels to be such near-ties: the count is printed per scene and stored (`<scene>_n_near_tie`).  The soft and
mixed scenes cannot meet that cap for any seed (see main()); the class map is pinned on a third scene, 'clear', recorded in the same
fixture with its own rig, on which the generator enforces the cap.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'tests'))
import _render_views_np as RV  # noqa: E402
from preworld_amd import synth as S  # noqa: E402

H, W, ORIGIN = 24, 40, (3, 5)          # output window: 24 x 40 pixels from source pixel (x0, y0) = (3, 5)
BDA = np.array([[0.98, 0.05, 0.0], [-0.05, 0.98, 0.0], [0.0, 0.0, 1.0]], np.float32)      # as test_fused_render_vs_oracle


def rig():
    """two cameras: the rig's front camera pitched down 12 deg and yawed 20 deg about its own axes, and the rear camera as it is;
    a short focal length (the window is 40 pixels wide) and an off-centre principal point"""
    s2e = S.synthetic_rig(6, dtype=np.float64)['sensor2ego'][0]
    p, y = np.radians(12.0), np.radians(20.0)
    Rx = np.array([[1, 0, 0], [0, np.cos(p), -np.sin(p)], [0, np.sin(p), np.cos(p)]])
    Ry = np.array([[np.cos(y), 0, np.sin(y)], [0, 1, 0], [-np.sin(y), 0, np.cos(y)]])
    a = s2e[1].copy()
    a[:3, :3] = a[:3, :3] @ Ry @ Rx.T
    a[:3, 3] += [0.3, -0.2, 0.1]
    c2w = np.stack([a, s2e[4]]).astype(np.float32)
    K = np.array([[[22.0, 0, 23.7], [0, 21.0, 15.2], [0, 0, 1]], [[25.5, 0, 21.3], [0, 24.0, 18.9], [0, 0, 1]]], np.float32)
    return K, c2w


def load_reference():
    G.install_shim()
    G._mod('mmdet3d.models.nerf.utils')
    import torch.utils.cpp_extension as cpp_ext
    real_load = cpp_ext.load
    cpp_ext.load = lambda name, **kw: G._NativeStubs
    sys.modules['turtle'] = types.ModuleType('turtle')
    sys.modules['turtle'].forward = None
    try:
        G.load_ref('mmdet3d.models.nerf.utils', 'mmdet3d/models/nerf/utils.py')
    finally:
        cpp_ext.load = real_load
    nh = G.load_ref('mmdet3d.models.nerf.nerf_head', 'mmdet3d/models/nerf/nerf_head.py')
    ray = G.load_ref('ref_ray', 'mmdet3d/datasets/ray.py')
    return nh, ray


def ref_rays(ray, K, c2w):
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))                   # (H, W): column / row of the output pixel
    x = torch.from_numpy((ORIGIN[0] + jj).reshape(-1).astype(np.float32))
    y = torch.from_numpy((ORIGIN[1] + ii).reshape(-1).astype(np.float32))
    rows = []
    for v in range(2):
        o, d, vd = ray.get_rays(x + 0.5, y + 0.5, K=torch.from_numpy(K[v]), c2w=torch.from_numpy(c2w[v]))       # as pts2ray calls it (:50)
        rows.append(torch.cat([o, d, vd], 1))
    return torch.stack(rows).contiguous()                              # (V, H*W, 9)


def main():
    seeds = dict(soft=int(sys.argv[1]) if len(sys.argv) > 1 else 31, mixed=int(sys.argv[2]) if len(sys.argv) > 2 else 61,
                 clear=int(sys.argv[3]) if len(sys.argv) > 3 else 63)      # clear: 61 -> 2 near-ties (over the cap), 62 -> 0, 63 -> 1
    nh, ray = load_reference()
    head = G._ref_head(nh)
    K, c2w = rig()
    Kc, c2wc = RV.clear_rig()
    rows, rows_c = ref_rays(ray, K, c2w), ref_rays(ray, Kc, c2wc)
    out = dict(K=K, c2w=c2w, bda=BDA, hw=np.array([H, W], np.int64), origin=np.array(ORIGIN, np.int64),
               rays=rows.numpy().reshape(2, H, W, 9), clear_K=Kc, clear_c2w=c2wc, clear_rays=rows_c.numpy().reshape(2, H, W, 9))
    n = 2 * H * W
    for tag, grids, rows in (('soft', S.render_grids(seeds['soft']), rows), ('mixed', S.render_grids_mixed(seeds['mixed']), rows),
                             ('clear', RV.clear_scene(seeds['clear']), rows_c)):
        density, semantic, color = [torch.from_numpy(a) for a in grids]
        with torch.no_grad():
            res = head.render_one_scene(rows[..., 0:3].reshape(-1, 3).contiguous(), rows[..., 3:6].reshape(-1, 3).contiguous(),
                                        torch.from_numpy(BDA), density, semantic, color, mask=None)
            res['N_ray'] = n
            depth, sem, col = head.render_depth(res), head.render_semantic(res), head.render_color(res)
        last = res['alphainv_last'].numpy()
        sem = sem.numpy()
        top2 = np.sort(sem, -1)[:, -2:]
        margin, top = top2[:, 1] - top2[:, 0], np.abs(sem).max(-1)
        near = margin <= 2 * (1e-3 * np.abs(top2[:, 1]) + 1e-3)
        print('  %-5s seed %d: %d pixels, %d terminated (T < 1e-3), %d with alphainv_last > 0.99; near-tie pixels of the class map: %d '
              '(cap %.1f)' % (tag, seeds[tag], n, int((last < 1e-3).sum()), int((last > 0.99).sum()), int(near.sum()), 1e-3 * n))
        print('        max |semantic| %.3e, median top-two margin %.3e' % (float(top.max()), float(np.median(margin))))
        # The class-map cap (at most 1e-3 of the pixels near-ties) is a condition on the reference's own output.  The 'soft' and
        # 'mixed' scenes cannot meet it for any seed: S.render_grids is transparent by construction (density = softplus(4 N(0,1) - 6)
        # against act_shift = -13.8): its semantic sums are ~1e-3, inside the absolute part of the bound (seeds 31, 21, 5: 1920 /
        # 1920); on the mixed scene a third of the pixels look past every box and the semantic field is i.i.d. N(0,1) per voxel, which
        # puts ~1 % of the pixels that hit something under the bound.  The class map is therefore pinned on the 'clear' scene
        # (tests/_render_views_np.py: every ray meets the ground or a box, region-wise winners), where the cap is enforced here.
        assert tag != 'clear' or near.sum() <= 1e-3 * n, 'too many near-ties in the reference class map of the clear scene: choose another seed'
        out.update({tag + '_seed': np.int64(seeds[tag]), tag + '_n_near_tie': np.int64(near.sum()),
                    tag + '_depth': depth.numpy().reshape(2, H, W), tag + '_semantic': sem.reshape(2, H, W, 17),
                    tag + '_color': col.numpy().reshape(2, H, W, 3), tag + '_alphainv_last': last.reshape(2, H, W),
                    tag + '_margin': margin.reshape(2, H, W), tag + '_max_abs_semantic': top.reshape(2, H, W)})
    G.save('render_views_small.npz', **out)


if __name__ == '__main__':
    main()
