"""CPU-side checks of the dense view renderer (pw_render_views / pw_render_label_views): the C ABI is declared and exported, the
numpy restatement of the pixel -> ray mapping reproduces the reference's get_rays rows, the restated label mode gives the
hand-computed image of a wall, and the Python entry point refuses host tensors (the package has no CPU path)."""
import ctypes

import numpy as np
import pytest
import torch

import _render_views_np as RV
from preworld_amd import _lib, build, modules as M, ops

ENTRY_POINTS = ('pw_render_views', 'pw_render_label_views')


def _head():
    return M.NerfHead(point_cloud_range=[-40, -40, -1, 40, 40, 5.4], voxel_size=0.4, scene_center=[0, 0, 2.2], radius=39)


def test_view_entry_points_declared_and_exported():
    protos = _lib.parse_header()
    lib = ctypes.CDLL(build.build())
    for name in ENTRY_POINTS:
        assert name in protos, name + ' is not declared in include/preworld_hip.h'
        assert hasattr(lib, name), name + ' is not exported by libpreworld_hip.so'
    # the argument lists the Python layer relies on
    assert protos['pw_render_views'][2][:8] == ['K', 'c2w', 'n_views', 'H', 'W', 'x0', 'y0', 'stride']
    assert protos['pw_render_label_views'][2][10:17] == ['labels', 'X', 'Y', 'Z', 'stride_x', 'stride_y', 'stride_z']


def test_pixel_ray_restatement_reproduces_reference_get_rays(golden):
    g = golden('render_views_small.npz')
    H, W = [int(v) for v in g['hw']]
    origin = tuple(int(v) for v in g['origin'])
    rows = RV.pixel_rays(g['K'], g['c2w'], (H, W), 1, origin)
    np.testing.assert_allclose(rows, g['rays'], rtol=1e-6)
    # stride 2 looks through every second source pixel of the same window
    rows2 = RV.pixel_rays(g['K'], g['c2w'], (H // 2, W // 2), 2, origin)
    np.testing.assert_allclose(rows2, g['rays'][:, ::2, ::2], rtol=1e-6)


def test_label_mode_restatement_on_a_wall():
    """A camera at the scene centre looking along +x at a wall that fills the grid from voxel column 150 on: every pixel's class is
    the wall's; the depth, mapped back from the reference's s = t / (1 + t) to metres along the ray, is the distance to the wall's
    near face (half a voxel before the centres of column 150) within one sample spacing (2 / 391 of the 39 m radius)."""
    head = _head()
    consts, t = head.consts(torch.eye(3)), head.t_table('cpu').numpy()
    labels = np.full((200, 200, 16), 17, np.uint8)
    labels[150:] = 3
    K = np.array([[[100.0, 0, 6.0], [0, 100.0, 4.0], [0, 0, 1]]], np.float32)
    c2w = np.eye(4, dtype=np.float32)[None].copy()
    c2w[0, :3, :3] = [[0, 0, 1], [-1, 0, 0], [0, -1, 0]]              # camera z (forward) = world +x, image x = -y, image y = -z
    c2w[0, :3, 3] = [0.0, 0.0, 2.2]
    rows = RV.pixel_rays(K, c2w, (8, 12)).reshape(-1, 9)
    cls, depth, last, first, _ = RV.label_views(labels, rows[:, 0:3], rows[:, 3:6], consts, t)
    assert (cls == 3).all() and (last == 0).all() and (first > 0).all()
    # the face: continuous index 149.5 of 199 intervals over [xyz_min, xyz_max] = [-40/39, 40/39] (normalised), times the radius
    x_face = (-40.0 / 39 + 149.5 / 199 * 80.0 / 39) * 39.0
    along = x_face / rows[:, 6]                                        # metres along the unit view direction until x = x_face
    s = depth.astype(np.float64) / 39.0 - 1e-7
    metres = s / (1 - s) * 39.0
    spacing = 2.0 / 391 * 39.0
    assert (metres >= along - 1e-3).all() and (metres <= along + spacing + 1e-3).all(), (metres - along).max()
    # nothing in front of the camera: a miss
    cls0, depth0, last0, first0, _ = RV.label_views(np.full((200, 200, 16), 17, np.uint8), rows[:, 0:3], rows[:, 3:6], consts, t)
    assert (cls0 == 17).all() and (last0 == 1).all() and (first0 == -1).all()
    np.testing.assert_allclose(depth0, np.float32(1e-7) * np.float32(39), rtol=1e-6)


def test_render_views_refuses_host_tensors():
    head = _head()
    K, c2w = torch.eye(3)[None], torch.eye(4)[None]
    consts, t = head.consts(torch.eye(3)), head.t_table('cpu')
    with pytest.raises(_lib.PreworldHipError):
        ops.render_views(torch.zeros(16, 200, 200, 24), K, c2w, (4, 4), consts, t)
    with pytest.raises(_lib.PreworldHipError):
        ops.render_label_views(torch.zeros(200, 200, 16, dtype=torch.uint8), K, c2w, (4, 4), consts, t)


def test_bad_arguments_are_refused_before_any_launch():
    """null outputs, V <= 0, n_samples > 448, a label grid handed to the packed-grid entry point, misaligned pointers: PW_EINVAL (-1)
    and a pw_last_error() text naming the entry point.  Validation precedes every HIP call, so the addresses are never touched."""
    l = _lib.lib()
    P = ctypes.c_void_p
    a = 0x10000                                                       # an aligned, never dereferenced address
    consts = (ctypes.c_float * 27)(*[1.0] * 27)

    def soft(K=a, c2w=a, V=2, H=8, W=8, S=417, grid=a, GC=24, n_sem=17, depth=a, cls=a, stride=1):
        return l.pw_render_views(P(K), P(c2w), V, H, W, 0, 0, stride, P(a), S, P(grid), 200, 200, 16, GC, 0, 2, n_sem, 19, consts,
                                 P(depth), P(cls), None, None, None, None, None, 0.0, 0, None)

    def label(V=1, S=417, labels=a, depth=a, cls=a, sx=3200, empty=17):
        return l.pw_render_label_views(P(a), P(a), V, 8, 8, 0, 0, 1, P(a), S, P(labels), 200, 200, 16, sx, 16, 1, empty, consts,
                                       P(depth), P(cls), None, None, None, 0, None)

    cases = [(lambda: soft(depth=None, cls=None), b'no output'), (lambda: soft(V=0), b'view count'), (lambda: soft(V=-3), b'view count'),
             (lambda: soft(S=449), b'n_samples'), (lambda: soft(GC=1), b'pw_render_label_views'), (lambda: soft(K=a + 2), b'aligned'),
             (lambda: soft(depth=a + 1), b'aligned'), (lambda: soft(grid=None), b'null'), (lambda: soft(stride=0), b'stride'),
             (lambda: soft(n_sem=5), b'17'), (lambda: label(depth=None, cls=None), b'no output'), (lambda: label(V=0), b'view count'),
             (lambda: label(S=1000), b'n_samples'), (lambda: label(labels=None), b'null'), (lambda: label(depth=a + 2), b'aligned'),
             (lambda: label(sx=0), b'strides'), (lambda: label(empty=300), b'empty_idx')]
    for k, (call, text) in enumerate(cases):
        assert call() == -1, k
        msg = l.pw_last_error()
        assert b'pw_render_' in msg and text in msg, (k, msg)
