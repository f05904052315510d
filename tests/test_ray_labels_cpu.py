"""Ray supervision from the sweep, the part that needs no GPU: the numpy restatement (tests/_ray_labels_np.py) against an ideal
float64 projection (stage A) and against the reference's own get_rays (stage B, tests/golden/ray_labels_small.npz, written by
`tools/gen_golden.py ray_labels`), the argument validation of the new entry points and the host-side pose composition."""
import numpy as np
import pytest

import _ray_labels_np as RN
from preworld_amd import _lib, transforms

@pytest.fixture(scope='module')
def fx(golden):
    return golden('ray_labels_small.npz')


def _fixture_lists(fx):
    off = fx['view_off']
    V = len(off) - 1
    return ([fx['depth_list'][off[v]:off[v + 1]] for v in range(V)], [fx['seg_list'][off[v]:off[v + 1]] for v in range(V)], off)


def test_restatement_vs_ideal_projection():
    """Stage A with its eight float32 roundings against one float64 chain, 2 frames x 6 cameras of 900 x 1600, P = 3 000 points
    per sweep: all around the lidar (behind every camera, depth <= 0 included) plus, per view, 6 points 0.15 .. 0.9 px on either
    side of each of the four mask thresholds.

    THE BOUND.  The chain rounds the cloud to float32 after each of its eight sub-steps (and rounds the four translations
    themselves); the coordinates are below 2048 m throughout (global translations ~1e3 m), where half a float32 ulp is
    2^-14 m = 6.1e-5 m.  Only three of these roundings actually act on ~1e3 m values (t2, the sum p + t2, and t3; every other
    intermediate is below 64 m, half-ulp 1.9e-6 m), so charging ALL EIGHT at 2^-14 m is conservative: E = 8 * 2^-14 m =
    4.9e-4 m per axis, |error vector| <= sqrt(3) E.  With u = f x / z + c, du <= (f / z) |err| (1 + |x / z|), and |x / z| <=
    max(W, H) / (2 f) inside the image; the float32 rounding of the pixel itself adds half an ulp of 1600, 6.1e-5 px:
        bound(z) = (f / z) * sqrt(3) * 8 * 2^-14 * (1 + max(W, H) / (2 f)) + 2^-14  [px]      (1.75 px at 1 m, 0.09 px at 20 m)
    The depth obeys |dz| <= sqrt(3) E.  This catches a wrong transpose or a wrong order of steps (errors of many pixels), not a
    subtle rounding; the sharp pin of the rounding is the bit-for-bit GPU test against this restatement.

    KEPT SETS may differ only where the ideal projection lies within bound(z) of a mask threshold (or the ideal depth within
    sqrt(3) E of 0).  Cap, a condition: such points are at most 2 % of the kept points of each view (about 0.4 % expected;
    the seed was checked on this restatement so that every view passes)."""
    T, N, P, H, W, f = 2, 6, 3000, 900, 1600, 1266.0
    S = RN.synthetic_sample(7, T=T, N=N, P=P, H=H, W=W, focal=f, border=6)
    E = np.sqrt(3.0) * 8 * 2.0 ** -14
    for v in range(T * N):
        pts = S['points'][v // N]
        keep, uvd = RN.project(pts, S['poses'][v], H, W)
        u, q, d = RN.project_ideal(pts, S['poses'][v])
        with np.errstate(all='ignore'):
            bound = (f / np.abs(d)) * E * (1 + max(W, H) / (2 * f)) + 2.0 ** -14
            ideal_keep = (d > 0) & (u > 1) & (u < W - 1) & (q > 1) & (q < H - 1)
            near = (np.abs(d) <= E) | (np.minimum(np.abs(u - 1), np.abs(u - (W - 1))) <= bound) | \
                   (np.minimum(np.abs(q - 1), np.abs(q - (H - 1))) <= bound)
        eu, ev = np.abs(uvd[keep, 0] - u[keep]), np.abs(uvd[keep, 1] - q[keep])
        print('view %2d: kept %d, max pixel error %.4f / %.4f px (largest share of its bound %.3f), near a threshold %d (%.2f %%), '
              'kept sets differ in %d' % (v, keep.sum(), eu.max(), ev.max(), max((eu / bound[keep]).max(), (ev / bound[keep]).max()),
                                          (near & (keep | ideal_keep)).sum(), 100.0 * (near & (keep | ideal_keep)).sum() / keep.sum(),
                                          (keep != ideal_keep).sum()))
        assert keep.sum() > 300
        assert (d <= 0).sum() > 1000                                                    # behind the camera / depth <= 0
        band = ideal_keep & ((u < 2) | (u > W - 2) | (q < 2) | (q > H - 2))
        assert band.sum() >= 8 and (~ideal_keep & (d > 0) & (u > 0) & (u < W) & (q > 0) & (q < H)).sum() >= 8      # both sides of the borders
        assert (eu <= bound[keep]).all() and (ev <= bound[keep]).all()
        assert (np.abs(uvd[keep, 2] - d[keep]) <= E).all()
        assert not ((keep != ideal_keep) & ~near).any()
        assert (near & (keep | ideal_keep)).sum() <= 0.02 * keep.sum()


def test_stage_a_is_what_the_fixture_holds(fx):
    """the lists in the fixture are the restatement's stage A on the seeded sample (so the GPU tests can start from the sweeps)"""
    T, N, P, H, W = [int(v) for v in fx['shape']]
    S = RN.synthetic_sample(int(fx['seed']), T=T, N=N, P=P, H=H, W=W, focal=float(fx['focal']))
    dl, sl = RN.stage_a(S['points'], S['labels'], RN.LUT, S['poses'], N, H, W)
    assert np.array_equal(np.concatenate(dl).view(np.uint32), fx['depth_list'].view(np.uint32))
    assert np.array_equal(np.concatenate(sl).view(np.uint32), fx['seg_list'].view(np.uint32))
    assert np.array_equal(RN.offsets(dl), fx['view_off']) and np.array_equal(S['frames'], fx['frames'])
    for a, b in zip(dl, sl):
        assert a.dtype == np.float32 and np.array_equal(a[:, :2], b[:, :2])


def test_stage_b_vs_reference(fx):
    """The restatement's table and weights against the reference's get_rays on the same lists and frames.  Integer and label
    columns (0-3) exact, the colours (13-15) exact as well (one float32 expression on both sides); the float columns within the
    bound test_ray_table_and_wrs_weights uses (rtol 2e-6, atol 1e-6); weights rtol 1e-5 (batch) and 1e-6 (given)."""
    T, N, P, H, W = [int(v) for v in fx['shape']]
    dl, sl, off = _fixture_lists(fx)
    table = RN.stage_b(dl, sl, fx['frames'], None, fx['c2w'], fx['K'], H, W)
    want = fx['table']
    assert table.shape == want.shape == (int(off[-1]), 16)
    np.testing.assert_array_equal(table[:, :4], want[:, :4])
    np.testing.assert_array_equal(table[:, 13:], want[:, 13:])
    np.testing.assert_allclose(table, want, rtol=2e-6, atol=1e-6)
    for v in range(T * N):                                # numpy's one-shot fancy assignment keeps the last point too
        a, b = RN.view_labels(dl[v], sl[v], fx['frames'][v], H, W), RN.view_labels(dl[v], sl[v], fx['frames'][v], H, W, fancy=True)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    frame_ids = [0] * N + [1] * N
    w = RN.weights(table, off, frame_ids, fx['dynamic_class'])
    np.testing.assert_allclose(w, fx['weights_batch'], rtol=1e-5)
    adj, dyn = [float(v) for v in fx['weight_adj_dyn']]
    w2 = RN.weights(table, off, frame_ids, fx['dynamic_class'], fx['balance_weight'], adj, dyn)
    np.testing.assert_allclose(w2, fx['weights_given'], rtol=1e-6)
    assert (w2[int(off[N]):] < w2[int(off[N]):].max()).any() and (w[int(off[N]):] == 0).any()       # dynamic classes in the later frame
    # all 17 classes, and pixels hit by points of different labels: the last in sweep order wins
    assert set(np.unique(want[:, 3]).astype(int)) == set(range(17))
    n_multi = 0
    for v in range(T * N):
        rows = want[int(off[v]):int(off[v + 1])]
        pix = rows[:, 1].astype(np.int64) * W + rows[:, 0].astype(np.int64)
        assert np.array_equal(rows[:, :2], dl[v][:, :2].astype(np.int16).astype(np.float32))
        for p in np.unique(pix):
            m = np.nonzero(pix == p)[0]
            labels = sl[v][m, 2]
            if len(m) >= 2 and len(set(labels)) >= 2:
                n_multi += 1
                assert (rows[m, 3] == labels[-1]).all()                  # every point of the pixel carries the last one's label
                assert np.array_equal(rows[m, 2], dl[v][m, 2])           # ... and keeps its own depth
    print('pixels hit by points of different labels: %d' % n_multi)
    assert n_multi >= 50


def test_rays_header_parses_like_the_main_header():
    """include/preworld_hip_rays.h (included by preworld_hip.h) under the rules tests/test_abi.py and tests/test_marshal_cpu.py hold
    the main header to: every pw_*( parses, every pointer parameter has a converter, the library exports every name"""
    import ctypes
    import re
    text = open(_lib.RAYS_HEADER_PATH).read()
    code = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    protos = _lib.parse_header(_lib.RAYS_HEADER_PATH)
    assert set(re.findall(r'\b(pw_\w+)\s*\(', code)) == set(protos) == {
        'pw_ray_sweep_count', 'pw_ray_sweep_lists', 'pw_ray_sweep_table', 'pw_ray_lists_table', 'pw_ray_table_weights'}
    assert '#include "preworld_hip_rays.h"' in open(_lib.HEADER_PATH).read()
    l = _lib.lib()
    for fn, (_, argtypes, argnames) in protos.items():
        assert hasattr(l, fn) and fn in _lib.protos()
        params = re.search(r'\b%s\s*\(([^;{]*?)\)\s*;' % fn, code).group(1).split(',')
        assert len(params) == len(argtypes) == len(argnames), fn
        for ptext, a, name in zip(params, argtypes, argnames):
            assert ('*' in ptext) == isinstance(a, _lib._PtrArg), (fn, name)
            if '*' in ptext:
                assert not a.table and a.host == name.endswith('_host'), (fn, name)
        assert ctypes.c_void_p not in _lib._fns[fn].argtypes and argnames[-1] == 'stream', fn
    assert _lib.PW_RAYS['PW_RAY_POSE_DOUBLES'] == RN.POSE_DOUBLES


def test_new_entry_points_validate_before_any_hip_call():
    l = _lib.lib()
    one = 0x1000                                     # a non-null, 16-byte aligned address that is never dereferenced
    sweep = (one, 5, None, 2, 2, 3001, one, 48, 80)
    rows = (one, 11520, 240, 3, 1, 4, None, one, one, one, 4096, one, 17, one, None)
    cases = [
        ('pw_ray_sweep_count', (None,) + sweep[1:] + (one, 32768, one, one, None)),                        # null points
        ('pw_ray_sweep_count', (one, 2) + sweep[2:] + (one, 32768, one, one, None)),                       # stride < 3
        ('pw_ray_sweep_count', sweep + (one, 30000, one, one, None)),                                      # slots not a power of two
        ('pw_ray_sweep_count', sweep + (one, 8192, one, one, None)),                                       # fewer slots than points
        ('pw_ray_sweep_count', sweep + (one, 1 << 32, one, one, None)),                                    # more than 2^31 slots
        ('pw_ray_sweep_count', sweep + (None, 32768, one, one, None)),                                     # a slot count without slots
        ('pw_ray_sweep_count', sweep[:7] + (48, 40000) + (one, 32768, one, one, None)),                    # W beyond int16
        ('pw_ray_sweep_count', sweep + (one, 32768, None, one, None)),                                     # null block_base
        ('pw_ray_sweep_lists', (one, 5, None, None, 2, 2, 3001, one, one, 48, 80, one, 100, one, one, None)),      # null labels
        ('pw_ray_sweep_lists', (one, 5, one, None, 2, 2, 3001, one, one, 48, 80, one, 0, one, one, None)),         # capacity 0
        ('pw_ray_sweep_table', (one, 5, one, None, 2, 2, 3001, one, one, 48, 80, one, 32768, one) + rows[:7] + (None,) + rows[8:]),   # no mean / std
        ('pw_ray_sweep_table', (one, 5, one, None, 2, 2, 3001, one, one, 48, 80, one, 32768, one) + rows[:11] + (one + 4,) + rows[12:]),  # rays misaligned
        ('pw_ray_sweep_table', (one, 5, one, None, 2, 2, 3001, one, one, 48, 80, one, 32768, one) + rows[:12] + (65,) + rows[13:]),   # n_cls > 64
        ('pw_ray_lists_table', (one, one, 0, one, 4, 48, 80, one, 4096) + rows),                                      # n = 0
        ('pw_ray_lists_table', (one, one, 2600, None, 4, 48, 80, one, 8192) + rows),                                  # null view_off
        ('pw_ray_lists_table', (one, one, 2600, one, 4, 48, 80, one, 2048) + rows),                                   # too few slots
        ('pw_ray_lists_table', (one, one, 2600, one, 4, 48, 80, one, 8192) + (one, -1) + rows[2:]),                   # negative stride
        ('pw_ray_table_weights', (one, 4096, one, 4, one, None, None, 17, one, 8, 0.3, 0.0, one, None)),              # neither weights nor counts
        ('pw_ray_table_weights', (one, 4096, one, 4, one, one, None, 17, None, 8, 0.3, 0.0, one, None)),              # null dynamic_class
        ('pw_ray_table_weights', (one, 0, one, 4, one, one, None, 17, one, 8, 0.3, 0.0, one, None)),                  # capacity 0
    ]
    for name, args in cases:
        assert len(args) == len(_lib.protos()[name][1]), (name, len(args), len(_lib.protos()[name][1]))
        rc = getattr(l, name)(*args)
        assert rc == -1, (name, rc)
        assert name.encode() in l.pw_last_error(), (name, l.pw_last_error())


def test_host_pose_composition(fx):
    """transforms.compose_sensor2keyegos (the reference's float32 poses, float64 products, float32 result) against an independent
    all-float64 product from the quaternions.  Bound: the two ego translations (~1.7e3 m) are rounded to float32, each off by
    at most 2^-14 m per axis, sqrt(3) 2^-14 m as a vector, and the rotations applied to them preserve length; the float32
    rotation entries (6e-8 off) act on the few metres between the two ego poses and on the mount, and the result is rounded at
    ~1e1 m: together under 1e-5 m.  Translation column <= 2 sqrt(3) 2^-14 + 1e-5 = 2.2e-4 m, rotation block <= 1e-6.  Catches a
    missing inverse, a swapped factor or a wrong key frame (metres), not a change of precision.  compose_view_poses is checked
    entry for entry against the restatement's."""
    T, N, P, H, W = [int(v) for v in fx['shape']]
    S = RN.synthetic_sample(int(fx['seed']), T=T, N=N, P=P, H=H, W=W, focal=float(fx['focal']))
    got = transforms.compose_sensor2keyegos(S['infos'], S['cam_names']).numpy()
    want = RN.sensor2keyegos_f64(S['infos'], S['cam_names'])
    assert got.dtype == np.float32 and got.shape == (T * N, 4, 4)
    assert np.abs(got[:, :3, 3] - want[:, :3, 3]).max() <= 2 * np.sqrt(3) * 2.0 ** -14 + 1e-5
    assert np.abs(got[:, :3, :3] - want[:, :3, :3]).max() <= 1e-6
    assert np.abs(got[:, 3] - np.array([0, 0, 0, 1], np.float32)).max() <= 1e-12       # the LU inverse leaves ~1e-20 there
    assert np.abs(got[N:, :3, 3] - got[:N, :3, 3]).max() > 1.0             # the later frame really is elsewhere
    np.testing.assert_allclose(got, fx['c2w'], rtol=0, atol=1e-6)          # what the reference's get_rays composed
    poses = transforms.compose_view_poses(S['infos'], S['cam_names'])
    assert poses.dtype.is_floating_point and poses.element_size() == 8
    assert np.array_equal(poses.numpy(), S['poses'])
    q = S['infos'][0]['ego2global_rotation']
    assert np.array_equal(transforms.quaternion_rotation_matrix(q), RN.quat_matrix(q))


def test_pipeline_picks_frames_like_get_rays(monkeypatch):
    """SweepsToRays without a GPU: the neighbour of another scene and the missing neighbour fall back to the key sample, the
    frames of a repeated sample are passed once, and the registry gets the class through the NEW registration function."""
    import torch
    from preworld_amd import rays
    S = RN.synthetic_sample(3, T=3, N=2, P=50, scenes=[0, 1, 0])
    calls = {}

    def fake(points, labels, frames, view_pose, c2w, intrins, **kw):
        calls.update(points=points, labels=labels, frames=frames, view_pose=view_pose, c2w=c2w, intrins=intrins, kw=kw)
        return 'rays'
    monkeypatch.setattr(rays, 'generate_rays_from_sweeps', fake)
    entry = [dict(info=S['infos'][t], points=torch.from_numpy(S['points'][t]), point_labels=torch.from_numpy(S['labels'][t]),
                  frames=torch.from_numpy(S['frames'][2 * t:2 * t + 2])) for t in range(3)]
    results = dict(curr=S['infos'][0], ray_frames={0: entry[0], -1: entry[1], 2: entry[2]})      # -1: another scene; 1: missing
    t = transforms.SweepsToRays(aux_frames=[-1, 1, 2], max_ray_nums=77, class_nums=np.arange(1, 18), dynamic_class=[0, 4], device='cpu')
    assert t(results)['rays'] == 'rays'
    used = [S['infos'][0], S['infos'][0], S['infos'][0], S['infos'][2]]
    assert np.array_equal(calls['view_pose'].numpy(), RN.view_poses(used, S['cam_names']))
    assert np.array_equal(calls['c2w'].numpy(), transforms.compose_sensor2keyegos(used, S['cam_names']).numpy())
    assert [p.shape[0] for p in calls['points']] == [50] * 4 and torch.equal(calls['points'][1], calls['points'][0])
    assert calls['frames'].shape[0] == 4 and calls['kw']['view_frame'] == [0, 1, 0, 1, 0, 1, 2, 3]
    assert calls['kw']['time_ids'] == {0: [0, 1], -1: [2, 3], 1: [4, 5], 2: [6, 7]} and calls['kw']['max_ray_nums'] == 77
    n = torch.arange(1, 18).float()
    assert torch.equal(calls['kw']['balance_weight'], torch.exp(0.005 * (n.max() / n - 1)))
    assert calls['kw']['dynamic_class'].tolist() == [0, 4]
    assert transforms.SweepsToRays(wrs_use_batch=True, class_nums=np.arange(1, 18)).balance_weight is None
    assert transforms.SweepsToRays().dynamic_class is None              # the dataset's class list is the caller's

    class Reg:
        def __init__(self):
            self.d = {}

        def register_module(self, name=None, force=False, module=None):
            self.d[name] = module
    reg = Reg()
    assert transforms.register_ray_pipelines(reg) == ['SweepsToRays'] and reg.d['SweepsToRays'] is transforms.SweepsToRays
