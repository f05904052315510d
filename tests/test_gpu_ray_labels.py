"""Ray supervision from the sweep on the GPU (csrc/pw_ray_labels.hip; ops.sweep_pixel_labels / ray_table / ray_table_weights,
rays.generate_rays_from_sweeps / generate_rays_from_labels, transforms.SweepsToRays) against the numpy restatement
(tests/_ray_labels_np.py) and the reference fixture (tests/golden/ray_labels_small.npz).

Both sides of stage A run the same written float64 / float32 contract, so lists are compared BIT FOR BIT: no pixel is excused.
Table: columns 0-3 (pixel, depth, class) and 13-15 (colour) bit-equal; columns 4-12 (origin, direction, view direction) within
test_ray_table_and_wrs_weights_gpu's bound, rtol 2e-6 / atol 1e-6.  Class counts exact, weights bit-equal to the restatement."""
import numpy as np
import pytest
import torch

import _ray_labels_np as RN
from preworld_amd import ops, rays as R, transforms

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DYN = [0, 1, 3, 4, 5, 7, 9, 10]


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope='module')
def fx(golden):
    return golden('ray_labels_small.npz')


def _reference(S, frame_ids, view_frame=None):
    """the restatement on one synthetic sample, computed once per sample"""
    N, H, W = S['N'], S['H'], S['W']
    dl, sl = RN.stage_a(S['points'], S['labels'], RN.LUT, S['poses'], N, H, W)
    c2w, K = RN.camera_tables(S['infos'], S['cam_names'])
    table = RN.stage_b(dl, sl, S['frames'], view_frame, c2w, K, H, W)
    return dict(dl=dl, sl=sl, off=RN.offsets(dl), c2w=c2w, K=K, table=table, frame_ids=frame_ids, counts=RN.class_counts(table))


def _sweeps(S):
    return ops.RaySweeps([T(p) for p in S['points']], [T(l) for l in S['labels']], T(S['poses']), T(RN.LUT))


@pytest.fixture(scope='module')
def small():
    S = RN.synthetic_sample(11, T=2, N=2, P=3001, H=48, W=80, focal=40.0)
    return S, _reference(S, [0, 0, 1, 1])


def _check_table(got, want, tag=''):
    got = got.cpu().numpy()
    assert got.shape == want.shape, (got.shape, want.shape)
    same = bits(got) == bits(want)
    print('%s rows %d: columns 4-12 differ in %d of %d entries, largest difference %.3e' %
          (tag, len(want), int((~same[:, 4:13]).sum()), same[:, 4:13].size, float(np.abs(got[:, 4:13] - want[:, 4:13]).max()) if len(want) else 0.0))
    assert same[:, :4].all() and same[:, 13:].all()
    np.testing.assert_allclose(got[:, 4:13], want[:, 4:13], rtol=2e-6, atol=1e-6)
    return same.all()


def test_stage_a_bit_exact(small):
    """5: T = 2 x N = 2, P = 3 001 (12 blocks of 256 per view, the last one partial), 48 x 80 so that multi-hit pixels are the norm"""
    S, ref = small
    dlist, slist, off = ops.sweep_pixel_labels([T(p) for p in S['points']], [T(l) for l in S['labels']], T(S['poses']), (S['H'], S['W']), T(RN.LUT))
    assert np.array_equal(off.cpu().numpy(), ref['off']) and off.dtype == torch.int32
    assert ref['off'][-1] > 2000 and min(np.diff(ref['off'])) > 300
    assert np.array_equal(bits(dlist), bits(np.concatenate(ref['dl'])))             # kept set, order, u, v, depth
    assert np.array_equal(bits(slist), bits(np.concatenate(ref['sl'])))             # ... and labels


def test_table_from_sweeps(small):
    """6"""
    S, ref = small
    sw = _sweeps(S)
    table, off, counts = ops.ray_table(T(ref['c2w']), T(ref['K']), T(S['frames']), sweeps=sw)
    n = int(ref['off'][-1])
    assert table.shape == (n, 16) and np.array_equal(off.cpu().numpy(), ref['off'])
    _check_table(table, ref['table'], 'sweeps')
    assert np.array_equal(counts.cpu().numpy(), ref['counts']) and counts.dtype == torch.int64
    w = ops.ray_table_weights(table, off, ref['frame_ids'], DYN, counts=counts)
    assert np.array_equal(bits(w), bits(RN.weights(ref['table'], ref['off'], ref['frame_ids'], DYN)))
    bw = np.exp(0.005 * (17.0 / np.arange(1, 18) - 1)).astype(np.float32)
    w = ops.ray_table_weights(table, off, ref['frame_ids'], DYN, balance_weight=T(bw))
    assert np.array_equal(bits(w), bits(RN.weights(ref['table'], ref['off'], ref['frame_ids'], DYN, bw)))
    w = ops.ray_table_weights(table, off, ref['frame_ids'], DYN, counts=counts, weight_adj=0.25, weight_dyn=0.1)
    assert np.array_equal(bits(w), bits(RN.weights(ref['table'], ref['off'], ref['frame_ids'], DYN, None, 0.25, 0.1)))
    # capacity above R: the rows are the same, rows >= n_rows have weight 0 and are zero
    big, w, n_rows = R.generate_rays_from_sweeps(sw, None, T(S['frames']), None, T(ref['c2w']), T(ref['K']), time_ids={0: [0, 1], 1: [2, 3]},
                                                 dynamic_class=torch.tensor(DYN), balance_weight=T(bw), weight_adj=0.25, weight_dyn=0.1,
                                                 capacity=n + 300)
    assert int(n_rows) == n and big.shape == (n + 300, 16) and torch.equal(big[:n], table)
    assert not bool(w[n:].any()) and not bool(big[n:].any())
    assert np.array_equal(bits(w[:n]), bits(RN.weights(ref['table'], ref['off'], ref['frame_ids'], DYN, bw, 0.25, 0.1)))


def test_table_from_lists(fx):
    """7: the fixture's lists -> the reference's own table (get_rays) and weights, and the restatement bit for bit"""
    Tn, N, P, H, W = [int(v) for v in fx['shape']]
    off = fx['view_off']
    frame_ids = [0] * N + [1] * N
    dyn = fx['dynamic_class']
    args = (T(fx['depth_list']), T(fx['seg_list']), [int(v) for v in off], T(fx['frames']), T(fx['c2w']), T(fx['K']))
    table, view_off, counts = ops.ray_table(args[4], args[5], args[3], lists=args[:3])
    assert np.array_equal(view_off.cpu().numpy(), off)
    _check_table(table, fx['table'], 'lists vs the reference')
    dl = [fx['depth_list'][off[v]:off[v + 1]] for v in range(Tn * N)]
    sl = [fx['seg_list'][off[v]:off[v + 1]] for v in range(Tn * N)]
    mine = RN.stage_b(dl, sl, fx['frames'], None, fx['c2w'], fx['K'], H, W)
    _check_table(table, mine, 'lists vs the restatement')
    assert np.array_equal(counts.cpu().numpy(), RN.class_counts(mine))
    time_ids = {0: list(range(N)), 1: list(range(N, 2 * N))}
    _, w, _ = R.generate_rays_from_labels(*args, max_ray_nums=100, time_ids=time_ids, dynamic_class=torch.from_numpy(dyn), return_weights=True)
    np.testing.assert_allclose(w.cpu().numpy(), fx['weights_batch'], rtol=1e-5)
    assert np.array_equal(bits(w), bits(RN.weights(mine, off, frame_ids, dyn)))
    adj, wd = [float(v) for v in fx['weight_adj_dyn']]
    rays, w2, sel = R.generate_rays_from_labels(*args, max_ray_nums=100, time_ids=time_ids, dynamic_class=torch.from_numpy(dyn),
                                                balance_weight=T(fx['balance_weight']), weight_adj=adj, weight_dyn=wd, return_weights=True)
    np.testing.assert_allclose(w2.cpu().numpy(), fx['weights_given'], rtol=1e-6)
    assert np.array_equal(bits(w2), bits(RN.weights(mine, off, frame_ids, dyn, fx['balance_weight'], adj, wd)))
    assert rays.shape == (100, 16) and len(set(sel.cpu().tolist())) == 100 and torch.equal(rays, table[sel])
    # a depth row on a pixel no seg row touches reads the zero-filled map; a row outside the image gets class 0, colour 0
    d2, s2 = fx['depth_list'][:40].copy(), fx['seg_list'][:40].copy()
    s2[:, :2] = np.float32([3.5, 4.5])
    d2[7, :2] = np.float32([200.0, 7.0])
    t2, _, c2 = ops.ray_table(args[4][:1], args[5][:1], args[3], lists=(T(d2), T(s2), [0, 40]))
    t2 = t2.cpu().numpy()
    assert not t2[:, 3].any() and int(c2[0]) == 40 and not t2[7, 13:].any() and t2[7, 0] == 200.0 and t2[6, 13:].any()


def _all_kept_sample(P=700):
    """T = N = 1; every point back-projected from inside the image: all are kept"""
    S = RN.synthetic_sample(13, T=1, N=1, P=P, H=48, W=80, focal=40.0)
    rs = np.random.RandomState(5)
    pose = S['poses'][0]
    Minv, Kinv = np.linalg.inv(RN.chain_ideal(pose)), np.linalg.inv(pose[48:57].reshape(3, 3))
    d = rs.uniform(3.0, 40.0, P)
    cam = (Kinv @ np.stack([rs.uniform(2.5, 77.5, P) * d, rs.uniform(2.5, 45.5, P) * d, d])).T
    S['points'][0][:, :3] = (cam @ Minv[:3, :3].T + Minv[:3, 3]).astype(np.float32)
    return S


def test_edges(small):
    """8"""
    S, ref = small
    frames, c2w, K = T(S['frames']), T(ref['c2w']), T(ref['K'])
    time_ids = {0: [0, 1], 1: [2, 3]}
    # a view with no kept point (its points taken out of the sweep) and an empty sweep
    keep1, _ = RN.project(S['points'][0], S['poses'][1], S['H'], S['W'])
    S2 = dict(S, points=[S['points'][0][~keep1], S['points'][1][:0]], labels=[S['labels'][0][~keep1], S['labels'][1][:0]])
    ref2 = _reference(S2, [0, 0, 1, 1])
    assert list(np.diff(ref2['off'])[1:]) == [0, 0, 0] and ref2['off'][1] > 300
    dlist, slist, off = ops.sweep_pixel_labels([T(p) for p in S2['points']], [T(l) for l in S2['labels']], T(S2['poses']), (48, 80), T(RN.LUT))
    assert np.array_equal(off.cpu().numpy(), ref2['off']) and np.array_equal(bits(dlist), bits(np.concatenate(ref2['dl'])))
    table, w, _ = R.generate_rays_from_sweeps([T(p) for p in S2['points']], [T(l) for l in S2['labels']], frames, T(S2['poses']), c2w, K,
                                              time_ids=time_ids, dynamic_class=torch.tensor(DYN), label_lut=T(RN.LUT), return_weights=True)
    _check_table(table, ref2['table'], 'one view only')
    assert np.array_equal(bits(w), bits(RN.weights(ref2['table'], ref2['off'], [0, 0, 1, 1], DYN)))
    # nothing kept at all
    far = [T(np.full((5, 5), 1e6, np.float32)), T(np.zeros((0, 5), np.float32))]
    none = R.generate_rays_from_sweeps(far, [T(np.zeros(5, np.uint8)), T(np.zeros(0, np.uint8))], frames, T(S['poses']), c2w, K, time_ids=time_ids)
    assert none.shape == (0, 16)
    # every point kept
    S3 = _all_kept_sample()
    ref3 = _reference(S3, [0])
    assert ref3['off'][-1] == 700
    t3 = R.generate_rays_from_sweeps([T(S3['points'][0])], [T(S3['labels'][0])], T(S3['frames']), T(S3['poses']), T(ref3['c2w']), T(ref3['K']),
                                     time_ids={0: [0]}, label_lut=T(RN.LUT))
    _check_table(t3, ref3['table'], 'all kept')
    # capacity < R: n_rows reports R, the first `cap` rows are the table's, nothing outside the buffer is written
    n, cap, guard = int(ref['off'][-1]), 1000, 64
    sw = _sweeps(S)
    buf = torch.full(((cap + 2 * guard) * 16,), float('nan'), device=DEV)
    out = buf[guard * 16:(guard + cap) * 16].view(cap, 16)
    table, off, counts = ops.ray_table(c2w, K, frames, sweeps=sw, capacity=cap, out=out)
    assert table.data_ptr() == out.data_ptr() and int(off[-1]) == n > cap
    _check_table(table, ref['table'][:cap], 'capacity < R')
    assert bool(torch.isnan(buf[:guard * 16]).all()) and bool(torch.isnan(buf[(guard + cap) * 16:]).all())
    assert np.array_equal(counts.cpu().numpy(), RN.class_counts(ref['table'][:cap]))
    w = ops.ray_table_weights(table, off, [0, 0, 1, 1], DYN, counts=counts)
    want = RN.weights(ref['table'][:cap], np.minimum(ref['off'], cap), [0, 0, 1, 1], DYN)
    assert w.shape == (cap,) and np.array_equal(bits(w), bits(want))
    # max_ray_nums >= R: the whole table, the reference's shape; below R: a draw of distinct rows with positive weight
    full = R.generate_rays_from_sweeps(sw, None, frames, None, c2w, K, max_ray_nums=n, time_ids=time_ids, dynamic_class=torch.tensor(DYN))
    assert full.shape == (n, 16)
    _check_table(full, ref['table'], 'max_ray_nums >= R')
    g = torch.Generator(device=DEV).manual_seed(3)
    drawn, w, sel = R.generate_rays_from_sweeps(sw, None, frames, None, c2w, K, max_ray_nums=500, time_ids=time_ids,
                                                dynamic_class=torch.tensor(DYN), generator=g, return_weights=True)
    assert drawn.shape == (500, 16) and len(set(sel.cpu().tolist())) == 500 and bool((w[sel] > 0).all()) and torch.equal(drawn, full[sel])


def test_real_image_size():
    """9: one view of 900 x 1600 with P = 34 720: pixel indices past 2^16, 136 scan blocks, the owner table at its real load"""
    S = RN.synthetic_sample(17, T=1, N=1, P=34720, H=900, W=1600, focal=1266.0)
    ref = _reference(S, [0])
    n = int(ref['off'][-1])
    assert n > 3000 and (ref['table'][:, 1] * 1600 + ref['table'][:, 0]).max() > 2 ** 20
    pts, lab, frames = [T(S['points'][0])], [T(S['labels'][0])], T(S['frames'])
    dlist, slist, off = ops.sweep_pixel_labels(pts, lab, T(S['poses']), (900, 1600), T(RN.LUT))
    assert int(off[-1]) == n
    assert np.array_equal(bits(dlist), bits(ref['dl'][0])) and np.array_equal(bits(slist), bits(ref['sl'][0]))
    table, w, _ = R.generate_rays_from_sweeps(pts, lab, frames, T(S['poses']), T(ref['c2w']), T(ref['K']), time_ids={0: [0]},
                                              dynamic_class=torch.tensor(DYN), label_lut=T(RN.LUT), return_weights=True)
    assert _check_table(table, ref['table'], '900 x 1600')                       # every column bit-equal
    assert np.array_equal(bits(w), bits(RN.weights(ref['table'], ref['off'], [0], DYN)))
    assert ops.ray_scratch_bytes(1, 1, 34720) == 8 * 131072 + 4 * 136 + 8


def test_capacity_mode_under_capture():
    """10: one capture, replayed on a second sample with sweeps of other lengths and another kept count; nothing in the captured
    region synchronises (a synchronising call raises during capture)"""
    A = RN.synthetic_sample(21, T=2, N=2, P=3001, H=48, W=80, focal=40.0, lengths=[3001, 2800])
    B = RN.synthetic_sample(22, T=2, N=2, P=3001, H=48, W=80, focal=40.0, lengths=[2500, 3001])
    refs = [_reference(s, [0, 0, 1, 1]) for s in (A, B)]
    assert refs[0]['off'][-1] != refs[1]['off'][-1]
    cap, Pmax = 3000, 3001
    st = dict(points=torch.zeros(2, Pmax, 5, device=DEV), labels=torch.zeros(2, Pmax, dtype=torch.uint8, device=DEV),
              n_pts=torch.zeros(2, dtype=torch.int32, device=DEV), pose=torch.zeros(4, 57, dtype=torch.float64, device=DEV),
              frames=torch.zeros(4, 48, 80, 3, dtype=torch.uint8, device=DEV), c2w=torch.zeros(4, 4, 4, device=DEV), K=torch.zeros(4, 3, 3, device=DEV))
    frame_ids, dyn, lut = torch.tensor([0, 0, 1, 1], dtype=torch.int32, device=DEV), torch.tensor(DYN, dtype=torch.int32, device=DEV), T(RN.LUT)

    def load(S, ref):
        st['points'].zero_()
        for t in range(2):
            st['points'][t, :len(S['points'][t])] = T(S['points'][t])
            st['labels'][t, :len(S['labels'][t])] = T(S['labels'][t])
        st['n_pts'].copy_(torch.tensor([len(p) for p in S['points']], dtype=torch.int32))
        st['pose'].copy_(T(S['poses']))
        st['frames'].copy_(T(S['frames']))
        st['c2w'].copy_(T(ref['c2w']))
        st['K'].copy_(T(ref['K']))

    def run():
        sw = ops.RaySweeps(st['points'], st['labels'], st['pose'], lut, st['n_pts'])
        return R.generate_rays_from_sweeps(sw, None, st['frames'], None, st['c2w'], st['K'], time_ids=frame_ids, dynamic_class=dyn, capacity=cap)

    load(A, refs[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                            # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        table, w, n_rows = run()
    for S, ref in ((B, refs[1]), (A, refs[0])):
        load(S, ref)
        graph.replay()
        got = [x.clone() for x in (table, w, n_rows)]
        eager = run()
        n = int(ref['off'][-1])
        assert int(got[2]) == n == int(eager[2])
        assert torch.equal(got[0], eager[0]) and torch.equal(got[1], eager[1])
        _check_table(got[0][:min(n, cap)], ref['table'][:cap], 'replay')
        assert not bool(got[1][n:].any())


def test_determinism(small):
    """11"""
    S, ref = small
    out = []
    for _ in range(2):
        sw = _sweeps(S)
        table, off, counts = ops.ray_table(T(ref['c2w']), T(ref['K']), T(S['frames']), sweeps=sw, capacity=int(ref['off'][-1]) + 50)
        w = ops.ray_table_weights(table, off, [0, 0, 1, 1], DYN, counts=counts)
        out.append([x.cpu().numpy().tobytes() for x in (table, w, counts, off)])
    assert out[0] == out[1]


def test_pipeline_class():
    """12: three frames wanted; the neighbour at -1 belongs to another scene and falls back to the key sample"""
    S = RN.synthetic_sample(31, T=3, N=2, P=1500, H=48, W=80, focal=40.0, scenes=[0, 1, 0])
    entry = [dict(info=S['infos'][t], points=torch.from_numpy(S['points'][t]), point_labels=torch.from_numpy(S['labels'][t]),
                  frames=T(S['frames'][2 * t:2 * t + 2])) for t in range(3)]
    class_nums = np.arange(1, 18) * 1000
    tf = transforms.SweepsToRays(aux_frames=[-1, 1], class_nums=class_nums, dynamic_class=DYN, label_lut=RN.LUT, device=DEV)
    got = tf(dict(curr=S['infos'][0], ray_frames={0: entry[0], -1: entry[1], 1: entry[2]}))['rays']
    used = [0, 0, 2]
    infos = [S['infos'][t] for t in used]
    n = torch.as_tensor(class_nums, dtype=torch.float32)
    by_hand = R.generate_rays_from_sweeps(
        [T(S['points'][t]) for t in used], [T(S['labels'][t]) for t in used], T(np.concatenate([S['frames'][2 * t:2 * t + 2] for t in used])),
        transforms.compose_view_poses(infos, S['cam_names']), transforms.compose_sensor2keyegos(infos, S['cam_names']),
        torch.tensor([i['cams'][c]['cam_intrinsic'] for i in infos for c in S['cam_names']], dtype=torch.float32),
        time_ids={0: [0, 1], -1: [2, 3], 1: [4, 5]}, dynamic_class=torch.tensor(DYN), balance_weight=torch.exp(0.005 * (n.max() / n - 1)),
        label_lut=RN.LUT)
    assert got.shape[0] > 600 and torch.equal(got, by_hand)
    S2 = dict(S, infos=infos, points=[S['points'][t] for t in used], labels=[S['labels'][t] for t in used],
              frames=np.concatenate([S['frames'][2 * t:2 * t + 2] for t in used]), poses=RN.view_poses(infos, S['cam_names']))
    ref = _reference(S2, [0, 0, -1, -1, 1, 1])
    _check_table(got, ref['table'], 'pipeline')
    assert np.array_equal(bits(got[int(ref['off'][2]):int(ref['off'][4]), :4]), bits(got[:int(ref['off'][2]), :4]))    # the fallback frame repeats the key's labels
