"""tests/_pool_ref64.py must be trusted before it judges a kernel: the float64 restatement of the voxel pooling against the CPU
oracle and the reference's own stored results (to the fp32 rounding of those), against float64 torch autograd through an index_add
composition, and against the bilinear identity <og, F(d, f)> = <d, depth_grad> = <f, feat_grad>.  No GPU."""
import numpy as np
import pytest
import torch

import _pool_ref64 as R
from oracle import oracle as O


def _rand(seed, ranks, C):
    rs = np.random.RandomState(seed)
    depth = rs.random_sample(ranks.BN * ranks.D * ranks.HW).astype(np.float32)
    feat = rs.standard_normal((ranks.BN * ranks.HW, C)).astype(np.float32)
    og = rs.standard_normal((ranks.n_vox, C)).astype(np.float32)
    return depth, feat, og


def _profile(seed, BN, HW, D):
    """lengths 0 .. D with empty pixels, full pixels and everything between"""
    rs = np.random.RandomState(seed)
    ln = rs.randint(0, D + 1, (BN, HW))
    ln[rs.random_sample((BN, HW)) < 0.2] = 0
    ln[0, 0], ln[-1, -1] = D, 1
    return ln


def test_builder_obeys_the_operator_contract():
    D, HW, BN = 7, 13, 3
    ln = _profile(0, BN, HW, D)
    r = R.build_ranks(ln, D, 29, seed=1)
    assert r.ranks_depth.dtype == r.ranks_feat.dtype == r.ranks_bev.dtype == r.interval_starts.dtype == np.int32
    assert len(r.ranks_depth) == ln.sum() and len(np.unique(r.ranks_depth)) == len(r.ranks_depth)
    rd = r.ranks_depth.astype(np.int64)
    np.testing.assert_array_equal(r.ranks_feat, (rd // (D * HW)) * HW + rd % HW)         # the frustum layout
    np.testing.assert_array_equal(np.bincount(r.ranks_feat, minlength=BN * HW).reshape(BN, HW), ln)
    assert r.ranks_bev.min() >= 0 and r.ranks_bev.max() < 29 and np.all(np.diff(r.ranks_bev) >= 0)
    # forward intervals: one per occupied voxel, covering the points in order; ties in ranks_depth order (the stable sort)
    assert r.interval_lengths.sum() == len(rd) and np.all(r.interval_lengths > 0)
    np.testing.assert_array_equal(r.interval_starts, np.concatenate([[0], np.cumsum(r.interval_lengths)[:-1]]))
    for s, l in zip(r.interval_starts, r.interval_lengths):
        assert np.all(r.ranks_bev[s:s + l] == r.ranks_bev[s]) and np.all(np.diff(rd[s:s + l]) > 0)
    assert len(r.interval_starts) == len(np.unique(r.ranks_bev))
    # backward intervals: one per pixel with a point, lengths = the profile
    bd, bf, bb, st, lens = R.backward_intervals(r.ranks_depth, r.ranks_feat, r.ranks_bev)
    np.testing.assert_array_equal(lens, ln.reshape(-1)[ln.reshape(-1) > 0])
    assert np.all(np.diff(bf) >= 0) and sorted(zip(bd, bf, bb)) == sorted(zip(r.ranks_depth, r.ranks_feat, r.ranks_bev))
    # a voxel pool concentrates the points
    r2 = R.build_ranks(ln, D, 29, seed=1, vox_pool=[3, 28])
    assert set(np.unique(r2.ranks_bev)) == {3, 28}


def test_ref64_vs_oracle_and_stored_results_small(golden):
    """lss_small.npz: the oracle's fp32 forward / backward and the reference's stored bev_feat / depth_grad / feat_grad are all
    fp32 sums of the same products, so each lies within the derived bound of the float64 value."""
    g = golden('lss_small.npz')
    gc = {'x': list(g['grid_x']), 'y': list(g['grid_y']), 'z': list(g['grid_z']), 'depth': list(g['grid_depth'])}
    lower, interval, size = O.grid_infos(gc)
    rb, rd, rf, st, ln = O.voxel_pooling_prepare_v2(g['coor'], lower, interval, size)
    C = g['feat'].shape[2]
    feat = np.ascontiguousarray(g['feat'].transpose(0, 1, 3, 4, 2))
    og = np.ascontiguousarray(g['out_grad'].transpose(0, 2, 3, 4, 1))
    ref = R.pool_ref64(g['depth'], feat, og, rd, rf, rb)
    shape = (1, size[2], size[1], size[0], C)
    o_out = O.bev_pool_v2(g['depth'], feat, rd, rf, rb, shape, st, ln).transpose(0, 2, 3, 4, 1).reshape(-1, C)
    o_dg, o_fg = O.bev_pool_v2_backward(og, g['depth'], feat, rd, rf, rb)
    R.assert_within_bound('cpu small oracle out', o_out, ref.out, ref.n['out'], ref.S['out'])
    R.assert_within_bound('cpu small oracle depth_grad', o_dg, ref.depth_grad, ref.n['depth_grad'], ref.S['depth_grad'])
    R.assert_within_bound('cpu small oracle feat_grad', o_fg.reshape(-1, C), ref.feat_grad, ref.n['feat_grad'], ref.S['feat_grad'])
    R.assert_within_bound('cpu small stored bev_feat', g['bev_feat'].transpose(0, 2, 3, 4, 1).reshape(-1, C), ref.out,
                          ref.n['out'], ref.S['out'])
    R.assert_within_bound('cpu small stored depth_grad', g['depth_grad'], ref.depth_grad, ref.n['depth_grad'], ref.S['depth_grad'])
    R.assert_within_bound('cpu small stored feat_grad', g['feat_grad'].transpose(0, 1, 3, 4, 2).reshape(-1, C), ref.feat_grad,
                          ref.n['feat_grad'], ref.S['feat_grad'])
    # the reference's own unstable point order names the same points: same float64 sums
    ref2 = R.pool_ref64(g['depth'], feat, og, g['ranks_depth'], g['ranks_feat'], g['ranks_bev'])
    for a, b in zip(ref[:3], ref2[:3]):
        np.testing.assert_allclose(a, b, rtol=1e-14, atol=1e-300)
    assert ref.n['depth_grad'].max() == C and set(np.unique(ref.n['depth_grad'])) <= {0, C}
    assert ref.n['out'].sum() == len(rb) * C == ref.n['feat_grad'].sum()


def test_ref64_vs_known_answer(golden):
    """kat_bev_pool_v2.npz (bev_pool.py:145-176): loss = sum(out) -> out_grad of ones"""
    g = golden('kat_bev_pool_v2.npz')
    C = g['feat'].shape[-1]
    n_vox = g['out'].size // C
    og = np.ones((n_vox, C), np.float32)
    ref = R.pool_ref64(g['depth'], g['feat'], og, g['ranks_depth'], g['ranks_feat'], g['ranks_bev'])
    assert abs(ref.out.sum() - 4.4) < 1e-6
    R.assert_within_bound('cpu kat stored out', g['out'].transpose(0, 2, 3, 4, 1).reshape(-1, C), ref.out, ref.n['out'], ref.S['out'])
    R.assert_within_bound('cpu kat stored depth_grad', g['depth_grad'], ref.depth_grad, ref.n['depth_grad'], ref.S['depth_grad'])
    R.assert_within_bound('cpu kat stored feat_grad', g['feat_grad'].reshape(-1, C), ref.feat_grad, ref.n['feat_grad'],
                          ref.S['feat_grad'])
    o_out = O.bev_pool_v2(g['depth'], g['feat'], g['ranks_depth'], g['ranks_feat'], g['ranks_bev'], (1, 1, 2, 2, 2),
                          g['interval_starts'], g['interval_lengths'])
    o_dg, o_fg = O.bev_pool_v2_backward(og.reshape(1, 1, 2, 2, C), g['depth'], g['feat'], g['ranks_depth'], g['ranks_feat'],
                                        g['ranks_bev'])
    R.assert_within_bound('cpu kat oracle out', o_out.transpose(0, 2, 3, 4, 1).reshape(-1, C), ref.out, ref.n['out'], ref.S['out'])
    R.assert_within_bound('cpu kat oracle depth_grad', o_dg, ref.depth_grad, ref.n['depth_grad'], ref.S['depth_grad'])
    R.assert_within_bound('cpu kat oracle feat_grad', o_fg.reshape(-1, C), ref.feat_grad, ref.n['feat_grad'], ref.S['feat_grad'])


CASES = [(1, 1, 1, 1, 3), (2, 5, 7, 4, 11), (3, 88, 9, 32, 40), (2, 16, 33, 12, 5)]       # BN, D, HW, C, n_vox


@pytest.mark.parametrize('BN,D,HW,C,n_vox', CASES)
def test_ref64_vs_float64_autograd_and_bilinear_identity(BN, D, HW, C, n_vox):
    ranks = R.build_ranks(_profile(BN + D, BN, HW, D), D, n_vox, seed=C)
    depth, feat, og = _rand(5, ranks, C)
    ref = R.pool_ref64(depth, feat, og, ranks.ranks_depth, ranks.ranks_feat, ranks.ranks_bev)
    d = torch.from_numpy(depth).double().requires_grad_()
    f = torch.from_numpy(feat).double().requires_grad_()
    out = R.pool_torch64(d, f, ranks.ranks_depth, ranks.ranks_feat, ranks.ranks_bev, n_vox)
    (out * torch.from_numpy(og).double()).sum().backward()
    # float64 against float64: a few ulp of the terms' absolute sum
    for got, want, S in ((out.detach(), ref.out, ref.S['out']), (d.grad, ref.depth_grad, ref.S['depth_grad']),
                         (f.grad, ref.feat_grad, ref.S['feat_grad'])):
        err = np.abs(got.numpy() - want)
        assert np.all(err <= 2.0 ** -45 * S), float((err / np.maximum(S, 1e-300)).max())
    # untouched elements: exactly zero, no term counted
    assert np.all(ref.depth_grad[ref.n['depth_grad'] == 0] == 0) and np.all(ref.feat_grad[ref.n['feat_grad'] == 0] == 0)
    assert np.all(ref.out[ref.n['out'] == 0] == 0)
    # bilinear identity, each side a float64 sum of the same P * C products
    a = float((og.astype(np.float64) * ref.out).sum())
    b = float((depth.astype(np.float64) * ref.depth_grad).sum())
    c = float((feat.astype(np.float64) * ref.feat_grad).sum())
    scale = float((np.abs(og) * ref.S['out']).sum())
    assert abs(a - b) <= 1e-13 * scale and abs(a - c) <= 1e-13 * scale, (a, b, c, scale)
    # the counts: every point adds C terms to each of the three
    P = len(ranks.ranks_depth)
    assert ref.n['out'].sum() == ref.n['feat_grad'].sum() == ref.n['depth_grad'].sum() == P * C


def test_bound_notices_a_dropped_term_and_ignores_the_order():
    """the tolerance does its job on the CPU already: fp32 sums in two different orders pass, one dropped / doubled / misrouted
    term fails"""
    D, HW, BN, C, n_vox = 88, 6, 2, 32, 4
    ranks = R.build_ranks(np.full((BN, HW), D), D, n_vox, seed=3)           # 264 terms per voxel element
    depth, feat, og = _rand(6, ranks, C)
    rd, rf, rb = ranks.ranks_depth, ranks.ranks_feat, ranks.ranks_bev
    ref = R.pool_ref64(depth, feat, og, rd, rf, rb)

    def fp32(order):
        out = np.zeros((n_vox, C), np.float32)
        for i in order:
            out[rb[i]] = out[rb[i]] + (feat[rf[i]] * depth[rd[i]]).astype(np.float32)
        return out
    P = len(rd)
    fwd, rev = fp32(range(P)), fp32(range(P - 1, -1, -1))
    assert not np.array_equal(fwd, rev)
    for name, got in (('cpu fp32 point order', fwd), ('cpu fp32 reverse order', rev)):
        assert R.assert_within_bound(name, got, ref.out, ref.n['out'], ref.S['out']) < 0.5
    for order in (list(range(1, P)), [0] + list(range(P)), ):                # dropped, doubled
        ratio, _, n_out = R.worst_ratio(fp32(order), ref.out, ref.n['out'], ref.S['out'])
        assert n_out > 0 and ratio > 10
    bad = ref.out.copy()
    bad[[0, 1]] = bad[[1, 0]]                                               # misrouted rows
    assert R.worst_ratio(bad, ref.out, ref.n['out'], ref.S['out'])[2] > 0
    ln = np.full((BN, HW), D)                                               # a write where no term belongs
    ln[0, 0] = D - 1
    r2 = R.build_ranks(ln, D, n_vox, seed=3)
    ref2 = R.pool_ref64(depth, feat, og, r2.ranks_depth, r2.ranks_feat, r2.ranks_bev)
    bad = ref2.depth_grad.copy()
    bad[np.flatnonzero(ref2.n['depth_grad'] == 0)[0]] = 1e-30
    assert R.worst_ratio(bad, ref2.depth_grad, ref2.n['depth_grad'], ref2.S['depth_grad'])[1] == 1
