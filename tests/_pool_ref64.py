"""The Lift-Splat-Shoot voxel pooling (bev_pool_v2) and its gradient restated in float64 numpy -- the yardstick
pw_bev_pool_v2_forward / pw_bev_pool_v2_backward (csrc/pw_lss.hip, behind ops.bev_pool_v2 / ops.QuickCumsumCuda) answer to.

One frustum point i names a depth element ranks_depth[i], a feature row ranks_feat[i] and a voxel ranks_bev[i]:

    out[rb]        += feat[rf] * depth[rd]              (forward)
    depth_grad[rd]  = <out_grad[rb], feat[rf]>          (one point per depth element)
    feat_grad[rf]  += out_grad[rb] * depth[rd]

No intervals, no sorting, no kernel structure: np.add.at over the points in whatever order they come.  Next to every value the
reference returns what a tolerance needs: the number of summed products n and the float64 sum of their absolute values S.

THE BOUND (stated here once, used by every test of the pooling): an fp32 kernel that sums n rounded products in any order is
within  gamma_n * S  of the exact sum, gamma_n = n u / (1 - n u) with u = 2^-24; product and sum round separately where the
compiler does not fuse them, so the bound is doubled:

    |got - ref64| <= 2 (n + 2) 2^-24 S

and an element with S == 0 (no term, or only zero terms) must be exactly 0.0.  A dropped, doubled or misrouted term is of order
S / n and breaks this by five orders of magnitude; a different summation order does not.  Nothing here calls a project kernel."""
import collections

import numpy as np

U32 = 2.0 ** -24

PoolRef = collections.namedtuple('PoolRef', 'out depth_grad feat_grad n S')
# n and S are dicts keyed 'out', 'depth_grad', 'feat_grad', each of the shape of the value it describes


def bound(n, S):
    return 2.0 * (np.asarray(n, np.float64) + 2.0) * U32 * np.asarray(S, np.float64)


def pool_ref64(depth, feat, out_grad, ranks_depth, ranks_feat, ranks_bev):
    """depth (B*N*D*H*W,) [any shape, taken flat], feat (B*N*H*W, C) [leading dims flattened], out_grad (n_vox, C) [likewise]
    -> PoolRef.  out is (n_vox, C), depth_grad has depth's flat shape, feat_grad feat's (rows, C)."""
    C = feat.shape[-1]
    d = np.asarray(depth, np.float64).reshape(-1)
    f = np.asarray(feat, np.float64).reshape(-1, C)
    og = np.asarray(out_grad, np.float64).reshape(-1, C)
    rd, rf, rb = (np.asarray(r).astype(np.int64).reshape(-1) for r in (ranks_depth, ranks_feat, ranks_bev))
    assert len(rd) == len(rf) == len(rb)
    assert len(rd) == 0 or (rd.min() >= 0 and rd.max() < len(d) and rf.min() >= 0 and rf.max() < len(f)
                            and rb.min() >= 0 and rb.max() < len(og))
    assert len(np.unique(rd)) == len(rd), 'a depth element belongs to one frustum point'
    n, S = {}, {}
    # forward
    t = f[rf] * d[rd][:, None]
    out = np.zeros_like(og)
    S['out'] = np.zeros_like(og)
    np.add.at(out, rb, t)
    np.add.at(S['out'], rb, np.abs(t))
    n['out'] = np.broadcast_to(np.bincount(rb, minlength=len(og))[:, None], og.shape)
    # depth gradient: one dot product of C terms per point
    t = og[rb] * f[rf]
    dg = np.zeros_like(d)
    S['depth_grad'] = np.zeros_like(d)
    n['depth_grad'] = np.zeros(len(d), np.int64)
    np.add.at(dg, rd, t.sum(1))
    np.add.at(S['depth_grad'], rd, np.abs(t).sum(1))
    np.add.at(n['depth_grad'], rd, C)
    # feature gradient: one term per point of the pixel
    t = og[rb] * d[rd][:, None]
    fg = np.zeros_like(f)
    S['feat_grad'] = np.zeros_like(f)
    np.add.at(fg, rf, t)
    np.add.at(S['feat_grad'], rf, np.abs(t))
    n['feat_grad'] = np.broadcast_to(np.bincount(rf, minlength=len(f))[:, None], f.shape)
    return PoolRef(out, dg, fg, n, S)


def worst_ratio(got, ref, n, S):
    """(max err / bound over the elements with S > 0, number of elements with S == 0 that are not exactly 0.0, number of
    elements outside the bound).  Every element is looked at."""
    got = np.asarray(got, np.float64).reshape(-1)
    ref, S = np.asarray(ref, np.float64).reshape(-1), np.asarray(S, np.float64).reshape(-1)
    n = np.asarray(n).reshape(-1)
    assert got.shape == ref.shape == S.shape == n.shape, (got.shape, ref.shape, S.shape, n.shape)
    zero = S == 0
    bad_zero = int(np.count_nonzero(got[zero] != 0.0))
    err, b = np.abs(got - ref)[~zero], bound(n, S)[~zero]
    ratio = float((err / b).max()) if err.size else 0.0
    with np.errstate(invalid='ignore'):
        n_out = int(np.count_nonzero(~(err <= b)))            # a NaN counts as outside
    return ratio, bad_zero, n_out


def assert_within_bound(name, got, ref, n, S):
    """print the worst err / bound on a [parity] line (a record, not a threshold), then assert the bound element by element"""
    ratio, bad_zero, n_out = worst_ratio(got, ref, n, S)
    size = int(np.asarray(ref).size)
    print('[parity] %-58s worst err/bound %.3e over %d elements (%d with S == 0)' % (
        name, ratio, size, int(np.count_nonzero(np.asarray(S) == 0))))
    assert bad_zero == 0, (name, '%d elements without a term are not exactly 0.0' % bad_zero)
    assert n_out == 0, (name, '%d of %d elements outside 2 (n + 2) 2^-24 S, worst err/bound %.3e' % (n_out, size, ratio))
    return ratio


def softmax_link_bound(logits, ref, D):
    """(n, S) for the gradient at the DepthNet output x (rows, D + C, ...) [channel axis 1]: the C context channels receive
    feat_grad itself; a depth logit k of a pixel receives p_k (g_k - sum_j p_j g_j) with p = softmax(logits) and g = depth_grad,
    whose fully expanded terms have the absolute sum p_k (S_k + sum_j p_j S_j) and count D + the pooling's n.
    logits (rows, D, H, W) float64; ref.depth_grad viewed (rows, D, H, W); ref.feat_grad (rows, H, W, C)."""
    z = np.asarray(logits, np.float64)
    rows, _, H, W = z.shape
    e = np.exp(z - z.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    Sd = ref.S['depth_grad'].reshape(rows, D, H, W)
    nd = ref.n['depth_grad'].reshape(rows, D, H, W)
    S_logit = p * (Sd + (p * Sd).sum(1, keepdims=True))
    n_logit = D + np.broadcast_to(nd.max(1, keepdims=True), nd.shape)
    C = ref.feat_grad.shape[-1]
    S_ctx = ref.S['feat_grad'].reshape(rows, H, W, C).transpose(0, 3, 1, 2)
    n_ctx = ref.n['feat_grad'].reshape(rows, H, W, C).transpose(0, 3, 1, 2)
    return np.concatenate([n_logit, n_ctx], 1), np.concatenate([S_logit, S_ctx], 1)


def pool_torch64(depth, feat, ranks_depth, ranks_feat, ranks_bev, n_vox):
    """the forward as a float64 torch index_add composition (differentiable): depth flat, feat (rows, C) -> (n_vox, C)"""
    import torch
    rd, rf, rb = (torch.as_tensor(np.asarray(r).astype(np.int64)) for r in (ranks_depth, ranks_feat, ranks_bev))
    t = feat.double().reshape(-1, feat.shape[-1])[rf] * depth.double().reshape(-1)[rd][:, None]
    return torch.zeros(n_vox, feat.shape[-1], dtype=torch.float64).index_add(0, rb, t)


# ------------------------------------------------------------------------------------------------ synthetic ranks
Ranks = collections.namedtuple('Ranks', 'ranks_depth ranks_feat ranks_bev interval_starts interval_lengths BN D HW n_vox')


def _runs(keys):
    """(starts, lengths) of the runs of equal values in a sorted int array"""
    if len(keys) == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    cut = np.flatnonzero(np.diff(keys)) + 1
    starts = np.concatenate([[0], cut])
    return starts.astype(np.int32), np.diff(np.concatenate([starts, [len(keys)]])).astype(np.int32)


def build_ranks(lengths, D, n_vox, seed, vox_pool=None):
    """Synthetic ranks that obey the operator's contract.  lengths: (BN, HW) ints in 0 .. D -- how many of the D depth bins of
    every feature pixel fall inside the grid (the per-pixel interval length of the BACKWARD pass; 0 = a pixel without a point).
    Every kept (pixel, bin) pair is one point: ranks_depth = (bn D + d) HW + p occurs once, ranks_feat = bn HW + p is the function
    of it the frustum layout dictates, ranks_bev is drawn from 0 .. n_vox - 1 (from `vox_pool` when given: few voxels -> long
    forward segments).  The arrays come back sorted by ranks_bev, ties in ranks_depth order, with the forward intervals, exactly
    as ops.lss_ranks returns them (all int32)."""
    lengths = np.asarray(lengths, np.int64)
    BN, HW = lengths.shape
    assert lengths.min() >= 0 and lengths.max() <= D
    rs = np.random.RandomState(seed)
    rd, rf = [], []
    for bn in range(BN):
        for p in range(HW):
            bins = np.sort(rs.permutation(D)[:lengths[bn, p]])
            rd.append((bn * D + bins) * HW + p)
            rf.append(np.full(len(bins), bn * HW + p, np.int64))
    rd, rf = np.concatenate(rd), np.concatenate(rf)
    o = np.argsort(rd, kind='stable')
    rd, rf = rd[o], rf[o]
    pool = np.arange(n_vox) if vox_pool is None else np.asarray(vox_pool)
    rb = pool[rs.randint(0, len(pool), len(rd))]
    o = np.argsort(rb, kind='stable')
    rd, rf, rb = rd[o].astype(np.int32), rf[o].astype(np.int32), rb[o].astype(np.int32)
    st, ln = _runs(rb)
    return Ranks(rd, rf, rb, st, ln, BN, D, HW, n_vox)


def backward_intervals(ranks_depth, ranks_feat, ranks_bev):
    """what bev_pool.py:47-57 hands the backward kernel: the points re-sorted (stably) by feature pixel and one interval per
    pixel that has a point -> (ranks_depth, ranks_feat, ranks_bev, interval_starts, interval_lengths), int32"""
    o = np.argsort(np.asarray(ranks_feat), kind='stable')
    rd, rf, rb = (np.ascontiguousarray(np.asarray(r)[o], np.int32) for r in (ranks_depth, ranks_feat, ranks_bev))
    st, ln = _runs(rf)
    return rd, rf, rb, st, ln
