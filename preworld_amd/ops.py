"""Functional wrappers over the C ABI for torch tensors resident in HBM.

torch is plumbing here: device memory, the current HIP stream and autograd glue.
All arithmetic happens in libpreworld_hip.so.  Names and argument order follow the
reference operators these replace (cited per function, paths relative to the reference).
"""
import ctypes
import functools
import os

import numpy as np
import torch

from . import _lib

_i32 = torch.int32
_f32 = torch.float32
RNG_ROW = _lib.PW['PW_RNG_ROW']       # int32 per range slot


def _host3(vals):
    return (ctypes.c_float * 3)(*[float(v) for v in vals])


def _slice(t):
    """a destination / residual that may be a channel slice: its layout was validated by _row_stride / _rows (or against the strides
    the call passes) and goes to the kernel as a row stride"""
    return _lib.strided(t) if t is not None else None


def _f32_typed(grid):
    """a contiguous bf16 attribute grid for a `const float* grid` parameter (the kernel is told by its grid_bf16 flag)"""
    return grid.view(-1).view(_f32) if grid.dtype == torch.bfloat16 else grid


def _workspace(nbytes, device):
    # torch's caching allocator returns >=512-byte aligned blocks
    return torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=device)


def copy_many(dsts, srcs):
    """dst[i].copy_(src[i]) for lists of same-shaped contiguous device tensors in ONE launch (pw_copy_many) -- a sample's inputs going
    into the static buffers of a captured step are 15 small copies, mostly launch latency as separate kernels"""
    n = len(dsts)
    if n != len(srcs):
        raise _lib.PreworldHipError('copy_many: %d destinations, %d sources' % (n, len(srcs)))
    for d, s_ in zip(dsts, srcs):
        if d.shape != s_.shape or d.dtype != s_.dtype or not (d.is_contiguous() and s_.is_contiguous() and d.is_cuda and s_.is_cuda):
            raise _lib.PreworldHipError('copy_many: tensors must be contiguous device tensors of equal shape and dtype')
    if n == 0:
        return
    B = (ctypes.c_size_t * n)(*[d.numel() * d.element_size() for d in dsts])
    _lib.call('pw_copy_many', _lib.table(srcs), _lib.table(dsts), B, n, _lib.STREAM)


def device_info():
    cu = ctypes.c_int(0)
    lds = ctypes.c_int(0)
    name = ctypes.create_string_buffer(64)
    _lib.call('pw_device_info', ctypes.byref(cu), ctypes.byref(lds), name, 64)
    return dict(cu_count=cu.value, lds_bytes_per_cu=lds.value, arch=name.value.decode())


# ------------------------------------------------------------------------------ LSS geometry
def lss_camera_matrices(sensor2ego, cam2imgs, post_rots):
    """inverse(post_rots), sensor2ego[:3,:3] @ inverse(cam2imgs), sensor2ego[:3,3]
    (mmdet3d/models/necks/view_transformer.py:141-150).  Inputs (B,N,4,4),(B,N,3,3),(B,N,3,3)."""
    B, N = sensor2ego.shape[:2]
    s = sensor2ego.contiguous().float()
    k = cam2imgs.contiguous().float()
    r = post_rots.contiguous().float()
    dev = s.device
    ipr = torch.empty(B, N, 3, 3, device=dev, dtype=_f32)
    comb = torch.empty(B, N, 3, 3, device=dev, dtype=_f32)
    tr = torch.empty(B, N, 3, device=dev, dtype=_f32)
    _lib.call('pw_lss_camera_matrices', B * N, s, k, r, ipr, comb, tr, _lib.STREAM)
    return ipr, comb, tr


def lss_voxel_index(frustum, inv_post_rot, post_trans, combine, trans, bda, lower, interval,
                    grid_size, B, N, return_coor=False):
    """get_lidar_coor + the voxel-id half of voxel_pooling_prepare_v2
    (view_transformer.py:114-153, :226-245).  Returns int32 voxel id per frustum point (-1 =
    outside) and, optionally, the reference's coor tensor (B,N,D,H,W,3)."""
    D, H, W, _ = frustum.shape
    dev = frustum.device
    vox = torch.empty(B * N * D * H * W, device=dev, dtype=_i32)
    coor = torch.empty(B, N, D, H, W, 3, device=dev, dtype=_f32) if return_coor else None
    _lib.call('pw_lss_voxel_index', B, N, D, H, W, frustum, inv_post_rot, post_trans, combine, trans, bda, _host3(lower),
              _host3(interval), int(grid_size[0]), int(grid_size[1]), int(grid_size[2]), vox, coor, _lib.STREAM)
    return (vox, coor) if return_coor else vox


LONG_SEGMENT = 64   # voxels holding more points than this are pooled by whole waves


class VoxelSort:
    """Result of the device counting sort over voxel ids (all tensors stay on the GPU)."""
    __slots__ = ('seg_start', 'order', 'order_feat', 'long_list', 'n_long', 'n_keys')

    def __init__(self, seg_start, order, order_feat, long_list, n_long, n_keys):
        self.seg_start, self.order, self.order_feat = seg_start, order, order_feat
        self.long_list, self.n_long, self.n_keys = long_list, n_long, n_keys


def segment_sort(keys, n_keys, aux_div=0, aux_mod=0, long_threshold=0):
    """Stable counting sort of indices by int32 key (key<0 dropped).
    Returns VoxelSort(seg_start int32[n_keys+1], order int32[n], order_feat, long_list, n_long)."""
    n = keys.numel()
    dev = keys.device
    nbytes = _lib.call_size('pw_segment_sort_workspace_bytes', n, n_keys)
    ws = _workspace(nbytes, dev)
    seg_start = torch.empty(n_keys + 1, device=dev, dtype=_i32)
    order = torch.empty(n, device=dev, dtype=_i32)
    aux = torch.empty(n, device=dev, dtype=_i32) if aux_div else None
    ll = torch.empty(n // (long_threshold + 1) + 1, device=dev, dtype=_i32) if long_threshold else None
    nl = torch.empty(1, device=dev, dtype=_i32) if long_threshold else None
    _lib.call('pw_segment_sort', n, n_keys, keys, ws, nbytes, seg_start, order, aux_div, aux_mod, aux, long_threshold, ll, nl,
              _lib.STREAM)
    return VoxelSort(seg_start, order, aux, ll, nl, n_keys)


def lss_ranks(seg_start, order, n_voxels, D, HW):
    """Expand a voxel sort into the reference's (ranks_bev, ranks_depth, ranks_feat,
    interval_starts, interval_lengths) -- view_transformer.py:246-261.  One D2H sync (the
    reference's boolean-mask indexing syncs several times)."""
    dev = seg_start.device
    n = order.numel()
    nbytes = _lib.call_size('pw_lss_ranks_workspace_bytes', n_voxels)
    ws = _workspace(nbytes, dev)
    rb = torch.empty(n, device=dev, dtype=_i32)
    rd = torch.empty(n, device=dev, dtype=_i32)
    rf = torch.empty(n, device=dev, dtype=_i32)
    nmax = min(n, n_voxels)
    st = torch.empty(nmax, device=dev, dtype=_i32)
    ln = torch.empty(nmax, device=dev, dtype=_i32)
    counts = torch.empty(2, device=dev, dtype=_i32)
    _lib.call('pw_lss_ranks', n_voxels, seg_start, order, D, HW, ws, nbytes, rb, rd, rf, st, ln, counts, _lib.STREAM)
    kept, ni = counts.tolist()
    if kept == 0:
        return None, None, None, None, None
    return rb[:kept], rd[:kept], rf[:kept], st[:ni], ln[:ni]


def bev_pool_dense(depth, feat, vs, out=None, out_h2=False):
    """Write-once dense pooling.  depth (B,N,D,H,W) flat, feat (B,N,H,W,C), vs = VoxelSort built
    with aux_div=D*H*W, aux_mod=H*W  ->  (n_voxels, C) fp32, or (out_h2=True) the same sums as an ops.H2 under a new
    range slot (or under `out`'s when an ops.H2 is passed)."""
    C = feat.shape[-1]
    if vs.order_feat is None:
        raise _lib.PreworldHipError('bev_pool_dense needs a VoxelSort built with aux_div/aux_mod')
    if out is None:
        out = torch.empty(vs.n_keys, C, device=feat.device, dtype=_f32)
    orng = None
    if out_h2:
        out, orng = _out_h2(out, feat.device)
    _lib.call('pw_bev_pool_dense', depth, feat, vs.seg_start, vs.order, vs.order_feat, vs.n_keys, C,
              LONG_SEGMENT if vs.long_list is not None else 0, vs.long_list, vs.n_long, out, int(bool(out_h2)), orng, _lib.STREAM)
    return H2(out, orng) if out_h2 else out


def lss_lift_pool(frustum, sensor2ego, cam2imgs, post_rots, post_trans, bda, lower, interval, grid_size, depth, feat,
                  out=None, out_h2=False):
    """get_lidar_coor + voxel_pooling_prepare_v2 + bev_pool_v2 forward of one batch of frames in one call (inference, C == 32;
    view_transformer.py:114-153, :203-261, bev_pool_cuda.cu:21-48): the same bits as lss_camera_matrices -> lss_voxel_index ->
    segment_sort -> bev_pool_dense in 5 launches.  depth (B,N,D,H,W), feat (B,N,H,W,C) fp32; returns (n_voxels, C) fp32 or an
    ops.H2 (out_h2).  (A voxel-driven gather form was built and measured in round 5 -- same bits, 1.2 x instead of 2.0 x the
    algorithmic HBM bytes, but instruction-bound at 2-3 x the time: profiles/r05_lss_gather_experiment.md, commit 69d8f73.)"""
    B, N = sensor2ego.shape[:2]
    D, H, W, _ = frustum.shape
    C = feat.shape[-1]
    dev = feat.device
    n_vox = B * int(grid_size[0]) * int(grid_size[1]) * int(grid_size[2])
    if out is None:
        out = torch.empty(n_vox, C, device=dev, dtype=_f32)
    orng = None
    if out_h2:
        out, orng = _out_h2(out, dev)
    nbytes = _lib.call_size('pw_lss_lift_pool_workspace_bytes', B * N * D * H * W, n_vox, B * N)
    ws = _workspace(nbytes, dev)
    f = lambda t: t.contiguous().float()
    _lib.call('pw_lss_lift_pool', B, N, D, H, W, frustum, f(sensor2ego), f(cam2imgs), f(post_rots), f(post_trans), f(bda),
              _host3(lower), _host3(interval), int(grid_size[0]), int(grid_size[1]), int(grid_size[2]), depth, feat, C, ws, nbytes,
              out, int(bool(out_h2)), orng, _lib.STREAM)
    return H2(out, orng) if out_h2 else out


# ------------------------------------------------------------------------------ bev_pool_v2
def bev_pool_v2_forward(depth, feat, out, ranks_depth, ranks_feat, ranks_bev, interval_lengths,
                        interval_starts):
    """Same call as bev_pool_v2_ext.bev_pool_v2_forward
    (mmdet3d/ops/bev_pool_v2/src/bev_pool.cpp:30-57): out (B,Z,Y,X,C) pre-zeroed, in/out;
    interval_lengths BEFORE interval_starts."""
    _lib.call('pw_bev_pool_v2_forward', depth, feat, out, ranks_depth, ranks_feat, ranks_bev, interval_lengths, interval_starts,
              feat.shape[-1], interval_lengths.numel(), _lib.STREAM)


def bev_pool_v2_backward(out_grad, depth_grad, feat_grad, depth, feat, ranks_depth, ranks_feat,
                         ranks_bev, interval_lengths, interval_starts):
    """Same call as bev_pool_v2_ext.bev_pool_v2_backward (bev_pool.cpp:74-104)."""
    _lib.call('pw_bev_pool_v2_backward', out_grad, depth_grad, feat_grad, depth, feat, ranks_depth, ranks_feat, ranks_bev,
              interval_lengths, interval_starts, out_grad.shape[-1], interval_lengths.numel(), _lib.STREAM)


class QuickCumsumCuda(torch.autograd.Function):
    """Drop-in for mmdet3d/ops/bev_pool_v2/bev_pool.py:11-83 (same name, same signature)."""

    @staticmethod
    def forward(ctx, depth, feat, ranks_depth, ranks_feat, ranks_bev, bev_feat_shape,
                interval_starts, interval_lengths):
        ranks_bev = ranks_bev.int()
        depth = depth.contiguous().float()
        feat = feat.contiguous().float()
        ranks_depth = ranks_depth.contiguous().int()
        ranks_feat = ranks_feat.contiguous().int()
        interval_lengths = interval_lengths.contiguous().int()
        interval_starts = interval_starts.contiguous().int()
        out = feat.new_zeros(bev_feat_shape)
        bev_pool_v2_forward(depth, feat, out, ranks_depth, ranks_feat, ranks_bev, interval_lengths,
                            interval_starts)
        ctx.save_for_backward(ranks_bev, depth, feat, ranks_feat, ranks_depth)
        return out

    @staticmethod
    def backward(ctx, out_grad):
        ranks_bev, depth, feat, ranks_feat, ranks_depth = ctx.saved_tensors
        n_pix = feat.numel() // feat.shape[-1]
        # re-sort by feat pixel (bev_pool.py:47-57) with the same device counting sort
        vs = segment_sort(ranks_feat.contiguous(), n_pix)
        seg_start = vs.seg_start
        order = vs.order[:ranks_feat.numel()].long()
        rf, rd, rb = ranks_feat[order].contiguous(), ranks_depth[order].contiguous(), \
            ranks_bev[order].contiguous()
        lens = seg_start[1:] - seg_start[:-1]
        nz = lens > 0
        interval_starts_bp = seg_start[:-1][nz].contiguous()
        interval_lengths_bp = lens[nz].contiguous()
        depth_grad = depth.new_zeros(depth.shape)
        feat_grad = feat.new_zeros(feat.shape)
        bev_pool_v2_backward(out_grad.contiguous(), depth_grad, feat_grad, depth, feat, rd, rf, rb,
                             interval_lengths_bp, interval_starts_bp)
        return depth_grad, feat_grad, None, None, None, None, None, None


def bev_pool_v2(depth, feat, ranks_depth, ranks_feat, ranks_bev, bev_feat_shape, interval_starts,
                interval_lengths):
    """mmdet3d/ops/bev_pool_v2/bev_pool.py:86-92.  Returns (B,C,Z,Y,X); unlike the reference
    the permute is a stride view of the channels-last buffer (no 82 MB copy)."""
    x = QuickCumsumCuda.apply(depth, feat, ranks_depth, ranks_feat, ranks_bev, bev_feat_shape,
                              interval_starts, interval_lengths)
    return x.permute(0, 4, 1, 2, 3)


# ------------------------------------------------------------------------------ conv3d
def pack_conv_weight(w, cout_total=None):
    """torch Conv3d weight (Cout, Cin, k, k, k) -> the MFMA operand order documented in
    include/preworld_hip.h: float[Cin/32][k^3][cout_total/32][4 pieces][64 lanes][4] with
    wpk[ch][tap][nt][q][h*32+j][e] = w[nt*32+j][ch*32+h*16+4*q+e][tap]; columns >= Cout are zero."""
    Cout, Cin, k = w.shape[0], w.shape[1], w.shape[2]
    if Cin % 32:
        raise _lib.PreworldHipError('Cin must be a multiple of 32, got %d' % Cin)
    if cout_total is None:
        cout_total = (Cout + 31) // 32 * 32
    taps = k ** 3
    wp = w.new_zeros(cout_total, Cin, taps)
    wp[:Cout] = w.reshape(Cout, Cin, taps)
    nt, nch = cout_total // 32, Cin // 32
    wp = wp.view(nt, 32, nch, 2, 4, 4, taps)            # (nt, j, ch, h, q, e, tap): s = 4 q + e
    wp = wp.permute(2, 6, 0, 4, 3, 1, 5).contiguous()   # (ch, tap, nt, q, h, j, e): piece-major, a piece = 64 lanes x 16 B
    return wp.view(nch, taps, nt, 64, 16).float().contiguous()


def pack_conv_weights_concat(ws):
    """Concatenate several convs over the SAME input along packed output columns, each padded
    to a multiple of 32 columns (conv1 + downsample of a BasicBlock3D share one pass)."""
    return torch.cat([pack_conv_weight(w) for w in ws], dim=2).contiguous()


def fold_bn(bn_weight, bn_bias, running_mean, running_var, eps=1e-5, conv_bias=None):
    """BatchNorm(eval) -> per-channel (scale, bias): y = conv*scale + bias."""
    inv = 1.0 / torch.sqrt(running_var.float() + eps)
    scale = bn_weight.float() * inv if bn_weight is not None else inv
    bias = (bn_bias.float() if bn_bias is not None else 0) - running_mean.float() * scale
    if conv_bias is not None:
        bias = bias + conv_bias.float() * scale
    return scale.contiguous(), bias.contiguous()


def _pad32(v, fill):
    n = v.numel()
    n32 = (n + 31) // 32 * 32
    if n32 == n:
        return v.contiguous()
    out = v.new_full((n32,), fill)
    out[:n] = v
    return out


def _row_stride(t, shape, name):
    """t must be (B,Do,Ho,Wo,c) laid out as a channel slice of a dense channels-last buffer:
    strides (Do*Ho*Wo*ld, Ho*Wo*ld, Wo*ld, ld, 1).  Returns ld."""
    if not t.is_cuda or t.dtype != _f32 or tuple(t.shape) != tuple(shape):
        raise _lib.PreworldHipError('%s must be a float32 device tensor of shape %s' % (name, tuple(shape)))
    B, Do, Ho, Wo, c = shape
    ld, below = c, 1                      # the stride of a size-1 axis is arbitrary: take ld from the innermost axis > 1
    for i in (3, 2, 1, 0):
        if shape[i] > 1:
            ld = t.stride(i) // below if t.stride(i) % below == 0 else -1
            break
        below *= shape[i]
    want = (Do * Ho * Wo * ld, Ho * Wo * ld, Wo * ld, ld, 1)
    ok = ld >= c and all(t.stride(i) == want[i] or t.shape[i] == 1 for i in range(5))
    if not ok:
        raise _lib.PreworldHipError('%s must be dense or a channel slice of a dense channels-last buffer' % name)
    return ld


def conv3d_ndhwc(x, wpk, scale=None, bias=None, residual=None, cout0=None, cout1=0, ksize=3,
                 stride=1, relu0=False, relu1=False, algo=0, out0=None, out1=None):
    """x (B,D,H,W,Cin) channels-last -> y0 (B,Do,Ho,Wo,cout0) [, y1 (B,Do,Ho,Wo,cout1)].
    scale/bias: per packed column (length cout_total, see include/preworld_hip.h).
    out0 / out1 may be channel slices of a wider channels-last buffer (e.g. buf[..., 32:64]); a
    residual then has to share out0's layout (it may BE out0: each element is read, then written)."""
    B, D, H, W, Cin = x.shape
    nch, taps, nt = wpk.shape[:3]
    cout_total = nt * 32
    if cout0 is None:
        cout0 = cout_total
    pad = (ksize - 1) // 2
    Do = (D + 2 * pad - ksize) // stride + 1
    Ho = (H + 2 * pad - ksize) // stride + 1
    Wo = (W + 2 * pad - ksize) // stride + 1
    y0 = out0 if out0 is not None else torch.empty(B, Do, Ho, Wo, cout0, device=x.device, dtype=_f32)
    ld0 = _row_stride(y0, (B, Do, Ho, Wo, cout0), 'y0')
    y1, ld1 = None, 0
    if cout1:
        y1 = out1 if out1 is not None else torch.empty(B, Do, Ho, Wo, cout1, device=x.device, dtype=_f32)
        ld1 = _row_stride(y1, (B, Do, Ho, Wo, cout1), 'y1')
    if residual is not None and _row_stride(residual, (B, Do, Ho, Wo, cout0), 'residual') != ld0:
        raise _lib.PreworldHipError('residual must have the same row stride as y0')
    if scale is not None and scale.numel() != cout_total:
        raise _lib.PreworldHipError('scale must have cout_total=%d entries' % cout_total)
    if bias is not None and bias.numel() != cout_total:
        raise _lib.PreworldHipError('bias must have cout_total=%d entries' % cout_total)
    if nch * 32 != Cin or taps != ksize ** 3:
        raise _lib.PreworldHipError('packed weight does not match Cin/ksize')
    _lib.call('pw_conv3d_ndhwc', x, wpk, scale, bias, _slice(residual), _slice(y0), _slice(y1), B, D, H, W, Cin, cout_total, cout0,
              cout1, ld0, ld1, ksize, stride, int(relu0), int(relu1), algo, _lib.STREAM)
    return (y0, y1) if cout1 else y0


_WINO_G = ((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0))


def pack_conv_weight_wino(w, cout_total=None):
    """torch Conv3d weight (Cout, Cin, 3, 3, 3) -> Winograd F(2,3)^3 transform-domain weights in the
    operand order of pw_conv3d_wino: float[Cin/32][64][cout_total/16][64][8] (include/preworld_hip.h).
    The transform U = G w G^T along d, h, w is done in float64 and rounded once."""
    Cout, Cin = w.shape[:2]
    if tuple(w.shape[2:]) != (3, 3, 3) or Cin % 32:
        raise _lib.PreworldHipError('pack_conv_weight_wino expects (Cout, 32k, 3, 3, 3)')
    if cout_total is None:
        cout_total = (Cout + 31) // 32 * 32
    G = torch.tensor(_WINO_G, dtype=torch.float64, device=w.device)
    U = torch.einsum('ia,jb,kc,oeabc->oeijk', G, G, G, w.double())           # (Cout, Cin, 4, 4, 4)
    Up = U.new_zeros(cout_total, Cin, 64)
    Up[:Cout] = U.reshape(Cout, Cin, 64)
    n16, nch = cout_total // 16, Cin // 32
    Up = Up.view(n16, 16, nch, 4, 8, 64)                   # (n16, j, ch, g, s, p)
    Up = Up.permute(2, 5, 0, 3, 1, 4).contiguous()         # (ch, p, n16, g, j, s)
    return Up.view(nch, 64, n16, 64, 8).float().contiguous()


def pack_conv_weights_wino_concat(ws):
    """conv1 + downsample of a BasicBlock3D over the same input: each padded to a multiple of 32 columns."""
    return torch.cat([pack_conv_weight_wino(w) for w in ws], dim=2).contiguous()


def conv3d_wino(x, uwpk, scale=None, bias=None, residual=None, cout0=None, cout1=0, relu0=False, relu1=False,
                out0=None, out1=None):
    """3x3x3 stride-1 pad-1 conv by Winograd F(2x2x2,3x3x3) (pw_conv3d_wino): same contract as
    conv3d_ndhwc(ksize=3, stride=1) with weights from pack_conv_weight_wino."""
    B, D, H, W, Cin = x.shape
    nch, npts, n16 = uwpk.shape[:3]
    cout_total = n16 * 16
    if npts != 64 or nch * 32 != Cin or cout_total % 32:
        raise _lib.PreworldHipError('packed Winograd weight does not match the input')
    if cout0 is None:
        cout0 = cout_total
    y0 = out0 if out0 is not None else torch.empty(B, D, H, W, cout0, device=x.device, dtype=_f32)
    ld0 = _row_stride(y0, (B, D, H, W, cout0), 'y0')
    y1, ld1 = None, 0
    if cout1:
        y1 = out1 if out1 is not None else torch.empty(B, D, H, W, cout1, device=x.device, dtype=_f32)
        ld1 = _row_stride(y1, (B, D, H, W, cout1), 'y1')
    if residual is not None and _row_stride(residual, (B, D, H, W, cout0), 'residual') != ld0:
        raise _lib.PreworldHipError('residual must have the same row stride as y0')
    if scale is not None and scale.numel() != cout_total:
        raise _lib.PreworldHipError('scale must have cout_total=%d entries' % cout_total)
    if bias is not None and bias.numel() != cout_total:
        raise _lib.PreworldHipError('bias must have cout_total=%d entries' % cout_total)
    _lib.call('pw_conv3d_wino', x, uwpk, scale, bias, _slice(residual), _slice(y0), _slice(y1), B, D, H, W, Cin, cout_total, cout0,
              cout1, ld0, ld1, int(relu0), int(relu1), _lib.STREAM)
    return (y0, y1) if cout1 else y0


# ------------------------------------------------------------------------------ split-fp16 ("h2") path
class RangeCtx:
    """Activation ranges of the split-fp16 path (include/preworld_hip.h "RANGE SLOTS").

    fp16 has 5 exponent bits, the reference's fp32 activations 8 (backbones/resnet.py:88-123 is plain Conv3d): an h2 tensor
    stores value / 2^e with a per-tensor exponent e kept in a device-resident *range slot* (int32[2] = [e, bit pattern of the
    largest |value| written]).  A RangeCtx owns a table of slots.  Producers take the next slot in CALL ORDER
    (`new_slot`), so the i-th h2 tensor of a deterministic forward pass always maps to slot i and its exponent persists from
    one pass to the next; kernels read the exponents from the table itself, so a captured hipGraph follows later updates.

    `ranged(fn)` is the calibration loop: run the pass, read the recorded maxima back (one small D2H copy), move every
    exponent whose tensor left the comfortable window, and repeat until nothing moves -- typically two passes on a cold
    table, one afterwards.  `check()` is the cheap steady-state test (hard window) a graph replay is followed by."""
    TARGET = 12          # ideal exponent puts the largest magnitude in [2^12, 2^13) stored units
    SETTLE_LO, SETTLE_HI = 8, 15      # calibration accepts a stored maximum in [2^8, 2^15)
    HARD_LO, HARD_HI = 6, 65504.0     # steady state accepts [2^6, 65504]

    def __init__(self, device, n_slots=128):
        # a slot = RNG_ROW int32: [exponent, folded maximum, ..., 1 024 partial maxima] (include/preworld_hip.h "RANGE SLOTS")
        self.tab = torch.zeros(n_slots, RNG_ROW, dtype=_i32, device=device)
        self.compact = torch.zeros(n_slots, 2, dtype=_i32, device=device)      # [exponent, maximum] pairs, written by fold()
        self.sticky = torch.zeros(4, dtype=_i32, device=device)                 # audit(): [bad slots, bad passes, passes audited, -]
        self.n = 0
        self.device = torch.device(device)
        self._jumped = set()             # slots whose last settle() step was the + 12 of a non-finite maximum

    def begin(self):
        """start of a pass: slots are handed out from 0 again, recorded maxima are cleared (a kernel, capturable)"""
        self.n = 0
        self.tab[:, 1].zero_()

    def fold(self):
        """end of a pass: fold the partial maxima the kernels raised into the slots and refresh `compact` (one small launch)"""
        _lib.call('pw_rng_fold', self.tab, self.tab.shape[0], self.compact, _lib.STREAM)

    def audit(self):
        """after fold(): the hard-window test of check() on the device, accumulated in `sticky` (pw_rng_audit) -- capturable, so
        every replay of a graph is tested without the host waiting for it; read the verdict with audited()"""
        _lib.call('pw_rng_audit', self.compact, self.compact.shape[0], self.sticky, _lib.STREAM)

    def audited(self):
        """(passes that left their calibrated ranges, passes audited) since the table was created (synchronises)"""
        bad_slots, bad_passes, passes, _ = self.sticky.tolist()
        return bad_passes, passes

    def new_slot(self):
        if self.n >= self.tab.shape[0]:
            raise _lib.PreworldHipError('RangeCtx: more than %d h2 tensors in one pass' % self.tab.shape[0])
        self.n += 1
        return self.tab[self.n - 1]

    @staticmethod
    def ideal_exp(amax):
        """the exponent k_f32_to_h2 / rng_ideal_exp (pw_h2.h) derive from a maximum: largest magnitude in [2^12, 2^13)"""
        import math
        if not (amax > 0.0) or math.isinf(amax) or math.isnan(amax):
            return 0
        return max(-100, min(100, math.frexp(amax)[1] - 1 - RangeCtx.TARGET))

    def _read(self, host=None):
        import numpy as np
        t = (self.compact.cpu() if host is None else host).numpy()
        return t[:, 0].astype(np.int64), t[:, 1].astype(np.int32).view(np.float32).astype(np.float64)

    def check(self, host=None):
        """indices of the slots whose recorded maximum left the hard window under the exponent it was written with, as of the
        last fold() (host: an already copied `compact` table, e.g. the one a graph replay delivers)"""
        import numpy as np
        e, amax = self._read(host)
        with np.errstate(over='ignore', invalid='ignore'):
            stored = amax * np.exp2(-e.astype(np.float64))
        bad = (amax != 0) & ~((stored >= 2.0 ** self.HARD_LO) & (stored <= self.HARD_HI))
        return np.nonzero(bad)[0].tolist()

    def settle(self):
        """after a pass: move the exponents of tensors outside the calibration window; True when nothing had to move"""
        import numpy as np
        self.fold()
        e, amax = self._read()
        new = e.copy()
        for i in range(len(e)):
            a = float(amax[i])
            if a == 0.0:
                self._jumped.discard(i)               # not written in this pass: a later user of the index starts afresh
                continue
            if not np.isfinite(a):                    # overflowed under this exponent (or fed by a tensor that did)
                new[i] = min(int(e[i]) + 12, 100)
                self._jumped.add(i)
                continue
            ideal = self.ideal_exp(a)
            if i in self._jumped:                     # the blind + 12 only brought the tensor back into sight: with a finite maximum known,
                self._jumped.discard(i)               # take ITS ideal exponent instead of whatever the jump landed on inside the window
                new[i] = ideal
                continue
            if not (ideal + self.TARGET - self.SETTLE_HI < e[i] <= ideal + self.TARGET - self.SETTLE_LO):
                new[i] = ideal
        if (new == e).all():
            return True
        self.tab[:len(e), 0] = torch.from_numpy(new.astype(np.int32)).to(self.device)
        return False


_range_stack = []


class use_range:
    """`with ops.use_range(ctx):` h2 producers called inside take their slots from ctx"""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        _range_stack.append(self.ctx)
        return self.ctx

    def __exit__(self, *exc):
        _range_stack.pop()


def current_range():
    return _range_stack[-1] if _range_stack else None


def new_slot(device):
    """range slot for a new h2 tensor: the active RangeCtx's next one, else a private slot with exponent 0 (the stored units
    are the values themselves -- fine for O(1) data; wrap the computation in ops.ranged() for anything else)"""
    ctx = current_range()
    return ctx.new_slot() if ctx is not None else torch.zeros(RNG_ROW, dtype=_i32, device=device)


def slot_state(slot):
    """(exponent, largest recorded |value|) of one range slot as host numbers (folds its partial maxima first; syncs)"""
    _lib.call('pw_rng_fold', slot, 1, None, _lib.STREAM)
    e, bits = slot[:2].tolist()
    import struct
    return e, struct.unpack('f', struct.pack('i', bits))[0]


def ranged(fn, ctx, max_iter=12, agree=None):
    """Run fn() under ctx until its activation ranges have settled (RangeCtx.settle) and return the last result.  Under
    stream capture fn() runs once with the exponents as they are (calibrate before capturing; `check()` after replays).
    agree(ok) -> bool: multi-process passes (fn contains collectives) pass a function that ANDs `ok` over the ranks."""
    with use_range(ctx):
        for _ in range(max_iter):
            ctx.begin()
            out = fn()
            if torch.cuda.is_current_stream_capturing():
                ctx.fold()
                return out
            ok = ctx.settle()
            if agree(ok) if agree is not None else ok:
                return out
    raise _lib.PreworldHipError('activation ranges did not settle in %d passes (non-finite inputs or weights?): slots %s'
                                % (max_iter, ctx.check()))


class H2:
    """A channels-last activation tensor in h2 storage (include/preworld_hip.h): `.buf` is a float32-typed torch
    tensor of the logical shape (.., C), C % 32 == 0, whose bytes are the split-fp16 encoding of value / 2^e; `.rng` is the
    range slot (int32[2] device tensor: [e, recorded maximum]) the tensor was written under, or None for e = 0.  Channel
    slices at multiples of 32 and leading-axis slices of `.buf` are again valid h2 tensors under the same slot."""
    __slots__ = ('buf', 'rng')

    def __init__(self, buf, rng=None):
        if buf.dtype != _f32 or buf.shape[-1] % 32:
            raise _lib.PreworldHipError('h2 tensors are float32-typed with a multiple of 32 channels')
        if rng is not None and (rng.dtype != _i32 or rng.numel() != RNG_ROW or not rng.is_contiguous() or rng.device != buf.device):
            raise _lib.PreworldHipError('h2 range slot must be a contiguous int32[%d] tensor on the same device' % RNG_ROW)
        self.buf = buf
        self.rng = rng

    @property
    def shape(self):
        return self.buf.shape

    @property
    def device(self):
        return self.buf.device

    def __getitem__(self, idx):
        return H2(self.buf[idx], self.rng)

    def view(self, *shape):
        return H2(self.buf.view(*shape), self.rng)


def _rng(h):
    """an H2's range slot (None -> NULL without one)"""
    return h.rng if isinstance(h, H2) and h.rng is not None else None


def _out_h2(o, device):
    """(buffer, slot) of an h2 destination: an ops.H2 keeps its slot, a raw buffer / a new tensor gets a new one"""
    if isinstance(o, H2):
        return o.buf, (o.rng if o.rng is not None else None)
    return o, new_slot(device)


def _rows(t, name):
    """(n_vox, C, ld) of a channels-last tensor that is dense or a channel slice of a dense buffer."""
    C = t.shape[-1]
    n = t.numel() // C
    if t.is_contiguous():
        return n, C, C
    ld, expect = None, None
    for i in range(t.dim() - 2, -1, -1):                 # innermost voxel axis of extent > 1 defines the row stride
        if t.shape[i] == 1:
            continue
        if ld is None:
            ld, expect = t.stride(i), t.stride(i) * t.shape[i]
        elif t.stride(i) != expect:
            ld = -1
            break
        else:
            expect *= t.shape[i]
    if ld is None:
        ld = C
    if t.stride(-1) != 1 or ld < C:
        raise _lib.PreworldHipError('%s must be dense or a channel slice of a dense channels-last buffer' % name)
    return n, C, ld


def f32_to_h2(x, out=None):
    """fp32 channels-last (.., C) -> H2 of the same shape (pw_f32_to_h2).  out: None (new tensor under a private slot whose
    exponent is derived from max|x| on the device: exact for any scale), an ops.H2 (written under ITS slot's exponent) or a
    raw float32 buffer (same, new private slot)."""
    n, C, ldx = _rows(x, 'x')
    if isinstance(out, H2) and out.rng is not None:
        buf, slot, auto = out.buf, out.rng, 0
    else:
        buf = out.buf if isinstance(out, H2) else out
        if buf is None:
            buf = torch.empty(x.shape, device=x.device, dtype=_f32)
        slot, auto = torch.zeros(RNG_ROW, dtype=_i32, device=x.device), 1
    _, _, ldy = _rows(buf, 'out')
    _lib.call('pw_f32_to_h2', _slice(x), _slice(buf), n, C, ldx, ldy, slot, auto, _lib.STREAM)
    return H2(buf, slot)


def h2_to_f32(x, out=None):
    """H2 -> fp32 channels-last tensor of the same shape (pw_h2_to_f32): (hi + lo) * 2^e, exact."""
    n, C, ldx = _rows(x.buf, 'x')
    if out is None:
        out = torch.empty(x.shape, device=x.buf.device, dtype=_f32)
    _, _, ldy = _rows(out, 'out')
    _lib.call('pw_h2_to_f32', _slice(x.buf), _slice(out), n, C, ldx, ldy, _rng(x), _lib.STREAM)
    return out


def pack_conv_weight_h2(w, cout_total=None):
    """torch Conv3d weight (Cout, Cin, 3,3,3) -> (wpk, inv_scale): split-fp16 weights in the operand order of
    pw_conv3d_h2 (include/preworld_hip.h) as a float32-typed tensor [Cin/32][27][cout_total/32][4 pieces][64 lanes][4], and the
    per-column factor (cout_total,) = 1 / S[n] to multiply into the epilogue scale.  S[n] = 2^k puts the largest
    |w[n]| in [512, 1024): both halves of the split are then normal fp16 numbers for every weight above 2^-13 of it."""
    Cout, Cin = w.shape[:2]
    taps = w.shape[2] * w.shape[3] * w.shape[4]
    if Cin % 32:
        raise _lib.PreworldHipError('pack_conv_weight_h2 expects Cin % 32 == 0')
    if cout_total is None:
        cout_total = (Cout + 31) // 32 * 32
    wf = w.reshape(Cout, -1).double()
    amax = wf.abs().amax(dim=1).clamp_min(1e-30)
    S = torch.exp2(torch.floor(torch.log2(1023.0 / amax)))                       # power of two per output channel
    ws = torch.zeros(cout_total, Cin, taps, dtype=torch.float64, device=w.device)
    ws[:Cout] = (wf * S[:, None]).view(Cout, Cin, taps)
    hi = ws.to(torch.float16)
    lo = (ws - hi.double()).to(torch.float16)
    planes = torch.stack([hi, lo], 0)                                            # (p, n, c, tap)
    nt, nch = cout_total // 32, Cin // 32
    t = planes.view(2, nt, 32, nch, 2, 2, 8, taps)                               # (p, nt, j, ch, ks, h, e, tap)
    t = t.permute(3, 7, 1, 4, 0, 5, 2, 6).contiguous()                           # (ch, tap, nt, ks, p, h, j, e): piece-major
    wpk = t.view(nch, taps, nt, 4 * 64 * 8).view(torch.float32).view(nch, taps, nt, 64, 16).contiguous()
    inv = torch.ones(cout_total, dtype=torch.float64, device=w.device)
    inv[:Cout] = 1.0 / S
    return wpk, inv.float()


def pack_conv_weights_h2_concat(ws):
    """conv1 + downsample of a BasicBlock3D over the same input: packed columns side by side."""
    parts = [pack_conv_weight_h2(w) for w in ws]
    return torch.cat([p[0] for p in parts], dim=2).contiguous(), torch.cat([p[1] for p in parts]).contiguous()


def conv3d_h2(x, wpk, scale, bias=None, residual=None, cout0=None, cout1=0, relu0=False, relu1=False, out0=None,
              out1=None, out_h2=(True, True), ksize=3, stride=1, algo=0):
    """3x3x3 stride-1 pad-1 conv on the fp16 matrix cores with split-fp16 operands (pw_conv3d_h2).
    x: H2 (B,D,H,W,Cin); wpk from pack_conv_weight_h2; scale (cout_total,) MUST already contain the packer's
    inv_scale (scale = bn_scale * inv_scale).  residual: H2 or fp32 tensor with y0's layout (may be out0 itself).
    out_h2: storage of (y0, y1): True -> H2, False -> fp32 tensor.  out0 / out1: destinations -- an ops.H2 is written under
    its own range slot, a raw buffer (or None) in h2 format gets a new slot (ops.new_slot).  Returns y0 [, y1]."""
    if not isinstance(x, H2):
        raise _lib.PreworldHipError('conv3d_h2 takes an ops.H2 input (ops.f32_to_h2)')
    B, D, H, W, Cin = x.shape
    nch, taps, nt = wpk.shape[:3]
    cout_total = nt * 32
    if nch * 32 != Cin or taps != ksize ** 3:
        raise _lib.PreworldHipError('packed h2 weight does not match Cin / ksize')
    pad = (ksize - 1) // 2
    D, H, W = [(v + 2 * pad - ksize) // stride + 1 for v in (D, H, W)]      # output grid from here on
    Din, Hin, Win = x.shape[1:4]
    if cout0 is None:
        cout0 = cout_total
    fm0, fm1 = int(bool(out_h2[0])), int(bool(out_h2[1]))

    def _dst(o, c, fm):
        if o is None:
            o = torch.empty(B, D, H, W, c, device=x.buf.device, dtype=_f32)
        if not fm:
            return (o.buf if isinstance(o, H2) else o), None
        return _out_h2(o, x.buf.device)
    y0, rng0 = _dst(out0, cout0, fm0)
    ld0 = _row_stride(y0, (B, D, H, W, cout0), 'y0')
    y1, ld1, rng1 = None, 0, None
    if cout1:
        y1, rng1 = _dst(out1, cout1, fm1)
        ld1 = _row_stride(y1, (B, D, H, W, cout1), 'y1')
    res, fmr = None, 0
    if residual is not None:
        fmr = int(isinstance(residual, H2))
        res = residual.buf if fmr else residual
        if _row_stride(res, (B, D, H, W, cout0), 'residual') != ld0:
            raise _lib.PreworldHipError('residual must have the same row stride as y0')
    if scale is None:
        raise _lib.PreworldHipError('conv3d_h2 needs scale = (BN scale or 1) * inv_scale of pack_conv_weight_h2')
    if scale.numel() != cout_total or (bias is not None and bias.numel() != cout_total):
        raise _lib.PreworldHipError('scale (with the weight pre-scale folded in) / bias must have cout_total=%d entries' % cout_total)
    _lib.call('pw_conv3d_h2', x.buf, wpk, scale, bias, _slice(res), _slice(y0), _slice(y1), B, Din, Hin, Win, Cin, cout_total,
              cout0, cout1, ld0, ld1, ksize, stride, int(relu0), int(relu1), algo, fm0, fm1, fmr, _rng(x), _rng(residual), rng0,
              rng1, _lib.STREAM)
    r0 = H2(y0, rng0) if fm0 else y0
    if cout1:
        return r0, (H2(y1, rng1) if fm1 else y1)
    return r0


def fpn3d_fuse(x8, wpk8, y16, y32, scale, bias, relu=True, out=None, out_h2=False):
    """LSSFPN3D tail: ReLU(BN(W8 x8 + up2(y16) + up4(y32))) -- lss_fpn.py:132-148.  x8: fp32 tensor (wpk8 from
    pack_conv_weight) or ops.H2 (wpk8 from pack_conv_weight_h2, its inv_scale folded into scale); out_h2: return ops.H2."""
    x_h2 = isinstance(x8, H2)
    xb = x8.buf if x_h2 else x8
    B, D, H, W, C8 = xb.shape
    if out is None:
        out = torch.empty(B, D, H, W, 32, device=xb.device, dtype=_f32)
    orng = None
    if out_h2:
        out, orng = _out_h2(out, xb.device)
    _lib.call('pw_fpn3d_fuse', xb, wpk8, y16, y32, scale, bias, out, B, D, H, W, C8, y16.shape[1], y16.shape[2], y16.shape[3],
              y32.shape[1], y32.shape[2], y32.shape[3], int(relu), int(x_h2), int(bool(out_h2)), _rng(x8), orng, _lib.STREAM)
    return H2(out, orng) if out_h2 else out


def pack_conv_weight16(w):
    """(16, Cin, 3,3,3) conv weight -> float[Cin/32][27][64][8] for the 16x16x4 MFMA OccHead
    kernel: wpk[ch][tap][g*16+j][s] = w[j][ch*32+g*8+s][tap]."""
    Cout, Cin = w.shape[:2]
    if Cout != 16 or Cin % 32:
        raise _lib.PreworldHipError('pack_conv_weight16 expects (16, 32k, 3,3,3)')
    nch = Cin // 32
    wp = w.reshape(16, nch, 4, 8, 27).permute(1, 4, 2, 0, 3).contiguous()    # (ch, tap, g, j, s)
    return wp.view(nch, 27, 64, 8).float().contiguous()


def occ_head_fused(x, wpk, scale, bias, w1, s1, b1, w2, want_logits=False, occ=None, want_geo=False,
                   empty_idx=17):
    """OccHead (occupancy_head.py:124-177) on channels-last x (B,D,H,W,32); wpk from pack_conv_weight16 (direct
    MFMA kernel) or pack_conv_weight_wino(w, cout_total=16) (Winograd kernel, 32 input channels):
    returns uint8 argmax (B,D,H,W) [, logits (B,D,H,W,18)] [, geo_occ uint8 (B,D,H,W) =
    0 where occupied / 17 where empty, preworld_temporal_traj.py:313-319]."""
    B, D, H, W, Cin = x.shape
    if occ is None:
        occ = torch.empty(B, D, H, W, device=x.device, dtype=torch.uint8)
    logits = torch.empty(B, D, H, W, 18, device=x.device, dtype=_f32) if want_logits else None
    geo = torch.empty(B, D, H, W, device=x.device, dtype=torch.uint8) if want_geo else None
    _lib.call('pw_occ_head_fused', x, wpk, scale, bias, w1, s1, b1, w2, occ, logits, geo, int(empty_idx), B, D, H, W, Cin, 16, 8,
              18, 64 if wpk.dim() == 5 else (16 if wpk.shape[-1] == 8 else 32), _lib.STREAM)
    out = (occ,) + ((logits,) if want_logits else ()) + ((geo,) if want_geo else ())
    return out if len(out) > 1 else occ


def pack_occ_weight_h2(w):
    """OccHead conv weight (16, 32, 3,3,3) -> (wpk, inv_scale (16,)) for pw_occ_head_h2 (include/preworld_hip.h):
    wpk[tap][plane][g*16 + j][e] = plane of S_j * w[j][16*(g>>1) + 8*(g&1) + e][tap] as a float32-typed (27, 2, 64, 4) tensor."""
    Cout, Cin = w.shape[:2]
    if (Cout, Cin) != (16, 32) or tuple(w.shape[2:]) != (3, 3, 3):
        raise _lib.PreworldHipError('pack_occ_weight_h2 expects a (16, 32, 3, 3, 3) weight')
    wf = w.reshape(Cout, -1).double()
    S = torch.exp2(torch.floor(torch.log2(1023.0 / wf.abs().amax(dim=1).clamp_min(1e-30))))
    ws = (wf * S[:, None]).view(Cout, Cin, 27)
    hi = ws.to(torch.float16)
    lo = (ws - hi.double()).to(torch.float16)
    t = torch.stack([hi, lo], 0).view(2, 16, 2, 2, 8, 27)                          # (p, j, ks, half, e, tap): c = 16 ks + 8 half + e
    t = t.permute(5, 0, 2, 3, 1, 4).contiguous()                                   # (tap, p, ks, half, j, e): g = 2 ks + half
    wpk = t.view(27, 2, 64, 8).view(torch.float32).view(27, 2, 64, 4).contiguous()
    return wpk, (1.0 / S).float()


def occ_head_bounds(w0, s0, b0, w1, s1, b1):
    """a-priori magnitude bounds of OccHead's two hidden layers for pw_occ_head_h2 (include/preworld_hip.h): w0 (16,32,3,3,3) /
    w1 (8,16) conv weights, s* / b* folded BN.  Returns host floats (mid_a, mid_b, hid_a, hid_b)."""
    mid_a = float((s0.double().abs()[:w0.shape[0]] * w0.double().abs().flatten(1).sum(1)).max())
    hid_a = float((s1.double().abs() * w1.double().abs().flatten(1).sum(1)).max())
    return mid_a, float(b0.double().abs().max()), hid_a, float(b1.double().abs().max())


def pack_occ_tail_h2(w1, s1, b1, w2):
    """The 16 -> 8 (+BN+ReLU) -> 18 tail of OccHead as operands of pw_occ_head_h2: w1 (8,16), s1 / b1 (8,) folded BN, w2 (18,8)
    -> (tailpk float32 (800,), inv2).  One power-of-two pre-scale per matrix (argmax must see one common scale)."""
    dev = w1.device
    S1, h1, l1 = _split_planes(w1.double())
    S2, h2_, l2 = _split_planes(w2.double())
    lane = torch.arange(64, device=dev)
    row, kg = lane & 15, lane >> 4
    k = (4 * kg)[:, None] + torch.arange(4, device=dev)[None, :]                    # (64, 4): k = 4 g + e

    def frag(plane, nrow, ncol, row0=0):
        full = torch.zeros(32, 16, dtype=torch.float16, device=dev)
        full[:nrow, :ncol] = plane
        return full[(row0 + row)[:, None], k]                                       # (64, 4) fp16

    frags = [frag(h1, 8, 16), frag(l1, 8, 16), frag(h2_, 18, 8), frag(l2, 18, 8), frag(h2_, 18, 8, 16), frag(l2, 18, 8, 16)]
    pk = torch.stack(frags, 0).contiguous().view(torch.float32).reshape(-1)        # 6 * 64 * 2 floats
    s1p = torch.zeros(16, dtype=_f32, device=dev)
    b1p = torch.zeros(16, dtype=_f32, device=dev)
    s1p[:8] = (s1.double() / S1).float()
    b1p[:8] = b1.float()
    return torch.cat([pk, s1p, b1p]).contiguous(), 1.0 / S2


def occ_head_h2(x, wpk, scale, bias, tailpk, inv2, bounds, want_logits=False, occ=None, want_geo=False, empty_idx=17, geo=None):
    """OccHead (occupancy_head.py:124-177) on the fp16 matrix cores: x = ops.H2 (B,D,H,W,32); wpk from pack_occ_weight_h2;
    scale (16,) MUST already contain the packer's inv_scale; (tailpk, inv2) from pack_occ_tail_h2; bounds from occ_head_bounds.
    Returns like occ_head_fused.  occ / geo: optional uint8 (B,D,H,W) destinations with ARBITRARY (equal) strides -- e.g. the
    .permute(0,3,2,1) view of an (B,X,Y,Z)-contiguous payload buffer: the kernel then writes the reference's (X,Y,Z) arrays in
    place (pw_occ_head_h2_strided) and no transposing copy is needed afterwards."""
    if not isinstance(x, H2):
        raise _lib.PreworldHipError('occ_head_h2 takes an ops.H2 input (ops.f32_to_h2)')
    B, D, H, W, Cin = x.shape
    if geo is not None:
        want_geo = True
    if occ is None:
        occ = torch.empty(B, D, H, W, device=x.device, dtype=torch.uint8)
    logits = torch.empty(B, D, H, W, 18, device=x.device, dtype=_f32) if want_logits else None
    if want_geo and geo is None:
        # (empty_strided sizes the storage for the gapped / interleaved strides; as_strided over a dense allocation did not)
        geo = torch.empty_strided(tuple(occ.shape), tuple(occ.stride()), device=x.device, dtype=torch.uint8)
    if tailpk.numel() != 800 or scale.numel() < 16 or bias.numel() < 16:
        raise _lib.PreworldHipError('occ_head_h2: tailpk (800,), scale / bias (16,) expected')
    for t in (occ, geo):
        if t is not None and (tuple(t.shape) != (B, D, H, W) or t.dtype != torch.uint8 or not t.is_cuda):
            raise _lib.PreworldHipError('occ_head_h2: occ / geo must be uint8 device tensors of shape (B, D, H, W)')
    strides, span = None, 0
    if not occ.is_contiguous() or (geo is not None and not geo.is_contiguous()):
        if geo is not None and tuple(geo.stride()) != tuple(occ.stride()):
            raise _lib.PreworldHipError('occ_head_h2: occ and geo must have the same strides')
        st = [int(v) for v in occ.stride()]
        strides = (ctypes.c_int64 * 4)(*st)
        span = 1 + sum((n - 1) * v for n, v in zip((B, D, H, W), st))
        # (the C side rejects overlapping stride sets -- two voxels storing to one byte would race)
    _lib.call('pw_occ_head_h2_strided', x.buf, wpk, scale, bias, tailpk, float(inv2), _slice(occ), logits, _slice(geo), strides,
              int(span), int(empty_idx), B, D, H, W, Cin, 16, 8, 18, _rng(x), float(bounds[0]), float(bounds[1]), float(bounds[2]),
              float(bounds[3]), _lib.STREAM)
    out = (occ,) + ((logits,) if want_logits else ()) + ((geo,) if want_geo else ())
    return out if len(out) > 1 else occ


def forecast_pack(fusion_w1, fusion_w2):
    w1p = torch.empty(4096, device=fusion_w1.device, dtype=_f32)
    w2p = torch.empty(4096, device=fusion_w1.device, dtype=_f32)
    _lib.call('pw_forecast_pack', fusion_w1, fusion_w2, w1p, w2p, _lib.STREAM)
    return w1p, w2p


def forecast_prologue(ego, plan, fusion_w1, fusion_b1):
    """ego (n_samples, 21); plan = [(w0,b0),(w2,b2),(w4,b4)] ->
    (ego_feat (n,32), c1 (n,128) natural order, c1p (n,128) accumulator order)."""
    n, dim = ego.shape
    ef = torch.empty(n, 32, device=ego.device, dtype=_f32)
    c1 = torch.empty(n, 128, device=ego.device, dtype=_f32)
    c1p = torch.empty(n, 128, device=ego.device, dtype=_f32)
    (w0, b0), (w2, b2), (w4, b4) = plan
    _lib.call('pw_forecast_prologue', ego, n, dim, w0, b0, w2, b2, w4, b4, fusion_w1, fusion_b1, ef, c1, c1p, _lib.STREAM)
    return ef, c1, c1p


def forecast_steps(v0, n_samples, w1p, w2p, c1p, fusion_b2, n_steps, states=None):
    """v0 (n_samples, ..., 32) channels-last -> states (n_steps, *v0.shape)."""
    n_total = v0.numel() // 32
    if states is None:
        states = torch.empty((n_steps,) + tuple(v0.shape), device=v0.device, dtype=_f32)
    _lib.call('pw_forecast_steps', v0, n_total // n_samples, n_samples, w1p, w2p, c1p, fusion_b2, n_steps, states, _lib.STREAM)
    return states


def _split_planes(w):
    """float64 tensor -> (power-of-two scale S, fp16 hi, fp16 lo) of S * w, largest |S w| in [512, 1024)"""
    S = float(2.0 ** torch.floor(torch.log2(1023.0 / w.abs().max().clamp_min(1e-30))))
    ws = w * S
    hi = ws.to(torch.float16)
    return S, hi, (ws - hi.double()).to(torch.float16)


def forecast_pack_h2(fusion_w1, fusion_w2):
    """fusion_head.{0,2}.weight ([128][64], [32][128]) -> (w1p, w2p, inv1, inv2, w1_l1max): split-fp16 MFMA A operands in the
    order pw_forecast_steps_h2 documents (include/preworld_hip.h), the inverses of their power-of-two pre-scales and the largest
    row L1 norm of the voxel part of W1 (the kernel's a-priori bound on the hidden activations)."""
    import numpy as np
    dev = fusion_w1.device
    lane = np.arange(64)
    i, h = lane & 31, lane >> 5
    e = np.arange(8)
    # row_of(8 kb + e, h) = ((8kb+e) & 3) + 8 * ((8kb+e) >> 2) + 4 h
    t, kb, ln, ee = np.meshgrid(np.arange(4), np.arange(2), lane, e, indexing='ij')
    r = 8 * kb + ee
    k = (r & 3) + 8 * (r >> 2) + 4 * (ln >> 5)
    row = ln & 31
    T = lambda a: torch.from_numpy(a.reshape(-1)).to(dev)                      # noqa: E731
    S1, h1, l1 = _split_planes(fusion_w1[:, :32].double())                     # voxel part of W1 (128, 32)
    S2, h2_, l2 = _split_planes(fusion_w2.double())                            # (32, 128)
    idx1 = (T(t) * 32 + T(row), T(k))
    idx2 = (T(row), T(t) * 32 + T(k))
    w1p = torch.stack([h1[idx1].view(4, 2, 64, 8), l1[idx1].view(4, 2, 64, 8)], dim=2)     # (t, kb, p, lane, e)
    w2p = torch.stack([h2_[idx2].view(4, 2, 64, 8), l2[idx2].view(4, 2, 64, 8)], dim=2)
    return (w1p.contiguous().view(torch.float32).contiguous(), w2p.contiguous().view(torch.float32).contiguous(),
            1.0 / S1, 1.0 / S2, float(fusion_w1[:, :32].double().abs().sum(1).max()))


def forecast_steps_h2(v0, n_samples, packed, c1p, fusion_b2, n_steps, states=None, out_h2=False):
    """forecast_steps on the fp16 matrix cores with split-fp16 operands; packed = forecast_pack_h2(...).
    v0: fp32 tensor or ops.H2; out_h2=True returns the states as ONE ops.H2 of shape (n_steps, *v0.shape).  The recursion
    runs in the units of the states' range slot (a new one, or `states.rng`) whatever the output format."""
    w1p, w2p, inv1, inv2, l1 = packed
    v0_h2 = isinstance(v0, H2)
    vbuf = v0.buf if v0_h2 else v0
    n_total = vbuf.numel() // 32
    if states is None:
        states = torch.empty((n_steps,) + tuple(vbuf.shape), device=vbuf.device, dtype=_f32)
    states, srng = _out_h2(states, vbuf.device)
    if srng is None:
        srng = new_slot(vbuf.device)
    _lib.call('pw_forecast_steps_h2', vbuf, n_total // n_samples, n_samples, w1p, w2p, float(inv1), float(inv2), c1p, fusion_b2,
              n_steps, states, int(v0_h2), int(bool(out_h2)), _rng(v0), srng, float(l1), _lib.STREAM)
    return H2(states, srng) if out_h2 else states


def softplus(x):
    y = torch.empty_like(x)
    _lib.call('pw_softplus', x, y, x.numel(), _lib.STREAM)
    return y


# ------------------------------------------------------------------------------ ray table + WRS weights
def pts2ray(coor, label_depth, label_seg, label_img, c2w, cam_intrinsic):
    """mmdet3d/datasets/ray.py:47-55 (one camera): (n,16) rows
    {x, y, depth, seg, rays_o[3], rays_d[3], viewdirs[3], rgb[3]}."""
    n = coor.shape[0]
    rays = torch.empty(n, 16, device=coor.device, dtype=_f32)
    _lib.call('pw_pts2ray', coor.float().contiguous(), label_depth.float().contiguous(), label_seg.float().contiguous(),
              label_img.float().contiguous(), c2w.float().contiguous(), cam_intrinsic.float().contiguous(), n, rays, _lib.STREAM)
    return rays


def class_count(rays, n_cls=17, counts=None):
    if counts is None:
        counts = torch.zeros(n_cls, device=rays.device, dtype=torch.int64)
    _lib.call('pw_class_count', rays, rays.shape[0], n_cls, counts, _lib.STREAM)
    return counts


def wrs_weights(rays, frame_id, balance_weight, dynamic_class, weight_adj=0.3, weight_dyn=0.0):
    """ray.py:99-112 for one camera's rays of frame `frame_id`."""
    n = rays.shape[0]
    w = torch.empty(n, device=rays.device, dtype=_f32)
    dyn = dynamic_class.to(device=rays.device, dtype=_i32).contiguous()
    _lib.call('pw_wrs_weights', rays, n, int(frame_id), balance_weight.float().contiguous(), balance_weight.numel(), dyn,
              dyn.numel(), float(weight_adj), float(weight_dyn), w, _lib.STREAM)
    return w


# ------------------------------------------------------------------------------ depth supervision from the sweep
def _sweep_args(points, offsets, lidar2img, post_rots, post_trans):
    """-> (points (P,C) f32, offsets int32 (B+1) device tensor or None, B, N, lidar2img (B N,3,4), post_rots (B N,3,3),
    post_trans (B N,3)).  points: one (P,C) tensor (with `offsets`, or alone for B == 1) or a list of B per-sample tensors."""
    if lidar2img.dim() != 4 or lidar2img.shape[-1] != 4 or lidar2img.shape[-2] not in (3, 4):
        raise _lib.PreworldHipError('lidar2img must be (B,N,4,4) or (B,N,3,4), got %s' % (tuple(lidar2img.shape),))
    B, N = lidar2img.shape[:2]
    if isinstance(points, (list, tuple)):
        if len(points) != B:
            raise _lib.PreworldHipError('%d sweeps for %d samples' % (len(points), B))
        if offsets is None and B > 1:                # offsets are known on the host here: one small H2D copy, nothing read back
            counts = [0] + [int(p.shape[0]) for p in points]
            offsets = torch.tensor(np.cumsum(counts), dtype=_i32).to(points[0].device, non_blocking=True)
        points = torch.cat([p.float() for p in points], 0) if B > 1 else points[0]
    if points.dim() != 2 or points.shape[1] < 3:
        raise _lib.PreworldHipError('points must be (P, >=3), got %s' % (tuple(points.shape),))
    if offsets is None and B != 1:
        raise _lib.PreworldHipError('B = %d samples in one points tensor need offsets (int32, B + 1, on the device)' % B)
    if offsets is not None and (offsets.dtype != _i32 or offsets.numel() != B + 1):
        raise _lib.PreworldHipError('offsets must be int32 with B + 1 = %d entries' % (B + 1))
    l2i = lidar2img[..., :3, :].float().contiguous().view(B * N, 3, 4)
    return (points.float().contiguous(), offsets, B, N, l2i, post_rots.float().contiguous().view(B * N, 3, 3),
            post_trans.float().contiguous().view(B * N, 3))


def lidar_depth_maps(points, lidar2img, post_rots, post_trans, image_hw, depth_range, downsample=1, offsets=None):
    """PointToMultiViewDepth (mmdet3d/datasets/pipelines/loading.py:762-844) on the device: the sweep(s) `points` projected into
    the B x N views -> gt_depth (B, N, H // downsample, W // downsample), per pixel the exact minimum depth in
    [depth_range[0], depth_range[1]), 0 where nothing lands.  lidar2img (B,N,4,4) is what the reference composes from the four
    poses and the intrinsics (transforms.compose_lidar2img)."""
    pts, offsets, B, N, l2i, pr, pt = _sweep_args(points, offsets, lidar2img, post_rots, post_trans)
    H, W = int(image_hw[0]), int(image_hw[1])
    out = torch.empty(B, N, H // downsample, W // downsample, device=pts.device, dtype=_f32)
    _lib.call('pw_lidar_depth_maps', pts, pts.shape[0], pts.shape[1], offsets, B, N, l2i, pr, pt, H, W, int(downsample),
              float(depth_range[0]), float(depth_range[1]), out, _lib.STREAM)
    return out


def lidar_depth_labels(points, lidar2img, post_rots, post_trans, image_hw, depth_cfg, loss_downsample, D=None, downsample=1,
                       offsets=None):
    """The depth labels of get_downsampled_gt_depth straight from the sweep: (B*N, h, w) int32, label k >= 0 = depth bin k of the
    minimum depth landing in the cell, -1 = no label.  depth_cfg = grid_config['depth'] = [d0, d1, dstep]; equals
    depth_map_labels(lidar_depth_maps(...)) without the maps."""
    pts, offsets, B, N, l2i, pr, pt = _sweep_args(points, offsets, lidar2img, post_rots, post_trans)
    H, W = int(image_hw[0]), int(image_hw[1])
    d0, d1, dstep = [float(v) for v in depth_cfg]
    D = int(D) if D is not None else int(round((d1 - d0) / dstep))
    ld = int(loss_downsample)
    out = torch.empty(B * N, H // downsample // ld, W // downsample // ld, device=pts.device, dtype=_i32)
    _lib.call('pw_lidar_depth_labels', pts, pts.shape[0], pts.shape[1], offsets, B, N, l2i, pr, pt, H, W, int(downsample), ld, d0,
              d1, dstep, D, out, _lib.STREAM)
    return out


def depth_map_labels(gt_depth, downsample, depth_cfg, D=None):
    """get_downsampled_gt_depth (view_transformer.py:736-773, sid=False) as labels: gt_depth (B,N,H,W) or (B*N,H,W) float32 ->
    (B*N, H // downsample, W // downsample) int32; label k >= 0 is the hot column of the reference's one-hot row, -1 its all-zero
    row."""
    g = gt_depth.float().contiguous()
    H, W = g.shape[-2:]
    V = g.numel() // (H * W)
    d0, d1, dstep = [float(v) for v in depth_cfg]
    D = int(D) if D is not None else int(round((d1 - d0) / dstep))
    out = torch.empty(V, H // downsample, W // downsample, device=g.device, dtype=_i32)
    _lib.call('pw_depth_map_labels', g, V, H, W, int(downsample), d0, dstep, D, out, _lib.STREAM)
    return out


class DepthBCE(torch.autograd.Function):
    """get_depth_loss (view_transformer.py:775-789) on labels: pred (B*N, D, h, w) softmaxed depth in its own layout, labels
    (B*N, h, w) int32 -> weight * BCE sum over the labelled cells / max(1, n_fg), a 0-dim tensor.  n_fg stays in device memory
    (nothing synchronises, so the term can sit inside a captured step); the sum is bit-reproducible."""

    @staticmethod
    def forward(ctx, pred, labels, weight):
        BN, D = pred.shape[:2]
        hw = pred[0, 0].numel()
        if pred.dtype != _f32:       # the gradient comes back as float32 in this layout; autocast callers cast the softmax first
            raise _lib.PreworldHipError('depth_bce: pred must be float32, got %s' % pred.dtype)
        pred = pred.detach().contiguous()
        if labels.dtype != _i32 or labels.numel() != BN * hw:
            raise _lib.PreworldHipError('labels must be int32 with %d entries, got %s %s' % (BN * hw, labels.dtype, tuple(labels.shape)))
        labels = labels.contiguous()
        ws = _workspace(_lib.call_size('pw_depth_bce_ws_bytes', BN * hw), pred.device)
        loss = torch.empty((), device=pred.device, dtype=_f32)
        n_fg = torch.empty(1, device=pred.device, dtype=_i32)
        _lib.call('pw_depth_bce_fwd', pred, labels, BN, D, hw, float(weight), ws, loss, n_fg, _lib.STREAM)
        ctx.save_for_backward(pred, labels, n_fg)
        ctx.weight = float(weight)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        pred, labels, n_fg = ctx.saved_tensors
        BN, D = pred.shape[:2]
        grad = torch.empty_like(pred)
        g = grad_out.detach().float().contiguous().view(1)
        _lib.call('pw_depth_bce_bwd', pred, labels, g, n_fg, BN, D, pred[0, 0].numel(), ctx.weight, grad, _lib.STREAM)
        return grad, None, None


def depth_bce(pred, labels, weight):
    return DepthBCE.apply(pred, labels, weight)


# ------------------------------------------------------------------------------ ray supervision from the sweep
RAY_MEAN_STD = (0.485, 0.456, 0.406, 0.229, 0.224, 0.225)       # transforms.Normalize of nuscenes_dataset_occ.py:133-140
RAY_POSE_DOUBLES = _lib.PW_RAYS['PW_RAY_POSE_DOUBLES']
_RAY_BLOCK = 256


class RaySweeps:
    """The T sweeps of a sample as the kernels take them: points (T, Pmax, C) float32, labels (T, Pmax) uint8, n_pts int32 (T)
    on the device (None: every row counts), view_pose (T N, 57) float64 (transforms.compose_view_poses), lut uint8 (256).
    `points` / `point_labels` may be lists of T per-sweep tensors (padded here, lengths known on the host: one small copy,
    nothing read back) or the padded tensors themselves with `n_pts`."""

    def __init__(self, points, point_labels, view_pose, label_lut=None, n_pts=None):
        if isinstance(points, (list, tuple)):
            dev = points[0].device
            T, C = len(points), int(points[0].shape[1])
            lens = [int(p.shape[0]) for p in points]
            Pmax = max(1, max(lens))
            if len(point_labels) != T or any(int(l.numel()) != n for l, n in zip(point_labels, lens)):
                raise _lib.PreworldHipError('point_labels must hold one uint8 label per point of every sweep')
            pts = torch.zeros(T, Pmax, C, device=dev, dtype=_f32)
            lab = torch.zeros(T, Pmax, device=dev, dtype=torch.uint8)
            for t in range(T):
                pts[t, :lens[t]] = points[t]
                lab[t, :lens[t]] = point_labels[t].view(-1)
            if n_pts is None and any(n != Pmax for n in lens):
                n_pts = torch.tensor(lens, dtype=_i32).to(dev, non_blocking=True)
            points, point_labels = pts, lab
        if points.dim() != 3 or points.shape[2] < 3 or points.shape[1] < 1:
            raise _lib.PreworldHipError('points must be (T, Pmax >= 1, >= 3), got %s' % (tuple(points.shape),))
        T, Pmax = int(points.shape[0]), int(points.shape[1])
        if point_labels.dtype != torch.uint8 or tuple(point_labels.shape) != (T, Pmax):
            raise _lib.PreworldHipError('point_labels must be uint8 (T, Pmax) = (%d, %d), got %s %s' %
                                        (T, Pmax, point_labels.dtype, tuple(point_labels.shape)))
        if n_pts is not None and (n_pts.dtype != _i32 or n_pts.numel() != T):
            raise _lib.PreworldHipError('n_pts must be int32 with T = %d entries' % T)
        V = int(view_pose.shape[0])
        if view_pose.dim() != 2 or view_pose.shape[1] != RAY_POSE_DOUBLES or V % T:
            raise _lib.PreworldHipError('view_pose must be (T N, %d), got %s for T = %d' % (RAY_POSE_DOUBLES, tuple(view_pose.shape), T))
        dev = points.device
        self.points, self.labels, self.n_pts = points.float().contiguous(), point_labels.contiguous(), n_pts
        self.pose = view_pose.to(device=dev, dtype=torch.float64).contiguous()
        if label_lut is None:
            label_lut = torch.arange(256, dtype=torch.uint8)
        label_lut = torch.as_tensor(label_lut)
        if label_lut.numel() != 256:
            raise _lib.PreworldHipError('label_lut must have 256 entries')
        self.lut = label_lut.to(device=dev, dtype=torch.uint8).contiguous()
        self.T, self.N, self.V, self.Pmax = T, V // T, V, Pmax
        self.nblk = -(-Pmax // _RAY_BLOCK)

    def head(self):
        return (self.points, self.points.shape[2])

    def count(self, H, W, owners=True):
        """project (+ owners) + scan -> (slots, block_base, view_off); view_off[V] is the number of rows, on the device.
        owners=False: no owner table is allocated, cleared or filled (slots None): what stage A alone needs"""
        dev = self.points.device
        slots = torch.empty(ray_slot_count(self.V * self.Pmax), device=dev, dtype=torch.int64) if owners else None
        block_base = torch.empty(self.V * self.nblk, device=dev, dtype=_i32)
        view_off = torch.empty(self.V + 1, device=dev, dtype=_i32)
        _lib.call('pw_ray_sweep_count', self.points, self.points.shape[2], self.n_pts, self.T, self.N, self.Pmax, self.pose, H, W,
                  slots, slots.numel() if owners else 0, block_base, view_off, _lib.STREAM)
        return slots, block_base, view_off


def ray_slot_count(n_items):
    """entries of the owner table for n_items insertions: the power of two >= 2 n_items (load <= 1/2), at least 1024"""
    n = 1024
    while n < 2 * n_items:
        n *= 2
    return n


def ray_scratch_bytes(T, N, Pmax):
    """device scratch of one sweeps-mode table: owner slots + block bases + view offsets"""
    V = T * N
    return 8 * ray_slot_count(V * Pmax) + 4 * V * (-(-Pmax // _RAY_BLOCK)) + 4 * (V + 1)


def _ray_frames(frames_u8, view_frame, V, H, W):
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or tuple(frames_u8.shape[1:]) != (H, W, 3):
        raise _lib.PreworldHipError('frames_u8 must be uint8 (F, %d, %d, 3), got %s %s' % (H, W, frames_u8.dtype, tuple(frames_u8.shape)))
    if any(s < 0 for s in frames_u8.stride()):
        raise _lib.PreworldHipError('frames_u8 must not have negative strides')
    F = int(frames_u8.shape[0])
    if view_frame is None:
        if F < V:
            raise _lib.PreworldHipError('%d frames for %d views: pass view_frame' % (F, V))
    else:
        if isinstance(view_frame, torch.Tensor):
            if view_frame.dtype != _i32 or view_frame.numel() != V:
                raise _lib.PreworldHipError('view_frame must be int32 with V = %d entries' % V)
        else:
            idx = [int(i) for i in view_frame]
            if len(idx) != V or min(idx) < 0 or max(idx) >= F:
                raise _lib.PreworldHipError('view_frame must name one of the %d frames for each of the %d views' % (F, V))
            view_frame = torch.tensor(idx, dtype=_i32).to(frames_u8.device, non_blocking=True)
    return (_lib.strided(frames_u8),) + tuple(int(s) for s in frames_u8.stride()) + (F, view_frame)


def _ray_cams(c2w, K, V, dev):
    c2w = torch.as_tensor(c2w).to(device=dev, dtype=_f32).contiguous()
    K = torch.as_tensor(K).to(device=dev, dtype=_f32).contiguous()
    if tuple(c2w.shape) != (V, 4, 4) or tuple(K.shape) != (V, 3, 3):
        raise _lib.PreworldHipError('c2w must be (V,4,4) and K (V,3,3) with V = %d, got %s %s' % (V, tuple(c2w.shape), tuple(K.shape)))
    return c2w, K


def _ray_out(out, cap, dev):
    if out is None:
        return torch.empty(max(cap, 1), 16, device=dev, dtype=_f32)
    if out.dtype != _f32 or tuple(out.shape) != (cap, 16) or cap < 1 or not out.is_contiguous() or out.data_ptr() % 16:
        raise _lib.PreworldHipError('out must be a contiguous, 16-byte aligned float32 (capacity, 16) = (%d, 16) buffer' % cap)
    return out


def sweep_pixel_labels(points, point_labels, view_pose, image_hw, label_lut=None, n_pts=None):
    """Stage A alone: tools/gen_data/gen_depth_gt.py and gen_seg_gt_from_lidarseg.py for every sweep and camera of a sample.
    -> (depth_list (R,3) float32 rows (u, v, depth), seg_list (R,3) rows (u, v, class), view_off int32 (V+1)): rows
    view_off[v] .. view_off[v+1]-1 are, byte for byte, the contents of the two .bin files of view v = t N + camera.  Reads the
    row count back (one host synchronisation)."""
    sw = points if isinstance(points, RaySweeps) else RaySweeps(points, point_labels, view_pose, label_lut, n_pts)
    H, W = int(image_hw[0]), int(image_hw[1])
    _, block_base, view_off = sw.count(H, W, owners=False)
    R = int(view_off[-1].item())
    dev = sw.points.device
    depth_list = torch.empty(max(R, 1), 3, device=dev, dtype=_f32)
    seg_list = torch.empty(max(R, 1), 3, device=dev, dtype=_f32)
    _lib.call('pw_ray_sweep_lists', *sw.head(), sw.labels, sw.n_pts, sw.T, sw.N, sw.Pmax, sw.lut, sw.pose, H, W, block_base,
              max(R, 1), depth_list, seg_list, _lib.STREAM)
    return depth_list[:R], seg_list[:R], view_off


def ray_table(c2w, K, frames_u8, sweeps=None, lists=None, view_frame=None, capacity=None, n_cls=17, mean_std=RAY_MEAN_STD, out=None):
    """The (R,16) ray table of nuscenes_dataset_occ.py:197-270 get_rays + ray.py:47-56 for all V views of a sample.
      sweeps = RaySweeps(...)                               -- from the raw sweeps (stage A and B), or
      lists = (depth_list (n,3), seg_list (n,3), view_off)  -- from the contents of the two gen tools' files, views back to back
                                                               (view_off int32 (V+1) on the device or a host sequence)
    c2w (V,4,4) = sensor2keyego, K (V,3,3); frames_u8 uint8 (F,H,W,3) with any strides, view_frame[v] the frame of view v
    (default v).  -> (rays (capacity,16), view_off (V+1) int32 on the device, counts int64 (n_cls) of the rows written).
    view_off[V] = R is the number of kept points; rows >= capacity are dropped, rows between R and capacity are not written
    (ray_table_weights zeroes them).  capacity=None: R is read back (one host synchronisation) and capacity = R.  out: the
    caller's own (capacity,16) float32 buffer."""
    if (sweeps is None) == (lists is None):
        raise _lib.PreworldHipError('ray_table takes either sweeps= or lists=')
    H, W = int(frames_u8.shape[1]), int(frames_u8.shape[2])
    dev = frames_u8.device
    ms = (ctypes.c_float * 6)(*[float(v) for v in mean_std])
    counts = torch.zeros(n_cls, device=dev, dtype=torch.int64)
    if sweeps is not None:
        sw = sweeps
        c2w, K = _ray_cams(c2w, K, sw.V, dev)
        fr = _ray_frames(frames_u8, view_frame, sw.V, H, W)
        slots, block_base, view_off = sw.count(H, W)
        cap = int(view_off[-1].item()) if capacity is None else int(capacity)
        rays = _ray_out(out, cap, dev)
        _lib.call('pw_ray_sweep_table', *sw.head(), sw.labels, sw.n_pts, sw.T, sw.N, sw.Pmax, sw.lut, sw.pose, H, W, slots,
                  slots.numel(), block_base, *fr, ms, c2w, K, max(cap, 1), rays, n_cls, counts, _lib.STREAM)
        return rays[:cap], view_off, counts
    depth_list, seg_list, view_off = lists
    depth_list, seg_list = depth_list.float().contiguous(), seg_list.float().contiguous()
    n = int(depth_list.shape[0])
    if depth_list.dim() != 2 or depth_list.shape[1] != 3 or tuple(seg_list.shape) != (n, 3):
        raise _lib.PreworldHipError('depth_list and seg_list must both be (n, 3), got %s %s' % (tuple(depth_list.shape), tuple(seg_list.shape)))
    if not isinstance(view_off, torch.Tensor):
        off = [int(v) for v in view_off]
        if off[0] != 0 or off[-1] != n or any(a > b for a, b in zip(off, off[1:])):
            raise _lib.PreworldHipError('view_off must rise from 0 to n = %d' % n)
        view_off = torch.tensor(off, dtype=_i32).to(dev, non_blocking=True)
    if view_off.dtype != _i32 or view_off.dim() != 1 or view_off.numel() < 2:
        raise _lib.PreworldHipError('view_off must be int32 (V + 1)')
    V = view_off.numel() - 1
    c2w, K = _ray_cams(c2w, K, V, dev)
    fr = _ray_frames(frames_u8, view_frame, V, H, W)
    cap = n if capacity is None else int(capacity)
    rays = _ray_out(out, cap, dev)
    if n > 0:
        slots = torch.empty(ray_slot_count(n), device=dev, dtype=torch.int64)
        _lib.call('pw_ray_lists_table', depth_list, seg_list, n, view_off, V, H, W, slots, slots.numel(), *fr, ms, c2w, K,
                  max(cap, 1), rays, n_cls, counts, _lib.STREAM)
    return rays[:cap], view_off, counts


def ray_table_weights(rays, view_off, frame_ids, dynamic_class=None, balance_weight=None, counts=None, weight_adj=0.3,
                      weight_dyn=0.0, n_cls=17):
    """ray.py:93-112 over the whole table in one launch: rays (capacity,16) and view_off, counts of ray_table; frame_ids[v] the
    frame id of view v (0 = key frame).  balance_weight (n_cls) float32, or None for the batch statistics from `counts`.
    Rows >= view_off[V] get weight 0 (torch.multinomial never draws them) and are zeroed."""
    cap = int(rays.shape[0])
    dev = rays.device
    w = torch.empty(cap, device=dev, dtype=_f32)
    if cap == 0:
        return w
    V = view_off.numel() - 1
    if not isinstance(frame_ids, torch.Tensor):
        frame_ids = torch.tensor([int(f) for f in frame_ids], dtype=_i32).to(dev, non_blocking=True)
    if frame_ids.dtype != _i32 or frame_ids.numel() != V:
        raise _lib.PreworldHipError('frame_ids must be int32 with V = %d entries' % V)
    if dynamic_class is None:
        dynamic_class = torch.zeros(0, dtype=_i32)
    dyn = torch.as_tensor(dynamic_class).to(device=dev, dtype=_i32).contiguous()
    if balance_weight is not None:
        balance_weight = torch.as_tensor(balance_weight).to(device=dev, dtype=_f32).contiguous()
        n_cls = balance_weight.numel()
    elif counts is None or counts.numel() != n_cls:
        raise _lib.PreworldHipError('ray_table_weights needs balance_weight or the int64 counts of ray_table')
    _lib.call('pw_ray_table_weights', rays, cap, view_off, V, frame_ids, balance_weight, counts, n_cls,
              dyn if dyn.numel() else None, dyn.numel(), float(weight_adj), float(weight_dyn), w, _lib.STREAM)
    return w


# ------------------------------------------------------------------------------ DepthNet tail
def depthnet_tail(x, D, C):
    """x (BN, >=D+C, H, W) DepthNet output -> (depth (BN,D,H,W) softmaxed over D,
    feat_cl (BN,H,W,C) channels-last context) -- view_transformer.py:797-801 and :189 in one pass."""
    BN, XC, H, W = x.shape
    depth = torch.empty(BN, D, H, W, device=x.device, dtype=_f32)
    feat = torch.empty(BN, H, W, C, device=x.device, dtype=_f32)
    _lib.call('pw_depthnet_tail', x, BN, XC, D, C, H * W, depth, feat, _lib.STREAM)
    return depth, feat


def stereo_cost_volume(prev, curr, frustum, k2s_sensor, intrins, post_rots, post_trans, bias=0.0):
    """DepthNet.calculate_cost_volumn (view_transformer.py:546-604).  prev/curr (B*N, C, H, W) stereo
    features (any strides; torch.channels_last storage is the fast path), frustum (D,H,W,3) the
    cv_frustum, k2s_sensor (B,N,4,4), intrins/post_rots (B,N,3,3), post_trans (B,N,3).
    Returns the softmaxed cost volume (B*N, D, H, W)."""
    BN, C, H, W = curr.shape
    D = frustum.shape[0]
    prev, curr = prev.float(), curr.float()          # no-op on fp32; keeps the strides of a dense tensor
    if tuple(frustum.shape[1:3]) != (H, W) or tuple(prev.shape) != tuple(curr.shape) or prev.stride() != curr.stride():
        raise _lib.PreworldHipError('stereo_cost_volume: prev/curr/frustum shapes or strides disagree')
    dev = curr.device
    ds = frustum[:, 0, 0, 2].contiguous().float()
    xs = frustum[0, 0, :, 0].contiguous().float()
    ys = frustum[0, :, 0, 1].contiguous().float()
    ipr, comb, tr = lss_camera_matrices(k2s_sensor, intrins, post_rots)
    out = torch.empty(BN, D, H, W, device=dev, dtype=_f32)
    sbn, sc, sy, sx = curr.stride()
    _lib.call('pw_stereo_cost_volume', _lib.strided(prev), _lib.strided(curr), BN, C, H, W, sbn, sc, sy, sx, ds, D, xs, ys, ipr,
              post_trans.reshape(BN, 3).float().contiguous(), comb, tr, intrins.reshape(BN, 9).float().contiguous(),
              post_rots.reshape(BN, 9).float().contiguous(), float(4 * W), float(4 * H), float(bias), out, _lib.STREAM)
    return out


# ------------------------------------------------------------------------------ A20 trajectory branch
def global_avgpool_ndhwc(x):
    """x (B, ..., C) channels-last -> (B, C): nn.AdaptiveAvgPool3d((1,1,1)) of
    DownScaleModule3DCustom (occupancy_head.py:187,198)."""
    B, C = x.shape[0], x.shape[-1]
    n_vox = x.numel() // (B * C)
    y = torch.empty(B, C, device=x.device, dtype=_f32)
    _lib.call('pw_global_avgpool_ndhwc', x, B, n_vox, C, y, _lib.STREAM)
    return y


_ACT = {None: 0, 'none': 0, 'relu': 1, 'softplus': 2}


def linear_act(x, weight, bias=None, act=None):
    """nn.Linear (+ReLU / Softplus) on a few rows: x (rows, in), weight (out, in) as stored."""
    rows, n_in = x.shape
    n_out = weight.shape[0]
    y = torch.empty(rows, n_out, device=x.device, dtype=_f32)
    _lib.call('pw_linear_act', x, weight, bias.contiguous() if bias is not None else None, y, rows, n_in, n_out, _ACT[act],
              _lib.STREAM)
    return y


# ------------------------------------------------------------------------------ attribute MLPs
def _row_of(r, h):
    return (r & 3) + 8 * (r >> 2) + 4 * h


def _mfma_pack_indices(n_tiles):
    """index helpers for the transposed MFMA chain (see pw_forecast.hip): for packed position
    [t][q][lane][e] returns (tile-row i, k index row_of(4q+e, lane>>5))."""
    import numpy as np
    t, q, lane, e = np.meshgrid(np.arange(n_tiles), np.arange(4), np.arange(64), np.arange(4),
                                indexing='ij')
    i, h = lane & 31, lane >> 5
    k = ((4 * q + e) & 3) + 8 * ((4 * q + e) >> 2) + 4 * h
    return t, i, k


def pack_mlp_blocks(mlps):
    """Up to three nn.Sequential(Linear(32,64), Softplus, Linear(64,n_i)[, ...]) over the same 32-channel input ->
    (w1p, w2p, b1p, b2) in the operand order pw_attr_mlp consumes: hidden block i occupies units [64i, 64i+64), its n_i
    outputs follow block i-1's in the packed output row (sum n_i <= 24); absent blocks are zero."""
    import numpy as np
    dev = mlps[0][0].weight.device
    W1 = torch.zeros(192, 32, device=dev)
    b1 = torch.zeros(192, device=dev)
    W2 = torch.zeros(32, 192, device=dev)
    b2 = torch.zeros(32, device=dev)
    row = 0
    for blk, m in enumerate(mlps):
        if tuple(m[0].weight.shape) != (64, 32) or m[2].weight.shape[1] != 64:
            raise _lib.PreworldHipError('pw_attr_mlp is built for Linear(32,64) -> Softplus -> Linear(64,n) blocks')
        n = m[2].weight.shape[0]
        W1[blk * 64:(blk + 1) * 64] = m[0].weight.float()
        b1[blk * 64:(blk + 1) * 64] = m[0].bias.float()
        W2[row:row + n, blk * 64:(blk + 1) * 64] = m[2].weight.float()
        b2[row:row + n] = m[2].bias.float()
        row += n
    if row > 24 or len(mlps) > 3:
        raise _lib.PreworldHipError('pw_attr_mlp writes 24 packed output channels from at most 3 blocks')
    t, i, k = _mfma_pack_indices(6)
    ti, ii, ki = [torch.from_numpy(a.reshape(-1)).to(dev) for a in (t, i, k)]
    w1p = W1[ti * 32 + ii, ki].contiguous()                       # W1[t*32+i][k]
    w2p = W2[ii, ti * 32 + ki].contiguous()                       # W2[i][t*32+k]
    hh, tt, rr = np.meshgrid(np.arange(2), np.arange(6), np.arange(16), indexing='ij')
    idx = tt * 32 + ((rr & 3) + 8 * (rr >> 2) + 4 * hh)
    b1p = b1[torch.from_numpy(idx.reshape(-1)).to(dev)].contiguous()
    return w1p, w2p, b1p, b2.contiguous()


def pack_attr_mlp(density_mlp, semantic_mlp, color_mlp):
    """density (2) / semantic (17) / color (3) MLPs of preworld.py:81-104 -> packed channels [0:2], [2:19], [19:22]."""
    return pack_mlp_blocks([density_mlp, semantic_mlp, color_mlp])


def attr_mlp(v_cl, packed, final_softplus=True, out=None):
    """v_cl (..., 32) channels-last -> packed attribute grid (..., 24):
    [0:2] density_prob, [2:19] semantic, [19:22] color (preworld_temporal_traj.py:231-236)."""
    w1p, w2p, b1p, b2 = packed
    n = v_cl.numel() // 32
    if out is None:
        out = torch.empty(tuple(v_cl.shape[:-1]) + (24,), device=v_cl.device, dtype=_f32)
    _lib.call('pw_attr_mlp', v_cl, n, w1p, w2p, b1p, b2, int(final_softplus), out, _lib.STREAM)
    return out


# ------------------------------------------------------------------------------ render ops
_i64 = torch.int64


def raw2alpha(density, shift, interval):
    """render_utils_cuda.raw2alpha (render_utils.cpp:120-124) -> (exp, alpha)."""
    d = density.contiguous()
    e = torch.empty_like(d)
    a = torch.empty_like(d)
    _lib.call('pw_raw2alpha', d, float(shift), float(interval), d.numel(), e, a, _lib.STREAM)
    return e, a


def raw2alpha_backward(exp, grad_back, interval):
    g = torch.empty_like(exp)
    _lib.call('pw_raw2alpha_backward', exp, grad_back.contiguous(), float(interval), exp.numel(), g, _lib.STREAM)
    return g


def alpha2weight(alpha, ray_id, n_rays):
    """render_utils_cuda.alpha2weight (render_utils.cpp:142-149) ->
    (weight, T, alphainv_last, i_start, i_end)."""
    a = alpha.contiguous()
    n = a.numel()
    dev = a.device
    w = torch.empty(n, device=dev, dtype=_f32)
    T = torch.empty(n, device=dev, dtype=_f32)
    last = torch.empty(n_rays, device=dev, dtype=_f32)
    i_s = torch.empty(n_rays, device=dev, dtype=_i64)
    i_e = torch.empty(n_rays, device=dev, dtype=_i64)
    _lib.call('pw_alpha2weight', a, ray_id.contiguous(), n, int(n_rays), w, T, last, i_s, i_e, _lib.STREAM)
    return w, T, last, i_s, i_e


def alpha2weight_backward(alpha, weight, T, alphainv_last, i_start, i_end, n_rays, grad_weights,
                          grad_last):
    g = torch.empty_like(alpha)
    _lib.call('pw_alpha2weight_backward', alpha, weight, T, alphainv_last, i_start, i_end, int(n_rays), grad_weights.contiguous(),
              grad_last.contiguous(), alpha.numel(), g, _lib.STREAM)
    return g


def cumdist_thres(dist, thres):
    """ub360_utils_cuda.cumdist_thres (ub360_utils.cpp:15-18): (R,S) float -> bool mask."""
    d = dist.contiguous()
    R, S = d.shape
    m = torch.empty(R, S, device=d.device, dtype=torch.uint8)
    _lib.call('pw_cumdist_thres', d, float(thres), R, S, m, _lib.STREAM)
    return m.bool()


class Raw2Alpha(torch.autograd.Function):
    """Drop-in for mmdet3d/models/nerf/utils.py:26-50."""

    @staticmethod
    def forward(ctx, density, shift, interval):
        exp, alpha = raw2alpha(density, shift, interval)
        if density.requires_grad:
            ctx.save_for_backward(exp)
            ctx.interval = interval
        return alpha

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_back):
        exp = ctx.saved_tensors[0]
        return raw2alpha_backward(exp, grad_back.contiguous(), ctx.interval), None, None


class Alphas2Weights(torch.autograd.Function):
    """Drop-in for mmdet3d/models/nerf/utils.py:52-68."""

    @staticmethod
    def forward(ctx, alpha, ray_id, N):
        weights, T, alphainv_last, i_start, i_end = alpha2weight(alpha, ray_id, N)
        if alpha.requires_grad:
            ctx.save_for_backward(alpha, weights, T, alphainv_last, i_start, i_end)
            ctx.n_rays = N
        return weights, alphainv_last

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_weights, grad_last):
        alpha, weights, T, alphainv_last, i_start, i_end = ctx.saved_tensors
        grad = alpha2weight_backward(alpha, weights, T, alphainv_last, i_start, i_end, ctx.n_rays,
                                     grad_weights, grad_last)
        return grad, None, None


def render_rays(rays_o, rays_d, t, grid, consts, c_sigma=0, c_sem=2, n_sem=17, c_rgb=19,
                want_debug=False):
    """Fused forward of NerfHead.render_one_scene + render_depth/semantic/color
    (nerf_head.py:165-269,331-353).  grid: packed (Z,Y,X,GC) attribute grid.  consts: 27 floats
    (see include/preworld_hip.h).  Returns dict(depth (R), semantic (R,17), color (R,3),
    alphainv_last (R) [, counts (R,3), weights (R,S), mask (R,S)])."""
    R, S = rays_o.shape[0], t.numel()
    Z, Y, X, GC = grid.shape
    dev = rays_o.device
    bf16 = grid.dtype == torch.bfloat16           # bf16 STORAGE of the packed grid (grid.to(torch.bfloat16)); fp32 arithmetic
    if not bf16 and grid.dtype != _f32:
        raise _lib.PreworldHipError('grid must be float32 or bfloat16')
    if not grid.is_cuda or not grid.is_contiguous():
        raise _lib.PreworldHipError('grid must be a contiguous device tensor')
    depth = torch.empty(R, device=dev, dtype=_f32)
    sem = torch.empty(R, n_sem, device=dev, dtype=_f32)
    rgb = torch.empty(R, 3, device=dev, dtype=_f32)
    last = torch.empty(R, device=dev, dtype=_f32)
    counts = torch.empty(R, 3, device=dev, dtype=_i32) if want_debug else None
    weights = torch.empty(R, S, device=dev, dtype=_f32) if want_debug else None
    mask = torch.empty(R, S, device=dev, dtype=torch.uint8) if want_debug else None
    ch = (ctypes.c_float * 27)(*[float(v) for v in consts])
    _lib.call('pw_render_rays', rays_o.contiguous(), rays_d.contiguous(), R, t, S, _f32_typed(grid), X, Y, Z, GC, c_sigma, c_sem,
              n_sem, c_rgb, ch, depth, sem, rgb, last, counts, weights, mask, int(bf16), _lib.STREAM)
    out = dict(depth=depth, semantic=sem, color=rgb, alphainv_last=last)
    if want_debug:
        out.update(counts=counts, weights=weights, mask=mask.bool())
    return out


_VIEW_OUTPUTS = {'depth': (_f32, ()), 'cls': (torch.uint8, ()), 'sem': (_f32, (17,)), 'color': (_f32, (3,)),
                 'alphainv_last': (_f32, ()), 'rgb8': (torch.uint8, (3,))}


def _view_args(who, first, K, c2w, hw, outputs, allowed, palette):
    """shared checks of render_views / render_label_views (a host tensor raises PreworldHipError here: the package has no CPU path),
    then the output tensors; the callers check what is theirs BEFORE calling this, so nothing is allocated for a refused call"""
    if not isinstance(first, torch.Tensor) or not first.is_cuda:
        raise _lib.PreworldHipError('%s: the grid must be a CUDA(HIP) tensor (there is no CPU fallback)' % who)
    if K.dim() != 3 or tuple(K.shape[1:]) != (3, 3) or c2w.dim() != 3 or tuple(c2w.shape[1:]) != (4, 4) or K.shape[0] != c2w.shape[0]:
        raise _lib.PreworldHipError('%s: K must be (V,3,3) and c2w (V,4,4), got %s and %s' % (who, tuple(K.shape), tuple(c2w.shape)))
    outputs = tuple(outputs)
    bad = [o for o in outputs if o not in allowed]
    if bad or not outputs:
        raise _lib.PreworldHipError('%s: outputs must be a non-empty subset of %s, got %s' % (who, allowed, outputs))
    if 'rgb8' in outputs:
        if palette is None:
            raise _lib.PreworldHipError('%s: output rgb8 needs a palette' % who)
        if palette.dtype != torch.uint8 or palette.dim() != 2 or palette.shape[1] != 3:
            raise _lib.PreworldHipError('%s: palette must be (n, 3) uint8' % who)
    V, (H, W) = K.shape[0], hw
    out = {o: torch.empty((V, int(H), int(W)) + _VIEW_OUTPUTS[o][1], device=first.device, dtype=_VIEW_OUTPUTS[o][0]) for o in outputs}
    return V, int(H), int(W), out


def render_views(grid, K, c2w, hw, consts, t, stride=1, origin=(0, 0), outputs=('depth', 'cls', 'color'), palette=None,
                 min_opacity=0.0, c_sigma=0, c_sem=2, n_sem=17, c_rgb=19):
    """V dense camera views of the packed (Z,Y,X,GC) attribute grid in ONE launch (pw_render_views: the rays of ray.py:34-45,50
    generated per pixel + the march of render_rays, one lane per ray).  K (V,3,3), c2w (V,4,4) device tensors; hw = (H, W) of
    the OUTPUT; output pixel (i, j) looks through source pixel (x, y) = (origin[0] + j stride, origin[1] + i stride).
    consts / t as render_rays.  outputs: any of depth (V,H,W), cls u8 (V,H,W), sem (V,H,W,17), color (V,H,W,3),
    alphainv_last (V,H,W), rgb8 u8 (V,H,W,3) = palette[cls] with palette u8 (n_sem+1,3) on the device.  min_opacity > 0:
    pixels with 1 - alphainv_last below it get cls = n_sem.  Returns a dict of device tensors; no host sync (capturable)."""
    if not isinstance(grid, torch.Tensor) or not grid.is_cuda:
        raise _lib.PreworldHipError('render_views: the grid must be a CUDA(HIP) tensor (there is no CPU fallback)')
    bf16 = grid.dtype == torch.bfloat16
    if not bf16 and grid.dtype != _f32:
        raise _lib.PreworldHipError('render_views: the packed grid must be float32 or bfloat16 (uint8 labels go through render_label_views)')
    if grid.dim() != 4 or not grid.is_contiguous():
        raise _lib.PreworldHipError('render_views: grid must be a contiguous (Z,Y,X,GC) tensor')
    if palette is not None and 'rgb8' in outputs and palette.shape[0] != n_sem + 1:
        raise _lib.PreworldHipError('render_views: palette must have n_sem + 1 = %d rows' % (n_sem + 1))
    V, H, W, out = _view_args('render_views', grid, K, c2w, hw, outputs, tuple(_VIEW_OUTPUTS), palette)
    Z, Y, X, GC = grid.shape
    ch = (ctypes.c_float * 27)(*[float(v) for v in consts])
    _lib.call('pw_render_views', K, c2w, V, H, W, int(origin[0]), int(origin[1]), int(stride), t, t.numel(), _f32_typed(grid), X, Y,
              Z, GC, c_sigma, c_sem, n_sem, c_rgb, ch, out.get('depth'), out.get('cls'), out.get('sem'), out.get('color'),
              out.get('alphainv_last'), out.get('rgb8'), palette, float(min_opacity), int(bf16), _lib.STREAM)
    return out


def render_label_views(occ_u8, K, c2w, hw, consts, t, empty_idx=17, stride=1, origin=(0, 0), outputs=('depth', 'cls'), palette=None):
    """render_views in LABEL MODE (pw_render_label_views): occ_u8 is a uint8 (X,Y,Z) label grid on the device with ANY strides
    (the (X,Y,Z)-contiguous semantic_occ_* arrays, or the permuted view of the OccHead's (Z,Y,X) buffer).  Same rays, samples and
    inner | cumdist mask as the soft path; a sample's voxel is floor(u + 0.5) per axis of the align_corners=True continuous
    index u (outside = miss); the first kept sample whose label is not empty_idx is the hit: cls = label,
    depth = (s_hit + 1e-7) radius, alphainv_last = 0; no hit: cls = empty_idx, depth = 1e-7 radius, alphainv_last = 1.
    outputs: any of depth, cls, alphainv_last, rgb8 (= palette[cls])."""
    if not isinstance(occ_u8, torch.Tensor) or not occ_u8.is_cuda:
        raise _lib.PreworldHipError('render_label_views: the label grid must be a CUDA(HIP) tensor (there is no CPU fallback)')
    if occ_u8.dtype != torch.uint8 or occ_u8.dim() != 3:
        raise _lib.PreworldHipError('render_label_views: the label grid must be a uint8 (X,Y,Z) tensor')
    sx, sy, sz = occ_u8.stride()
    if min(sx, sy, sz) <= 0:
        raise _lib.PreworldHipError('render_label_views: the label grid must have positive strides')
    V, H, W, out = _view_args('render_label_views', occ_u8, K, c2w, hw, outputs, ('depth', 'cls', 'alphainv_last', 'rgb8'), palette)
    X, Y, Z = occ_u8.shape
    ch = (ctypes.c_float * 27)(*[float(v) for v in consts])
    _lib.call('pw_render_label_views', K, c2w, V, H, W, int(origin[0]), int(origin[1]), int(stride), t, t.numel(),
              _lib.strided(occ_u8), X, Y, Z, sx, sy, sz, int(empty_idx), ch, out.get('depth'), out.get('cls'),
              out.get('alphainv_last'), out.get('rgb8'), palette, 0 if palette is None else palette.shape[0], _lib.STREAM)
    return out


def render_rays_backward(rays_o, rays_d, t, grid, consts, g_depth, g_sem, g_rgb, g_last, g_weights=None, c_sigma=0, c_sem=2,
                         n_sem=17, c_rgb=19, grad_grid=None, algo=None, max_entries=0):
    """Backward of render_rays: gradient of the packed (Z,Y,X,GC) grid given the gradients of depth (R), semantic (R,17),
    color (R,3), alphainv_last (R) [and of the dense weights (R,S)].
    algo 'sorted' (default): pw_render_rays_backward_sorted -- entries sorted by voxel,
    fixed-point segmented sums, no float atomics, bit-reproducible; 'atomics': pw_render_rays_backward (168 float atomics per
    kept sample, arrival order decides the last bits; kept for A/B).  max_entries: upper bound of the (sample, corner) entries of the
    sorted form -- 8 x render_rays' counts[:, 1].sum() -- which sizes its workspace (0: worst case, 40 B x R x S x 8)."""
    import os
    R, S = rays_o.shape[0], t.numel()
    Z, Y, X, GC = grid.shape
    if grad_grid is None:
        grad_grid = torch.zeros_like(grid)
    if R == 0:
        return grad_grid
    algo = algo or 'sorted'
    ch = (ctypes.c_float * 27)(*[float(v) for v in consts])
    gw = g_weights.contiguous() if g_weights is not None else None
    args = (rays_o.contiguous(), rays_d.contiguous(), R, t, S, grid, X, Y, Z, GC, c_sigma, c_sem, n_sem, c_rgb, ch,
            g_depth.contiguous(), g_sem.contiguous(), g_rgb.contiguous(), g_last.contiguous(), gw)
    if algo == 'atomics':
        _lib.call('pw_render_rays_backward', *args, grad_grid, _lib.STREAM)
        return grad_grid
    g20 = torch.cat([g_sem.float(), g_rgb.float()], dim=1).contiguous()
    gmax = g20.abs().max().reshape(1).contiguous()
    nbytes = _lib.call_size('pw_render_backward_workspace_bytes', R, S, X, Y, Z, int(max_entries))
    ws = _workspace(nbytes, grid.device)
    off = (-ws.data_ptr()) % 256
    _lib.call('pw_render_rays_backward_sorted', *args, g20, gmax, ws[off:], nbytes, int(max_entries), grad_grid, _lib.STREAM)
    return grad_grid


_PINNED = []          # spare pinned int64[1] buffers (hipHostMalloc is slow: reused)


def _async_host_scalar(t):
    """start the copy of a device scalar to the host and return poll() -> its value as an int once it has arrived, else None (never
    blocks, never synchronises)"""
    buf = _PINNED.pop() if _PINNED else torch.empty(1, dtype=torch.int64, pin_memory=True)
    buf.copy_(t.reshape(1), non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    state = {}

    def poll():
        if 'v' not in state and ev.query():
            state['v'] = int(buf[0])
            _PINNED.append(buf)
        return state.get('v')
    return poll


class RenderRays(torch.autograd.Function):
    """Differentiable fused render head: forward = pw_render_rays, backward = pw_render_rays_backward.  Replaces the autograd
    graph the reference builds through 3x F.grid_sample, Raw2Alpha, Alphas2Weights and 3x segment_coo
    (nerf_head.py:165-269,331-353; utils.py:26-68).  Returns (depth, semantic, color, alphainv_last, weights (R,S) dense)."""

    @staticmethod
    def forward(ctx, grid, rays_o, rays_d, t, consts):
        grid = grid.contiguous()
        out = render_rays(rays_o, rays_d, t, grid, consts, want_debug=True)
        ctx.save_for_backward(grid, rays_o, rays_d, t)
        ctx.consts = tuple(float(v) for v in consts)
        # how many samples passed the alpha threshold: on its way to the host without anyone waiting for it; if it has arrived by
        # the time the backward runs, the backward's entry arrays are sized by it instead of by the worst case (5.1 GB at 38 400 x 417)
        ctx.kept = _async_host_scalar(out['counts'][:, 1].sum(dtype=torch.int64))
        return out['depth'], out['semantic'], out['color'], out['alphainv_last'], out['weights']

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_depth, g_sem, g_rgb, g_last, g_w):
        grid, rays_o, rays_d, t = ctx.saved_tensors
        kept = ctx.kept()
        gg = render_rays_backward(rays_o, rays_d, t, grid, ctx.consts, g_depth, g_sem, g_rgb, g_last, g_w,
                                  max_entries=0 if kept is None else 8 * max(kept, 1))
        return gg, None, None, None, None


class _Distortion(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w, s):
        R, S_ = w.shape
        nbytes = _lib.call_size('pw_distortion_workspace_bytes', R)
        ws = _workspace(nbytes, w.device)
        out = torch.empty(3, device=w.device, dtype=_f32)
        _lib.call('pw_distortion_loss', w, s, R, S_, ws, nbytes, out[0:1], out[1:3], _lib.STREAM)
        ctx.save_for_backward(w, s, out)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        w, s, out = ctx.saved_tensors
        gw = torch.empty_like(w)
        _lib.call('pw_distortion_loss_backward', w, s, w.shape[0], w.shape[1], out[1:3], g.reshape(1).float().contiguous(), gw,
                  _lib.STREAM)
        return gw, None


def distortion_loss(weights, s):
    """flatten_eff_distloss (torch_efficient_distloss, called at nerf_head.py:316-327) on the dense (R, S) render weights (0 where a
    sample was culled) and the normalised sample positions s (S,): sum over rays of (1/3) sum w_i^2 / n_kept + 2 sum_i w_i (s_i
    sum_{j<i} w_j - sum_{j<i} w_j s_j), divided by 1 + the index of the last ray that kept a sample (pw_distortion_loss); autograd
    through pw_distortion_loss_backward."""
    if weights.dim() != 2 or s.numel() != weights.shape[1]:
        raise _lib.PreworldHipError('distortion_loss: weights (R, S), s (S,)')
    if weights.shape[0] == 0 or weights.shape[1] == 0:          # an empty ray batch: flatten_eff_distloss' sums are empty, the loss 0
        return weights.sum() * 0.0
    return _Distortion.apply(_chk_t(weights), _chk_t(s.reshape(-1)))


def _chk_t(t):
    return t if (t.dtype == _f32 and t.is_contiguous()) else t.float().contiguous()


def confusion_hist(pred, gt, mask, n_cl, hist):
    """hist (n_cl,n_cl) int64 += bincount(n_cl*gt + pred) over (masked) voxels -- occ_metrics.py:82-105."""
    p = pred.contiguous().view(-1)
    g = gt.contiguous().view(-1)
    m = mask.contiguous().view(-1).to(torch.uint8) if mask is not None else None
    if p.dtype != torch.uint8 or g.dtype != torch.uint8:
        raise _lib.PreworldHipError('pred/gt must be uint8')
    _lib.call('pw_confusion_hist', p, g, m, p.numel(), int(n_cl), hist, _lib.STREAM)
    return hist


OCC_SCORE_MAX_H = 8


def occ_score_bins(n_cl):
    """entries per horizon of an occ_score table: the n_cl x n_cl confusion matrix, then the binary 2x2 histogram"""
    return int(n_cl) * int(n_cl) + 4


def occ_score(preds, gts, masks, n_cl, counts):
    """counts (H, n_cl*n_cl + 4) int64 += one sample's scores for H <= 8 horizons in ONE launch (pw_occ_score): per horizon h the
    confusion matrix of occ_metrics.py:82-105 over masked voxels with gt < n_cl, then the binary free / occupied 2x2 histogram of
    occ_metrics.py:150-154 (gt = 255 counts as occupied there).  preds / gts: H contiguous uint8 device grids of one voxel count;
    masks: None or H uint8 / bool device grids (an entry None: no mask for that horizon).  Capturable: the pointers travel by value."""
    H = len(preds)
    if H < 1 or H > OCC_SCORE_MAX_H or len(gts) != H or (masks is not None and len(masks) != H):
        raise _lib.PreworldHipError('occ_score: 1 <= H <= %d horizons, one gt (and mask) per prediction' % OCC_SCORE_MAX_H)
    n = preds[0].numel()
    if any(t.numel() != n for t in list(preds) + list(gts) + [m for m in (masks or ()) if m is not None]):
        raise _lib.PreworldHipError('occ_score: every grid must hold the same number of voxels')
    if tuple(counts.shape) != (H, occ_score_bins(n_cl)):
        raise _lib.PreworldHipError('occ_score: counts must be (H, n_cl*n_cl + 4) = (%d, %d), got %s'
                                    % (H, occ_score_bins(n_cl), tuple(counts.shape)))
    M = None
    if masks is not None:
        M = _lib.table(None if m is None else m.view(torch.uint8) if m.dtype == torch.bool else m for m in masks)
    _lib.call('pw_occ_score', _lib.table(preds), _lib.table(gts), M, H, n, int(n_cl), counts, _lib.STREAM)
    return counts


OCC_FSCORE_MAX_H = 8
OCC_FSCORE_MAX_Z = 64
OCC_FSCORE_MAX_R = 7


def fscore_offsets(threshold, voxel_size):
    """The lattice form of occ_metrics.py:383-397's `distance < threshold`: an int8 table m of shape (2rx + 1, 2ry + 1), where a
    voxel at integer offset (dx, dy, dz) from another lies closer than `threshold` (voxel centres, voxel_size = (vx, vy, vz))
    exactly when |dz| <= m[dx + rx, dy + ry]; -1: no dz at that (dx, dy).  rx / ry are the largest |dx| / |dy| with an entry.
    Distances are float64; |dz| is enumerated up to 63 (pw_occ_fscore's Z <= 64) and m is at most 63.  ValueError when some
    lattice distance lies within 1e-9 (relative) of the threshold: there the reference's answer depends on how each point's
    coordinates round, so no table reproduces it."""
    t = float(threshold)
    v = [float(x) for x in voxel_size]
    if len(v) != 3 or not all(x > 0 for x in v) or not t > 0 or not np.isfinite(t):
        raise ValueError('fscore_offsets: threshold and the three voxel sizes must be finite and > 0, got %r, %r'
                         % (threshold, voxel_size))
    r = [int(np.floor(t / x)) + 2 for x in v]
    if max(r[:2]) > 64:
        raise ValueError('fscore_offsets: threshold %r spans more than 63 columns of voxel size %r' % (threshold, voxel_size))
    r[2] = min(r[2], 63)
    dx, dy, dz = (np.arange(-k, k + 1, dtype=np.float64) * x for k, x in zip(r, v))
    d = np.sqrt(dx[:, None, None] ** 2 + dy[None, :, None] ** 2 + dz[None, None, :] ** 2)
    if np.any(np.abs(d - t) <= 1e-9 * t):
        raise ValueError('fscore_offsets: a lattice distance of voxel size %r ties threshold %r (within 1e-9): the answer '
                         'would depend on per-point rounding' % (tuple(voxel_size), threshold))
    absz = np.abs(np.arange(-r[2], r[2] + 1))
    m = np.where(d < t, absz[None, None, :], -1).max(axis=2)
    used = m >= 0
    rx = int(np.abs(np.arange(-r[0], r[0] + 1))[used.any(axis=1)].max())
    ry = int(np.abs(np.arange(-r[1], r[1] + 1))[used.any(axis=0)].max())
    return m[r[0] - rx:r[0] + rx + 1, r[1] - ry:r[1] + ry + 1].astype(np.int8)


def _fscore_pad(m, rx, ry):
    out = np.full((2 * rx + 1, 2 * ry + 1), -1, dtype=np.int8)
    a, b = (m.shape[0] - 1) // 2, (m.shape[1] - 1) // 2
    out[rx - a:rx + a + 1, ry - b:ry + b + 1] = m
    return out


@functools.lru_cache(maxsize=64)
def _fscore_args(void, voxel_size, thr_acc, thr_cmpl):
    """(void bitset, m_acc, m_cmpl, rx, ry) as ctypes arguments of pw_occ_fscore, both tables on one (rx, ry) window"""
    if any(not 0 <= int(v) <= 255 for v in void):
        raise ValueError('occ_fscore: void values must lie in [0, 255], got %r' % (void,))
    bits = np.zeros(8, dtype=np.uint32)
    for v in void:
        bits[int(v) >> 5] |= np.uint32(1 << (int(v) & 31))
    ma, mc = fscore_offsets(thr_acc, voxel_size), fscore_offsets(thr_cmpl, voxel_size)
    rx = (max(ma.shape[0], mc.shape[0]) - 1) // 2
    ry = (max(ma.shape[1], mc.shape[1]) - 1) // 2
    ma, mc = _fscore_pad(ma, rx, ry).reshape(-1), _fscore_pad(mc, rx, ry).reshape(-1)
    return ((ctypes.c_uint32 * 8)(*[int(b) for b in bits]), (ctypes.c_int8 * ma.size)(*[int(x) for x in ma]),
            (ctypes.c_int8 * mc.size)(*[int(x) for x in mc]), rx, ry)


def occ_fscore(preds, gts, masks, table, void=(17, 255), voxel_size=(0.4, 0.4, 0.4), thr_acc=0.6, thr_cmpl=0.6):
    """table (H, 4) int64 += one sample's F-score counts {n_pred, n_pred_hit, n_gt, n_gt_hit} for H <= 8 horizons in ONE launch
    (pw_occ_fscore; occ_metrics.py:322-410 Metric_FScore restated on the lattice, see fscore_offsets).  preds / gts: H contiguous
    uint8 (X, Y, Z) device grids of one shape, Z <= 64; masks: None or H uint8 / bool device grids (an entry None: no mask;
    where a mask is 0 pred and gt read as 255).  A voxel is occupied when its value is not in `void`.  Capturable: the pointers
    and tables travel by value."""
    H = len(preds)
    if H < 1 or H > OCC_FSCORE_MAX_H or len(gts) != H or (masks is not None and len(masks) != H):
        raise _lib.PreworldHipError('occ_fscore: 1 <= H <= %d horizons, one gt (and mask) per prediction' % OCC_FSCORE_MAX_H)
    shape = tuple(preds[0].shape)
    if len(shape) != 3 or any(tuple(t.shape) != shape for t in list(preds) + list(gts) + [m for m in (masks or ()) if m is not None]):
        raise _lib.PreworldHipError('occ_fscore: every grid must be (X, Y, Z) of one shape, got %s'
                                    % [tuple(t.shape) for t in preds])
    if tuple(table.shape) != (H, 4):
        raise _lib.PreworldHipError('occ_fscore: table must be (H, 4) = (%d, 4), got %s' % (H, tuple(table.shape)))
    vb, ma, mc, rx, ry = _fscore_args(tuple(int(v) for v in void), tuple(float(v) for v in voxel_size), float(thr_acc),
                                      float(thr_cmpl))
    M = None
    if masks is not None:
        M = _lib.table(None if m is None else m.view(torch.uint8) if m.dtype == torch.bool else m for m in masks)
    _lib.call('pw_occ_fscore', _lib.table(preds), _lib.table(gts), M, H, shape[0], shape[1], shape[2], vb, ma, mc, rx, ry, table,
              _lib.STREAM)
    return table


def occ_fscore_accumulate(table, totals, empty):
    """totals (H, 3) float64 += (accuracy, completeness, F1) of every sample of table ((H, 4) or (n_s, H, 4) int64, from
    occ_fscore), in sample order, with occ_metrics.py:399-408's float64 arithmetic; empty (H,) int64 counts the samples with a
    non-empty prediction and an empty ground truth (the reference raises there; they add (0, 0, 0)).  ONE launch
    (pw_occ_fscore_accumulate), no host sync."""
    t = table.reshape(-1, *table.shape[-2:]) if table.dim() >= 2 else table
    if t.dim() != 3 or t.shape[-1] != 4:
        raise _lib.PreworldHipError('occ_fscore_accumulate: table must be (H, 4) or (n_s, H, 4), got %s' % (tuple(table.shape),))
    H = t.shape[1]
    if tuple(totals.shape) != (H, 3) or tuple(empty.shape) != (H,):
        raise _lib.PreworldHipError('occ_fscore_accumulate: totals (%d, 3) float64 and empty (%d,) int64, got %s and %s'
                                    % (H, H, tuple(totals.shape), tuple(empty.shape)))
    _lib.call('pw_occ_fscore_accumulate', t, t.shape[0], H, totals, empty, _lib.STREAM)
    return totals


# ------------------------------------------------------------------------------ camera frames to network input
IMAGE_PREP_NPARAM = _lib.PW['PW_IMAGE_PREP_NPARAM']
IMAGE_PREP_TILE = (_lib.PW['PW_IMAGE_PREP_TH'], _lib.PW['PW_IMAGE_PREP_TW'])
_PREC = 22


def _bicubic(x):
    """Keys' cubic with a = -0.5 on an array of float64 offsets, the two polynomial pieces as Pillow writes them"""
    a = -0.5
    x = np.abs(x)
    inner = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    outer = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, inner, np.where(x < 2.0, outer, 0.0))


@functools.lru_cache(maxsize=1024)
def image_resize_table(n_in, n_out):
    """Pillow's 8 bpc bicubic (a = -0.5, antialiased) coefficients of one axis n_in -> n_out, built in float64 in Pillow's
    operation order (Resample.c precompute_coeffs, normalize_coeffs_8bpc): (bounds (n_out,2) int32 [first source index, taps],
    coefs (n_out,ksize) int32, 22-bit fixed point).  All outputs at once, tap by tap, so that the weight sum of an output is
    formed in tap order as the C loop forms it.  n_in == n_out is the identity (PIL skips that pass).  Cached per pair (the
    released training range reaches about 230 widths and 130 heights); the arrays are shared, hence read-only."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in == n_out:
        bounds = np.stack([np.arange(n_out), np.ones(n_out, np.int64)], 1).astype(np.int32)
        coefs = np.full((n_out, 1), 1 << _PREC, np.int32)
    else:
        scale = float(n_in) / float(n_out)
        fs = scale if scale > 1.0 else 1.0
        support = 2.0 * fs
        ksize = int(np.ceil(support)) * 2 + 1
        inv = 1.0 / fs
        center = (np.arange(n_out) + 0.5) * scale
        first = np.maximum((center - support + 0.5).astype(np.int64), 0)              # the casts truncate, like C's (int)
        taps = np.minimum((center + support + 0.5).astype(np.int64), n_in) - first
        w = np.zeros((n_out, ksize))
        total = np.zeros(n_out)
        for k in range(ksize):
            w[:, k] = np.where(k < taps, _bicubic((k + first - center + 0.5) * inv), 0.0)
            total = total + w[:, k]
        has = total != 0.0
        w[has] = w[has] / total[has][:, None]
        q = w * float(1 << _PREC)
        coefs = np.where(w < 0, np.trunc(-0.5 + q), np.trunc(0.5 + q)).astype(np.int32)
        bounds = np.stack([first, taps], 1).astype(np.int32)
    bounds.setflags(write=False)
    coefs.setflags(write=False)
    return bounds, coefs


def image_rotation_fixed(angle, w, h):
    """The six 16.16 integers a0..a5 of PIL's Image.rotate(angle) on a w x h image (nearest, about the centre, no expand):
    output (x, y) reads ((a2 + a1 y + a0 x) >> 16, (a5 + a4 y + a3 x) >> 16)."""
    import math
    if not abs(angle) < 45:
        raise _lib.PreworldHipError('image rotation must satisfy |angle| < 45 degrees, got %r' % (angle,))
    t = -math.radians(angle % 360.0)
    m0, m1 = round(math.cos(t), 15), round(math.sin(t), 15)
    m3, m4 = round(-math.sin(t), 15), round(math.cos(t), 15)
    cx, cy = w / 2.0, h / 2.0
    m2 = m0 * -cx + m1 * -cy + 0.0 + cx
    m5 = m3 * -cx + m4 * -cy + 0.0 + cy
    fix = lambda v: int(math.floor(v * 65536.0 + 0.5))      # noqa: E731
    return (fix(m0), fix(m1), fix(m2 + m0 * 0.5 + m1 * 0.5), fix(m3), fix(m4), fix(m5 + m3 * 0.5 + m4 * 0.5))


class ImagePrepPlan:
    """What pw_image_prep needs besides the pixels, resident on the device: `tables` (int32), `params` (M, 16) int32, and the
    host-side numbers of the call.  `host_params` / `host_tables` / `offsets` keep the host copies for inspection."""
    pass


def _image_prep_host(src_hw, input_size, augs):
    H, W = int(src_hw[0]), int(src_hw[1])
    fH, fW = int(input_size[0]), int(input_size[1])
    if H < 1 or W < 1 or fH < 1 or fW < 1 or max(H, W, fH, fW) > 32767:
        raise _lib.PreworldHipError('image_prep_plan: sizes must be 1 .. 32767, got %r -> %r' % (src_hw, input_size))
    if len(augs) < 1:
        raise _lib.PreworldHipError('image_prep_plan: no images')
    TH = IMAGE_PREP_TILE[0]
    chunks, offsets, n_table = [], {}, 0

    def table(n_in, n_out):
        nonlocal n_table
        key = (n_in, n_out)
        if key not in offsets:
            b, c = image_resize_table(n_in, n_out)
            offsets[key] = (n_table, c.shape[1])
            chunks.extend([b.reshape(-1), c.reshape(-1)])
            n_table += b.size + c.size
        return offsets[key]
    params = np.zeros((len(augs), IMAGE_PREP_NPARAM), np.int32)
    rows_max = 1
    for i, (dims, crop, flip, angle) in enumerate(augs):
        newW, newH = int(dims[0]), int(dims[1])
        x0, y0, x1, y1 = [int(v) for v in crop]
        if newW < 1 or newH < 1 or max(newW, newH) > 32767:
            raise _lib.PreworldHipError('image_prep_plan: image %d: resize dims %r out of range' % (i, dims))
        if x1 - x0 != fW or y1 - y0 != fH:
            raise _lib.PreworldHipError('image_prep_plan: image %d: crop %r is not input_size %r' % (i, crop, (fH, fW)))
        if max(abs(x0), abs(y0)) > 65535:
            raise _lib.PreworldHipError('image_prep_plan: image %d: crop origin out of range' % i)
        angle = float(angle)
        rot = angle % 360.0 != 0
        a = image_rotation_fixed(angle, fW, fH) if rot else (65536, 0, 0, 0, 65536, 0)
        (hoff, hks), (voff, vks) = table(W, newW), table(H, newH)
        params[i] = (newW, newH, x0, y0, 1 if flip else 0, 1 if rot else 0) + tuple(a) + (hoff, hks, voff, vks)
        vb = image_resize_table(H, newH)[0].astype(np.int64)
        oy0 = np.arange(0, fH, TH)                  # the band of source rows each tile row stages in LDS
        ra, rb = np.maximum(oy0 + y0, 0), np.minimum(np.minimum(oy0 + TH, fH) - 1 + y0, newH - 1)
        ra, rb = ra[ra <= rb], rb[ra <= rb]
        if ra.size:
            rows_max = max(rows_max, int((vb[rb, 0] + vb[rb, 1] - vb[ra, 0]).max()))
    if rows_max > 224:
        raise _lib.PreworldHipError('image_prep_plan: a %d-row band of the output needs %d source rows; the kernel stages at most 224 '
                                    '(down-scaling beyond about 6.5x is not supported)' % (TH, rows_max))
    return H, W, fH, fW, params, np.concatenate(chunks).astype(np.int32), offsets, rows_max


def image_prep_plan(src_hw, input_size, augs, device='cuda'):
    """Plan of ops.prepare_images for M = len(augs) frames of src_hw = (H, W) going to input_size = (fH, fW).  augs: per image
    (resize_dims (newW, newH), crop (x0, y0, x1, y1), flip, rotate degrees), the tuple the reference's sample_augmentation
    returns without its first entry (loading_traj_temporal.py:303-329).  Builds PIL's coefficient tables (cached per axis pair)
    and the per-image parameters on the host and copies them to the device once; a plan is reused for every call with the same
    augmentation (the test-time one is a constant)."""
    H, W, fH, fW, params, tables, offsets, rows_max = _image_prep_host(src_hw, input_size, augs)
    p = ImagePrepPlan()
    p.src_hw, p.input_size, p.M, p.rows_max = (H, W), (fH, fW), len(augs), rows_max
    p.any_rot = bool(params[:, 5].any())
    p.host_params, p.host_tables, p.offsets = params, tables, offsets
    p.device = torch.device(device)
    p.params = torch.from_numpy(params).to(p.device)
    p.tables = torch.from_numpy(tables).to(p.device)
    p.ws = _workspace(_lib.call_size('pw_image_prep_ws_bytes', p.M, fH, fW, 1), p.device) if p.any_rot else None
    p.launches = None
    return p


def prepare_images(src_u8, plan, out=None, canvas=None):
    """img_transform_core + mmlabNormalize (mmdet3d/datasets/pipelines/loading_traj_temporal.py:283-290, 173-180) for all frames
    of a call: src_u8 (M,H,W,3) uint8 RGB on the device -> (M,3,fH,fW) float32, plane 0 blue (the reference's to_rgb on RGB
    input).  canvas: optional (M,fH,fW,3) uint8 that receives the transformed image before normalisation (results['canvas']),
    bit-equal to PIL's.  No host-to-device copy and no synchronisation happen here; `plan.launches` is the number of kernel
    launches the call enqueued as the library reports it: 1 when no image is rotated, 2 otherwise."""
    H, W = plan.src_hw
    fH, fW = plan.input_size
    if not isinstance(src_u8, torch.Tensor) or tuple(src_u8.shape) != (plan.M, H, W, 3):
        raise _lib.PreworldHipError('src_u8 must be a (%d,%d,%d,3) tensor, got %s' % (plan.M, H, W, tuple(getattr(src_u8, 'shape', ()))))
    if out is None:
        out = torch.empty(plan.M, 3, fH, fW, device=src_u8.device, dtype=_f32)
    elif tuple(out.shape) != (plan.M, 3, fH, fW):
        raise _lib.PreworldHipError('out must be (%d,3,%d,%d)' % (plan.M, fH, fW))
    if canvas is not None and tuple(canvas.shape) != (plan.M, fH, fW, 3):
        raise _lib.PreworldHipError('canvas must be (%d,%d,%d,3)' % (plan.M, fH, fW))
    n = ctypes.c_int(0)
    _lib.call('pw_image_prep', src_u8, plan.M, H, W, fH, fW, plan.params, plan.tables, plan.tables.numel(), plan.rows_max,
              int(plan.any_rot), plan.ws, out, canvas, ctypes.byref(n), _lib.STREAM)
    plan.launches = n.value
    return out


# ------------------------------------------------------------------------------ the optimizer step (preworld_amd/optim.py)
OPTIM_LAUNCHES = {'sqnorm': 0, 'update': 0}       # kernel launches the two wrappers below enqueued (tests count them)


def optim_plan(p, g, m, v, e, weight_decay, lr_mul, group):
    """Lay out the device plan of pw_optim_sqnorm / pw_optim_update for rows of fp32 device tensors: p[i] with g / m / v [i] all
    tensors (an optimizer row) or all None (an EMA-only row), e[i] the shadow or None.  Returns (plan_host, n_chunks): a pinned
    int64 host tensor for ONE asynchronous copy to the device, and the chunk count.  Nothing is dereferenced or launched."""
    n = len(p)
    numel = torch.tensor([t.numel() for t in p], dtype=torch.int64)
    tabs = [_lib.table(x) for x in (p, g, m, v, e)]
    nbytes = _lib.call_size('pw_optim_plan_bytes', n, numel, *tabs)
    if nbytes < 0:
        raise _lib.PreworldHipError('pw_optim_plan_bytes failed: %s' % _lib.lib().pw_last_error().decode())
    plan = torch.empty(nbytes // 8, dtype=torch.int64, pin_memory=torch.cuda.is_available())
    n_chunks = torch.zeros(1, dtype=torch.int64)
    _lib.call('pw_optim_plan_layout', n, numel, *tabs, torch.tensor(weight_decay, dtype=torch.float64).reshape(n),
              torch.tensor(lr_mul, dtype=torch.float64).reshape(n), torch.tensor(group, dtype=_i32).reshape(n), plan, nbytes, n_chunks)
    return plan, int(n_chunks[0])


def optim_sqnorm(plan, n_rows, n_chunks, slab):
    """launch 1: per-block partial sums of g*g in double into slab (clip_grad_norm_'s norm, first half)"""
    _lib.call('pw_optim_sqnorm', plan, plan.numel() * 8, n_rows, n_chunks, slab, _lib.STREAM)
    OPTIM_LAUNCHES['sqnorm'] += 1


def optim_update(plan, n_rows, n_chunks, hyper, n_groups, slab, ctr, ema_updates, norm_out, use_norm, clip, use_ema, skip_nonfinite):
    """launch 2: the clipped AdamW update (torch/optim/adam.py single-tensor path) and ModelEMA.update's blend (core/hook/ema.py:48-59)"""
    _lib.call('pw_optim_update', plan, plan.numel() * 8, n_rows, n_chunks, hyper, n_groups, slab, int(use_norm), int(clip),
              int(use_ema), int(skip_nonfinite), ctr, ema_updates, norm_out, _lib.STREAM)
    OPTIM_LAUNCHES['update'] += 1


# ------------------------------------------------------------------------------ Swin window attention (preworld_amd/image_encoder.py)
SWIN_MAX_WS, SWIN_MAX_HEAD_DIM = _lib.PW_SWIN['PW_SWIN_MAX_WS'], _lib.PW_SWIN['PW_SWIN_MAX_HEAD_DIM']


def swin_attention_supported(embed_dims, num_heads, ws):
    """None if pw_swin_window_attention takes this (embed_dims, num_heads, window), else the reason it does not"""
    if embed_dims % num_heads:
        return 'embed_dims %d is no multiple of num_heads %d' % (embed_dims, num_heads)
    d = embed_dims // num_heads
    if not 2 <= ws <= SWIN_MAX_WS:
        return 'window %d outside 2 .. %d' % (ws, SWIN_MAX_WS)
    if d > SWIN_MAX_HEAD_DIM or d % 4:
        return 'head width %d (supported: multiples of 4 up to %d)' % (d, SWIN_MAX_HEAD_DIM)
    return None


def _swin_check(fn, qkv, pad_qkv, bias_table, H, W, num_heads, ws, shift):
    """the argument checks the forward and the backward wrapper share; returns (B, C)"""
    if qkv.dim() not in (3, 4) or (qkv.dim() == 3 and qkv.shape[1] != H * W) or (qkv.dim() == 4 and tuple(qkv.shape[1:3]) != (H, W)):
        raise _lib.PreworldHipError('%s: qkv must be (B, H*W, 3C) or (B, H, W, 3C) with H, W = %d, %d, got %s' % (fn, H, W, tuple(qkv.shape)))
    if qkv.dtype not in (_f32, torch.bfloat16):
        raise _lib.PreworldHipError('%s: qkv must be float32 or bfloat16, got %s' % (fn, qkv.dtype))
    if not qkv.is_contiguous():
        raise _lib.PreworldHipError('%s: qkv must be contiguous' % fn)
    B, C3 = qkv.shape[0], qkv.shape[-1]
    if B < 1 or H < 1 or W < 1 or C3 % 3:
        raise _lib.PreworldHipError('%s: empty input or a last dimension that is no multiple of 3: %s' % (fn, tuple(qkv.shape)))
    C = C3 // 3
    why = swin_attention_supported(C, num_heads, ws)
    if why is not None:
        raise _lib.PreworldHipError('%s: not supported: %s' % (fn, why))
    if not 0 <= shift < ws:
        raise _lib.PreworldHipError('%s: need 0 <= shift < ws, got %d, %d' % (fn, shift, ws))
    if pad_qkv is not None and (tuple(pad_qkv.shape) != (C3,) or pad_qkv.dtype != qkv.dtype or not pad_qkv.is_contiguous()):
        raise _lib.PreworldHipError('%s: pad_qkv must be a contiguous (%d,) tensor of %s' % (fn, C3, qkv.dtype))
    if tuple(bias_table.shape) != ((2 * ws - 1) ** 2, num_heads) or bias_table.dtype != _f32 or not bias_table.is_contiguous():
        raise _lib.PreworldHipError('%s: bias_table must be a contiguous float32 (%d, %d) tensor, got %s %s'
                                    % (fn, (2 * ws - 1) ** 2, num_heads, bias_table.dtype, tuple(bias_table.shape)))
    return B, C


def swin_window_attention(qkv, pad_qkv, bias_table, H, W, num_heads, ws, shift, scale):
    """Shifted-window attention of one Swin block in one launch (include/preworld_hip_swin.h): qkv (B, H*W, 3C) or (B, H, W, 3C), the
    qkv Linear applied to the un-padded, un-rolled tokens, fp32 or bf16; pad_qkv (3C) in the same dtype = the Linear's output for a
    zero token (its bias) or None for zeros; bias_table ((2 ws - 1)^2, num_heads) fp32.  Returns softmax(q k^T scale + bias + mask) v
    as (B, H*W, C) / (B, H, W, C), the proj Linear's input.  Forward only; no workspace, no synchronisation."""
    B, C = _swin_check('swin_window_attention', qkv, pad_qkv, bias_table, H, W, num_heads, ws, shift)
    out = torch.empty(qkv.shape[:-1] + (C,), device=qkv.device, dtype=qkv.dtype)
    _lib.call('pw_swin_window_attention', qkv, pad_qkv, bias_table, out, B, H, W, C, num_heads, ws, shift, float(scale),
              _lib.PW_SWIN['PW_SWIN_BF16' if qkv.dtype == torch.bfloat16 else 'PW_SWIN_F32'], _lib.STREAM)
    return out


def swin_backward_workspace_bytes(B, H, W, num_heads, ws):
    """the workspace formula of include/preworld_hip_swin_bwd.h: one partial of (2 ws - 1)^2 + 64 floats per (window, head)"""
    return 4 * B * (-(-H // ws)) * (-(-W // ws)) * num_heads * ((2 * ws - 1) ** 2 + _lib.PW_SWIN_BWD['PW_SWIN_BWD_PAD_SLOTS'])


def swin_window_attention_backward(qkv, pad_qkv, bias_table, out, dout, H, W, num_heads, ws, shift, scale, need_pad=True, need_table=True):
    """Gradient of swin_window_attention in two launches (include/preworld_hip_swin_bwd.h): qkv, pad_qkv, bias_table as the forward
    took them, out what it returned, dout the gradient of out (same shape and dtype, contiguous).  Returns (dqkv like qkv,
    dpad_qkv (3C) float32 or None, dbias_table like bias_table or None); dpad_qkv is None when pad_qkv is None or need_pad is False,
    dbias_table when need_table is False.  Allocates the workspace of partials; deterministic, no synchronisation, no fallback."""
    fn = 'swin_window_attention_backward'
    B, C = _swin_check(fn, qkv, pad_qkv, bias_table, H, W, num_heads, ws, shift)
    for name, t in (('out', out), ('dout', dout)):
        if tuple(t.shape) != tuple(qkv.shape[:-1]) + (C,) or t.dtype != qkv.dtype or not t.is_contiguous():
            raise _lib.PreworldHipError('%s: %s must be a contiguous %s tensor of shape %s, got %s %s'
                                        % (fn, name, qkv.dtype, tuple(qkv.shape[:-1]) + (C,), t.dtype, tuple(t.shape)))
    dev = qkv.device
    dqkv = torch.empty_like(qkv)
    dpad = torch.empty(3 * C, device=dev, dtype=_f32) if need_pad and pad_qkv is not None else None
    dtable = torch.empty_like(bias_table) if need_table else None
    nbytes = swin_backward_workspace_bytes(B, H, W, num_heads, ws) if dpad is not None or dtable is not None else 0
    wsp = torch.empty(nbytes // 4, device=dev, dtype=_f32) if nbytes else None
    _lib.call('pw_swin_window_attention_backward', qkv, pad_qkv, bias_table, out, dout, dqkv, dpad, dtable, wsp, nbytes, B, H, W, C,
              num_heads, ws, shift, float(scale), _lib.PW_SWIN['PW_SWIN_BF16' if qkv.dtype == torch.bfloat16 else 'PW_SWIN_F32'],
              _lib.STREAM)
    return dqkv, dpad, dtable


class SwinWindowAttention(torch.autograd.Function):
    """swin_window_attention with swin_window_attention_backward as its gradient: apply(qkv, pad_qkv or None, bias_table, H, W,
    num_heads, ws, shift, scale).  The forward is the same call, so the same bits; saved are qkv, pad_qkv, bias_table and out."""

    @staticmethod
    def forward(ctx, qkv, pad_qkv, bias_table, H, W, num_heads, ws, shift, scale):
        out = swin_window_attention(qkv, pad_qkv, bias_table, H, W, num_heads, ws, shift, scale)
        ctx.save_for_backward(qkv, pad_qkv, bias_table, out)
        ctx.cfg = (H, W, num_heads, ws, shift, scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, pad_qkv, bias_table, out = ctx.saved_tensors
        if not dout.is_contiguous():
            dout = dout.contiguous()
        need = ctx.needs_input_grad
        dqkv, dpad, dtable = swin_window_attention_backward(qkv, pad_qkv, bias_table, out, dout, *ctx.cfg, need_pad=need[1],
                                                            need_table=need[2])
        return (dqkv if need[0] else None, None if dpad is None else dpad.to(pad_qkv.dtype), dtable) + (None,) * 6


# ------------------------------------------------------------------------------ Swin block Linears (include/preworld_hip_swin_linear.h)
SWIN_LINEAR_MIN_DIM, SWIN_LINEAR_MAX_DIM = _lib.PW_SWIN_LINEAR['PW_SWIN_LINEAR_MIN_DIM'], _lib.PW_SWIN_LINEAR['PW_SWIN_LINEAR_MAX_DIM']
_SWIN_LINEAR_DTYPES = {_f32: 'PW_SWIN_F32', torch.bfloat16: 'PW_SWIN_BF16'}


class SwinLinearPacked:
    """the packed operand of one Linear for pw_swin_linear: `buf` (uint8, pw_swin_linear_packed_bytes), K, N and the mode
    (torch.float32: split-fp16 planes; torch.bfloat16: one bf16 plane)"""
    __slots__ = ('buf', 'K', 'N', 'dtype')

    def __init__(self, buf, K, N, dtype):
        self.buf, self.K, self.N, self.dtype = buf, K, N, dtype


def swin_linear_supported(K, N):
    """None if pw_swin_linear takes a Linear with K inputs and N outputs, else the reason it does not"""
    for what, v in (('in_features', K), ('out_features', N)):
        if v % 16 or not SWIN_LINEAR_MIN_DIM <= v <= SWIN_LINEAR_MAX_DIM:
            return '%s %d (supported: multiples of 16 in %d .. %d)' % (what, v, SWIN_LINEAR_MIN_DIM, SWIN_LINEAR_MAX_DIM)
    return None


def swin_linear_pack(weight, bias, ln_weight=None, ln_bias=None, dtype=torch.float32):
    """Pack nn.Linear's weight (N, K) and bias (N) or None, with the LayerNorm in front of it (ln_weight, ln_bias (K), or neither), for
    swin_linear in the mode `dtype`: torch.float32 (split-fp16 planes under per-row powers of two) or torch.bfloat16 (weights rounded
    to bf16).  All inputs are float32 device tensors; gamma and beta are not folded, the packed bias is the Linear's own.  Runs on the
    device without synchronisation."""
    fn = 'swin_linear_pack'
    if dtype not in _SWIN_LINEAR_DTYPES:
        raise _lib.PreworldHipError('%s: dtype must be torch.float32 or torch.bfloat16, got %s' % (fn, dtype))
    if weight.dim() != 2:
        raise _lib.PreworldHipError('%s: weight must be (N, K), got %s' % (fn, tuple(weight.shape)))
    N, K = weight.shape
    why = swin_linear_supported(K, N)
    if why is not None:
        raise _lib.PreworldHipError('%s: not supported: %s' % (fn, why))
    if (ln_weight is None) != (ln_bias is None):
        raise _lib.PreworldHipError('%s: ln_weight and ln_bias come together or not at all' % fn)
    for name, t, shape in (('weight', weight, (N, K)), ('bias', bias, (N,)), ('ln_weight', ln_weight, (K,)), ('ln_bias', ln_bias, (K,))):
        if t is not None and (tuple(t.shape) != shape or t.dtype != _f32 or not t.is_contiguous()):
            raise _lib.PreworldHipError('%s: %s must be a contiguous float32 %s tensor, got %s %s' % (fn, name, shape, t.dtype, tuple(t.shape)))
    mode = _lib.PW_SWIN[_SWIN_LINEAR_DTYPES[dtype]]
    nbytes = _lib.call_size('pw_swin_linear_packed_bytes', K, N, mode)
    if not weight.is_cuda:
        raise _lib.PreworldHipError('%s: weight must be a CUDA(HIP) tensor' % fn)
    buf = torch.empty(nbytes, dtype=torch.uint8, device=weight.device)
    _lib.call('pw_swin_linear_pack', weight.detach(), None if bias is None else bias.detach(), None if ln_weight is None else ln_weight.detach(),
              None if ln_bias is None else ln_bias.detach(), buf, K, N, mode, _lib.STREAM)
    return SwinLinearPacked(buf, K, N, dtype)


def swin_linear(x, packed, *, ln=False, eps=1e-5, act=None, residual=None):
    """out (.., N) = epi(pro(x (.., K)) W^T + b) in one launch (include/preworld_hip_swin_linear.h): ln=True normalises every row over
    K first (the packed gamma / beta, biased variance, `eps`); act='gelu' applies the erf GELU; residual (.., N) float32 is added
    (`residual + y`).  Two launches: the row statistics ((M, 2) floats of workspace), then the GEMM.  packed.dtype float32: x, residual, out float32.  packed.dtype bfloat16 (autocast's data flow): x is float32
    with ln and bfloat16 without, out is float32 with a residual and bfloat16 without.  Forward only; no workspace, no synchronisation."""
    fn = 'swin_linear'
    if not isinstance(packed, SwinLinearPacked):
        raise _lib.PreworldHipError('%s: packed must come from swin_linear_pack' % fn)
    if act not in (None, 'gelu'):
        raise _lib.PreworldHipError("%s: act must be None or 'gelu', got %r" % (fn, act))
    if act is not None and residual is not None:
        raise _lib.PreworldHipError('%s: act and residual exclude each other' % fn)
    K, N, bf = packed.K, packed.N, packed.dtype == torch.bfloat16
    if x.dim() < 1 or x.shape[-1] != K or x.numel() == 0:
        raise _lib.PreworldHipError('%s: x must be (.., %d) and not empty, got %s' % (fn, K, tuple(x.shape)))
    xdt = torch.bfloat16 if bf and not ln else _f32
    if x.dtype != xdt:
        raise _lib.PreworldHipError('%s: x must be %s in this mode (packed %s, ln=%s), got %s' % (fn, xdt, packed.dtype, bool(ln), x.dtype))
    if not x.is_contiguous():
        raise _lib.PreworldHipError('%s: x must be contiguous' % fn)
    lead = tuple(x.shape[:-1])
    if residual is not None and (tuple(residual.shape) != lead + (N,) or residual.dtype != _f32 or not residual.is_contiguous()):
        raise _lib.PreworldHipError('%s: residual must be a contiguous float32 %s tensor, got %s %s'
                                    % (fn, lead + (N,), residual.dtype, tuple(residual.shape)))
    if not x.is_cuda or (residual is not None and not residual.is_cuda) or packed.buf.device != x.device:
        raise _lib.PreworldHipError('%s: x%s must be a CUDA(HIP) tensor on the device of the packed operand' % (fn, '' if residual is None else ', residual'))
    out = torch.empty(lead + (N,), device=x.device, dtype=torch.bfloat16 if bf and residual is None else _f32)
    epi = 'PW_SWIN_LINEAR_EPI_RESIDUAL' if residual is not None else ('PW_SWIN_LINEAR_EPI_GELU' if act == 'gelu' else 'PW_SWIN_LINEAR_EPI_BIAS')
    M, mode = x.numel() // K, _lib.PW_SWIN[_SWIN_LINEAR_DTYPES[packed.dtype]]
    nbytes = _lib.call_size('pw_swin_linear_workspace_bytes', M, int(bool(ln)), mode)          # (M, 2) floats of row statistics, or 0
    wsp = torch.empty(nbytes // 4, device=x.device, dtype=_f32) if nbytes else None
    _lib.call('pw_swin_linear', x, packed.buf, residual, out, wsp, nbytes, M, K, N, int(bool(ln)), float(eps), _lib.PW_SWIN_LINEAR[epi],
              mode, _lib.STREAM)
    return out


# ------------------------------------------------------------------------ their gradient (include/preworld_hip_swin_linear_bwd.h)
SWIN_LINEAR_ROLES = ('ln', 'ln_gelu', 'res')      # Linear(LayerNorm(x)); GELU(Linear(LayerNorm(x))); residual + Linear(x)


def _swin_bwd_f32(fn, **tensors):
    """every named tensor (None is skipped) is a contiguous float32 CUDA(HIP) tensor on one device"""
    dev = None
    for name, t in tensors.items():
        if t is None:
            continue
        if t.dtype != _f32 or not t.is_contiguous():
            raise _lib.PreworldHipError('%s: %s must be a contiguous float32 tensor, got %s %s' % (fn, name, t.dtype, tuple(t.shape)))
        if not t.is_cuda or (dev is not None and t.device != dev):
            raise _lib.PreworldHipError('%s: %s must be a CUDA(HIP) tensor on the device of the other operands' % (fn, name))
        dev = t.device


def _swin_bwd_packed(fn, packed, name='packed'):
    if not isinstance(packed, SwinLinearPacked):
        raise _lib.PreworldHipError('%s: %s must come from swin_linear_pack / swin_linear_pack_transposed' % (fn, name))
    if packed.dtype != _f32:
        raise _lib.PreworldHipError('%s: the gradient is float32 only, %s is packed for %s' % (fn, name, packed.dtype))


def _swin_bwd_rows(fn, t, name, width):
    if t.dim() < 1 or t.shape[-1] != width or t.numel() == 0:
        raise _lib.PreworldHipError('%s: %s must be (.., %d) and not empty, got %s' % (fn, name, width, tuple(t.shape)))
    return t.numel() // width


def swin_linear_pack_transposed(weight):
    """nn.Linear's weight (N, K), float32 on the device -> W^T packed as the weight of swin_linear_backward_data: a SwinLinearPacked
    with N inputs and K outputs (the columns of W as rows, each under its own power of two; zero bias, no LayerNorm)."""
    fn = 'swin_linear_pack_transposed'
    if weight.dim() != 2:
        raise _lib.PreworldHipError('%s: weight must be (N, K), got %s' % (fn, tuple(weight.shape)))
    N, K = weight.shape
    why = swin_linear_supported(K, N)
    if why is not None:
        raise _lib.PreworldHipError('%s: not supported: %s' % (fn, why))
    _swin_bwd_f32(fn, weight=weight)
    nbytes = _lib.call_size('pw_swin_linear_backward_packed_bytes', K, N)
    buf = torch.empty(nbytes, dtype=torch.uint8, device=weight.device)
    _lib.call('pw_swin_linear_backward_pack', weight.detach(), buf, K, N, _lib.STREAM)
    return SwinLinearPacked(buf, N, K, _f32)


def swin_linear_backward_data(g, packed_t):
    """dx (.., K) = g (.., N) W, the forward GEMM with swin_linear_pack_transposed's operand as its weight (two launches)"""
    fn = 'swin_linear_backward_data'
    _swin_bwd_packed(fn, packed_t, 'packed_t')
    N, K = packed_t.K, packed_t.N                       # the transposed operand has N inputs and K outputs
    M = _swin_bwd_rows(fn, g, 'g', N)
    _swin_bwd_f32(fn, g=g)
    if not g.is_cuda or packed_t.buf.device != g.device:
        raise _lib.PreworldHipError('%s: g must be a CUDA(HIP) tensor on the device of the packed operand' % fn)
    dx = torch.empty(tuple(g.shape[:-1]) + (K,), device=g.device, dtype=_f32)
    nbytes = _lib.call_size('pw_swin_linear_backward_rows_workspace_bytes', M)
    wsp = torch.empty(nbytes // 4, device=g.device, dtype=_f32)
    _lib.call('pw_swin_linear_backward_data', g, packed_t.buf, dx, wsp, nbytes, M, K, N, _lib.STREAM)
    return dx


def swin_linear_backward_gelu(x, packed, dh, eps=1e-5, out=None):
    """dz (.., N) = dh o gelu'(LayerNorm(x) W^T + b): the fc1 forward GEMM with the GELU gradient as its epilogue; the pre-activation
    is recomputed and never stored.  out=dh writes dz over dh."""
    fn = 'swin_linear_backward_gelu'
    _swin_bwd_packed(fn, packed)
    K, N = packed.K, packed.N
    M = _swin_bwd_rows(fn, x, 'x', K)
    if tuple(dh.shape) != tuple(x.shape[:-1]) + (N,):
        raise _lib.PreworldHipError('%s: dh must be %s, got %s' % (fn, tuple(x.shape[:-1]) + (N,), tuple(dh.shape)))
    if out is not None and tuple(out.shape) != tuple(dh.shape):
        raise _lib.PreworldHipError('%s: out must have the shape of dh' % fn)
    _swin_bwd_f32(fn, x=x, dh=dh, out=out)
    if not x.is_cuda or packed.buf.device != x.device:
        raise _lib.PreworldHipError('%s: x must be a CUDA(HIP) tensor on the device of the packed operand' % fn)
    dz = torch.empty_like(dh) if out is None else out
    nbytes = _lib.call_size('pw_swin_linear_backward_rows_workspace_bytes', M)
    wsp = torch.empty(nbytes // 4, device=x.device, dtype=_f32)
    _lib.call('pw_swin_linear_backward_gelu', x, packed.buf, dh, dz, wsp, nbytes, M, K, N, float(eps), _lib.STREAM)
    return dz


def swin_linear_backward_weight(g, x, packed=None, *, ln=False, eps=1e-5, need_weight=True, need_bias=True):
    """(dweight (N, K) = g^T pro(x), dbias (N) = column sums of g) for g (.., N), x (.., K); pro = LayerNorm with the gamma / beta of
    `packed` (the forward's operand) when ln, identity otherwise.  A gradient that is not needed is None and its work is skipped."""
    fn = 'swin_linear_backward_weight'
    if not (need_weight or need_bias):
        return None, None
    if ln:
        _swin_bwd_packed(fn, packed)
    if g.dim() < 1 or x.dim() < 1 or tuple(g.shape[:-1]) != tuple(x.shape[:-1]) or g.numel() == 0:
        raise _lib.PreworldHipError('%s: g (.., N) and x (.., K) must share their leading dimensions, got %s and %s' % (fn, tuple(g.shape), tuple(x.shape)))
    K, N = x.shape[-1], g.shape[-1]
    if ln and (packed.K, packed.N) != (K, N):
        raise _lib.PreworldHipError('%s: packed is a (%d -> %d) Linear, g and x say (%d -> %d)' % (fn, packed.K, packed.N, K, N))
    why = swin_linear_supported(K, N)
    if why is not None:
        raise _lib.PreworldHipError('%s: not supported: %s' % (fn, why))
    _swin_bwd_f32(fn, g=g, x=x)
    if ln and packed.buf.device != g.device:
        raise _lib.PreworldHipError('%s: g must be on the device of the packed operand' % fn)
    M = g.numel() // N
    dw = torch.empty(N, K, device=g.device, dtype=_f32) if need_weight else None
    db = torch.empty(N, device=g.device, dtype=_f32) if need_bias else None
    nbytes = _lib.call_size('pw_swin_linear_backward_weight_workspace_bytes', M, K, N, int(bool(ln)))
    wsp = torch.empty(nbytes // 8, device=g.device, dtype=torch.float64)
    _lib.call('pw_swin_linear_backward_weight', g, x, packed.buf if ln else None, dw, db, wsp, nbytes, M, K, N, int(bool(ln)), float(eps),
              _lib.STREAM)
    return dw, db


def swin_layernorm_backward(dxn, x, gamma, dres=None, *, eps=1e-5, need_x=True, need_affine=True, out=None):
    """Gradient of LayerNorm(x) over the last dimension for dxn: (dx = dres + ..., dgamma, dbeta); dres (like x) or None is the
    residual stream's own gradient, folded in.  need_x / need_affine False skip that part (None).  out=dxn writes dx over dxn."""
    fn = 'swin_layernorm_backward'
    if not (need_x or need_affine):
        return None, None, None
    K = x.shape[-1] if x.dim() else 0
    why = swin_linear_supported(K, K) if K else 'empty x'
    if why is not None:
        raise _lib.PreworldHipError('%s: not supported: %s' % (fn, why))
    M = _swin_bwd_rows(fn, x, 'x', K)
    for name, t in (('dxn', dxn), ('dres', dres), ('out', out)):
        if t is not None and tuple(t.shape) != tuple(x.shape):
            raise _lib.PreworldHipError('%s: %s must have the shape of x %s, got %s' % (fn, name, tuple(x.shape), tuple(t.shape)))
    if tuple(gamma.shape) != (K,):
        raise _lib.PreworldHipError('%s: gamma must be (%d,), got %s' % (fn, K, tuple(gamma.shape)))
    _swin_bwd_f32(fn, dxn=dxn, x=x, gamma=gamma, dres=dres, out=out)
    dx = (torch.empty_like(x) if out is None else out) if need_x else None
    dg = torch.empty(K, device=x.device, dtype=_f32) if need_affine else None
    db = torch.empty(K, device=x.device, dtype=_f32) if need_affine else None
    nbytes = _lib.call_size('pw_swin_layernorm_backward_workspace_bytes', M, K)
    wsp = torch.empty(nbytes // 8, device=x.device, dtype=torch.float64)
    _lib.call('pw_swin_layernorm_backward', dxn, x, gamma.detach(), dres if need_x else None, dx, dg, db, wsp, nbytes, M, K, float(eps),
              _lib.STREAM)
    return dx, dg, db


def swin_linear_backward(role, g, x, packed, packed_t=None, *, gamma=None, eps=1e-5, dres=None, need_x=True, need_weight=True,
                         need_bias=True, need_ln=True):
    """The gradient of one role of swin_linear for the cotangent g of its output: (dx, dweight, dbias, dgamma, dbeta).
    'res': dx = g W, dweight = g^T x, dbias = column sums of g (the residual's gradient is g itself).
    'ln' / 'ln_gelu': gy = g or g o gelu'(y); dweight = gy^T LayerNorm(x), dbias; dx = dres + LayerNorm'(gy W), dgamma, dbeta.
    packed is the forward's operand, packed_t swin_linear_pack_transposed's (needed for dx, dgamma, dbeta), gamma the LayerNorm's
    weight.  A gradient whose need_* is False is None and its launches are skipped."""
    fn = 'swin_linear_backward'
    if role not in SWIN_LINEAR_ROLES:
        raise _lib.PreworldHipError('%s: role must be one of %s, got %r' % (fn, SWIN_LINEAR_ROLES, role))
    _swin_bwd_packed(fn, packed)
    ln = role != 'res'
    need_ln = need_ln and ln
    if not (need_x or need_weight or need_bias or need_ln):
        return None, None, None, None, None
    if (need_x or need_ln) and packed_t is None:
        raise _lib.PreworldHipError('%s: dx, dgamma and dbeta need packed_t' % fn)
    if (need_x or need_ln) and ln and gamma is None:
        raise _lib.PreworldHipError('%s: role %r needs gamma' % (fn, role))
    if not g.is_contiguous():
        g = g.contiguous()
    gy = swin_linear_backward_gelu(x, packed, g, eps) if role == 'ln_gelu' else g
    dw, db = swin_linear_backward_weight(gy, x, packed, ln=ln, eps=eps, need_weight=need_weight, need_bias=need_bias)
    dx = dg = dbeta = None
    if need_x or need_ln:
        dxn = swin_linear_backward_data(gy, packed_t)
        if ln:
            dx, dg, dbeta = swin_layernorm_backward(dxn, x, gamma, dres, eps=eps, need_x=need_x, need_affine=need_ln, out=dxn)
        else:
            dx = dxn
    return dx, dw, db, dg, dbeta


class SwinLinear(torch.autograd.Function):
    """swin_linear with swin_linear_backward as its gradient, float32 only: apply(x, weight, bias or None, gamma, beta (None for 'res'),
    residual (None unless 'res'), packed, packed_t, role, eps).  The forward is the same swin_linear call, so the same bits.  Role
    'res' returns out.  Roles 'ln' and 'ln_gelu' return (out, x): the second output is x itself, for the residual addition behind
    the Linear -- its gradient comes back here and is folded into the LayerNorm's gradient, so autograd adds nothing.  Saved are x
    and the (small) parameters; the residual is not needed, the normalised tokens and the pre-GELU tensor are recomputed."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, residual, packed, packed_t, role, eps):
        if role not in SWIN_LINEAR_ROLES:
            raise _lib.PreworldHipError('SwinLinear: role must be one of %s, got %r' % (SWIN_LINEAR_ROLES, role))
        _swin_bwd_packed('SwinLinear', packed)
        ln = role != 'res'
        if ln != (gamma is not None) or ln != (beta is not None) or ln == (residual is not None):
            raise _lib.PreworldHipError("SwinLinear: gamma and beta go with the roles 'ln' and 'ln_gelu', residual with 'res'")
        out = swin_linear(x, packed, ln=ln, eps=eps, act='gelu' if role == 'ln_gelu' else None, residual=residual)
        ctx.save_for_backward(x, gamma)
        ctx.cfg = (role, eps, packed, packed_t)
        ctx.set_materialize_grads(False)               # an unused output's gradient arrives as None, not as a tensor of zeros
        return (out, x) if ln else out

    @staticmethod
    def backward(ctx, g, dres=None):
        x, gamma = ctx.saved_tensors
        role, eps, packed, packed_t = ctx.cfg
        need = ctx.needs_input_grad
        if g is None:                                  # only the pass-through x was used
            return (dres if need[0] else None,) + (None,) * 9
        shape = g.shape
        if dres is not None and not dres.is_contiguous():
            dres = dres.contiguous()
        if not g.is_contiguous():
            g = g.contiguous()
        dx, dw, db, dg, dbeta = swin_linear_backward(role, g, x, packed, packed_t, gamma=gamma, eps=eps, dres=dres, need_x=need[0],
                                                     need_weight=need[1], need_bias=need[2], need_ln=need[3] or need[4])
        if need[0] and dx is None:
            dx = dres
        dresidual = g.view(shape) if role == 'res' and need[5] else None
        return (dx, dw, db, dg if need[3] else None, dbeta if need[4] else None, dresidual, None, None, None, None)


# ------------------------------------------------------------------- FPN_LSS / DepthNet convolutions (include/preworld_hip_conv2d.h)
CONV2D_MIN_DIM, CONV2D_MAX_DIM = _lib.PW_CONV2D['PW_CONV2D_MIN_DIM'], _lib.PW_CONV2D['PW_CONV2D_MAX_DIM']


class Conv2dPacked:
    """the packed operand of one convolution for pw_conv2d: `buf` (uint8, pw_conv2d_packed_bytes: the split-fp16 weight planes and the
    folded BatchNorm / bias), Cin, Cout and ksize"""
    __slots__ = ('buf', 'Cin', 'Cout', 'ksize')

    def __init__(self, buf, Cin, Cout, ksize):
        self.buf, self.Cin, self.Cout, self.ksize = buf, Cin, Cout, ksize


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def conv2d_supported(Cin, Cout, ksize, stride=1, dilation=1, padding=0, groups=1):
    """None if pw_conv2d takes an nn.Conv2d with these arguments (ints or pairs, as nn.Conv2d stores them), else the reason it does
    not: square 1x1 or 3x3, stride 1, groups 1, padding dilation (ksize - 1) / 2, channels multiples of 4 in 4 .. 4096"""
    ks, st, dl, pd = _pair(ksize), _pair(stride), _pair(dilation), _pair(padding)
    if ks not in ((1, 1), (3, 3)):
        return 'kernel_size %s (supported: 1 and 3)' % (ks,)
    if st != (1, 1):
        return 'stride %s (supported: 1)' % (st,)
    if groups != 1:
        return 'groups %d (supported: 1)' % groups
    if dl[0] != dl[1] or dl[0] < 1:
        return 'dilation %s (supported: one value >= 1 for both axes)' % (dl,)
    want = dl[0] * (ks[0] - 1) // 2
    if pd != (want, want):
        return "padding %s (supported: dilation (kernel_size - 1) / 2 = %d, the 'same' size)" % (pd, want)
    for what, v in (('in_channels', Cin), ('out_channels', Cout)):
        if v % 4 or not CONV2D_MIN_DIM <= v <= CONV2D_MAX_DIM:
            return '%s %d (supported: multiples of 4 in %d .. %d)' % (what, v, CONV2D_MIN_DIM, CONV2D_MAX_DIM)
    return None


def conv2d_pack(conv, bn=None):
    """Pack an nn.Conv2d (float32, on the device) and the eval-mode nn.BatchNorm2d behind it, if any, for conv2d: the weight rows as
    split-fp16 planes under per-row powers of two, and scale = gamma / sqrt(var + eps), shift = beta + (bias - mean) scale (without a
    BatchNorm: 1 and the bias), computed on the device from the raw parameters and running statistics.  One launch, no
    synchronisation.  The dilation is an argument of conv2d, not of the packed operand."""
    fn = 'conv2d_pack'
    why = conv2d_supported(conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride, conv.dilation, conv.padding, conv.groups)
    if why is not None:
        raise _lib.PreworldHipError('%s: not supported: %s' % (fn, why))
    if getattr(conv, 'padding_mode', 'zeros') != 'zeros':
        raise _lib.PreworldHipError('%s: not supported: padding_mode %r' % (fn, conv.padding_mode))
    Cin, Cout, ks = conv.in_channels, conv.out_channels, conv.kernel_size[0]
    named = [('weight', conv.weight, (Cout, Cin, ks, ks)), ('bias', conv.bias, (Cout,))]
    if bn is not None:
        if bn.num_features != Cout or bn.running_mean is None or bn.running_var is None:
            raise _lib.PreworldHipError('%s: bn must be a BatchNorm2d over %d channels with running statistics' % (fn, Cout))
        named += [('bn.weight', bn.weight, (Cout,)), ('bn.bias', bn.bias, (Cout,)), ('bn.running_mean', bn.running_mean, (Cout,)),
                  ('bn.running_var', bn.running_var, (Cout,))]
    for name, t, shape in named:
        if t is not None and (tuple(t.shape) != shape or t.dtype != _f32 or not t.is_contiguous()):
            raise _lib.PreworldHipError('%s: %s must be a contiguous float32 %s tensor, got %s %s' % (fn, name, shape, t.dtype, tuple(t.shape)))
    if bn is not None and (bn.weight is None or bn.bias is None):
        raise _lib.PreworldHipError('%s: not supported: a BatchNorm2d without affine parameters' % fn)
    nbytes = _lib.call_size('pw_conv2d_packed_bytes', Cin, Cout, ks)
    if not conv.weight.is_cuda:
        raise _lib.PreworldHipError('%s: weight must be a CUDA(HIP) tensor' % fn)
    buf = torch.empty(nbytes, dtype=torch.uint8, device=conv.weight.device)
    d = lambda t: None if t is None else t.detach()
    stats = (None,) * 4 if bn is None else (d(bn.weight), d(bn.bias), d(bn.running_mean), d(bn.running_var))
    _lib.call('pw_conv2d_pack', d(conv.weight), d(conv.bias), *stats, float(bn.eps) if bn is not None else 0.0, buf, Cin, Cout, ks, _lib.STREAM)
    return Conv2dPacked(buf, Cin, Cout, ks)


def _conv2d_map(fn, name, t, shape):
    """t: a float32 NCHW-shaped tensor of this shape in torch.channels_last storage, i.e. (B, H, W, C) contiguous in memory"""
    if t.dim() != 4 or tuple(t.shape) != tuple(shape) or t.dtype != _f32:
        raise _lib.PreworldHipError('%s: %s must be a float32 %s tensor, got %s %s' % (fn, name, tuple(shape), t.dtype, tuple(t.shape)))
    if not t.permute(0, 2, 3, 1).is_contiguous():
        raise _lib.PreworldHipError('%s: %s must be in torch.channels_last storage ((B, H, W, C) contiguous), got strides %s; '
                                    'convert it with .contiguous(memory_format=torch.channels_last)' % (fn, name, tuple(t.stride())))


def conv2d(x, packed, *, dilation=1, relu=False, residual=None):
    """out = epi(scale . conv(x) + shift) in one implicit GEMM (include/preworld_hip_conv2d.h): the stride-1 'same' convolution that
    conv2d_pack packed, at this dilation, with its BatchNorm and bias folded; relu=True applies ReLU; residual (the output's shape) is
    added before the ReLU (needs relu=True: BasicBlock's tail).  x (B, Cin, H, W), residual and the result (B, Cout, H, W) are float32
    NCHW-shaped tensors in torch.channels_last storage; a tensor in another layout is refused, never copied.  Two launches: the
    partial maxima of |x| (1 KB of workspace), then the GEMM.  Forward only, no synchronisation."""
    fn = 'conv2d'
    if not isinstance(packed, Conv2dPacked):
        raise _lib.PreworldHipError('%s: packed must come from conv2d_pack' % fn)
    if residual is not None and not relu:
        raise _lib.PreworldHipError('%s: residual needs relu=True (out = max(y + residual, 0))' % fn)
    if not isinstance(dilation, int) or dilation < 1:
        raise _lib.PreworldHipError('%s: dilation must be a positive int, got %r' % (fn, dilation))
    if x.dim() != 4 or x.numel() == 0:
        raise _lib.PreworldHipError('%s: x must be (B, %d, H, W) and not empty, got %s' % (fn, packed.Cin, tuple(x.shape)))
    B, _, H, W = x.shape
    _conv2d_map(fn, 'x', x, (B, packed.Cin, H, W))
    if residual is not None:
        _conv2d_map(fn, 'residual', residual, (B, packed.Cout, H, W))
    if not x.is_cuda or (residual is not None and not residual.is_cuda) or packed.buf.device != x.device:
        raise _lib.PreworldHipError('%s: x%s must be a CUDA(HIP) tensor on the device of the packed operand' % (fn, '' if residual is None else ', residual'))
    out = torch.empty((B, H, W, packed.Cout), device=x.device, dtype=_f32).permute(0, 3, 1, 2)
    epi = 'PW_CONV2D_EPI_RESIDUAL_RELU' if residual is not None else ('PW_CONV2D_EPI_RELU' if relu else 'PW_CONV2D_EPI_NONE')
    nbytes = _lib.call_size('pw_conv2d_workspace_bytes', B, H, W)
    wsp = torch.empty(nbytes // 4, device=x.device, dtype=_f32)
    _lib.call('pw_conv2d', _lib.strided(x), packed.buf, None if residual is None else _lib.strided(residual), _lib.strided(out), wsp, nbytes,
              B, H, W, packed.Cin, packed.Cout, packed.ksize, dilation, _lib.PW_CONV2D[epi], _lib.STREAM)
    return out
