"""GPU drop-in for mmdet3d/datasets/ray.py:34-119: the (R,16) ray table and the
weighted-ray-sampling weights of the pre-train dataloader.  Same call signature as the reference's
`generate_rays`; inputs are device tensors.  The draw itself (WeightedRandomSampler without
replacement, ray.py:116-118) is torch.multinomial on the device -- same distribution, not the same
random stream.

generate_rays_from_sweeps / generate_rays_from_labels build the same table for all views of a sample at once, from the raw
sweeps + lidarseg bytes + uint8 frames or from the contents of the reference's gen_depth_gt / gen_seg_gt_from_lidarseg files
(csrc/pw_ray_labels.hip; INTEGRATION.md, "Ray supervision from the sweep")."""
import torch

from . import ops


def pts2ray(coor, label_depth, label_seg, label_img, c2w, cam_intrinsic):
    return ops.pts2ray(coor, label_depth, label_seg, label_img, c2w, cam_intrinsic)


def generate_rays(coors, label_depths, label_segs, label_imgs, c2w, intrins, max_ray_nums=0, time_ids=None,
                  dynamic_class=None, balance_weight=None, weight_adj=0.3, weight_dyn=0.0, use_wrs=True,
                  return_weights=False, generator=None):
    rays, ids = [], []
    for time_id in time_ids:                       # frames
        for i in time_ids[time_id]:                # cameras of one frame
            rays.append(ops.pts2ray(coors[i], label_depths[i], label_segs[i], label_imgs[i], c2w[i], intrins[i]))
            ids.append(time_id)
    if not use_wrs:
        return torch.cat(rays, dim=0)
    dev = rays[0].device
    if balance_weight is None:                     # batch statistics (ray.py:93-97)
        counts = torch.zeros(17, device=dev, dtype=torch.int64)
        for r in rays:
            ops.class_count(r, 17, counts)
        class_nums = counts.float()
        balance_weight = torch.exp(0.005 * (class_nums.max() / class_nums - 1))
    if dynamic_class is None:
        dynamic_class = torch.zeros(0, dtype=torch.int32)
    weights = [ops.wrs_weights(r, ids[k], balance_weight.to(dev), dynamic_class, weight_adj, weight_dyn)
               for k, r in enumerate(rays)]
    rays = torch.cat(rays, dim=0)
    weights = torch.cat(weights, dim=0)
    if max_ray_nums != 0 and rays.shape[0] > max_ray_nums:
        sel = torch.multinomial(weights, max_ray_nums, replacement=False, generator=generator)
        rays = rays[sel]
        if return_weights:
            return rays, weights, sel
    return (rays, weights, None) if return_weights else rays


# ------------------------------------------------------------------------------ the table straight from the sweeps / the lists
def _frame_ids(time_ids, V):
    """time_ids as get_rays builds it ({frame id: [view indices]}, nuscenes_dataset_occ.py:209-246) -> frame id per view; the
    table's rows are in view order, so the views must be numbered in the order the dict walks them.  A device int32 (V) tensor
    of frame ids passes through (needed under graph capture: nothing is copied from the host then)."""
    if isinstance(time_ids, torch.Tensor):
        return time_ids
    ids = []
    for time_id in time_ids:
        for i in time_ids[time_id]:
            if i != len(ids):
                raise ValueError('time_ids must number the views 0 .. V-1 in the order it lists them (get_rays does)')
            ids.append(int(time_id))
    if len(ids) != V:
        raise ValueError('time_ids lists %d views, the poses %d' % (len(ids), V))
    return ids


def _finish(table, view_off, counts, frame_ids, max_ray_nums, dynamic_class, balance_weight, weight_adj, weight_dyn, capacity,
            generator, return_weights):
    weights = ops.ray_table_weights(table, view_off, frame_ids, dynamic_class, balance_weight, counts, weight_adj, weight_dyn)
    if capacity is not None:
        return table, weights, view_off[-1]
    if max_ray_nums != 0 and table.shape[0] > max_ray_nums:
        sel = torch.multinomial(weights, max_ray_nums, replacement=False, generator=generator)
        return (table[sel], weights, sel) if return_weights else table[sel]
    return (table, weights, None) if return_weights else table


def generate_rays_from_sweeps(points, point_labels, frames_u8, view_pose, c2w, intrins, max_ray_nums=0, time_ids=None,
                              dynamic_class=None, balance_weight=None, weight_adj=0.3, weight_dyn=0.0, label_lut=None,
                              capacity=None, generator=None, view_frame=None, n_pts=None, return_weights=False):
    """get_rays of the pre-train dataloader (nuscenes_dataset_occ.py:197-270) without the two offline gen tools: the T sweeps
    (`points`, a list of (P_t, >= 3) tensors or (T, Pmax, C) with n_pts, and their lidarseg bytes `point_labels`; or a prepared
    ops.RaySweeps) are projected into the V = T N views with `view_pose` (transforms.compose_view_poses), labelled through
    `label_lut` (256 entries, lidarseg byte -> class; None: the bytes are classes), coloured from `frames_u8` (F,H,W,3) uint8
    and turned into rows with c2w = sensor2keyegos (transforms.compose_sensor2keyegos) and `intrins`.

    capacity=None: the reference's result -- all R rows if R <= max_ray_nums (or max_ray_nums == 0), else a torch.multinomial
    draw of max_ray_nums rows without replacement (same distribution, not the reference's random stream); the row count is read
    back, one host synchronisation.  return_weights=True -> (rays, weights, sel).
    capacity=C: no synchronisation, capturable (hand in a prepared RaySweeps and device tensors): (table (C,16), weights (C),
    n_rows on the device); rows beyond C are dropped, rows >= n_rows have weight 0, so a caller who knows n_rows >=
    max_ray_nums draws with torch.multinomial(weights, max_ray_nums)."""
    sw = points if isinstance(points, ops.RaySweeps) else ops.RaySweeps(points, point_labels, view_pose, label_lut, n_pts)
    frame_ids = _frame_ids(time_ids, sw.V)
    table, view_off, counts = ops.ray_table(c2w, intrins, frames_u8, sweeps=sw, view_frame=view_frame, capacity=capacity)
    return _finish(table, view_off, counts, frame_ids, max_ray_nums, dynamic_class, balance_weight, weight_adj, weight_dyn,
                   capacity, generator, return_weights)


def generate_rays_from_labels(depth_list, seg_list, view_off, frames_u8, c2w, intrins, max_ray_nums=0, time_ids=None,
                              dynamic_class=None, balance_weight=None, weight_adj=0.3, weight_dyn=0.0, capacity=None,
                              generator=None, view_frame=None, return_weights=False):
    """The same from the contents of the gen tools' files: depth_list (n,3) rows (u, v, depth) and seg_list (n,3) rows
    (u, v, class) of all views back to back, view_off (V+1) the first row of each view.  Results as generate_rays_from_sweeps;
    nothing is read back in either mode (n is known)."""
    V = (view_off.numel() if isinstance(view_off, torch.Tensor) else len(view_off)) - 1
    frame_ids = _frame_ids(time_ids, V)
    table, view_off, counts = ops.ray_table(c2w, intrins, frames_u8, lists=(depth_list, seg_list, view_off), view_frame=view_frame,
                                            capacity=capacity)
    return _finish(table, view_off, counts, frame_ids, max_ray_nums, dynamic_class, balance_weight, weight_adj, weight_dyn,
                   capacity, generator, return_weights)
