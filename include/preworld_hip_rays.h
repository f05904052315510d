/*
 * preworld_hip_rays.h -- the ray-supervision part of the C ABI of libpreworld_hip.so; included by preworld_hip.h, whose
 * conventions hold: device pointers unless the name ends in _host, `stream` last, 0 or a negative PW_E* code with a thread-local message.
 * Kept in a file of its own so that the entry-point and pointer-parameter census of preworld_hip.h
 * (tests/test_marshal_cpu.py) stays what it was; preworld_amd/_lib.py parses all the part files the same way and
 * tests/test_ray_labels_cpu.py holds this one to the same rules (every declaration parses, every pointer has a converter).
 */
#ifndef PREWORLD_HIP_RAYS_H_
#define PREWORLD_HIP_RAYS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Pre-train ray supervision on the GPU (pw_ray_labels.hip): the T lidar sweeps of a sample with their lidarseg bytes and the
 * staged uint8 frames in, the (R, 16) ray table of ray.py and its weighted-ray-sampling weights out, for all V = T N views
 * (view v = t N + camera) at once.  Nothing here synchronises the host; everything is written by kernels, so a call can be
 * captured.  Rows, counts and weights are the same bits on every run.
 *
 * Stage A, tools/gen_data/gen_depth_gt.py:17-76 and gen_seg_gt_from_lidarseg.py:17-81 (map_pointcloud_to_image):
 *   points       float[T][Pmax][point_stride], x y z first; sweep t owns its first n_pts[t] rows (n_pts int32[T] IN DEVICE
 *                MEMORY, clamped to [0, Pmax]; NULL: all Pmax), so a captured graph replays on sweeps of other lengths
 *   point_labels uint8[T][Pmax], the lidarseg byte of each point;  label_lut uint8[256], byte -> class
 *   view_pose    double[V][PW_RAY_POSE_DOUBLES]: R1[9] t1[3] (lidar->ego), R2[9] t2[3] (ego->global), t3[3] R3[9]
 *                (global->camera ego: -t and R^T, prepared on the host), t4[3] R4[9] (camera ego->camera, likewise), K[9]
 *   The cloud is a float32 array: p = float32(R p) with R p = (r0 x + r1 y) + r2 z in float64, p = p + float32(t) in float32,
 *   in the order above.  depth = z;  (u, v) = K p / (K p)_2 in float64;  kept iff depth > 0, 1 < u < W - 1, 1 < v < H - 1
 *   (float64 comparisons).  A kept point's row: views in order, then sweep order.
 * pw_ray_sweep_count: projects, records per pixel its OWNER -- the largest kept point index that truncates to it, i.e. the
 *   point whose label a dense map written by fancy assignment would hold (nuscenes_dataset_occ.py:58-66) -- and scans.
 *   slots      int64[n_slots] scratch, n_slots a power of two > T N Pmax and <= 2^31 (open-addressed {view, pixel | point}
 *              words); NULL with n_slots 0: no owners are recorded (enough for pw_ray_sweep_lists)
 *   block_base int32[V ceil(Pmax / 256)]: first row of each 256-point block;  view_off int32[V + 1]: first row of each view,
 *              view_off[V] = R, the number of kept points (the device scalar n_rows)
 * pw_ray_sweep_lists: float[capacity][3] depth_list (u, v, depth) and seg_list (u, v, class), float32, what the two gen tools
 *   write into their .bin files; rows >= capacity are dropped.  Needs block_base of pw_ray_sweep_count on the same inputs.
 * pw_ray_sweep_table (nuscenes_dataset_occ.py:48-66, 197-270 load_depth / load_seg_label / get_rays; ray.py:34-56): row =
 *   {x, y, depth, seg, rays_o[3], rays_d[3], viewdirs[3], rgb[3]} with (x, y) = (u, v) truncated (int16), seg the class of
 *   the pixel's owner, rays_* pw_pts2ray's arithmetic on c2w float[V][16] / K float[V][9], rgb[ch] = (u8 / 255.0f - mean[ch])
 *   / std[ch] at (x, y) of frame view_frame[v] (int32[V] in device memory; NULL: frame v).
 *   frames     uint8, element (f, y, x, ch) at byte f s_f + y s_y + x s_x + ch s_c; n_frames of H x W x 3
 *   mean_std_host  float[6] IN HOST MEMORY: mean[3], std[3]
 *   rays       float[capacity][16]; rows >= capacity are dropped;  counts int64[n_cls] += classes of the rows written
 *   Needs slots and block_base of pw_ray_sweep_count on the same inputs.
 * pw_ray_lists_table: the same table from the CONTENTS of the two .bin files of every view, back to back: depth_list and
 *   seg_list float[n][3], view_off int32[V + 1] in device memory with view_off[0] = 0, view_off[V] = n.  The owner of a pixel
 *   is the last row of seg_list on it; a depth_list row on a pixel no seg_list row touches gets class 0 (the zero-filled
 *   map); a row outside the image gets class 0 and colour 0.  slots: n_slots a power of two > n.
 * pw_ray_table_weights (ray.py:93-112) over the whole table: weight = bw[class] * (frame_ids[view] == 0 ? 1 : (class in
 *   dynamic_class ? weight_dyn : weight_adj)), the view of a row from view_off.  bw = balance_weight float[n_cls], or when
 *   that is NULL the batch statistics float32(exp(double(0.005f * (max(counts) / counts[c] - 1)))), quotient and product in
 *   float32.  Rows >= view_off[V] get weight 0 and are zeroed.  frame_ids int32[V], dynamic_class int32[n_dyn], device. */
#define PW_RAY_POSE_DOUBLES 57
int pw_ray_sweep_count(const float* points, int point_stride, const int32_t* n_pts, int T, int N, int Pmax,
                       const double* view_pose, int H, int W, int64_t* slots, int64_t n_slots, int32_t* block_base,
                       int32_t* view_off, void* stream);
int pw_ray_sweep_lists(const float* points, int point_stride, const uint8_t* point_labels, const int32_t* n_pts, int T,
                       int N, int Pmax, const uint8_t* label_lut, const double* view_pose, int H, int W,
                       const int32_t* block_base, int64_t capacity, float* depth_list, float* seg_list, void* stream);
int pw_ray_sweep_table(const float* points, int point_stride, const uint8_t* point_labels, const int32_t* n_pts, int T,
                       int N, int Pmax, const uint8_t* label_lut, const double* view_pose, int H, int W,
                       const int64_t* slots, int64_t n_slots, const int32_t* block_base, const uint8_t* frames,
                       int64_t s_f, int64_t s_y, int64_t s_x, int64_t s_c, int n_frames, const int32_t* view_frame,
                       const float* mean_std_host, const float* c2w, const float* K, int64_t capacity, float* rays,
                       int n_cls, int64_t* counts, void* stream);
int pw_ray_lists_table(const float* depth_list, const float* seg_list, int64_t n, const int32_t* view_off, int V, int H,
                       int W, int64_t* slots, int64_t n_slots, const uint8_t* frames, int64_t s_f, int64_t s_y,
                       int64_t s_x, int64_t s_c, int n_frames, const int32_t* view_frame, const float* mean_std_host,
                       const float* c2w, const float* K, int64_t capacity, float* rays, int n_cls, int64_t* counts,
                       void* stream);
int pw_ray_table_weights(float* rays, int64_t capacity, const int32_t* view_off, int V, const int32_t* frame_ids,
                         const float* balance_weight, const int64_t* counts, int n_cls, const int32_t* dynamic_class,
                         int n_dyn, float weight_adj, float weight_dyn, float* weights, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PREWORLD_HIP_RAYS_H_ */
