/*
 * pvcnn_hip.h -- C ABI of libpvcnn_hip.so, the MI355X (gfx950) native backend of the PVConv
 * hot path.  It is what the reference's Python seam `modules/functional/backend.py:_backend`
 * (12 pybind functions, modules/functional/src/bindings.cpp:10-37) binds to on AMD hardware.
 *
 * Conventions (all entry points)
 *   - plain pointers and sizes only; no torch / ATen types cross this boundary;
 *   - every pointer is a DEVICE pointer on the current HIP device; tensors are dense,
 *     row-major, channel-major: features (B, C, N), coords (B, 3, N), voxel grids (B, C, R^3);
 *     data fp32, indices int32 (same as the reference, utils.hpp:7-18);
 *   - the library NEVER allocates or frees device memory and never synchronises the host:
 *     outputs and scratch are caller-owned, work is enqueued on `stream` (a hipStream_t,
 *     e.g. torch.cuda.current_stream().cuda_stream; NULL = the null stream);
 *   - every output buffer is FULLY written by the call -- the caller does not pre-zero
 *     anything (the reference's host code zero-fills with torch::zeros first);
 *   - return value: 0 on success; PVCNN_ERR_INVALID_ARGUMENT for a rejected argument;
 *     otherwise the (positive) hipError_t of the failed launch.  The reference instead
 *     prints and exit(-1)s (cuda_utils.cuh:28-37).  pvcnn_last_error_string() describes the
 *     calling thread's most recent failure;
 *   - re-entrant: no global mutable state except the thread-local error string.
 *
 * Numerics contract (what tests/ check against oracle/)
 *   bit-exact : EVERY output -- ind, cnt, inds, ball_query, FPS and 3-NN indices; devoxelize
 *               fwd outs/wgts, 3-NN weights/outputs, grouping/gather fwd; and also all
 *               scatter-adds (avg_voxelize fwd, devoxelize bwd, grouping/gather bwd, 3-NN bwd):
 *               they are evaluated without float atomics, in the serial point-index order
 *               the oracle defines, so results are run-to-run deterministic as well
 *               (the reference's atomicAdd order is undefined);
 *   <= 1e-5   : only the atomic fallback taken beyond 2^20 scatter targets per cloud (R > 101 grids).
 *   Scatter-type calls take caller-owned scratch: `workspace` must hold at least the matching
 *   *_workspace_bytes(...) bytes and be 16-byte aligned.
 */
#ifndef PVCNN_HIP_H_
#define PVCNN_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden; only these entry points are exported. */
#if defined(__GNUC__)
#define PVCNN_API __attribute__((visibility("default")))
#else
#define PVCNN_API
#endif

#define PVCNN_ABI_VERSION 17
#define PVCNN_OK 0
#define PVCNN_ERR_INVALID_ARGUMENT (-1)

/* ABI version of the loaded library (== PVCNN_ABI_VERSION it was built with). */
PVCNN_API int pvcnn_version(void);
/* Description of the calling thread's last error ("" if none).  Never NULL. */
PVCNN_API const char *pvcnn_last_error_string(void);

/* ---- coordinate pre-pass of modules/voxelization.py:16-25 (a dozen torch kernels in the reference) ------------
 * coords (B,3,N) float -> norm_coords (B,3,N) float in [0,R-1] (centred, optionally normalised to the unit cube,
 * scaled by R, clamped) and vox_coords (B,3,N) int32 = round-half-even(norm_coords).  normalize != 0:
 * c / (max ||c||_2 * 2 + eps) + 0.5, else (c + 1) / 2.  A degenerate cloud with eps = 0 gives NaN like the reference. */
PVCNN_API int pvcnn_voxel_coords(const float *coords, int B, int N, int R, int normalize, float eps, float *norm_coords,
                       int32_t *vox_coords, void *stream);

/* The same pre-pass with the two reductions left to the caller (DEFAULT path of pvcnn_amd.modules.Voxelization): the
 * reference computes mean = coords.mean(2) and radius = (coords - mean).norm(dim=1).max(dim=2) with torch ops; calling
 * those same ops on the same device and handing the results to this fused elementwise tail (centre, / (radius*2+eps),
 * + 0.5, * R, clamp, round-half-even -- each step separately rounded like the reference's separate kernels) gives
 * norm_coords / vox_coords BIT-IDENTICAL to modules/voxelization.py:16-25, whatever reduction tree the library uses.
 * coords: rows of a cloud contiguous, clouds coords_batch_stride floats apart (>= 3N: a channel slice of the input);
 * mean (B,3); radius (B) or NULL for normalize=False [(c + 1) / 2]. pvcnn_voxel_coords above (one launch, fp64 mean,
 * exact max: the correctly rounded statistics) remains as an opt-in; it may differ from torch in the last bit of the mean. */
PVCNN_API int pvcnn_voxel_coords_tail(const float *coords, long coords_batch_stride, const float *mean, const float *radius,
                            int B, int N, int R, float eps, float *norm_coords, int32_t *vox_coords, void *stream);

/* ---- avg_voxelize -------------------------------------------------------------------------
 * replaces avg_voxelize_forward  (voxelization/vox.cpp:17-43, kernels vox.cu:18-72)
 *          avg_voxelize_backward (voxelization/vox.cpp:54-76, kernel  vox.cu:86-110)
 * fwd: feat (B,C,N) f32, coords (B,3,N) i32 voxel coordinates in [0,R)
 *      -> out (B,C,R^3) f32, ind (B,N) i32, cnt (B,R^3) i32.
 *      out[b,c,v] = sum_{i: ind[b,i]=v} feat[b,c,i] * (1/cnt[b,v]), summed in ascending i
 *      (deterministic; no float atomics).  `workspace` is scratch of at least
 *      pvcnn_avg_voxelize_fwd_workspace_bytes(B,C,N,R) bytes, 16-byte aligned.
 *      Out-of-range coords are clamped into the grid (the reference has no bounds check).
 * bwd: grad_y (B,C,S) f32, ind (B,N), cnt (B,S) -> grad_x (B,C,N) f32.
 */
PVCNN_API size_t pvcnn_avg_voxelize_fwd_workspace_bytes(int B, int C, int N, int R);
PVCNN_API int pvcnn_avg_voxelize_fwd(const float *feat, const int32_t *coords, int B, int C, int N, int R,
                           float *out, int32_t *ind, int32_t *cnt, void *workspace,
                           size_t workspace_bytes, void *stream);
PVCNN_API int pvcnn_avg_voxelize_bwd(const float *grad_y, const int32_t *ind, const int32_t *cnt, int B,
                           int C, int N, int S, float *grad_x, void *stream);

/* ---- trilinear_devoxelize -----------------------------------------------------------------
 * replaces trilinear_devoxelize_forward  (interpolate/trilinear_devox.cpp:18-55, .cu:21-105)
 *          trilinear_devoxelize_backward (interpolate/trilinear_devox.cpp:67-91, .cu:119-162)
 * fwd: coords (B,3,N) f32 in [0,R-1], feat (B,C,R^3) -> outs (B,C,N); when is_training != 0
 *      also inds (B,8,N) i32 and wgts (B,8,N) f32 (corner order 000..111, z fastest);
 *      when is_training == 0 inds/wgts are not touched and may be NULL.
 * bwd: grad_y (B,C,N), inds, wgts -> grad_x (B,C,R^3) (every element written).
 */
PVCNN_API int pvcnn_trilinear_devox_fwd(const float *coords, const float *feat, int B, int C, int N, int R,
                              int is_training, int32_t *inds, float *wgts, float *outs,
                              void *stream);
PVCNN_API size_t pvcnn_trilinear_devox_bwd_workspace_bytes(int B, int C, int N, int R);
PVCNN_API int pvcnn_trilinear_devox_bwd(const float *grad_y, const int32_t *inds, const float *wgts, int B,
                              int C, int N, int R, float *grad_x, void *workspace,
                              size_t workspace_bytes, void *stream);

/* ---- scatter plans: the counting sort of a scatter depends on its entries only -----------------------------------
 * Both scatters of the voxel branch are "plan, then apply".  The plan -- entries (source index, weight) grouped by
 * target voxel in the reference's serial order, their prefix offsets, and a count-sorted lane assignment -- depends on
 * (voxel coordinates, R) for avg_voxelize and on (inds, wgts) = (point coordinates, R) for the devoxelize backward, NOT
 * on the features, their channel count or the layer: every PVConv that shares coords and R (PVCNN: three at R = 16)
 * applies one plan, forward and backward.  pvcnn_avg_voxelize_fwd / pvcnn_trilinear_devox_bwd above are plan + apply in
 * one call.  *_plan_bytes returns 0 when the grid is too large for a plan (R > 101): use the one-shot calls then.
 * plan: caller-owned, 16-byte aligned, *_plan_bytes(...) bytes, opaque; scratch: *_plan_scratch_bytes(...) bytes, free
 * to reuse once the plan call is enqueued on the same stream.  ind / cnt are avg_voxelize_forward's outputs.
 */
PVCNN_API size_t pvcnn_avg_voxelize_plan_bytes(int B, int N, int R);
PVCNN_API size_t pvcnn_avg_voxelize_plan_scratch_bytes(int B, int N, int R);
PVCNN_API int pvcnn_avg_voxelize_plan(const int32_t *coords, int B, int N, int R, int32_t *ind, int32_t *cnt, void *plan,
                            size_t plan_bytes, void *scratch, size_t scratch_bytes, void *stream);
/* (ABI v11) Both plans of one PVConv geometry in ONE chain of three launches: vox_plan as pvcnn_avg_voxelize_plan(vox_coords)
 * writes it (with ind / cnt), devox_bwd_plan as pvcnn_trilinear_devox_bwd_plan writes it from the (inds, wgts) that
 * pvcnn_trilinear_devox_fwd(norm_coords) emits -- the corner entries are derived from norm_coords (B,3,N) with the same expressions
 * (trilinear_devox.cu:41-75), so the plan exists before any layer has devoxelized.  The two sorts run side by side in each launch
 * (each alone is a latency chain that leaves most of the chip idle).  Plan sizes: the *_plan_bytes queries above;
 * scratch: pvcnn_pvconv_plans_scratch_bytes.  N > 0. */
PVCNN_API size_t pvcnn_pvconv_plans_scratch_bytes(int B, int N, int R);
PVCNN_API int pvcnn_pvconv_plans(const int32_t *vox_coords, const float *norm_coords, int B, int N, int R, int32_t *ind, int32_t *cnt,
                                 void *vox_plan, size_t vox_plan_bytes, void *devox_bwd_plan, size_t devox_bwd_plan_bytes,
                                 void *scratch, size_t scratch_bytes, void *stream);
PVCNN_API int pvcnn_avg_voxelize_apply(const float *feat, const void *plan, size_t plan_bytes, int B, int C, int N, int R,
                             float *out, void *stream);
PVCNN_API size_t pvcnn_trilinear_devox_bwd_plan_bytes(int B, int N, int R);
PVCNN_API size_t pvcnn_trilinear_devox_bwd_plan_scratch_bytes(int B, int N, int R);
PVCNN_API int pvcnn_trilinear_devox_bwd_plan(const int32_t *inds, const float *wgts, int B, int N, int R, void *plan,
                                   size_t plan_bytes, void *scratch, size_t scratch_bytes, void *stream);
PVCNN_API int pvcnn_trilinear_devox_bwd_apply(const float *grad_y, long grad_y_batch_stride, const void *plan, size_t plan_bytes,
                                    int B, int C, int N, int R, float *grad_x, void *stream);

/* ---- ball_query ---------------------------------------------------------------------------
 * replaces ball_query_forward (ball_query/ball_query.cpp:6-30, kernel ball_query.cu:19-50)
 * centers (B,3,M), points (B,3,N) -> out (B,M,U) i32: the first U points (ascending index)
 * with d^2 < radius^2 (radius^2 evaluated in float); short rows padded with the first hit,
 * rows without a hit are all 0.
 */
PVCNN_API int pvcnn_ball_query(const float *centers, const float *points, int B, int N, int M, float radius,
                     int U, int32_t *out, void *stream);

/* ---- grouping / gather --------------------------------------------------------------------
 * replaces grouping_forward/backward        (grouping/grouping.cpp:6-44, grouping.cu:18-77)
 *          gather_features_forward/backward (sampling/sampling.cpp:6-41, sampling.cu:17-66)
 * grouping fwd: features (B,C,N), indices (B,M,U) -> out (B,C,M,U)
 * grouping bwd: grad_y (B,C,M,U), indices -> grad_x (B,C,N)
 * gather   fwd: features (B,C,N), indices (B,M)   -> out (B,C,M)
 * gather   bwd: grad_y (B,C,M), indices -> grad_x (B,C,N)
 * Indices must lie in [0,N).
 */
PVCNN_API int pvcnn_grouping_fwd(const float *features, const int32_t *indices, int B, int C, int N, int M,
                       int U, float *out, void *stream);
PVCNN_API size_t pvcnn_grouping_bwd_workspace_bytes(int B, int C, int N, int M, int U);
PVCNN_API int pvcnn_grouping_bwd(const float *grad_y, const int32_t *indices, int B, int C, int N, int M,
                       int U, float *grad_x, void *workspace, size_t workspace_bytes, void *stream);
PVCNN_API int pvcnn_gather_fwd(const float *features, const int32_t *indices, int B, int C, int N, int M,
                     float *out, void *stream);
PVCNN_API size_t pvcnn_gather_bwd_workspace_bytes(int B, int C, int N, int M);
PVCNN_API int pvcnn_gather_bwd(const float *grad_y, const int32_t *indices, int B, int C, int N, int M,
                     float *grad_x, void *workspace, size_t workspace_bytes, void *stream);

/* ---- furthest point sampling --------------------------------------------------------------
 * replaces furthest_point_sampling_forward (sampling/sampling.cpp:43-58, sampling.cu:86-167)
 * coords (B,3,N) -> indices (B,M) i32, starting from point 0, with the reference's tie rule
 * (lowest (k mod 512, k) among equidistant candidates).  `distances` is optional scratch
 * (B,N) f32: NULL is allowed for N <= PVCNN_FPS_MAX_RESIDENT_POINTS; when given it receives
 * the final point-to-set distances (the reference's caller-visible scratch).
 */
#define PVCNN_FPS_MAX_RESIDENT_POINTS 16384
PVCNN_API int pvcnn_fps(const float *coords, int B, int N, int M, float *distances, int32_t *indices,
              void *stream);

/* ---- Device draws (csrc/philox.h; tests/draws_truth.py) ---------------------------------------------------------------------
 * The one random stream of the entry points that draw on the device.
 * `seed`: two int64 words in DEVICE memory (no host round trip; a replayed graph reads fresh words).  The stream is Philox4x32-10
 * with key (lo32 seed[0], hi32 seed[0]) and counter (a, b, lo32 seed[1], use): a, b are the use's own -- the point or list position
 * (0 for a per-sample draw) and the sample -- and `use` names who draws, so that one pair of words may key every stage of a loader:
 *    0  the picks of pvcnn_batch_*, pvcnn_frame_batch, pvcnn_frame_store_batch; pvcnn_mask_select's selection keys
 *    1  pvcnn_batch_shapenet's jitter; pvcnn_mask_select's shuffle keys
 *    2  the flip and shift of pvcnn_batch_frustum and pvcnn_frame_store_batch
 *    3  pvcnn_frame_store_batch's box perturbation
 *   16 .. 19  pvcnn_augment_draw's per-cloud draws     20  pvcnn_augment_apply's jitter     21  pvcnn_augment_apply's keep
 * A pick of [0, n) is mulhi(word x, n); n distinct of k in random order are the low halves of the n smallest words x << 32 | a;
 * a flip is bit 31 of word x; uniforms are word * 2^-32 in [0, 1) or (word + 0.5) * 2^-32 in (0, 1) in fp64, (word >> 8) * 2^-24 in
 * fp32; normals are Box-Muller pairs of two words in the precision stated.  pvcnn_room_fill keys the same generator with seed[0] but
 * lays out its own counter (a, b, lo32 seed[1] ^ use, hi32 seed[1]).
 */

/* ---- foreground selection of logits_mask (Frustum-PVCNN) --------------------------------------------------------
 * replaces the per-cloud Python loop of modules/functional/sampling.py:69-82 (nonzero() sync + numpy draws per cloud).
 * mask (B,N) bytes (non-zero = foreground) -> selected (B,M) int32 point ids:
 *   k = foreground count; k >= M: M distinct foreground points in random order; 0 < k < M: every one M/k times plus M%k
 *   distinct extra ones, shuffled; k == 0: all 0 -- the reference's three cases.
 * Randomness: `choices` (B,M) int32 = positions into the ascending foreground list, supplied by the caller (PARITY MODE:
 * with numpy's own draws the result is bit-identical to the reference), or, when choices is NULL, the stream of `seed`
 * ("Device draws" above) -- no host round trip.  count (B) optional: receives k.
 * N, M <= 8192.
 */
PVCNN_API int pvcnn_mask_select(const uint8_t *mask, int B, int N, int M, const int32_t *choices, const int64_t *seed,
                      int32_t *selected, int32_t *count, void *stream);

/* ---- batches assembled on the device (ABI v15; pvcnn_amd/data.py) --------------------------------------------------
 * replace one iteration of the reference's DataLoader (datasets/s3dis.py:81-94, shapenet.py:62-81, kitti/frustum.py:95-147 +
 * default_collate) for a split held in device memory.  One launch, never allocates, every pointer is device memory.
 * The store: `rows` (R, C) fp32, ROW-major and packed (item i owns rows offsets[i] .. offsets[i+1]; C = 9 / 6 / 4), `labels` (R) of
 * label_bytes each (1: uint8, 2: int16, 4: int32, 8: int64), `offsets` (W + 1) int64.  Row addressing is 64-bit.
 * Sample b of the batch is item order[cursor[0] + b] (`order` (order_len) int64, `cursor` one int64 word or NULL = 0), read on the
 * device: a captured launch walks an epoch when the caller adds B to the cursor after it.  Positions, items and parity choices out of
 * range are clamped (no out-of-bounds access); an empty item yields zeros.
 * Randomness as pvcnn_mask_select: `choices` (B, N) int32 rows within the item (PARITY MODE, with the other draws of the dataset
 * kind; bit-identical to the reference for numpy's draws), or, when choices is NULL, the stream of `seed` ("Device draws").
 * Outputs are what default_collate makes of the reference's items: features (B, C_out, N) fp32, targets (B, N) int64, ...
 */
/* LDS the S3DIS launch takes in device mode for N samples from items of at most max_n rows (0: no selection without replacement). */
PVCNN_API size_t pvcnn_batch_lds_bytes(int N, int max_n);
/* S3DIS: C = 9; C_out = 9, or 6 (without the normalised coordinates).  np.random.choice(n, N, replace = n < N): in device mode items
 * with n >= N are sampled WITHOUT replacement by a sort in LDS; max_n = the largest item of the store, refused beyond 8192 when it is
 * >= N. */
PVCNN_API int pvcnn_batch_s3dis(const float *rows, const void *labels, int label_bytes, const int64_t *offsets, long long W, int max_n,
                      const int64_t *order, long long order_len, const int64_t *cursor, int B, int N, int C_out,
                      const int32_t *choices, const int64_t *seed, float *features, int64_t *targets, void *stream);
/* ShapeNet: C = 6 (normalised coords, normals); features (B, 3 [+ 3 if with_normal] [+ num_shapes], N) with the one-hot plane of
 * shape_ids[item] (num_shapes = 0: none).  jitter_on: coord += fp32(clip(0.01 z, -0.05, 0.05)), z from `jitter` (B, 3, N) fp64 in
 * parity mode, Box-Muller fp32 in device mode. */
PVCNN_API int pvcnn_batch_shapenet(const float *rows, const void *labels, int label_bytes, const int64_t *offsets, long long W,
                         const int32_t *shape_ids, const int64_t *order, long long order_len, const int64_t *cursor, int B, int N,
                         int with_normal, int num_shapes, int jitter_on, const int32_t *choices, const double *jitter,
                         const int64_t *seed, float *features, int64_t *targets, void *stream);
/* Frustum-KITTI with ground truth: C = 4 (rows already rotated when frustum_rotate), labels = the mask.  Per item, computed on the
 * host: item_f64 (W, 4) centre x y z and dist; item_f32 (W, K + 5) one-hot (K classes), heading residual without / with flip, size
 * residual; item_i64 (W, 4) heading bin without / with flip, size template id, class id.  random_flip: x and centre x negated, the
 * flipped heading taken, when flip[b] > 0.5 (`flip` (B) fp64 in parity mode); random_shift: clip(z dist 0.05, 0.8 dist, 1.2 dist) in
 * fp64 (the reference's expression as written; z = shift[b] in parity mode) added to the z coordinate and the centre in fp64, rounded
 * once.  Outputs: features (B,4,N), one_hot_vectors (B,K), mask_logits (B,N) i64, center (B,3), heading_bin_id (B) i64,
 * heading_residual (B), size_template_id (B) i64, size_residual (B,3), class_id (B) i64. */
PVCNN_API int pvcnn_batch_frustum(const float *rows, const void *labels, int label_bytes, const int64_t *offsets, long long W,
                        const double *item_f64, const float *item_f32, const int64_t *item_i64, int K, int random_flip,
                        int random_shift, const int64_t *order, long long order_len, const int64_t *cursor, int B, int N,
                        const int32_t *choices, const double *flip, const double *shift, const int64_t *seed, float *features,
                        float *one_hot_vectors, int64_t *mask_logits, float *center, int64_t *heading_bin_id,
                        float *heading_residual, int64_t *size_template_id, float *size_residual, int64_t *class_id, void *stream);
/* Frustum-KITTI from RGB detections: item_f64 (W) rgb score, item_f32 (W, K + 1) one-hot and rotation angle.  Outputs: features
 * (B,4,N), one_hot_vectors (B,K), rotation_angle (B) fp32, rgb_score (B) fp64 (default_collate of a Python float). */
PVCNN_API int pvcnn_batch_frustum_rgb(const float *rows, const int64_t *offsets, long long W, const double *item_f64,
                            const float *item_f32, int K, const int64_t *order, long long order_len, const int64_t *cursor, int B,
                            int N, const int32_t *choices, const int64_t *seed, float *features, float *one_hot_vectors,
                            float *rotation_angle, double *rgb_score, void *stream);

/* ---- augmentation of an assembled batch (pvcnn_amd/augment.py, csrc/augment.hip; an additive group: the ABI version does not
 * move) -------------------------------------------------------------------------------------------------------------
 * NOT in the reference (its datasets draw what pvcnn_batch_* draw): the usual transforms of point-cloud training -- a rotation about
 * an axis, a rotation perturbation, axis flips, scale, translation, clipped Gaussian jitter, PointNet++'s random point dropout -- as
 * two launches that never allocate.  Every pointer is device memory except `layout`.
 *
 * pvcnn_augment_draw: params (B, PVCNN_AUGMENT_PARAMS = 24) fp64, one row per cloud, from the stream of `seed` ("Device draws": one
 * pair of words may key an assembly and its augmentation).  Row: [0:9] the matrix Rp row-major, [9] scale s, [10:13] translation t,
 * [13] dropout ratio, [14:18] the raw angles theta, a, b, c, [18:21] the three flip uniforms, [21:24] zeros.
 *   theta ~ U(-rot_max, rot_max) about `axis` (0: x, 1: y, 2: z);  a, b, c = clip(perturb_sigma z, +-perturb_clip), z standard normal;
 *   axis k is flipped when u_k < flip_k;  s ~ U(scale_lo, scale_hi);  t ~ U(-translate_max, translate_max)^3;  ratio = u drop_max.
 *   Rp = Rx(a) Ry(b) Rz(c) R_axis(theta) diag(+-1), right-handed rotations, composed in fp64.
 * A range that is off gives that stage's identity exactly: rot_max = 0 -> theta = 0.0, perturb_sigma = 0 -> a = b = c = 0.0 (with both
 * Rp is a 0 / 1 matrix, +-1 with flips), scale_lo = scale_hi = 1 -> s = 1.0, translate_max = 0 -> t = 0.0, drop_max = 0 -> ratio = 0.0.
 *
 * pvcnn_augment_apply: src (B, C, N) fp32 -> dst (B, C, N) fp32, out of place; the C * N floats of a sample are contiguous, samples
 * are *_batch_stride elements apart (>= C * N; ignored for B = 1).  targets_src / targets_dst (B, N) int64 with batch strides of
 * their own: both or neither.  `layout` (HOST memory, read before the call returns): num_triples <= 4 pairs (role, first plane);
 * the planes (c, c + 1, c + 2) of a PVCNN_AUGMENT_POSITION triple become y = s (Rp x) + t + jitter, those of a
 * PVCNN_AUGMENT_DIRECTION triple y = Rp x (normals); every other plane is copied.  Triples beyond C or overlapping are refused.
 *   jitter (jitter_on): per point and axis clip(jitter_sigma z, +-jitter_clip); z from `jitter` (B, 3, N) fp32 when given (PARITY
 *   MODE), else from the Philox stream of `seed` (Box-Muller, fp32).
 *   dropout (drop_on): point n > 0 is dropped when u[b, n] <= ratio[b] (params column 13); u from `keep` (B, N) fp32 when given, else
 *   from the stream.  A dropped point takes point 0's TRANSFORMED planes in all C channels (point 0's own jitter draw) and point 0's
 *   target -- PointNet++'s pc[drop_idx] = pc[0] after the fact.
 *   jitter_out (B, 3, N), keep_out (B, N) fp32, optional: every point's own draws (a dropped point uses point 0's jitter row).
 * Arithmetic: each element in fp64 from the fp32 input, r = (Rp[k][0] x0 + Rp[k][1] x1) + Rp[k][2] x2, y = (s r + t[k]) + jitter[k],
 * no fused multiply-add, rounded once to fp32.
 * Aliasing: dst may be src (the same address and batch stride) when drop_on = 0 only; any other overlap, and any aliasing with
 * dropout on, is refused (a dropped point reads point 0 while another thread writes it).  Likewise the targets.
 * 16-byte accesses when N % 4 == 0 and every base and batch stride is 16-byte aligned, scalar ones otherwise: the same bits.
 * C * N <= 2^31 - 1; sample addressing is 64-bit; the grid strides over N and B. */
#define PVCNN_AUGMENT_PARAMS 24
#define PVCNN_AUGMENT_MAX_TRIPLES 4
#define PVCNN_AUGMENT_POSITION 1
#define PVCNN_AUGMENT_DIRECTION 2
PVCNN_API int pvcnn_augment_draw(int B, int axis, double rot_max, double perturb_sigma, double perturb_clip, double flip_x,
                       double flip_y, double flip_z, double scale_lo, double scale_hi, double translate_max, double drop_max,
                       const int64_t *seed, double *params, void *stream);
PVCNN_API int pvcnn_augment_apply(const float *src, long long src_batch_stride, const int64_t *targets_src,
                        long long targets_src_batch_stride, int B, int C, int N, const int32_t *layout, int num_triples,
                        const double *params, double jitter_sigma, double jitter_clip, int jitter_on, int drop_on,
                        const float *jitter, const float *keep, const int64_t *seed, float *dst, long long dst_batch_stride,
                        int64_t *targets_dst, long long targets_dst_batch_stride, float *jitter_out, float *keep_out,
                        void *stream);

/* ---- 3-nearest-neighbour interpolation ----------------------------------------------------
 * replaces three_nearest_neighbors_interpolate_forward/backward
 *          (interpolate/neighbor_interpolate.cpp:6-65, neighbor_interpolate.cu:20-170)
 * fwd: points_coords (B,3,N), centers_coords (B,3,M), centers_features (B,C,M)
 *      -> indices (B,3,N) i32, weights (B,3,N) f32, out (B,C,N)
 * bwd: grad_y (B,C,N), indices, weights -> grad_x (B,C,M)
 */
PVCNN_API int pvcnn_three_nn_interp_fwd(const float *points_coords, const float *centers_coords,
                              const float *centers_features, int B, int C, int M, int N,
                              int32_t *indices, float *weights, float *out, void *stream);
PVCNN_API size_t pvcnn_three_nn_interp_bwd_workspace_bytes(int B, int C, int N, int M);
PVCNN_API int pvcnn_three_nn_interp_bwd(const float *grad_y, const int32_t *indices, const float *weights,
                              int B, int C, int N, int M, float *grad_x, void *workspace,
                              size_t workspace_bytes, void *stream);

/* ---- 3x3x3 voxel convolution (PVConv.voxel_layers) -------------------------------------------
 * replaces the nn.Conv3d(k=3, stride 1, padding 1) calls of modules/pvconv.py:20-27 (cuDNN in the
 * reference) with an fp32-MFMA implicit GEMM.  x (B,Ci,R,R,R), y (B,Co,R,R,R), channel-major.
 * weight_transform: w (Co,Ci,3,3,3) -> wt, the layout the kernels consume:
 *     for_bwd_data = 0 : wt (Ci,27,Co)                      [forward: y = conv(x, w) + bias]
 *     for_bwd_data = 1 : wt (Co,27,Ci), taps reversed       [grad_x = conv3d_fwd(grad_y, wt) with
 *                                                            Ci and Co exchanged, bias = NULL]
 * fp32 in / fp32 accumulate (v_mfma_f32_32x32x2_f32); results agree with an fp64 evaluation to
 * fp32 round-off (summation order differs from cuDNN / MIOpen / torch-CPU, as theirs do).
 */
PVCNN_API int pvcnn_conv3d_weight_transform(const float *w, int Co, int Ci, int for_bwd_data, float *wt,
                                            void *stream);
PVCNN_API int pvcnn_conv3d_fwd(const float *x, const float *wt, const float *bias, int B, int Ci, int Co,
                               int R, float *y, void *stream);
/* grad_w (Co,Ci,3,3,3) = sum over batch and voxels of grad_y (B,Co,R^3) x shifted x (B,Ci,R^3);
 * grad_bias (Co) = sum of grad_y over batch and voxels (optional: NULL to skip; it comes for free
 * from the grad_y tiles the kernel stages anyway).  Every element written.  `workspace`:
 * >= pvcnn_conv3d_bwd_weight_workspace_bytes(...) bytes of 16-byte aligned scratch (per-partition
 * partial sums; no float atomics). */
PVCNN_API size_t pvcnn_conv3d_bwd_weight_workspace_bytes(int B, int Ci, int Co, int R);
PVCNN_API int pvcnn_conv3d_bwd_weight(const float *x, const float *grad_y, int B, int Ci, int Co, int R,
                                      float *grad_w, float *grad_bias, void *workspace, size_t workspace_bytes,
                                      void *stream);

/* ---- the same convolution on the bf16 matrix cores (csrc/conv3d_bf16.hip) ---------------------------------------
 * nsplit = 1: bf16 operands, fp32 accumulate (BASELINE configs[4], "bf16 with MFMA 3D conv"; ~4e-3 relative).
 * nsplit = 3: "bf16x3" -- both fp32 operands split exactly into three bf16 pieces, the six significant partial products
 *             accumulated in fp32: fp32-class accuracy (<= 1e-5 vs fp64, like pvcnn_conv3d_fwd) at up to 16/6 = 2.7x
 *             the fp32-MFMA rate.
 * nsplit = 2: "f16x2" -- both fp32 operands scaled by a power of two (x: per workgroup tile, see "amax buffers" below; w: per
 *             output channel) and split into fp16 hi + lo (11 + 11 bits); hi*hi + hi*lo + lo*hi accumulated in fp32 and scaled
 *             back exactly: fp32-class accuracy (<= 1e-5 vs fp64) at 3 MFMAs per k-step.  Needs x_absmax = an amax buffer of the
 *             input.
 * amax buffers (f16x2 operand scales): 1 + T uint32 in device memory, T = B * ceil(L / seg) for x viewed as (B, C, L):
 *             [0]     = bit pattern of max |x| over the whole tensor -- the scale of the backward-weight kernels (they reduce
 *                       over positions, where small entries are negligible next to large ones in fp32 as well);
 *             [1 + t] = bit pattern of max |x| over ALL CHANNELS of position segment t = b * ceil(L / seg) + l / seg.
 *             The forward / backward-data kernels scale the tile of x a workgroup stages by the largest segment that tile
 *             (with its halo) touches: Conv3d seg = R (one z row of the grid, T = B*R*R), 1x1 GEMM seg = 256 points (its
 *             point tile).  RANGE CONTRACT: an output element is fp32-class (operands keep 22 bits) whenever the inputs it
 *             depends on are within 2^-17 of the largest magnitude of ITS OWN tile; smaller inputs keep fewer bits (absolute
 *             error <= 2^-38 of the tile maximum per product).  An outlier or a heavy-tailed gradient therefore costs
 *             precision only inside the tiles it occupies -- tests/test_gpu_range.py.  amax_seg = 0 selects the old single
 *             scale ([0] only; any 1-word buffer from pvcnn_absmax_bits will do).
 *             pvcnn_absmax_tiles computes a buffer in one read of x; pvcnn_bnact_fwd / pvcnn_bnact_bwd_strided emit the buffer
 *             of the tensor they write (no extra pass).
 * weight_split: w (Co,Ci,3,3,3) fp32 -> the kernels' pre-split, pre-swizzled LDS image (opaque, *_split_bytes bytes,
 *             16-byte aligned); for_bwd_data = 1 builds the flipped / channel-transposed image with which
 *             grad_x = conv3d_fwd_split(grad_y, wts, NULL, B, Ci = Co_fwd, Co = Ci_fwd, ...).
 * stats_part: NULL, or (Co, *_split_stats_parts) float pairs of per-workgroup (sum, sum of squares) of (y - bias).
 */
PVCNN_API size_t pvcnn_conv3d_weight_split_bytes(int Co, int Ci, int for_bwd_data, int nsplit);
PVCNN_API int pvcnn_conv3d_weight_split(const float *w, int Co, int Ci, int for_bwd_data, int nsplit, void *wts, void *stream);
/* both f16x2 images (for_bwd_data = 0 and 1) of one weight in ONE launch: a training step needs both, the weights do not change in between */
PVCNN_API int pvcnn_conv3d_weight_split_pair(const float *w, int Co, int Ci, void *wts_fwd, void *wts_bwd, void *stream);
PVCNN_API size_t pvcnn_conv3d_fwd_split_stats_parts(int B, int Co, int R, int nsplit);
/* (ABI v8) which launch shape pvcnn_conv3d_fwd_split takes for this problem: (voxels per workgroup tile) << 8 | weight rows per
 * tile (64, or 32 for the half-height tile of layers with Co <= 32 at R = 32).  Pure function of the sizes and the process's
 * switches; for tests and tools that have to prove a given tile ran (tests/test_gpu_parity_as_benched.py).
 * (ABI v17) the value is read off the launch's own plan (csrc/route.h): where the persistent kernel runs (f16x2, R = 32 -- R = 16 with
 * PVCNN_CONV_WIDE16=1 --, Ci % 16 == 0, Ci >= 32, Co > 32, tensors below 4 GiB) it reports that kernel's 4 x 4 x R tile, 512 voxels
 * (256 at R = 16), and the two-workgroup kernel's tile under PVCNN_CONV_WIDE=0; before, the two-workgroup tile in either case. */
PVCNN_API int pvcnn_conv3d_fwd_split_route(int B, int Ci, int Co, int R, int nsplit);
PVCNN_API int pvcnn_absmax_bits(const float *x, size_t n, void *out, void *stream);
PVCNN_API size_t pvcnn_absmax_tiles_count(int B, long L, int seg);      /* 1 + T words */
/* (ABI v11) `ticket`: NULL, or ONE zeroed 32-bit word in device memory that the call leaves zeroed.  With a ticket the global
 * maximum out[0] is written by the workgroup of the table pass that finishes last (release / acquire at device scope) instead of a
 * one-workgroup launch behind it (tables of <= 1024 words; longer ones keep the launch).  MEASURED (round 5, profiles/ab/r05c_*,
 * r05d_*): correct and bit-identical, but NOT faster on gfx950 -- the published atomics and tickets of every workgroup cross the
 * eight XCDs and cost what the ~5 us launches cost; pvcnn_amd passes NULL unless PVCNN_FOLD_FINALIZE=1.  The word must not be shared
 * with a launch that can run concurrently (another stream); launches on one stream may reuse it.  The same convention: `tickets` of
 * pvcnn_bnact_bwd_strided (C words: the per-channel sums are finalised by the workgroup that writes a channel's last partial),
 * `ticket` of pvcnn_concat_points. */
/* (ABI v12) ticket == PVCNN_TABLE_ONLY: the table out[1 ..] only -- word [0] is left UNWRITTEN and nothing is launched for it (~5 us
 * of launch latency, eleven times per PVCNN step).  For buffers whose every consumer takes the maximum from the table: the f16x2
 * convolutions / GEMMs with amax_seg > 0, and pvcnn_conv3d_bwd_weight_f16 / pvcnn_pwconv_bwd_weight_f16 with x_amax_seg / gy_amax_seg
 * > 0 (their workgroups reduce the table themselves: <= 64 KiB from L2).  The same value of `ticket` in pvcnn_concat_points. */
#define PVCNN_TABLE_ONLY ((void *)1)
PVCNN_API int pvcnn_absmax_tiles(const float *x, int B, int C, long L, int seg, void *out, void *ticket, void *stream);
PVCNN_API int pvcnn_conv3d_fwd_split(const float *x, const void *wts, const float *bias, int B, int Ci, int Co, int R, int nsplit,
                           const void *x_absmax, int amax_seg /* 0 | R */, float *y, float *stats_part, void *stream);
/* NEEDED ROWS (additions to ABI v17).  The backward-data product of a PVConv's first convolution has one reader, avg_voxelize's
 * backward, which gathers grad_grid[b, c, ind[n]]: voxels that hold a point.
 *   pvcnn_voxel_need_rows: cnt (B, R^3), the voxel counts of an avg_voxelize plan -> rows (B * R * R words), word (b, x, y) = 1 where
 *   some voxel of the z row holds a point, else 0.  One small launch; depends on the coordinates only.
 *   pvcnn_conv3d_fwd_split_rows: pvcnn_conv3d_fwd_split without bias and statistics.  A workgroup whose own output tile (no halo) has
 *   no needed row stores +0 to its tile and stages nothing; a tile with a needed row is computed exactly as without the table, so
 *   every voxel of a needed row has the bits pvcnn_conv3d_fwd_split gives, and every other voxel either those bits or +0.  Served by
 *   the pipelined R = 16 / 12 kernel and the generic kernel; the persistent wide kernel (R = 32) takes no table and computes
 *   everything.  PVCNN_CONV_BWD_ROWS=0: the table is ignored. */
PVCNN_API int pvcnn_voxel_need_rows(const int32_t *cnt, int B, int R, void *rows, void *stream);
PVCNN_API int pvcnn_conv3d_fwd_split_rows(const float *x, const void *wts, int B, int Ci, int Co, int R, int nsplit, const void *x_absmax,
                                int amax_seg /* 0 | R */, float *y, const void *need_rows, void *stream);
/* THE ACTIVATION TAIL (additions to ABI v17; inference with BatchNorm folded into the weights).  The four *_act entry points are
 * their namesakes with two more steps behind the bias, in the products' epilogues:
 *   y = v > 0 ? v : v * slope          (slope 0: ReLU; 0.1: PVConv's LeakyReLU)
 *   y_amax != NULL: y's amax buffer is emitted.  y_amax points to 1 + (segments of y) words that the caller has ZEROED, y_amax_seg is
 *   the segment length (R: one z row / 256 points); word [1 + t] receives the bits of max |y| over all channels of segment t, combined
 *   across the row tiles by vector atomicMax on the bit patterns (order-independent).  Word [0] is not written: a table-only buffer,
 *   like one made with PVCNN_TABLE_ONLY.  Same shape checks and the same arithmetic as the plain entry points:
 *   y == leaky_relu(plain y, slope) bit for bit.  Same routes (pvcnn_*_fwd_split_route), with one exception: where the plain 1x1 launch
 *   takes the persistent wide kernel (256 / 512 weight rows per item), pvcnn_pwconv_fwd_split_act takes the 128-row kernels, which
 *   compute the same bits -- the wide kernel has no register left for the tail. */
PVCNN_API int pvcnn_conv3d_fwd_split_act(const float *x, const void *wts, const float *bias, int B, int Ci, int Co, int R, int nsplit,
                           const void *x_absmax, int amax_seg /* 0 | R */, float *y, float *stats_part, float slope, void *y_amax,
                           int y_amax_seg /* R */, void *stream);
PVCNN_API int pvcnn_conv3d_fwd_act(const float *x, const float *wt, const float *bias, int B, int Ci, int Co, int R, float *y,
                           float slope, void *y_amax, int y_amax_seg /* R */, void *stream);

/* Backward-weight in the same f16x2 arithmetic (csrc/conv3d_wgrad_f16.hip), R = 8, 12, 16 or 32 (workspace_bytes returns 0 for
 * any other R: use pvcnn_conv3d_bwd_weight).  x_absmax / gy_absmax: pvcnn_absmax_bits of x and grad_y (word [0] of an amax
 * buffer).  (ABI v8) x_amax_seg = R says x_absmax IS an amax buffer with one maximum per z row (pvcnn_absmax_tiles(x, ..., seg = R),
 * or what pvcnn_bnact_fwd emitted): output rows whose nine neighbouring x rows are all zero -- the empty part of a voxelised
 * cloud -- skip their matrix work (exact: they would add zeros); x_amax_seg = 0: a 1-word buffer, nothing is skipped.
 * (ABI v12) gy_amax_seg = R: gy_absmax IS an amax buffer with one maximum per z row, too; with x_amax_seg / gy_amax_seg = R the
 * global maximum the kernel scales by is taken from the TABLE (word [0] is not read: its producer may have been asked for
 * PVCNN_TABLE_ONLY); 0: from word [0] as before.
 * Deterministic (split-K partials summed in a fixed order), <= 1e-5 vs fp64 like pvcnn_conv3d_bwd_weight. */
PVCNN_API size_t pvcnn_conv3d_bwd_weight_f16_workspace_bytes(int B, int Ci, int Co, int R);
PVCNN_API int pvcnn_conv3d_bwd_weight_f16(const float *x, const float *grad_y, const void *x_absmax, int x_amax_seg, const void *gy_absmax,
                                int gy_amax_seg, int B, int Ci, int Co, int R, float *grad_w, float *grad_bias, void *workspace,
                                size_t workspace_bytes, void *stream);

/* ---- 1x1 convolutions of SharedMLP (point branch, classifier) ------------------------------------
 * replaces the nn.Conv1d / nn.Conv2d (kernel 1) calls of modules/shared_mlp.py:9-25 (cuDNN / cuBLAS in the
 * reference) with fp32-MFMA GEMMs that work on the reference's channel-major layout directly:
 *     x (B,K,N), y (B,M,N);  N = points (Conv2d: N = M_centres * U_neighbours, flattened)
 * pwconv_fwd:  y[b,m,n] = sum_k wt[k,m] * x[b,k,n] + bias[m]   -- wt is the weight k-major, (wt_rows >= K, M):
 *     forward       : wt = pwconv_transpose(w (Co,Ci)): (Ci rounded up to 32, Co), zero tail rows; K = Ci, M = Co
 *     backward-data : wt = w (Co,Ci) as it is, wt_rows = Co; K = Co, M = Ci, bias = NULL, x = grad_y
 *   (rows K..wt_rows-1 must be zero; with wt_rows a multiple of 32 the unguarded fast path is available)
 * pwconv_bwd_weight: grad_w (M,K) = sum_{b,n} grad_y[b,m,n] * x[b,k,n]; grad_bias (M) optional (NULL).
 * fp32 in / fp32 accumulate; results agree with an fp64 evaluation to fp32 round-off.
 */
PVCNN_API int pvcnn_pwconv_transpose(const float *w, int M, int K, float *wt, void *stream);
PVCNN_API int pvcnn_pwconv_fwd(const float *x, const float *wt, int wt_rows, const float *bias, int B, int K, int M,
                     int N, float *y, void *stream);
PVCNN_API size_t pvcnn_pwconv_bwd_weight_workspace_bytes(int B, int K, int M, int N);
PVCNN_API int pvcnn_pwconv_bwd_weight(const float *x, const float *grad_y, int B, int K, int M, int N,
                            float *grad_w, float *grad_bias, void *workspace, size_t workspace_bytes,
                            void *stream);

/* ---- the same 1x1 GEMMs on the bf16 matrix cores (csrc/pointwise_bf16.hip): nsplit = 3 "bf16x3" (fp32-class accuracy, <= 1e-5
 * vs fp64) or nsplit = 1 (bf16 operands); see the Conv3d split entry points for the arithmetic.  weight_split: w (Co,Ci) fp32 -> the
 * kernel's pre-split, pre-swizzled image (opaque, *_split_bytes bytes, 16-byte aligned); for_bwd_data = 1 builds the transposed image
 * with which grad_x = pwconv_fwd_split(grad_y, wts, NULL, B, K = Co, M = Ci, ...). */
PVCNN_API size_t pvcnn_pwconv_weight_split_bytes(int Co, int Ci, int for_bwd_data, int nsplit);
PVCNN_API int pvcnn_pwconv_weight_split(const float *w, int Co, int Ci, int for_bwd_data, int nsplit, void *wts, void *stream);
PVCNN_API int pvcnn_pwconv_weight_split_pair(const float *w, int Co, int Ci, void *wts_fwd, void *wts_bwd, void *stream);
PVCNN_API size_t pvcnn_pwconv_fwd_split_stats_parts(int B, int N);
/* (ABI v17) the twin of pvcnn_conv3d_fwd_split_route: the weight rows per workgroup item of the launch pvcnn_pwconv_fwd_split takes
 * for a 16-byte aligned x: 64 or 128, and 256 or 512 where the persistent kernel runs (PVCNN_PW_WIDE=0: never; =2: never 512). */
PVCNN_API int pvcnn_pwconv_fwd_split_route(int B, int K, int M, int N, int nsplit);
PVCNN_API int pvcnn_pwconv_fwd_split(const float *x, const void *wts, const float *bias, int B, int K, int M, int N, int nsplit,
                           const void *x_absmax, int amax_seg /* 0 | 256 */, float *y, float *stats_part, void *stream);
/* ... with the activation tail (see pvcnn_conv3d_fwd_split_act) */
PVCNN_API int pvcnn_pwconv_fwd_split_act(const float *x, const void *wts, const float *bias, int B, int K, int M, int N, int nsplit,
                           const void *x_absmax, int amax_seg /* 0 | 256 */, float *y, float *stats_part, float slope, void *y_amax,
                           int y_amax_seg /* 256 */, void *stream);
PVCNN_API int pvcnn_pwconv_fwd_act(const float *x, const float *wt, int wt_rows, const float *bias, int B, int K, int M, int N,
                           float *y, float slope, void *y_amax, int y_amax_seg /* 256 */, void *stream);
/* Backward-weight of the 1x1 convolution in f16x2 (csrc/pointwise_wgrad_f16.hip), N % 4 == 0 (workspace_bytes returns 0 otherwise:
 * use pvcnn_pwconv_bwd_weight).  x (B,K,N), grad_y (B,M,N) -> grad_w (M,K) [, grad_bias (M)]; *_absmax: pvcnn_absmax_bits of the two
 * tensors (word [0] of an amax buffer).  (ABI v12) x_amax_seg / gy_amax_seg > 0: the buffer is an amax buffer with segments of that
 * many points (pvcnn_absmax_tiles_count(B, N, seg) words) and the global maximum is taken from its TABLE, word [0] is not read (see
 * PVCNN_TABLE_ONLY); 0: from word [0].  Deterministic split-K, <= 1e-5 vs fp64. */
PVCNN_API size_t pvcnn_pwconv_bwd_weight_f16_workspace_bytes(int B, int K, int M, int N);
PVCNN_API int pvcnn_pwconv_bwd_weight_f16(const float *x, const float *grad_y, const void *x_absmax, int x_amax_seg, const void *gy_absmax,
                                int gy_amax_seg, int B, int K, int M, int N, float *grad_w, float *grad_bias, void *workspace,
                                size_t workspace_bytes, void *stream);

/* ---- BatchNorm fused with the following ReLU / LeakyReLU -----------------------------------------
 * replaces the (nn.BatchNorm{1,2,3}d, nn.ReLU | nn.LeakyReLU) module pairs of modules/pvconv.py:20-27
 * and modules/shared_mlp.py:20-25 (cuDNN BN + one more elementwise pass each way in the reference).
 * x, y, grad_* are (B, C, S) channel-major; statistics per channel over B*S.  slope = 0 for ReLU.
 * fwd, training != 0: computes mean / rstd (outputs, saved for backward), updates running_mean /
 *      running_var in place with `momentum` (unbiased variance; NULL = do not track), writes y.
 * fwd, training == 0: the caller supplies mean = running_mean and rstd = 1/sqrt(running_var+eps).
 * bwd: grad_x, grad_gamma, grad_beta (batch statistics differentiated through when training != 0).
 * gamma / beta may be NULL (affine = False).  `workspace`: >= pvcnn_bnact_workspace_bytes(B,C,S).
 * y_amax / gx_amax (NULL, or pvcnn_absmax_tiles_count(B, S, amax_seg) words): the amax buffer of the tensor the call writes (y
 *      resp. grad_x) with segments of amax_seg positions, emitted by the apply pass itself -- the f16x2 convolution that consumes
 *      that tensor needs no pass of its own over it.  amax_seg: ANY length in 1..256 on every entry that takes one (a z row of an
 *      R = 12 grid is a segment of 12; a workgroup then owns floor(256 / amax_seg) whole segments) -- the one exception is
 *      pvcnn_bnact_apply_rowmax, whose row-maximum butterfly needs all 256 lanes: amax_seg must DIVIDE 256 there and it says so.
 *      Word [0] (the global maximum) is accumulated with
 *      one atomic per workgroup when it was zeroed beforehand: by the call's own finalize kernel (training != 0, and always in
 *      bwd), or -- amax_zeroed != 0 -- by the pvcnn_bn_finalize call that produced mean / rstd (its zero_words argument, the WHOLE
 *      buffer: on small position counts the pass splits the channels over several workgroups whose table entries meet by atomic
 *      maxima); with training == 0 and amax_zeroed == 0 a one-workgroup reduction of the table is launched behind the pass instead.
 * tickets (pvcnn_bnact_bwd_strided, ABI v11; NULL, or C zeroed 32-bit words the call leaves zeroed -- see pvcnn_absmax_tiles): the
 *      per-channel sums grad_gamma / grad_beta are combined by the workgroup that writes a channel's last partial (the same fp64
 *      combine, the same bits) instead of a finalize launch between the two passes.
 * drop_seed / drop_p (pvcnn_bnact_fwd, pvcnn_bnact_bwd_strided; NULL / 0: off): the nn.Dropout(p) that follows the pair in the
 *      classifier heads (models/utils.py:15-36), fused: fwd writes y = keep ? act(bn(x)) / (1 - p) : 0 (and y's amax buffer of THAT
 *      tensor), bwd takes grad_y as the gradient of the dropped tensor.  keep(e) of element e is a pure function of (e, *drop_seed):
 *      16 bits of a 32-bit integer mixer, recomputed in every pass, never stored (P(keep) = 1 - round(p * 65536) / 65536).
 *      drop_seed: ONE int64 in device memory, drawn by the caller per forward call and handed to the matching backward call.
 *      Requires y_amax / gx_amax (the position-block-major passes) and B * C * S < 2^33.  pvcnn_dropout_keep_mask writes keep(e) for
 *      e = 0 .. numel - 1 as bytes (tests; not on the training path).
 */
PVCNN_API int pvcnn_dropout_keep_mask(const void *drop_seed, float drop_p, long numel, unsigned char *keep, void *stream);
PVCNN_API size_t pvcnn_bnact_workspace_bytes(int B, int C, int S);
PVCNN_API int pvcnn_bnact_fwd(const float *x, const float *gamma, const float *beta, float *running_mean,
                              float *running_var, int B, int C, int S, float eps, float momentum, float slope,
                              int training, float *mean, float *rstd, float *y, void *y_amax, int amax_seg, int amax_zeroed,
                              void *workspace, size_t workspace_bytes, const void *drop_seed, float drop_p, void *stream);
/* Batch statistics only (training): mean / rstd per channel + running-stat update; the first half of bnact_fwd.
 * Used with pvcnn_trilinear_devox_bnact_fwd, which applies BatchNorm + LeakyReLU while it stages the voxel
 * grid into LDS -- out = trilinear_devoxelize(leaky_relu(bn(feat))) without writing the activated grid
 * (PVConv: the last BatchNorm3d + LeakyReLU of voxel_layers followed by the devoxelization, modules/pvconv.py:
 * 25-27,36).  Bit-identical to bnact_fwd followed by trilinear_devox_fwd.  Requires R^3 * 4 bytes <= 160 KiB.
 * addend (B,C,N) or NULL: outs = devoxelized + addend in the gather's store -- PVConv's "voxel branch + point branch"
 * (modules/pvconv.py:38) without a separate read-modify-write pass; one rounded fp32 addition, as in the reference.
 * se_scale (B,C) or NULL: the squeeze-and-excitation factor of SE3d (modules/se.py:17) applied to the activated grid while it is
 * staged, out = trilinear_devoxelize(leaky_relu(bn(feat)) * se_scale[b][c]) -- a second rounded multiplication, as in the reference. */
/* Convolution forward WITH BatchNorm statistics: as pvcnn_conv3d_fwd / pvcnn_pwconv_fwd, and the epilogue also
 * writes per-workgroup partial (sum, sum of squares) of every output channel to stats_part -- (C, nparts) pairs of
 * floats, nparts = *_fwd_stats_parts(...) -- so the BatchNorm that follows needs no pass over y:
 * pvcnn_bn_finalize turns the partials into mean / rstd (fp64 combine) and updates the running statistics. */
PVCNN_API size_t pvcnn_conv3d_fwd_stats_parts(int B, int Co, int R);
PVCNN_API int pvcnn_conv3d_fwd_stats(const float *x, const float *wt, const float *bias, int B, int Ci, int Co, int R,
                           float *y, float *stats_part, void *stream);
PVCNN_API size_t pvcnn_pwconv_fwd_stats_parts(int B, int N);
PVCNN_API int pvcnn_pwconv_fwd_stats(const float *x, const float *wt, int wt_rows, const float *bias, int B, int K, int M,
                           int N, float *y, float *stats_part, void *stream);
/* The epilogue partials are sums of (y - bias) and (y - bias)^2: pass the convolution's bias as `shift` (NULL = no bias) and
 * bn_finalize adds it back to the mean -- a variance from E[a^2] - E[a]^2 stays accurate when the bias dwarfs the spread. */
PVCNN_API int pvcnn_bn_finalize(const float *part, int C, long nparts, double count, float eps, float momentum, const float *shift,
                      float *running_mean, float *running_var, float *mean, float *rstd,
                      void *zero_words /* NULL | the amax buffer the apply pass that follows will fill: */, long zero_count /* its words, set to 0 */,
                      void *num_batches_tracked /* NULL | one int64 incremented by 1 (nn.BatchNorm's counter) */, void *stream);
PVCNN_API int pvcnn_bn_stats(const float *x, float *running_mean, float *running_var, int B, int C, int S,
                   float eps, float momentum, float *mean, float *rstd, void *workspace,
                   size_t workspace_bytes, void *stream);
PVCNN_API int pvcnn_trilinear_devox_bnact_fwd(const float *coords, const float *feat, const float *gamma,
                                    const float *beta, const float *mean, const float *rstd, float slope,
                                    int B, int C, int N, int R, int is_training, int32_t *inds, float *wgts,
                                    const float *addend, const float *se_scale, float *outs, void *stream);
/* As pvcnn_trilinear_devox_bnact_fwd (no se_scale), with `addend` (B,C,N, required) the PRE-BatchNorm point branch of the PVConv:
 * outs = devoxelized + act(bn(addend)), the addend's BatchNorm (add_gamma / add_beta: C or NULL; add_mean / add_rstd: C) and
 * ReLU | LeakyReLU(add_slope) applied to the addend quad where the store adds it.  Bit-identical to pvcnn_bnact_fwd on the addend
 * followed by pvcnn_trilinear_devox_bnact_fwd; the activated point branch is never written. */
PVCNN_API int pvcnn_trilinear_devox_bnact_addbn_fwd(const float *coords, const float *feat, const float *gamma,
                                    const float *beta, const float *mean, const float *rstd, float slope,
                                    int B, int C, int N, int R, int is_training, int32_t *inds, float *wgts,
                                    const float *addend, const float *add_gamma, const float *add_beta,
                                    const float *add_mean, const float *add_rstd, float add_slope, float *outs, void *stream);
PVCNN_API int pvcnn_bnact_bwd(const float *x, const float *grad_y, const float *gamma, const float *beta,
                              const float *mean, const float *rstd, int B, int C, int S, float slope, int training,
                              float *grad_x, float *grad_gamma, float *grad_beta, void *workspace,
                              size_t workspace_bytes, void *stream);
/* As pvcnn_bnact_bwd / pvcnn_trilinear_devox_bwd, but grad_y may be a channel-slice VIEW of a wider tensor (what
 * the backward of torch.cat hands to each consumer): the C rows of one sample / cloud are contiguous, samples
 * are grad_y_batch_stride elements apart (>= C*S resp. C*N).  Saves the .contiguous() copy of every gradient. */
PVCNN_API int pvcnn_bnact_bwd_strided(const float *x, const float *grad_y, long grad_y_batch_stride, const float *gamma,
                            const float *beta, const float *mean, const float *rstd, int B, int C, int S,
                            float slope, int training, float *grad_x, float *grad_gamma, float *grad_beta,
                            void *gx_amax, int amax_seg, void *workspace, size_t workspace_bytes, const void *drop_seed,
                            float drop_p, void *tickets, void *stream);
/* The two halves of pvcnn_bnact_bwd_strided on their own, for callers that put something between them (PVConv's SE tail,
 * pvcnn_amd/modules/functional/bnact.py: the per-(cloud, channel) sums feed the excitation's backward before the apply pass runs).
 * partial_sums: part (C, B, slices) float pairs, slices = pvcnn_bnact_slices(S): per slice of row (b, c) the sums of g' and g' * xhat
 *   with g' = grad_y * act'(z), z = gamma * xhat + beta, xhat = (x - mean) * rstd; grad_y = NULL means grad_y == 1 (then the two sums
 *   are what SE3d's squeeze needs: sum act(z) = gamma * sum act'(z) xhat + beta * sum act'(z)).
 * bwd_apply: grad_x = gamma * rstd * (g' - sum_beta * inv_count - xhat * sum_gamma * inv_count) [training] or gamma * rstd * g' [eval] with
 *   g' = (grad_y * bc_mul[b][c] + bc_add[b][c]) * act'(z); bc_mul / bc_add (B,C) or NULL (1 / 0); sum_gamma / sum_beta (C) given by
 *   the caller; gx_amax / amax_seg as in pvcnn_bnact_bwd_strided. */
PVCNN_API int pvcnn_bnact_slices(int S);
/* Batched refresh of the f16x2 weight images (pvcnn_conv3d_weight_split_pair / pvcnn_pwconv_weight_split_pair of MANY weights in one
 * launch each): a training step changes every weight once (the optimizer) and needs both images of every layer afterwards -- 13
 * launches per PVCNN step, 56 per PVCNN++ step as per-layer calls.
 * _entry: fills `entry` (HOST memory, 10 int64 words) for one weight and its two image buffers (sized by *_weight_split_bytes(.., 0 / 1,
 *      2)) and returns the number of workgroups it takes (-1: bad argument).  The caller sets entry[9] to the running sum of the counts
 *      of the entries before it, and copies the n x 10 words to device memory.
 * _batch: table = those words on the device, total_rows = the sum of the counts.  Writes exactly what the per-weight calls write. */
PVCNN_API long pvcnn_conv3d_weight_split_pair_entry(const float *w, int Co, int Ci, void *wts_fwd, void *wts_bwd, long long *entry);
PVCNN_API int pvcnn_conv3d_weight_split_pair_batch(const void *table, int n, long total_rows, void *stream);
PVCNN_API long pvcnn_pwconv_weight_split_pair_entry(const float *w, int Co, int Ci, void *wts_fwd, void *wts_bwd, long long *entry);
PVCNN_API int pvcnn_pwconv_weight_split_pair_batch(const void *table, int n, long total_rows, void *stream);
/* (ABI v10) The same for the plain-bf16 images (nsplit = 1: torch.autocast; buffers sized by *_weight_split_bytes(.., 0 / 1, 1)): a
 * Frustum-PVCNN step issued 41 per-layer launches for them. */
PVCNN_API long pvcnn_conv3d_weight_split_pair_entry_bf16(const float *w, int Co, int Ci, void *wts_fwd, void *wts_bwd, long long *entry);
PVCNN_API int pvcnn_conv3d_weight_split_pair_batch_bf16(const void *table, int n, long total_rows, void *stream);
PVCNN_API long pvcnn_pwconv_weight_split_pair_entry_bf16(const float *w, int Co, int Ci, void *wts_fwd, void *wts_bwd, long long *entry);
PVCNN_API int pvcnn_pwconv_weight_split_pair_batch_bf16(const void *table, int n, long total_rows, void *stream);

/* The max over the K neighbours of a centre (modules/pointnet.py:85: `mlp(grouper(...)).max(dim=-1).values` on (B, C, M, K)) and its
 * backward, one streaming pass each.  x: (rows, K) contiguous, 16-byte aligned, rows = B * C * M; K in {4, 8, 16, 32, 64}
 * (pvcnn_neighbor_max_supported; other K: the caller keeps torch's reduction).  out (rows) = the maxima, winners (rows) = their k
 * (ties: the smallest k; a NaN wins against numbers, like torch.max).  bwd: grad_x (rows, K) = grad_out at the winner, 0 elsewhere. */
PVCNN_API int pvcnn_neighbor_max_supported(int K);
PVCNN_API int pvcnn_neighbor_max_fwd(const float *x, long rows, int K, float *out, unsigned char *winners, void *stream);
PVCNN_API int pvcnn_neighbor_max_bwd(const float *grad_out, const unsigned char *winners, long rows, int K, float *grad_x, void *stream);

/* arg-max over long rows: the global max-pool over the points of a cloud (models/s3dis/pvcnn.py:41-43, `features.max(dim=-1)` on
 * (B, C, N)).  x: (rows, K) contiguous, 16-byte aligned, K % 4 == 0; winners (rows) int64 = the first index of the row maximum (a NaN
 * wins against numbers), values (rows) = the maxima or NULL. */
PVCNN_API int pvcnn_row_argmax(const float *x, long rows, int K, long long *winners, float *values, void *stream);

/* (ABI v9) The same arg-max WITHOUT a read of its own: the BatchNorm + activation pass that writes the tensor the max-pool reduces
 * (the last SharedMLP of models/s3dis/pvcnn.py:37-43) emits, per (sample, channel) row, a 64-bit key
 *     (orderable bits of the maximum << 32) | ~(first position of that maximum)
 * into row_keys[b * C + c] by atomic maxima, and pvcnn_row_keys_decode turns the keys into int64 winners (the indices torch.max
 * returns: first index on ties, -0 == +0, a NaN wins) and, unless NULL, the values (read back from y: bit-identical elements).
 * pvcnn_bnact_apply_rowmax is the apply pass of pvcnn_bnact_fwd alone: mean / rstd from pvcnn_bn_finalize, whose zero_words
 * argument must have zeroed BOTH y_amax (pvcnn_absmax_tiles_count(B, S, amax_seg) words) and row_keys (B * C uint64, 8-byte aligned)
 * -- e.g. one buffer holding the two.  S % 256 == 0, amax_seg a multiple of 4 that DIVIDES 256 (4, 8, 16, 32, 64, 128, 256: every lane
 * of a workgroup's 256 positions takes part in the row butterfly), x / y 16-byte aligned. */
/* (ABI v11) y_batch_stride (0 = C * S): the samples of y may be that many elements apart -- the pass writes its output INTO a channel
 * slice of a wider (B, C_total, S) tensor, the concatenation in front of the classifier (models/s3dis/pvcnn.py:45), so that
 * pvcnn_concat_points has nothing to copy for the widest of its sources (`src_amax` there).  pvcnn_row_keys_decode reads the values
 * back from such a y with C and the same stride (C <= 0: a contiguous (rows, S) tensor). */
PVCNN_API int pvcnn_bnact_apply_rowmax(const float *x, const float *gamma, const float *beta, const float *mean, const float *rstd, int B,
                                       int C, int S, float slope, float *y, long y_batch_stride, void *y_amax, int amax_seg,
                                       void *row_keys, void *stream);
PVCNN_API int pvcnn_row_keys_decode(const void *row_keys, const float *y, long rows, int S, long long *winners, float *values,
                                    int C, long y_batch_stride, void *stream);

/* (ABI v10) The box part of Frustum-PointNet's multi-task loss (modules/frustum.py:43-124: FrustumPointNetLoss without the
 * foreground-mask cross entropy) AND its gradient, one launch:
 *   box = huber(|c_t - c|, 2) + huber(|c_t - c_reg|, 1) + CE(heading_scores, h) + CE(size_scores, s)
 *       + w_heading_residual * huber(hrn[h] - h_res_t / heading_bin_width, 1) + w_size_residual * huber(|s_res_t / T[s] - srn[s]|, 1)
 *       + w_corners * huber(min(|corners - corners_t|, |corners - corners_t turned by pi|), 1),   every term a mean over the batch.
 * Inputs (fp32, contiguous): center, center_reg, center_t (B,3); heading_scores, heading_residuals_normalized, heading_residuals
 * (B,NH); size_scores (B,NS); size_residuals_normalized, size_residuals (B,NS,3); heading_bin_id, size_template_id (B) int64;
 * heading_residual_t (B); size_residual_t (B,3); size_templates (NS,3); heading_bin_centers (NH); heading_bin_width = pi / NH in
 * the reference.  Outputs: loss[0] = box; grads (pvcnn_frustum_box_loss_grad_floats(B, NH, NS) floats) = d box / d of the eight network
 * outputs, concatenated: [center 3B | center_reg 3B | heading_scores B*NH | size_scores B*NS | heading_residuals_normalized B*NH |
 * size_residuals_normalized B*NS*3 | heading_residuals B*NH | size_residuals B*NS*3], every element written.  Sub-gradients as
 * autograd takes them (0 at |x| = 0 and at a zero-length vector; an exact tie of the two corner distances splits evenly). */
PVCNN_API size_t pvcnn_frustum_box_loss_grad_floats(int B, int NH, int NS);
PVCNN_API int pvcnn_frustum_box_loss(const float *center, const float *center_reg, const float *heading_scores, const float *size_scores,
                                     const float *heading_residuals_normalized, const float *size_residuals_normalized,
                                     const float *heading_residuals, const float *size_residuals, const long long *heading_bin_id,
                                     const long long *size_template_id, const float *heading_residual_t, const float *size_residual_t,
                                     const float *center_t, const float *size_templates, const float *heading_bin_centers, int B, int NH,
                                     int NS, float heading_bin_width, float w_heading_residual, float w_size_residual, float w_corners,
                                     float *loss, float *grads, void *stream);

/* The excitation of SE3d (modules/se.py:6-17: Linear(C, H, bias=False) + ReLU + Linear(H, C, bias=False) + Sigmoid on the squeezed
 * (B, C) descriptor) between the two reduction passes of PVConv's fused squeeze-and-excitation tail, and its backward.
 * part: (C, B, slices, 2) as pvcnn_bnact_partial_sums writes it (slices = pvcnn_bnact_slices(S)); the sums over the slices are taken here.
 * fwd: part from grad_y == NULL -> a_sum / ax_sum (B, C) = the sums of act'(z) and act'(z) * xhat over the grid (outputs, kept for the
 *      backward); squeezed = (gamma * ax_sum + beta * a_sum) * inv_s, hidden = relu(squeezed W1^T) (B, H), excite = sigmoid(hidden W2^T) (B, C).
 * bwd: part from grad_y = g_y -> P / Q = the sums of g_y act'(z) and g_y act'(z) xhat; -> g_w1 (H, C), g_w2 (C, H), g_mean (B, C) =
 *      dL/dsqueezed * inv_s, and the BatchNorm backward's per-channel sums sum_beta / sum_gamma (C) of g' = (excite g_y + g_mean) act'(z).
 *      workspace: B * (3 C + H) floats.  C <= 2048, H <= 256.  Deterministic (sums over slices and clouds in index order). */
PVCNN_API int pvcnn_se_excite_fwd(const float *part, int slices, const float *gamma, const float *beta, const float *w1, const float *w2,
                        int B, int C, int H, float inv_s, float *a_sum, float *ax_sum, float *squeezed, float *hidden, float *excite,
                        void *stream);
PVCNN_API int pvcnn_se_excite_bwd(const float *part, int slices, const float *a_sum, const float *ax_sum, const float *gamma,
                        const float *beta, const float *squeezed, const float *hidden, const float *excite, const float *w1,
                        const float *w2, int B, int C, int H, float inv_s, float *g_w1, float *g_w2, float *g_mean, float *sum_beta,
                        float *sum_gamma, float *workspace, void *stream);
PVCNN_API int pvcnn_bnact_partial_sums(const float *x, const float *grad_y, long grad_y_batch_stride, const float *gamma, const float *beta,
                             const float *mean, const float *rstd, int B, int C, int S, float slope, float *part, void *stream);
PVCNN_API int pvcnn_bnact_bwd_apply(const float *x, const float *grad_y, long grad_y_batch_stride, const float *gamma, const float *beta,
                          const float *mean, const float *rstd, const float *sum_gamma, const float *sum_beta, const float *bc_mul,
                          const float *bc_add, int B, int C, int S, float slope, int training, float *grad_x, void *gx_amax,
                          int amax_seg, void *stream);
PVCNN_API int pvcnn_trilinear_devox_bwd_strided(const float *grad_y, long grad_y_batch_stride, const int32_t *inds,
                                      const float *wgts, int B, int C, int N, int R, float *grad_x,
                                      void *workspace, size_t workspace_bytes, void *stream);

/* ---- concatenation of per-point feature maps along the channels: torch.cat(features, dim=1) of models/s3dis/pvcnn.py:45 (and
 * models/shapenet/pvcnn.py:41) in one pass that also emits the amax buffer (256-point segments) of its output, i.e. the f16x2 scale
 * table of the classifier GEMM that consumes it.  nsrc <= 8 sources; source i has channels[i] channels, its clouds are bstrides[i]
 * elements apart and pstrides[i] is 1 (rows of N points) or 0 (one value per (cloud, channel), broadcast over the points). */
PVCNN_API int pvcnn_concat_points(const float *const *srcs, const long *bstrides, const int *channels, const int *pstrides,
                        const void *const *src_amax /* (ABI v11) NULL, or per source: NULL = copy it; else the source ALREADY IS its channel
                        slice of out (srcs[i] == out + c0_i * N, bstrides[i] == C_total * N: the pass that produced it wrote it there) and
                        this is its amax buffer (256-point segments), merged into out_amax; nothing is copied for it */,
                        int nsrc, int B, int N, float *out, void *out_amax,
                        void *ticket /* (ABI v11) see pvcnn_absmax_tiles; NULL: a reduce launch */, void *stream);

/* ---- (ABI v11) Linear + BatchNorm1d + ReLU on a handful of rows: the `_linear_bn_relu` blocks of models/utils.py:11-12 -- the cloud
 * descriptor head of models/s3dis/pvcnn.py:22-25 ((B, 1024) -> 256 -> 128) and the dense heads of the Frustum nets -- where B is the
 * batch (16 ... 32 rows).  With so few rows the workgroup that owns an output channel owns that channel's whole batch, so the layer is
 * ONE launch forward (dot products, batch statistics, running statistics + num_batches_tracked, normalise, ReLU; torch modules: 5) and
 * ONE launch backward for everything but grad_x (ReLU mask, the BatchNorm backward, grad_z and the four parameter gradients; torch: 6
 * with the two GEMMs); grad_x = grad_z (rows, Cout) . weight (Cout, Cin) is left to the caller's GEMM.
 * x (rows, Cin), weight (Cout, Cin), z / y / grad_y / grad_z (rows, Cout) row-major fp32; bias / gamma / beta may be NULL;
 * running_mean / running_var NULL = not tracked; num_batches_tracked: NULL or one int64 in device memory (incremented).
 * z (the Linear's output) and mean / rstd are what backward needs.  Training mode only (batch statistics); 2 <= rows <= 64 and
 * rows * Cin * 4 bytes <= 144 KiB: ask pvcnn_dense_bn_relu_supported. */
PVCNN_API int pvcnn_dense_bn_relu_supported(int rows, int Cin, int Cout);
PVCNN_API int pvcnn_dense_bn_relu_fwd(const float *x, const float *weight, const float *bias, const float *gamma, const float *beta,
                                      float *running_mean, float *running_var, void *num_batches_tracked, int rows, int Cin, int Cout,
                                      float eps, float momentum, float *z, float *y, float *mean, float *rstd, void *stream);
PVCNN_API int pvcnn_dense_bn_relu_bwd(const float *x, const float *grad_y, const float *z, const float *mean, const float *rstd,
                                      const float *gamma, const float *beta, int rows, int Cin, int Cout, float *grad_z,
                                      float *grad_weight, float *grad_bias, float *grad_gamma, float *grad_beta, void *stream);

/* ---- the optimizer update of the training step on flat buffers (csrc/optim.hip) ----------------------------------------------
 * replaces torch.optim.Adam's per-tensor update of train.py:96-119 (optimizer.step()) when the parameters share the flat layout of
 * the gradient buckets (pvcnn_amd/dp.py): p, m (exp_avg), v (exp_avg_sq) updated in place, g read; arithmetic of torch.optim.Adam
 * (no amsgrad; weight_decay added to the gradient), fp32.  `step`: one float in device memory = updates done so far (nothing is
 * read back: graph-capturable); inc_step != 0 increments it behind this update (the last buffer of an optimizer step).
 * (ABI v8) `hyper`: five floats in DEVICE memory -- lr, beta1, beta2, eps, weight_decay -- read by the kernel, so that a learning-rate
 * schedule (train.py:121-122: scheduler.step()) reaches launches that were captured into a hipGraph. */
PVCNN_API int pvcnn_adam_step(float *p, const float *g, float *m, float *v, size_t n, float *step, const float *hyper, int inc_step,
                    void *stream);
/* Additions without a version step (nothing existing changes): parameter groups, AdamW, amsgrad and a global gradient norm with a
 * clip coefficient and a skip guard, all on the device -- nothing is allocated, nothing is read back, every launch is capturable.
 *
 * The STATUS BLOCK: 8 floats in device memory (4-byte aligned), owned by the caller.
 *   [0] norm     (written by pvcnn_grad_norm_finalize)  L2 norm over everything the partials covered, before clipping
 *   [1] coef     (written)  min(1, max_norm / (norm + 1e-6)): torch.nn.utils.clip_grad_norm_'s coefficient
 *   [2] skip     (written)  1.0 when the sum of squares is not finite AND [5] != 0, else 0.0
 *   [3] skipped  (updated)  += 1.0 with every finalize that sets [2]; the caller zeroes it once
 *   [4] max_norm (read)     written by the caller (a schedule may move it between replays of a graph); +inf = no clipping
 *   [5] skip_nonfinite (read)  != 0 enables the skip flag
 *   [6], [7] reserved, never touched.
 *
 * pvcnn_grad_sqsum: partials[0 .. nparts) = sums of g[i]^2 over the n floats of one buffer (g 16-byte aligned), one per workgroup of a
 *   grid of nparts (1 ... 65535) workgroups: the caller fixes the grid and with it the order of every addition.  Each lane adds
 *   its squares in index order in fp32; lane totals, waves and workgroups are added in fp64 and the partial is rounded to fp32 once.
 *   n == 0 writes zeros.  Writes partials only.
 * pvcnn_grad_norm_finalize: one workgroup adds partials[0 .. nparts) -- the partials of ALL buffers of an optimizer step, laid out
 *   back to back by the caller -- in a fixed order in fp64 and writes status[0 .. 3] as above (reads [4], [5]).  No atomics: two runs
 *   on the same gradients give the same bits.
 * pvcnn_adam_step_grouped: pvcnn_adam_step for a buffer that holds parameters of several GROUPS, ONE launch for the buffer.
 *   hyper: (ngroups, 5) floats in device memory, lr, beta1, beta2, eps, weight_decay per group (1 <= ngroups <= 256).
 *   runs:  nruns (1 ... 4096) int32 pairs (end offset, group id) in device memory (4-byte aligned): run r covers the elements
 *          [end[r-1], end[r]) (end[-1] = 0); ends strictly increasing, the last one == n (hence n < 2^31); a group boundary may fall on
 *          any element.  A group id outside [0, ngroups) is clamped into it.
 *   vmax:  NULL, or the amsgrad buffer max_exp_avg_sq (n floats, 16-byte aligned, updated in place: vmax = max(vmax, v), and used
 *          in the denominator in v's place).
 *   decoupled != 0: torch.optim.AdamW's order -- p *= 1 - lr * weight_decay, then Adam on the bare gradient -- instead of
 *          g += weight_decay * p.  vmax and decoupled hold for the whole launch, not per group.
 *   status: NULL, or a status block as above: the gradient is multiplied by status[1] in registers (g itself is only read) before
 *          the weight decay -- the order clip_grad_norm_ followed by step() gives -- and with status[2] != 0 the launch writes
 *          NOTHING and inc_step does not increment the counter.
 *   p, g, m, v 16-byte aligned; step, inc_step as for pvcnn_adam_step.  With every group holding the same hyper-parameters, vmax and
 *   status NULL and decoupled 0, p / m / v come out bit-identical to pvcnn_adam_step's. */
PVCNN_API int pvcnn_grad_sqsum(const float *g, size_t n, float *partials, int nparts, void *stream);
PVCNN_API int pvcnn_grad_norm_finalize(const float *partials, int nparts, float *status, void *stream);
PVCNN_API int pvcnn_adam_step_grouped(float *p, const float *g, float *m, float *v, float *vmax, size_t n, float *step,
                                      const float *hyper, int ngroups, const int *runs, int nruns, const float *status,
                                      int decoupled, int inc_step, void *stream);

/* ---- (ABI v13) evaluation on the device (csrc/evaluate.hip): evaluate/s3dis/eval.py:139-216, evaluate/shapenet/eval.py:124-200,
 * meters/s3dis.py, meters/shapenet.py.  Integer atomics only: every output is bitwise deterministic.  Index arrays are int64 (what
 * the reference's numpy code holds); an index outside its range is never dereferenced (see each entry point).
 *
 * pvcnn_eval_tile: the reference's repeat / shuffle / tile + reshape(B*E, num_points, C).transpose in one pass,
 *   out[b*E+e, c, j] = src[b*batch_stride + shuffled[b, e*num_points+j]*point_stride + c*chan_stride],   E = V / num_points,
 * shuffled (B, V), out (B*E, C, num_points) fp32; element strides: a channels-last (W, maxpts, C) window block is (maxpts*C, C, 1),
 * a channels-first (C, P) point set (0, 1, P).  An index outside [0, src_points) writes a quiet NaN.  Bit-exact (a copy). */
PVCNN_API int pvcnn_eval_tile(const float *src, long long batch_stride, long long point_stride, long long chan_stride, long long src_points,
                              const long long *shuffled, int B, int V, int num_points, int C, float *out, void *stream);
/* pvcnn_vote_confidence: logits (B, C, N) -> conf (B, N) fp32, pred (B, N) int32 = F.softmax(x, 1)[:, c0:c1].max(1) with pred += c0.
 * The class range is (c0, c1) for every cloud, or, with `ranges` non-NULL, the per-cloud int32 table ranges (B, 2) in device memory
 * (clamped to [0, C); an empty range gives conf 0, pred -1).  Per point: m = max over all C; s = sum of expf(x_c - m) in class order;
 * conf = expf(x_k - m) / s.  Ties go to the LOWEST k.  expf is the ocml function torch's softmax calls: only the order of torch's sum
 * can differ. */
PVCNN_API int pvcnn_vote_confidence(const float *logits, int B, int C, int N, int c0, int c1, const int *ranges, float *conf, int *pred,
                                    void *stream);
/* pvcnn_vote_merge: update_scene_predictions / update_shape_predictions reproduced exactly, without a host sync.  Vote (b, p) of
 * conf / pred (B, V) targets t = mapping[b*map_stride + shuffled[b, p]] (mapping NULL: t = shuffled[b, p]); the result equals running,
 * in (b, p) order, `if conf > scene_conf[t]: scene_conf[t] = conf; scene_pred[t] = pred`: the first vote that carries a point's
 * maximum wins, and only if it is strictly greater than the stored value.  Votes with conf <= 0 or NaN never win (the state starts
 * at 0) and are dropped, as are votes whose index or target is out of range (shuffled outside [0, map_stride) with a mapping; t outside
 * [0, P)).  scene_conf (P) fp32 and scene_pred (P) int64 are updated in place.  workspace: pvcnn_vote_merge_workspace_bytes(P) bytes,
 * 8-byte aligned, ZERO before the first call; every call leaves it zero again (a captured graph can replay it).  Two launches.
 * Requires B*V < 2^32 and P < 2^31. */
PVCNN_API size_t pvcnn_vote_merge_workspace_bytes(long long P);
PVCNN_API int pvcnn_vote_merge(const float *conf, const int *pred, const long long *shuffled, const long long *mapping, long long map_stride,
                               int B, int V, long long P, float *scene_conf, long long *scene_pred, void *workspace, size_t workspace_bytes,
                               void *stream);
/* pvcnn_seg_counts: update_stats of evaluate/s3dis/eval.py:205-213.  ADDS [seen; positive; correct] of (gt, pred), P int64 values
 * each, into counts (3, C) int64 (accumulated: the caller zeroes it).  wrap_negative != 0 reproduces the reference's numpy indexing:
 * a value in [-C, 0) counts for class value + C -- a point no window voted for keeps pred = -1 and is a POSITIVE OF CLASS C-1
 * (stats[1, -1]); wrap_negative == 0: such values count nowhere.  Any other value outside [0, C) counts nowhere.  C <= 4096. */
PVCNN_API int pvcnn_seg_counts(const long long *gt, const long long *pred, long long P, int C, int wrap_negative, long long *counts,
                               void *stream);
/* pvcnn_seg_meter_update: one read of logits (B, C, N) and int64 targets (B, N), argmax semantics of torch.argmax (the first maximum;
 * a NaN wins against numbers).  B*N < 2^31, C <= 4096.
 *   S3DIS mode (part_ranges NULL): counts (3C + 2) int64 += [seen C | positive C | correct C | numel | correct] (MeterS3DIS.update).
 *   ShapeNet mode: part_ranges (num_part_classes, 2) int32 in device memory maps targets[b, 0] to the shape's part range [s, e),
 *   e - s <= max_parts <= 64; the prediction is the argmax inside [s, e) plus s.  Cloud b WRITES row r = *row_cursor + b (row_cursor:
 *   one int64 in device memory, NULL = 0) of rows (row_capacity, max_parts + 1, 2) int32: (s, e), then (intersection, union) of the
 *   part classes s .. e-1, zeros after.  A label outside the table or a bad range writes (0, 0); a row at or beyond row_capacity is
 *   not written (the caller advances the cursor and checks it against the capacity).  counts is unused. */
PVCNN_API int pvcnn_seg_meter_update(const float *logits, const long long *targets, int B, int C, int N, const int *part_ranges,
                                     int num_part_classes, int max_parts, long long *counts, int *rows, const long long *row_cursor,
                                     long long row_capacity, void *stream);

/* ---- (ABI v14) oriented-box overlaps of the Frustum-PVCNN KITTI metrics (csrc/boxes.hip): meters/kitti/frustum.py,
 * meters/kitti/utils.get_box_iou_3d, evaluate/kitti/utils/iou.py (rotate_iou_gpu_eval), evaluate/kitti/utils/eval.py:58-103
 * (d3_box_overlap), evaluate/kitti/frustum/eval.py:168-244 (update_predictions).  Every intersection is the same fp64 device function on
 * fp32 corners (convex quads in bird's-eye view); no NaN comes out of finite corners: identical boxes give IoU 1, boxes that touch 0,
 * a box of zero area intersects nothing, a union (or a criterion's denominator) of 0 gives 0.
 *
 * pvcnn_frustum_meter_update: MeterFrustumKitti.update in one launch, no host sync.
 *   Box metrics (mask_logits NULL): predicted box = argmax (first maximum, NaN wins) over heading_scores (B, NH) and size_scores
 *   (B, NS); heading = bin_centers[id] + heading_residuals[b, id], size = size_templates[id] + size_residuals[b, id] (fp32); the target
 *   box from heading_bin_id_t / size_template_id_t (int64 (B)), heading_residual_t (B), size_residual_t (B, 3); corners as
 *   get_box_corners_3d.  sums (2) fp64 += [sum iou_2d, sum iou_3d], reduced in a fixed order (bitwise reproducible);
 *   counts (3 + 2 * num_classes) int64 += [B, -, #(iou_3d >= 0.7), #correct of class k (iou_3d >= thresholds[k]) ..., #seen of
 *   class k ...], where box b is of class k when class_id_t[b] == class_ids[k] (int64 / fp64 tables of num_classes <= 64 entries).
 *   A target id outside its table gives IoU 0.
 *   Accuracy (mask_logits (B, C, N) fp32, mask_targets (B, N) int64): counts[0] += B * N, counts[1] += #(argmax over C == target). */
PVCNN_API int pvcnn_frustum_meter_update(const float *center, const float *heading_scores, const float *heading_residuals,
                                         const float *size_scores, const float *size_residuals, const float *center_t,
                                         const long long *heading_bin_id_t, const float *heading_residual_t,
                                         const long long *size_template_id_t, const float *size_residual_t, const long long *class_id_t,
                                         int B, int NH, int NS, const float *bin_centers, const float *size_templates,
                                         const long long *class_ids, const double *thresholds, int num_classes, const float *mask_logits,
                                         const long long *mask_targets, int C, int N, double *sums, long long *counts, void *stream);
/* pvcnn_box_iou_3d: get_box_iou_3d per pair of (B, 3, 8) fp32 corner sets -> iou_3d, iou_2d (B) fp64.  BEV on the upper face's x-z
 * (corners 3, 2, 1, 0), height overlap from the y of corners 0 and 4, a box's volume = BEV area * |y0 - y4|. */
PVCNN_API int pvcnn_box_iou_3d(const float *corners_1, const float *corners_t, int B, double *iou_3d, double *iou_2d, void *stream);
/* pvcnn_rotate_iou: out (N, K) fp32 over rboxes (x, y, dx, dy, angle) fp32, boxes (N, 5) and query_boxes (K, 5), corners as
 * rbbox_to_corners.  out[n, k] is the reference's dev_rotate_iou_eval(query_boxes[k], boxes[n], criterion): criterion -1: IoU,
 * 0: inter / area(query box k), 1: inter / area(box n), other: the intersection area.  Areas are the corner quads' shoelace areas.
 * N <= 65535 * 64; N == 0 or K == 0 launches nothing. */
PVCNN_API int pvcnn_rotate_iou(const float *boxes, long long N, const float *query_boxes, long long K, int criterion, float *out,
                               void *stream);
/* pvcnn_box3d_overlap: d3_box_overlap fused.  bev_boxes (N, 5) / bev_query_boxes (K, 5) fp32 are the BEV columns of boxes (N, 7) /
 * query_boxes (K, 7) fp64 (x, y, z, l, h, w, ry with the height axis z_axis dropped); rinc = the fp32 BEV intersection, then where
 * rinc > 0 the height overlap iw of [c - d * z_center, c + d * (1 - z_center)] (c = column z_axis, d = column z_axis + 3) and
 * inc = iw * rinc, volumes l * h * w, criterion as pvcnn_rotate_iou, in fp64; out (N, K) fp32, 0 where rinc <= 0 or iw <= 0. */
PVCNN_API int pvcnn_box3d_overlap(const float *bev_boxes, const double *boxes, long long N, const float *bev_query_boxes,
                                  const double *query_boxes, long long K, int criterion, int z_axis, double z_center, float *out,
                                  void *stream);
/* pvcnn_frustum_predictions: the decode of evaluate/kitti/frustum/eval.py:180-185 and update_predictions: row step + b of table
 * (rows, 8) fp64 = [h, w, l, cx, cy, cz, angle, rgb_score] with cx = cos(r) x + sin(r) z, cy = y + h / 2, cz = cos(r) z - sin(r) x,
 * angle = r + heading wrapped into [-pi, pi] (at most 64 steps of 2 pi each way), r = rotation_angle[b]; fp64 from the fp32 decode.
 * Requires step + B <= rows. */
PVCNN_API int pvcnn_frustum_predictions(const float *center, const float *heading_scores, const float *heading_residuals,
                                        const float *size_scores, const float *size_residuals, int B, int NH, int NS,
                                        const float *bin_centers, const float *size_templates, const double *rotation_angle,
                                        const double *rgb_score, double *table, long long rows, long long step, void *stream);

/* ---- (ABI v16) S3DIS room preparation (csrc/rooms.hip; reference: data/s3dis/prepare_data.py:119-282) --------------------------------
 * One pass (one block offset) over a room xyzrgb (n, 6) fp64, colours 0..255, is the sequence
 *   pvcnn_room_extent -> [host reads extent, sizes the (gx, gy) block table] -> pvcnn_room_blocks -> pvcnn_room_cells
 *   -> [host orders the points by (merged block, cell key)] -> pvcnn_room_plan -> [host reads status: cells, entries, windows, error]
 *   -> pvcnn_room_fill -> [host orders the entries by (block, shuffle key)] -> pvcnn_room_pack.
 * extent (6) fp64: per-axis minimum and maximum of the raw coordinates.  num_blocks = gx * gy (dense table, at most 2^24); n at most 2^29.
 * status (5) int32: [cells, entries, windows, error bits (1: a point outside the block table, 2: a cell index outside 21 bits),
 * cells that draw from more than 2048 copies (they take the workgroup-per-cell path)].
 * block_tables (5, num_blocks) int32: points, cells, resampled entries, first entry, first window of every merged block.
 * workspace: pvcnn_room_workspace_bytes(n, num_blocks) bytes, 8-byte aligned, for every call that takes one.
 * seed: two int64 words in device memory (the key and counter words of the pass: "Device draws").  All fp64 arithmetic is the
 * reference's, one rounding per operation; minima and counts use integer atomics only: two runs with the same seed are
 * bit-identical. */
PVCNN_API size_t pvcnn_room_workspace_bytes(long long n, long long num_blocks);
PVCNN_API int pvcnn_room_extent(const double *xyzrgb, long long n, double *extent, void *workspace, size_t workspace_bytes, void *stream);
/* point_block (n): dense block key bx * gy + by; block_count, block_target (merge map, step 3), block_rank (the reference's block
 * number: rank among the occupied blocks), each (num_blocks); zeroes status. */
PVCNN_API int pvcnn_room_blocks(const double *xyzrgb, long long n, const double *extent, double offset, double block_size, int gx, int gy,
                                int max_num_points, int *point_block, int *block_count, int *block_target, int *block_rank, int *status,
                                void *workspace, size_t workspace_bytes, void *stream);
/* point_block: in the original key, out the merged block; block_min (num_blocks, 3) bit patterns of the fp64 minima; cell_key (n):
 * (cx, cy, cz) relative to the merged block's minimum, 21 bits each. */
PVCNN_API int pvcnn_room_cells(const double *xyzrgb, long long n, const double *extent, double grid_size, long long num_blocks,
                               const int *block_target, int *point_block, unsigned long long *block_min, long long *cell_key, int *status,
                               void *stream);
/* sorted_block / sorted_key (n): the points ordered by (merged block, cell key).  point_cell (n), cell_start (n + 1), cell_out (n),
 * cell_out_start (n): the cell of every sorted point, the first point, the output count and the first entry of every cell. */
PVCNN_API int pvcnn_room_plan(const int *sorted_block, const long long *sorted_key, long long n, long long num_blocks, int max_num_points,
                              int *point_cell, int *cell_start, int *cell_out, int *cell_out_start, int *block_tables, int *status,
                              void *workspace, size_t workspace_bytes, void *stream);
/* perm (n): the original index of every sorted point.  entry_point / entry_block / entry_key (num_entries): the resampled entries in
 * (block, cell) order, their merged block and the block shuffle's 63-bit keys. */
PVCNN_API int pvcnn_room_fill(const int *perm, const int *sorted_block, const int *point_cell, const int *cell_start,
                              const int *cell_out_start, const int *block_tables, const int *status, long long n, long long num_blocks,
                              long long num_entries, const long long *seed, int *entry_point, int *entry_block, long long *entry_key,
                              void *stream);
/* entry_point / entry_block ordered by (block, shuffle key).  rows (num_entries, 9) fp32, labels_out / indices (num_entries) int32
 * (labels and labels_out may both be NULL), offsets (num_windows + 1) int64, window_block (num_windows) int32; block_minxy
 * (num_blocks, 2) is scratch for the per-block minima over the resampled entries. */
PVCNN_API int pvcnn_room_pack(const double *xyzrgb, const int *labels, long long n, const double *extent, double half_block,
                              const int *entry_point, const int *entry_block, long long num_entries, long long num_blocks,
                              int max_num_points, long long num_windows, const int *block_tables, const int *block_rank,
                              unsigned long long *block_minxy, float *rows, int *labels_out, int *indices, long long *offsets,
                              int *window_block, void *stream);

/* ---- (additive to ABI v16) the KITTI AP evaluation (csrc/kitti_ap.hip, csrc/boxes.hip; reference: evaluate/kitti/utils/eval.py) ---------
 * All data is ragged per image, described by int64 prefix offsets of I + 1 words: gt_off (ground truths), dt_off (detections), dc_off
 * (DontCare ground truths) and pair_off (image i holds dt_i x gt_i overlaps: overlaps[pair_off[i] + det * gt_i + gt], the reference's
 * overlaps[det, gt]).  G / D: all ground truths / detections.  A cell is (class m, difficulty l, min_overlap row k), index
 * (m * L + l) * K + k; min_overlaps (K, M) fp64, all >= 0.  Names are int32 codes: 0 car, 1 pedestrian, 2 cyclist, 3 van,
 * 4 person_sitting, 6 tractor, 7 trailer (the lower-cased name), -2 the exact string 'DontCare', -1 anything else; classes are the
 * reference's 0..7 (5 is 'car' again), difficulties 0..2.
 * An image may hold at most PVCNN_KITTI_AP_MAX_BOXES ground truths and as many detections: the matching entry points take the
 * per-image maxima (max_gt, max_dt) from the caller, who built the offsets, and refuse more -- nothing is truncated.
 * No entry point allocates, synchronises or uses an atomic; every sum has a fixed order: two runs give the same bits. */
#define PVCNN_KITTI_AP_MAX_BOXES 2048
#define PVCNN_KITTI_AP_SAMPLE_POINTS 41
/* pvcnn_image_box_overlap: the reference's image_box_overlap, out (N, K) fp64 over (x1, y1, x2, y2) fp64 boxes (N, 4) and query_boxes
 * (K, 4), bit-equal to the reference's expression (one rounding per operation).  criterion -1: IoU, 0: inter / area(box),
 * 1: inter / area(query box), other: the intersection. */
PVCNN_API int pvcnn_image_box_overlap(const double *boxes, long long N, const double *query_boxes, long long K, int criterion,
                                      double *out, void *stream);
/* pvcnn_kitti_ap_bbox_overlaps: the same IoU over the per-image blocks (boxes = detections, query boxes = ground truths); out
 * (total_pairs) fp64. */
PVCNN_API int pvcnn_kitti_ap_bbox_overlaps(const double *dt_bbox, const double *gt_bbox, const long long *dt_off, const long long *gt_off,
                                           const long long *pair_off, long long images, long long total_pairs, double *out,
                                           void *stream);
/* pvcnn_kitti_ap_box_overlaps: pvcnn_rotate_iou (boxes and query_boxes NULL) or pvcnn_box3d_overlap over the per-image blocks, by the
 * same intersection routine; out (total_pairs) fp32.  box_off / query_off: the offsets of the boxes (detections) and the query boxes
 * (ground truths). */
PVCNN_API int pvcnn_kitti_ap_box_overlaps(const float *bev_boxes, const double *boxes, const float *bev_query_boxes,
                                          const double *query_boxes, const long long *box_off, const long long *query_off,
                                          const long long *pair_off, long long images, long long total_pairs, int criterion, int z_axis,
                                          double z_center, float *out, void *stream);
/* pvcnn_kitti_ap_clean: clean_data for every (class, difficulty): ignored_gt (M * L, G) and ignored_det (M * L, D) int8 in {-1, 0, 1},
 * num_valid_gt (M * L) int64, and dc_index (dc_off[I]) int32: the positions of every image's DontCare ground truths, in order.
 * gt_occluded / gt_truncated (G) fp64; bboxes (., 4) fp64. */
PVCNN_API int pvcnn_kitti_ap_clean(const int *gt_name, const double *gt_bbox, const double *gt_occluded, const double *gt_truncated,
                                   long long G, const int *dt_name, const double *dt_bbox, long long D, const long long *gt_off,
                                   const long long *dc_off, long long images, const int *classes, int num_classes, const int *difficulties,
                                   int num_difficulties, signed char *ignored_gt, signed char *ignored_det, int *dc_index,
                                   long long *num_valid_gt, void *stream);
/* pvcnn_kitti_ap_match: compute_statistics_jit with compute_fp = False for every (image, cell), one wave each: for each ground truth
 * in order, the unassigned detection (ignored_det != -1) with overlap > min_overlap and the highest score, the lowest index among
 * equal scores.  tp_scores (cells, G) fp64: a true positive's score in the slot of its ground truth, -inf in every other slot. */
PVCNN_API int pvcnn_kitti_ap_match(const double *overlaps, const long long *gt_off, const long long *dt_off, const long long *dc_off,
                                   const long long *pair_off, long long images, long long G, long long D, int max_gt, int max_dt,
                                   const signed char *ignored_gt, const signed char *ignored_det, const double *dt_score,
                                   const double *dt_alpha, const double *gt_alpha, const double *dt_bbox, const double *gt_bbox,
                                   const int *dc_index, const double *min_overlaps, int num_classes, int num_difficulties,
                                   int num_min_overlaps, double *tp_scores, void *stream);
/* pvcnn_kitti_ap_thresholds: get_thresholds per cell on sorted_scores (cells, G): tp_scores sorted descending along G (the -inf slots
 * last).  thresholds (cells, 41) fp64, zero behind the first counts[cell] entries; counts (cells) int32.  num_valid_gt (cells / K). */
PVCNN_API int pvcnn_kitti_ap_thresholds(const double *sorted_scores, long long G, const long long *num_valid_gt, int num_cells,
                                        int num_min_overlaps, double *thresholds, int *counts, void *stream);
/* pvcnn_kitti_ap_stats: compute_statistics_jit with compute_fp = True for every (image, threshold slot < counts[cell], cell), summed
 * over the images as fused_compute_statistics does: pr (cells, 41, 4) fp64 = [tp, fp, fn, similarity], zero in the slots at and
 * behind counts[cell].  metric 0 subtracts the detections in DontCare regions from fp; compute_aos != 0 sums (1 + cos(gt_alpha -
 * dt_alpha)) / 2 over the true positives.  workspace: pvcnn_kitti_ap_workspace_bytes(images, cells) bytes, 8-byte aligned. */
PVCNN_API size_t pvcnn_kitti_ap_workspace_bytes(long long images, int num_cells);
PVCNN_API int pvcnn_kitti_ap_stats(const double *overlaps, const long long *gt_off, const long long *dt_off, const long long *dc_off,
                                   const long long *pair_off, long long images, long long G, long long D, int max_gt, int max_dt,
                                   const signed char *ignored_gt, const signed char *ignored_det, const double *dt_score,
                                   const double *dt_alpha, const double *gt_alpha, const double *dt_bbox, const double *gt_bbox,
                                   const int *dc_index, const double *min_overlaps, int num_classes, int num_difficulties,
                                   int num_min_overlaps, const double *thresholds, const int *counts, int metric, int compute_aos,
                                   double *pr, void *workspace, size_t workspace_bytes, void *stream);

/* The segmentation criterion: torch.nn.functional.cross_entropy(x, target, weight, ignore_index, reduction, label_smoothing) for
 * reduction mean / sum, and its gradient, in three launches (an additive group: the ABI version does not move).
 *   x       fp32 (B, C, S): the S positions of a class row contiguous, class stride S, batch stride x_bstride >= C * S elements
 *           (a channel slice of a wider tensor is fine);
 *   target  int64 (B, S): rows contiguous, batch stride t_bstride >= S elements.  A point whose target is ignore_index adds nothing
 *           to the loss and gets a zero gradient.  A target outside [0, C) that is not ignore_index is handled the same way and is
 *           counted; it is never used as an index (torch asserts on the device instead);
 *   weight  fp32 (C) or NULL;
 *   workspace  pvcnn_xent_workspace_bytes(B, S) bytes, 16-byte aligned, written by the two forward launches and read by the
 *           backward one: [denominator, sum of the weights, 0, 0] fp32 | 5 x pvcnn_xent_parts(B, S) fp64 per-workgroup partial sums
 *           (nll numerator, sum of log-sum-exp, weight denominator, out-of-range count, weighted logit sum) | (max, sum of exp) fp32
 *           per point.  weight must be packed (element stride 1).
 *           Both queries are host-only and return 0 for sizes the kernels refuse.
 * pvcnn_xent_partials: the per-point (max, sum of exp) and the per-workgroup partial sums (smoothing != 0: the smoothing numerator
 *   too).  pvcnn_xent_finalize: one workgroup adds the partials in a fixed order in fp64; loss[0] = [(1 - label_smoothing) nll +
 *   label_smoothing / C smooth] / denominator (mean != 0; every point ignored: NaN, as torch) or the numerator (mean == 0);
 *   bad_targets (one int64 in device memory, or NULL) += the out-of-range count, a plain read-modify-write by one
 *   thread: calls that run concurrently (different streams) must not share a counter.  pvcnn_xent_bwd: grad_x (B, C, S) contiguous,
 *   every element written, = grad_out[0] (one fp32 in device memory, read on the device) / denominator * [(1 - eps) w_t (p_j - [j == t])
 *   + eps / C (W p_j - w_j)] (mean == 0: without the division).  The same arguments must go to all three; a bad value is refused before any
 *   pointer is looked at.  Deterministic: no float
 *   atomics, the same bits for the same inputs. */
PVCNN_API size_t pvcnn_xent_parts(long long B, long long S);
PVCNN_API size_t pvcnn_xent_workspace_bytes(long long B, long long S);
PVCNN_API int pvcnn_xent_partials(const float *x, long long x_bstride, const long long *target, long long t_bstride, const float *weight,
                                  long long B, int C, long long S, long long ignore_index, int smoothing, void *workspace, void *stream);
PVCNN_API int pvcnn_xent_finalize(const float *weight, long long B, int C, long long S, double label_smoothing, int mean, void *workspace,
                                  float *loss, long long *bad_targets, void *stream);
PVCNN_API int pvcnn_xent_bwd(const float *x, long long x_bstride, const long long *target, long long t_bstride, const float *weight,
                             const float *grad_out, long long B, int C, long long S, long long ignore_index, float label_smoothing,
                             int mean, const void *workspace, float *grad_x, void *stream);

/* The deep-mutual-learning criterion (csrc/dml.hip; an additive group: the ABI version does not move).  a / x and b / y are fp32
 * (B, C, S) logits laid out like pvcnn_xent_*'s x (batch strides >= C * S elements, no alignment requirement); target, weight,
 * ignore_index, out-of-range targets, grad_out (one fp32 in device memory) and bad_targets are pvcnn_xent_*'s too.  With
 * p = softmax(a), q = softmax(b) per point, log p formed as (a_c - max a) - log(sum exp) so that p_c = 0 gives a zero term, not NaN:
 *
 * KL alone -- the reference's kl_loss(x, y):  loss[0] = sum_points sum_c p_c (log p_c - log q_c) / (B S) with p from x, q from y;
 *   pvcnn_kl_bwd writes grad_y (B, C, S) contiguous, every element, = grad_out[0] (q_j - p_j) / (B S).  x has no gradient.
 *   workspace  pvcnn_kl_workspace_bytes(B, S) = 16 + 16 B S + 8 pvcnn_xent_parts(B, S) bytes, 16-byte aligned:
 *           [0, 1 / (B S), 0, 0] fp32 | (max x, sum exp x, max y, sum exp y) fp32 per point | fp64 per-workgroup partial sums.
 * Pair -- the four terms of a DML step from one pass over both tensors:
 *   loss[0] = cross_entropy(a, target, weight, ignore_index, mean) + KL(q || p) / (B S)     (the first network's loss)
 *   loss[1] = cross_entropy(b, target, weight, ignore_index, mean) + KL(p || q) / (B S)     (the student's)
 *   The KL terms take every point, ignored ones too; the cross-entropy terms skip (and, out of range, count) what pvcnn_xent_*
 *   skips.  Every point ignored: both losses NaN (0 / 0), the gradients hold the KL part alone.
 *   pvcnn_dml_pair_bwd writes the gradient of loss[side] for ITS network (side 0: a, side 1: b; the other network is a constant
 *   of that loss), (B, C, S) contiguous, every element: grad_out[0] [w_t (x_p_j - [j == t]) / den + (x_p_j - other_p_j) / (B S)],
 *   the first term only for a live point.  a and b go in the same order to all three launches.
 *   workspace  pvcnn_dml_pair_workspace_bytes(B, S) = 16 + 16 B S + 48 pvcnn_xent_parts(B, S) bytes, 16-byte aligned:
 *           [den, 1 / (B S), 0, 0] fp32 | (max a, sum exp a, max b, sum exp b) per point | 6 x parts fp64 (nll a, nll b, den,
 *           out-of-range count, KL(q || p), KL(p || q)).
 * Both size queries are host-only and return 0 for sizes the kernels do not index.  A bad value is refused (-1, no launch) before
 * any pointer is looked at.  Deterministic: no float atomics, the same bits for the same inputs. */
PVCNN_API size_t pvcnn_kl_workspace_bytes(long long B, long long S);
PVCNN_API int pvcnn_kl_partials(const float *x, long long x_bstride, const float *y, long long y_bstride, long long B, int C, long long S,
                                void *workspace, void *stream);
PVCNN_API int pvcnn_kl_finalize(long long B, int C, long long S, void *workspace, float *loss, void *stream);
PVCNN_API int pvcnn_kl_bwd(const float *x, long long x_bstride, const float *y, long long y_bstride, const float *grad_out, long long B,
                           int C, long long S, const void *workspace, float *grad_y, void *stream);
PVCNN_API size_t pvcnn_dml_pair_workspace_bytes(long long B, long long S);
PVCNN_API int pvcnn_dml_pair_partials(const float *a, long long a_bstride, const float *b, long long b_bstride, const long long *target,
                                      long long t_bstride, const float *weight, long long B, int C, long long S, long long ignore_index,
                                      void *workspace, void *stream);
PVCNN_API int pvcnn_dml_pair_finalize(long long B, int C, long long S, void *workspace, float *loss, long long *bad_targets, void *stream);
PVCNN_API int pvcnn_dml_pair_bwd(const float *a, long long a_bstride, const float *b, long long b_bstride, const long long *target,
                                 long long t_bstride, const float *weight, const float *grad_out, long long B, int C, long long S,
                                 long long ignore_index, int side, const void *workspace, float *grad, void *stream);

/* The Lovasz-Softmax criterion (csrc/lovasz.hip; Berman et al., CVPR 2018, per_image; an additive group: the ABI version does not
 * move).  THIS is its definition; tests/lovasz_truth.py restates it in numpy.
 *   p       fp32 (B, C, S) probabilities, laid out like pvcnn_xent_*'s x (class rows contiguous, batch stride p_bstride >= C * S):
 *           the caller's own, or softmax(x) over the classes as pvcnn_lovasz_probs writes it (packed, expf(x_c - max) / sum in fp32);
 *   target  int64 (B, S), batch stride t_bstride >= S.  A point is LIVE when its target is not ignore_index and lies in [0, C).  A
 *           target outside [0, C) that is not ignore_index is treated as ignored and counted (pvcnn_xent_*'s bad_targets contract).
 * Per cloud b and class c, over the live points i:  fg_i = (target_i == c),  G = the number of foreground points,
 *   e_i = fg_i ? 1.0f - p_i : p_i                                                (ONE fp32 IEEE subtraction)
 *   the points are ordered by e descending, ties by ascending point index; walking the order with position i = 1, 2, ... and
 *   cf = the foreground points among the first i:  I = G - cf,  U = G + i - cf  (integers, U >= 1); the Jaccard index after i
 *   elements is 1 - I / U and its step, in closed form (never a difference of two indices), in fp64:
 *     step_i = 1 / U for a foreground element,  I / (U (U - 1)) for a background element,
 *     G == 0: step_1 = 1, all others 0                                            (the steps are >= 0 and add up to 1)
 *   loss(b, c) = sum_i e_(i) step_i, added in fp64 in a fixed order.
 * Cloud loss: the mean of loss(b, c) over the COUNTED classes -- classes_all == 0 ('present'): those with G > 0; classes_all != 0
 *   ('all'): all C classes of a cloud that has a live point; a cloud without counted classes gives 0 (k_b = counted classes).
 * loss[0] = the mean of the cloud losses over all B clouds, rounded to fp32 once.
 * Gradient: the order is a constant, so d loss / d e_(i) = step_i / (k_b B); d / d p = -that at a foreground point, +that at a
 *   background one; for logits the softmax Jacobian follows, dx_j = p_j (g_j - sum_c p_c g_c).  Dead points and classes that are
 *   not counted get exact zeros; every element is written.
 * Launches, in this order, with the same arguments:
 *   pvcnn_lovasz_probs     (logits only) p (B, C, S) packed <- softmax(x);
 *   pvcnn_lovasz_sort      grid (C, B), one workgroup per list, the list sorted in LDS (S <= 16384); grad_p (B, C, S) packed <-
 *                          -step / +step at every live point of a counted class (d loss(b, c) / d p), zeros elsewhere;
 *   pvcnn_lovasz_finalize  one workgroup, fp64: loss[0]; bad_targets (one int64 in device memory, or NULL) += the out-of-range
 *                          count (a plain read-modify-write by one thread, as pvcnn_xent_finalize's);
 *   pvcnn_lovasz_bwd       grad (B, C, S) packed, every element: with g_c = grad_out[0] (one fp32 in device memory) * scale[b] *
 *                          grad_p[b][c][.]:  probas != 0: g_c (the gradient for the probabilities);  probas == 0: p_c (g_c - sum_j p_j g_j),
 *                          the products, the sum and the difference formed in fp64 and rounded to fp32 once (at a saturated point the
 *                          difference cancels to the order of 1 - max p).
 *   workspace  pvcnn_lovasz_workspace_bytes(B, C, S) bytes, 16-byte aligned, written by sort and finalize, read by finalize and bwd:
 *           scale (B) fp32 = 1 / (k_b B) (0 for a cloud without counted classes), padded to 16 bytes | (B, C, 4) fp64: loss(b, c),
 *           G, the cloud's live points, the cloud's out-of-range targets.
 *           The query is host-only and returns 0 for what the kernels refuse: S > 16384, B > 65535, sizes they do not index.
 * A bad value is refused (-1, no launch) before any pointer is looked at.  No allocation, no host synchronisation.  Deterministic:
 * no float atomics, the same bits for the same inputs. */
PVCNN_API size_t pvcnn_lovasz_workspace_bytes(long long B, int C, long long S);
PVCNN_API int pvcnn_lovasz_probs(const float *x, long long x_bstride, long long B, int C, long long S, float *p, void *stream);
PVCNN_API int pvcnn_lovasz_sort(const float *p, long long p_bstride, const long long *target, long long t_bstride, long long B, int C,
                                long long S, long long ignore_index, int classes_all, void *workspace, float *grad_p, void *stream);
PVCNN_API int pvcnn_lovasz_finalize(long long B, int C, long long S, int classes_all, void *workspace, float *loss,
                                    long long *bad_targets, void *stream);
PVCNN_API int pvcnn_lovasz_bwd(const float *p, long long p_bstride, const float *grad_p, const float *grad_out, long long B, int C,
                               long long S, int probas, const void *workspace, float *grad, void *stream);

/* ---- KITTI frames: a LiDAR sweep, a calibration and 2-D boxes -> frustums (csrc/frames.hip; an additive group: the ABI version does not
 * move).  The reference reads prepared pickles and has no code for this stage; THIS is its definition, restated in numpy by
 * tests/frames_truth.py.  All geometry is fp64, one rounding per operation, sums left to right; a comparison with NaN is false.
 *
 * calib (33) fp64: P (3, 4), V2C (3, 4), R0 (3, 3), row-major, in that order.  A scan row (x, y, z, r) is fp32, widened:
 *   ref_i  = ((V2C[i,0] x + V2C[i,1] y) + V2C[i,2] z) + V2C[i,3]
 *   rect_i = (R0[i,0] ref_0 + R0[i,1] ref_1) + R0[i,2] ref_2
 *   img_i  = ((P[i,0] rect_0 + P[i,1] rect_1) + P[i,2] rect_2) + P[i,3]
 *   u = img_0 / img_2, v = img_1 / img_2;   in_image = u >= 0 & u < width & v >= 0 & v < height & x > clip_distance
 *   (img_2 == 0 needs no special case: an infinite or NaN u fails a comparison)
 *   rows[i] = (fp32 rect_0, fp32 rect_1, fp32 rect_2, r);  uv[i] = (u, v).  The scan has n points (count[0] when `count` is not NULL,
 *   clamped to [0, cap]); rows, uv and in_image beyond them are zero.
 * boxes (M, PVCNN_FRAME_BOX_COLUMNS) fp64, one row per 2-D box, every angle-dependent scalar computed on the host:
 *   [0..3] xmin ymin xmax ymax   [4] 1 when a 3-D box follows, else 0   [5..7] h w l   [8..10] tx ty tz   [11, 12] cos ry, sin ry
 *   [13, 14] cos, sin of rotation_angle = pi / 2 + frustum_angle   [15] rotation_angle   [16] class id   [17] score
 *   point in box m:  in_image & u >= xmin & u < xmax & v >= ymin & v < ymax
 *   label (3-D box given), on the STORED fp32 coordinates widened: d = rect - t, xl = c dx - s dz, zl = s dx + c dz,
 *   inside = in box m & |xl| <= l / 2 & |zl| <= w / 2 & dy <= 0 & dy >= -h.
 * A point tile is PVCNN_FRAME_TILE consecutive points; tiles = pvcnn_frame_tiles(cap) (0 for a cap outside [1, 2^30]).
 *   mask / label_mask (M, tiles) 64-bit words: bit j of word [m][t] says point 64 t + j lies in box m / in its 3-D box;
 *   prefix (M, tiles + 1) int32: exclusive prefix of the tile counts, [m][tiles] the total;  counts (M, 2) int32: (selected, positives).
 *   label_mask may be NULL (no 3-D boxes: positives are 0).
 * pvcnn_frame_pack: rows (and labels, uint8, may be NULL) of box kept[w] to out_rows[offsets[w] + k], k-th selected point in ascending
 *   point index, for w < W; offsets (W + 1) int64 from the caller (offsets[w + 1] - offsets[w] = the box's count), R = all rows of
 *   out_rows: nothing is written beyond an item's own range or R.
 * pvcnn_frame_batch: for m < M with k = counts[m][0] selected points, position p of num_points takes choices[m][p] clamped to [0, k)
 *   (parity mode) or the pick of [0, k) at (p, m) of the stream of `seed` ("Device draws"), as pvcnn_batch_* draw; the point at that
 *   position (ascending point index) is found through the tile prefix; with `rotate`, x' = fp32(x c + z (-s)), z' = fp32(x s + z c) in
 *   fp64 from the fp32 row (c, s = columns 13, 14).  features (Bmax, 4, num_points), one_hot_vectors (Bmax, K), rotation_angle (Bmax)
 *   fp32, rgb_score (Bmax) fp64, valid (Bmax) bytes.  A box with k < max(min_points, 1) or ymax - ymin < min_box_height, and every row
 *   m >= M, is all zero with valid = 0.
 * pvcnn_frame_rotate_rows: the same rotation of packed rows (R, 4) in place, item w (rows offsets[w] .. offsets[w + 1]) by
 *   cos_sin[w] = (cos, sin) fp64.
 * No entry point allocates, synchronises or uses an atomic: the same bits for the same inputs.  scan, rows, uv, out_rows: 16-byte
 * aligned. */
#define PVCNN_FRAME_TILE 64
#define PVCNN_FRAME_BOX_COLUMNS 18
#define PVCNN_FRAME_MAX_BOXES 4096
PVCNN_API long long pvcnn_frame_tiles(long long cap);
PVCNN_API int pvcnn_frame_project(const float *scan, long long cap, long long n, const int *count, const double *calib, double width,
                                  double height, double clip_distance, float *rows, double *uv, unsigned char *in_image, void *stream);
PVCNN_API int pvcnn_frame_count(const double *uv, const unsigned char *in_image, const float *rows, long long cap, const double *boxes,
                                int M, unsigned long long *mask, unsigned long long *label_mask, int *prefix, int *counts, void *stream);
PVCNN_API int pvcnn_frame_pack(const float *rows, long long cap, const unsigned long long *mask, const unsigned long long *label_mask,
                               const int *prefix, int M, const long long *kept, const long long *offsets, long long W, long long R,
                               float *out_rows, unsigned char *out_labels, void *stream);
PVCNN_API int pvcnn_frame_batch(const float *rows, long long cap, const unsigned long long *mask, const int *prefix, const int *counts,
                                const double *boxes, int M, int Bmax, int num_points, int K, int rotate, int min_points,
                                double min_box_height, const int *choices, const long long *seed, float *features,
                                float *one_hot_vectors, float *rotation_angle, double *rgb_score, unsigned char *valid, void *stream);
PVCNN_API int pvcnn_frame_rotate_rows(float *rows, long long R, const long long *offsets, long long W, const double *cos_sin,
                                      void *stream);

/* ---- KITTI frame store: Frustum-KITTI training batches cut out of the frames, with a fresh perturbation of every sample's 2-D box
 * (csrc/frame_store.hip, pvcnn_amd/frame_store.py; an additive group: the ABI version does not move).  The original preparation
 * (frustum-pointnets' extract_frustum_data, perturb_box2d) draws five perturbed copies of every ground-truth box once, offline; here the
 * draw is made per sample when the batch is assembled.  THIS is the definition, restated in numpy by tests/frame_store_truth.py: fp64,
 * one rounding per operation, left to right.
 *
 * The store: `rows` (R, 4) fp32 and `uv` (R, 2) fp64 of the IN-IMAGE points of every frame (pvcnn_frame_project's outputs, the points
 * with in_image = 0 left out, ascending point index), frame f owning rows frame_offsets[f] .. frame_offsets[f + 1] (at most
 * max_frame_points <= PVCNN_FRAME_STORE_MAX_POINTS of them: it sizes the launch's LDS, pvcnn_frame_store_lds_bytes).  An item is one
 * object: item_f64 (W, PVCNN_FRAME_STORE_ITEM_COLUMNS), every trigonometric scalar from the host:
 *   [0..2] P[0,0] P[0,2] P[0,3]   [3..6] xmin ymin xmax ymax   [7..9] h w l   [10..12] tx ty tz   [13, 14] cos ry, sin ry   [15] ry
 *   [16..18] the centre (corner 0 + corner 6) / 2, not rotated   [19] rotation_angle = pi / 2 + frustum_angle of the stored box
 *   [20, 21] its cos, sin   [22, 23] zero;
 * item_f32 (W, K + 3): one-hot, size residual;  item_i64 (W, 3): frame, size template id, class id.
 * Sample b is item order[cursor[0] + b], as pvcnn_batch_* read it; items, frames, offsets and parity choices are clamped to the store.
 *
 * Box perturbation, r = shift_ratio, four uniforms u0..u3 in [0, 1) (the original's random_shift_box2d, its draws in its order):
 *   w = xmax - xmin;  h = ymax - ymin;  cx = (xmin + xmax) / 2;  cy = (ymin + ymax) / 2
 *   cx2 = cx + (w r) (u0 2 - 1);  cy2 = cy + (h r) (u1 2 - 1);  h2 = h ((1 + (u2 2) r) - r);  w2 = w ((1 + (u3 2) r) - r)
 *   box' = (cx2 - w2 / 2, cy2 - h2 / 2, cx2 + w2 / 2, cy2 + h2 / 2)
 *   rotation_angle' = pi / 2 + (-atan2(20, X)),  X = ((cu - P02) 20) / P00 + P03 / (-P00),  cu = (xmin' + xmax') / 2.
 * shift_ratio == 0: no perturbation -- no draw is consumed, the stored box and the host's angle are used, used = 0.
 * Selection: point in box = u >= xmin & u < xmax & v >= ymin & v < ymax on the stored uv; positive = selected & inside the 3-D box by
 * the box-frame test of pvcnn_frame_count on the stored fp32 row.  The perturbed box is used iff ymax' - ymin' >= min_box_height and it
 * selects a positive point (used = 1); otherwise the item's stored box with the host's angle, cos and sin (used = 0).
 * Of the k selected points of the box used, position p of N takes choices[b][p] clamped to [0, k) or
 * the pick of [0, k) at (p, b) of the stream of `seed` ("Device draws"), as pvcnn_frame_batch; k == 0 yields zeros.
 * mask_logits = the box-frame test of the picked row.  With frustum_rotate: the row as pvcnn_frame_batch rotates it
 * (x' = fp32(x c + z (-s)), z' = fp32(x s + z c)), the centre cx' = cx c + cz (-s), cz' = cx s + cz c, heading = ry - rotation_angle
 * (c, s, rotation_angle of the box used); without it, rows, centre and heading = ry stay.  dist = sqrt(c0 c0 + c1 c1) of that centre
 * (the reference's expression as written); heading bin and residual = pvcnn_amd.data.angle_to_bin_id of heading, or of pi - heading
 * when flipped (% is numpy's: fmod, plus the divisor when the remainder is non-zero and negative); flip and shift are those of
 * pvcnn_batch_frustum, the same draws (use 2 at (0, b)) and the same arithmetic.
 *
 * PARITY MODE (`choices` given): `params` (B, PVCNN_FRAME_STORE_PARAMS) fp64 rows [0..3] u0..u3, [4..7] the perturbed box,
 * [8] rotation_angle', [9, 10] its cos, sin, [11] zero -- required when shift_ratio != 0; the box and the angle are TAKEN from the row
 * (no trigonometric function runs on the device); `flip` / `shift` (B) fp64 as pvcnn_batch_frustum.  params, flip or shift without
 * choices are refused.  DEVICE MODE: u_j = word j of use 3 at (0, b) of the stream of `seed` ("Device draws") times 2^-32; cos and
 * sin of rotation_angle' are the device's fp64 library functions.  Optional outputs in both modes: params_out (B, 12) the rows used,
 * `used` (B) int32, choices_out (B, N) int32, flip_out (B) fp64 (1 / 0), shift_out (B) fp64 (the normal draw) -- fed back in parity
 * mode they reproduce the batch bit for bit.  Outputs as pvcnn_batch_frustum.  One launch; never allocates, synchronises or uses an
 * atomic. */
#define PVCNN_FRAME_STORE_PARAMS 12
#define PVCNN_FRAME_STORE_ITEM_COLUMNS 24
#define PVCNN_FRAME_STORE_MAX_POINTS 131072
PVCNN_API size_t pvcnn_frame_store_lds_bytes(long long max_frame_points);
PVCNN_API int pvcnn_frame_store_batch(const float *rows, const double *uv, const int64_t *frame_offsets, long long F, long long R,
                                      long long max_frame_points, const double *item_f64, const float *item_f32,
                                      const int64_t *item_i64, long long W, int K, int num_heading_angle_bins, int frustum_rotate,
                                      int random_flip, int random_shift, double shift_ratio, double min_box_height,
                                      const int64_t *order, long long order_len, const int64_t *cursor, int B, int N,
                                      const double *params, const int32_t *choices, const double *flip, const double *shift,
                                      const int64_t *seed, float *features, float *one_hot_vectors, int64_t *mask_logits, float *center,
                                      int64_t *heading_bin_id, float *heading_residual, int64_t *size_template_id, float *size_residual,
                                      int64_t *class_id, double *params_out, int32_t *used, int32_t *choices_out, double *flip_out,
                                      double *shift_out, void *stream);

/* ---- Shapes on the device: exact k-nearest neighbours over packed ragged clouds and PCA surface normals from them (csrc/shapes.hip,
 * pvcnn_amd/shapes.py; an additive group: the ABI version does not move).  The reference's ShapeNet recipes read xyz, a surface normal
 * and a one-hot shape id per point, and only the benchmark's text files carry those normals; these entry points compute them from xyz.
 * THIS is the definition, restated in numpy by tests/shapes_truth.py.
 *
 * Layout (data._Store's): rows (R, ld) fp32, ld >= 3, xyz in the first three columns; offsets (W + 1) int64, cloud w owning rows
 * offsets[w] .. offsets[w + 1], n_w >= 1 of them, offsets[0] = 0, offsets[W] = R; R <= 2^31 - 64.
 *
 * pvcnn_k_nearest, 1 <= k <= PVCNN_K_NEAREST_MAX_K: for a query row i and a candidate row j of the same cloud
 *   dx = fl32(xj - xi), dy, dz likewise;  d = fl32(fl32(fl32(dx dx) + fl32(dy dy)) + fl32(dz dz))
 *   (one rounding per operation, no fused multiply-add).  out (R, k) int32: the min(k, n_w) candidates smallest in (d, j), ascending,
 *   as positions INSIDE the cloud (0 .. n_w - 1); the query is a candidate like any other (d = 0); columns past n_w hold -1.  Finite
 *   coordinates are the contract: with others the result is unspecified, but every index written lies in [-1, n_w) and nothing is read
 *   out of range.  The search is exhaustive, O(n_w^2) per cloud: the caller bounds n_w (pvcnn_amd.shapes: max_cloud_points).
 *
 * pvcnn_shape_normals: knn (R, k) as above.  For a point with c = min(k, n_w) neighbours: m = their mean, C = sum (p - m)(p - m)^T;
 *   the normal is a unit eigenvector of C's smallest eigenvalue lambda_0, the curvature lambda_0 / trace(C); with c < 3 or
 *   trace(C) == 0 the normal is (0, 0, 0) and the curvature 0.  Mean and C are accumulated in fp64 over the table's columns in order, the
 *   eigenvector comes from a fixed number of Jacobi sweeps in fp64 (csrc/eig3.h) and is rounded to fp32 once.  ref (W, 3) fp32, one
 *   point per cloud, and mode: 0 sign unspecified (ref may be NULL); 1 outward, n . (p - ref_w) >= 0; 2 towards, n . (ref_w - p) >= 0
 *   (the product of the ROUNDED normal, in fp64; a zero product keeps the solver's sign).  normals (R, 3) fp32; curvature (R) fp32 or
 *   NULL.  Table entries outside [0, n_w) are skipped (and not counted in c).
 *
 * pvcnn_cloud_centroids: out (W, 3) fp32 = the fp64 mean of each cloud's xyz, rounded once (the `ref` of mode 1).  One wave per cloud:
 *   lane l adds rows l, l + 64, ... in order, then the butterfly over the lane bits 5 .. 0: the same bits for the same input.
 *
 * Plain launches on `stream`: no allocation, no synchronisation, no atomics, no workspace; they can be captured. */
#define PVCNN_K_NEAREST_MAX_K 64
PVCNN_API int pvcnn_k_nearest(const float *rows, long long R, int ld, const int64_t *offsets, long long W, int k, int32_t *out,
                              void *stream);
PVCNN_API int pvcnn_shape_normals(const float *rows, long long R, int ld, const int64_t *offsets, long long W, const int32_t *knn,
                                  int k, const float *ref, int mode, float *normals, float *curvature, void *stream);
PVCNN_API int pvcnn_cloud_centroids(const float *rows, long long R, int ld, const int64_t *offsets, long long W, float *out,
                                    void *stream);

/* ---- Sparse voxels: the submanifold sparse 3x3x3 convolution on the occupied voxels of a cloud (csrc/sparse.hip,
 * pvcnn_amd/modules/functional/sparse.py; an additive group: the ABI version does not move).  A dense Conv3d forms an output at every
 * voxel of the grid; this operator is defined on the ACTIVE voxels only -- those that hold at least one point -- which is the
 * convolution of SPVCNN.  THIS is the definition, restated in torch fp64 by tests/sparse_conv_truth.py.
 *
 * The map, from cnt (B, R^3) int32 (what voxelization already has), built once per (coordinates, R).  A voxel is active when
 * cnt > 0.  With `cap` the static capacity in rows, chosen by the caller, and count = min(active voxels, cap):
 *   voxel   (cap)     int32  the flat voxel number b R^3 + (x R + y) R + z of row j < count, ascending: the rows of one cloud are
 *                            consecutive, neighbours in z are adjacent rows; -1 for j >= count.
 *   index   (B R^3)   int32  the row of a voxel, or -1 (inactive, or dropped because cap was too small).
 *   offsets (B + 1)   int32  the first row of every cloud, clamped to cap; offsets[B] IS the device word `count` that every other
 *                            entry point takes.  The count never visits the host: every launch is sized by cap and bounded by this
 *                            word, so the group can be captured in a graph and replayed on another occupancy.
 *   nbr     (cap, 27) int32  the row of each of the 27 neighbours of row j, in nn.Conv3d's tap order (dx, dy, dz), tap = 9 (dx + 1) +
 *                            3 (dy + 1) + (dz + 1); tap 13 is j itself; -1 for a neighbour that is inactive, outside [0, R) in any
 *                            axis (never a voxel of another cloud or of the next z row), and everywhere for j >= count.
 *   overflow (1)      int32  1 when more than cap voxels are active -- the map then keeps the first cap of them and nothing is written
 *                            out of bounds -- else 0.
 * Supported: 1 <= R <= PVCNN_SPARSE_MAX_R, B R^3 < 2^31, 1 <= cap < 2^31 / 27; the size queries return 0 outside that range.  Four
 * launches (count per chunk, scan, fill, table), no atomics: deterministic.
 *
 * pvcnn_sparse_gather: grid (B, C, R^3) fp32 -> rows (cap, C) fp32, row-major (a voxel's channels are contiguous); rows >= count are
 *   written as zeros.  pvcnn_sparse_scatter: rows -> grid, zero at every voxel without a row; every word of the grid is written.  Each
 *   is the other's backward.
 *
 * The convolution, weight (Co, Ci, 3, 3, 3) as nn.Conv3d holds it:
 *   y[j, co] = bias[co] + sum_tap sum_ci W[co, ci, tap] x[nbr[j, tap], ci]      j < count; nbr = -1 contributes nothing
 *   y[j, :]  = 0                                                                j >= count (no bias there)
 *   = F.conv3d(padding = 1) of the zero-filled dense grid, read at the active voxels.  No row >= count of x is ever read.
 *   Arithmetic: v_mfma_f32_32x32x2_f32, exact fp32 operands, fp32 accumulation in the order (tap, ci) ascending -- the `fp32` math
 *   mode of csrc/conv3d.hip.  A tile of PVCNN_SPARSE_ROW_TILE rows leaves out a tap at which none of its rows has a neighbour: only
 *   products with an exact zero, the same bits (pvcnn_sparse_debug_skip(0) keeps them in; -1 only asks; returns the previous state).
 *   pvcnn_sparse_conv3d_weight_transform: W -> the image `wt` pvcnn_sparse_conv3d_fwd takes, (27, Ci, Co); for_bwd_data: (27, Co, Ci)
 *   with the taps reversed, on which the same entry point (Ci and Co exchanged, no bias, grad_y for x) is backward-data
 *   grad_x[i, ci] = sum_tap sum_co W[co, ci, tap] grad_y[nbr[i, 26 - tap], co].
 *   pvcnn_sparse_conv3d_bwd_weight: grad_w[co, ci, tap] = sum_j grad_y[j, co] x[nbr[j, tap], ci] and grad_bias[co] = sum_{j < count}
 *   grad_y[j, co] (either may be NULL): partial sums over chunks of PVCNN_SPARSE_WGRAD_CHUNK rows in `workspace` (16-byte aligned),
 *   added in ascending chunk order by a second launch.  No float atomics: every result of the group is the same bits on every run.
 *
 * Plain launches on `stream`: no allocation, no synchronisation. */
#define PVCNN_SPARSE_MAX_R 128
#define PVCNN_SPARSE_ROW_TILE 64
#define PVCNN_SPARSE_WGRAD_CHUNK 1024
PVCNN_API size_t pvcnn_sparse_map_workspace_bytes(int B, int R);
PVCNN_API size_t pvcnn_sparse_map_bytes(int B, int R, long long cap);
PVCNN_API int pvcnn_sparse_map(const int32_t *cnt, int B, int R, long long cap, int32_t *voxel, int32_t *index, int32_t *offsets,
                               int32_t *nbr, int32_t *overflow, void *workspace, size_t workspace_bytes, void *stream);
PVCNN_API int pvcnn_sparse_gather(const float *grid, const int32_t *voxel, const int32_t *count, int B, int C, int R, long long cap,
                                  float *rows, void *stream);
PVCNN_API int pvcnn_sparse_scatter(const float *rows, const int32_t *index, const int32_t *count, int B, int C, int R, long long cap,
                                   float *grid, void *stream);
PVCNN_API int pvcnn_sparse_conv3d_weight_transform(const float *w, int Co, int Ci, int for_bwd_data, float *wt, void *stream);
PVCNN_API int pvcnn_sparse_conv3d_fwd(const float *x, const float *wt, const float *bias, const int32_t *nbr, const int32_t *count,
                                      long long cap, int Ci, int Co, float *y, void *stream);
PVCNN_API size_t pvcnn_sparse_conv3d_bwd_weight_workspace_bytes(long long cap, int Ci, int Co);
PVCNN_API int pvcnn_sparse_conv3d_bwd_weight(const float *x, const float *grad_y, const int32_t *nbr, const int32_t *count,
                                             long long cap, int Ci, int Co, float *grad_w, float *grad_bias, void *workspace,
                                             size_t workspace_bytes, void *stream);
PVCNN_API int pvcnn_sparse_debug_skip(int on);

#ifdef __cplusplus
}
#endif
#endif /* PVCNN_HIP_H_ */
