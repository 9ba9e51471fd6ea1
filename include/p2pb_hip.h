/*
 * p2pb_hip.h -- C ABI of libp2pb_hip.so, the MI355X (gfx950) implementation of the P2P-Bridge hot path.
 *
 * This is the drop-in boundary: every entry point replaces one launcher of the reference's CUDA
 * extensions (the closest thing the reference has to a C interface are the raw-pointer launcher
 * prototypes in its .cuh files; the pybind layer above them only allocates outputs and checks dtypes).
 * Reference paths are relative to the reference repository root;
 *   PN2 = third_party/openpoints/cpp/pointnet2_batch/src.
 *
 * Conventions
 *   - all pointers are DEVICE pointers (HBM), fp32 / int32, contiguous, layouts exactly as the
 *     reference's tensors: point tensors channel-major [B,C,N], coords [B,3,N], metric clouds [B,N,3];
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream). Every kernel is enqueued
 *     on it; nothing synchronises, allocates or touches the host, so a sequence of calls is
 *     hipGraph-capturable (the reference launches vox/devox/FPS/metrics on the legacy default
 *     stream: PN2/vox_gpu.cu:125, PN2/trilinear_devox_gpu.cu:175, PN2/pvcnn_sampling_gpu.cu:189);
 *   - outputs are fully written by the callee (no pre-zeroing needed) unless stated;
 *   - workspaces are caller-provided (sizes via the *_ws_bytes helpers);
 *   - return value: 0 on success, a hipError_t value on launch failure, negative on invalid
 *     arguments (P2PB_EINVAL). The reference exit(-1)s (PN2/cuda_utils.cuh:30-39) or returns 0/1.
 */
#ifndef P2PB_HIP_H
#define P2PB_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define P2PB_EINVAL (-22)

/* ABI version of THIS header: bumped whenever an entry point is added, removed or changes meaning (13: the four
 * p2pb_imgfeat_* entry points added -- the nine p2pb_scan_* and the five p2pb_pairs_* entry points came later WITHOUT a bump: they are pure additions, no
 * existing entry point changed, and the loader's symbol check already refuses a library that lacks them; 12: the eleven p2pb_pointops_* operators added; 11: the five p2pb_pn2_* operators added; 10: the GroupNorm finisher is
 * passed to p2pb_pointwise_conv_forward / _conv_pool_forward / _conv_pool_gather as fin_* arguments, the three
 * entry points that armed one for the thread's next launch removed; 9: the set metrics
 * p2pb_pairwise_chamfer / p2pb_pairwise_emd / p2pb_occupancy_* added; 8: p2pb_softmax_attention_* added; 7: p2pb_norm_act_backward_ex, p2pb_affine_act_train; 6, since 1: p2pb_debug_gn_finisher removed, flag bit 5 of
 * p2pb_conv3d_k3_forward_sparse, arithmetic code 3 in p2pb_set_split_terms_thread, p2pb_group_sub_stats*, p2pb_se_gate_*,
 * p2pb_conv3d_k3_wgrad_occ*, the *_amax / *_adjoint packs).
 * A binding must compare p2pb_version() with the P2PB_ABI_VERSION it was written against and refuse a mismatch
 * (p2p_bridge_amd/_lib.py does): a stale library behind P2PB_LIB_PATH otherwise fails late, or silently differently.
 * The Python binding takes every entry point's name, return type and parameter types, and this version, from this file
 * when it loads, so a declaration must keep the plain `type name(params);` form (no macros, no function pointers). */
#define P2PB_ABI_VERSION 13

/* library / device info --------------------------------------------------------------------- */
int p2pb_version(void);            /* == P2PB_ABI_VERSION of the header the library was built from */
const char *p2pb_target_arch(void); /* "gfx950" */
/* Arithmetic of the split-operand matrix kernels (conv3d_k3 *_forward, pointwise_conv *_forward with >= 128 channels).
 * The reference's layers are cuDNN / cuBLAS convolutions in fp32, which on its Ampere+ targets run as TF32
 * (torch.backends.cudnn.allow_tf32 defaults to True; train.py:221 also sets float32_matmul_precision("high")).
 * gfx950 has no TF32: an fp32 operand is split into 16-bit terms and a product is a sum of EXACT matrix products of the
 * terms, accumulated in fp32 (operands, accumulation and results stay fp32):
 *   16 (default) fp16 pair h0 + h1 of the SCALED operand, h1g0 + h0g1 + h0g0 -- <= 3 * 2^-22 relative per product inside
 *                fp16's range: activations are multiplied by 4 and saturate at |x| = 16376, below |x| = 2^-5 the
 *                representation error is an absolute 2^-27; weights get a per-tensor power-of-two scale at pack time;
 *    6           bf16 terms x0 + x1 + x2: x2y0 + x1y1 + x0y2 + x1y0 + x0y1 + x0y0 -- within a quarter ulp of fp32 at any
 *                magnitude (use it for operands without a usable scale: gradients).
 * Process-wide; takes effect at the next launch (a captured graph keeps what it captured). The *_pack_weights_split
 * functions pack for the arithmetic selected when they are called: re-pack after a switch.
 * -> 0, or P2PB_EINVAL for anything but 6 or 16. */
int p2pb_set_split_terms(int terms);
/* the same for the CALLING THREAD only (0 clears it): a temporary switch, e.g. around one backward pass, that other
 * threads' launches and weight packs do not see; p2pb_get_split_terms returns what a launch from this thread would use */
int p2pb_set_split_terms_thread(int terms);
int p2pb_get_split_terms(void);
/* Deterministic mode (process-wide, default off): the scatter-add backward passes (csrc/scatter_grad.hip: p2pb_trilinear_devoxelize_backward,
 * p2pb_grouping_backward, p2pb_three_nn_interpolate_backward -- the adjoints of PN2/trilinear_devox_gpu.cu:111,
 * pvcnn_grouping_gpu.cu:51, pvcnn_neighbor_interpolate_gpu.cu:101, whose float atomicAdd order is arbitrary in the reference
 * too) accumulate in a fixed order -- one wave per workgroup over rows held in LDS -- so that a training run is bit-reproducible;
 * slower. A row that does not fit 128 KB of LDS is refused (P2PB_EINVAL) instead of falling back to global atomics.
 * HARDWARE ASSUMPTION (gfx950, the only architecture this library is built for -- p2pb_target_arch): the 64 lanes of ONE
 * ds_add_f32 instruction that hit the same LDS address are served in ascending lane order. The ISA manual does not promise
 * it; tests/test_train_gpu.py::test_deterministic_mode_makes_training_bit_reproducible (two whole training runs, bit for bit) is what holds it on this part. */
int p2pb_set_deterministic(int on);
int p2pb_get_deterministic(void);
/* Test / debug hook: the kernel form the most recent p2pb_pointwise_conv* launch with these (cin, cout, npos) took
 * (0 exact-fp32 unaligned, 1 wide exact-fp32, 2 wide f16x3, 3 split 128-channel, 4 split 256-channel, 5 ping-pong,
 * 6 gathered wide f16x3), or -1 if none; *launches (may be NULL) = how many such launches since the last reset.
 * cin < 0 resets the table. Host-side bookkeeping only (under hipGraph capture: recorded at capture time). */
int p2pb_debug_pointwise_form(int cin, int cout, int npos, unsigned long long *launches);

/* Voxelization.forward normalisation (models/pvcnn.py:215-228): centre on the mean, divide by
 * 2*max-norm (+eps), +0.5, *r, clamp [0,r-1]; also the half-to-even rounded int voxel coords.
 * The reference does this with torch reductions; the build fixes the summation order
 * (DESIGN.md "voxel_coords") so CPU oracle and HIP agree bit-for-bit.
 *   coords f32[b,3,n] -> norm f32[b,3,n], vox i32[b,3,n] */
int p2pb_voxel_coords(int b, int n, int r, int normalize, float eps, const float *coords, float *norm,
                      int *vox, void *stream);

/* avg_voxelize forward: replaces avg_voxelize() PN2/vox.cuh:5-6 (kernels PN2/vox_gpu.cu:18,50),
 * called from avg_voxelize_forward PN2/vox.cpp:17.
 *   coords i32[b,3,n], feat f32[b,c,n] -> ind i32[b,n], cnt i32[b,r^3], out f32[b,c,r^3]
 * Deterministic: each voxel sums its points in ascending point index (the reference's float
 * atomicAdd order is arbitrary). ws: p2pb_avg_voxelize_ws_bytes(b,n,r) bytes. */
size_t p2pb_avg_voxelize_ws_bytes(int b, int n, int r);
int p2pb_avg_voxelize_forward(int b, int c, int n, int r, const int *coords, const float *feat, int *ind,
                              int *cnt, float *out, void *ws, void *stream);
/* replaces avg_voxelize_grad() PN2/vox.cuh:7-8 (kernel PN2/vox_gpu.cu:92) */
int p2pb_avg_voxelize_backward(int b, int c, int n, int r3, const int *ind, const int *cnt,
                               const float *grad_y, float *grad_x, void *stream);

/* trilinear devoxelize: replaces trilinear_devoxelize() / _grad() PN2/trilinear_devox.cuh:5-11
 * (kernels PN2/trilinear_devox_gpu.cu:21,123). inds i32[b,8,n] / wgts f32[b,8,n] are written only
 * when is_training != 0 (may be NULL otherwise).
 *   coords f32[b,3,n] (voxel units), feat f32[b,c,r^3] -> outs f32[b,c,n] */
int p2pb_trilinear_devoxelize_forward(int b, int c, int n, int r, int is_training, const float *coords,
                                      const float *feat, int *inds, float *wgts, float *outs, void *stream);
/* grad_x f32[b,c,r^3] is zero-filled by the callee, then scatter-added (fp32 atomics) */
int p2pb_trilinear_devoxelize_backward(int b, int c, int n, int r3, const int *inds, const float *wgts,
                                       const float *grad_y, float *grad_x, void *stream);

/* ball query: replaces ball_query() PN2/pvcnn_ball_query.cuh:4-6 (kernel PN2/pvcnn_ball_query_gpu.cu:19).
 * r2 = radius*radius (float product, PN2/pvcnn_ball_query.cpp:25).
 *   centers f32[b,3,m], points f32[b,3,n] -> idx i32[b,m,u]: first u points (ascending index) with
 *   d2 < r2, remaining slots padded with the first hit; all zero when nothing is in range. */
int p2pb_ball_query(int b, int n, int m, float r2, int u, const float *centers, const float *points, int *idx,
                    void *stream);

/* grouping: replaces grouping() / grouping_grad() PN2/pvcnn_grouping.cuh:4-7
 * (kernels PN2/pvcnn_grouping_gpu.cu:18,62).  feat f32[b,c,n], idx i32[b,m,u] -> out f32[b,c,m,u] */
int p2pb_grouping_forward(int b, int c, int n, int m, int u, const float *feat, const int *idx, float *out,
                          void *stream);
int p2pb_grouping_backward(int b, int c, int n, int m, int u, const float *grad_y, const int *idx,
                           float *grad_x, void *stream);
/* the same with sample b of grad_y at grad_y + b * gy_pitch floats (gy_pitch >= c*m*u): a channel slice of a wider tensor -- one
 * part of the gradient of a concatenation (models/pvcnn.py:126) -- is read in place (build addition; training) */
int p2pb_grouping_backward_pitched(int b, int c, int n, int m, int u, const float *grad_y, long gy_pitch, const int *idx,
                                   float *grad_x, void *stream);

/* fused set-abstraction operand (BallQuery.forward, models/pvcnn.py:116-126, inference): out f32[b,3+c,m,u] =
 * [coords[:, idx] - centers (3 ch) | feat[:, idx] (c ch)] in one pass */
int p2pb_group_concat(int b, int c, int n, int m, int u, const float *coords, const float *centers,
                      const float *feat, const int *idx, float *out, void *stream);

/* gather: replaces gather_features() / _grad() PN2/pvcnn_sampling.cuh:4-7
 * (kernels PN2/pvcnn_sampling_gpu.cu:17,55).  feat f32[b,c,n], idx i32[b,m] -> out f32[b,c,m] */
int p2pb_gather_features_forward(int b, int c, int n, int m, const float *feat, const int *idx, float *out,
                                 void *stream);
int p2pb_gather_features_backward(int b, int c, int n, int m, const float *grad_y, const int *idx,
                                  float *grad_x, void *stream);

/* furthest point sampling: replaces furthest_point_sampling() PN2/pvcnn_sampling.cuh:8-9
 * (kernel PN2/pvcnn_sampling_gpu.cu:92). Starts at index 0; ties resolve exactly like the
 * reference's 512-thread block: (d desc, k mod 512 asc, k asc).
 *   coords f32[b,3,n] -> idx i32[b,m].  dist_ws f32[b,n] is scratch (running min distances),
 *   required (non-NULL) only when n > 16384; initialised by the callee. */
int p2pb_furthest_point_sampling(int b, int n, int m, const float *coords, float *dist_ws, int *idx,
                                 void *stream);

/* the same sampling for LARGE clouds (object merge, denoise_object.py:112: 3N patch points -> N; the 50000-point
 * room patches of BASELINE configs 4-5): 64 workgroups share a cloud, points and running distances stay in registers,
 * one global all-gather per round. Same indices as p2pb_furthest_point_sampling. 16384 < n <= 524288, any b (launched
 * four clouds at a time). ws: p2pb_fps_coop_ws_bytes(b, n) bytes; after the call the b ints at ws + b*1024 are
 * per-cloud flags (1 = the cooperative kernel lost a peer; the single-workgroup kernel then recomputed that cloud on
 * the device, so idx is valid either way). P2PB_EINVAL when the device cannot hold 64 workgroups at once. */
size_t p2pb_fps_coop_ws_bytes(int b, int n);
int p2pb_furthest_point_sampling_coop(int b, int n, int m, const float *coords, void *ws, int *idx, void *stream);
/* The same indices for large clouds from ONE workgroup per cloud with exact pruning (sampling.hip: a 16^3 grid over the
 * cloud; a round only revisits the cells whose bounding box is closer to the new sample than their current maximum --
 * ~n/j points in round j instead of n). Any n >= 1; ws: p2pb_fps_grid_ws_bytes(b, n) bytes, 16-byte aligned. */
size_t p2pb_fps_grid_ws_bytes(int b, int n);
int p2pb_furthest_point_sampling_grid(int b, int n, int m, const float *coords, void *ws, int *idx, void *stream);

/* point <-> triangle-mesh squared distances (P2M metric): replace pytorch3d._C.point_face_dist_forward /
 * face_point_dist_forward as called by metrics/p2m.py:66,131 for one (mesh, cloud) pair. points f32[np,3],
 * tris f32[nt,3,3] (faces as vertex triples); triangles of area < min_triangle_area count as their edges.
 *   p2pb_point_face_dist -> dist f32[np], idx i32[np] (closest triangle of every point, first minimum)
 *   p2pb_face_point_dist -> dist f32[nt], idx i32[nt] (closest point of every triangle) */
int p2pb_point_face_dist(int np, int nt, const float *points, const float *tris, float min_triangle_area, float *dist,
                         int *idx, void *stream);
int p2pb_face_point_dist(int np, int nt, const float *points, const float *tris, float min_triangle_area, float *dist,
                         int *idx, void *stream);

/* exact K nearest neighbours with patch-sized K: replaces pytorch3d.ops.knn_points(seeds, cloud, K, return_nn=True)
 * as called by denoise_object.py:91 (pytorch3d: pip dependency, not vendored; contract = the K smallest squared
 * distances per query, ascending, with indices). Ties: ascending point index.
 *   query f32[b,s,3], points f32[b,n,3] (point-major) -> dist2 f32[b,s,k], idx i32[b,s,k], nn f32[b,s,k,3]
 *   (any output may be NULL); 1 <= k <= min(n, 4096); ws: p2pb_knn_points_ws_bytes(b,s,n) bytes of scratch. */
size_t p2pb_knn_points_ws_bytes(int b, int s, int n);
int p2pb_knn_points(int b, int s, int n, int k, const float *query, const float *points, float *dist2, int *idx,
                    float *nn, void *ws, void *stream);

/* 3-NN inverse-squared-distance interpolation: replaces three_nearest_neighbors_interpolate() /
 * _grad() PN2/pvcnn_neighbor_interpolate.cuh:4-14 (kernels PN2/pvcnn_neighbor_interpolate_gpu.cu:20,96,154).
 *   points f32[b,3,n], centers f32[b,3,m], cfeat f32[b,c,m] -> idx i32[b,3,n], w f32[b,3,n], out f32[b,c,n] */
int p2pb_three_nn_interpolate_forward(int b, int c, int m, int n, const float *points, const float *centers,
                                      const float *cfeat, int *idx, float *w, float *out, void *stream);
/* the same op in two launches (search: coordinates only; interpolation: features), for callers that
 * overlap the geometry pipeline with the feature path */
int p2pb_three_nn(int b, int m, int n, const float *points, const float *centers, int *idx, float *w, void *stream);
int p2pb_three_interpolate(int b, int c, int m, int n, const float *cfeat, const int *idx, const float *w,
                           float *out, void *stream);
/* p2pb_three_nn through a uniform 16^3 grid over the centres (exact: same idx / w, ties by ascending index);
 * m >= 3 (the centre records sit in LDS up to 8192 centres and stay in global memory / L2 above), ws:
 * p2pb_three_nn_cells_ws_bytes(b, m) bytes of scratch (16-byte aligned) */
size_t p2pb_three_nn_cells_ws_bytes(int b, int m);
int p2pb_three_nn_cells(int b, int m, int n, const float *points, const float *centers, int *idx, float *w, void *ws,
                        void *stream);
int p2pb_three_nn_interpolate_backward(int b, int c, int n, int m, const float *grad_y, const int *idx,
                                       const float *w, float *grad_x, void *stream);
/* (gy_pitch >= c*n: as p2pb_grouping_backward_pitched; the slice of models/pvcnn.py:219's concatenation) */
int p2pb_three_nn_interpolate_backward_pitched(int b, int c, int n, int m, const float *grad_y, long gy_pitch, const int *idx,
                                               const float *w, float *grad_x, void *stream);

/* ---- the classic PointNet++ operators of the same extension (csrc/ball_query.hip, three_nn.hip; FPS: fps_ref.hip) ----
 * Replace the launchers behind ball_query_wrapper, three_nn_wrapper, furthest_point_sampling_wrapper,
 * three_interpolate_wrapper and three_interpolate_grad_wrapper (PN2/pointnet2_api.cpp:17-29; kernels PN2/ball_query_gpu.cu:15,
 * interpolate_gpu.cu:16,84,127, sampling_gpu.cu:101). Clouds are POINT-major f32[b,n,3], features channel-major; argument
 * order is the reference launchers'. THE CALLER ALLOCATES AND INITIALISES EVERY OUTPUT, as the reference's layers do
 * (third_party/openpoints/models/layers/{group,subsample,upsampling}.py). Squared distances: fma(dz,dz, fma(dy,dy, dx*dx)).
 * (group_points* / gather_points* of that list are p2pb_grouping_* / p2pb_gather_features_* above.)
 *
 * p2pb_pn2_ball_query: new_xyz f32[b,m,3], xyz f32[b,n,3] -> idx i32[b,m,nsample]: the first nsample points k (ascending)
 *   with d2 < radius*radius (float product, strict); the first hit fills every slot, later hits overwrite slots 1, 2, ...
 *   A centre with no neighbour LEAVES ITS ROW UNTOUCHED (the layer zero-fills idx before the call).
 * p2pb_pn2_three_nn: unknown f32[b,n,3], known f32[b,m,3] -> dist2 f32[b,n,3] (SQUARED distances, ascending), idx i32[b,n,3];
 *   strict '<' in ascending k (equal distances: lower index first); for m < 3 the unfilled slots are idx 0, dist2 +inf.
 * p2pb_pn2_fps: xyz f32[b,n,3], temp f32[b,n] IN/OUT (running minima; the layer fills it with 1e10) -> idx i32[b,m].
 *   idx[:,0] = 0; round j = 1..m-1 does temp[k] = min(temp[k], d2(k, idx[j-1])) and picks the maximum of temp in the order
 *   (temp desc, k mod T asc, k asc), T = min(2^floor(log2 n), 1024): the reference's block size and lower-thread-wins tree
 *   (1024, not the 512 of p2pb_furthest_point_sampling). On return temp holds the minima over samples 0..m-2. m == 0 writes
 *   nothing. Any n (n <= 16384: registers; above: temp is the working array, one workgroup streaming the cloud).
 * p2pb_pn2_three_interpolate: features f32[b,c,m], idx i32[b,n,3], weight f32[b,n,3] -> out f32[b,c,n] =
 *   fma(f[idx2], w2, fma(f[idx1], w1, f[idx0] * w0)).
 * p2pb_pn2_three_interpolate_grad: grad_out f32[b,c,n] -> grad_features f32[b,c,m] += grad_out * w_k at idx_k (fp32 global
 *   atomics; ACCUMULATES, the layer passes zeros). Refused (P2PB_EINVAL) in deterministic mode: the order is not fixed. */
int p2pb_pn2_ball_query(int b, int n, int m, float radius, int nsample, const float *new_xyz, const float *xyz, int *idx,
                        void *stream);
int p2pb_pn2_three_nn(int b, int n, int m, const float *unknown, const float *known, float *dist2, int *idx, void *stream);
int p2pb_pn2_fps(int b, int n, int m, const float *xyz, float *temp, int *idx, void *stream);
int p2pb_pn2_three_interpolate(int b, int c, int m, int n, const float *features, const int *idx, const float *weight,
                               float *out, void *stream);
int p2pb_pn2_three_interpolate_grad(int b, int c, int n, int m, const float *grad_out, const int *idx, const float *weight,
                                    float *grad_features, void *stream);

/* ---- the packed-batch ("offset") operators of the reference's pointops extension (csrc/pointops.hip; FPS: fps_ref.hip) --
 * Replace the launchers behind third_party/openpoints/cpp/pointops/src/pointops_api.cpp:15-25 (PO = that src directory).
 * A batch is ONE packed cloud xyz f32[n,3] with cumulative ends offset i32[b]: segment s holds the points
 * [offset[s-1], offset[s]), offset[-1] = 0; queries new_xyz f32[m,3] are packed the same way by new_offset i32[b]. Features
 * are POINT-major f32[n,c]. THE CALLER ALLOCATES AND INITIALISES EVERY OUTPUT, as the reference's layer does
 * (PO/../functions/pointops.py). A size of 0 (m, c, nsample of the arithmetic kernels, ...) returns 0 without a launch; a
 * negative size or a NULL operand is P2PB_EINVAL. Squared distances: fma(dz,dz, fma(dy,dy, dx*dx)), d = query - point.
 * Segment lookup: query i belongs to the first segment s with i < new_offset[s], found by a search over b entries that ends
 * in [0, b-1] whatever the array holds (a query past new_offset[b-1] falls to the last segment); segment ends are clamped
 * to [0, n] and an end below its start is an empty segment. Offsets holding garbage therefore give no out-of-range access
 * and no index outside [0, n) (PO/knnquery/knnquery_cuda_kernel.cu:6 get_bt_idx has no such bound).
 * The kernels that CONSUME an idx trust its values, as the reference and p2pb_grouping_forward do.
 *
 * p2pb_pointops_knnquery (PO/knnquery/knnquery_cuda_kernel.cu:65): idx i32[m,nsample], dist2 f32[m,nsample] = the nsample
 *   smallest squared distances of the query's segment, ascending, with GLOBAL point indices. EQUAL DISTANCES: ASCENDING POINT
 *   INDEX (a deliberate deviation: the reference's order among equals is whatever its heap leaves). Slots start as
 *   (1e10, segment start) and admission is strict '<', so a segment with fewer than nsample points leaves its trailing slots
 *   at dist2 = 1e10, idx = segment start (min(start, n-1) for an empty segment at the very end), as in the reference.
 *   1 <= nsample <= 100, else P2PB_EINVAL (the reference overruns its 100-entry arrays above that).
 * p2pb_pointops_ballquery (PO/ballquery/ballquery_cuda_kernel.cu:26): idx i32[m,nsample] = the first nsample points of the
 *   segment in ascending index with d2 < radius*radius (float product, strict); the first hit fills every slot, later hits
 *   overwrite slots 1, 2, ... A QUERY WITHOUT A HIT LEAVES ITS ROW UNTOUCHED (p2pb_pn2_ball_query's contract, with segments
 *   and global indices). nsample >= 1.
 * p2pb_pointops_furthestsampling (PO/sampling/sampling_cuda_kernel.cu:15): tmp f32[n] IN/OUT (running minima by GLOBAL point
 *   index; the layer fills it with 1e10) -> idx i32[m], m = new_offset[b-1] (passed so that the kernel holds to the buffer:
 *   sample ranges are clamped to [0, m]). Per segment idx[start_m] = start_n; each later sample does
 *   tmp[k] = min(tmp[k], d2(k, last)) over the segment and takes the maximum of tmp in the order (tmp desc,
 *   (k - start_n) mod T asc, k asc), T = min(2^floor(log2 n_max), 1024): the reference's block size (PO/cuda_utils.h:11-15)
 *   and its lower-thread-wins tree. T COMES FROM n_max, THE LONGEST SEGMENT, AND IS THE SAME FOR EVERY SEGMENT. A segment with
 *   no samples, or with no points, writes nothing (the reference writes idx[start_m] even then); one that asks for more
 *   samples than it has points repeats indices. One workgroup per segment: minima in registers for segments up to 16384
 *   points (and up to what n_max announced), else tmp itself is the working array.
 * p2pb_pointops_grouping_forward (PO/grouping/grouping_cuda_kernel.cu:27): output f32[m,nsample,c] = input f32[n,c] at idx.
 * p2pb_pointops_grouping_backward (:34): grad_input f32[n,c] += grad_output f32[m,nsample,c] at idx.
 * p2pb_pointops_interpolation_forward (PO/interpolation/interpolation_cuda_kernel.cu:35): input f32[m,c], idx i32[n,k],
 *   weight f32[n,k]: acc = output[.]; for i < k: acc = fma(input[idx_i], w_i, acc); output f32[n,c] = acc -- it ADDS TO WHAT
 *   THE CALLER PASSED (the reference's +=; the layer passes zeros).
 * p2pb_pointops_interpolation_backward (:42): grad_input f32[m,c] at idx_i += grad_output * w_i.
 * p2pb_pointops_subtraction_forward (PO/subtraction/subtraction_cuda_kernel.cu:32): output f32[n,nsample,c] =
 *   input1[n] - input2[idx] (written).
 * p2pb_pointops_subtraction_backward (:39): grad_input1[n] += grad_output[n,s] for s ascending (a row sum, no atomics);
 *   grad_input2[idx] += -grad_output.
 * p2pb_pointops_aggregation_forward (PO/aggregation/aggregation_cuda_kernel.cu:41): acc = output[.]; for s ascending:
 *   acc = fma(input[idx_s, ch] + position[n,s,ch], weight[n,s, ch mod w_c], acc); output f32[n,c] = acc. c % w_c == 0, else
 *   P2PB_EINVAL.
 * p2pb_pointops_aggregation_backward (:48): grad_input[idx_s, ch] += g w; grad_position[n,s,ch] = g w (WRITTEN);
 *   grad_weight[n,s,j] += g (input + position) over the channels ch = j (mod w_c) in ascending ch (one thread per (n,s,j),
 *   no atomics).
 * The four scatter-adds (grad_input of grouping, interpolation and aggregation, grad_input2 of subtraction) are fp32 global
 * atomics in no fixed order: in deterministic mode (p2pb_set_deterministic) those four entry points return P2PB_EINVAL
 * before anything is launched, like p2pb_pn2_three_interpolate_grad. subtraction_backward and aggregation_backward accept
 * NULL for that one target and then run only their fixed-order parts, in either mode. */
int p2pb_pointops_knnquery(int b, int n, int m, int nsample, const float *xyz, const float *new_xyz, const int *offset,
                           const int *new_offset, int *idx, float *dist2, void *stream);
int p2pb_pointops_ballquery(int b, int n, int m, float radius, int nsample, const float *xyz, const float *new_xyz,
                            const int *offset, const int *new_offset, int *idx, void *stream);
int p2pb_pointops_furthestsampling(int b, int n, int m, int n_max, const float *xyz, const int *offset, const int *new_offset,
                                   float *tmp, int *idx, void *stream);
int p2pb_pointops_grouping_forward(int m, int nsample, int c, const float *input, const int *idx, float *output, void *stream);
int p2pb_pointops_grouping_backward(int n, int m, int nsample, int c, const float *grad_output, const int *idx,
                                    float *grad_input, void *stream);
int p2pb_pointops_interpolation_forward(int n, int c, int k, const float *input, const int *idx, const float *weight,
                                        float *output, void *stream);
int p2pb_pointops_interpolation_backward(int n, int c, int k, const float *grad_output, const int *idx, const float *weight,
                                         float *grad_input, void *stream);
int p2pb_pointops_subtraction_forward(int n, int nsample, int c, const float *input1, const float *input2, const int *idx,
                                      float *output, void *stream);
int p2pb_pointops_subtraction_backward(int n, int nsample, int c, const int *idx, const float *grad_output, float *grad_input1,
                                       float *grad_input2, void *stream);
int p2pb_pointops_aggregation_forward(int n, int nsample, int c, int w_c, const float *input, const float *position,
                                      const float *weight, const int *idx, float *output, void *stream);
int p2pb_pointops_aggregation_backward(int n, int nsample, int c, int w_c, const float *input, const float *position,
                                       const float *weight, const int *idx, const float *grad_output, float *grad_input,
                                       float *grad_position, float *grad_weight, void *stream);

/* chamfer_3D: replaces chamfer_cuda_forward/backward (metrics/chamfer3D/chamfer3D.cu:135,176;
 * kernels :12,:155). xyz are POINT-major f32[b,n,3] / f32[b,m,3]. Lowest index wins distance ties.
 * backward ACCUMULATES into gradxyz1/2 (caller zero-fills, metrics/chamfer3D/dist_chamfer_3D.py:77-83). */
int p2pb_chamfer_forward(int b, int n, int m, const float *xyz1, const float *xyz2, float *dist1, float *dist2,
                         int *idx1, int *idx2, void *stream);
/* the same with scratch (p2pb_chamfer_ws_bytes(b, n, m) bytes): small batches split the target cloud over more
 * workgroups and combine through 64-bit atomicMin keys (distance bits, index) -- identical results */
size_t p2pb_chamfer_ws_bytes(int b, int n, int m);
int p2pb_chamfer_forward_ws(int b, int n, int m, const float *xyz1, const float *xyz2, float *dist1, float *dist2,
                            int *idx1, int *idx2, void *ws, void *stream);
int p2pb_chamfer_backward(int b, int n, int m, const float *xyz1, const float *xyz2, float *gradxyz1,
                          float *gradxyz2, const float *graddist1, const float *graddist2, const int *idx1,
                          const int *idx2, void *stream);

/* PyTorchEMD: replaces ApproxMatchForward / MatchCostForward / MatchCostBackward
 * (metrics/PyTorchEMD/cuda/emd_kernel.cu:177,264,377; kernels :33,:211,:300,:347).
 *   xyz1 f32[b,n,3], xyz2 f32[b,m,3] -> match f32[b,m,n]; temp = the reference's scratch, 2(n+m) floats per cloud
 *   (emd_kernel.cu:34). p2pb_approxmatch_temp_floats(b,n,m) = that plus the partial sums of the chunked launches the _ws
 *   entry point uses when the batch alone cannot fill the chip */
size_t p2pb_approxmatch_temp_floats(int b, int n, int m);
int p2pb_approxmatch_forward(int b, int n, int m, const float *xyz1, const float *xyz2, float *match,
                             float *temp, void *stream);
/* explicit scratch size: temp_floats >= p2pb_approxmatch_temp_floats() enables the chunked kernels (small batches of large
 * clouds); the plain entry point above keeps the reference's contract (temp = 2 (n + m) b floats, emd_kernel.cu:34) */
int p2pb_approxmatch_forward_ws(int b, int n, int m, const float *xyz1, const float *xyz2, float *match, float *temp,
                                size_t temp_floats, void *stream);
int p2pb_matchcost_forward(int b, int n, int m, const float *xyz1, const float *xyz2, const float *match,
                           float *cost, void *stream);
int p2pb_matchcost_backward(int b, int n, int m, const float *grad_cost, const float *xyz1, const float *xyz2,
                            const float *match, float *grad1, float *grad2, void *stream);

/* emd_assignment (auction): replaces emd_cuda_forward / emd_cuda_backward
 * (metrics/emd_assignment/emd_assignment/emd_cuda.cu:228,305; kernels :23-226,:284). Buffers as
 * allocated by emd_module.py:43-54; assignment/assignment_inv must be -1-filled, price and
 * max_increments zero-filled by the caller, as the reference's Python does.
 * Returns 1 on success (the reference's convention), -1 on n != m / n % 128 / b > 512 (:236-249).
 * A round is Bid (one wave per unassigned bidder) / GetMax / Assign; the first ten rounds are three launches each, the
 * latency-bound rest is ONE launch (one workgroup per cloud, n <= 8192; csrc/emd.hip auction_persist_kernel). The assignment is
 * schedule dependent in the reference as well (racing atomicMax / Assign): the contract is the invariants + transport cost. */
int p2pb_auction_forward(int b, int n, int m, const float *xyz1, const float *xyz2, float *dist, int *assignment,
                         float *price, int *assignment_inv, int *bid, float *bid_increments,
                         float *max_increments, int *unass_idx, int *unass_cnt, int *unass_cnt_sum, int *cnt_tmp,
                         int *max_idx, float eps, int iters, void *stream);
int p2pb_auction_backward(int b, int n, const float *xyz1, const float *xyz2, float *gradxyz,
                          const float *graddist, const int *idx, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Fused voxel-branch kernels. These have no counterpart in the reference's extension modules: they
 * replace the torch.nn / cuDNN calls between avg_voxelize and trilinear_devoxelize inside PVConv
 * (models/pvcnn.py:265-286,318-324: Conv3d, AdaGN, Swish, Conv3d, AdaGN, SE3d) for inference.
 * ------------------------------------------------------------------------------------------- */

/* 3x3x3, stride 1, pad 1 convolution (nn.Conv3d of models/pvcnn.py:266-282) on the fp32 matrix cores.
 * Weights are pre-packed once: w f32[cout,cin,3,3,3] -> wt_packed f32[p2pb_conv3d_k3_packed_floats()]. */
size_t p2pb_conv3d_k3_packed_floats(int cout, int cin);
int p2pb_conv3d_k3_pack_weights(int cout, int cin, const float *w, float *wt_packed, void *stream);
/* The split pack: every weight as 16-bit terms for the split-operand form of the same convolution, in the arithmetic
 * selected by p2pb_set_split_terms WHEN THE PACK IS MADE -- 16: an fp16 pair of w * S_w (S_w = the power of two that
 * brings max |w| into [2^13, 2^14), found on the device; 1 / (4 S_w) is stored behind the pack), three MFMA products per
 * fp32 product; 6: three bf16 terms, six products, dropped terms < 2^-26 |x*w|. fp32 accumulate either way
 * (conv3d.hip). Selected by flags bit 2 below. */
size_t p2pb_conv3d_k3_split_packed_bytes(int cout, int cin);
int p2pb_conv3d_k3_pack_weights_split(int cout, int cin, const float *w, void *wt_split, void *stream);
/* out[b,cout,r,r,r] = conv(xf(in[b,cin,r,r,r])) + bias;  xf(x) = x when in_scale == NULL, else
 * x*in_scale[b,ci] + in_shift[b,ci] followed by Swish when in_swish != 0 (the preceding AdaGN+Swish,
 * folded). stats_part (optional, f32[p2pb_conv3d_k3_stats_floats()]) receives per-(b, slot, cout)
 * {sum, sum of squares} of the output for the GroupNorm that follows. r in {4,8,16,32}. */
size_t p2pb_conv3d_k3_stats_floats(int b, int cout, int r);
int p2pb_conv3d_k3_forward(int b, int cin, int cout, int r, const float *in, const float *wt_packed,
                           const float *bias, const float *in_scale, const float *in_shift, int in_swish,
                           float *out, float *stats_part, void *stream);

/* Sparse-aware form (exact): in_sub f32[b,cin] is subtracted from the transformed operand, out_class
 * f32[b,27,cout] replaces bias per boundary class (low / interior / high along d,h,w) -- see conv3d.hip:
 * conv(x) = conv(x - a) + conv(a). flags bit 0: skip all-zero operand tiles; bit 1: compact 4x8x8 bricks;
 * bit 2: wt_packed is the split pack (bf16x6 arithmetic), else the fp32 pack (exact-fp32 MFMA);
 * bit 3: voxel-major grids, in f32[b,r,r,r,cin] / out f32[b,r,r,r,cout] (the fused voxel branch's layout: a
 * voxel's channels are contiguous for the staging loads, the stores, voxelize and devoxelize). */
int p2pb_conv3d_k3_forward_ex(int b, int cin, int cout, int r, const float *in, const void *wt_packed,
                              const float *bias, const float *out_class, const float *in_scale,
                              const float *in_shift, int in_swish, const float *in_sub, int flags, float *out,
                              float *stats_part, void *stream);
/* List-driven sparse form. p2pb_conv3d_brick_lists derives, from the voxel occupancy cnt i32[b,r^3] of
 * avg_voxelize, the compacted lists of (sample*NBRICK + brick) with / without MFMA work for the first
 * (halo 1) and second (halo 2) convolution of a PVConv: lists i32[4][b*NBRICK] = {active0, inactive0,
 * active1, inactive1}, counts i32[4]; flags_ws = b*NBRICK*2 bytes scratch; NBRICK = 128 (r=32) / 16 (r=16).
 * p2pb_conv3d_k3_forward_sparse runs the MFMA kernel on the active pairs only and writes the (exactly
 * known) constants + statistics of the inactive bricks. flags bit 5 (32): the inactive bricks' STATISTICS only -- their
 * outputs are left unwritten, for a caller that reads `out` inside the active bricks alone (a PVConv's second
 * convolution: the devoxelisation's corners lie within one voxel of an occupied voxel). */
int p2pb_conv3d_brick_lists(int b, int r, const int *cnt, unsigned char *flags_ws, int *lists, int *counts,
                            void *stream);
int p2pb_conv3d_k3_forward_sparse(int b, int cin, int cout, int r, const float *in, const void *wt_packed,
                                  const float *bias, const float *out_class, const float *in_scale,
                                  const float *in_shift, int in_swish, const float *in_sub, int flags /* bits 2, 3, 4, 5 */,
                                  const int *active_list, const int *active_count, const int *inactive_list,
                                  const int *inactive_count, float *out, float *stats_part, void *stream);
/* Compact form (voxel-level sparsity inside the bricks; conv3d.hip). p2pb_conv3d_active_lists derives, from the voxel
 * occupancy cnt i32[b,r^3], per (sample, 4x8x8 brick) the sorted local ids of the voxels in D1 = dilate(occupied,1)
 * (set 0) and D2 = dilate(D1,1) (set 1), followed by the ids outside the set: lists u8[2][b][NBRICK][256], counts
 * i32[2][b][NBRICK]; r in {8,16,32}. p2pb_conv3d_k3_forward_compact computes only the listed outputs of every brick
 * (a first convolution with set 0; a second one in far-field form -- in_sub / out_class -- with set 1) and writes the
 * known constants (+ their exact statistics) elsewhere. Voxel-major tensors, split weight pack. flags bit 5 (32, as in
 * p2pb_conv3d_k3_forward_sparse; ABI 6): the constants of the UNLISTED voxels are left unwritten (statistics still exact) --
 * for a caller that reads `out` at listed voxels alone (a PVConv's second convolution: read by the devoxelisation only). */
int p2pb_conv3d_active_lists(int b, int r, const int *cnt, unsigned char *lists, int *counts, void *stream);
int p2pb_conv3d_k3_forward_compact(int b, int cin, int cout, int r, const float *in, const void *wt_split,
                                   const float *bias, const float *out_class, const float *in_scale,
                                   const float *in_shift, int in_swish, const float *in_sub,
                                   const unsigned char *alist, const int *acount, float *out, float *stats_part,
                                   int flags /* bit 5 */, void *stream);
/* Pre-split operand grids ("S format", round 3; conv3d.hip PreStage). The split kernels' staging phase -- load, folded
 * norm + Swish, fp16-pair split, LDS write, repeated for every brick halo and channel block that touches a voxel -- can be
 * done ONCE per element by the operand's producer: S = u32x4[b][r^3][ceil(cin/16)][2 planes][2 khalf], 8 fp16 per entry
 * (h0 | h1 of 4 x value), 4 bytes per (voxel, channel) with the channels zero-padded to a multiple of 16. The f16x3
 * kernels then stage with LDS-DMA alone. Bit-identical outputs. Producers: p2pb_avg_voxelize_cl_gather_split (a first
 * convolution's operand straight from the voxeliser) and p2pb_conv3d_presplit (y f32[b,nvox,c] voxel-major -> S, applying
 * swish?(y*in_scale + in_shift) - in_sub; in_scale == NULL: the plain split). Consumers: p2pb_conv3d_k3_forward_ex /
 * _sparse with flags bit 4 (16; needs bits 2 and 3, no in_scale / in_sub) and
 * p2pb_conv3d_k3_forward_compact_pre. f16x3 arithmetic only (P2PB_EINVAL under bf16x6). */
int p2pb_conv3d_presplit(int b, int c, long nvox, const float *y, const float *in_scale, const float *in_shift,
                         int in_swish, const float *in_sub, void *out_split, void *stream);
int p2pb_conv3d_k3_forward_compact_pre(int b, int cin, int cout, int r, const void *in_split, const void *wt_split,
                                       const float *bias, const float *out_class, const unsigned char *alist,
                                       const int *acount, float *out, float *stats_part, int flags /* bit 5 */,
                                       void *stream);
/* a[b,cin] = xf(prev_bias[cin]) (the operand's far-field constant) and k_out[b,27,cout] = conv(a) + bias per
 * boundary class, for p2pb_conv3d_k3_forward_ex */
int p2pb_conv3d_k3_far_field(int b, int cin, int cout, const float *prev_bias, const float *in_scale,
                             const float *in_shift, int in_swish, const float *wt_packed, const float *bias,
                             float *a, float *k_out, float *tap_ws /* f32[b,27,cout] scratch */, void *stream);
/* The same with the GroupNorm(+AdaGN) BETWEEN the two convolutions of a PVConv (models/pvcnn.py:267-268, modules.py:341-358)
 * folded into the launch: part f32[b,nslots,cin,2] = the first convolution's statistics partials and the norm's parameters as
 * in p2pb_gn_affine_params; scale / shift f32[b,cin] are OUTPUTS (the values and bits p2pb_gn_affine_params writes) for the
 * kernels that stage the second convolution's operand. One launch instead of two on the sampler's dependent chain. */
int p2pb_conv3d_k3_far_field_gn(int b, int cin, int cout, const float *prev_bias, const float *part, int nslots,
                                double count_per_channel, int groups, const float *gamma, const float *beta,
                                const float *style, int style_stride, float eps, int in_swish, const float *wt_packed,
                                const float *bias, float *scale, float *shift, float *a, float *k_out, float *tap_ws,
                                void *stream);

/* GroupNorm (+AdaGN style, models/modules.py:341-358) folded into a per-(sample, channel) affine:
 * AdaGN(GN(x)) == x*scale + shift. part f32[b,nslots,c,2] partial {sum,sumsq}; gamma/beta f32[c] or
 * NULL; style = b rows of (factor[c] | bias[c]) with a row pitch of style_stride floats, or NULL; chmean
 * (optional) = per-channel mean of the transformed output (SE3d squeeze, models/modules.py:377-378). */
int p2pb_gn_affine_params(int b, int c, int groups, int nslots, double count_per_channel, const float *part,
                          const float *gamma, const float *beta, const float *style, int style_stride, float eps,
                          float *scale, float *shift, float *chmean, void *stream);
/* the same, additionally returning the group moments mean_rstd f32[b,groups,2] = {mean, 1/sqrt(var+eps)} (may be NULL)
 * for the training backward pass (p2pb_norm_act_backward) */
int p2pb_gn_affine_params_ex(int b, int c, int groups, int nslots, double count_per_channel, const float *part,
                             const float *gamma, const float *beta, const float *style, int style_stride, float eps,
                             float *scale, float *shift, float *chmean, float *mean_rstd, void *stream);
/* Training backward of y = act(GroupNorm(x) * gamma + beta [* factor + bias]) (torch.nn.GroupNorm + AdaGN,
 * models/modules.py:341-358, + Swish :14-19) given the folded affine (scale, shift) and mean_rstd of the forward pass:
 * x, gy f32[b,c,npos] -> dx f32[b,c,npos], dgamma / dbeta f32[c] (NULL to skip), dstyle f32[b,2c] = (d factor | d bias)
 * (required iff style != NULL). ws: 2*b*c + 2*b*groups floats. Deterministic. */
int p2pb_norm_act_backward(int b, int c, int groups, int npos, const float *x, const float *gy, const float *scale,
                           const float *shift, const float *mean_rstd, const float *gamma, const float *beta,
                           const float *style, int style_stride, int swish, float *dx, float *dgamma, float *dbeta,
                           float *dstyle, float *ws, void *stream);
/* The same with the layer's neighbours in a training step folded in (each used to be 1-3 elementwise launches per layer):
 *   gmean f32[b,c] | NULL    gradient of the per-channel MEAN of the activation-free output (SE3d's squeeze input,
 *                            models/modules.py:377-378, which the forward pass takes from p2pb_gn_affine_params_ex's chmean):
 *                            gy_eff = gy + gmean / npos. Requires swish == 0 and drop_p == 0.
 *   drop_p, seed, salt       nn.Dropout(drop_p) behind the Swish (models/pvcnn.py:268-272): the keep mask is a counter-based hash
 *                            of (element index, seed[0], seed[1] read from DEVICE memory, salt); pass the forward pass's values.
 *   residual, rgate          the forward pass added residual f32[b,c,npos] * rgate f32[b,c] (PVConv: devoxelised grid * SE gate,
 *                            models/pvcnn.py:322-326): dres f32[b,c,npos] = gy * rgate, drgate f32[b,c] = sum_p gy * residual.
 *                            All four or none (a residual without a gate needs no kernel: its gradient is gy).
 *   gy_pitch                 floats between two samples of gy (0 = c * npos): a channel slice of a wider tensor -- one part of a
 *                            concatenation's gradient -- is read in place instead of through a contiguous copy.
 * Everything NULL / 0 = p2pb_norm_act_backward (same bits). */
int p2pb_norm_act_backward_ex(int b, int c, int groups, int npos, const float *x, const float *gy, const float *scale,
                              const float *shift, const float *mean_rstd, const float *gamma, const float *beta,
                              const float *style, int style_stride, int swish, long gy_pitch, const float *gmean,
                              const float *residual, const float *rgate, float drop_p, const unsigned *seed, unsigned salt, float *dx, float *dgamma,
                              float *dbeta, float *dstyle, float *dres, float *drgate, float *ws, void *stream);
/* Forward of the folded norm in train(): y = drop(act(x * scale[b,c] + shift[b,c])) + residual * rgate[b,c]; residual, rgate
 * NULL = none (rgate alone is ignored), drop_p == 0 = no dropout (then p2pb_affine_act's bits). seed: two 32-bit words in
 * DEVICE memory (drawn once per forward pass by the host framework's generator, so that a captured step replays with fresh
 * masks), salt: a per-layer constant. */
int p2pb_affine_act_train(int b, int c, int npos, const float *x, const float *scale, const float *shift, int swish,
                          const float *residual, const float *rgate, float drop_p, const unsigned *seed, unsigned salt,
                          float *y, void *stream);
/* SE3d gate (models/modules.py:362-378) folded into the devoxelisation affine: gate = sigmoid(w2 relu(w1 chmean)),
 * aff_a = scale*gate, aff_b = shift*gate. w1 f32[hidden,c], w2 f32[c,hidden] (nn.Linear layouts, no bias). */
int p2pb_se_gate_affine(int b, int c, int hidden, const float *chmean, const float *w1, const float *w2,
                        const float *scale, const float *shift, float *aff_a, float *aff_b, void *stream);
/* The tail of a PVConv's voxel branch in one launch (models/pvcnn.py:283-286 AdaGN + SE3d behind the second Conv3d, and the
 * norm of the point branch's SharedMLP, :162-205): part2 f32[b,nslots2,c,2] + its norm (as p2pb_gn_affine_params) ->
 * aff_a, aff_b f32[b,c] = (scale, shift) x the SE3d gate (hidden == 0: no gate) -- what p2pb_gn_affine_params(..., chmean)
 * followed by p2pb_se_gate_affine returns, same bits; partp f32[b,nslotsp,cp,2] (NULL: none) + its norm -> scale_p, shift_p
 * f32[b,cp]. Three launches of the dependent chain become one. */
int p2pb_pvconv_tail(int b, int c, int hidden, const float *part2, int nslots2, double count2, int groups2,
                     const float *gamma2, const float *beta2, const float *style2, int style_stride2, float eps2,
                     const float *w1, const float *w2, float *aff_a, float *aff_b, int cp, const float *partp, int nslotsp,
                     double countp, int groupsp, const float *gammap, const float *betap, const float *stylep,
                     int style_stridep, float epsp, float *scale_p, float *shift_p, void *stream);

/* Voxel-major forms for the fused branch (grid f32[b,r,r,r,c]; conv flags bit 3): same values as
 * p2pb_avg_voxelize_forward / p2pb_trilinear_devoxelize_affine, coalesced on both sides (voxel_gather.hip, devoxelize.hip).
 * feat_t: f32[b,n,c] scratch (the point-major copy of feat); aff_a/aff_b may both be NULL. With add:
 * outs += swish(add*add_scale[b,c] + add_shift[b,c]), PVConv's point branch (models/pvcnn.py:286,325). */
int p2pb_avg_voxelize_cl_forward(int b, int c, int n, int r, const int *coords, const float *feat, int *ind, int *cnt,
                                 float *out, float *feat_t, void *ws, void *stream);
/* the same in two halves: the coordinate-only sort (run once per (level, resolution), on the geometry stream) and
 * the feature gather that consumes its cnt / ws */
int p2pb_voxel_sort(int b, int n, int r, const int *coords, int *ind, int *cnt, void *ws, void *stream);
int p2pb_avg_voxelize_cl_gather(int b, int c, int n, int r, const float *feat, const int *cnt, const void *ws,
                                float *out, float *feat_t, void *stream);
/* the same straight into the pre-split operand format of the voxel convolutions (S format above):
 * out_split = b * r^3 * ceil(c/16) * 64 bytes */
int p2pb_avg_voxelize_cl_gather_split(int b, int c, int n, int r, const float *feat, const int *cnt, const void *ws,
                                      void *out_split, float *feat_t, void *stream);
int p2pb_trilinear_devoxelize_cl_affine(int b, int c, int n, int r, const float *coords, const float *grid,
                                        const float *aff_a, const float *aff_b, const float *add /* f32[b,c,n] or NULL */,
                                        const float *add_scale, const float *add_shift, float *outs, void *stream);
/* trilinear devoxelize of feat*aff_a[b,c] + aff_b[b,c] (AdaGN + SE gate folded), inference only */
int p2pb_trilinear_devoxelize_affine(int b, int c, int n, int r, const float *coords, const float *feat,
                                     const float *aff_a, const float *aff_b, float *outs, void *stream);

/* Set abstraction with the first 1x1 convolution applied before the grouping (linear: W[xyz[idx]-centre; f[idx]]
 * = Z[:,idx] - Cx[:,centre], Z = W[xyz;f]+bias on the n points, Cx = W_xyz centre): out[b,c,j,k] = z[b,c,idx[b,j,k]]
 * - cx[b,c,j] (cx may be NULL), plus the {sum, sumsq} partials f32[p2pb_group_sub_stats_floats()] = [b,nslots,c,2] of
 * the GroupNorm that follows. Replaces grouping + concat + the (3+C)-channel GEMM of models/pvcnn.py:117-126,408. */
/* Feature propagation likewise (interpolation is linear too): out[b,c,j] = sum_k w_k cz[b,c,idx[b,k,j]] + add[b,c,j]
 * (+ bias[c]), cz = W_g g on the m coarse points, add = W_s skip + bias on the n fine ones (either may be NULL);
 * stats_part f32[p2pb_group_sub_stats_floats(b,c,n,1)]. Replaces interpolate + concat + the first GEMM of
 * models/pvcnn.py:457-461. */
int p2pb_three_interpolate_add(int b, int c, int m, int n, const float *cz, const int *idx, const float *w,
                               const float *add, const float *bias, float *out, float *stats_part,
                               float *ws /* f32[b*m*c], or NULL if cz is point-major f32[b,m,c] */, void *stream);
size_t p2pb_group_sub_stats_floats(int b, int c, int m, int u);
/* The statistics of the grouped tensor alone (two-layer set abstractions: the consuming GEMM, p2pb_pointwise_conv_pool_gather,
 * gathers its operand itself): zt f32[b,n,c], cxt f32[b,m,c] | NULL point-major, idx i32[b,m,u] ->
 * stats_part f32[b, p2pb_group_sub_stats_slots(m,u), c, 2] ({sum, sum of squares} of z[idx] - cx per slot of 128 positions). */
int p2pb_group_sub_stats_slots(int m, int u);
int p2pb_group_sub_stats(int b, int c, int n, int m, int u, const float *zt, const float *cxt, const int *idx,
                         float *stats_part, void *stream);
int p2pb_group_sub(int b, int c, int n, int m, int u, const float *z, const float *cx, const int *idx, float *out,
                   float *stats_part, float *ws /* f32[b*(n+m)*c], or NULL if z, cx are point-major */, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Fused shared point MLPs (SharedMLP models/pvcnn.py:162-205 = k=1 Conv1d/Conv2d -> AdaGN|GroupNorm ->
 * Swish, chained; set-abstraction neighbour max :414; Pnet2Stage max-pool :923,930). Inference only.
 * ------------------------------------------------------------------------------------------- */
size_t p2pb_pointwise_packed_floats(int cout, int cin);
int p2pb_pointwise_pack_weights(int cout, int cin, const float *w /* [cout][cin] */, float *wp, void *stream);
size_t p2pb_pointwise_stats_floats(int b, int cout, int npos);
/* out[b,cout,npos] = bias[cout] (+ bias_b[b,cout]) + W * xf(in[b,cin,npos]); xf / stats_part as in
 * p2pb_conv3d_k3_forward (stats_part f32[b, ceil(npos/256)*4, cout, 2]). bias, bias_b may be NULL. */
/* `flags` of p2pb_pointwise_conv_forward, p2pb_pointwise_conv_pool_forward and p2pb_pointwise_minmax_floats:
 * bit 2 (4): wp is the split pack (p2pb_pointwise_pack_weights_split, made for the arithmetic of p2pb_set_split_terms) and the GEMM
 *   runs in the split-operand form (bf16x6: three bf16 terms per fp32 operand, six MFMA products, fp32 accumulate -- see the conv3d
 *   split pack); needs npos % 4 == 0 and 16-byte aligned in/out. Meant for the matrix-bound layers (wide channel counts).
 * bit 5 (32), p2pb_pointwise_conv_forward only: point-major output, out f32[b,npos,cout] (what p2pb_group_sub /
 *   p2pb_three_interpolate_add gather whole rows from); stats_part must be NULL; needs npos % 4 == 0 and 16-byte aligned in/out.
 * bit 7 (128, with bit 2, f16x3 arithmetic, 16-byte rows): a NARROW layer (cin or cout < 128) on the split pack -- the
 *   register-tiled kernel of the fp32 pack with its products on the 16-bit matrix pipe (three MFMAs of K = 16 instead of eight
 *   exact-fp32 ones of K = 2 per 32x32x16 block); outputs, statistics and minmax in the layout of the fp32-pack form.
 * The thread arithmetic bf16x3 (p2pb_set_split_terms_thread(3)) runs bit 2 alone: no in_scale, no bit 5, no pooling. */
int p2pb_pointwise_conv_forward(int b, int cin, int cout, int npos, const float *in, const void *wp,
                                const float *bias, const float *bias_b, const float *in_scale,
                                const float *in_shift, int in_swish, int flags, float *out, float *stats_part,
                                double fin_count_per_channel, int fin_groups, const float *fin_gamma, const float *fin_beta,
                                const float *fin_style, int fin_style_stride, float fin_eps, float *fin_scale, float *fin_shift,
                                float *fin_chmean, void *stream);
/* fin_*: the GroupNorm(+AdaGN) that FOLLOWS the layer, handed to the layer's own launch (here, p2pb_pointwise_conv_pool_forward and
 * p2pb_pointwise_conv_pool_gather). fin_scale == NULL: none, the other nine are ignored. Otherwise fin_scale / fin_shift /
 * fin_chmean (f32[b, cout]; fin_chmean may be NULL) are filled in stream order exactly as
 * p2pb_gn_affine_params(b, cout, fin_groups, nslots, fin_count_per_channel, stats_part, fin_gamma, fin_beta, fin_style,
 * fin_style_stride, fin_eps, ...) called right after this launch would fill them (same bits; nslots = ceil(P / 256) * 4 with
 * P = npos, m * u for the gather form): the entry point puts the gn_affine
 * launch behind the producer (the forms that ran it in the producing kernel's last workgroup measured slower and left in
 * round 5). Replaces the reference's separate nn.GroupNorm / AdaGN pass after each 1x1 convolution (models/pvcnn.py:162-205,
 * models/modules.py:341-358). P2PB_EINVAL, before anything is launched, for stats_part == NULL, fin_shift == NULL,
 * fin_count_per_channel <= 0 or a shape p2pb_gn_affine_params refuses (cout % fin_groups != 0, cout / fin_groups > 256,
 * fin_style != NULL with fin_style_stride < 2 * cout). The arguments are all the state there is: nothing is kept between calls. */
size_t p2pb_pointwise_split_packed_bytes(int cout, int cin);
int p2pb_pointwise_pack_weights_split(int cout, int cin, const float *w /* [cout][cin] */, void *wp, void *stream);
/* The same GEMM with the max-pool that follows the layer (set abstraction: max over the pool_u = 4..64
 * neighbours, models/pvcnn.py:414; Pnet2Stage: pool_u = 0, max over all positions, :923,930) prepared in the
 * epilogue: minmax receives {min, max} of the raw output per pooling group (pool_u > 0: f32[b,cout,npos/pool_u,2];
 * pool_u == 0: per-wave partials f32[b, nslots, cout, 2], nslots from p2pb_pointwise_minmax_floats) and p2pb_minmax_act turns them into the
 * pooled activations once the norm parameters are known (the activations are quasi-convex, so the max sits at
 * the min or the max of the pre-activation). out may be NULL: the layer output is then never written.
 * Needs npos % 4 == 0 and 16-byte aligned in/out (p2pb_pointwise_pool_supported), else P2PB_EINVAL. */
int p2pb_pointwise_pool_supported(int npos, int pool_u);
size_t p2pb_pointwise_minmax_floats(int b, int cout, int npos, int pool_u, int flags);
int p2pb_pointwise_conv_pool_forward(int b, int cin, int cout, int npos, const float *in, const void *wp,
                                     const float *bias, const float *bias_b, const float *in_scale,
                                     const float *in_shift, int in_swish, int flags, float *out, float *stats_part,
                                     int pool_u, float *minmax, double fin_count_per_channel, int fin_groups,
                                     const float *fin_gamma, const float *fin_beta, const float *fin_style, int fin_style_stride,
                                     float fin_eps, float *fin_scale, float *fin_shift, float *fin_chmean, void *stream);
/* The same for the grouped tensor of a set abstraction WITHOUT building it: operand[ci, (mi, ui)] = zt[b, idx[b,mi,ui], ci]
 * - cxt[b, mi, ci] gathered on load from the point-major rows zt f32[b,n,cin] / cxt f32[b,m,cin] (or NULL) -- exactly what
 * p2pb_group_sub would have written as f32[b,cin,m*u] (call it with out = NULL for the statistics in_scale / in_shift are
 * folded from). Split pack, f16x3 arithmetic, cin % 8 == 0; minmax f32[b,cout,m,2]; the output itself is never stored. */
int p2pb_pointwise_conv_pool_gather(int b, int cin, int cout, int n, int m, int u, const float *zt, const float *cxt,
                                    const int *idx, const void *wp_split, const float *bias, const float *in_scale,
                                    const float *in_shift, int in_swish, float *stats_part, float *minmax,
                                    double fin_count_per_channel, int fin_groups, const float *fin_gamma, const float *fin_beta,
                                    const float *fin_style, int fin_style_stride, float fin_eps, float *fin_scale,
                                    float *fin_shift, float *fin_chmean, void *stream);
/* nn.Linear on a handful of rows (the per-evaluation Linears: AdaGN styles models/modules.py:337-345, time embedding
 * models/unet_pvc.py:108-112, the global embedding's per-sample bias models/pvcnn.py:926): out[b,co] = bias[co] + sum_ci
 * w[co,ci] x[b,ci]. x f32[b,cin] with row pitch x_stride (floats), w f32[cout,cin] with row pitch w_stride (a column slice of
 * a wider matrix is fine), bias f32[cout] or NULL, out f32[b,cout] with row pitch out_stride. cin % 4 == 0, 16-byte aligned
 * rows. No scratch memory (safe in concurrently replayed hipGraphs, unlike a BLAS call with a per-stream workspace). */
int p2pb_linear_rows(int b, int cin, int cout, const float *x, long x_stride, const float *w, long w_stride,
                     const float *bias, float *out, long out_stride, void *stream);
/* y = max(act(scale*min+shift), act(scale*max+shift)); nslots == 0: minmax f32[b,c,m,2] -> y f32[b,c,m];
 * nslots > 0: minmax f32[b,nslots,c,2] (reduced over nslots first) -> y f32[b,c] */
int p2pb_minmax_act(int b, int c, int m, int nslots, const float *minmax, const float *scale, const float *shift,
                    int swish, float *y, void *stream);
/* the global max-pool form (minmax f32[b,nslots,c,2], nslots >= 1 -> y f32[b,c]) with the GroupNorm in front of the activation
 * folded in (Pnet2Stage, models/pvcnn.py:905-932: MyGroupNorm -> Swish -> max over the points): part f32[b,nslots_st,c,2] = the
 * producing GEMM's statistics partials + the norm's parameters; scale / shift f32[b,c] are OUTPUTS (p2pb_gn_affine_params'
 * values and bits: the next GEMM applies them to the same tensor on load). c <= 4096. */
int p2pb_minmax_act_pool_gn(int b, int c, int nslots, const float *minmax, const float *part, int nslots_st,
                            double count_per_channel, int groups, const float *gamma, const float *beta, const float *style,
                            int style_stride, float eps, int swish, float *scale, float *shift, float *y, void *stream);
/* y[b,c,p] = act(x*scale[b,c] + shift[b,c]) (+ residual[b,c,p]); act = Swish when swish != 0 */
int p2pb_affine_act(int b, int c, int npos, const float *x, const float *scale, const float *shift, int swish,
                    const float *residual, float *y, void *stream);
/* y[b,c,m] = max_{k<u} act(x[b,c,m,k]*scale + shift), u a power of two <= 64; u == 0: y[b,c] = max over m */
int p2pb_affine_act_max(int b, int c, int m, int u, const float *x, const float *scale, const float *shift,
                        int swish, float *y, void *stream);

/* ---- LinearAttention core (models/modules.py:165-194: `global_att`, models/unet_pvc.py:124-125,234-244) ----
 * replaces k.softmax(-1) + the two torch.einsum calls (:186-188) between the to_qkv and to_out 1x1 convolutions
 * (which run on p2pb_pointwise_conv_forward). qkv f32[b, 3*heads*dim_head, n] in the reference's channel order
 * (q | k | v) x heads x dim_head; out f32[b, heads*dim_head, n]; dim_head must be 32 (the reference's only value).
 * ctx (optional, f32[b, heads, 32, 32]) receives softmax(k) v^T for the backward pass.
 * backward: grad_out f32[b, heads*32, n] -> grad_qkv f32[b, 3*heads*32, n]. */
int p2pb_linear_attention_forward(int b, int heads, int dim_head, int n, const float *qkv, float *out, float *ctx,
                                  void *stream);
int p2pb_linear_attention_backward(int b, int heads, int dim_head, int n, const float *qkv, const float *ctx,
                                   const float *grad_out, float *grad_qkv, void *stream);

/* Softmax attention core (models/modules.py:197-264 Attention(norm=False, flash=True): `attention_type: flash`), the part
 * between to_q / to_kv and to_out. Channel-major like everything at this boundary: q f32[b, heads*dim_head, n];
 * kv f32[b, 2*heads*dim_head, n] in channel order (k | v) x heads x dim_head; dim_head must be 32 (P2PB_EINVAL otherwise).
 *   out[b, h*32 + d, i] = sum_j softmax_j((q_i . k_j) * 32^-0.5) v[d, j]       f32[b, heads*32, n]   (no mask, no dropout)
 *   lse[b, h, i]        = log sum_j exp((q_i . k_j) * 32^-0.5)                 f32[b, heads, n]
 * lse is optional in forward (NULL when no gradient is needed) and required by backward, which recomputes the
 * probabilities from it. Any n >= 1: keys / values are streamed in tiles with a running max / sum, nothing of size n^2 is
 * stored. fp32 throughout; no atomics -- the same inputs give the same bits in both directions.
 * backward: grad_out f32[b, heads*32, n] -> grad_q (q's shape), grad_kv (kv's shape); two launches on `stream`. */
int p2pb_softmax_attention_forward(int b, int heads, int dim_head, int n, const float *q, const float *kv, float *out,
                                   float *lse, void *stream);
int p2pb_softmax_attention_backward(int b, int heads, int dim_head, int n, const float *q, const float *kv,
                                    const float *out, const float *lse, const float *grad_out, float *grad_q,
                                    float *grad_kv, void *stream);

/* ---- training: the squeeze-excite gate (csrc/normact.hip) ---------------------------------------------------------------
 * SE3d of the reference (models/modules.py:362-378): gate = sigmoid(W2 relu(W1 mean)); mean f32[b,c] = per-channel mean of the
 * voxel grid, w1 f32[hidden,c], w2 f32[c,hidden] (the two bias-free nn.Linear weights), c <= 1024, hidden <= 128.
 * forward -> hid f32[b,hidden] (post-ReLU, kept for backward), gate f32[b,c];
 * backward (dgate f32[b,c]) -> dmean f32[b,c], dw1 f32[hidden,c], dw2 f32[c,hidden]; ws: b * (c + hidden) floats.
 * Replaces the two cuBLAS GEMMs + ReLU + sigmoid and their autograd of the eager module; deterministic. */
int p2pb_se_gate_forward(int b, int c, int hidden, const float *mean, const float *w1, const float *w2, float *hid, float *gate,
                         void *stream);
int p2pb_se_gate_backward(int b, int c, int hidden, const float *mean, const float *w1, const float *w2, const float *hid,
                          const float *gate, const float *dgate, float *dmean, float *dw1, float *dw2, float *ws, void *stream);

/* Max over the last axis with its arg-max, and the backward that writes the whole input gradient (csrc/normact.hip, ABI 6):
 * the neighbour max of a set abstraction (models/pvcnn.py:414) and Pnet2Stage's global max-pools (:923,930) in train().
 *   x f32[rows,u] -> y f32[rows], idx i32[rows] (first position of the maximum; a NaN in the row is returned);
 *   gy f32[rows], idx -> gx f32[rows,u] = gy at idx, 0 elsewhere (no pre-zeroing). */
int p2pb_row_max_forward(long rows, int u, const float *x, float *y, int *idx, void *stream);
int p2pb_row_max_backward(long rows, int u, const float *gy, const int *idx, float *gx, void *stream);

/* ---- training: weight gradients of the dense layers (csrc/wgrad*.hip) -------------------------------------
 * What cuDNN / cuBLAS compute in the reference's backward pass for nn.Conv3d(k 3, pad 1) (models/pvcnn.py:265-282)
 * and the k = 1 Conv1d / Conv2d layers (models/pvcnn.py:162-205, 803-823): MFMA GEMMs over the voxel / position index
 * in the arithmetic `math` names (split bf16 operands by default), split over K with a deterministic reduction
 * (ws = scratch for the partials).
 *   x f32[b,cin,r,r,r], dy f32[b,cout,r,r,r]  ->  dw f32[cout,cin,3,3,3], db f32[cout] (db may be NULL); r in {4,8,16,32}
 *   x f32[b,cin,npos],  dy f32[b,cout,npos]   ->  dw f32[cout,cin],       db f32[cout] (db may be NULL)
 * (data gradients: p2pb_conv3d_k3_forward_ex on dy with the point-reflected, channel-swapped weight;
 *  p2pb_pointwise_conv_forward with the transposed weight)
 * math: 0 = bf16x3 split operands (default: torch's "high" float32 matmul precision, which the reference selects in
 * train.py:221; 16 significand bits, the class of its TF32 kernels), 1 = bf16x6 (fp32-faithful), 2 = exact-fp32 MFMA.
 * Size limit of the bf16 forms: they use 32-bit buffer offsets, so a convolution batch with b * max(cin, cout) * r^3 * 4 >= 2 GiB
 * runs form 2 instead (both functions below apply the same rule; nothing is refused). */
size_t p2pb_conv3d_k3_wgrad_ws_floats(int b, int cin, int cout, int r, int math);
int p2pb_conv3d_k3_wgrad(int b, int cin, int cout, int r, const float *x, const float *dy, float *dw, float *db,
                         float *ws, int math, void *stream);
/* The same weight gradient for a PVConv's FIRST convolution, whose operand x is zero outside the occupied voxels: K runs over
 * the occupied voxels only (cnt i32[b, r^3] = avg_voxelize's counts; n = points per cloud, an upper bound of their number).
 * Exact fp32 products, deterministic. ws: p2pb_conv3d_k3_wgrad_occ_ws_floats(b, cin, cout, r, n) floats. db may be NULL. */
size_t p2pb_conv3d_k3_wgrad_occ_ws_floats(int b, int cin, int cout, int r, int n);
int p2pb_conv3d_k3_wgrad_occ(int b, int cin, int cout, int r, int n, const float *x, const float *dy, const int *cnt, float *dw,
                             float *db, float *ws, void *stream);
size_t p2pb_pointwise_wgrad_ws_floats(int b, int cin, int cout, int npos, int math);
int p2pb_pointwise_wgrad(int b, int cin, int cout, int npos, const float *x, const float *dy, float *dw, float *db,
                         float *ws, int math, void *stream);

/* ---- room pipeline (denoise_room.py) ---------------------------------------------------------
 * exact radius query = sklearn.neighbors.KDTree.query_radius as used at denoise_room.py:459-464: for every patch
 * centre the indices of ALL points with |p - c|^2 <= r^2 (fp32, fma(dz,dz,fma(dy,dy,dx*dx))), ascending. Ragged, so two
 * passes: p2pb_radius_count -> counts i32[s]; the caller prefix-sums them into offsets i64[s] (exclusive) and calls
 * p2pb_radius_fill -> out i32[total]. centers f32[s,3], points f32[n,3] (point-major). */
int p2pb_radius_count(int s, int n, const float *centers, const float *points, float radius, int *counts, void *stream);
int p2pb_radius_fill(int s, int n, const float *centers, const float *points, float radius, const long long *offsets,
                     int *out, void *stream);
/* running-mean merge of overlapping patch predictions (update_prediction_noisy_batches, denoise_room.py:263-289):
 * pred f32[npatch,k,3], idx i32[npatch,k] (room point of each patch point), cuts i32[npatch] (only the first cuts[p]
 * entries of patch p count). sums f64[n,3] / counts i32[n] are accumulators zeroed by the caller once per room; any
 * number of batches add into them; p2pb_merge_finish writes sums / counts (or `original` where counts == 0). */
int p2pb_merge_accumulate(int npatch, int k, const float *pred, const int *idx, const int *cuts, double *sums,
                          int *counts, void *stream);
int p2pb_merge_finish(int n, const double *sums, const int *counts, const float *original, float *out, void *stream);

/* ---- room pipeline, batched patch construction (denoise_room.py create_patches_batched; csrc/room_patches.hip) -------
 * create_patches (denoise_room.py:352-421) for the whole room in a constant number of launches, same bits as the loop
 * of batch-1 FPS calls. points f32[n,3] (point-major), idx_flat i32[idx_len] and offsets i64[s+1] are the radius lists.
 *
 * p2pb_room_fps_jobs: `jobs` independent FPS jobs, one workgroup each. table i64[jobs,5], one row per job =
 * (list offset into idx_flat, list length L, start position in [0, L), output row in [0, rows), workspace offset in
 * floats). The job's cloud is points[idx_flat[off .. off+L)]; the result is exactly furthest point sampling of m samples
 * on that cloud with positions 0 and `start` swapped, picks mapped back (first pick = start; running minimum 1e38f;
 * fma(dz,dz,fma(dy,dy,dx*dx)); ties in the order of the reference's 512-thread block over the swapped positions).
 * picks i32[rows,m] receives POSITIONS WITHIN THE LIST (0 .. L-1), not room indices; rows no job names stay untouched.
 * All jobs of one call belong to one tier: tier t takes L <= p2pb_room_fps_tier_capacity(t), t = 0..3 keep the list in
 * registers (1024, 4096, 8192, 16384), t = 4 takes any longer list: the job gathers it once into (x, y, z, running minimum)
 * records in ws and streams those every round (ws f32[ws_floats], 16-byte aligned, p2pb_room_fps_jobs_ws_bytes(sum of
 * the streamed jobs' L) bytes; every streamed job owns 4 L floats at its workspace offset, a multiple of 4; ws may be NULL
 * for t < 4). A row that breaks any of these bounds, or a list entry outside [0, n), is passed
 * over on the device: nothing is read or written out of bounds.
 * p2pb_room_list_bounds: bounds f32[s,6] = (min x, y, z, max x, y, z) over each list's points, exact fp32.
 * p2pb_room_assemble_patches: xyz f32[npatch,k,3] and idx i64[npatch,k] (room indices) of both kinds of patch.
 * table i64[npatch,4], one row per patch = (list offset, list length L, source, kind). kind 1: an FPS patch, source =
 * its row of picks i32[rows,k]. kind 0: a padded patch (L < k): the L list points in order, then entry L+q = the list
 * position pad_r[source+q] (i64[pad_total]) moved by jitter[source+q] (f32[pad_total,3]), one fp32 add per coordinate.
 * Every launch goes on `stream`. -> 0, P2PB_EINVAL or a hipError_t code */
int p2pb_room_fps_tier_capacity(int tier);
size_t p2pb_room_fps_jobs_ws_bytes(long long stream_points);
int p2pb_room_fps_jobs(int tier, int jobs, int m, int n, const float *points, const int *idx_flat, long long idx_len,
                       const long long *table, int rows, float *ws, long long ws_floats, int *picks, void *stream);
int p2pb_room_list_bounds(int s, int n, const float *points, const int *idx_flat, long long idx_len,
                          const long long *offsets, float *bounds, void *stream);
int p2pb_room_assemble_patches(int npatch, int k, int n, const float *points, const int *idx_flat, long long idx_len,
                               const long long *table, const int *picks, int rows, const long long *pad_r,
                               const float *jitter, long long pad_total, float *xyz, long long *idx, void *stream);

/* ---- packs of the ADJOINT (data-gradient) operator, read straight from the forward layer's weight ----
 * dX of a layer is the same convolution kernel on dY with the transposed weight (and the taps point-reflected for the
 * 3x3x3 convolution). These pack variants take the FORWARD weight -- w_forward f32[cin][cout][27] resp. f32[cin][cout],
 * where cout / cin are the adjoint operator's (cout = the layer's input channels) -- and produce the pack the forward
 * kernels take; same sizes and arithmetic selection as the non-adjoint functions (p2pb_*_packed_bytes / _floats).
 * Replaces the flipped / transposed weight copies an autograd backward would make (the reference gets dX from
 * cuDNN / cuBLAS: models/pvcnn.py:265-282 Conv3d, :162-205 SharedMLP). -> 0 or P2PB_EINVAL */
int p2pb_conv3d_k3_pack_weights_split_adjoint(int cout, int cin, const float *w_forward, void *wt_split, void *stream);
int p2pb_pointwise_pack_weights_adjoint(int cout, int cin, const float *w_forward, float *wp, void *stream);
int p2pb_pointwise_pack_weights_split_adjoint(int cout, int cin, const float *w_forward, void *wp, void *stream);

/* ---- optimiser tail of a training step: clip_grad_norm_ + Adam / AdamW in three launches (csrc/optim.hip) ----
 * replaces torch.nn.utils.clip_grad_norm_(model.parameters(), clip) + torch.optim.AdamW/Adam.step() of the reference's
 * loop (train.py:127-133, models/model_loader.py:13-33); same arithmetic, per element, as torch's _single_tensor_adam.
 *   table   device array of n_tensors entries {float *param, *grad, *exp_avg, *exp_avg_sq; int64 numel}
 *           (p2pb_optim_entry_bytes() each)
 *   chunks  device int32[nchunks][2] = (tensor index, chunk index within the tensor), p2pb_optim_chunk() elements per chunk
 *   partial device f64[nchunks] scratch
 *   ctl     device f64[8]: [0] updates applied so far (in/out), [1] learning rate (in: the host writes it, so a captured
 *           graph follows a scheduler), [2] gradient norm before clipping (out), [3] clip coefficient applied (out),
 *           [4] 1.0 when this update was skipped (out), [5], [6] bias corrections (scratch)
 *   max_norm <= 0: no clipping (gradients are not rewritten). decoupled: AdamW (p *= 1 - lr wd) / Adam (g += wd p).
 *   skip_nonfinite: a non-finite gradient norm leaves parameters, moments and the step count untouched (what the
 *           GradScaler of the reference's loop does to optimizer.step()).
 *   amax    NULL, or device u32[ntensors]: bits of max |param| per tensor AFTER this update (0 for an empty / all-zero
 *           tensor) -- what p2pb_*_pack_weights_split_amax take, so that the next forward's weight packs need no reduction
 *           launch of their own
 * -> 0 or a hipError_t code */
size_t p2pb_optim_entry_bytes(void);
int p2pb_optim_chunk(void);
int p2pb_optim_clip_adam_step(int nchunks, const void *table, const int *chunks, double *partial, double *ctl, double max_norm,
                              double beta1, double beta2, double eps, double weight_decay, int decoupled, int skip_nonfinite,
                              unsigned *amax, int ntensors, void *stream);
/* p2pb_conv3d_k3_pack_weights_split / p2pb_pointwise_pack_weights_split with max |w| (float bits, device) supplied by the
 * caller instead of reduced in front of the pack: the same pack for the same value. -> 0 or P2PB_EINVAL */
int p2pb_conv3d_k3_pack_weights_split_amax(int cout, int cin, const float *w, void *wt_split, const unsigned *amax_bits,
                                           void *stream);
int p2pb_pointwise_pack_weights_split_amax(int cout, int cin, const float *w, void *wp, const unsigned *amax_bits, void *stream);

/* ---- set-against-set generative metrics (metrics/evaluation_metrics_fast.py; csrc/setmetrics.hip) ----
 * A f32[s,n,3], B f32[r,m,3] are two SETS of clouds; out f32[s,r] gets one distance per pair (A_i, B_j). The reference builds
 * such a matrix row by row from an expanded copy of one cloud (_pairwise_EMD_CD_sub :209-231, _pairwise_EMD_CD_ :262-281);
 * here pairs are indexed inside the kernels and no copy of either set is made.
 *
 * p2pb_pairwise_chamfer: out[i,j] = mean_p min_q |A_ip - B_jq|^2 + mean_q min_p |A_ip - B_jq|^2, what :219-228 assembles from
 * chamfer_3DDist_nograd (dl.mean(dim=1) + dr.mean(dim=1)). The per-point minima are the fp32 numbers of p2pb_chamfer_forward;
 * each direction's sum is taken in fp64 in a fixed order and the entry is rounded to fp32 once (run-to-run deterministic).
 * A == B with s == r, n == m is the symmetric case: each directional sum is computed once and out equals its transpose bitwise.
 * ws: p2pb_pairwise_chamfer_ws_bytes(s, r) bytes. s, r <= 65535. */
size_t p2pb_pairwise_chamfer_ws_bytes(int s, int r);
int p2pb_pairwise_chamfer(int s, int r, int n, int m, const float *A, const float *B, float *out, void *ws, void *stream);
/* p2pb_pairwise_emd: out[i,j] = earth_mover_distance_nograd(A_i, B_j) = approxmatch match cost / n (:230,
 * PyTorchEMD/emd_nograd.py:13-14,43; cuda/emd_kernel.cu:33,211). The match matrix is never stored: its cost is accumulated
 * level by level. Not symmetric in its arguments: every entry is computed. Pairs run in chunks of ws_bytes / ((3 n + 2 m) * 4)
 * (at least one pair must fit, else P2PB_EINVAL); p2pb_pairwise_emd_ws_bytes is the size past which more does not help. */
size_t p2pb_pairwise_emd_ws_bytes(int s, int r, int n, int m);
int p2pb_pairwise_emd(int s, int r, int n, int m, const float *A, const float *B, float *out, void *ws, size_t ws_bytes,
                      void *stream);
/* p2pb_occupancy_counts: the inner loop of entropy_of_occupancy_grid (:587-600). pts f32[clouds,npts,3]; every point goes to
 * its nearest centre of the resolution^3 unit-cube grid (unit_cube_grid_point_cloud :534-552; with clip_sphere only the cells
 * whose centre norm is <= 0.5, numbered in row-major order after the clip). counters i32[G] counts points, bernoulli i32[G]
 * counts clouds that touch the cell; G = p2pb_occupancy_grid_cells(resolution, clip_sphere) (host arithmetic only; < 0 for a
 * bad resolution). Integer atomics only: deterministic. 2 <= resolution <= 80, G > 0; ws: p2pb_occupancy_ws_bytes(resolution). */
int p2pb_occupancy_grid_cells(int resolution, int clip_sphere);
size_t p2pb_occupancy_ws_bytes(int resolution);
int p2pb_occupancy_counts(int clouds, int npts, int resolution, int clip_sphere, const float *pts, int *counters,
                          int *bernoulli, void *ws, void *stream);

/* image features onto a scan ----------------------------------------------------------------------------------
 * Replaces the per-point stages of process_scene, data/processing/image_features.py:329-514 (the reference runs them on the
 * host with numba, torch indexing and a KD-tree). Python side: p2p_bridge_amd/image_features.py. No float atomics anywhere:
 * the same inputs give the same bits.
 *
 * p2pb_imgfeat_visibility: project_point_cloud_batch (:114-143) + filter_points_batch_with_occlusion (:146-190) for b frames.
 *   points f64[n,3], rotation f64[b,3,3], translation f64[b,3], camera f64[b,3,3] -> valid u8[b,n] (0 / 1), xy i32[b,n,2].
 *   Projection in fp64 in this order: cam = ((r0*x + r1*y) + r2*z) + t per row, then (k0*X + k1*Y) + k2*Z per row of the
 *   camera matrix, then x = u / w, y = v / w (IEEE divides), depth = w.
 *   A point is INSIDE iff -1 < x < width, -1 < y < height and min_depth < depth < max_depth, all strict and all decided in
 *   floating point before any conversion (NaN, +-inf, w <= 0 and coordinates beyond the int range are outside); its pixel is
 *   (trunc(x), trunc(y)), truncation toward zero, so x in (-1, 0) is column 0. valid[f,i] = INSIDE and depth strictly below
 *   the smallest depth of the inside points j < i of the same pixel of frame f (the first point of a pixel is valid, an equal
 *   depth is not, a later nearer point does not revoke an earlier farther one): the records of the running minimum of each
 *   pixel in index order, the reference's fresh-per-frame depth buffer. xy[f,i] = the truncated pixel of every INSIDE point
 *   (valid or occluded), (-1, -1) for the others.
 *   ws: p2pb_imgfeat_visibility_ws_bytes(b, n, width, height) bytes, 8-byte aligned. b <= 65535, b*n and width*height < 2^31.
 *   Cost note: a pixel holding L inside points costs one wave L^2/64 steps once L > 64.
 * p2pb_imgfeat_fuse: map_image_features_to_filtered_ptc_batch_torch (:223-250) + update_features_batched_torch (:253-279),
 *   all b frames of a batch in one launch, frame f's rows paired with frame f's points. maps f16[b,hmap,wmap,c] channel-last;
 *   a valid point takes the row at [clamp(xy.y, 0, hmap-1), clamp(xy.x, 0, wmap-1)]. mean f16[n,c] and count i32[n] are
 *   updated in place, per frame 0..b-1 in order: count += 1, d = f16(f32(new) - f32(mean)), q = f16(f32(d) / f32(count)),
 *   mean = f16(f32(mean) + f32(q)). Any c >= 1 (16-byte vectors when c % 8 == 0 and maps / mean are 16-byte aligned).
 * p2pb_imgfeat_fill_round: one round of interpolate_missing_features (:282-326) as a wavefront. missing i32[m] (the points with
 *   count 0, ascending), nbr i32[m,k] (their k nearest points of the cloud, the point itself among them; k <= 32), feat
 *   f16[n,c] in place, done_round i32[n] (zeros before round 1), round >= 1, remaining i32[1] (m before round 1). A missing
 *   point i not yet done is READY iff every neighbour j < i with count 0 has 1 <= done_round[j] < round. A ready point takes
 *   the rows of its neighbours j != i with count[j] > 0, or count[j] == 0 and j < i (filled rows), drops the all-zero ones,
 *   and stores the per-channel median (mean of the two middle values in fp32 for an even number, one rounding to fp16; zeros
 *   if no row is left; NaN if a value is NaN), sets done_round[i] = round and decrements remaining. The caller launches
 *   rounds 1, 2, ... until remaining is 0; the lowest unfinished point is always ready.
 * p2pb_imgfeat_sample_grid: the value that bilinear upsampling (align_corners = false) of a coarse channel-last grid
 *   f16[b,h,w,c] to (out_h, out_w) has at pixel (clamp(xy.x, 0, out_w-1), clamp(xy.y, 0, out_h-1)), for every point (valid or
 *   not) of xy i32[b,n,2] -> out f16[b,n,c]: the full-resolution map is never built. Per axis, in fp32:
 *     src = max((dst + 0.5) * ((float)in / (float)out) - 0.5, 0), i0 = floor(src), i1 = min(i0 + 1, in - 1), l1 = src - i0,
 *     l0 = 1 - l1;   value = ly0 * (lx0*a + lx1*b) + ly1 * (lx0*c + lx1*d)
 *   with a, b the grid values at row y0, columns x0, x1 and c, d those at row y1, every written operator one fp32 operation
 *   (no contraction), the value rounded to fp16 once.
 * p2pb_imgfeat_fuse_grid: p2pb_imgfeat_fuse whose `new` row of (frame f, point i) is p2pb_imgfeat_sample_grid's row, formed in
 *   registers; one launch for the batch, mean / count updated in place under the same three roundings per frame.
 * -> 0, P2PB_EINVAL for bad sizes or NULL operands. */
size_t p2pb_imgfeat_visibility_ws_bytes(int b, int n, int width, int height);
int p2pb_imgfeat_visibility(int b, int n, const double *points, const double *rotation, const double *translation,
                            const double *camera, int width, int height, double min_depth, double max_depth,
                            unsigned char *valid, int *xy, void *ws, void *stream);
int p2pb_imgfeat_fuse(int b, int n, int c, int hmap, int wmap, const void *maps, const unsigned char *valid, const int *xy,
                      void *mean, int *count, void *stream);
int p2pb_imgfeat_fill_round(int m, int n, int c, int k, const int *missing, const int *nbr, const int *count, void *feat,
                            int *done_round, int round, int *remaining, void *stream);
int p2pb_imgfeat_sample_grid(int b, int n, int c, int h, int w, int out_h, int out_w, const void *grid, const int *xy, void *out,
                             void *stream);
int p2pb_imgfeat_fuse_grid(int b, int n, int c, int h, int w, int out_h, int out_w, const void *grid,
                           const unsigned char *valid, const int *xy, void *mean, int *count, void *stream);

/* vision transformer ----------------------------------------------------------------------------------------------
 * The forward of a DINOv2 ViT (the model behind get_dino_features, data/processing/image_features.py:88-111, which the
 * reference fetches with torch.hub). Python side: p2p_bridge_amd/dinov2.py; kernels: csrc/vit.hip. Pure additions (no ABI
 * bump, like the p2pb_scan_* entry points).
 * Layout: tokens are ROW-major, x f32[rows = B*T, C] -- a deliberate exception to the channel-major convention above: every
 * reduction of a ViT runs over C, the checkpoints' weights are [out, in], the result is read as [B, T, C], and T = 1 + h*w
 * (235 at 192 x 256) needs no padding this way. Arithmetic: fp32 operands, fp32 FMAs, fp32 results at any magnitude (not the
 * split-operand arithmetic: p2pb_set_split_terms does not reach these); sums over K and over keys are two-level (tiles of 16 /
 * 32 terms, then the tile totals). No atomics: the same inputs give the same bits. Pointers 16-byte aligned.
 * One forward is 3 + 7 * depth launches (87 for ViT-S/14): patch_embed is 2, then per block layernorm, linear (qkv),
 * attention, linear (proj, RESIDUAL), layernorm, linear (fc1, GELU), linear (fc2, RESIDUAL), then the final layernorm.
 *
 * p2pb_vit_layernorm: y[r,:] = (x[r,:] - mean) / sqrt(var + eps) * gamma + beta per row of x f32[rows,c], mean and the BIASED
 *   variance of x - mean in two passes (never E[x^2] - E[x]^2). y may not alias x.
 * p2pb_vit_linear: y f32[m,n] from x f32[m,k], w f32[n,k] (a Linear's weight as stored), bias f32[n]; n % 4 == k % 4 == 0.
 *     P2PB_VIT_EPI_BIAS      y  = x w^T + bias
 *     P2PB_VIT_EPI_GELU      y  = gelu(x w^T + bias), the exact form 0.5 v (1 + erf(v / sqrt 2))
 *     P2PB_VIT_EPI_RESIDUAL  y += gamma * (x w^T + bias), gamma f32[n] (LayerScale), y read and written in place
 * p2pb_vit_patch_embed: images f32[b,3,hp*patch,wp*patch] (already normalised), weight f32[c, 3*patch*patch] (the Conv2d
 *   weight [c,3,patch,patch] as stored), cls f32[c], pos f32[1 + hp*wp, c] (already interpolated to this grid) ->
 *   x f32[b, 1 + hp*wp, c]: x[:,0] = cls + pos[0], x[:,1 + p] = patch p (row-major over (hp, wp)) projected + bias + pos[1 + p].
 *   ws: p2pb_vit_patch_embed_ws_floats(b, hp, wp, patch) floats. patch even, c % 4 == 0, hp*wp <= 65535.
 * p2pb_vit_attention_forward: qkv f32[b, n, 3*heads*64], channel order (q | k | v) x heads x 64 -> out f32[b, n, heads*64],
 *   out[i] = sum_j softmax_j((q_i * 64^-0.5) . k_j) v_j over the keys j < n_valid, no mask, no dropout. Keys and values are
 *   streamed in tiles of 32 with a running max and sum; nothing of size n^2 exists. Rows n_valid .. n-1 are padding: they are
 *   never read (whatever they hold, NaN included, carries exactly zero weight) and their OUTPUT rows are written as zeros.
 *   1 <= n_valid <= n. (p2pb_softmax_attention_forward stays the 32-wide channel-major operator of the point networks.)
 *
 * The same forward with fp16 matrix operands (csrc/vit_f16.hip; DinoV2(precision="fp16")): the arithmetic the reference runs
 * under fp16 autocast. Only the OPERANDS of matrix products are fp16, each rounded once to nearest-even by the IEEE conversion
 * (beyond +-65504: +-inf, as torch.Tensor.half(); nothing saturates, nothing checks): products run on
 * v_mfma_f32_32x32x16_f16 with fp32 accumulators, and bias, GELU, LayerScale, the residual stream, softmax and the LayerNorm
 * statistics stay fp32. Patch embedding and the final norm use the fp32 entry points above. Same launch count, no atomics.
 * Pure additions (no ABI bump). fp16 buffers are passed as void *.
 * p2pb_vit_layernorm_f16: p2pb_vit_layernorm with y f16[rows,c]: the fp32 result rounded once (the bits of `.half()` of it).
 * p2pb_vit_linear_f16: x f16[m,k], w f16[n,k], bias f32[n]; n % 64 == 0 and k % 32 == 0 (every DINOv2 layer: C = 64 * heads),
 *   any m >= 1 (no padded row is read or written).
 *     P2PB_VIT_EPI_BIAS      y f16[m,n]  = x w^T + bias
 *     P2PB_VIT_EPI_GELU      y f16[m,n]  = gelu(x w^T + bias)
 *     P2PB_VIT_EPI_RESIDUAL  y f32[m,n] += gamma * (x w^T + bias), gamma f32[n], y read and written in place
 * p2pb_vit_attention_forward_f16: qkv f16[b, n, 3*heads*64] -> out f16[b, n, heads*64], the contract of
 *   p2pb_vit_attention_forward (keys < n_valid only, padded rows never read, padded output rows zeros). Both products on the
 *   matrix pipe; the logits, the running max and sum are fp32; the un-normalised weights exp(s - max) enter P.V rounded to
 *   fp16, the sum that divides the result is the fp32 one.
 * -> 0, P2PB_EINVAL for bad sizes, a bad epilogue, misaligned or NULL operands. */
#define P2PB_VIT_EPI_BIAS 0
#define P2PB_VIT_EPI_GELU 1
#define P2PB_VIT_EPI_RESIDUAL 2
int p2pb_vit_layernorm(int rows, int c, const float *x, const float *gamma, const float *beta, float eps, float *y, void *stream);
int p2pb_vit_linear(int m, int n, int k, const float *x, const float *w, const float *bias, int epilogue, const float *gamma,
                    float *y, void *stream);
size_t p2pb_vit_patch_embed_ws_floats(int b, int hp, int wp, int patch);
int p2pb_vit_patch_embed(int b, int hp, int wp, int patch, int c, const float *images, const float *weight, const float *bias,
                         const float *cls, const float *pos, float *ws, float *x, void *stream);
int p2pb_vit_attention_forward(int b, int heads, int n, int n_valid, const float *qkv, float *out, void *stream);
int p2pb_vit_layernorm_f16(int rows, int c, const float *x, const float *gamma, const float *beta, float eps, void *y, void *stream);
int p2pb_vit_linear_f16(int m, int n, int k, const void *x, const void *w, const float *bias, int epilogue, const float *gamma,
                        void *y, void *stream);
int p2pb_vit_attention_forward_f16(int b, int heads, int n, int n_valid, const void *qkv, void *out, void *stream);

/* scan fusion ---------------------------------------------------------------------------------------------------
 * Depth frames -> one cleaned room cloud: the GPU stages of data/scannetpp/iphone/process_dataset.py:102-283 and arkit_pcl.py
 * (the reference runs them through Open3D's CUDA tensor geometry and cuML). Python side: p2p_bridge_amd/scan_fusion.py, which
 * sorts keys, takes prefix sums and compacts with torch. No float atomics anywhere: the same inputs give the same bits.
 * Squared distances are fma(dz,dz, fma(dy,dy, dx*dx)), d = point - query, as everywhere in this header.
 *
 * p2pb_scan_depth_valid: valid u8[npix] = 1 iff min_depth <= depth <= max_depth (fp32 compares; NaN and +-inf are 0).
 * p2pb_scan_backproject: pix i64[n] (row-major pixel indices y*width + x, any subset), image u8[height,width,3], depth
 *   f32[height,width]; kinv f64[9] (the inverse intrinsic, row-major) and camera_to_world f64[>= 12] (row-major, the top three
 *   rows are read) are HOST pointers, copied before the call returns. fp64: cam = ((k0*x + k1*y) + k2) * z per row of kinv,
 *   world = ((c0*X + c1*Y) + c2*Z) + c3 per row, one rounding -> xyz f32[n,3]; rgb f32[n,3] = the bytes as floats.
 * p2pb_scan_cell_keys: keys i64[n] = (kx + 2^20) << 42 | (ky + 2^20) << 21 | (kz + 2^20), k = floor(p / cell) with an IEEE fp32
 *   divide (no origin shift; -0.001 lies in cell -1). *bad (i32, zeroed by the caller) is set to 1 when a k falls outside
 *   [-2^20, 2^20) or a coordinate is NaN; such a row's key is meaningless.
 * p2pb_scan_segment_mean: rows perm[starts[v] .. starts[v+1]) of src f32[*,c] form segment v of m (perm: the stable argsort
 *   of the keys, so each segment is in ascending row order). out f32[m,c] = (float)(fp64 sum in that order / count) for the
 *   segments of at most `small` rows, one thread per (segment, channel); longer ones are NOT written.
 * p2pb_scan_segment_mean_big: the longer ones. big i64[nbig] = their segment numbers; segment big[b] is cut into the chunks
 *   chunk_begin[b] .. chunk_begin[b+1] (chunk_begin i64[nbig+1]) of at most p2pb_scan_big_chunk_rows() rows; chunk q covers the
 *   sorted rows chunk_row0[q] .. + chunk_rows[q]. One workgroup per chunk adds it in fp64 in a fixed order into partial
 *   f64[nchunks,c]; a second kernel adds a segment's chunks in chunk order, divides and rounds once.
 * The grid of the neighbour search is the reference points sorted by p2pb_scan_cell_keys: sorted_points f32[n,3] and
 *   sorted_keys i64[n] in the same order. Cells (x, y, z0..z1) have consecutive keys: one column of cells is one run.
 * p2pb_scan_radius_count: counts[q] = min(limit, #{ j : sqdist <= r2 }), one thread per query. reach >= the largest
 *   |p - q| per axis that can pass the fp32 test (the caller adds the roundings to the radius); the cells between those of
 *   q - reach and q + reach are visited, the 27 around the query's cell when cell is the radius. Exact.
 * p2pb_scan_knn_grid: one wave per query qidx[w] (i32[nq]; NULL: query w), rings 1..max_ring (<= 16) of cells around the
 *   query's cell; a ring is final when the k-th smallest squared distance so far is no larger than the squared distance to
 *   the nearest cell not yet visited (roundings of the cell index allowed for). Then out[q] = sqrtf(k-th smallest squared
 *   distance) and unresolved[q] = 0; otherwise unresolved[q] = 1 and out[q] is not written. 1 <= k <= 64.
 * p2pb_scan_knn_brute: the same result from a walk over all n points (any order), one wave per query; k <= n.
 * -> 0, P2PB_EINVAL for bad sizes or NULL operands. */
int p2pb_scan_depth_valid(int npix, const float *depth, float min_depth, float max_depth, unsigned char *valid, void *stream);
int p2pb_scan_backproject(int n, int width, int height, const long long *pix, const unsigned char *image, const float *depth,
                          const double *kinv, const double *camera_to_world, float *xyz, float *rgb, void *stream);
int p2pb_scan_cell_keys(int n, const float *xyz, float cell, long long *keys, int *bad, void *stream);
int p2pb_scan_segment_mean(long long m, int c, int small, const float *src, const long long *perm, const long long *starts,
                           float *out, void *stream);
int p2pb_scan_big_chunk_rows(void);
int p2pb_scan_segment_mean_big(int nbig, int nchunks, int c, const float *src, const long long *perm, const long long *starts,
                               const long long *big, const long long *chunk_begin, const long long *chunk_row0,
                               const long long *chunk_rows, double *partial, float *out, void *stream);
int p2pb_scan_radius_count(int nq, int n, const float *query, const float *sorted_points, const long long *sorted_keys,
                           float cell, float r2, float reach, int limit, int *counts, void *stream);
int p2pb_scan_knn_grid(int nq, int n, int k, int max_ring, const int *qidx, const float *query, const float *sorted_points,
                       const long long *sorted_keys, float cell, float *out, unsigned char *unresolved, void *stream);
int p2pb_scan_knn_brute(int nq, int n, int k, const int *qidx, const float *query, const float *points, float *out,
                        void *stream);

/* room training pairs ---------------------------------------------------------------------------------------------
 * (noisy patch, aligned clean patch) pairs of a room: the device stages of data/preprocess_batches.py and
 * data/processing/utils.py:create_spherical_batches (the reference runs them through Open3D, cuML and a Python double loop).
 * Python side: p2p_bridge_amd/room_pairs.py. No float atomics: the same inputs give the same bits. Clean patches are RAGGED:
 * ref f32[total,3] holds them one after another, patch p is rows ref_off[p] .. ref_off[p+1] (ref_off i64[P+1], DEVICE memory).
 * The entry points that take ref_off copy it to the host and wait for the stream (they are not for stream capture): offsets
 * that are negative, decreasing or beyond `total` are P2PB_EINVAL before any kernel runs.
 *
 * p2pb_pairs_tri_areas: area f64[F] = |cross(b - a, c - a)| / 2 in fp64 of faces i32[F,3] over verts f32[V,3]; a face with a
 *   vertex index outside [0, V) has area 0 and sets *bad (i32, zeroed by the caller) to 1.
 * p2pb_pairs_sample_mesh: cdf f64[F] = the inclusive prefix sum of the areas, u f64[n,3] in [0,1). face[i] = the first f with
 *   cdf[f] > u0 * cdf[F-1] (numpy's searchsorted(cdf, u0 * total, side="right"), at most F-1: a zero-area triangle is never
 *   drawn); s = sqrt(u1), w = (1 - s, s * (1 - u2), s * u2); xyz[i] = (float)((w0*a + w1*b) + w2*c) per axis in fp64, one
 *   rounding; rgb[i] the same over vcol f32[V,3] (vcol and rgb NULL: no colours).
 * p2pb_pairs_knn: query f32[P,s,3] -> idx i32[P,s,K] (the index INSIDE the patch) and dist2 f32[P,s,K] (may be NULL): the K
 *   smallest fma(dz,dz, fma(dy,dy, dx*dx)), d = point - query, ascending, ties by ascending index -- the contract and the bits
 *   of p2pb_knn_points. 1 <= K <= 128; a patch of fewer than K points is P2PB_EINVAL. One launch, one wave per query, no
 *   scratch: the clean patch streams through LDS.
 * p2pb_pairs_unique_assign: nn i32[P,s,K] (indices inside the patch). assign[p,i], i ascending = the first entry of nn[p,i,:]
 *   that no point j < i of the patch has taken; all K taken: nn[p,i,0], and the point takes nothing. Computed in parallel
 *   (deferred acceptance on integer atomicMin, one workgroup per patch), bit-equal to that sequential rule. unique[p] = the
 *   number of points that took an entry = the number of distinct values in assign[p] (a fall-back value nn[p,i,0] is one that
 *   an earlier point took). owner i32[total] is scratch (no need to initialise it). Entries of nn outside
 *   [0, ref_off[p+1] - ref_off[p]) count as taken; a fall-back to such an entry puts a value into assign[p] that nobody took,
 *   and unique[p] does NOT count it. 1 <= K <= 128.
 * p2pb_pairs_finish: center[p] = (float)(fp64 sum of noisy[p,:,a] in index order / s); d = noisy - center in fp32; scale[p] =
 *   max_i (float)sqrt(dx*dx + dy*dy + dz*dz in fp64); noisy_out[p,i] = (d / scale, noisy_rgb[p,i]); clean_out[p,i] =
 *   ((ref[j] - center) / scale, ref_rgb[j]), j = ref_off[p] + assign[p,i] (fp32 subtract and IEEE divide; an assign outside
 *   the patch gives a row of NaN). noisy f32[P,s,3], noisy_rgb f32[P,s,3], ref_rgb f32[total,3], outputs f32[P,s,6],
 *   center f32[P,3], scale f32[P].
 * -> 0, P2PB_EINVAL for bad sizes, offsets or NULL operands. */
int p2pb_pairs_tri_areas(int nverts, int nfaces, const float *verts, const int *faces, double *area, int *bad, void *stream);
int p2pb_pairs_sample_mesh(int nverts, int nfaces, int n, const float *verts, const float *vcol, const int *faces,
                           const double *cdf, const double *u, int *face, float *xyz, float *rgb, void *stream);
int p2pb_pairs_knn(int npatch, int s, int k, int total, const float *query, const float *ref, const long long *ref_off,
                   int *idx, float *dist2, void *stream);
int p2pb_pairs_unique_assign(int npatch, int s, int k, int total, const int *nn, const long long *ref_off, int *owner,
                             int *assign, int *unique, void *stream);
int p2pb_pairs_finish(int npatch, int s, int total, const float *noisy, const float *noisy_rgb, const float *ref,
                      const float *ref_rgb, const long long *ref_off, const int *assign, float *clean_out, float *noisy_out,
                      float *center, float *scale, void *stream);

/* point-to-mesh grid ----------------------------------------------------------------------------------------------
 * The (dist, idx) of p2pb_point_face_dist / p2pb_face_point_dist, bit for bit and ties included, from an exact search over a
 * uniform grid (csrc/p2m_grid.hip; Python side: metrics.TriangleGrid; argument for the bounds: DESIGN.md, "Point-to-mesh
 * grid"). Pure additions like the p2pb_scan_* and p2pb_pairs_* entry points: P2PB_ABI_VERSION stays 13. Cells and keys are
 * those of p2pb_scan_cell_keys. tris f32[nt,3,3], points f32[np,3]; `mag` > 0 bounds every coordinate the bounds were
 * proven for, pad = mag * 2^-19 is the absolute rounding allowance.
 *
 * p2pb_p2m_grid_classify: per triangle cls u8[nt] (0: prunable, box f32[nt,6] = lo xyz, hi xyz holds every point of the
 *   region in which point_triangle_d2 can fall below the squared distance to that box times shrink[t]^2; 1: no such finite
 *   box -- a vertex that is not finite or beyond mag, an ill-conditioned or tiny triangle with the inside test enabled, an
 *   enlargement above 1e6 -- test it against everything) and shrink f32[nt] in (0, 1].
 * p2pb_p2m_grid_count: counts i32[nt] = the number of cells a prunable box overlaps if that is at most `cap`, else 0;
 *   wide u8[nt] = 1 for every triangle that gets no incidences (cls 1, over the cap, outside the key range).
 * p2pb_p2m_grid_fill: offsets i64[nt] = the exclusive prefix sum of counts; writes keys i64[total] and ids i32[total], the
 *   (cell key, triangle) incidences of triangle t at offsets[t] .. offsets[t] + counts[t].
 * p2pb_p2m_grid_point_face: keys ascending with ids permuted alike (ninc >= 0 of them), wide_ids i32[nwide] the wide
 *   triangles. One thread per point: the wide triangles, then rings 1..max_ring (<= 8) of cells around the point's cell. A
 *   ring is final when best < (shrink * (rho cells less rounding less pad))^2 less a margin; then dist / idx are written and
 *   unresolved[i] = 0. Otherwise (ring limit, a point that is not finite or beyond mag) unresolved[i] = 1 and dist / idx are
 *   left alone.
 * p2pb_p2m_grid_face_point: sorted_points f32[ns,3] ascending by sorted_keys, order i32[ns] their indices in the caller's
 *   cloud, extra f32[nextra,3] / extra_idx i32[nextra] the points that are not in the grid (tested by every triangle). One
 *   thread per triangle: rings 1..max_ring around the cells of its box while the ring has at most max_cols columns;
 *   unresolved[t] as above (cls 1 included). ns may be 0 (sorted_* then unused).
 * p2pb_p2m_point_face_subset / p2pb_p2m_face_point_subset: the brute-force result for the listed queries qidx i32[nq] only
 *   (one wave each, over ALL triangles / points), written to dist[q], idx[q].
 * -> 0, P2PB_EINVAL for bad sizes or NULL operands. */
int p2pb_p2m_grid_classify(int nt, const float *tris, float min_triangle_area, float mag, float *box, float *shrink,
                           unsigned char *cls, void *stream);
int p2pb_p2m_grid_count(int nt, const unsigned char *cls, const float *box, float cell, int cap, int *counts,
                        unsigned char *wide, void *stream);
int p2pb_p2m_grid_fill(int nt, const int *counts, const long long *offsets, const float *box, float cell, long long total,
                       long long *keys, int *ids, void *stream);
int p2pb_p2m_grid_point_face(int np, int nt, int ninc, int nwide, int max_ring, const float *points, const float *tris,
                             float min_triangle_area, const long long *keys, const int *ids, const int *wide_ids, float cell,
                             float mag, float shrink, float *dist, int *idx, unsigned char *unresolved, void *stream);
int p2pb_p2m_grid_face_point(int ns, int nt, int nextra, int max_ring, int max_cols, const float *sorted_points,
                             const int *order, const long long *sorted_keys, const float *extra, const int *extra_idx,
                             const float *tris, float min_triangle_area, const unsigned char *cls, const float *box, float cell,
                             float mag, float shrink, float *dist, int *idx, unsigned char *unresolved, void *stream);
int p2pb_p2m_point_face_subset(int nq, const int *qidx, int np, int nt, const float *points, const float *tris,
                               float min_triangle_area, float *dist, int *idx, void *stream);
int p2pb_p2m_face_point_subset(int nq, const int *qidx, int np, int nt, const float *points, const float *tris,
                               float min_triangle_area, float *dist, int *idx, void *stream);

/* point-to-mesh, packed batches with gradients ---------------------------------------------------------------------
 * The eight pytorch3d._C operators of the reference's metrics/p2m.py ({point_face, face_point, point_edge, edge_point}_dist_
 * {forward, backward}) as two entry points with a `kind` (csrc/p2m_packed.hip; Python side: p2p_bridge_amd/p2m.py). Pure
 * additions like the p2pb_p2m_grid_* entry points: P2PB_ABI_VERSION stays 13.
 * A QUERY is a point (kinds POINT_*) or a primitive (kinds FACE_POINT, EDGE_POINT), a TARGET the other side. points f32[np,3];
 * prims f32[ns,3,3] (FACE kinds, triangles) or f32[ns,2,3] (EDGE kinds, segments). Example b of the n packed ones owns points
 * [points_first_idx[b], points_first_idx[b+1]) and primitives [prims_first_idx[b], prims_first_idx[b+1]), the last example
 * up to np / ns (first indices i64[n], ascending, inside [0, np] / [0, ns]: values outside are clamped, never followed).
 *
 * p2pb_p2m_packed_forward: dist f32[nq], idx i64[nq] (nq = np or ns by kind): the squared distance of every query to the
 *   nearest target OF ITS EXAMPLE and that target's PACKED index, the first minimum in ascending packed index. The pair
 *   functions are those of p2pb_point_face_dist (csrc/p2m_geom.h), bit for bit: point_triangle_d2 with min_triangle_area for
 *   the FACE kinds, point_segment_d2 for the EDGE kinds (min_triangle_area unused). The grid is (ceil(max_queries / 256), n):
 *   a query beyond the first max_queries of its example is NOT written (pytorch3d's contract: pass the largest example's
 *   count); an example without targets gets dist 3.4e38 and idx -1. n <= 65535.
 * p2pb_p2m_packed_backward: idx i64[nq] as the forward wrote it, grad_dist f32[nq] -> grad_points f32[np,3], grad_prims shaped
 *   like prims: the derivative of dist[q] for the branch the forward took (csrc/p2m_grad.h; selections -- inside, the first
 *   nearest side, the clamp of t, the short-segment test -- are constants) times grad_dist[q]. A query's own row is WRITTEN; an
 *   idx outside the targets writes a zero row and contributes nothing. Target rows are sums over the queries that chose them:
 *     default mode: ADDED with fp32 atomics -- the caller passes the target tensor zeroed; order, start = NULL;
 *     deterministic mode (p2pb_set_deterministic): order i64[nq] = the queries sorted by idx (stable), start i64[nt+1] = the
 *     first position of every target in it (start[nt] = the end); one wave per target sums its list in ascending position,
 *     lanes strided, then across lanes in a fixed tree, and WRITES the row (zeros for a target nobody chose): no atomics, no
 *     zero fill needed, the same bits every run. order / start NULL in that mode: P2PB_EINVAL.
 * -> 0, P2PB_EINVAL for a bad kind, non-positive np, ns, n or max_queries, n > 65535 or NULL operands. */
#define P2PB_P2M_POINT_FACE 0
#define P2PB_P2M_FACE_POINT 1
#define P2PB_P2M_POINT_EDGE 2
#define P2PB_P2M_EDGE_POINT 3
int p2pb_p2m_packed_forward(int kind, int n, int np, int ns, int max_queries, const float *points,
                            const long long *points_first_idx, const float *prims, const long long *prims_first_idx,
                            float min_triangle_area, float *dist, long long *idx, void *stream);
int p2pb_p2m_packed_backward(int kind, int np, int ns, const float *points, const float *prims, const long long *idx,
                             const float *grad_dist, float min_triangle_area, const long long *order, const long long *start,
                             float *grad_points, float *grad_prims, void *stream);

/* grid k-NN -------------------------------------------------------------------------------------------------------
 * The K nearest points of a whole cloud WITH their indices, K <= 128: the (dist2, idx) of p2pb_knn_points, bit for bit and ties
 * included, from the ring search of p2pb_scan_knn_grid (csrc/knn_grid.hip; Python side: p2p_bridge_amd/knn_grid.py; the tie and
 * finality arguments: DESIGN.md, "Grid k-NN"). Pure additions like the p2pb_scan_* entry points: P2PB_ABI_VERSION stays 13.
 * The grid is the one of "scan fusion": sorted_points f32[n,3] and sorted_keys i64[n] (keys of p2pb_scan_cell_keys at the edge
 * `cell`, ascending), and rows i32[n] = the row of every sorted point in the caller's cloud. A wave keeps its K best as keys
 * (bits of fma(dz,dz, fma(dy,dy, dx*dx)) << 32 | row), d = point - query: all different, ordered by (distance, index).
 *
 * p2pb_knn_grid: one wave per query qidx[w] (i32[nq]; NULL: query w), rings 1..max_ring (<= 16) of cells around the query's
 *   cell. A ring is final when the K-th best squared distance is no larger than the squared distance to the nearest cell not
 *   yet visited (roundings of the cell index allowed for, less a margin of 1e-6: no unvisited point can tie). Then dist2
 *   f32[*,K] / idx i32[*,K] of row q hold the K pairs ascending and unresolved[q] = 0. Otherwise -- no final ring, fewer than K
 *   points seen, a query cell outside the key range -- unresolved[q] = 1 and row q is not written.
 * p2pb_knn_grid_brute: the same rows from a walk over all n points in the caller's order, one wave per query qidx[w].
 * No atomics: the same inputs give the same bits.
 * -> 0, P2PB_EINVAL for K outside [1, min(n, 128)], bad sizes or NULL operands (qidx may be NULL). */
int p2pb_knn_grid(int nq, int n, int k, int max_ring, const int *qidx, const float *query, const float *sorted_points,
                  const long long *sorted_keys, const int *rows, float cell, float *dist2, int *idx, unsigned char *unresolved,
                  void *stream);
int p2pb_knn_grid_brute(int nq, int n, int k, const int *qidx, const float *query, const float *points, float *dist2, int *idx,
                        void *stream);

/* grid nearest point -------------------------------------------------------------------------------------------------
 * The ONE nearest point of a whole cloud with its index, for the 10^6 .. 10^7 queries of a room-size Chamfer distance: row q
 * of p2pb_knn_grid at K = 1, and the (dist, idx) of p2pb_chamfer_forward's nm_distance_kernel, bit for bit and ties included
 * (the lowest row among the nearest), from the same ring search over the same grid (csrc/nn_grid.hip; Python side:
 * p2p_bridge_amd/knn_grid.py, PointGrid.nearest; the arguments: DESIGN.md, "Grid nearest point / Chamfer"). A pure addition:
 * P2PB_ABI_VERSION stays 13. sorted_points, sorted_keys, rows, cell: as for "grid k-NN".
 *
 * p2pb_nn_grid: one LANE per query qidx[w] (i32[nq]; NULL: query w), rings 1..max_ring (<= 16) of cells around the query's
 *   cell, one running minimum of the keys (bits of fma(dz,dz, fma(dy,dy, dx*dx)) << 32 | row), d = point - query. A ring is
 *   final by p2pb_knn_grid's test with the best distance in the K-th's place. Then dist2[q] f32 / idx[q] i32 hold the pair and
 *   unresolved[q] = 0. Otherwise -- no final ring, nothing seen, a query cell outside the key range -- unresolved[q] = 1 and
 *   dist2[q] / idx[q] are not written. The lanes are independent: the order of qidx decides which queries share a wave (give
 *   it a spatially coherent one, neighbouring lanes then read the same lines) and cannot change a bit of the result.
 * No atomics: the same inputs give the same bits.
 * -> 0, P2PB_EINVAL for bad sizes or NULL operands (qidx may be NULL). */
int p2pb_nn_grid(int nq, int n, int max_ring, const int *qidx, const float *query, const float *sorted_points,
                 const long long *sorted_keys, const int *rows, float cell, float *dist2, int *idx, unsigned char *unresolved,
                 void *stream);

#ifdef __cplusplus
}
#endif
#endif /* P2PB_HIP_H */
