/*
 * demf_hip.h — C ABI of libdemf_hip.so: the MI355X (gfx950) kernels behind the
 * DeMF fusion hot path.
 *
 * Every entry point replaces one native operator that the reference
 * (haoy945/DeMF) reaches through mmdet3d.ops / mmcv.ops.  The reference has no
 * native code of its own; each declaration cites the reference call site that
 * consumes the operator (file:line under the reference tree) and the upstream
 * operator it stands in for.
 *
 * Conventions (all entry points):
 *   - All pointers are DEVICE pointers on the current HIP device unless the
 *     name says otherwise.  Tensors are dense, row-major, fp32 / int32 / int64.
 *   - The caller owns every buffer.  The library never allocates, frees or
 *     synchronises; work is enqueued on `stream` (graph-capture safe).
 *   - Buffers documented "accumulated" must arrive zero-filled.
 *   - Return 0 on success; a negative DEMF_E* code otherwise.  A human-readable
 *     message for the calling thread is available from demf_last_error().
 *   - Re-entrant; no global mutable state besides the thread-local error text and a device-side ring
 *     of self-resetting tile counters (256 KB) that the persistent shared-MLP GEMM launches claim
 *     their row tiles from: a launch is handed the next counter set of the ring and leaves it zeroed,
 *     so captured launches replay with the set they were given.  Two launches share a set only if
 *     a multiple of 1024 counter-using launches lies between their enqueues; that matters only if
 *     they also run concurrently on different streams (the path itself is single-stream;
 *     DEMF_STATIC_TILES=1 switches the counters off).
 */
#ifndef DEMF_HIP_H_
#define DEMF_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* hipStream_t without dragging the HIP headers into the consumer. */
typedef void* demf_stream_t;

#define DEMF_OK 0
#define DEMF_EINVAL (-1)   /* bad argument (sizes, null pointer)            */
#define DEMF_ELAUNCH (-2)  /* hipGetLastError() reported a launch failure   */
#define DEMF_EUNSUPPORTED (-3)

#define DEMF_ABI_VERSION 2

/* Two tiers of entry points.
 *   PUBLIC (unmarked): the operators with an upstream counterpart that the reference reaches through mmdet3d.ops /
 *     mmcv.ops - furthest_point_sample, ball_query, group_points, gather_points, three_nn, three_interpolate,
 *     ms_deform_attn - with upstream's argument lists (+ stream), plus demf_version / demf_last_error.  These are
 *     what a maintainer of the reference binds (INTEGRATION.md sections 1-2) and what stays stable.
 *   DEMF_INTERNAL: everything else - fused layer kernels, layout-specific variants, scratch-size queries, the step
 *     engine's helpers.  They are exported (the Python host layer of this package calls them through ctypes) and
 *     declared here so that tests/test_abi.py can hold header, exports and binding table against each other, but
 *     they are shaped by THIS package's modules (one decoder layer, one stack shape) and may change with them.   */
#define DEMF_INTERNAL

int demf_version(void);
const char* demf_last_error(void);

/* A stream restricted to the listed CUs (invert != 0: to all CUs except them); used to keep the
 * pipelined FPS pre-pass and the main training stream on disjoint CUs.  Host-side helper: `cus`
 * and `out` are HOST pointers; the stream is owned by the caller (hipStreamDestroy).        */
DEMF_INTERNAL int demf_stream_create_cu_masked(const int* cus, int n, int invert, void** out);

/* One wave that spins for `microseconds` of wall-clock time on `stream` and touches no memory: a
 * stand-in of known length for the gradient all-reduce (reference: MMDistributedDataParallel's NCCL
 * all-reduce, /root/reference/train.py:56-63) when the engine's communication / compute overlap is
 * measured on a single GPU (bench.py --allreduce-stub-us).                                        */
DEMF_INTERNAL int demf_spin_us(int microseconds, demf_stream_t stream);

/* ------------------------------------------------------------------ *
 * PointNet++ set-abstraction operators
 * ------------------------------------------------------------------ */

/* furthest_point_sample(points_xyz (B,N,3), num_points M) -> idx (B,M) i32.
 * Reference call sites: demf/modeling/heads/class_agnostic_vote_head.py:429-430
 * (direct) and every PointSAModule of the backbone / vote aggregation
 * (configs/demf/demf_votenet.py:48-62,155-162).  Stands in for mmdet3d.ops
 * furthest_point_sample.  idx[b,0] = 0; ties resolve exactly as the upstream
 * block reduction does (see DESIGN.md "canonical arithmetic").
 * `temp` is the (B,N) scratch the upstream ABI carries; it may be NULL for 64 <= N <= 24576.
 * When it is given (>= B ints) and N <= 4M <= 4096, a dependency-free check first tests whether
 * the cloud already is in FPS order (as every SA level after the first is) and, if so, answers
 * 0..M-1 without running the M-round chain; ties fall back to the chain, results are identical. */
int demf_fps_f32(int B, int N, int M, const float* xyz, float* temp, int* idx,
                 demf_stream_t stream);
/* The same with the scratch size stated (floats): with >= B * (M + 2) floats the ordered-input check runs spread
 * over the chip (two launches, one workgroup per 256 points) instead of on one compute unit per scene - 162 -> ~25 us
 * at 2 048 -> 1 024, on the serial pre-pass chain.  Identical results.                                   */
DEMF_INTERNAL int demf_fps_ws_f32(int B, int N, int M, const float* xyz, float* temp, long long temp_floats, int* idx,
                    demf_stream_t stream);

/* ball_query(min_radius, max_radius, sample_num, xyz (B,N,3), center (B,M,3))
 * -> idx (B,M,nsample) i32.  Reference: QueryAndGroup inside build_sa_module
 * (class_agnostic_vote_head.py:383,455; config radii demf_votenet.py:51-53,158).
 * First `nsample` hits in index order; first hit pre-fills all slots; a centre
 * with no hit yields zeros.                                                  */
int demf_ball_query_f32(int B, int N, int M, float min_radius, float max_radius,
                        int nsample, const float* center_xyz, const float* xyz,
                        int* idx, demf_stream_t stream);
/* The same result (min_radius = 0) for large clouds, N <= 32768, through a hashed uniform grid built on
 * the fly (two launches): every centre only meets the points of the 2x2x2 cells of edge 2r its ball can
 * reach instead of all N; the hit set and the index order are the scan's (csrc/ball_query.hip).
 * Workspace (device): ws_start = *start_ints ints, ws_cells = *cell_floats floats (16-byte aligned), the
 * sizes from demf_ball_query_grid_ws.                                                              */
DEMF_INTERNAL int demf_ball_query_grid_ws(int B, int N, long long* start_ints, long long* cell_floats);
DEMF_INTERNAL int demf_ball_query_grid_f32(int B, int N, int M, float max_radius, int nsample,
                             const float* center_xyz, const float* xyz, int* idx,
                             int* ws_start, float* ws_cells, demf_stream_t stream);

/* grouping_operation: features (B,C,N), idx (B,M,ns) -> out (B,C,M,ns).
 * bwd: grad_out (B,C,M,ns) -> grad_features (B,C,N), accumulated.            */
int demf_group_points_fwd(int B, int C, int N, int M, int ns, const float* features,
                          const int* idx, float* out, demf_stream_t stream);
int demf_group_points_bwd(int B, int C, int N, int M, int ns, const float* grad_out,
                          const int* idx, float* grad_features, demf_stream_t stream);

/* gather_points: features (B,C,N), idx (B,M) -> out (B,C,M).
 * bwd: grad_out (B,C,M) -> grad_features (B,C,N), accumulated.               */
int demf_gather_points_fwd(int B, int C, int N, int M, const float* features,
                           const int* idx, float* out, demf_stream_t stream);
int demf_gather_points_bwd(int B, int C, int N, int M, const float* grad_out,
                           const int* idx, float* grad_features, demf_stream_t stream);

/* three_nn(target (B,n,3), source (B,m,3)) -> dist2 (B,n,3) SQUARED distances
 * (the Python wrapper applies sqrt, as upstream does), idx (B,n,3) i32.
 * Reference: PointFPModule of the backbone (demf_votenet.py:56).             */
int demf_three_nn_f32(int B, int n, int m, const float* target, const float* source,
                      float* dist2, int* idx, demf_stream_t stream);
/* the same search + what PointFPModule.forward derives from it (mmdet3d PointFPModule: dist_recip =
 * 1 / (dist + 1e-8), weight = dist_recip / sum(dist_recip)): dist (B,n,3) = sqrt of the squared
 * distances, idx (B,n,3), weight (B,n,3) - one launch instead of the search + 6 element-wise ones. */
DEMF_INTERNAL int demf_three_nn_weights_f32(int B, int n, int m, const float* target, const float* source,
                              float* dist, int* idx, float* weight, demf_stream_t stream);

/* three_interpolate: features (B,C,m), idx (B,n,3), weight (B,n,3) -> (B,C,n).
 * bwd: grad_out (B,C,n) -> grad_features (B,C,m), accumulated.               */
int demf_three_interpolate_fwd(int B, int C, int m, int n, const float* features,
                               const int* idx, const float* weight, float* out,
                               demf_stream_t stream);
int demf_three_interpolate_bwd(int B, int C, int n, int m, const float* grad_out,
                               const int* idx, const float* weight,
                               float* grad_features, demf_stream_t stream);

/* ------------------------------------------------------------------ *
 * Channels-last (point-major) fused variants used by the MI355X modules.
 * Same arithmetic as the operators above; layout chosen so that a gathered
 * neighbour is one contiguous C*4-byte row.
 * ------------------------------------------------------------------ */

/* QueryAndGroup fused (ball-query indices -> grouped MLP input), one row per
 * neighbour:  out[b,m,s, xyz_col:xyz_col+3]  = (xyz[b,idx]-center[b,m]) / radius
 * (no division when normalize_xyz == 0), out[b,m,s, feat_col:feat_col+C] =
 * feat[b,idx,:]; every other column of the ldo-wide row is written as zero.
 * xyz (B,N,3), center (B,M,3), feat (B,N,C) or NULL (C=0), idx (B,M,ns),
 * out (B,M,ns,ldo).  The two column ranges must not overlap.                 */
DEMF_INTERNAL int demf_group_concat_cl_fwd(int B, int N, int M, int ns, int C, int ldo,
                             int xyz_col, int feat_col, float radius,
                             int normalize_xyz, const float* xyz,
                             const float* center, const float* feat, const int* idx,
                             float* out, demf_stream_t stream);
/* bwd: grad_out (B,M,ns,ldo) -> grad_feat (B,N,C), grad_xyz (B,N,3), grad_center
 * (B,M,3), all accumulated.  grad_feat may be NULL; grad_xyz/grad_center may both be
 * NULL (backbone levels: raw coordinates carry no gradient; the vote aggregation of
 * class_agnostic_vote_head.py:455 needs them - vote_points are learned).        */
DEMF_INTERNAL int demf_group_concat_cl_bwd(int B, int N, int M, int ns, int C, int ldo,
                             int xyz_col, int feat_col, float radius,
                             int normalize_xyz, const float* grad_out, const int* idx,
                             float* grad_feat, float* grad_xyz, float* grad_center,
                             demf_stream_t stream);

/* rows gather: feat (B,N,C), idx (B,M) -> out (B,M,C); bwd accumulated.      */
DEMF_INTERNAL int demf_gather_rows_cl_fwd(int B, int N, int M, int C, const float* feat,
                            const int* idx, float* out, demf_stream_t stream);
DEMF_INTERNAL int demf_gather_rows_cl_bwd(int B, int N, int M, int C, const float* grad_out,
                            const int* idx, float* grad_feat, demf_stream_t stream);

/* three_nn + inverse-distance weights + interpolate fused, channels-last:
 * feat (B,m,C), idx/weight (B,n,3) -> out (B,n,ldo) columns [col0, col0+C).  */
DEMF_INTERNAL int demf_three_interpolate_cl_fwd(int B, int m, int n, int C, int ldo, int col0,
                                  const float* feat, const int* idx,
                                  const float* weight, float* out,
                                  demf_stream_t stream);
DEMF_INTERNAL int demf_three_interpolate_cl_bwd(int B, int m, int n, int C, int ldo, int col0,
                                  const float* grad_out, const int* idx,
                                  const float* weight, float* grad_feat,
                                  demf_stream_t stream);
/* PointFPModule.forward's interpolate + torch.cat([interpolated, target_feats]) in one launch:
 * out (B,n,C+Cs) = [ three_interpolate(feat (B,m,C)) | skip (B,n,Cs) ].  Backward: the interpolated
 * columns through demf_three_interpolate_cl_bwd(ldo = C+Cs, col0 = 0); the skip gradient is the
 * column range [C, C+Cs) of the incoming gradient itself.                                        */
DEMF_INTERNAL int demf_three_interpolate_cat_cl_fwd(int B, int m, int n, int C, int Cs, const float* feat,
                                      const int* idx, const float* weight, const float* skip,
                                      float* out, demf_stream_t stream);

/* max over the ns neighbours: x (R, ns, C) -> out (R, C), arg (R, C) i32
 * (first maximum wins, as torch max_pool2d does).  bwd scatters to x grad.   */
DEMF_INTERNAL int demf_maxpool_ns_fwd(int R, int ns, int C, const float* x, float* out, int* arg,
                        demf_stream_t stream);
DEMF_INTERNAL int demf_maxpool_ns_bwd(int R, int ns, int C, const float* grad_out, const int* arg,
                        float* grad_x /* (R,ns,C), fully written */,
                        demf_stream_t stream);

/* Inverse neighbour lists of a ball-query result: idx (B,E) int32 with values in [0,N), E = M*ns
 * -> CSR by source point: off (B,N+1), rows (B,E) = entry positions e = m*ns+s, ascending within a
 * list.  N <= 16384.  Coordinate-only (QueryAndGroup's idx, class_agnostic_vote_head.py:383). */
DEMF_INTERNAL int demf_invert_index(int B, int N, int E, const int* idx, int* off, int* rows, demf_stream_t stream);
/* The same with B * E ints of workspace: for E >= 32 768 entries per scene (SA1: the lists do not fit one workgroup's
 * LDS) the inversion runs spread over the chip - histogram, scan, fill, rank (five launches) - instead of one
 * workgroup per scene with a global insertion sort (102 -> ~35 us).  Identical output.                     */
DEMF_INTERNAL int demf_invert_index_ws(int B, int N, int E, const int* idx, int* off, int* rows, int* workspace,
                         demf_stream_t stream);

/* sa_indices of the backbone (mmdet3d PointNet2SASSG.forward as used by demf/modeling: every level's samples as
 * indices into the INPUT cloud): out[0] (B,N) = arange(N), out[l] (B, samples[l-1]) = out[l-1] gathered by the
 * level's FPS indices idx[l-1] (B, samples[l-1]) int32; int64 outputs as the reference returns them.  nlev <= 8. */
DEMF_INTERNAL int demf_sa_index_chain(int B, int N, int nlev, const int* const* idx, const int* samples, int64_t* const* out,
                        demf_stream_t stream);
/* points (rows, 3 + C) -> xyz (rows, 3) | feat (rows, C): `points[..., :3]`, `points[..., 3:]` of the backbone
 * input as contiguous tensors, one launch. */
DEMF_INTERNAL int demf_split_points(long long rows, int C, const float* points, float* xyz, float* feat, demf_stream_t stream);

/* grad_feat (B,N,C) of demf_group_concat_cl_fwd through the inverse lists: every source point sums
 * the grad_out rows (B,E,ldo)[.., feat_col:feat_col+C] that gathered it.  No atomics; grad_feat is
 * fully written (need not arrive zeroed).  C % 4 == 0.  Same result as demf_group_concat_cl_bwd's
 * grad_feat up to summation order. */
DEMF_INTERNAL int demf_group_concat_cl_bwd_gather(int B, int N, int E, int C, int ldo, int feat_col,
                                    const float* grad_out, const int* off, const int* rows,
                                    float* grad_feat, demf_stream_t stream);

/* First 1x1 convolution of a set-abstraction level without the grouped tensor (PointSAModule built by
 * build_sa_module, class_agnostic_vote_head.py:383,455; QueryAndGroup with use_xyz / normalize_xyz).
 * The grouped row is [(xyz_j - centre)/radius | feat_j]; with U (B*N, C1) = feat . Wf^T computed per
 * SOURCE point and Wx (3, C1) the xyz columns of the weight (k-major),
 *   Y[b,m,s,:] = U[b, idx[b,m,s], :] + rel(b,m,s) . Wx          (rows (B*M*ns, C1), fully written)
 * stats (2*C1 fp64: column sum | sum of squares, accumulated, as demf_mlp_gemm_fwd) or NULL.
 * C1 in {64,128,256}. */
DEMF_INTERNAL int demf_group_first_fwd(int B, int N, int M, int ns, int C1, float radius, int normalize_xyz,
                         const float* xyz, const float* center, const int* idx, const float* U,
                         const float* Wx, int w_ld /* 0: Wx is the (3, C1) copy; > 0: Wx is the layer's
                         weight (C1 x w_ld row-major) itself, columns 0..2 read in place */,
                         float* Y, double* stats,
                         /* train-mode BatchNorm bookkeeping of the layer (demf_bn_finalize's arguments) done by the
                          * launch's last workgroup - or, without a counter set, by a demf_bn_finalize launch behind it;
                          * scale_shift == NULL: none, the sums stay in stats */
                         const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
                         float* running_var, long long* num_batches_tracked, float* scale_shift, float* mean_invstd,
                         const float* conv_bias, demf_stream_t stream);
/* Backward of the above through the inverse lists of demf_invert_index: with dY the BN-backward
 * transform of (G, Y) by vec6 (demf_bn_bwd_vectors; same formula as demf_mlp_gemm_bwd_dx),
 *   dU[b,j,:]  = sum of dY over the rows that gathered point j        (fully written, no atomics)
 *   dWx[k,:]  += sum over all rows of rel_k . dY                      (3*C1 fp32, arrives zeroed)
 * and, when the coordinates carry a gradient (the vote aggregation), d rel = dY . Wx^T per row:
 *   dxyz[b,j,:] = + sum over the rows of point j / radius,  dcenter[b,m,:] -= sum over s / radius */
DEMF_INTERNAL int demf_group_first_bwd(int B, int N, int M, int ns, int C1, float radius, int normalize_xyz,
                         const float* xyz, const float* center, const float* G, const float* Y,
                         const float* U /* the forward's U (B*N, C1): y is formed again from it instead of being read
                         (half the bytes; needs Wx), or NULL: y read from Y */,
                         const float* vec6, const int* inv_off, const int* inv_rows, float* dU,
                         float* dWx, int dw_ld /* 0: (3, C1) layout; > 0: dWx[c*dw_ld + k], i.e. columns
                         0..2 of the (C1 x dw_ld) weight gradient */,
                         const float* Wx /* needed with dxyz or U */, int w_ld /* as in the forward */,
                         float* dxyz /* (B,N,3) fully written, or NULL */,
                         float* dcenter /* (B,M,3) accumulated: arrives zeroed, or NULL */,
                         double* wacc /* 8*3*C1 doubles, zero on entry and left zeroed: the workgroups' partial dWx are
                         summed there (contiguous atomics) and the last workgroup adds the totals to dWx; or NULL:
                         every workgroup adds to dWx itself */,
                         demf_stream_t stream);

/* One pyramid level (B,C,HW) channel-major -> rows [row0,row0+HW) of the channels-last token buffer
 * (B,S,C): the flatten + transpose + concat of prepare_decoder_inputs
 * (class_agnostic_vote_head.py:570-591) as a tiled transpose.  mask (B,S) bytes or NULL: tokens
 * with a non-zero mask byte (image padding) are written as zeros.                               */
DEMF_INTERNAL int demf_nchw_to_tokens(int B, int C, int HW, int S, int row0, const float* src,
                        const unsigned char* mask, float* dst, demf_stream_t stream);
/* Every level of the pyramid in one launch: srcs[l] (B,C,hws[l]) channel-major -> consecutive row
 * ranges of dst (B,S,C), S = sum hws (nlev <= 8; srcs / hws are HOST arrays of device pointers / sizes). */
DEMF_INTERNAL int demf_pyramid_to_tokens(int B, int C, int S, int nlev, const float* const* srcs, const int* hws,
                           const unsigned char* mask, float* dst, demf_stream_t stream);
/* The same transposes into bf16 token rows (2-byte elements, round to nearest even; C % 4 == 0): what
 * demf_msda_{fwd,bwd}_bf16 gather from - BASELINE configs[3], half the bytes of the 152 MB token tensor. */
DEMF_INTERNAL int demf_pyramid_to_tokens_bf16(int B, int C, int S, int nlev, const float* const* srcs, const int* hws,
                                const unsigned char* mask, uint16_t* dst, demf_stream_t stream);
/* A batch's tokens out of the frozen image-feature cache (csrc/featcache.hip).  arena (arena_rows, C), fp32 or bf16
 * words (arena_bf16); table (N, 1 + 2L) int64 rows [row0, h_0, w_0, ..] on the device, table_host the same on the
 * host; indices (B) int64 dataset indices on the device (repeats allowed), indices_host the same on the host; hw
 * (HOST, 2L ints) the batch's level shapes (H_l, W_l), S = sum H_l W_l; mask (B,S) bytes or NULL; out (B,S,C) fp32 or
 * bf16 words (out_bf16).  Every row of out is written:
 *   out[b, start_l + y W_l + x] = (y < h_bl && x < w_bl && !mask) ? arena[row0_b + ownstart_bl + y w_bl + x] : 0
 * fp32 -> bf16 rounds to nearest even.  L <= 8, C % 4 == 0; every scene of the batch is checked against the host
 * table (index in range, own level <= the batch's, rows inside the arena) before anything is launched.           */
DEMF_INTERNAL int demf_tokens_assemble(int B, int C, int S, int L, long long N, long long arena_rows, const void* arena,
                         int arena_bf16, const long long* table, const long long* table_host,
                         const long long* indices, const long long* indices_host, const int* hw,
                         const unsigned char* mask, void* out, int out_bf16, demf_stream_t stream);

/* out (N) += column sums of x (R,N; row stride ld).  out arrives zeroed.  The bias gradient of the
 * path's linear layers (mmcv FFN / MultiheadAttention / MultiScaleDeformableAttention projections,
 * transformer.py:73; conv_cls / conv_reg, class_agnostic_vote_head.py:398) - replaces
 * at::sum's two-stage semaphore reduction, which mis-reduces inside hipGraph replays. */
DEMF_INTERNAL int demf_colsum_f32(int R, int N, int ld, const float* x, float* out, demf_stream_t stream);

/* ------------------------------------------------------------------ *
 * Fused shared-MLP (1x1 conv + train-mode BatchNorm + ReLU [+ max over
 * neighbours]) on point-major rows: the dense half of every PointSAModule
 * (class_agnostic_vote_head.py:383; demf_votenet.py:48-62).  fp32 MFMA.
 * act(y) = max(0, y*scale + shift) with scale = gamma*invstd, shift = beta - mean*scale.
 * ------------------------------------------------------------------ */

/* Y (R,N) = pro(X) (R,K; row stride ldx) @ Wt (N,K)^T.  pro = act of the PREVIOUS layer when
 * pro_scale_shift ([scale(K)|shift(K)]) is non-NULL, identity otherwise.  When stats is
 * non-NULL the per-column sum and sum of squares of Y are ACCUMULATED into stats[0:N],
 * stats[N:2N] (fp64).  K%4==0, ldx%4==0, N%32==0, N<=256.                        */
DEMF_INTERNAL int demf_mlp_gemm_fwd(int R, int K, int N, int ldx, const float* X,
                      const float* pro_scale_shift, const float* Wt, float* Y,
                      double* stats, demf_stream_t stream);

/* demf_mlp_gemm_fwd with the max-pool of the PointSAModule fused into the epilogue: per group of
 * ns consecutive rows and column, pmax/pmin (R/ns,N) = max/min of the raw output and amax/amin
 * their row offsets (first on ties).  max_s relu(sc*y_s+sh) = relu(sc*(sc>0 ? pmax : pmin)+sh), so
 * the pooled activation follows from these once the batch statistics are known
 * (demf_pool_select) without re-reading Y.  ns 16, 32 or 64; DEMF_EUNSUPPORTED otherwise.                                                                   */
DEMF_INTERNAL int demf_mlp_gemm_fwd_pool(int R, int K, int N, int ldx, const float* X,
                           const float* pro_scale_shift, const float* Wt, float* Y, double* stats,
                           int ns, float* pmax, float* pmin, int* amax, int* amin,
                           demf_stream_t stream);

/* demf_mlp_gemm_fwd / demf_mlp_gemm_fwd_pool followed by demf_bn_finalize(N, count = R, stats, ...)
 * as ONE launch: the last workgroup of the GEMM turns the column sums into scale_shift,
 * mean_invstd and the running statistics (torch.nn.BatchNorm semantics, see demf_bn_finalize) and
 * leaves `stats` zeroed.  The following layer's launch reads scale_shift as its prologue.
 * demf_mlp_gemm_fwd_pool_bn with pmin == amin == NULL: the sign of the BN scale is the sign of gamma,
 * so only the extremum the consumer will select is reduced - pmax / amax then hold, per group and
 * column, the maximum of y for gamma >= 0 and the minimum otherwise (pass them to demf_pool_select
 * as both the max and the min operands).                                                            */
DEMF_INTERNAL int demf_mlp_gemm_fwd_bn(int R, int K, int N, int ldx, const float* X, const float* pro_scale_shift,
                         const float* Wt, float* Y, double* stats, const float* gamma,
                         const float* beta, float eps, float momentum, float* running_mean,
                         float* running_var, long long* num_batches_tracked, float* scale_shift,
                         float* mean_invstd, const float* conv_bias, demf_stream_t stream);
DEMF_INTERNAL int demf_mlp_gemm_fwd_pool_bn(int R, int K, int N, int ldx, const float* X,
                              const float* pro_scale_shift, const float* Wt, float* Y, double* stats,
                              int ns, float* pmax, float* pmin, int* amax, int* amin,
                              const float* gamma, const float* beta, float eps, float momentum,
                              float* running_mean, float* running_var,
                              long long* num_batches_tracked, float* scale_shift,
                              float* mean_invstd, const float* conv_bias, demf_stream_t stream);

/* out (Rp,C) = relu(scale*y*+shift), arg = row offset of y* (see demf_mlp_gemm_fwd_pool);
 * yraw (Rp,C) or NULL = y* itself, which spares demf_bn_bwd_reduce its gather from Y. */
DEMF_INTERNAL int demf_pool_select(int Rp, int C, const float* pmax, const float* pmin, const int* amax,
                     const int* amin, const float* scale_shift, float* out, int* arg, float* yraw,
                     demf_stream_t stream);

/* demf_pool_select behind the NO-STORE pooled forward (demf_mlp_gemm_fwd_pool_bn_st with store_flags = 4:
 * the raw (R x N) output of the pooled last layer is not written; zero-scale channels arrive with slot 0
 * and its raw value in pmax / amax, so yraw is complete).                                              */
DEMF_INTERNAL int demf_pool_select_slot0(int Rp, int C, const float* pmax, const int* amax, const float* scale_shift,
                           float* out, int* arg, float* yraw, demf_stream_t stream);

/* stats (2N fp64) over `count` rows -> scale_shift (2N), mean_invstd (2N); updates the
 * running statistics (momentum, unbiased variance) and increments *num_batches_tracked when
 * they are non-NULL (BatchNorm's train-mode bookkeeping).  The consumed accumulator is left
 * ZEROED, so a persistent stats buffer needs no per-step clearing.  conv_bias (N) or NULL: the bias
 * of the convolution in front of the BatchNorm - it cancels in the normalised output and never
 * reaches the GEMM; it only shifts the batch mean that enters the running mean.              */
DEMF_INTERNAL int demf_bn_finalize(int N, long long count, double* stats, const float* gamma,
                     const float* beta, float eps, float momentum, float* running_mean,
                     float* running_var, long long* num_batches_tracked, float* scale_shift,
                     float* mean_invstd, const float* conv_bias, demf_stream_t stream);

/* y = x / ||x||_2 over rows of C channels (VoteModule norm_feats, class_agnostic_vote_head.py:413-414 ->
 * mmdet3d VoteModule.forward); norm (R) kept for the backward dx = (dy - y (y . dy)) / norm.  */
DEMF_INTERNAL int demf_l2norm_rows_fwd(int R, int C, const float* x, float* y, float* norm, demf_stream_t stream);
DEMF_INTERNAL int demf_l2norm_rows_bwd(int R, int C, const float* y, const float* norm, const float* dy, float* dx,
                         demf_stream_t stream);

/* VoteModule tail (mmdet3d VoteModule.forward with vote_per_seed = 1, with_res_feat, norm_feats; built at
 * class_agnostic_vote_head.py:382) as one pass each way.  votes (R, 3 + C) = conv_out's rows:
 *   vote_xyz = seed_xyz + votes[:, :3];  vote_feats = l2-normalised rows of (rows + votes[:, 3:]).
 * Backward writes d_votes (R, 3 + C) completely and d_rows (R, C); d_vote_feats / d_vote_xyz may be
 * null (= zero).  C in {64, 128, 256, 512, 1024}.                                                  */
DEMF_INTERNAL int demf_vote_combine_fwd(int R, int C, const float* rows, const float* votes, const float* seed_xyz,
                          float* vote_xyz, float* vote_feats, float* norm, demf_stream_t stream);
DEMF_INTERNAL int demf_vote_combine_bwd(int R, int C, const float* vote_feats, const float* norm,
                          const float* d_vote_feats, const float* d_vote_xyz, float* d_votes,
                          float* d_rows, demf_stream_t stream);

/* out (R,C) = max over s of act(Y (R,ns,C)); arg = first maximising s.           */
DEMF_INTERNAL int demf_bnrelu_maxpool_fwd(int R, int ns, int C, const float* Y, const float* scale_shift,
                            float* out, int* arg, demf_stream_t stream);

/* BatchNorm backward reductions of one layer: g12[0:N] += sum dZ, g12[N:2N] += sum dZ*xhat
 * with dZ = dA * [act'(Y)].  Upstream gradient dA is either dense G (R,N) or, for the pooled
 * last layer, sparse: dP (R/ns,N) routed to slot arg (R/ns,N); yraw (R/ns,N) or NULL = Y at
 * those slots (from demf_pool_select), read instead of gathering it.               */
DEMF_INTERNAL int demf_bn_bwd_reduce(int R, int N, int ns, const float* G, const float* dP, const int* arg,
                       const float* Y, const float* yraw, const float* scale_shift,
                       const float* mean_invstd, double* g12, demf_stream_t stream);

/* g12 -> the five per-channel vectors the backward GEMM prologues consume (vec6: 5N floats:
 * scale, shift, gi = gamma*invstd, a, b with dY = gi*dZ + a*y + b) + dgamma, dbeta.  The
 * consumed g12 is left ZEROED.                                                            */
DEMF_INTERNAL int demf_bn_bwd_vectors(int N, long long count, double* g12, const float* gamma,
                        const float* scale_shift, const float* mean_invstd, float* vec6,
                        float* dgamma, float* dbeta, demf_stream_t stream);

/* dX (R,K; row stride ldo) = dY (R,N) @ W (N,K) with dY = BN/ReLU backward of (dA, Y)
 * formed on the fly.  Wtt = W^T stored (K,N) row-major.  N%4==0.                  */
DEMF_INTERNAL int demf_mlp_gemm_bwd_dx(int R, int N, int K, int ldo, const float* G, const float* dP,
                         const int* arg, int ns, const float* Y, const float* vec6,
                         const float* Wtt, float* dX, demf_stream_t stream);
/* Same, reading the layer's weight W (N x K row-major, K % 4 == 0) itself instead of a transposed
 * copy made per step (the B slab is transposed on its way into LDS). */
DEMF_INTERNAL int demf_mlp_gemm_bwd_dx_w(int R, int N, int K, int ldo, const float* G, const float* dP,
                         const int* arg, int ns, const float* Y, const float* vec6,
                         const float* W, float* dX, demf_stream_t stream);
/* demf_mlp_gemm_bwd_dx_w that also adds layer l-1's BN-backward sums - exactly what
 * demf_bn_bwd_reduce(R, K, G = dX, Yprev, ...) would add to g12_prev (2K fp64) - taken from the
 * output tiles on their way out, so that pass over dX and Yprev disappears.  K % 4 == 0. */
DEMF_INTERNAL int demf_mlp_gemm_bwd_dx_red(int R, int N, int K, int ldo, const float* G, const float* dP,
                             const int* arg, int ns, const float* Y, const float* vec6,
                             const float* W, float* dX, const float* Yprev,
                             const float* scale_shift_prev, const float* mean_invstd_prev,
                             double* g12_prev, demf_stream_t stream);

/* Backward of a shared-MLP stack whose FIRST layer has a 4-float input row and needs no input
 * gradient (SA1: [height | rel_xyz]).  The dx GEMM of layer 1 (dY1 from (G, Y1, vec6); W1 (N x K0))
 * does not store its (R x K0) output - the gradient of layer 0's activation - but takes the raw
 * sums of layer 0's whole backward from it: sums (10*K0 + 4 fp64, accumulated, arrives zeroed) =
 * g1 | g2 | P = dZ0^T X0 (K0 x 4) | Q = Y0^T X0 (K0 x 4) | colsum(X0).  K0 <= 64, K0 % 4 == 0.
 * demf_mlp_first_finish then forms dW0 (K0 x 4) = gi*P + a*Q + b*cx^T, dgamma0 = g2, dbeta0 = g1
 * (the BN-backward identities of demf_bn_bwd_vectors) and leaves the sums zeroed. */
DEMF_INTERNAL int demf_mlp_gemm_bwd_dx_first(int R, int N, int K0, const float* G, const float* Y1,
                               const float* vec6, const float* W1, const float* X0,
                               const float* Y0, const float* scale_shift0,
                               const float* mean_invstd0, double* sums, demf_stream_t stream);
DEMF_INTERNAL int demf_mlp_first_finish(int N0, long long count, double* sums, const float* gamma0,
                          const float* mean_invstd0, float* dW0, float* dgamma0, float* dbeta0,
                          demf_stream_t stream);

/* demf_mlp_gemm_bwd_dx_red + layer l-1's backward vectors (demf_bn_bwd_vectors on g12_prev) formed by
 * the launch's last workgroup: the ~5 us vectors launch behind every layer's backward disappears. */
DEMF_INTERNAL int demf_mlp_gemm_bwd_dx_red_v(int R, int N, int K, int ldo, const float* G, const float* dP,
                               const int* arg, int ns, const float* Y, const float* vec6,
                               const float* W, float* dX, const float* Yprev,
                               const float* scale_shift_prev, const float* mean_invstd_prev,
                               double* g12_prev, const float* gamma_prev, float* vec6_prev,
                               float* dgamma_prev, float* dbeta_prev, demf_stream_t stream);
/* demf_bn_bwd_reduce (sparse form: the pooled last layer of a stack) + demf_bn_bwd_vectors in ONE launch.
 * y_bf16: Y holds bf16 rows (demf_mlp_gemm_fwd_pool_bn_st).                                              */
DEMF_INTERNAL int demf_bn_bwd_reduce_vectors(int R, int N, int ns, const float* dP, const int* arg, const float* Y,
                               const float* yraw, const float* scale_shift, const float* mean_invstd,
                               double* g12, const float* gamma, float* vec6, float* dgamma, float* dbeta,
                               int y_bf16, demf_stream_t stream);

/* demf_mlp_gemm_fwd_bn / demf_mlp_gemm_fwd_pool_bn with the rows stored as bf16 in HBM (bf16 compute
 * mode, BASELINE configs[3]: "bf16 training step"): store_flags bit 0 = X holds bf16, bit 1 = Y is
 * written as bf16; ldx counts elements.  Statistics and the pooled extremum are taken from the fp32
 * accumulators.  Weight-resident forward only (K = 64, N = 64 / 128, R >= 16384; the forms built:
 * flags 2 for N = 64, flags 3 pooled for N = 128): DEMF_EUNSUPPORTED otherwise, callers keep fp32 rows. */
DEMF_INTERNAL int demf_mlp_gemm_fwd_bn_st(int R, int K, int N, int ldx, const void* X, const float* pro_scale_shift,
                            const float* Wt, void* Y, double* stats, const float* gamma,
                            const float* beta, float eps, float momentum, float* running_mean,
                            float* running_var, long long* num_batches_tracked, float* scale_shift,
                            float* mean_invstd, const float* conv_bias, int store_flags,
                            demf_stream_t stream);
DEMF_INTERNAL int demf_mlp_gemm_fwd_pool_bn_st(int R, int K, int N, int ldx, const void* X,
                                 const float* pro_scale_shift, const float* Wt, void* Y, double* stats,
                                 int ns, float* pmax, int* amax, const float* gamma, const float* beta,
                                 float eps, float momentum, float* running_mean, float* running_var,
                                 long long* num_batches_tracked, float* scale_shift, float* mean_invstd,
                                 const float* conv_bias, int store_flags, demf_stream_t stream);

/* One pass over a layer's saved output for its whole backward (csrc/mlp_bwd.hip): what
 * demf_mlp_gemm_bwd_dx_red + demf_mlp_gemm_bwd_dw do in two (or, with first_sums != NULL,
 * demf_mlp_gemm_bwd_dx_first + demf_mlp_gemm_bwd_dw: dX is then not stored and X0 (R x 4) / first_sums
 * take the place of dX / g12_prev).  The dY tile is rebuilt and split into bf16 planes once and feeds
 * both contractions; W stays in registers.  Yprev (R x K) = pre-BN output of layer l-1, row stride K;
 * dX row stride K; dW (N x K) accumulated (arrives zeroed).  Compute modes 1 (bf16) and 2 (fp32 as
 * three bf16 terms) only; shapes (N,K) in {(128,64), (128,128), (64,64), (256,128)}, ns % 4 == 0 when sparse
 * (G == NULL); anything else returns DEMF_EINVAL and callers use the two-launch path.  With gamma_prev !=
 * NULL (and not first_sums) the launch's last workgroup also forms layer l-1's backward vectors - what
 * demf_bn_bwd_vectors(K, R, g12_prev, gamma_prev, ...) would: vec6_prev (5K), dgamma_prev, dbeta_prev,
 * g12_prev left zeroed.  store_flags != 0 (bf16 compute mode, BASELINE configs[3]): rows stored as bf16 -
 * bit 0: Yprev, bit 1: Y, G and dX (the pointers then address 2-byte elements); built for the two forms
 * of SA1's stack ((128,64) sparse with 3, (64,64) first_sums with 2), DEMF_EUNSUPPORTED otherwise.  Replaces the
 * autograd backward of Conv2d -> BatchNorm2d -> ReLU in mmdet3d's PointSAModule stacks
 * (configs/demf/demf_votenet.py:48-62; class_agnostic_vote_head.py:383). */
DEMF_INTERNAL int demf_mlp_bwd_fused(int R, int N, int K, const float* G, const float* dP, const int* arg, int ns,
                       const float* Y, const float* vec6, const float* W, const float* Yprev,
                       const float* scale_shift_prev, const float* mean_invstd_prev, float* dX,
                       float* dW, double* g12_prev, const float* X0, double* first_sums,
                       const float* gamma_prev, float* vec6_prev, float* dgamma_prev, float* dbeta_prev,
                       int store_flags, demf_stream_t stream);
/* The same pass over columns c0 .. c0 + Kc of a Ktot-channel layer l-1 (Kc = 64 / 128, (N, Kc) one of the
 * shapes above; dense row storage): Yprev, dX (R x Ktot), W, dW (N x Ktot), scale_shift_prev / mean_invstd_prev
 * (2 Ktot), g12_prev (2 Ktot) and the vector outputs are the WHOLE layer's; one call per column chunk. */
DEMF_INTERNAL int demf_mlp_bwd_fused_cols(int R, int N, int Ktot, int c0, int Kc, const float* G, const float* dP,
                            const int* arg, int ns, const float* Y, const float* vec6, const float* W,
                            const float* Yprev, const float* scale_shift_prev,
                            const float* mean_invstd_prev, float* dX, float* dW, double* g12_prev,
                            const float* gamma_prev, float* vec6_prev, float* dgamma_prev,
                            float* dbeta_prev, demf_stream_t stream);
/* What demf_mlp_bwd_fused_cols called for every 128-column chunk (c0 = 0, 128, ...) does, in ONE launch: N = 256,
 * Ktot in {256, 384, 512}.  A workgroup takes its chunk and its rows from its block id (csrc/wide_map.h): the
 * workgroups that walk the same rows of different chunks share an XCD's L2, there are Ktot/128 times fewer
 * workgroups (and dW partials) per chunk, and the launch's single last workgroup forms the backward vectors of all
 * Ktot channels of layer l-1.  Same argument contract and compute modes as demf_mlp_bwd_fused_cols. */
DEMF_INTERNAL int demf_mlp_bwd_fused_wide(int R, int N, int Ktot, const float* G, const float* dP, const int* arg, int ns,
                            const float* Y, const float* vec6, const float* W, const float* Yprev,
                            const float* scale_shift_prev, const float* mean_invstd_prev, float* dX,
                            float* dW, double* g12_prev, const float* gamma_prev, float* vec6_prev,
                            float* dgamma_prev, float* dbeta_prev, demf_stream_t stream);

/* Which kernel form the last shared-MLP launch of THIS thread took - a host-side record (no device work) set by the
 * forward / input-gradient dispatch of csrc/mlp.hip and by the one-pass backward entry points of csrc/mlp_bwd.hip.
 * For tests: from Python a dispatch condition that silently stops matching is invisible, the same entry point just
 * runs a slower kernel and every numeric check still passes. */
#define DEMF_FORM_NONE 0        /* no such launch on this thread yet */
#define DEMF_FORM_GENERIC 1     /* mlp_gemm_kernel (any prologue; also the pooled epilogue) */
#define DEMF_FORM_TILE 2        /* mlp_fwd_tile_kernel / mlp_dx_tile_kernel (few rows) */
#define DEMF_FORM_RES 3         /* mlp_fwd_res_kernel (weight-resident, 64-channel inputs) */
#define DEMF_FORM_PC 4          /* mlp_fwd_pc_kernel (producer / consumer, 128-channel inputs) */
#define DEMF_FORM_FUSED 5       /* mlp_bwd_fused_kernel through demf_mlp_bwd_fused / _x4 */
#define DEMF_FORM_FUSED_COLS 6  /* ... through demf_mlp_bwd_fused_cols: one launch per column chunk */
#define DEMF_FORM_FUSED_WIDE 7  /* ... through demf_mlp_bwd_fused_wide: one launch for all column chunks */
#define DEMF_FORM_POOL 8        /* mlp_bwd_pool_kernel (demf_mlp_bwd_pool) */
DEMF_INTERNAL int demf_mlp_last_form(void);

/* The library's A/B switches (csrc/switches.h), read from the environment ONCE per process at the first call that
 * needs one.  Entry ``index`` of the table: its environment name, the value this process runs with and the default
 * (any of the three pointers may be NULL).  DEMF_EINVAL past the end; no device work. */
DEMF_INTERNAL int demf_switch_at(int index, const char** name, int* value, int* dflt);

/* SA1-shaped stacks (4-float grouped rows -> N0 <= 64 channels -> ...): the first layer WITHOUT its (R x N0)
 * output.  y = x.W0^T is linear in the 16-byte row, so
 *   demf_mlp_first_stats      the layer's train-mode BN statistics + bookkeeping from the 14 second moments of the
 *                             rows (one pass over 16 MB instead of a GEMM writing 268 MB); ``moments``: >= 14
 *                             doubles of a zeroed accumulator, left zeroed;
 *   demf_mlp_gemm_fwd_bn_x4   the second layer (64 -> 64): demf_mlp_gemm_fwd_bn with its BN + ReLU prologue
 *                             fed by rows rebuilt from X4 and W0 (R >= 16384, compute modes 1 / 2);
 *   demf_mlp_bwd_fused_x4     the second layer's one-pass backward with the FIRST epilogue
 *                             (demf_mlp_bwd_fused, first_sums != NULL), likewise rebuilding layer 0's output.
 * mmdet3d PointSAModule's shared MLP at SA1 (configs/demf/demf_votenet.py:48-62).                          */
DEMF_INTERNAL int demf_mlp_first_stats(int R, int N0, const float* X, const float* W0, double* moments, const float* gamma,
                         const float* beta, float eps, float momentum, float* running_mean,
                         float* running_var, long long* num_batches_tracked, float* scale_shift,
                         float* mean_invstd, const float* conv_bias, demf_stream_t stream);
DEMF_INTERNAL int demf_mlp_gemm_fwd_bn_x4(int R, int N, const float* X4, const float* W0, const float* prev_scale_shift,
                            const float* Wt, float* Y, double* stats, const float* gamma, const float* beta,
                            float eps, float momentum, float* running_mean, float* running_var,
                            long long* num_batches_tracked, float* scale_shift, float* mean_invstd,
                            const float* conv_bias, demf_stream_t stream);
DEMF_INTERNAL int demf_mlp_bwd_fused_x4(int R, int N, int K, const float* G, const float* Y, const float* vec6,
                          const float* W, const float* X0, const float* W0, const float* scale_shift_prev,
                          const float* mean_invstd_prev, float* dW, double* first_sums, demf_stream_t stream);

/* Backward of a POOLED last layer without its (R x N) output (SA1: 537 MB neither written by the forward
 * nor read here).  With y = A.W^T and dY = gi*dZ + a*y + b (train-mode BN), A = act(Y_{L-1}):
 *     dA = (gi*dZ).W + A.(W^T diag(a) W) + b^T W,    dW = (gi*dZ)^T.A + diag(a) W (A^T A) + b (x) colsum(A)
 * - functions of A and of the sparse pooled gradient (dP at the selected rows ``arg``, gated by the ReLU on
 * ``yraw`` = the raw output at the selected row, from demf_pool_select_slot0) alone.
 * N = 128, K = 64, ns = 64, R % 64 == 0, compute modes 1 / 2.  dX (R x K), dW (N x K) written;
 * g12_prev (2K doubles, zeroed accumulator) accumulated and, with gamma_prev, turned into layer L-1's
 * backward vectors by the last workgroup.  workspace: *floats of demf_mlp_bwd_pool_ws(R, &floats), scratch.
 * Replaces demf_mlp_bwd_fused for that layer
 * (mmdet3d PointSAModule's shared MLP, demf/modeling/heads/class_agnostic_vote_head.py:383,
 * configs/demf/demf_votenet.py:48-62).                                                                  */
DEMF_INTERNAL int demf_mlp_bwd_pool_ws(int R, long long* floats);
DEMF_INTERNAL int demf_mlp_bwd_pool(int R, int N, int K, int ns, const float* dP, const int* arg, const float* yraw,
                      const float* vec6, const float* W, const float* Yprev,
                      const float* scale_shift_prev, const float* mean_invstd_prev, float* dX, float* dW,
                      double* g12_prev, const float* gamma_prev, float* vec6_prev, float* dgamma_prev,
                      float* dbeta_prev, float* workspace, demf_stream_t stream);

/* dW (N,K) += dY^T @ A_prev, A_prev = act_prev(Xprev (R,K; stride ldx)) or Xprev itself
 * when prev_scale_shift is NULL (first layer).  dW accumulated (fp32 atomics).        */
DEMF_INTERNAL int demf_mlp_gemm_bwd_dw(int R, int N, int K, int ldx, const float* G, const float* dP,
                         const int* arg, int ns, const float* Y, const float* vec6,
                         const float* Xprev, const float* prev_scale_shift, float* dW,
                         demf_stream_t stream);
/* Same with an explicit row stride of dW (>= K): the (N x K) result lands inside a wider weight
 * gradient (the feature columns 3.. of a set-abstraction level's first layer).                  */
DEMF_INTERNAL int demf_mlp_gemm_bwd_dw_ld(int R, int N, int K, int ldx, const float* G, const float* dP,
                            const int* arg, int ns, const float* Y, const float* vec6,
                            const float* Xprev, const float* prev_scale_shift, float* dW, int lddw,
                            demf_stream_t stream);

/* Several demf_mlp_gemm_bwd_dw_ld products in as few launches as their kernel variants allow (one per variant,
 * twelve jobs at a time).  Nothing in a backward depends on a layer's weight gradient, so a caller may queue the
 * jobs of many layers and issue them together once the operands exist; fields as the arguments of
 * demf_mlp_gemm_bwd_dw_ld. */
typedef struct demf_dw_job {
  int R, N, K, ldx;
  const float* G;
  const float* dP;
  const int* arg;
  int ns;
  const float* Y;
  const float* vec6;
  const float* Xprev;
  const float* prev_scale_shift;
  float* dW;
  int lddw;
} demf_dw_job;
DEMF_INTERNAL int demf_mlp_gemm_bwd_dw_group(int n, const demf_dw_job* jobs, demf_stream_t stream);

/* ------------------------------------------------------------------ *
 * Fused head losses: DeMFVoteHead._loss (class_agnostic_vote_head.py:622-712)
 * over the raw conv-head rows  cls (R,12) = [objectness 2 | semantic 10],
 * reg (R,30) = [centre offset 3 | size 3 | dir class 12 | dir residual 12]
 * (split_pred of coder.py:196-240 folded in); base_xyz (R,3) = aggregated points.
 * hyper12 (host floats) = objectness class weights (2), loss weights of objectness /
 * dir_class / dir_res / size / centre / semantic / iou (7), SmoothL1 betas of dir_res /
 * size / centre (3)   [configs/demf/demf_votenet.py:116-141].
 * out7 (accumulated) = the seven reduction='sum' losses in that order.
 * ------------------------------------------------------------------ */
DEMF_INTERNAL int demf_head_loss_fwd(int R, int num_dir_bins, int num_classes, const float* hyper12,
                       const float* cls, const float* reg, const float* base_xyz,
                       const float* center_t, const float* size_t_, const int64_t* dir_class_t,
                       const float* dir_res_t, const int64_t* sem_t, const int64_t* obj_t,
                       const float* obj_w, const float* box_w, float* out7,
                       demf_stream_t stream);
/* gradients wrt cls, reg, base_xyz given the seven upstream scalars grad_out7 (device).  */
DEMF_INTERNAL int demf_head_loss_bwd(int R, int num_dir_bins, int num_classes, const float* hyper12,
                       const float* cls, const float* reg, const float* base_xyz,
                       const float* center_t, const float* size_t_, const int64_t* dir_class_t,
                       const float* dir_res_t, const int64_t* sem_t, const int64_t* obj_t,
                       const float* obj_w, const float* box_w, const float* grad_out7,
                       float* grad_cls, float* grad_reg, float* grad_base,
                       demf_stream_t stream);

/* The distance form of the same: CAVoteHead.loss (class_agnostic_vote_head.py:40-121) of the points-only
 * class-agnostic VoteNet baseline (configs/baseline/votenet.py), with ClassAgnosticBBoxCoder.split_pred
 * (class_agnostic_bbox_coder.py:88-127) folded in.  reg (R,30) = [log-distance to the six box faces 6 |
 * dir class 12 | dir residual 12]; distance = exp(reg[0:6]).  distance_t (R,6) as demf_proposal_targets
 * writes it (unclamped; clamped at 0 here, class_agnostic_vote_head.py:301).  Terms: objectness CE,
 * SmoothL1 of the six distances (beta = hyper12[10], weight hyper12[5]), direction class / residual and
 * semantic CE as above, AxisAlignedIoULoss on the corners (ref - d[3:6], ref + d[0:3]) against those of the
 * targets - a function of the distances alone, so no reference point is read.
 * There is no centre term: hyper12[6] and hyper12[11] are ignored and out7[4] receives exact zeros, so the
 * seven-slot layout (and demf_loss_total / demf_scalars_accum / demf_step_meter behind it) is shared.     */
DEMF_INTERNAL int demf_ca_head_loss_fwd(int R, int num_dir_bins, int num_classes, const float* hyper12,
                       const float* cls, const float* reg, const float* distance_t,
                       const int64_t* dir_class_t, const float* dir_res_t, const int64_t* sem_t,
                       const int64_t* obj_t, const float* obj_w, const float* box_w, float* out7,
                       demf_stream_t stream);
/* gradients wrt cls (R,12) and reg (R,30) given the seven upstream scalars grad_out7 (device).
 * grad_ref (R,3), nullable: the gradient wrt the reference points.  The reference builds distance_t from the
 * proposal point without detaching it (class_agnostic_vote_head.py:271-294, clamp_ at :301), so the SmoothL1
 * and IoU terms reach the point through their TARGETS: d t[0:3] = -Rz(-yaw) d point, d t[3:6] = +Rz(-yaw) d point
 * where the unclamped target is >= 0.  dir_t (R), nullable = the assigned boxes' yaw (dir_targets of
 * demf_proposal_targets; NULL: no rotation).                                                             */
DEMF_INTERNAL int demf_ca_head_loss_bwd(int R, int num_dir_bins, int num_classes, const float* hyper12,
                       const float* cls, const float* reg, const float* distance_t,
                       const int64_t* dir_class_t, const float* dir_res_t, const int64_t* sem_t,
                       const int64_t* obj_t, const float* obj_w, const float* box_w,
                       const float* grad_out7, const float* dir_t, float* grad_cls, float* grad_reg,
                       float* grad_ref, demf_stream_t stream);

/* VoteModule.get_loss (called at class_agnostic_vote_head.py:641-644): chamfer-L1 of each
 * seed's vote against its gt_per_seed target votes, min over targets, weighted by
 * mask/(mask_sum+1e-6)*dst_weight.  grad_out == NULL: forward (out accumulated);
 * otherwise backward: grad_vote (B,S,3) written.                                  */
DEMF_INTERNAL int demf_vote_loss(int B, int S, int N, int gt_per_seed, float dst_weight,
                   const float* seed_points, const float* vote_points,
                   const int64_t* seed_indices, const int64_t* vote_target_masks,
                   const float* vote_targets, const float* mask_sum, const float* grad_out,
                   float* out, float* grad_vote, demf_stream_t stream);
/* forward of the same with the denominator counted in the kernel: mask_sum = sum over the seeds of
 * vote_target_masks[b, seed_indices[b, s]] (torch.gather(...).sum() of VoteModule.get_loss), stored to
 * mask_sum_out[0] for the backward call above; out[0] accumulated.                              */
DEMF_INTERNAL int demf_vote_loss_fwd(int B, int S, int N, int gt_per_seed, float dst_weight,
                       const float* seed_points, const float* vote_points,
                       const int64_t* seed_indices, const int64_t* vote_target_masks,
                       const float* vote_targets, float* mask_sum_out, float* out,
                       demf_stream_t stream);

/* ------------------------------------------------------------------ *
 * DeMF fusion: multi-scale deformable attention core
 * ------------------------------------------------------------------ */

/* MultiScaleDeformableAttnFunction.forward: reference call site
 * demf/modeling/layers/transformer.py:73 -> mmcv MultiScaleDeformableAttention
 * (config demf_votenet.py:79-85: H=8, L=4, P=2, Dh=32).
 * value (B,S,H,Dh), spatial_shapes (L,2) i64 (h,w), level_start_index (L) i64,
 * sampling_loc (B,Q,H,L,P,2) (x,y in [0,1]), attn_weight (B,Q,H,L,P)
 * -> out (B,Q,H*Dh).  Bilinear, align_corners=False, zero padding.  Any Dh >= 1
 * with S*H*Dh < 2^31, L <= 8, P >= 1.  Dh = 4 G with G in {1,2,4,8,16,32,64}
 * (Dh <= 256) and 16-byte aligned value / out run G lanes per (b,q,h); every
 * other Dh or alignment runs one thread per (b,q,h), serial over the channels. */
int demf_msda_fwd_f32(int B, int S, int H, int Dh, int L, int Q, int P,
                      const float* value, const int64_t* spatial_shapes,
                      const int64_t* level_start_index, const float* sampling_loc,
                      const float* attn_weight, float* out, demf_stream_t stream);

/* backward: grad_out (B,Q,H*Dh) -> grad_value (B,S,H,Dh) accumulated (NULL: not wanted, the
 * scatter is skipped), grad_sampling_loc (B,Q,H,L,P,2) and grad_attn_weight (B,Q,H,L,P) written. */
int demf_msda_bwd_f32(int B, int S, int H, int Dh, int L, int Q, int P,
                      const float* value, const int64_t* spatial_shapes,
                      const int64_t* level_start_index, const float* sampling_loc,
                      const float* attn_weight, const float* grad_out,
                      float* grad_value, float* grad_sampling_loc,
                      float* grad_attn_weight, demf_stream_t stream);

/* The same two entry points over bf16 VALUE rows (B,S,H,Dh) of 2-byte elements (the upper halves of the fp32
 * bit patterns): the gather - the dominant traffic of the operator - moves half the bytes; sampling locations,
 * weights, every accumulation, the output and all gradients (grad_value too: fp32, same layout) stay fp32.
 * BASELINE.json configs[3]: a bf16 image-token buffer halves the 152 MB token tensor. */
DEMF_INTERNAL int demf_msda_fwd_bf16(int B, int S, int H, int Dh, int L, int Q, int P,
                       const uint16_t* value, const int64_t* spatial_shapes,
                       const int64_t* level_start_index, const float* sampling_loc,
                       const float* attn_weight, float* out, demf_stream_t stream);
DEMF_INTERNAL int demf_msda_bwd_bf16(int B, int S, int H, int Dh, int L, int Q, int P,
                       const uint16_t* value, const int64_t* spatial_shapes,
                       const int64_t* level_start_index, const float* sampling_loc,
                       const float* attn_weight, const float* grad_out,
                       float* grad_value, float* grad_sampling_loc,
                       float* grad_attn_weight, demf_stream_t stream);

/* ---- the frozen image stream's encoder layers --------------------------------------------- *
 * Long-row linear layer: C (R,N; ldc) = epi((A [+ A2 on output columns < a2_cols]) . W^T + bias), R ~ 150 000
 * token rows, K % 32 == 0, N % 128 == 0.  W arrives PRE-SPLIT as bf16 planes (planes, N, K): planes = 3 is
 * fp32-grade arithmetic (w = h + m + l exactly, six products per term pair on the bf16 matrix cores, as
 * compute mode 2 of the demf_mlp_gemm_* kernels), planes = 1 the bf16 compute mode; the A rows are fp32 and are
 * split inside the kernel.  mode 0: bias; rows with row_mask[r] != 0 are zeroed in columns >= mask_col0 (the
 * padding mask of value_proj); mode 1: bias + ReLU; mode 2 (N == 256): LayerNorm(resid + A.W^T + bias) * gamma +
 * beta.  Replaces, per encoder layer of demf/modeling/layers/deform_detr_encoder.py:68-154, six library GEMMs
 * and the elementwise launches between them (query + pos, masked_fill, ReLU, residual adds, two LayerNorms).  */
DEMF_INTERNAL int demf_rows_gemm_f32(int R, int N, int K, const float* A, long long lda, const float* A2, int a2_cols,
                       int a2_op /* 0: A + A2 on those columns, 1: A2 INSTEAD of A (a pre-added operand) */,
                       const void* w_planes, int planes, const float* bias, int mode,
                       const unsigned char* row_mask, int mask_col0, const float* resid, long long ldr,
                       const float* gamma, const float* beta, float eps, float* C, long long ldc,
                       demf_stream_t stream);
/* y = LayerNorm(resid + x) * gamma + beta over rows of C = 256 channels (gamma == beta == NULL: y = resid + x) and
 * ypos = y + pos; y or ypos may be NULL.  The FFN tail of an encoder layer and the `query + query_pos` of the next
 * layer's attention (mmcv MultiScaleDeformableAttention.forward) in one pass.                                    */
DEMF_INTERNAL int demf_rows_ln_pos_f32(int R, int C, const float* x, const float* resid, const float* gamma, const float* beta,
                         float eps, const float* pos, float* y, float* ypos, demf_stream_t stream);
/* Multi-scale deformable attention forward with RAW inputs: offsets (H*L*P*2 columns from off_col0) and attention
 * logits (H*L*P columns from lgt_col0) of row b*Q+q of `raw` (row stride ldraw), reference points ref (B,Q,L,2),
 * value rows of pitch vpitch floats (columns h*Dh.. of the same projection output).  The softmax over a head's
 * L*P logits and loc = ref + offset / (W_l, H_l) - separate elementwise launches in mmcv's
 * MultiScaleDeformableAttention.forward - happen on the way in.  Dh = 32, L = 4, P in {2, 4}. -> out (B,Q,H*Dh) */
DEMF_INTERNAL int demf_msda_fwd_raw_f32(int B, int S, int H, int Dh, int L, int Q, int P, const float* value,
                          long long vpitch, const int64_t* spatial_shapes, const int64_t* level_start_index,
                          const float* raw, long long ldraw, int off_col0, int lgt_col0, const float* ref,
                          float* out, demf_stream_t stream);
/* The same for H = 8, Dh = 32, L = 4 with the value rows of levels first_staged_level (2 or 3) .. 3 of one (scene, head)
 * resident in LDS: staged_tokens = S - level_start_index[first_staged_level], known to the caller on the host (the
 * library never reads a device array back); staged_tokens * 128 B + 8 KB * P / 2 ... must fit 160 KB or the call is
 * refused.  Results equal demf_msda_fwd_raw_f32's up to the summation order of a query's samples (Q = S rows). */
DEMF_INTERNAL int demf_msda_fwd_raw_head_f32(int B, int S, int Q, int P, const float* value, long long vpitch,
                               const int64_t* spatial_shapes, const int64_t* level_start_index, const float* raw,
                               long long ldraw, int off_col0, int lgt_col0, const float* ref, float* out,
                               int first_staged_level, int staged_tokens, demf_stream_t stream);

/* Per-point vote targets of DeMFVoteHead.get_targets_single (class_agnostic_vote_head.py:828-858),
 * batched: points (B,N,point_stride>=3), gt_boxes (B,G,7) = (x,y,z_bottom,dx,dy,dz,yaw) padded to
 * G <= 64 with valid (B,G) bytes, cos/sin of -yaw (B,G) -> vote_targets (B,N,9) = votes to the
 * gravity centres of the first | second-or-first | last-or-first containing box, zeros outside
 * every box; vote_target_masks (B,N) int64 = inside any box.                                  */
DEMF_INTERNAL int demf_vote_targets(int B, int N, int point_stride, int G, const float* points,
                      const float* gt_boxes, const float* cos_neg_yaw, const float* sin_neg_yaw,
                      const unsigned char* valid, float* vote_targets, int64_t* vote_target_masks,
                      demf_stream_t stream);

/* Per-proposal targets of DeMFVoteHead.get_targets_single (class_agnostic_vote_head.py:877-934),
 * batched over scenes: nearest valid ground-truth centre (first minimum of the squared distance),
 * the gathered centre / size / direction / class targets, the distance targets in the box frame
 * (rotation by -yaw when with_rot) and objectness label + mask (pos/neg distance thresholds).
 * gt_dir_class / gt_dir_res = bbox_coder.angle2class(yaw) per box; res_scale = pi/num_dir_bins.  */
DEMF_INTERNAL int demf_proposal_targets(int B, int Q, int G, int with_rot, float pos_thr, float neg_thr,
                          float res_scale, const float* aggregated_points, const float* gt_boxes,
                          const float* cos_neg_yaw, const float* sin_neg_yaw,
                          const int64_t* gt_dir_class, const float* gt_dir_res,
                          const int64_t* gt_labels, const unsigned char* valid,
                          float* center_targets, float* size_targets, int64_t* dir_class_targets,
                          float* dir_res_targets, float* dir_targets, int64_t* mask_targets,
                          float* distance_targets, int64_t* objectness_targets,
                          float* objectness_masks, demf_stream_t stream);

/* Position-embedding input of a fusion decoder layer from a prediction head's raw regression rows
 * (reg_rows (R, nreg >= 6) point-major, base_xyz (R,3)): out8 (R,8) = [base + reg[0:3] | reg[3:6] | 0 0] -
 * the reference's torch.cat([center, size], -1).detach() (class_agnostic_vote_head.py:497-498), padded
 * to the 8 columns the first GEMM of the position embedding stages.                                  */
DEMF_INTERNAL int demf_query_pos_rows(int R, int nreg, const float* reg_rows, const float* base_xyz, float* out8,
                        demf_stream_t stream);

/* Tail of DeMFVoteHead.loss (class_agnostic_vote_head.py:604-612: the losses of the num_fusion_layers + 1
 * decode results are averaged, the training loop sums the dict): vecs[0..n) are the (7,) per-decode-layer
 * loss vectors, vote the (1,) vote loss or NULL -> out8 = [mean of the vectors (7) | their sum + vote].
 * n <= 4.  demf_loss_total_bwd: g8 = gradient of out8 -> gvecs (n,7) = (g8[i] + g8[7]) / n, gvote = g8[7]. */
DEMF_INTERNAL int demf_loss_total(int n, const float* const* vecs, const float* vote, float* out8, demf_stream_t stream);
DEMF_INTERNAL int demf_loss_total_bwd(int n, const float* g8, float* gvecs, float* gvote, demf_stream_t stream);

/* Per-scene ground-truth lists -> the static-shape padded form the target kernels read: gt_padded
 * (B,G,7) fp32, labels_padded (B,G) int64 with -1 on padding slots, valid (B,G) u8 or NULL.  An empty
 * scene gets the reference's single all-zero fake box with label 0
 * (demf/modeling/heads/class_agnostic_vote_head.py:766-773).  counts / box_dims / boxes / labels are
 * HOST arrays of length B (<= 32): scene b's device pointers to its (counts[b], box_dims[b] >= 7) fp32
 * box rows and (counts[b]) int64 labels; they travel by value in the kernel arguments, so the call
 * issues one launch and no host -> device copy.                                                      */
DEMF_INTERNAL int demf_pad_gt(int B, int G, const int* counts, const int* box_dims, const void* const* boxes,
                const void* const* labels, float* gt_padded, int64_t* labels_padded,
                unsigned char* valid, demf_stream_t stream);

/* Everything the two target kernels need that depends on the padded ground truth alone (label -1 =
 * padding slot), one launch: cos/sin(-yaw), PartialBinBasedBBoxCoder.angle2class(yaw) in torch's
 * fp32 remainder / floor-divide semantics (class_agnostic_vote_head.py:877-883 via
 * bbox_coder.encode), valid = label >= 0, labels clamped at 0, gravity centres (B,G,3).           */
DEMF_INTERNAL int demf_gt_prep(int B, int G, int num_dir_bins, const float* gt_boxes, const int64_t* labels_padded,
                 float* cos_neg_yaw, float* sin_neg_yaw, int64_t* gt_dir_class, float* gt_dir_res,
                 unsigned char* valid, int64_t* labels_clamped, float* gravity_center,
                 demf_stream_t stream);

/* objectness_weights = masks / (sum + 1e-6), box_loss_weights = objectness / (sum + 1e-6) over all
 * R = B*Q proposals (class_agnostic_vote_head.py:797-816).                                          */
DEMF_INTERNAL int demf_target_weights(int R, const float* objectness_masks, const int64_t* objectness_targets,
                        float* objectness_weights, float* box_loss_weights, demf_stream_t stream);

/* ------------------------------------------------------------------ *
 * Test-time post-processing: DeMFVoteHead.get_bboxes (class_agnostic_vote_head.py:714-754) +
 * the inherited mmdet3d VoteHead.multiclass_nms_single / aligned_3d_nms.
 * ------------------------------------------------------------------ */

/* boxes7 (B,K,7) = decode() output (gravity centre, size, yaw) with cos/sin(yaw) (B,K) ->
 * boxes_bottom (B,K,7) upstream's bottom-centre form, extent6 (B,K,6) = min|max over the 8 rotated
 * corners, count (B,K) = scene points inside the box (points (B,N,point_stride>=3)).           */
DEMF_INTERNAL int demf_box_extent_count(int B, int N, int point_stride, int K, const float* points,
                          const float* boxes7, const float* cos_yaw, const float* sin_yaw,
                          float* boxes_bottom, float* extent6, int* count, demf_stream_t stream);

/* aligned_3d_nms per scene over the boxes with valid != 0 (K <= 1024): descending score order, a
 * kept box removes same-class boxes with IoU > iou_thr.  keep (B,K) bytes.                     */
DEMF_INTERNAL int demf_aligned_nms(int B, int K, float iou_thr, const float* extent6, const float* scores,
                     const int64_t* classes, const unsigned char* valid, unsigned char* keep,
                     demf_stream_t stream);

/* One ensemble layer of DeMFVoteHead.get_bboxes (class_agnostic_vote_head.py:714-754) as the decode reads it:
 * every field is a (B, K, n) array with a unit last stride, given by pointer, batch stride (_sb) and row
 * stride (_sk) in floats - the views of the raw conv-head rows go in as they are.  center_base != NULL:
 * center = center_base + center (class_agnostic_bbox_coder.py:214, base_xyz + reg[..., 0:3]);
 * dir_res is multiplied by res_scale (1, or pi / num_dir_bins for dir_res_norm, :233).                     */
typedef struct demf_detect_layer {
  int K;
  float res_scale;
  const float* center; int center_sb, center_sk;
  const float* center_base; int base_sb, base_sk;
  const float* size; int size_sb, size_sk;
  const float* dir_class; int dir_class_sb, dir_class_sk;
  const float* dir_res; int dir_res_sb, dir_res_sk;
  const float* obj; int obj_sb, obj_sk;
  const float* sem; int sem_sb, sem_sk;
} demf_detect_layer;

#define DEMF_DETECT_MAX_LAYERS 8
/* Decode + score of get_bboxes (class_agnostic_vote_head.py:714-733) for L <= DEMF_DETECT_MAX_LAYERS ensemble layers (HOST array)
 * in one launch, in the concatenated (B, K = sum K_l) layout: box7 (B,K,7) = the coder's decode (gravity
 * centre, size, yaw in [0, 2pi)), cos_yaw / sin_yaw (B,K), obj (B,K) = softmax(obj_scores)[..., 1],
 * sem (B,K,C) = softmax(sem_scores), classes (B,K) = argmax(sem).  K > 1024 returns DEMF_EUNSUPPORTED.   */
DEMF_INTERNAL int demf_detect_decode(int B, int K, int L, int C, int num_dir_bins, int with_rot,
                       const demf_detect_layer* layers, float* box7, float* cos_yaw, float* sin_yaw,
                       float* obj, float* sem, int64_t* classes, demf_stream_t stream);

/* The distance form of the same for the one layer of CAVoteHead: ClassAgnosticBBoxCoder.decode
 * (class_agnostic_bbox_coder.py:42-86) + the scoring of mmdet3d VoteHead.get_bboxes, straight from the raw
 * conv-head rows reg (B,K,6+2*num_dir_bins) / cls (B,K,2+C) and the reference points ref (B,K,3), each given
 * by pointer, batch stride (_sb) and row stride (_sk) in floats, unit last stride.  d = exp(reg[0:6]);
 * yaw = class2angle(argmax dir_class, dir_res_norm[argmax] * pi / num_dir_bins) mod 2pi (0 without rotation);
 * size = max(d[0:3] + d[3:6], 0.1); centre = ref - Rz(yaw) . (d[3:6] - d[0:3]) / 2 with mmdet3d's
 * rotation_3d_in_axis(axis=2) convention (x c + y s, -x s + y c).  Outputs as demf_detect_decode.        */
DEMF_INTERNAL int demf_ca_detect_decode(int B, int K, int C, int num_dir_bins, int with_rot,
                       const float* reg, int reg_sb, int reg_sk, const float* cls, int cls_sb, int cls_sk,
                       const float* ref, int ref_sb, int ref_sk, float* box7, float* cos_yaw,
                       float* sin_yaw, float* obj, float* sem, int64_t* classes, demf_stream_t stream);

/* Selection of get_bboxes (class_agnostic_vote_head.py:735-754; mmdet3d multiclass_nms_single's
 * per_class_proposal branch) into a detection store: survivors = keep & (obj > score_thr).  Scene b of the batch
 * becomes store scene first_scene + b; its rows start at scene_off[first_scene] + the rows of the batch's
 * earlier scenes and are class-major, proposal index ascending inside a class, score = obj * sem[c], label = c
 * (per_class = 0: one row per survivor, score = obj, label = classes).  Writes scene_off[first_scene + 1 ..
 * first_scene + B], state[0] = scene_off[first_scene + B] (rows needed so far) and, if a row index reaches
 * max_rows, state[1] = 1; such rows are counted but not written.  boxes (max_rows,7) bottom-centre, scores
 * (max_rows), labels (max_rows) int32, scene_off (max_scenes + 1).  K > 1024 returns DEMF_EUNSUPPORTED.  */
DEMF_INTERNAL int demf_detect_pack(int B, int K, int C, int per_class, float score_thr,
                     const unsigned char* keep, const float* obj, const float* sem, const int64_t* classes,
                     const float* boxes_bottom, int first_scene, int max_scenes, int max_rows, float* boxes,
                     float* scores, int* labels, int* scene_off, int* state, demf_stream_t stream);

/* ------------------------------------------------------------------ *
 * Indoor detection evaluation (csrc/eval3d.hip): mmdet3d 0.18.1 indoor_eval as SUNRGBDDataset.evaluate
 * calls it for `eval.py --eval mAP` (configs/_base_/datasets/sunrgbd-3d-10class.py:107).
 * Boxes are the bottom-centre form (x, y, z_bottom, dx, dy, dz, yaw); IoU arithmetic fp32.
 * ------------------------------------------------------------------ */

/* iou (N,M) = BaseInstance3DBoxes.overlaps(boxes1 (N,7), boxes2 (M,7), mode='iou') of depth boxes: rotated
 * footprint intersection x height overlap / max(vol1 + vol2 - inter, 1e-8).                              */
DEMF_INTERNAL int demf_box3d_iou(int N, int M, const float* boxes1, const float* boxes2, float* iou,
                   demf_stream_t stream);

/* Greedy matching of eval_det_cls over S (class, scene) segments.  Segment s: the detections
 * order[pred_off[s] .. pred_off[s+1]) (caller rows of pred_boxes, score-descending) and the ground truth
 * gt_boxes rows gt_off[s] .. gt_off[s+1) in that scene's order.  thresholds: T <= 4 IoU thresholds in HOST
 * memory.  tp (P,T) bytes in the caller's row order: 1 iff the row's best GT (first maximum) has
 * IoU > threshold and no earlier detection of the segment took it.  max_pred / max_gt: the largest segment;
 * above DEMF_EVAL_MAX_PRED_PER_SEGMENT detections or DEMF_EVAL_MAX_GT_PER_SEGMENT GT the call returns
 * DEMF_EUNSUPPORTED.                                                                                      */
#define DEMF_EVAL_MAX_PRED_PER_SEGMENT 4096
#define DEMF_EVAL_MAX_GT_PER_SEGMENT 256
DEMF_INTERNAL int demf_eval_match(int S, int T, const float* thresholds, int max_pred, int max_gt,
                    const float* pred_boxes, const int* order, const int* pred_off, const float* gt_boxes,
                    const int* gt_off, unsigned char* tp, demf_stream_t stream);

/* VOC-area average precision and final recall per (class, threshold) -> ap, rec (C,T) doubles.  tp_sorted
 * (P,T) bytes: class c's flags are rows cls_off[c] .. cls_off[c+1) in that class's global score order.
 * npos (C): ground-truth count per class (0 -> NaN, upstream's 0/0); ws_off (C+1): prefix sums of npos;
 * workspace: ws_off[C] * T ints.  tp_sorted / workspace may be null when they hold no element.            */
DEMF_INTERNAL int demf_eval_ap(int C, int T, const int* cls_off, const int* npos, const int* ws_off,
                 const unsigned char* tp_sorted, int* workspace, double* ap, double* rec, demf_stream_t stream);

/* ------------------------------------------------------------------ *
 * Test-time augmentation (csrc/tta.hip).  The reference's forward_test hands num_augs > 1 to self.aug_test
 * (demf/modeling/detectors/demfnet.py:236-238), which it inherits from a class whose members it lacks; mmdet3d
 * 0.18.1 builds that method from merge_aug_bboxes_3d: bbox3d_mapping_back per view, concatenation, a per-class
 * iou3d.nms_gpu (rotated BEV) or nms_normal_gpu (axis-aligned BEV), and a score-ordered cut [dep-recall].
 * Boxes are the bottom-centre form; arithmetic fp32; footprints are those of demf_box3d_iou.
 * mode: 0 rotated BEV IoU, 1 axis-aligned BEV IoU of centre +- (dx, dy) / 2 (yaw ignored), 2 rotated 3-D IoU;
 * iou = overlap / max(a + b - overlap, 1e-8); a footprint with dx * dy == 0 overlaps nothing (rotated modes).
 * ------------------------------------------------------------------ */

/* Segmented greedy NMS.  Segment s = rows seg_start[s] .. seg_start[s] + seg_count[s] of boxes (R,7) / scores (R)
 * (seg_start, seg_count: S ints on the DEVICE).  Candidates are the rows with valid != 0 (valid may be NULL: all)
 * whose score is neither NaN nor -inf, visited in score order (descending; ties: the lower row first); a visited
 * candidate that is still alive is kept and removes every alive candidate with !(iou <= thr), so NaN removes.
 * keep (R) bytes: 0 / 1 for the rows of every segment; rows outside every segment are not written.  n_max: the host's
 * bound on seg_count, at most DEMF_NMS_MAX_SEGMENT (beyond: DEMF_EUNSUPPORTED, nothing launched).  A segment whose count exceeds
 * n_max on the device, or whose rows leave [0, R), sets *overflow = 1 and none of its keep bytes is written.      */
#define DEMF_NMS_MAX_SEGMENT 1024
DEMF_INTERNAL int demf_nms_bev(int R, int S, int n_max, float thr, int mode, const float* boxes, const float* scores,
                 const int* seg_start, const int* seg_count, const unsigned char* valid, unsigned char* keep,
                 int* overflow, demf_stream_t stream);

/* The merge of a batch's views (merge_aug_bboxes_3d).  View store = the arrays of a DetectionStore whose scene
 * first_view_scene + v * B + b is view v of batch scene b (view-major), written by demf_detect_pack with at most
 * K rows per class and scene; params (V * B, 8) = the rows of demf_points_prep in the same order.  Per (scene, class):
 * the rows of that label are gathered over the views in (view, row) order and mapped back by the inverse of their
 * parameter row (centre -= t; [:6] /= scale; centre turned by -angle, yaw += angle; then, if flipped, x -> -x and
 * yaw -> pi - yaw); demf_nms_bev over the B * C segments; per scene the kept rows ordered by (score descending,
 * class, view, row ascending), cut at max_num and appended to the destination arrays with demf_detect_pack's
 * protocol (cursor read at scene_off[first_scene]; scene_off[first_scene + b + 1] and state[0] written; state[1] = 1
 * when rows do not fit, when a segment holds more than V * K rows, or when view_state[1] (may be NULL) is set; rows at
 * or beyond max_rows are not written).  Workspace: ws_boxes (B*C*V*K, 7), ws_scores (B*C*V*K), ws_seg (2*B*C + 1)
 * ints, ws_keep (B*C*V*K) bytes.  Three launches whatever the sizes, no host sync.  V * K > DEMF_NMS_MAX_SEGMENT or
 * V * K * C > DEMF_TTA_MAX_CANDIDATES returns DEMF_EUNSUPPORTED with nothing launched.                            */
#define DEMF_TTA_MAX_CANDIDATES 16384
DEMF_INTERNAL int demf_tta_merge(int B, int V, int C, int K, float thr, int mode, int max_num, const float* view_boxes,
                   const float* view_scores, const int* view_labels, const int* view_scene_off,
                   const int* view_state, int first_view_scene, int view_max_scenes, int view_max_rows,
                   const float* params, float* ws_boxes, float* ws_scores, int* ws_seg, unsigned char* ws_keep,
                   int first_scene, int max_scenes, int max_rows, float* boxes, float* scores, int* labels,
                   int* scene_off, int* state, demf_stream_t stream);

/* ------------------------------------------------------------------ *
 * Input pipeline of SUN RGB-D scenes (csrc/pipeline.hip): the per-point and per-pixel steps of the training /
 * test pipelines of configs/demf/demf_votenet.py:184-216 (mmdet3d 0.18.1 / mmcv transforms).  Scenes are
 * ragged: `offsets` (B+1) int64 DEVICE arrays into the concatenated raw buffers; `total` / `src_bytes` is the
 * size of that buffer (points / bytes), and a scene whose offsets fall outside it, or that is empty, yields NaN
 * (points) or padding (image) instead of a read out of bounds.
 * ------------------------------------------------------------------ */

/* LoadPointsFromFile(shift_height=True, load_dim=6) (demf_votenet.py:186-190): floor (B) = np.percentile(z, 0.99) of
 * each scene's whole raw cloud - numpy's linear interpolation between the order statistics of rank
 * floor(0.0099 (N-1)) and the next - from raw (total, load_dim) float32 records, z in column 2.               */
DEMF_INTERNAL int demf_points_floor(int B, int load_dim, long long total, const float* raw, const int64_t* offsets,
                      float* floor_out, demf_stream_t stream);

/* RandomFlip3D + GlobalRotScaleTrans(shift_height=True) + PointSample(num_points) (demf_votenet.py:198-207) on the raw
 * records: out (B, num_points, 4) = (xyz flipped (x -> -x), rotated by +angle about z, scaled, translated | (z_raw -
 * floor) * scale).  params (B, 8) fp32 = [flip, cos, sin, scale, tx, ty, tz, unused]; seeds (B) int64.  Source of
 * point j: with N >= num_points a keyed random permutation of [0, N) (without replacement, random order), else
 * iid indices (with replacement), as np.random.choice(N, num_points, replace=N < num_points).  src_index
 * (B, num_points) int32 or NULL.                                                                                  */
DEMF_INTERNAL int demf_points_prep(int B, int num_points, int load_dim, long long total, const float* raw,
                     const int64_t* offsets, const float* floor_in, const float* params, const int64_t* seeds,
                     float* out, int* src_index, demf_stream_t stream);

/* Resize(img_scale, keep_ratio) + Normalize(to_rgb) + Pad(size_divisor=32) + collate padding (demf_votenet.py:192-197):
 * src = uint8 HWC RGB images at byte offsets, shapes (B, 4) int32 = (h_in, w_in, h_out, w_out) (DEVICE), mean_std =
 * 6 HOST floats (mean RGB, std RGB) -> out (B, 3, Hp, Wp) fp32, every element written (padding 0).  Bilinear with
 * cv2 INTER_LINEAR's source coordinates, the resized value rounded to uint8 before normalising.  Wp % 4 == 0.     */
DEMF_INTERNAL int demf_image_prep(int B, int Hp, int Wp, long long src_bytes, const unsigned char* src,
                    const int64_t* offsets, const int* shapes, const float* mean_std, float* out,
                    demf_stream_t stream);

/* ------------------------------------------------------------------ *
 * RGB-D frame front end (csrc/frame.hip): what the SUN RGB-D toolbox's offline export does per pixel (unproject the
 * depth image, apply the tilt matrix) [dep-recall], so that a raw frame can take the place of a scene's `.bin`.
 * B ragged frames: depth = their row-major uint16 images concatenated (`total` pixels, depth_off (B+1) int64 pixel
 * offsets), rgb / rgb_off / shapes = the buffers of demf_image_prep (shapes (B,4) int32, the first two read as h, w),
 * calib (B,16) fp64 = [fx, fy, cx, cy, Rt row-major (9), pixel_origin, depth_scale, z_max]; all DEVICE arrays.
 * Pixel (row v, column u), fp64, one IEEE operation at a time (no contraction):
 *   d' = d rotated right by `shift` in 16 bits; the pixel is valid iff d' != 0
 *   z  = min(d' / depth_scale, z_max);  x3 = ((u + pixel_origin) - cx) * z / fx;  y3 = ((v + pixel_origin) - cy) * z / fy
 *   c  = (x3, z, -y3);  p_i = (Rt[i][0] c0 + Rt[i][1] c1) + Rt[i][2] c2
 *   record = fp32(p_0), fp32(p_1), fp32(p_2), fp32(r) / 255, fp32(g) / 255, fp32(b) / 255
 * raw (total, 6) fp32 receives the records of the valid pixels only, frames in order and row-major inside a frame;
 * rows at or beyond offsets[B] are not written.  offsets (B+1) int64 (DEVICE): offsets[b+1] - offsets[b] = frame b's
 * valid pixels - the (raw, offsets) pair of demf_points_floor / demf_points_prep.  A frame whose table entries do
 * not lie inside the buffers has no valid pixel.  tile_counts: ntiles = ceil(total / DEMF_FRAME_TILE) ints of
 * scratch.  Two launches, no atomics: the result is bit-identical from run to run.                                */
#define DEMF_FRAME_TILE 1024
DEMF_INTERNAL int demf_depth_to_points(int B, long long total, long long rgb_bytes, int shift,
                         const unsigned short* depth, const int64_t* depth_off, const unsigned char* rgb,
                         const int64_t* rgb_off, const int* shapes, const double* calib, int ntiles,
                         int* tile_counts, float* raw, int64_t* offsets, demf_stream_t stream);

/* ------------------------------------------------------------------ *
 * Optimizer step on flat buffers: torch.optim.AdamW + clip_grad_norm_ as the reference's
 * runner applies them (configs/_base_/schedules/schedule_3x.py:6-7: AdamW lr 0.008, wd 0.01,
 * grad_clip max_norm 10; configs/demf/demf_votenet.py:16-24: 'decoder' lr_mult 0.05).  One call
 * per parameter group.  g_eff = grad * grad_scale * min(1, max_norm / (norm*grad_scale + 1e-6))
 * with norm read from the device scalar grad_norm (NULL: no clipping); grad itself is not
 * modified.  step is the 1-based step count (bias correction).
 * ------------------------------------------------------------------ */
DEMF_INTERNAL int demf_adamw_f32(long long n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                   const float* grad_norm, float max_norm, float grad_scale, float lr, float beta1,
                   float beta2, float eps, float weight_decay, int step, demf_stream_t stream);

/* The same update with its state ON THE DEVICE, so that norm + clip + AdamW are nodes of the step's
 * hipGraph (nothing the host passes changes between replays).  `opt_state`: one zero-initialised demf_opt_state.
 * sumsq = squared L2 norm of the gradients of ALL groups, accumulated by demf_multi_copy_sumsq (the
 * gradient pack of a captured step) or demf_sumsq_f32 and cleared by demf_adamw_state_f32; t = completed
 * steps (the launch uses t + 1 for the bias corrections and publishes it from its last workgroup);
 * lr_factor multiplies every group's learning rate (the reference's step schedule,
 * configs/_base_/schedules/schedule_3x.py:7-9).  Up to 4 parameter groups (segments [start, start + n) of
 * the flat buffers, HOST arrays) in ONE launch; max_norm <= 0: no clipping.                            */
typedef struct demf_opt_state {
  double sumsq;
  long long t;
  unsigned ticket;    /* last-workgroup detection of the AdamW launch */
  float lr_factor;
  int reserved[10];   /* to 64 bytes */
} demf_opt_state;
DEMF_INTERNAL int demf_multi_copy_sumsq(int n, const void* table, int blocks_per_segment, void* opt_state,
                          demf_stream_t stream);
DEMF_INTERNAL int demf_sumsq_f32(long long n, const float* x, void* opt_state, demf_stream_t stream);
DEMF_INTERNAL int demf_adamw_state_f32(int nseg, const long long* seg_start, const long long* seg_n, const float* seg_lr,
                         const float* seg_weight_decay, float* param, const float* grad, float* exp_avg,
                         float* exp_avg_sq, void* opt_state, float max_norm, float grad_scale, float beta1,
                         float beta2, float eps, demf_stream_t stream);

/* Step meter (csrc/meter.hip): one record per optimizer step in a device-resident ring of `rows` rows, written
 * by one wave between the launch that completes opt_state.sumsq and the demf_adamw_state_f32 launch that clears
 * it (same stream, or a node of the same hipGraph).  Row t % rows, 16 words of 4 bytes:
 *   word 0-1  int64  t           opt_state.t at the launch = optimizer steps completed before this one (the stamp)
 *   word 2    uint32 flags       bit i (i < 10): scalar i is NaN or +-Inf; DEMF_METER_FLAG_GRAD_NORM: grad_norm is
 *   word 3    float  lr_factor   opt_state.lr_factor
 *   word 4    float  grad_norm   (float)sqrt(sumsq) * grad_scale: the norm before clipping (mmcv's `grad_norm`)
 *   word 5    float  clip        min(1, max_norm / (grad_norm + 1e-6)), the expression of demf_adamw_state_f32
 *                                (1 when max_norm <= 0)
 *   word 6-15 float  scalar 0 .. n-1 as read (non-finite values included), 0 in the unused slots
 * scalars: HOST array of n (1..10) DEVICE pointers to single floats, anywhere (views into a loss vector are
 * fine); they are passed by value in the kernel arguments.  grad_scale / max_norm: the values the AdamW launch
 * of the same step gets.  The launch only reads opt_state; every other row of the ring is left alone.        */
#define DEMF_METER_ROW_WORDS 16
#define DEMF_METER_HEAD_WORDS 6
#define DEMF_METER_MAX_SCALARS 10
#define DEMF_METER_FLAG_GRAD_NORM (1u << 16)
DEMF_INTERNAL int demf_step_meter(int n, const float* const* scalars, const void* opt_state, float grad_scale,
                    float max_norm, void* ring, int rows, demf_stream_t stream);

/* Gradient accumulation (csrc/accum.hip): W forward + backward passes feed ONE optimizer step, the reference's
 * 8-rank step (tools/dist_train.sh:4) on one GPU.  The flat gradient buffer is zero between optimizer steps; every
 * pass ADDS its gradients into it, the last pass takes the norm of the sum on its way, and demf_adamw_state_f32
 * gets grad_scale = 1 / (W * world).
 * demf_multi_add: the table, launch geometry and vector / scalar paths of demf_multi_copy (3 x n int64 DEVICE table
 *   src | dst | words, grid (blocks_per_segment, n), 256 threads, 16-byte loads and stores with a 4q tail when
 *   source and destination both sit on 16 bytes), computing dst[j] = dst[j] + src[j] in fp32 (one correctly rounded
 *   add).  A null source adds nothing: dst is NOT written (demf_multi_copy zero-fills there).  n <= 65535.
 * demf_multi_add_sumsq: the same, plus the sum of squares of every STORED sum added to opt_state.sumsq as
 *   demf_multi_copy_sumsq adds it (fp32 partial per thread, fp64 wave / workgroup reduction, one fp64 atomic per
 *   workgroup, none when the partial is 0).  A null-source segment is read and its squares counted: sumsq is the
 *   squared norm of the whole accumulated buffer the table covers, not of this pass's share.
 * demf_scalars_accum: acc[i] = acc[i] + scale * *scalars[i] for i < n (1..DEMF_METER_MAX_SCALARS), one wave, plain
 *   stores, no atomics; scalars as demf_step_meter takes them (HOST array of DEVICE pointers, passed by value in
 *   the kernel arguments), acc = n contiguous DEVICE floats.  NOT contracted: the product is rounded to fp32, then
 *   the sum is (no fmaf; the library is built with -ffp-contract=off).  With scale = 1/W over the W passes of a
 *   group, acc holds the group's mean loss terms, which demf_step_meter then reads as its scalars.          */
DEMF_INTERNAL int demf_multi_add(int n, const void* table, int blocks_per_segment, demf_stream_t stream);
DEMF_INTERNAL int demf_multi_add_sumsq(int n, const void* table, int blocks_per_segment, void* opt_state,
                         demf_stream_t stream);
DEMF_INTERNAL int demf_scalars_accum(int n, const float* const* scalars, float* acc, float scale,
                       demf_stream_t stream);

/* ------------------------------------------------------------------ *
 * Rank merges (csrc/ranks.hip): the device state of W data-parallel ranks, ALREADY GATHERED into rank-major
 * device arrays, merged into one.  No communication in here; W > DEMF_RANKS_MAX returns DEMF_EUNSUPPORTED.
 * ------------------------------------------------------------------ */
#define DEMF_RANKS_MAX 64

/* W DetectionStores -> one, in rank order.  counts: HOST array of W ints, n_r = the scenes rank r appended
 * (0 <= n_r <= S, sum <= max_scenes).  Sources, DEVICE, the ranks' arrays stacked: src_scene_off (W, S+1),
 * src_state (W, 2), src_boxes (W, R, 7), src_scores (W, R), src_labels (W, R); S / R = the common per-rank scene /
 * row capacity.  Destination: the arrays of a store of max_scenes scenes and max_rows rows.
 *   rows_r = max(src_scene_off[r][n_r], 0)  - it keeps counting past R when rank r overflowed
 *   base_r = sum of rows_q over q < r (64-bit);  global scene g = sum of n_q over q < r, + i
 *   scene_off[g] = base_r + src_scene_off[r][i];  scene_off[sum n_r] = state[0] = sum rows_r
 *   state[1] = 1 if any src_state[r][1] != 0 or sum rows_r > max_rows (a row index reaches max_rows), else 0
 *   row j < min(rows_r, R) of rank r is copied bit for bit to row base_r + j when base_r + j < max_rows
 * (demf_detect_pack's rule: rows that do not fit are counted, not written).  Nothing else is written: neither
 * scene_off beyond sum n_r nor a row at or beyond sum rows_r.  One launch sized for R full rows per rank; the
 * row counts are read on the device, no host sync.  Vector stores only, one writer per word.                 */
DEMF_INTERNAL int demf_store_concat(int W, const int* counts, int S, int R, const int* src_scene_off,
                      const int* src_state, const float* src_boxes, const float* src_scores,
                      const int* src_labels, int max_scenes, int max_rows, float* boxes, float* scores,
                      int* labels, int* scene_off, int* state, demf_stream_t stream);

/* W step-meter rings (W, rows, 16) words in demf_step_meter's row layout -> out (rows, 16).  A row whose int64
 * stamp is the same on every rank: stamp kept; flags = OR over ranks; words 3-5 (lr_factor, grad_norm, clip) rank
 * 0's; each of the ten scalars (float)(sum over r of (double)x_r, ascending r, then / W) - non-finite values
 * propagate.  A row whose stamps differ is written as the row of an empty ring (stamp -1, other words 0).
 * W == 1 copies bit for bit.                                                                              */
DEMF_INTERNAL int demf_meter_merge(int W, int rows, const void* rings, void* out, demf_stream_t stream);

/* ------------------------------------------------------------------ *
 * Dense blocks of the DeMF fusion decoder layer (csrc/dense.hip)
 * Reference: demf/modeling/layers/transformer.py:55-80 -> mmcv DetrTransformerDecoderLayer
 * (nn.MultiheadAttention, MultiScaleDeformableAttention, FFN, 3 x LayerNorm; cfg
 * configs/demf/demf_votenet.py:71-91).  Upstream reaches cuBLAS / ATen for these; here they are
 * one strided GEMM with fused prologue / epilogue and a few row kernels.
 * ------------------------------------------------------------------ */

#define DEMF_GEMM_RELU 1      /* v = max(v, 0) after the bias                                  */
#define DEMF_GEMM_DROPOUT 2   /* v *= keep / (1 - drop_p), counter-based mask (rng, op_id)      */
#define DEMF_GEMM_GATE 4      /* v = gate[m,n] != 0 ? v * gate_scale : 0  (ReLU+dropout bwd)    */
#define DEMF_GEMM_ACCUM 8     /* C += v (split-K always accumulates, atomically, into zeroed C) */
#define DEMF_GEMM_ROWBIAS 16  /* bias term = bias[n] * rowscale[m]                              */
#define DEMF_GEMM_ACCUM2 32   /* C2 += v instead of C2 = v                                      */
#define DEMF_GEMM_FP32 64     /* keep this launch on the fp32 MFMA path in bf16 compute mode    */

/* C[m,n] (+)= epi( alpha * sum_k (A[m,k] + A2[m,k]) * (B[n,k] + B2[n,k]) + bias[n] ), all operands
 * fp32 and addressed by element strides: A[m,k] at A + m*sam + k*sak, B[n,k] at B + n*sbn + k*sbk,
 * C[m,n] at C + m*scm + n.  Batched over z = zo*zdiv + zi in [0,batch): operand offsets
 * zo*s?b + zi*s?b2.  A2 (same strides as A) is added for blocks whose first column < a2_cols,
 * B2 (same strides as B) for blocks whose first row < b2_rows.  splitk > 1 splits K over blocks.
 * C2 (same strides as C): optional second destination of the same values.
 * HOST struct; every pointer inside is a device pointer.                                      */
typedef struct demf_gemm_desc {
  int M, N, K, batch, zdiv, splitk;
  const float* A; long long sam, sak, sab, sab2;
  const float* A2; int a2_cols;
  const float* B; long long sbn, sbk, sbb, sbb2;
  const float* B2; int b2_rows;
  float* C; long long scm, scb, scb2;
  float* C2;
  const float* bias; long long sbias_b;          /* bias[n + z*sbias_b]                  */
  const float* rowscale; long long srs_m, srs_b; /* rowscale[m*srs_m + z*srs_b]          */
  float alpha;
  int flags;
  const float* gate; long long sgm, sgb;         /* gate[z*sgb + m*sgm + n]              */
  float gate_scale;
  float drop_p;
  const void* rng;                                /* 2 x uint64: seed, step counter       */
  int op_id;
  float* asum;   /* optional, accumulated: asum[z*M + m] += sum_k A[m,k] - the bias gradient when this
                  * launch is a weight gradient dW = dY^T.X (A = dY, reduction-strided, small-tile path) */
} demf_gemm_desc;

DEMF_INTERNAL int demf_gemm_f32(const demf_gemm_desc* desc, demf_stream_t stream);
/* n GEMMs in as few launches as possible: consecutive descriptors of the weight-gradient form (both
 * operands reduction-strided, few tiles) share ONE launch (their descriptors travel by value in the
 * kernel arguments); anything else runs as its own demf_gemm_f32.  The weight / bias gradients of the
 * linear layers of mmcv's DetrTransformerDecoderLayer (configs/demf/demf_votenet.py:71-91) depend on
 * nothing but saved tensors, so a decoder layer issues them as one group at the end of its backward. */
DEMF_INTERNAL int demf_gemm_group_f32(const demf_gemm_desc* descs, int n, demf_stream_t stream);

/* Compute dtype of the dense MFMA kernels (demf_mlp_gemm_*, demf_gemm_f32): 0 = fp32 MFMA (the
 * reference's precision, class_agnostic_vote_head.py:384 fp16_enabled=False), 1 = bf16 MFMA with
 * fp32 accumulation (BASELINE.json configs[3]): operands are rounded to bf16 on their way into LDS,
 * after the fp32 prologues; stored tensors, BN statistics, indices and losses stay fp32;
 * 2 = fp32 emulated on the bf16 MFMA in the demf_mlp_gemm_* kernels: each fp32 operand is split
 * exactly into three bf16 terms (3 x 8 significand bits) and the six products of weight >= 2^-16
 * are accumulated in fp32 (dropped terms <= 2^-23 relative); demf_gemm_f32 stays on the fp32 MFMA.
 * demf_set_compute_dtype sets the PROCESS DEFAULT; a caller that runs several models / threads in different
 * modes passes the mode with the call instead (demf_ctx below).  demf_get_compute_dtype: the mode a dense
 * call made by this thread right now would run in.                                                 */
DEMF_INTERNAL int demf_set_compute_dtype(int mode);
/* Mode 2 only: kernels that have the form take every fp32 operand as TWO fp16 terms (x = h + l, three products on
 * v_mfma_f32_32x32x16_f16; gradient operands scaled by a power of two per slab) instead of three bf16 terms (six
 * products): half the matrix work, ~2^-22 relative instead of 2^-24 - the size of fp32's own accumulation noise.
 * Process default: on (off with DEMF_F16_TERMS=0 in the environment).  csrc/common.h. */
DEMF_INTERNAL int demf_set_f16_terms(int on);
DEMF_INTERNAL int demf_get_compute_dtype(void);

/* The compute mode as a PARAMETER.  compute_mode: 0 / 1 / 2 as above, -1 = the process default; reserved
 * must be zero.  Two ways to hand it over:
 *   - demf_*_ctx(ctx, ...) variants of the generic dense entry points: the context applies to that call;
 *   - demf_ctx_push(ctx) ... demf_ctx_pop(): every dense call THIS THREAD makes in between (all demf_mlp_*,
 *     demf_gemm_*, demf_attn_core_*, demf_linear_* entry points) - a per-thread stack of depth 8, so two host
 *     threads in different modes never see each other's setting and nothing process-global is written. */
typedef struct demf_ctx {
  int compute_mode;
  int reserved[7];
} demf_ctx;
DEMF_INTERNAL int demf_ctx_push(const demf_ctx* ctx);
DEMF_INTERNAL int demf_ctx_pop(void);
DEMF_INTERNAL int demf_gemm_f32_ctx(const demf_ctx* ctx, const demf_gemm_desc* desc, demf_stream_t stream);
DEMF_INTERNAL int demf_gemm_group_f32_ctx(const demf_ctx* ctx, const demf_gemm_desc* descs, int n, demf_stream_t stream);
DEMF_INTERNAL int demf_mlp_gemm_fwd_ctx(const demf_ctx* ctx, int R, int K, int N, int ldx, const float* X,
                          const float* pro_scale_shift, const float* Wt, float* Y, double* stats,
                          demf_stream_t stream);

/* Self-attention core of the fusion decoder layer (nn.MultiheadAttention inside mmcv's
 * DetrTransformerDecoderLayer; demf/modeling/layers/transformer.py:55-80, configs/demf/demf_votenet.py:71-91):
 * out[b, q, h] = dropout(softmax(scale * q_h k_h^T)) v_h for the packed projections qkv (B*Q, 3*H*Dh) =
 * [q | k | v], one launch, the (B*H, Q, Q) score / probability tensors never stored.  stats (B*H*Q, 2) = row
 * maximum of the scaled scores and 1 / sum of exponentials, all the backward needs besides qkv, out and dout.
 * Dropout element ((b*H + h)*Q + q)*Q + k of stream (rng, op_id), as demf_softmax_dropout_fwd draws it.
 * prob / prob_dropped: optional (B*H, Q, Q) outputs for tests (both or neither).
 * Built for the reference's head shape Q = 256, Dh = 32: DEMF_EUNSUPPORTED otherwise (callers keep the
 * demf_gemm_f32 + demf_softmax_dropout_* form).  Compute mode 1 rounds the operands to bf16 where those
 * launches did; modes 0 / 2 are fp32 FMAs. */
DEMF_INTERNAL int demf_attn_core_fwd(int B, int H, int Q, int Dh, const float* qkv, float scale, float p, const void* rng,
                       int op_id, float* out, float* stats, float* prob, float* prob_dropped,
                       demf_stream_t stream);
/* dqkv (B*Q, 3*H*Dh) = gradients of [q | k | v] for dout (B*Q, H*Dh): probabilities are recomputed from
 * stats bit for bit, D = dout . out per query; per (scene, head) four query blocks produce dq and four key
 * blocks dk, dv - no atomics, every element written once. */
DEMF_INTERNAL int demf_attn_core_bwd(int B, int H, int Q, int Dh, const float* qkv, const float* out, const float* dout,
                       const float* stats, float scale, float p, const void* rng, int op_id, float* dqkv,
                       demf_stream_t stream);

/* s = identity + dropout(x) ; y = LayerNorm(s) over rows of C channels (C in 64..1024, power of two
 * multiples of 64).  s_out may alias x; stats (R,2) = mean, rstd.  nn.LayerNorm + the
 * `identity + dropout(out)` tails of mmcv MultiheadAttention / MultiScaleDeformableAttention / FFN.
 * s_out and stats may be NULL (forward-only callers). */
DEMF_INTERNAL int demf_add_dropout_ln_fwd(int R, int C, const float* x, const float* identity, const float* gamma,
                            const float* beta, float eps, float p, const void* rng, int op_id,
                            float* s_out, float* y, float* stats, demf_stream_t stream);
/* backward of the above for dy (+ dy2): ds_out (=/+= per ds_accum) the gradient of s (residual
 * path), dx_out = ds * keep/(1-p) the gradient of x, dgamma / dbeta ACCUMULATED (atomics).        */
DEMF_INTERNAL int demf_add_dropout_ln_bwd(int R, int C, const float* dy, const float* dy2, const float* s,
                            const float* stats, const float* gamma, float p, const void* rng, int op_id,
                            float* ds_out, int ds_accum, float* dx_out, float* dgamma, float* dbeta,
                            demf_stream_t stream);
/* prob = softmax(scores) over rows of S keys, out = dropout(prob): nn.MultiheadAttention's core. */
DEMF_INTERNAL int demf_softmax_dropout_fwd(int R, int S, const float* scores, float p, const void* rng, int op_id,
                             float* prob, float* out, demf_stream_t stream);
/* in place: dio (gradient of `out`) -> gradient of `scores`.                                     */
DEMF_INTERNAL int demf_softmax_dropout_bwd(int R, int S, const float* prob, float p, const void* rng, int op_id,
                             float* dio, demf_stream_t stream);
/* Sampling locations + attention weights of the fusion attention from the raw projection
 * raw (R, H*L*P*3) = [offsets (H,L,P,2) | logits (H,L*P)] and the query points pts (R,3):
 * DeMFVoteHead.get_reference_points (class_agnostic_vote_head.py:524-547; M (B,4,4) and
 * ab (B,4) = (au,bu,av,bv) composed on the host), x valid ratios (transformer.py:62-68),
 * + offsets / (W_l,H_l), softmax over L*P (mmcv MultiScaleDeformableAttention.forward).
 * -> loc (R,H,L,P,2), w (R,H,L,P), uvw (R,4) kept for the backward.  R = B*Q, L*P <= 16.       */
DEMF_INTERNAL int demf_msda_prep_fwd(int R, int Q, int H, int L, int P, const float* pts, const float* M,
                       const float* ab, const float* valid_ratios, const int64_t* shapes,
                       const float* raw, float* loc, float* w, float* uvw, demf_stream_t stream);
/* backward: (dloc + dloc2, dw + dw2) -> draw (R, H*L*P*3), dpts (R,3) or NULL.                   */
DEMF_INTERNAL int demf_msda_prep_bwd(int R, int Q, int H, int L, int P, const float* pts, const float* M,
                       const float* ab, const float* valid_ratios, const int64_t* shapes,
                       const float* w, const float* uvw, const float* dloc, const float* dloc2,
                       const float* dw, const float* dw2, float* draw, float* dpts,
                       demf_stream_t stream);
/* rng[1] += 1: one per training step (a captured graph then draws fresh masks at every replay). */
DEMF_INTERNAL int demf_rng_advance(void* rng, demf_stream_t stream);
/* rng[1] += 1 and snapshot[0..1] = (seed, new step): the forward of a node that carries dropout
 * (nn.Dropout inside mmcv's DetrTransformerDecoderLayer, configs/demf/demf_votenet.py:78,84,87) draws
 * its own step and saves the pair for its backward, as torch saves the mask.                         */
DEMF_INTERNAL int demf_rng_next(void* rng, void* snapshot, demf_stream_t stream);
/* out[i] = keep(i) / (1-p): the mask the fused kernels apply for (rng, op_id) - test hook.       */
DEMF_INTERNAL int demf_dropout_mask(long long n, float p, const void* rng, int op_id, float* out,
                      demf_stream_t stream);

/* n device-to-device copies (or zero fills where src == 0) in one launch.  `table` is a DEVICE
 * array of 3*n int64: n source addresses (0 = fill with zeros), n destination addresses, n lengths in
 * 4-byte words.  Replaces the per-tensor copy / memset launches of a training step: the refresh of
 * the step's static index buffers from the pipelined pre-pass, the zeroing of accumulated outputs. */
DEMF_INTERNAL int demf_multi_copy(int n, const void* table, int blocks_per_segment, demf_stream_t stream);
/* x[0..n) = 0 as a kernel launch (the step's zero arena: one fill per step).                         */
DEMF_INTERNAL int demf_zero_f32(long long n, float* x, demf_stream_t stream);

/* ------------------------------------------------------------------ *
 * Frozen image stream: convolutions on channels-last (NHWC) activations (csrc/conv.hip)
 * Replaces the library convolutions under mmdet ResNet-50 / ChannelMapper as the reference runs them in
 * DeMFVoteNet.extract_img_feat (/root/reference/demf/modeling/detectors/demfnet.py:124-132; configuration
 * /root/reference/configs/deformdetr/imvotenet_image.py:3-20).
 * ------------------------------------------------------------------ */

/* y (B,Ho,Wo,Cout) = [relu]( conv(x (B,H,W,Cin), w) + bias [+ resid (B,Ho,Wo,Cout)] ), implicit GEMM.
 * w_planes: (planes, Cout, KH*KW*Cin) bf16 - the (Cout,Cin,KH,KW) weight permuted to (Cout,KH,KW,Cin) (a frozen
 * BatchNorm folded in by the caller) and split into `planes` bf16 terms (1: bf16 arithmetic; 3: fp32-grade, see
 * demf_split_planes).  Cin % 32 == 0, Cout % 64 == 0.
 * ksplit > 1: the reduction is split over ksplit workgroup rows that ADD their partial tiles into y, which
 * must arrive zeroed (few output pixels x a long reduction: the neck's 3x3 level); bias, resid, relu unused. */
DEMF_INTERNAL int demf_conv_nhwc_f32(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                       const float* x, const void* w_planes, int planes, const float* bias,
                       const float* resid, int relu, int ksplit, float* y, demf_stream_t stream);
/* ResNet's 7x7 stride-2 pad-3 stem on an image stored (B,H,W,4) (zero fourth channel; demf_nchw3_to_nhwc4_f32).
 * w_planes: (planes, Cout, 7*32) with element [kh*32 + kw*4 + c] = w[cout][c][kh][kw] (zeros at kw == 7, c == 3). */
DEMF_INTERNAL int demf_conv_stem7_nhwc4_f32(int B, int H, int W, int Cout, const float* x4, const void* w_planes, int planes,
                              const float* bias, int relu, float* y, demf_stream_t stream);
/* 3x3 stride-2 pad-1 max-pool, (B,H,W,C) -> (B,(H+1)/2,(W+1)/2,C), C % 4 == 0. */
DEMF_INTERNAL int demf_maxpool3x3s2_nhwc_f32(int B, int H, int W, int C, const float* x, float* y, demf_stream_t stream);
/* (B,3,H,W) -> (B,H,W,4), fourth channel zero. */
DEMF_INTERNAL int demf_nchw3_to_nhwc4_f32(int B, int H, int W, const float* x, float* y, demf_stream_t stream);
/* GroupNorm(G groups) over (B,HW,C = 256) channels-last rows; image b's rows are written at y + b * y_batch_stride
 * (floats): the levels of the pyramid land directly in the encoder's (B,S,256) token buffer.  `sums`: 2*B*G doubles
 * of scratch.                                                                                       */
DEMF_INTERNAL int demf_groupnorm_nhwc_f32(int B, int HW, int C, int G, float eps, const float* x, const float* gamma,
                            const float* beta, double* sums, float* y, long long y_batch_stride,
                            demf_stream_t stream);

/* ------------------------------------------------------------------ *
 * Test side of the image branch's 2D detector (csrc/detr2d.hip): the Deformable-DETR decoder and head of
 * configs/deformdetr/imvotenet_image.py:21-80, which ImVoteNet_Deformdetr.extract_bboxes_2d
 * (demf/modeling/detectors/imvotenet_deform.py:188-248) runs as img_bbox_head.simple_test.
 * ------------------------------------------------------------------ */
#define DEMF_ATTN_EVAL_MAX_Q 512          /* K and V of one (scene, head) stay in LDS */
#define DEMF_DETR2D_MAX_CLASSES 32
#define DEMF_DETR2D_MAX_CANDIDATES 8192   /* Q * C scores of one image: 64-bit keys in 64 KB of LDS */
#define DEMF_DETR2D_MAX_K 1024

/* Inference self-attention for any query count: out[b, q, h] = softmax(scale * q_h k_h^T) v_h from the packed
 * projections qkv (B*Q, 3*H*Dh) = [q | k | v] -> out (B*Q, H*Dh).  No dropout, no statistics, the scores are never
 * stored.  nn.MultiheadAttention in eval mode inside mmcv's DetrTransformerDecoderLayer as the 2D detector's decoder
 * runs it over its 300 learned queries (configs/deformdetr/imvotenet_image.py:52-57; demf_attn_core_fwd is built
 * for the fusion layer's Q = 256).  Dh = 32 and 1 <= Q <= DEMF_ATTN_EVAL_MAX_Q: DEMF_EUNSUPPORTED otherwise.
 * Compute mode 1 rounds q, k, v and the probabilities to bf16 where they become operands; modes 0 / 2 are fp32 FMAs. */
DEMF_INTERNAL int demf_attn_fwd_eval(int B, int H, int Q, int Dh, const float* qkv, float scale, float* out,
                       demf_stream_t stream);
/* Tail of the last decoder layer's branches (mmdet DeformableDETRHead.forward, which
 * img_bbox_head.simple_test reaches at imvotenet_deform.py:210): logits (R,C) = hs (R,K) . w_cls (C,K)^T + b_cls and
 * boxes (R,4) = sigmoid(hidden (R,K) . w_reg (4,K)^T + b_reg [+ inverse_sigmoid(reference) on columns 0, 1]) -
 * normalised (cx, cy, w, h); hidden = the box branch after its two Linear + ReLU layers; row r reads
 * reference[r % ref_rows] (ref_rows, 2); inverse_sigmoid with mmdet's eps = 1e-5.  fp32 FMAs in every compute mode.
 * C <= DEMF_DETR2D_MAX_CLASSES, K % 4 == 0, K <= 1024. */
DEMF_INTERNAL int demf_detr2d_head(int R, int C, int K, const float* hs, const float* hidden, const float* w_cls,
                     const float* b_cls, const float* w_reg, const float* b_reg, const float* reference,
                     int ref_rows, float* logits, float* boxes, demf_stream_t stream);
/* mmdet DeformableDETRHead._get_bboxes_single for a whole batch + the score filter of extract_bboxes_2d
 * (imvotenet_deform.py:181-186,210-230), one launch, nothing read back: per image the k best of the Q*C candidates
 * in the order (logit descending, flat index q*C + c ascending) - one of the orders torch.topk over the sigmoid
 * scores may return -, label = index % C, query = index / C, boxes (B*Q,4) cxcywh -> xyxy, x * img w, y * img h,
 * clamped to the image, divided by the four scale factors when rescale != 0; meta (B,6) = [img h, img w,
 * scale_factor x4].  rows (B,k,6) = [x1, y1, x2, y2, score, class] for the places with sigmoid(logit) > thr (a prefix
 * of the order; thr < 0: all min(k, Q*C) places), zeros behind them; counts (B) = their number.  NaN logits order
 * after every number and set bit 0 of *flag.  Q*C <= DEMF_DETR2D_MAX_CANDIDATES, k <= DEMF_DETR2D_MAX_K:
 * DEMF_EUNSUPPORTED otherwise. */
DEMF_INTERNAL int demf_detr2d_select(int B, int Q, int C, int k, const float* logits, const float* boxes,
                       const float* meta, int rescale, float thr, float* rows, int* counts, int* flag,
                       demf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DEMF_HIP_H_ */
