// The rest of DeMFVoteHead.get_bboxes (class_agnostic_vote_head.py:714-754) around the two kernels of
// postprocess.hip: the decode + score of every ensemble layer in one launch, and the selection of the NMS
// survivors into a device-resident detection store in the row order of mmdet3d's multiclass_nms_single.
// Arithmetic mirrors the torch expressions term by term (build: -ffp-contract=off).
#include <hip/hip_runtime.h>

#include "common.h"

namespace demf {

struct DetectLayers {
  demf_detect_layer l[DEMF_DETECT_MAX_LAYERS];
};

__device__ __forceinline__ const float* row_of(const float* p, int sb, int sk, int b, int k) {
  return p + (size_t)b * sb + (size_t)k * sk;
}

// Scores of one candidate: obj = softmax(obj_scores)[1]; sem = softmax(sem_scores); cls = argmax(sem) (first maximum).
__device__ __forceinline__ void score_one(const float* ob, const float* sm, size_t g, int C, float* __restrict__ obj,
                                          float* __restrict__ sem, long long* __restrict__ cls) {
  // F.softmax: exp(x - max) / sum
  {
    const float mx = fmaxf(ob[0], ob[1]);
    const float e0 = expf(ob[0] - mx), e1 = expf(ob[1] - mx);
    obj[g] = e1 / (e0 + e1);
  }
  float mx = sm[0];
  for (int j = 1; j < C; ++j) mx = fmaxf(mx, sm[j]);
  float sum = 0.f;
  for (int j = 0; j < C; ++j) sum += expf(sm[j] - mx);
  float* so = sem + g * C;
  int best = 0;
  float bp = -1.f;
  for (int j = 0; j < C; ++j) {
    const float p = expf(sm[j] - mx) / sum;
    so[j] = p;
    if (p > bp) { bp = p; best = j; }
  }
  cls[g] = best;
}

// yaw = class2angle(argmax dir_class, res_scale * dir_res[argmax]) % 2pi, in torch's fp32 steps
__device__ __forceinline__ float yaw_of(const float* dc, const float* dr, float res_scale, int nb) {
  int best = 0;
  float bv = dc[0];
  for (int j = 1; j < nb; ++j) {
    const float v = dc[j];
    if (v > bv) { bv = v; best = j; }
  }
  const float res = dr[best] * res_scale;
  const float two_pi = (float)(2.0 * 3.14159265358979323846);
  const float per = (float)(2.0 * 3.14159265358979323846 / (double)nb);
  float angle = (float)best * per + res;                                   // class2angle
  if (angle > (float)3.14159265358979323846) angle = angle - two_pi;       // limit_period
  float m = fmodf(angle, two_pi);                                          // torch.remainder(angle, 2pi)
  if (m != 0.f && m < 0.f) m += two_pi;
  return m;
}

// One candidate: box7 = coder.decode(): (centre, size, yaw) with yaw = class2angle(argmax dir_class,
// dir_res[argmax]) % 2pi; obj = softmax(obj_scores)[1]; sem = softmax(sem_scores); cls = argmax(sem) (first maximum).
__device__ __forceinline__ void decode_one(const demf_detect_layer& y, int b, int k, size_t g, int C, int nb,
                                           int with_rot, float* __restrict__ box7, float* __restrict__ cosy,
                                           float* __restrict__ siny, float* __restrict__ obj,
                                           float* __restrict__ sem, long long* __restrict__ cls) {
  float* o = box7 + g * 7;
  const float* c = row_of(y.center, y.center_sb, y.center_sk, b, k);
  if (y.center_base) {                                     // coder.py:214  center = base_xyz + reg[..., 0:3]
    const float* base = row_of(y.center_base, y.base_sb, y.base_sk, b, k);
    for (int a = 0; a < 3; ++a) o[a] = base[a] + c[a];
  } else {
    for (int a = 0; a < 3; ++a) o[a] = c[a];
  }
  const float* sz = row_of(y.size, y.size_sb, y.size_sk, b, k);
  for (int a = 0; a < 3; ++a) o[3 + a] = sz[a];
  float yaw = 0.f;
  if (with_rot) {
    // coder.py:233  dir_res = dir_res_norm * (pi / nb)  (res_scale = 1 when dir_res itself is given)
    yaw = yaw_of(row_of(y.dir_class, y.dir_class_sb, y.dir_class_sk, b, k),
                 row_of(y.dir_res, y.dir_res_sb, y.dir_res_sk, b, k), y.res_scale, nb);
  }
  o[6] = yaw;
  cosy[g] = cosf(yaw);
  siny[g] = sinf(yaw);
  score_one(row_of(y.obj, y.obj_sb, y.obj_sk, b, k), row_of(y.sem, y.sem_sb, y.sem_sk, b, k), g, C, obj, sem, cls);
}

// One lane per candidate (scene b, proposal kk of the concatenated K = sum K_l).  The layer loop index is uniform, so
// the descriptors are read from the kernel arguments as scalars; each lane takes the one layer its kk falls into.
__global__ __launch_bounds__(256) void detect_decode_k(int B, int K, int L, int C, int nb, int with_rot,
                                                       DetectLayers layers, float* __restrict__ box7,
                                                       float* __restrict__ cosy, float* __restrict__ siny,
                                                       float* __restrict__ obj, float* __restrict__ sem,
                                                       long long* __restrict__ cls) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= B * K) return;
  const int b = g / K, kk = g - b * K;
  int lo = 0;
#pragma unroll
  for (int i = 0; i < DEMF_DETECT_MAX_LAYERS; ++i) {
    if (i < L) {
      const int Kl = layers.l[i].K;
      if (kk >= lo && kk < lo + Kl)
        decode_one(layers.l[i], b, kk - lo, (size_t)g, C, nb, with_rot, box7, cosy, siny, obj, sem, cls);
      lo += Kl;
    }
  }
}

// The distance form (CAVoteHead: ClassAgnosticBBoxCoder.decode, class_agnostic_bbox_coder.py:42-86): one lane per
// proposal, straight from the raw conv rows.  d = exp(reg[0:6]) (split_pred, :100); size = clamp(d[0:3] + d[3:6],
// min=0.1) (:67-68); canonical = (d[3:6] - d[0:3]) / 2 (:71-72) rotated by yaw about z as mmdet3d's
// rotation_3d_in_axis does (x c + y s, -x s + y c, z); centre = ref - that (:83).
__global__ __launch_bounds__(256) void ca_detect_decode_k(int B, int K, int C, int nb, int with_rot,
                                                          const float* __restrict__ reg, int reg_sb, int reg_sk,
                                                          const float* __restrict__ cls_rows, int cls_sb, int cls_sk,
                                                          const float* __restrict__ ref, int ref_sb, int ref_sk,
                                                          float* __restrict__ box7, float* __restrict__ cosy,
                                                          float* __restrict__ siny, float* __restrict__ obj,
                                                          float* __restrict__ sem, long long* __restrict__ cls) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= B * K) return;
  const int b = g / K, k = g - b * K;
  const float* pr = row_of(reg, reg_sb, reg_sk, b, k);
  const float* pc = row_of(cls_rows, cls_sb, cls_sk, b, k);
  const float* rp = row_of(ref, ref_sb, ref_sk, b, k);
  float d[6];
#pragma unroll
  for (int a = 0; a < 6; ++a) d[a] = expf(pr[a]);
  const float yaw = with_rot ? yaw_of(pr + 6, pr + 6 + nb, (float)(3.14159265358979323846 / (double)nb), nb) : 0.f;
  const float c = cosf(yaw), s = sinf(yaw);
  const float x = (d[3] - d[0]) / 2.f, y = (d[4] - d[1]) / 2.f, z = (d[5] - d[2]) / 2.f;
  float* o = box7 + (size_t)g * 7;
  o[0] = rp[0] - (x * c + y * s);
  o[1] = rp[1] - ((-x) * s + y * c);
  o[2] = rp[2] - z;
#pragma unroll
  for (int a = 0; a < 3; ++a) o[3 + a] = fmaxf(d[a] + d[3 + a], 0.1f);
  o[6] = yaw;
  cosy[g] = c;
  siny[g] = s;
  score_one(pc, pc + 2, (size_t)g, C, obj, sem, cls);
}

// Block-wide sum of one int per thread (1024 threads = 16 waves); every thread receives the total.
__device__ __forceinline__ int block_sum_1024(int v, int* s_part) {
  for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
  __syncthreads();                                          // s_part may still be read from the previous use
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
  for (int w = 0; w < 16; ++w) t += s_part[w];
  return t;
}

// One workgroup per scene, one lane per candidate (K <= 1024).  Survivors = keep & (obj > score_thr); scene b's
// rows start at scene_off[first_scene] (the store's row cursor: written by the previous append, only read here) plus
// the rows of the batch's earlier scenes, which every workgroup counts itself - no cross-workgroup ordering.
// per_class: rows are class-major, proposal index ascending inside a class, score = obj * sem[c], label = c;
// otherwise one row per survivor with its arg-max class.  Rows at or beyond max_rows are not written.
__global__ __launch_bounds__(1024) void detect_pack_k(int B, int K, int C, int per_class, float score_thr,
                                                      const unsigned char* __restrict__ keep,
                                                      const float* __restrict__ obj,
                                                      const float* __restrict__ sem,
                                                      const long long* __restrict__ cls,
                                                      const float* __restrict__ bottom, int first_scene,
                                                      int max_rows, float* __restrict__ boxes,
                                                      float* __restrict__ scores, int* __restrict__ labels,
                                                      int* __restrict__ scene_off, int* __restrict__ state) {
  __shared__ int s_part[16];
  const int b = blockIdx.x, t = threadIdx.x;
  const int per = per_class ? C : 1;
  int earlier = 0;
  if (t < K)
    for (int e = 0; e < b; ++e) {
      const size_t i = (size_t)e * K + t;
      earlier += (keep[i] != 0 && obj[i] > score_thr) ? 1 : 0;
    }
  earlier = block_sum_1024(earlier, s_part);
  const size_t me = (size_t)b * K + t;
  const bool sel = t < K && keep[me] != 0 && obj[me] > score_thr;
  const unsigned long long ballot = __ballot(sel);
  const int lane = t & 63, wave = t >> 6;
  const int in_wave = __popcll(ballot & ((1ull << lane) - 1ull));
  __syncthreads();
  if (lane == 0) s_part[wave] = __popcll(ballot);
  __syncthreads();
  int before = 0, n = 0;
  for (int w = 0; w < 16; ++w) {
    const int c = s_part[w];
    before += w < wave ? c : 0;
    n += c;
  }
  const long long start = (long long)scene_off[first_scene] + (long long)earlier * per;
  const long long end = start + (long long)n * per;
  if (t == 0) {
    scene_off[first_scene + b + 1] = (int)end;
    if (end > max_rows) state[1] = 1;
    if (b == B - 1) state[0] = (int)end;                    // rows needed so far, whether they fitted or not
  }
  if (!sel) return;
  const int rank = before + in_wave;
  const float* bx = bottom + me * 7;
  const float o = obj[me];
  for (int c = 0; c < per; ++c) {
    const long long row = start + (long long)c * n + rank;
    if (row >= max_rows) continue;
    float* ob = boxes + (size_t)row * 7;
    for (int a = 0; a < 7; ++a) ob[a] = bx[a];
    scores[row] = per_class ? o * sem[me * C + c] : o;
    labels[row] = per_class ? c : (int)cls[me];
  }
}

}  // namespace demf

using namespace demf;

extern "C" int demf_detect_decode(int B, int K, int L, int C, int num_dir_bins, int with_rot,
                                  const demf_detect_layer* layers, float* box7, float* cos_yaw,
                                  float* sin_yaw, float* obj, float* sem, int64_t* classes,
                                  demf_stream_t stream) {
  DEMF_REQUIRE(B >= 0 && K >= 0 && L >= 1 && L <= DEMF_DETECT_MAX_LAYERS && C >= 1 && num_dir_bins >= 1,
               "detect_decode: bad sizes");
  DEMF_REQUIRE(layers, "detect_decode: null pointer");
  long long sum = 0;
  DetectLayers arg;
  for (int i = 0; i < L; ++i) {
    DEMF_REQUIRE(layers[i].K >= 0, "detect_decode: bad sizes");
    sum += layers[i].K;
    arg.l[i] = layers[i];
  }
  DEMF_REQUIRE(sum == K, "detect_decode: bad sizes (the layers hold %lld proposals, K=%d)", sum, K);
  if (K > 1024) {
    set_error("detect_decode: K=%d boxes per scene exceeds 1024", K);
    return DEMF_EUNSUPPORTED;
  }
  if (B * K == 0) return DEMF_OK;
  for (int i = 0; i < L; ++i) {
    if (layers[i].K == 0) continue;
    DEMF_REQUIRE(layers[i].center && layers[i].size && layers[i].obj && layers[i].sem &&
                     (!with_rot || (layers[i].dir_class && layers[i].dir_res)),
                 "detect_decode: null pointer");
  }
  DEMF_REQUIRE(box7 && cos_yaw && sin_yaw && obj && sem && classes, "detect_decode: null pointer");
  hipLaunchKernelGGL(detect_decode_k, dim3(cdiv(B * K, 256)), dim3(256), 0, (hipStream_t)stream, B, K, L, C,
                     num_dir_bins, with_rot, arg, box7, cos_yaw, sin_yaw, obj, sem, (long long*)classes);
  return check_launch("detect_decode");
}

extern "C" int demf_ca_detect_decode(int B, int K, int C, int num_dir_bins, int with_rot, const float* reg,
                                     int reg_sb, int reg_sk, const float* cls, int cls_sb, int cls_sk,
                                     const float* ref, int ref_sb, int ref_sk, float* box7, float* cos_yaw,
                                     float* sin_yaw, float* obj, float* sem, int64_t* classes,
                                     demf_stream_t stream) {
  DEMF_REQUIRE(B >= 0 && K >= 0 && C >= 1 && num_dir_bins >= 1, "ca_detect_decode: bad sizes");
  if (K > 1024) {
    set_error("ca_detect_decode: K=%d boxes per scene exceeds 1024", K);
    return DEMF_EUNSUPPORTED;
  }
  if (B * K == 0) return DEMF_OK;
  DEMF_REQUIRE(reg_sk >= 6 + 2 * num_dir_bins && cls_sk >= 2 + C && ref_sk >= 3 && reg_sb >= 0 && cls_sb >= 0 &&
                   ref_sb >= 0, "ca_detect_decode: bad strides");
  DEMF_REQUIRE(reg && cls && ref && box7 && cos_yaw && sin_yaw && obj && sem && classes,
               "ca_detect_decode: null pointer");
  hipLaunchKernelGGL(ca_detect_decode_k, dim3(cdiv(B * K, 256)), dim3(256), 0, (hipStream_t)stream, B, K, C,
                     num_dir_bins, with_rot, reg, reg_sb, reg_sk, cls, cls_sb, cls_sk, ref, ref_sb, ref_sk, box7,
                     cos_yaw, sin_yaw, obj, sem, (long long*)classes);
  return check_launch("ca_detect_decode");
}

extern "C" int demf_detect_pack(int B, int K, int C, int per_class, float score_thr,
                                const unsigned char* keep, const float* obj, const float* sem,
                                const int64_t* classes, const float* boxes_bottom, int first_scene,
                                int max_scenes, int max_rows, float* boxes, float* scores, int* labels,
                                int* scene_off, int* state, demf_stream_t stream) {
  DEMF_REQUIRE(B >= 0 && K >= 0 && C >= 1 && first_scene >= 0 && max_rows >= 0 &&
                   (long long)first_scene + B <= max_scenes,
               "detect_pack: bad sizes");
  if (K > 1024) {
    set_error("detect_pack: K=%d boxes per scene exceeds 1024", K);
    return DEMF_EUNSUPPORTED;
  }
  if (B == 0) return DEMF_OK;
  DEMF_REQUIRE(scene_off && state && (max_rows == 0 || (boxes && scores && labels)) &&
                   (K == 0 || (keep && obj && sem && classes && boxes_bottom)),
               "detect_pack: null pointer");
  hipLaunchKernelGGL(detect_pack_k, dim3(B), dim3(1024), 0, (hipStream_t)stream, B, K, C, per_class, score_thr,
                     keep, obj, sem, (const long long*)classes, boxes_bottom, first_scene, max_rows, boxes,
                     scores, labels, scene_off, state);
  return check_launch("detect_pack");
}
