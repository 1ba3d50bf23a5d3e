// Test-time augmentation: the merge of a scene's views.  The reference's forward_test hands num_augs > 1 to
// self.aug_test (demf/modeling/detectors/demfnet.py:236-238), which mmdet3d 0.18.1 builds from
// merge_aug_bboxes_3d (bbox3d_mapping_back per view, concatenate, per-class iou3d.nms_gpu / nms_normal_gpu, score-
// ordered cut) [dep-recall].  Here: a segmented greedy NMS on the exact rotated footprints (bev_clip.h) and the
// three-launch merge of a batch of view-major DetectionStore scenes into a destination store, without a host sync.
// All arithmetic is fp32 (build: -ffp-contract=off).  Deviations from upstream: DESIGN.md 3.16.
#include <hip/hip_runtime.h>

#include "bev_clip.h"
#include "common.h"

namespace demf {

namespace {

constexpr int kNmsMax = DEMF_NMS_MAX_SEGMENT;           // boxes of one NMS segment (one lane each)
constexpr int kMergeMaxCand = DEMF_TTA_MAX_CANDIDATES;  // candidates of one merged scene (V * K * C): 128 KB of sort LDS
constexpr int kGatherThreads = 256;
constexpr int kFinishThreads = 1024;

enum { kModeBev = 0, kModeAligned = 1, kMode3d = 2 };

// IoU of the current box a (with its half-diagonal ra) and the lane's box b under `mode`.  Rotated modes: centres
// further apart than the two half-diagonals cannot overlap (tests/eval_reference.py:bev_overlap makes the same
// test) - mostly true in a scene, and it spares the divergent clip; a footprint of zero area overlaps nothing.
__device__ __forceinline__ float pair_iou(int mode, const float* a, float ra, const float* b, float rb) {
  const float area_a = a[3] * a[4], area_b = b[3] * b[4];
  if (mode == kModeAligned) {                      // nms_normal_gpu: centre +- (dx, dy) / 2, yaw ignored
    const float l = fmaxf(0.f, fminf(a[0] + a[3] * 0.5f, b[0] + b[3] * 0.5f) - fmaxf(a[0] - a[3] * 0.5f, b[0] - b[3] * 0.5f));
    const float w = fmaxf(0.f, fminf(a[1] + a[4] * 0.5f, b[1] + b[4] * 0.5f) - fmaxf(a[1] - a[4] * 0.5f, b[1] - b[4] * 0.5f));
    const float ov = l * w;
    return ov / fmaxf(area_a + area_b - ov, 1e-8f);
  }
  const float tx = b[0] - a[0], ty = b[1] - a[1], rr = ra + rb;
  float ov = 0.f;
  if (area_a != 0.f && area_b != 0.f && !(tx * tx + ty * ty > rr * rr)) ov = bev_overlap(a, b);
  if (mode == kModeBev) return ov / fmaxf(area_a + area_b - ov, 1e-8f);
  // rotated 3-D IoU: box3d_iou's formula around the guarded footprint overlap
  const float h = fmaxf(fminf(a[2] + a[5], b[2] + b[5]) - fmaxf(a[2], b[2]), 0.f);
  const float inter = ov * h;
  return inter / fmaxf(area_a * a[5] + area_b * b[5] - inter, 1e-8f);
}

// Segmented greedy NMS, one workgroup per segment s = rows seg_start[s] .. + seg_count[s] of boxes / scores, one lane
// per box (blockDim.x = a power of two >= n_max).  The shape of aligned_nms_k (postprocess.hip): an LDS bitonic sort
// of (score, index) - score descending, ties: the lower index first -, then rounds over the boxes that are still
// alive: the current box is broadcast through LDS, every alive lane computes its IoU with it and falls when
// !(iou <= thr), so NaN suppresses.  A dead box costs no barrier: nothing is written between the end of a round
// and the next alive box, so s_alive[i] is read uniformly.  Candidates: valid != 0 (when given) and a score that
// is neither NaN nor -inf.  A segment that does not fit (count > n_max, or rows outside [0, R)) sets *overflow and
// keeps nothing: none of its keep bytes is written.
__global__ __launch_bounds__(kNmsMax) void nms_bev_k(int R, int n_max, float thr, int mode,
                                                     const float* __restrict__ boxes,
                                                     const float* __restrict__ scores,
                                                     const int* __restrict__ seg_start,
                                                     const int* __restrict__ seg_count,
                                                     const unsigned char* __restrict__ valid,
                                                     unsigned char* __restrict__ keep, int* __restrict__ overflow) {
  __shared__ float s_key[kNmsMax];
  __shared__ int s_ord[kNmsMax];
  __shared__ unsigned char s_alive[kNmsMax];
  __shared__ float s_cur[8];
  const int s = blockIdx.x, t = threadIdx.x, P = blockDim.x;
  const int start = seg_start[s], n = seg_count[s];
  if (n < 0 || n > n_max || n > P || start < 0 || (long long)start + n > (long long)R) {     // uniform
    if (t == 0) *overflow = 1;
    return;
  }
  if (n == 0) return;
  const size_t me = (size_t)start + t;
  float b[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float sc = -__builtin_inff();
  bool mine = false;
  if (t < n) {
#pragma unroll
    for (int k = 0; k < 7; ++k) b[k] = boxes[me * 7 + k];
    sc = scores[me];
    mine = (valid == nullptr || valid[me] != 0) && sc == sc && sc != -__builtin_inff();
    keep[me] = 0;
  }
  s_key[t] = mine ? sc : -__builtin_inff();
  s_ord[t] = t;
  s_alive[t] = mine ? 1 : 0;
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      const int p = t ^ stride;
      if (p > t) {
        const bool desc = (t & size) == 0;
        const float a = s_key[t], c = s_key[p];
        const int ia = s_ord[t], ic = s_ord[p];
        const bool a_first = a > c || (a == c && ia < ic);      // a should come before c
        if (desc ? !a_first : a_first) {
          s_key[t] = c; s_key[p] = a;
          s_ord[t] = ic; s_ord[p] = ia;
        }
      }
      __syncthreads();
    }
  const float rb = 0.5f * sqrtf(b[3] * b[3] + b[4] * b[4]);
  bool undecided = mine;                                  // this lane's box is neither kept nor removed yet
  for (int r = 0; r < n; ++r) {
    if (s_key[r] == -__builtin_inff()) break;             // only non-candidates remain (uniform)
    const int i = s_ord[r];
    if (!s_alive[i]) continue;                            // uniform: no write since the last barrier
    if (t == i) {                                         // (s_alive[i] stays 1: a rank is visited once, and a
      keep[me] = 1;                                       //  write here would race with the uniform read above)
      undecided = false;
#pragma unroll
      for (int k = 0; k < 7; ++k) s_cur[k] = b[k];
      s_cur[7] = rb;
    }
    __syncthreads();
    if (undecided) {
      float a[7];
#pragma unroll
      for (int k = 0; k < 7; ++k) a[k] = s_cur[k];
      const float iou = pair_iou(mode, a, s_cur[7], b, rb);
      if (!(iou <= thr)) {                                // upstream keeps `iou <= thresh`
        s_alive[t] = 0;
        undecided = false;
      }
    }
    __syncthreads();
  }
}

// Merge, launch (a).  One workgroup per (class c, batch scene b): the rows with label c of the V view scenes
// first_view + v * B + b, in (view, row) order, go to the workspace segment (b * C + c) * VK .. with VK = V * K,
// mapped back through the inverse of the view's parameter row [flip, cos, sin, scale, tx, ty, tz, -] - the exact
// inverse of pipeline.apply_aug_params on a box: c -= t; [:6] /= s; the centre turned by -angle and yaw += angle;
// then the flip (x -> -x, yaw -> pi - yaw).  The rows of a class are found from the labels, whatever their order.
// seg_count may exceed VK (a view scene that holds more than K rows of a class): the NMS launch then reports the
// segment as overflowing.  Rows of the view store at or beyond its max_rows were never written and are not read.
__global__ __launch_bounds__(kGatherThreads) void tta_gather_k(int B, int V, int C, int VK,
                                                               const float* __restrict__ vboxes,
                                                               const float* __restrict__ vscores,
                                                               const int* __restrict__ vlabels,
                                                               const int* __restrict__ vscene_off, int first_view,
                                                               int v_max_rows, const float* __restrict__ params,
                                                               float* __restrict__ ws_boxes,
                                                               float* __restrict__ ws_scores,
                                                               int* __restrict__ seg_start,
                                                               int* __restrict__ seg_count,
                                                               int* __restrict__ ws_flag) {
  __shared__ int s_part[kGatherThreads / 64];
  const int c = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const int seg = b * C + c;
  const size_t base = (size_t)seg * VK;
  if (seg == 0 && t == 0) *ws_flag = 0;                   // the NMS launch behind this one may set it
  const int lane = t & 63, wave = t >> 6;
  int at = 0;
  for (int v = 0; v < V; ++v) {
    const int sv = first_view + v * B + b;
    int lo = vscene_off[sv], hi = vscene_off[sv + 1];
    lo = max(lo, 0);
    hi = min(hi, v_max_rows);
    const float* p = params + (size_t)(v * B + b) * 8;
    const float flip = p[0], cs = p[1], sn = p[2], sc = p[3], tx = p[4], ty = p[5], tz = p[6];
    const float angle = atan2f(sn, cs);
    for (int r0 = lo; r0 < hi; r0 += kGatherThreads) {
      const int row = r0 + t;
      const bool sel = row < hi && vlabels[row] == c;
      const unsigned long long ballot = __ballot(sel);
      const int in_wave = __popcll(ballot & ((1ull << lane) - 1ull));
      __syncthreads();                                    // s_part may still be read from the previous chunk
      if (lane == 0) s_part[wave] = __popcll(ballot);
      __syncthreads();
      int before = 0, total = 0;
      for (int w = 0; w < kGatherThreads / 64; ++w) {
        const int k = s_part[w];
        before += w < wave ? k : 0;
        total += k;
      }
      const int pos = at + before + in_wave;
      at += total;
      if (sel && pos < VK) {
        const float* in = vboxes + (size_t)row * 7;
        const float x = (in[0] - tx) / sc, y = (in[1] - ty) / sc, z = (in[2] - tz) / sc;
        float ox = x * cs + y * sn;
        const float oy = (-x) * sn + y * cs;
        float yaw = in[6] + angle;
        if (flip != 0.f) {
          ox = -ox;
          yaw = -yaw + 3.14159265358979323846f;
        }
        float* o = ws_boxes + (base + pos) * 7;
        o[0] = ox; o[1] = oy; o[2] = z;
        o[3] = in[3] / sc; o[4] = in[4] / sc; o[5] = in[5] / sc;
        o[6] = yaw;
        ws_scores[base + pos] = vscores[row];
      }
    }
  }
  if (t == 0) {
    seg_start[seg] = (int)base;
    seg_count[seg] = at;
  }
}

// Kept rows of a scene's C segments: candidate e of the scene is workspace row scene * C * VK + e, class e / VK.
__device__ __forceinline__ bool merge_kept(const unsigned char* keep, const int* seg_count, int scene, int C,
                                           int VK, int e) {
  const int cnt = seg_count[scene * C + e / VK];
  return cnt <= VK && e % VK < cnt && keep[(size_t)scene * C * VK + e] != 0;
}

// Merge, launch (c).  One workgroup per batch scene: the kept rows of its C segments are ordered by (score
// descending, class ascending, view ascending, row ascending) - the last three are the workspace index, so an LDS
// bitonic sort of (score, index) over the next power of two of the kept count gives a total order -, cut at max_num
// and appended to the destination store with detect_pack_k's protocol: the cursor is read at scene_off[first_scene],
// every workgroup counts the rows of the batch's earlier scenes itself, scene_off[first_scene + b + 1] = end,
// state[1] = 1 when rows do not fit (or a segment overflowed, or the view store had), rows at or beyond max_rows
// are not written.  Dynamic LDS: cap floats + cap ints, cap = the next power of two of C * VK.
__global__ __launch_bounds__(kFinishThreads) void tta_finish_k(int B, int C, int VK, int cap, int max_num,
                                                               const float* __restrict__ ws_boxes,
                                                               const float* __restrict__ ws_scores,
                                                               const int* __restrict__ seg_count,
                                                               const unsigned char* __restrict__ keep,
                                                               const int* __restrict__ ws_flag,
                                                               const int* __restrict__ vstate, int first_scene,
                                                               int max_rows, float* __restrict__ boxes,
                                                               float* __restrict__ scores, int* __restrict__ labels,
                                                               int* __restrict__ scene_off, int* __restrict__ state) {
  extern __shared__ unsigned char s_dyn[];
  float* s_key = reinterpret_cast<float*>(s_dyn);
  int* s_idx = reinterpret_cast<int*>(s_dyn) + cap;
  __shared__ int s_part[kFinishThreads / 64];
  __shared__ int s_n;
  const int b = blockIdx.x, t = threadIdx.x;
  const int cand = C * VK;
  // rows of the batch's earlier scenes
  long long earlier = 0;
  for (int e = 0; e < b; ++e) {
    int local = 0;
    for (int i = t; i < cand; i += kFinishThreads) local += merge_kept(keep, seg_count, e, C, VK, i) ? 1 : 0;
    for (int d = 32; d; d >>= 1) local += __shfl_xor(local, d);
    __syncthreads();
    if ((t & 63) == 0) s_part[t >> 6] = local;
    __syncthreads();
    int total = 0;
    for (int w = 0; w < kFinishThreads / 64; ++w) total += s_part[w];
    earlier += min(total, max_num);
  }
  if (t == 0) s_n = 0;
  __syncthreads();
  // this scene's kept rows, in any order: the sort's key is a total order
  for (int i = t; i < cand; i += kFinishThreads)
    if (merge_kept(keep, seg_count, b, C, VK, i)) {
      const int slot = atomicAdd(&s_n, 1);
      s_key[slot] = ws_scores[(size_t)b * cand + i];
      s_idx[slot] = i;
    }
  __syncthreads();
  const int n = s_n;
  int P = 1;
  while (P < n) P <<= 1;
  for (int i = n + t; i < P; i += kFinishThreads) {
    s_key[i] = -__builtin_inff();
    s_idx[i] = 0x7fffffff;
  }
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int q = t; q < P; q += kFinishThreads) {
        const int p = q ^ stride;
        if (p > q) {
          const bool desc = (q & size) == 0;
          const float a = s_key[q], c = s_key[p];
          const int ia = s_idx[q], ic = s_idx[p];
          const bool a_first = a > c || (a == c && ia < ic);
          if (desc ? !a_first : a_first) {
            s_key[q] = c; s_key[p] = a;
            s_idx[q] = ic; s_idx[p] = ia;
          }
        }
      }
      __syncthreads();
    }
  const int n_out = min(n, max_num);
  const long long start = (long long)scene_off[first_scene] + earlier;
  const long long end = start + n_out;
  if (t == 0) {
    scene_off[first_scene + b + 1] = (int)end;
    if (end > max_rows || *ws_flag != 0 || (vstate != nullptr && vstate[1] != 0)) state[1] = 1;
    if (b == B - 1) state[0] = (int)end;                    // rows needed so far, whether they fitted or not
  }
  for (int r = t; r < n_out; r += kFinishThreads) {
    const long long row = start + r;
    if (row >= max_rows) continue;
    const int i = s_idx[r];
    const float* in = ws_boxes + ((size_t)b * cand + i) * 7;
    float* o = boxes + (size_t)row * 7;
    for (int a = 0; a < 7; ++a) o[a] = in[a];
    scores[row] = s_key[r];
    labels[row] = i / VK;
  }
}

int pow2_threads(int n) {
  int p = 64;
  while (p < n) p <<= 1;
  return p;
}

unsigned long long g_finish_lds_done = 0;

}  // namespace

}  // namespace demf

using namespace demf;

extern "C" int demf_nms_bev(int R, int S, int n_max, float thr, int mode, const float* boxes, const float* scores,
                            const int* seg_start, const int* seg_count, const unsigned char* valid,
                            unsigned char* keep, int* overflow, demf_stream_t stream) {
  DEMF_REQUIRE(R >= 0 && S >= 0 && n_max >= 0 && mode >= 0 && mode <= 2, "nms_bev: bad sizes");
  if (n_max > kNmsMax) {
    set_error("nms_bev: n_max=%d boxes per segment exceeds %d", n_max, kNmsMax);
    return DEMF_EUNSUPPORTED;
  }
  if (S == 0) return DEMF_OK;
  DEMF_REQUIRE(seg_start && seg_count && overflow && (R == 0 || (boxes && scores && keep)),
               "nms_bev: null pointer");
  hipLaunchKernelGGL(nms_bev_k, dim3(S), dim3(pow2_threads(n_max)), 0, (hipStream_t)stream, R, n_max, thr, mode,
                     boxes, scores, seg_start, seg_count, valid, keep, overflow);
  return check_launch("nms_bev");
}

extern "C" int demf_tta_merge(int B, int V, int C, int K, float thr, int mode, int max_num, const float* view_boxes,
                              const float* view_scores, const int* view_labels, const int* view_scene_off,
                              const int* view_state, int first_view_scene, int view_max_scenes, int view_max_rows,
                              const float* params, float* ws_boxes, float* ws_scores, int* ws_seg,
                              unsigned char* ws_keep, int first_scene, int max_scenes, int max_rows, float* boxes,
                              float* scores, int* labels, int* scene_off, int* state, demf_stream_t stream) {
  DEMF_REQUIRE(B >= 0 && V >= 1 && C >= 1 && K >= 0 && mode >= 0 && mode <= 2 && max_num >= 0 &&
                   first_view_scene >= 0 && view_max_rows >= 0 && first_scene >= 0 && max_rows >= 0 &&
                   (long long)first_view_scene + (long long)V * B <= view_max_scenes &&
                   (long long)first_scene + B <= max_scenes,
               "tta_merge: bad sizes");
  const long long vk = (long long)V * K;
  if (vk > kNmsMax || vk * C > kMergeMaxCand) {
    set_error("tta_merge: V * K = %lld rows per class (at most %d) and V * K * C = %lld candidates per scene (at "
              "most %d)", vk, kNmsMax, vk * C, kMergeMaxCand);
    return DEMF_EUNSUPPORTED;
  }
  if (B == 0) return DEMF_OK;
  DEMF_REQUIRE(view_scene_off && params && ws_seg && scene_off && state &&
                   (max_rows == 0 || (boxes && scores && labels)) &&
                   (view_max_rows == 0 || (view_boxes && view_scores && view_labels)) &&
                   (vk == 0 || (ws_boxes && ws_scores && ws_keep)),
               "tta_merge: null pointer");
  const int VK = (int)vk, S = B * C;
  int cap = 1;
  while (cap < VK * C) cap <<= 1;
  const int lds = cap * 8;
  if (lds > 64 * 1024 && !reserve_lds((const void*)tta_finish_k, lds, &g_finish_lds_done)) {
    set_error("tta_merge: the device does not offer %d bytes of LDS to one workgroup", lds);
    return DEMF_EUNSUPPORTED;
  }
  int* seg_start = ws_seg;                 // (S)
  int* seg_count = ws_seg + S;             // (S)
  int* ws_flag = ws_seg + 2 * S;           // (1)
  hipLaunchKernelGGL(tta_gather_k, dim3(C, B), dim3(kGatherThreads), 0, (hipStream_t)stream, B, V, C, VK, view_boxes,
                     view_scores, view_labels, view_scene_off, first_view_scene, view_max_rows, params, ws_boxes,
                     ws_scores, seg_start, seg_count, ws_flag);
  int rc = check_launch("tta_merge (gather)");
  if (rc != DEMF_OK) return rc;
  hipLaunchKernelGGL(nms_bev_k, dim3(S), dim3(pow2_threads(VK)), 0, (hipStream_t)stream, S * VK, VK, thr, mode,
                     ws_boxes, ws_scores, seg_start, seg_count, (const unsigned char*)nullptr, ws_keep, ws_flag);
  rc = check_launch("tta_merge (nms)");
  if (rc != DEMF_OK) return rc;
  hipLaunchKernelGGL(tta_finish_k, dim3(B), dim3(kFinishThreads), lds, (hipStream_t)stream, B, C, VK, cap, max_num,
                     ws_boxes, ws_scores, seg_count, ws_keep, ws_flag, view_state, first_scene, max_rows, boxes,
                     scores, labels, scene_off, state);
  return check_launch("tta_merge (finish)");
}
