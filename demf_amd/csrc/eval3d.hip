// Indoor 3D detection evaluation (mmdet3d 0.18.1 indoor_eval / eval_det_cls / average_precision,
// as SUNRGBDDataset.evaluate calls them for `eval.py --eval mAP`): rotated-box 3D IoU of depth boxes,
// the greedy score-order matching of detections to ground truth, and the VOC-area AP scan.
// Boxes are upstream's bottom-centre form (x, y, z_bottom, dx, dy, dz, yaw).  All IoU arithmetic
// is fp32 (build: -ffp-contract=off), the AP scan fp64.
#include <hip/hip_runtime.h>

#include "bev_clip.h"   // clip_half_plane, bev_overlap, box3d_iou (shared with csrc/tta.hip)
#include "common.h"

namespace demf {

namespace {

constexpr int kMatchThreads = 256;
constexpr int kMatchMaxGt = DEMF_EVAL_MAX_GT_PER_SEGMENT;      // ground-truth boxes of one (class, scene) segment
constexpr int kMatchMaxPred = DEMF_EVAL_MAX_PRED_PER_SEGMENT;  // detections of one (class, scene) segment
constexpr int kApThreads = 512;
constexpr int kApPerThread = 16;     // consecutive detections per thread and chunk
constexpr int kMaxThr = 4;

struct Thresholds {
  float v[kMaxThr];
};

__global__ __launch_bounds__(256) void box3d_iou_k(int N, int M, const float* __restrict__ b1,
                                                   const float* __restrict__ b2, float* __restrict__ iou) {
  const long long total = (long long)N * M;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const long long n = e / M, m = e - n * M;
    float a[7], b[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      a[k] = b1[n * 7 + k];
      b[k] = b2[m * 7 + k];
    }
    iou[e] = box3d_iou(a, b);
  }
}

// One workgroup per (class, scene) segment s: detections order[pred_off[s] .. pred_off[s+1]) in score
// order, ground truth gt[gt_off[s] .. gt_off[s+1]).  Per detection: iou_max over the segment's GT and
// jmax = the first GT reaching it (upstream's strict `>` loop from -inf).  The greedy pass of
// eval_det_cls makes a detection TP at threshold t iff iou_max > t and GT jmax is not yet taken, and a
// detection never falls back to another GT: so TP(i, t) iff i is the FIRST detection, in score order,
// with that jmax and iou_max > t.  An LDS atomicMin per (t, GT) finds those firsts without a serial pass.
__global__ __launch_bounds__(kMatchThreads) void eval_match_k(int T, Thresholds thr, const float* __restrict__ pred,
                                                              const int* __restrict__ order,
                                                              const int* __restrict__ pred_off,
                                                              const float* __restrict__ gt,
                                                              const int* __restrict__ gt_off,
                                                              unsigned char* __restrict__ tp) {
  __shared__ float s_gt[kMatchMaxGt * 7];
  __shared__ int s_info[kMatchMaxPred];          // (jmax + 1) << 4 | pass mask over thresholds
  __shared__ int s_first[kMaxThr][kMatchMaxGt];
  const int s = blockIdx.x;
  const int p0 = pred_off[s], np = pred_off[s + 1] - p0;
  const int g0 = gt_off[s], ng = gt_off[s + 1] - g0;
  // sizes are validated by the host entry; a segment that still breaks them is left alone
  if (np <= 0 || np > kMatchMaxPred || ng < 0 || ng > kMatchMaxGt) return;
  for (int e = threadIdx.x; e < ng * 7; e += kMatchThreads) s_gt[e] = gt[(size_t)g0 * 7 + e];
  for (int e = threadIdx.x; e < kMaxThr * kMatchMaxGt; e += kMatchThreads) (&s_first[0][0])[e] = 0x7fffffff;
  __syncthreads();
  for (int i = threadIdx.x; i < np; i += kMatchThreads) {
    const size_t row = (size_t)order[p0 + i];
    float a[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) a[k] = pred[row * 7 + k];
    float best = -__builtin_inff();
    int jmax = -1;
    for (int g = 0; g < ng; ++g) {
      const float v = box3d_iou(a, s_gt + g * 7);
      if (v > best) {
        best = v;
        jmax = g;
      }
    }
    int mask = 0;
    for (int t = 0; t < T; ++t) {
      if (jmax >= 0 && best > thr.v[t]) {
        mask |= 1 << t;
        atomicMin(&s_first[t][jmax], i);
      }
    }
    s_info[i] = ((jmax + 1) << 4) | mask;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < np; i += kMatchThreads) {
    const size_t row = (size_t)order[p0 + i];
    const int info = s_info[i], j = (info >> 4) - 1;
    for (int t = 0; t < T; ++t)
      tp[row * T + t] = ((info >> t) & 1) && s_first[t][j] == i ? 1 : 0;
  }
}

// exclusive prefix sum over the workgroup (kApThreads lanes); every thread gets the total
__device__ __forceinline__ int block_excl_sum(int v, int* s_wave, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int x = v;
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  if (lane == 63) s_wave[w] = x;
  __syncthreads();
  int before = 0;
  total = 0;
  for (int k = 0; k < kApThreads / 64; ++k) {
    const int c = s_wave[k];
    before += k < w ? c : 0;
    total += c;
  }
  __syncthreads();
  return before + x - v;
}

// inclusive suffix max over the workgroup (lane order); every thread gets the maximum of its own and
// all later threads' values
__device__ __forceinline__ double block_suffix_max(double v, double* s_wave) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double x = v;
  for (int d = 1; d < 64; d <<= 1) {
    const double y = __shfl_down(x, d);
    if (lane + d < 64) x = fmax(x, y);
  }
  if (lane == 0) s_wave[w] = x;
  __syncthreads();
  for (int k = w + 1; k < kApThreads / 64; ++k) x = fmax(x, s_wave[k]);
  __syncthreads();
  return x;
}

// One workgroup per class c: tp rows cls_off[c] .. cls_off[c+1) (T flags each) in the class's global score
// order.  average_precision(mode='area') over [0, rec, 1] / [0, prec, 0] equals
//     AP = (1/npos) * sum over TP positions k of max_{j >= k} prec_j,   prec_j = tp_cum_j / (j + 1),
// and between two TPs prec only falls, so that max is attained at a TP: with the m-th TP at position
// k_m,  AP = (1/npos) * sum_m max_{m' >= m} m' / (k_m' + 1).  Pass 1 compacts the TP positions of every
// threshold in order into the workspace (npos slots each: every TP takes a distinct GT), pass 2 runs the
// suffix max over those <= npos values.  rec = ntp / npos.  npos = 0 gives NaN for both (upstream's 0/0).
__global__ __launch_bounds__(kApThreads) void eval_ap_k(int T, const int* __restrict__ cls_off,
                                                        const int* __restrict__ npos_arr,
                                                        const int* __restrict__ ws_off,
                                                        const unsigned char* __restrict__ tp, int* __restrict__ ws,
                                                        double* __restrict__ ap, double* __restrict__ rec) {
  __shared__ int s_wave[kApThreads / 64];
  __shared__ double s_dwave[kApThreads / 64];
  __shared__ double s_carry;
  const int c = blockIdx.x;
  const int k0 = cls_off[c], n = cls_off[c + 1] - k0;
  const int npos = npos_arr[c];
  int* wsc = ws + (size_t)ws_off[c] * T;         // T lists of npos positions
  int ntp[kMaxThr] = {0, 0, 0, 0};
  for (int base = 0; base < n; base += kApThreads * kApPerThread) {
    const int first = base + threadIdx.x * kApPerThread;
    unsigned bits[kMaxThr] = {0u, 0u, 0u, 0u};
    for (int e = 0; e < kApPerThread; ++e) {
      const int k = first + e;
      if (k < n) {
        const unsigned char* row = tp + (size_t)(k0 + k) * T;
        for (int t = 0; t < T; ++t) bits[t] |= (row[t] ? 1u : 0u) << e;
      }
    }
    for (int t = 0; t < T; ++t) {
      int total;
      int at = ntp[t] + block_excl_sum(__popc(bits[t]), s_wave, total);
      for (unsigned b = bits[t]; b; b &= b - 1) {
        if (at < npos) wsc[(size_t)t * npos + at] = first + __ffs(b) - 1;
        ++at;
      }
      ntp[t] += total;
    }
  }
  // pass 2 reads positions other waves wrote in pass 1: make them visible to the whole workgroup
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    const int m_n = min(ntp[t], npos);
    const int* pos = wsc + (size_t)t * npos;
    double carry = 0.0, sum = 0.0;     // carry: the maximum over the later chunks' TPs (TP precisions are > 0)
    for (int end = m_n; end > 0; end -= kApThreads) {
      const int m = end - kApThreads + (int)threadIdx.x;     // 0-based TP rank; chunk [end - threads, end)
      const double v = m >= 0 ? (double)(m + 1) / (double)(pos[m] + 1) : 0.0;
      const double mx = fmax(block_suffix_max(v, s_dwave), carry);
      double part = m >= 0 ? mx : 0.0;
      for (int d = 32; d; d >>= 1) part += __shfl_xor(part, d);
      if ((threadIdx.x & 63) == 0) s_dwave[threadIdx.x >> 6] = part;
      if (threadIdx.x == 0) s_carry = mx;                   // thread 0's suffix covers the whole chunk
      __syncthreads();
      for (int k = 0; k < kApThreads / 64; ++k) sum += s_dwave[k];
      carry = s_carry;
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      const double nan = __builtin_nan("");
      ap[(size_t)c * T + t] = npos > 0 ? sum / (double)npos : nan;
      rec[(size_t)c * T + t] = npos > 0 ? (double)ntp[t] / (double)npos : nan;
    }
  }
}

}  // namespace

}  // namespace demf

using namespace demf;

extern "C" int demf_box3d_iou(int N, int M, const float* boxes1, const float* boxes2, float* iou,
                              demf_stream_t stream) {
  DEMF_REQUIRE(N >= 0 && M >= 0, "box3d_iou: bad sizes");
  if ((long long)N * M == 0) return DEMF_OK;
  DEMF_REQUIRE(boxes1 && boxes2 && iou, "box3d_iou: null pointer");
  const long long total = (long long)N * M;
  const int blocks = (int)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536);
  hipLaunchKernelGGL(box3d_iou_k, dim3(blocks), dim3(256), 0, (hipStream_t)stream, N, M, boxes1, boxes2, iou);
  return check_launch("box3d_iou");
}

extern "C" int demf_eval_match(int S, int T, const float* thresholds, int max_pred, int max_gt,
                               const float* pred_boxes, const int* order, const int* pred_off,
                               const float* gt_boxes, const int* gt_off, unsigned char* tp,
                               demf_stream_t stream) {
  DEMF_REQUIRE(S >= 0 && T >= 1 && T <= kMaxThr && max_pred >= 0 && max_gt >= 0, "eval_match: bad sizes");
  if (max_pred > kMatchMaxPred || max_gt > kMatchMaxGt) {
    set_error("eval_match: a (class, scene) segment holds %d detections and %d ground-truth boxes; "
              "at most %d and %d are supported", max_pred, max_gt, kMatchMaxPred, kMatchMaxGt);
    return DEMF_EUNSUPPORTED;
  }
  DEMF_REQUIRE(thresholds, "eval_match: null pointer");
  if (S == 0 || max_pred == 0) return DEMF_OK;
  DEMF_REQUIRE(pred_boxes && order && pred_off && gt_off && tp && (gt_boxes || max_gt == 0),
               "eval_match: null pointer");
  Thresholds thr = {};
  for (int t = 0; t < T; ++t) thr.v[t] = thresholds[t];
  hipLaunchKernelGGL(eval_match_k, dim3(S), dim3(kMatchThreads), 0, (hipStream_t)stream, T, thr, pred_boxes,
                     order, pred_off, gt_boxes, gt_off, tp);
  return check_launch("eval_match");
}

extern "C" int demf_eval_ap(int C, int T, const int* cls_off, const int* npos, const int* ws_off,
                            const unsigned char* tp_sorted, int* workspace, double* ap, double* rec,
                            demf_stream_t stream) {
  DEMF_REQUIRE(C >= 0 && T >= 1 && T <= kMaxThr, "eval_ap: bad sizes");
  if (C == 0) return DEMF_OK;
  DEMF_REQUIRE(cls_off && npos && ws_off && ap && rec, "eval_ap: null pointer");
  hipLaunchKernelGGL(eval_ap_k, dim3(C), dim3(kApThreads), 0, (hipStream_t)stream, T, cls_off, npos, ws_off,
                     tp_sorted, workspace, ap, rec);
  return check_launch("eval_ap");
}
