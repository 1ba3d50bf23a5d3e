// Test side of the image branch's 2D detector (Deformable DETR, configs/deformdetr/imvotenet_image.py:21-80):
// what its decoder and head add to the kernels the frozen image stream already has.
//
//   demf_attn_fwd_eval   inference self-attention for any query count (the decoder's 300 learned queries;
//                        demf_attn_core_fwd is built for the fusion layer's 256): K and V of one (scene, head) in
//                        LDS, an online softmax per query row, no dropout, no statistics, no score tensor.
//   demf_detr2d_head     the last layer's class branch (256 -> C) and the last Linear of its box branch (256 -> 4)
//                        with mmdet's epilogue: + inverse_sigmoid(reference) on (cx, cy), sigmoid.
//   demf_detr2d_select   mmdet DeformableDETRHead._get_bboxes_single for a whole batch in one launch: top-k of
//                        the Q*C scores, label / query split, cxcywh -> xyxy, scale to img_shape, clamp, rescale,
//                        + the score filter of ImVoteNet.extract_bboxes_2d
//                        (demf/modeling/detectors/imvotenet_deform.py:181-239).
#include "common.h"

namespace demf {

// ---- (a) attention ---------------------------------------------------------------------------------------------
constexpr int AE_D = 32;                 // channels per head
constexpr int AE_LD = AE_D + 4;          // LDS row stride: the 8 keys a row's 8 lanes read hit 8 different bank groups
constexpr int AE_RB = 64;                // query rows per workgroup: 32 groups of 8 lanes, two rows per group
constexpr int AE_KC = 4;                 // keys per lane between two rescales of the running sums

template <bool BF>
__device__ __forceinline__ float ae_rnd(float x) {
  if constexpr (BF) return (float)(__bf16)x;
  return x;
}

// One workgroup = 64 query rows of one (scene, head) against all Q keys.  Lane group g (8 lanes) owns rows 2g and
// 2g + 1 of the block; lane part p of the group visits keys p, p + 8, p + 16, ... - a K / V row read from LDS feeds
// two query rows.  Per chunk of AE_KC keys a lane rescales its running (max, sum, 32-channel accumulator) once;
// the 8 partial results of a row are merged with xor shuffles at the end.  Rows >= Q read row Q - 1 and store
// nothing; keys >= Q score -inf (probability exactly 0).
template <bool BF>
__global__ __launch_bounds__(256) void attn_eval_kernel(int H, int Q, const float* __restrict__ qkv, float scale,
                                                        float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Ks = smem;
  float* Vs = smem + (size_t)Q * AE_LD;
  const int tid = threadIdx.x;
  const int nrb = (Q + AE_RB - 1) / AE_RB;
  const int bh = blockIdx.x / nrb, rb = blockIdx.x % nrb;
  const int b = bh / H, h = bh % H;
  const int E = H * AE_D;
  const size_t ld3 = 3 * (size_t)E;
  const float* base = qkv + (size_t)b * Q * ld3 + h * AE_D;
  for (int f = tid; f < Q * 8; f += 256) {
    const int row = f >> 3, d4 = f & 7;
    float4 k = *reinterpret_cast<const float4*>(base + (size_t)row * ld3 + E + 4 * d4);
    float4 v = *reinterpret_cast<const float4*>(base + (size_t)row * ld3 + 2 * E + 4 * d4);
    k.x = ae_rnd<BF>(k.x); k.y = ae_rnd<BF>(k.y); k.z = ae_rnd<BF>(k.z); k.w = ae_rnd<BF>(k.w);
    v.x = ae_rnd<BF>(v.x); v.y = ae_rnd<BF>(v.y); v.z = ae_rnd<BF>(v.z); v.w = ae_rnd<BF>(v.w);
    *reinterpret_cast<float4*>(Ks + row * AE_LD + 4 * d4) = k;
    *reinterpret_cast<float4*>(Vs + row * AE_LD + 4 * d4) = v;
  }
  const int part = tid & 7, grp = tid >> 3;
  const int row0 = rb * AE_RB + 2 * grp;
  float qr[2][AE_D], acc[2][AE_D], m[2], l[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int row = min(row0 + r, Q - 1);
    const float* qp = base + (size_t)row * ld3;
#pragma unroll
    for (int d4 = 0; d4 < 8; ++d4) {
      const float4 x = *reinterpret_cast<const float4*>(qp + 4 * d4);
      qr[r][4 * d4] = ae_rnd<BF>(x.x); qr[r][4 * d4 + 1] = ae_rnd<BF>(x.y);
      qr[r][4 * d4 + 2] = ae_rnd<BF>(x.z); qr[r][4 * d4 + 3] = ae_rnd<BF>(x.w);
    }
#pragma unroll
    for (int d = 0; d < AE_D; ++d) acc[r][d] = 0.f;
    m[r] = -1e30f;     // finite: a lane that never sees a key (Q < 8) merges with weight exp(-1e30 - max) = 0
    l[r] = 0.f;
  }
  __syncthreads();
  const float ninf = -__builtin_inff();
  for (int j0 = part; j0 < Q; j0 += 8 * AE_KC) {
    float s[2][AE_KC];
#pragma unroll
    for (int i = 0; i < AE_KC; ++i) {
      const int j = j0 + 8 * i;
      const int jr = min(j, Q - 1);
      const float* kp = Ks + jr * AE_LD;
      float d0 = 0.f, d1 = 0.f;
#pragma unroll
      for (int d4 = 0; d4 < 8; ++d4) {
        const float4 k = *reinterpret_cast<const float4*>(kp + 4 * d4);
        d0 = __builtin_fmaf(qr[0][4 * d4], k.x, d0); d1 = __builtin_fmaf(qr[1][4 * d4], k.x, d1);
        d0 = __builtin_fmaf(qr[0][4 * d4 + 1], k.y, d0); d1 = __builtin_fmaf(qr[1][4 * d4 + 1], k.y, d1);
        d0 = __builtin_fmaf(qr[0][4 * d4 + 2], k.z, d0); d1 = __builtin_fmaf(qr[1][4 * d4 + 2], k.z, d1);
        d0 = __builtin_fmaf(qr[0][4 * d4 + 3], k.w, d0); d1 = __builtin_fmaf(qr[1][4 * d4 + 3], k.w, d1);
      }
      s[0][i] = j < Q ? d0 * scale : ninf;
      s[1][i] = j < Q ? d1 * scale : ninf;
    }
    float p[2][AE_KC];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      float mx = m[r];
#pragma unroll
      for (int i = 0; i < AE_KC; ++i) mx = fmaxf(mx, s[r][i]);
      const float corr = __expf(m[r] - mx);
      m[r] = mx;
      float sum = l[r] * corr;
#pragma unroll
      for (int i = 0; i < AE_KC; ++i) { p[r][i] = __expf(s[r][i] - mx); sum += p[r][i]; p[r][i] = ae_rnd<BF>(p[r][i]); }
      l[r] = sum;
#pragma unroll
      for (int d = 0; d < AE_D; ++d) acc[r][d] *= corr;
    }
#pragma unroll
    for (int i = 0; i < AE_KC; ++i) {
      const int jr = min(j0 + 8 * i, Q - 1);      // (a key past the end carries p = 0)
      const float* vp = Vs + jr * AE_LD;
#pragma unroll
      for (int d4 = 0; d4 < 8; ++d4) {
        const float4 v = *reinterpret_cast<const float4*>(vp + 4 * d4);
        acc[0][4 * d4] = __builtin_fmaf(p[0][i], v.x, acc[0][4 * d4]);
        acc[1][4 * d4] = __builtin_fmaf(p[1][i], v.x, acc[1][4 * d4]);
        acc[0][4 * d4 + 1] = __builtin_fmaf(p[0][i], v.y, acc[0][4 * d4 + 1]);
        acc[1][4 * d4 + 1] = __builtin_fmaf(p[1][i], v.y, acc[1][4 * d4 + 1]);
        acc[0][4 * d4 + 2] = __builtin_fmaf(p[0][i], v.z, acc[0][4 * d4 + 2]);
        acc[1][4 * d4 + 2] = __builtin_fmaf(p[1][i], v.z, acc[1][4 * d4 + 2]);
        acc[0][4 * d4 + 3] = __builtin_fmaf(p[0][i], v.w, acc[0][4 * d4 + 3]);
        acc[1][4 * d4 + 3] = __builtin_fmaf(p[1][i], v.w, acc[1][4 * d4 + 3]);
      }
    }
  }
  // merge the 8 lanes of a row; lane `part` stores channels 4 part .. 4 part + 3
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    float mx = m[r];
    mx = fmaxf(mx, __shfl_xor(mx, 1)); mx = fmaxf(mx, __shfl_xor(mx, 2)); mx = fmaxf(mx, __shfl_xor(mx, 4));
    const float w = __expf(m[r] - mx);
    float sum = l[r] * w;
    sum += __shfl_xor(sum, 1); sum += __shfl_xor(sum, 2); sum += __shfl_xor(sum, 4);
    const float inv = 1.0f / sum;
    const int row = row0 + r;
    float* op = out + ((size_t)b * Q + min(row, Q - 1)) * E + h * AE_D;
#pragma unroll
    for (int d4 = 0; d4 < 8; ++d4) {
      float o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float x = acc[r][4 * d4 + e] * w;
        x += __shfl_xor(x, 1); x += __shfl_xor(x, 2); x += __shfl_xor(x, 4);
        o[e] = x * inv;
      }
      if (part == d4 && row < Q) *reinterpret_cast<float4*>(op + 4 * d4) = make_float4(o[0], o[1], o[2], o[3]);
    }
  }
}

// ---- (b) head tail ---------------------------------------------------------------------------------------------
// One wave per row: lane l holds channels 4l + 256 i of the row (K <= 1024), C + 4 wave-reduced dot products.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }

// mmdet.models.utils.transformer.inverse_sigmoid(x, eps = 1e-5)
__device__ __forceinline__ float inverse_sigmoid_f(float x) {
  x = fminf(fmaxf(x, 0.f), 1.f);
  const float x1 = fmaxf(x, 1e-5f), x2 = fmaxf(1.0f - x, 1e-5f);
  return logf(x1 / x2);
}

__global__ __launch_bounds__(256) void detr2d_head_kernel(int R, int C, int K, const float* __restrict__ hs,
                                                          const float* __restrict__ hid, const float* __restrict__ wc,
                                                          const float* __restrict__ bc, const float* __restrict__ wr,
                                                          const float* __restrict__ br, const float* __restrict__ ref,
                                                          int ref_rows, float* __restrict__ logits,
                                                          float* __restrict__ boxes) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;                      // (whole waves; no barrier below)
  const int K4 = K >> 2;
  float4 x[4], y[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k4 = lane + 64 * i;
    x[i] = y[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (k4 < K4) {
      x[i] = *reinterpret_cast<const float4*>(hs + (size_t)r * K + 4 * k4);
      y[i] = *reinterpret_cast<const float4*>(hid + (size_t)r * K + 4 * k4);
    }
  }
  auto dot = [&](const float4 (&a)[4], const float* __restrict__ w) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k4 = lane + 64 * i;
      if (k4 < K4) {
        const float4 v = *reinterpret_cast<const float4*>(w + 4 * k4);
        s = __builtin_fmaf(a[i].x, v.x, s); s = __builtin_fmaf(a[i].y, v.y, s);
        s = __builtin_fmaf(a[i].z, v.z, s); s = __builtin_fmaf(a[i].w, v.w, s);
      }
    }
    return wave_sum(s);
  };
  for (int c = 0; c < C; ++c) {
    const float v = dot(x, wc + (size_t)c * K) + bc[c];
    if (lane == 0) logits[(size_t)r * C + c] = v;
  }
  float t[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) t[c] = dot(y, wr + (size_t)c * K) + br[c];
  if (lane == 0) {
    const float* rp = ref + 2 * (size_t)(r % ref_rows);
    t[0] += inverse_sigmoid_f(rp[0]);
    t[1] += inverse_sigmoid_f(rp[1]);
    *reinterpret_cast<float4*>(boxes + 4 * (size_t)r) =
        make_float4(sigmoid_f(t[0]), sigmoid_f(t[1]), sigmoid_f(t[2]), sigmoid_f(t[3]));
  }
}

// ---- (c) selection ---------------------------------------------------------------------------------------------
constexpr int SEL_THREADS = 1024;

// ascending 64-bit key = (logit descending, flat index ascending); NaN after every number, padding after NaN
__device__ __forceinline__ unsigned long long sel_key(float v, unsigned idx) {
  unsigned u = __builtin_bit_cast(unsigned, v);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);       // ascending in v
  unsigned hi = ~u;                                     // descending in v; -inf -> 0xFF800000
  if (v != v) hi = 0xFFFFFFFEu;
  return ((unsigned long long)hi << 32) | idx;
}

// One workgroup per image: a bitonic sort of the Q*C keys (padded to a power of two) in LDS, then thread i < k
// decodes place i.
__global__ __launch_bounds__(SEL_THREADS) void detr2d_select_kernel(int Q, int C, int k, int P2,
                                                                    const float* __restrict__ logits,
                                                                    const float* __restrict__ boxes,
                                                                    const float* __restrict__ meta, int rescale, float thr,
                                                                    float* __restrict__ rows, int* __restrict__ counts,
                                                                    int* __restrict__ flag) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];
  __shared__ int s_count, s_nan;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int N = Q * C;
  const float* lg = logits + (size_t)b * N;
  if (tid == 0) { s_count = 0; s_nan = 0; }
  __syncthreads();
  bool nan = false;
  for (int i = tid; i < P2; i += SEL_THREADS) {
    unsigned long long key = ~0ull;
    if (i < N) {
      const float v = lg[i];
      nan |= v != v;
      key = sel_key(v, (unsigned)i);
    }
    keys[i] = key;
  }
  if (nan) s_nan = 1;
  __syncthreads();
  for (int size = 2; size <= P2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < (P2 >> 1); t += SEL_THREADS) {
        const int lo = ((t & ~(stride - 1)) << 1) | (t & (stride - 1));
        const int hi = lo | stride;
        const bool up = (lo & size) == 0;
        const unsigned long long a = keys[lo], c = keys[hi];
        if ((a > c) == up) { keys[lo] = c; keys[hi] = a; }
      }
      __syncthreads();
    }
  }
  const int kk = min(k, N);
  float row[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (tid < kk) {
    const unsigned idx = (unsigned)(keys[tid] & 0xFFFFFFFFull);
    const float score = sigmoid_f(lg[idx]);
    if (thr < 0.f || score > thr) {
      const int q = (int)(idx / (unsigned)C), c = (int)(idx % (unsigned)C);
      const float4 bx = *reinterpret_cast<const float4*>(boxes + 4 * ((size_t)b * Q + q));
      const float* mt = meta + 6 * (size_t)b;
      const float ih = mt[0], iw = mt[1];
      float x1 = (bx.x - 0.5f * bx.z) * iw, y1 = (bx.y - 0.5f * bx.w) * ih;
      float x2 = (bx.x + 0.5f * bx.z) * iw, y2 = (bx.y + 0.5f * bx.w) * ih;
      x1 = fminf(fmaxf(x1, 0.f), iw); x2 = fminf(fmaxf(x2, 0.f), iw);
      y1 = fminf(fmaxf(y1, 0.f), ih); y2 = fminf(fmaxf(y2, 0.f), ih);
      if (rescale) { x1 /= mt[2]; y1 /= mt[3]; x2 /= mt[4]; y2 /= mt[5]; }
      row[0] = x1; row[1] = y1; row[2] = x2; row[3] = y2; row[4] = score; row[5] = (float)c;
      atomicAdd(&s_count, 1);
    }
  }
  if (tid < k) {
    float* rp = rows + 6 * ((size_t)b * k + tid);
#pragma unroll
    for (int e = 0; e < 6; ++e) rp[e] = row[e];
  }
  __syncthreads();
  if (tid == 0) {
    counts[b] = s_count;
    if (s_nan) atomicOr(flag, 1);
  }
}

}  // namespace demf

using namespace demf;

extern "C" int demf_attn_fwd_eval(int B, int H, int Q, int Dh, const float* qkv, float scale, float* out,
                                  demf_stream_t stream) {
  DEMF_REQUIRE(B >= 0 && H >= 1 && Q >= 1 && Dh >= 1, "attn_fwd_eval: bad sizes B=%d H=%d Q=%d Dh=%d", B, H, Q, Dh);
  if (Q > DEMF_ATTN_EVAL_MAX_Q || Dh != AE_D) {
    set_error("attn_fwd_eval: built for at most %d queries x %d channels per head (got %d x %d)",
              DEMF_ATTN_EVAL_MAX_Q, AE_D, Q, Dh);
    return DEMF_EUNSUPPORTED;
  }
  if (B == 0) return DEMF_OK;
  DEMF_REQUIRE(qkv && out, "attn_fwd_eval: null pointer");
  DEMF_REQUIRE(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)out & 15) == 0, "attn_fwd_eval: pointers must be 16-byte aligned");
  const long long blocks = (long long)B * H * ((Q + AE_RB - 1) / AE_RB);
  DEMF_REQUIRE(blocks < (1ll << 31), "attn_fwd_eval: bad sizes (too many workgroups)");
  const int max_bytes = 2 * DEMF_ATTN_EVAL_MAX_Q * AE_LD * (int)sizeof(float);
  static unsigned long long reserved[2] = {0, 0};      // per kernel instantiation: bit per device
  const bool bf = compute_bf16();
  const void* fn = bf ? reinterpret_cast<const void*>(&attn_eval_kernel<true>)
                      : reinterpret_cast<const void*>(&attn_eval_kernel<false>);
  if (!reserve_lds(fn, max_bytes, &reserved[bf ? 1 : 0])) {
    set_error("attn_fwd_eval: cannot reserve %d bytes of LDS", max_bytes);
    return DEMF_ELAUNCH;
  }
  const size_t bytes = 2 * (size_t)Q * AE_LD * sizeof(float);
  if (bf) hipLaunchKernelGGL(attn_eval_kernel<true>, dim3((unsigned)blocks), dim3(256), bytes, (hipStream_t)stream, H, Q, qkv, scale, out);
  else hipLaunchKernelGGL(attn_eval_kernel<false>, dim3((unsigned)blocks), dim3(256), bytes, (hipStream_t)stream, H, Q, qkv, scale, out);
  return check_launch("attn_fwd_eval");
}

extern "C" int demf_detr2d_head(int R, int C, int K, const float* hs, const float* hidden, const float* w_cls,
                                const float* b_cls, const float* w_reg, const float* b_reg, const float* reference,
                                int ref_rows, float* logits, float* boxes, demf_stream_t stream) {
  DEMF_REQUIRE(R >= 0 && C >= 1 && K >= 4 && K % 4 == 0 && ref_rows >= 1, "detr2d_head: bad sizes R=%d C=%d K=%d ref_rows=%d",
               R, C, K, ref_rows);
  if (C > DEMF_DETR2D_MAX_CLASSES || K > 1024) {
    set_error("detr2d_head: at most %d classes and 1024 channels (got %d and %d)", DEMF_DETR2D_MAX_CLASSES, C, K);
    return DEMF_EUNSUPPORTED;
  }
  if (R == 0) return DEMF_OK;
  DEMF_REQUIRE(hs && hidden && w_cls && b_cls && w_reg && b_reg && reference && logits && boxes,
               "detr2d_head: null pointer");
  DEMF_REQUIRE((((uintptr_t)hs | (uintptr_t)hidden | (uintptr_t)w_cls | (uintptr_t)w_reg | (uintptr_t)boxes) & 15) == 0,
               "detr2d_head: pointers must be 16-byte aligned");
  hipLaunchKernelGGL(detr2d_head_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, (hipStream_t)stream, R, C, K, hs,
                     hidden, w_cls, b_cls, w_reg, b_reg, reference, ref_rows, logits, boxes);
  return check_launch("detr2d_head");
}

extern "C" int demf_detr2d_select(int B, int Q, int C, int k, const float* logits, const float* boxes,
                                  const float* meta, int rescale, float thr, float* rows, int* counts, int* flag,
                                  demf_stream_t stream) {
  DEMF_REQUIRE(B >= 0 && Q >= 1 && C >= 1 && k >= 1, "detr2d_select: bad sizes B=%d Q=%d C=%d k=%d", B, Q, C, k);
  if ((long long)Q * C > DEMF_DETR2D_MAX_CANDIDATES || k > DEMF_DETR2D_MAX_K) {
    set_error("detr2d_select: %lld candidates per image and k = %d; at most %d and %d are supported", (long long)Q * C, k,
              DEMF_DETR2D_MAX_CANDIDATES, DEMF_DETR2D_MAX_K);
    return DEMF_EUNSUPPORTED;
  }
  if (B == 0) return DEMF_OK;
  DEMF_REQUIRE(logits && boxes && meta && rows && counts && flag, "detr2d_select: null pointer");
  DEMF_REQUIRE(((uintptr_t)boxes & 15) == 0, "detr2d_select: boxes must be 16-byte aligned");
  int P2 = 2;
  while (P2 < Q * C) P2 <<= 1;
  static unsigned long long reserved = 0;
  const int max_bytes = DEMF_DETR2D_MAX_CANDIDATES * (int)sizeof(unsigned long long);
  if (!reserve_lds(reinterpret_cast<const void*>(&detr2d_select_kernel), max_bytes, &reserved)) {
    set_error("detr2d_select: cannot reserve %d bytes of LDS", max_bytes);
    return DEMF_ELAUNCH;
  }
  hipLaunchKernelGGL(detr2d_select_kernel, dim3(B), dim3(SEL_THREADS), (size_t)P2 * sizeof(unsigned long long),
                     (hipStream_t)stream, Q, C, k, P2, logits, boxes, meta, rescale, thr, rows, counts, flag);
  return check_launch("detr2d_select");
}
