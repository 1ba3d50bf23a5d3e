// On-GPU input pipeline of SUN RGB-D scenes (configs/demf/demf_votenet.py:184-207): the per-point and per-pixel
// work of mmdet3d 0.18.1 LoadPointsFromFile(shift_height=True) / RandomFlip3D / GlobalRotScaleTrans / PointSample
// and of mmcv Resize(keep_ratio) / Normalize / Pad(32) + collate padding [dep-recall: restated from the upstream
// pipelines' published behaviour; their sources are not in the reference tree].  The host uploads the raw
// `.bin` records and the decoded uint8 images as they are; everything per point or per pixel happens here.
//   points_floor_k   0.99-percentile of z per scene (numpy's linear interpolation) by a 4-pass radix select
//   points_prep_k    keyed random subset (Feistel permutation) + flip / rotate / scale / translate + height
//   image_prep_k     bilinear resize (cv2 INTER_LINEAR coordinates) + uint8 rounding + normalise + zero pad
#include <hip/hip_runtime.h>

#include "common.h"
#include "rng.h"

namespace demf {

namespace {

constexpr int kFloorThreads = 1024;
constexpr int kFloorWaves = kFloorThreads / 64;
constexpr int kPrepThreads = 256;
constexpr int kImgThreads = 256;

// float -> uint32 key with the float order (-0.0 folded onto +0.0; NaN is not expected)
__device__ __forceinline__ uint32_t f2key(float f) {
  uint32_t u = __float_as_uint(f);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// One full wave: tot[256] bin counts, `rank` (0-based) among the counted keys -> the bin holding it and the rank
// within that bin.  Lane l owns bins 4l .. 4l+3.
__device__ __forceinline__ void select_digit(const uint32_t* tot, uint32_t rank, uint32_t* digit, uint32_t* rank_out) {
  const int lane = threadIdx.x & 63;
  const uint32_t c0 = tot[4 * lane], c1 = tot[4 * lane + 1], c2 = tot[4 * lane + 2], c3 = tot[4 * lane + 3];
  const uint32_t s = c0 + c1 + c2 + c3;
  uint32_t incl = s;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(incl, d);
    if (lane >= d) incl += y;
  }
  const uint32_t excl = incl - s;
  if (excl <= rank && rank < incl) {
    const uint32_t c[4] = {c0, c1, c2, c3};
    uint32_t acc = excl;
    for (int k = 0; k < 4; ++k) {
      if (rank < acc + c[k]) {
        *digit = 4 * lane + k;
        *rank_out = rank - acc;
        break;
      }
      acc += c[k];
    }
  }
}

// One workgroup per scene.  Ranks lo = floor(v) and hi = min(lo + 1, N - 1) of v = (N - 1) * 0.0099 are selected
// together: each pass histograms the next 8-bit digit of the keys that match each rank's prefix so far (one LDS copy
// per wave and rank; a single histogram while both prefixes agree).  z is re-read from the records every pass.
__global__ __launch_bounds__(kFloorThreads) void points_floor_k(int load_dim, long long total,
                                                                const float* __restrict__ raw,
                                                                const int64_t* __restrict__ off,
                                                                float* __restrict__ floor_out) {
  __shared__ uint32_t s_hist[2][kFloorWaves][256];
  __shared__ uint32_t s_tot[2][256];
  __shared__ uint32_t s_sel[4];          // digit lo, rank lo, digit hi, rank hi
  const int b = blockIdx.x;
  const long long p0 = off[b], p1 = off[b + 1];
  if (p0 < 0 || p1 <= p0 || p1 > total) {                      // empty or inconsistent scene
    if (threadIdx.x == 0) floor_out[b] = __builtin_nanf("");
    return;
  }
  const long long n = p1 - p0;
  const double vi = (double)(n - 1) * (0.99 / 100.0);         // numpy: (n - 1) * (q / 100)
  const double flo = floor(vi);
  const long long ilo = (long long)flo, ihi = ilo + 1 < n ? ilo + 1 : n - 1;
  const float* z = raw + p0 * load_dim + 2;
  const int w = threadIdx.x >> 6;
  uint32_t pre_lo = 0, pre_hi = 0, mask = 0;
  uint32_t rank_lo = (uint32_t)ilo, rank_hi = (uint32_t)ihi;
  for (int shift = 24; shift >= 0; shift -= 8) {
    const bool same = pre_lo == pre_hi;
    for (int e = threadIdx.x; e < 2 * kFloorWaves * 256; e += kFloorThreads) (&s_hist[0][0][0])[e] = 0u;
    __syncthreads();
    for (long long i = threadIdx.x; i < n; i += kFloorThreads) {
      const uint32_t key = f2key(z[i * load_dim]);
      const uint32_t dig = (key >> shift) & 255u;
      if (((key ^ pre_lo) & mask) == 0u) atomicAdd(&s_hist[0][w][dig], 1u);
      if (!same && ((key ^ pre_hi) & mask) == 0u) atomicAdd(&s_hist[1][w][dig], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 512) {
      const int h = threadIdx.x >> 8, bin = threadIdx.x & 255;
      uint32_t t = 0;
      for (int k = 0; k < kFloorWaves; ++k) t += s_hist[h][k][bin];
      s_tot[h][bin] = t;
    }
    __syncthreads();
    if (w == 0) select_digit(s_tot[0], rank_lo, &s_sel[0], &s_sel[1]);
    else if (w == 1) select_digit(s_tot[same ? 0 : 1], rank_hi, &s_sel[2], &s_sel[3]);
    __syncthreads();
    pre_lo |= s_sel[0] << shift;
    rank_lo = s_sel[1];
    pre_hi |= s_sel[2] << shift;
    rank_hi = s_sel[3];
    mask |= 255u << shift;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    // numpy _lerp on the two float32 order statistics: diff = b - a in float32, the rest in float64
    const float a = key2f(pre_lo), bb = key2f(pre_hi);
    const double t = vi - flo;
    const double d = (double)(bb - a);
    const double r = t >= 0.5 ? (double)bb - d * (1.0 - t) : (double)a + d * t;
    floor_out[b] = (float)r;
  }
}

// ---- keyed bijection on [0, n): Feistel network on 2h bits, cycle-walked into [0, n) ---------------------------------
struct FeistelKey {
  uint32_t k[6];
};
__device__ __forceinline__ FeistelKey feistel_key(unsigned long long seed) {
  FeistelKey fk;
  uint32_t h = mix32((uint32_t)seed ^ 0x9E3779B9u);
  h = mix32(h ^ (uint32_t)(seed >> 32));
  for (int r = 0; r < 6; ++r) {
    h = mix32(h + 0x632BE5ABu * (uint32_t)(r + 1));
    fk.k[r] = h;
  }
  return fk;
}
__device__ __forceinline__ uint32_t feistel(uint32_t x, int h, uint32_t m, const FeistelKey& fk) {
  uint32_t L = x >> h, R = x & m;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const uint32_t nl = R;
    R = L ^ (mix32(R ^ fk.k[r]) & m);
    L = nl;
  }
  return (L << h) | R;
}

// Grid (ceil(k / 256), B).  prm (B, 8) fp32 = [flip, cos, sin, scale, tx, ty, tz, -]; the arithmetic is
// data.augment_3d's: x -> -x, p @ rotation_z(angle)^T, * scale, + trans; height = (z_raw - floor) * scale.
__global__ __launch_bounds__(kPrepThreads) void points_prep_k(int k, int load_dim, long long total,
                                                              const float* __restrict__ raw,
                                                              const int64_t* __restrict__ off,
                                                              const float* __restrict__ floor_in,
                                                              const float* __restrict__ prm,
                                                              const int64_t* __restrict__ seeds,
                                                              float4* __restrict__ out, int* __restrict__ src_idx) {
  const int b = blockIdx.y;
  const int j = blockIdx.x * kPrepThreads + threadIdx.x;
  if (j >= k) return;
  const size_t o = (size_t)b * k + j;
  const long long p0 = off[b], p1 = off[b + 1];
  if (p0 < 0 || p1 <= p0 || p1 > total) {
    const float nan = __builtin_nanf("");
    out[o] = make_float4(nan, nan, nan, nan);
    if (src_idx) src_idx[o] = -1;
    return;
  }
  const uint32_t n = (uint32_t)(p1 - p0);
  const unsigned long long seed = (unsigned long long)seeds[b];
  uint32_t src;
  if (n >= (uint32_t)k) {
    int bits = 32 - __clz(n - 1u);                      // n <= 2^bits
    if (bits < 2) bits = 2;
    bits += bits & 1;                                   // even number of bits: two halves of h
    const int h = bits >> 1;
    const uint32_t m = (1u << h) - 1u;
    const FeistelKey fk = feistel_key(seed);
    uint32_t x = (uint32_t)j;
    do {
      x = feistel(x, h, m, fk);
    } while (x >= n);
    src = x;
  } else {
    uint32_t hsh = mix32((uint32_t)seed ^ 0x85EBCA6Bu);
    hsh = mix32(hsh ^ (uint32_t)(seed >> 32));
    hsh = mix32(hsh ^ (uint32_t)j);
    src = __umulhi(hsh, n);
  }
  const float* r = raw + (p0 + src) * (long long)load_dim;
  float x = r[0], y = r[1];
  const float zr = r[2];
  const float* q = prm + (size_t)b * 8;
  if (q[0] != 0.f) x = -x;
  // as numpy does it: the rotation (a float64 matrix) and the translation (a float64 vector) in float64, each
  // result rounded to float32; the scale in float32
  const double c = q[1], s = q[2];
  const float sc = q[3];
  const float xr = (float)((double)x * c - (double)y * s), yr = (float)((double)x * s + (double)y * c);
  out[o] = make_float4((float)((double)(xr * sc) + (double)q[4]), (float)((double)(yr * sc) + (double)q[5]),
                       (float)((double)(zr * sc) + (double)q[6]), (zr - floor_in[b]) * sc);
  if (src_idx) src_idx[o] = (int)src;
}

struct NormParams {
  float mean[3], inv_std[3];
};

// Source tap and weight of output coordinate d (cv2 INTER_LINEAR): s = (d + 0.5) * in / out - 0.5 taken exactly as
// the fraction ((2d + 1) in - out) / (2 out); below 0 -> tap 0, weight 0; at or beyond in - 1 -> last tap, weight 0.
__device__ __forceinline__ void src_tap(int d, int in, int outn, int& i0, int& i1, float& f) {
  const long long num = (long long)(2 * d + 1) * in - outn, den = 2LL * outn;
  if (num < 0) {
    i0 = i1 = 0;
    f = 0.f;
    return;
  }
  const long long s = num / den;
  if (s >= in - 1) {
    i0 = i1 = in - 1;
    f = 0.f;
    return;
  }
  i0 = (int)s;
  i1 = i0 + 1;
  f = (float)(num - s * den) / (float)den;
}

// Grid (ceil(Hp * Wp / 4 / 256), B): one thread = 4 consecutive output pixels of a row, one 16-byte store per plane.
// shp (B, 4) int32 = (h_in, w_in, h_out, w_out); src: the scenes' HWC RGB bytes at byte offsets off[b].
__global__ __launch_bounds__(kImgThreads) void image_prep_k(int Hp, int Wp, long long src_bytes,
                                                            const unsigned char* __restrict__ src,
                                                            const int64_t* __restrict__ off,
                                                            const int* __restrict__ shp, NormParams np_,
                                                            float* __restrict__ out) {
  const int b = blockIdx.y;
  const int wq = Wp >> 2;
  const long long q = (long long)blockIdx.x * kImgThreads + threadIdx.x;
  if (q >= (long long)Hp * wq) return;
  const int y = (int)(q / wq), x0 = (int)(q - (long long)y * wq) * 4;
  const int hin = shp[b * 4], win = shp[b * 4 + 1];
  int hout = shp[b * 4 + 2], wout = shp[b * 4 + 3];
  const long long base = off[b];
  // an inconsistent table entry makes the scene all padding instead of a read out of bounds
  if (hin <= 0 || win <= 0 || hout <= 0 || wout <= 0 || base < 0 ||
      base + (long long)hin * win * 3 > src_bytes) hout = wout = 0;
  if (hout > Hp) hout = Hp;
  if (wout > Wp) wout = Wp;
  float v[3][4];
  if (y < hout) {
    int y0, y1;
    float fy;
    src_tap(y, hin, shp[b * 4 + 2], y0, y1, fy);
    const unsigned char* r0 = src + base + (long long)y0 * win * 3;
    const unsigned char* r1 = src + base + (long long)y1 * win * 3;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int x = x0 + e;
      if (x < wout) {
        int xa, xb;
        float fx;
        src_tap(x, win, shp[b * 4 + 3], xa, xb, fx);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float a0 = r0[xa * 3 + c], a1 = r0[xb * 3 + c], b0 = r1[xa * 3 + c], b1 = r1[xb * 3 + c];
          const float top = a0 + (a1 - a0) * fx, bot = b0 + (b1 - b0) * fx;
          const float val = fminf(fmaxf(__builtin_rintf(top + (bot - top) * fy), 0.f), 255.f);
          v[c][e] = (val - np_.mean[c]) * np_.inv_std[c];
        }
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c][e] = 0.f;
      }
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[c][e] = 0.f;
  }
  const size_t plane = (size_t)Hp * Wp;
  float* o = out + (size_t)b * 3 * plane + (size_t)y * Wp + x0;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    *reinterpret_cast<float4*>(o + c * plane) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
}

}  // namespace

}  // namespace demf

using namespace demf;

extern "C" int demf_points_floor(int B, int load_dim, long long total, const float* raw, const int64_t* offsets,
                                 float* floor_out, demf_stream_t stream) {
  DEMF_REQUIRE(B > 0 && load_dim >= 3 && total > 0 && total < (1LL << 31), "points_floor: bad sizes");
  DEMF_REQUIRE(raw && offsets && floor_out, "points_floor: null pointer");
  hipLaunchKernelGGL(points_floor_k, dim3(B), dim3(kFloorThreads), 0, (hipStream_t)stream, load_dim, total, raw,
                     offsets, floor_out);
  return check_launch("points_floor");
}

extern "C" int demf_points_prep(int B, int num_points, int load_dim, long long total, const float* raw,
                                const int64_t* offsets, const float* floor_in, const float* params,
                                const int64_t* seeds, float* out, int* src_index, demf_stream_t stream) {
  DEMF_REQUIRE(B > 0 && B <= 65535 && num_points > 0 && load_dim >= 3 && total > 0 && total < (1LL << 31),
               "points_prep: bad sizes");
  DEMF_REQUIRE(raw && offsets && floor_in && params && seeds && out, "points_prep: null pointer");
  hipLaunchKernelGGL(points_prep_k, dim3(cdiv(num_points, kPrepThreads), B), dim3(kPrepThreads), 0,
                     (hipStream_t)stream, num_points, load_dim, total, raw, offsets, floor_in, params, seeds,
                     reinterpret_cast<float4*>(out), src_index);
  return check_launch("points_prep");
}

extern "C" int demf_image_prep(int B, int Hp, int Wp, long long src_bytes, const unsigned char* src,
                               const int64_t* offsets, const int* shapes, const float* mean_std, float* out,
                               demf_stream_t stream) {
  DEMF_REQUIRE(B > 0 && B <= 65535 && Hp > 0 && Wp > 0 && Wp % 4 == 0 && src_bytes > 0 &&
               (long long)Hp * Wp < (1LL << 31), "image_prep: bad sizes");
  DEMF_REQUIRE(src && offsets && shapes && mean_std && out, "image_prep: null pointer");
  NormParams np_;
  for (int c = 0; c < 3; ++c) {
    DEMF_REQUIRE(mean_std[3 + c] > 0.f, "image_prep: std must be positive");
    np_.mean[c] = mean_std[c];
    np_.inv_std[c] = (float)(1.0 / (double)mean_std[3 + c]);
  }
  const long long quads = (long long)Hp * (Wp / 4);
  hipLaunchKernelGGL(image_prep_k, dim3((unsigned)((quads + kImgThreads - 1) / kImgThreads), B), dim3(kImgThreads),
                     0, (hipStream_t)stream, Hp, Wp, src_bytes, src, offsets, shapes, np_, out);
  return check_launch("image_prep");
}
