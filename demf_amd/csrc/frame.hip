// RGB-D frame front end: a 16-bit depth image, the registered colour image and a calibration -> the 6-float point
// records (x y z r g b, upright depth coordinates) that csrc/pipeline.hip takes, valid pixels only, in pixel order.
// This is the per-pixel part of the SUN RGB-D toolbox's offline export (read3dPoints: unproject, tilt) [dep-recall:
// restated from the toolbox's published behaviour; its sources are not in the reference tree]; rotation, depth scale,
// clamp and pixel origin are parameters.  All geometry is fp64, one IEEE operation at a time, no contraction, so a
// record is bit for bit what an element-wise numpy evaluation gives.
//
// The B frames' pixels are ONE concatenated run of `total` pixels, cut into tiles of kFrameTile whatever the frame
// boundaries are; the output order (frames in order, row-major inside a frame) is then the order of that run.
//   frame_count_k    per tile: ballot + popcount of the valid pixels -> tile_counts[tile]
//   frame_scatter_k  per tile: sums the counts of the earlier tiles itself, ranks its valid lanes (ballot, wave
//                    counts in LDS) and writes its records; B + 1 further workgroups write offsets[j] = the valid
//                    pixels in front of frame j (whole tiles from tile_counts, the cut tile re-counted)
// No atomics, no workgroup waits for another: two runs give the same bits.
#include <hip/hip_runtime.h>

#include "common.h"

namespace demf {

namespace {

constexpr int kFrameThreads = 256;
constexpr int kFrameWaves = kFrameThreads / 64;
constexpr int kFrameRounds = 4;
constexpr int kFrameTile = kFrameThreads * kFrameRounds;
static_assert(kFrameTile == DEMF_FRAME_TILE, "the tile of include/demf_hip.h, by which callers size tile_counts");

struct FrameArgs {
  int B, shift;
  long long total, rgb_bytes;
  const unsigned short* depth;
  const int64_t* depth_off;
  const unsigned char* rgb;
  const int64_t* rgb_off;
  const int* shapes;
  const double* calib;
};

struct Pixel {
  int b, w;              // frame, its width
  int l;                 // pixel index inside the frame (row-major)
  unsigned d;            // depth reading after the rotation
  long long rgb_at;      // byte offset of the pixel's r
};

// Pixel g of the concatenated run -> its frame and reading; false if the reading is 0 (no depth) or if the tables do
// not place g inside a frame whose depth and colour both lie within the buffers (then nothing is read out of bounds).
// The count and the scatter launch both decide validity here.
__device__ __forceinline__ bool frame_pixel(const FrameArgs& a, long long g, Pixel& p) {
  if (g < 0 || g >= a.total) return false;
  int lo = 0, hi = a.B;                                        // largest b in [0, B) with depth_off[b] <= g
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.depth_off[mid] <= g) lo = mid;
    else hi = mid;
  }
  const long long p0 = a.depth_off[lo], p1 = a.depth_off[lo + 1];
  if (p0 < 0 || g < p0 || g >= p1 || p1 > a.total) return false;
  const int h = a.shapes[lo * 4], w = a.shapes[lo * 4 + 1];
  if (h <= 0 || w <= 0) return false;
  const long long n = (long long)h * w, l = g - p0;
  const long long r0 = a.rgb_off[lo];
  if (l >= n || n >= (1LL << 31) || r0 < 0 || r0 + 3 * n > a.rgb_bytes) return false;
  const unsigned d = a.depth[g];
  p.d = a.shift ? ((d >> a.shift) | (d << (16 - a.shift))) & 0xFFFFu : d;
  p.b = lo;
  p.w = w;
  p.l = (int)l;
  p.rgb_at = r0 + 3 * l;
  return p.d != 0u;
}

// sum of counts[0 .. n) in every thread of the workgroup
__device__ __forceinline__ long long tiles_before(const int* __restrict__ counts, int n, long long* s_part) {
  long long s = 0;
  for (int i = threadIdx.x; i < n; i += kFrameThreads) s += counts[i];
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = s;
  __syncthreads();
  long long t = 0;
  for (int w = 0; w < kFrameWaves; ++w) t += s_part[w];
  return t;
}

// valid pixels among [g0, min(g0 + kFrameTile, g1)), in every thread of the workgroup
__device__ __forceinline__ int tile_valid(const FrameArgs& a, long long g0, long long g1, int* s_cnt) {
  int c = 0;
  Pixel p;
#pragma unroll
  for (int r = 0; r < kFrameRounds; ++r) {
    const long long g = g0 + r * kFrameThreads + threadIdx.x;
    c += __popcll(__ballot(g < g1 && frame_pixel(a, g, p)));
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = c;
  __syncthreads();
  int t = 0;
  for (int w = 0; w < kFrameWaves; ++w) t += s_cnt[w];
  return t;
}

__global__ __launch_bounds__(kFrameThreads) void frame_count_k(FrameArgs a, int* __restrict__ tile_counts) {
  __shared__ int s_cnt[kFrameWaves];
  const long long g0 = (long long)blockIdx.x * kFrameTile;
  const int n = tile_valid(a, g0, a.total, s_cnt);
  if (threadIdx.x == 0) tile_counts[blockIdx.x] = n;
}

// The record of one valid pixel.  calib row: [fx, fy, cx, cy, Rt row-major (9), pixel_origin, depth_scale, z_max].
__device__ __forceinline__ void frame_record(const FrameArgs& a, const Pixel& p, float* __restrict__ rec) {
#pragma clang fp contract(off)
  const double* q = a.calib + (size_t)p.b * 16;
  const int v = p.l / p.w, u = p.l - v * p.w;
  const double zs = (double)p.d / q[14];
  const double z = zs < q[15] ? zs : q[15];
  const double x3 = (((double)u + q[13]) - q[2]) * z / q[0];
  const double y3 = (((double)v + q[13]) - q[3]) * z / q[1];
  const double c0 = x3, c1 = z, c2 = -y3;                      // camera axes -> depth axes
  float2* o = reinterpret_cast<float2*>(rec);
  const float p0 = (float)((q[4] * c0 + q[5] * c1) + q[6] * c2);
  const float p1 = (float)((q[7] * c0 + q[8] * c1) + q[9] * c2);
  const float p2 = (float)((q[10] * c0 + q[11] * c1) + q[12] * c2);
  const unsigned char* px = a.rgb + p.rgb_at;
  const float r = (float)px[0] / 255.0f, g = (float)px[1] / 255.0f, b = (float)px[2] / 255.0f;
  o[0] = make_float2(p0, p1);
  o[1] = make_float2(p2, r);
  o[2] = make_float2(g, b);
}

// Grid ntiles + B + 1.
__global__ __launch_bounds__(kFrameThreads) void frame_scatter_k(FrameArgs a, int ntiles,
                                                                 const int* __restrict__ tile_counts,
                                                                 float* __restrict__ raw, int64_t* __restrict__ offsets) {
  __shared__ long long s_part[kFrameWaves];
  __shared__ int s_cnt[kFrameRounds * kFrameWaves];
  if ((int)blockIdx.x >= ntiles) {                             // offsets[j]: the valid pixels in front of frame j
    const int j = (int)blockIdx.x - ntiles;
    long long g = j == a.B ? a.total : a.depth_off[j];
    g = g < 0 ? 0 : (g > a.total ? a.total : g);
    const int full = (int)(g / kFrameTile);
    long long n = tiles_before(tile_counts, full, s_part);
    n += tile_valid(a, (long long)full * kFrameTile, g, s_cnt);
    if (threadIdx.x == 0) offsets[j] = n;
    return;
  }
  const long long base = tiles_before(tile_counts, (int)blockIdx.x, s_part);
  const long long g0 = (long long)blockIdx.x * kFrameTile;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  Pixel p[kFrameRounds];
  bool ok[kFrameRounds];
  int in_wave[kFrameRounds];
#pragma unroll
  for (int r = 0; r < kFrameRounds; ++r) {                     // pixel order in the tile: round, wave, lane
    ok[r] = frame_pixel(a, g0 + r * kFrameThreads + threadIdx.x, p[r]);
    const unsigned long long m = __ballot(ok[r]);
    in_wave[r] = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_cnt[r * kFrameWaves + wave] = __popcll(m);
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kFrameRounds; ++r) {
    int before = 0;
    for (int e = 0; e < r * kFrameWaves + wave; ++e) before += s_cnt[e];
    const long long row = base + before + in_wave[r];
    if (ok[r] && row < a.total) frame_record(a, p[r], raw + row * 6);
  }
}

}  // namespace

}  // namespace demf

using namespace demf;

extern "C" int demf_depth_to_points(int B, long long total, long long rgb_bytes, int shift,
                                    const unsigned short* depth, const int64_t* depth_off, const unsigned char* rgb,
                                    const int64_t* rgb_off, const int* shapes, const double* calib, int ntiles,
                                    int* tile_counts, float* raw, int64_t* offsets, demf_stream_t stream) {
  DEMF_REQUIRE(B > 0 && B <= 65535 && total > 0 && total < (1LL << 31) && rgb_bytes > 0 && shift >= 0 && shift <= 15,
               "depth_to_points: bad sizes");
  DEMF_REQUIRE(ntiles == (int)((total + kFrameTile - 1) / kFrameTile), "depth_to_points: bad sizes (tile count)");
  DEMF_REQUIRE(depth && depth_off && rgb && rgb_off && shapes && calib && tile_counts && raw && offsets,
               "depth_to_points: null pointer");
  DEMF_REQUIRE(((uintptr_t)raw & 7u) == 0, "depth_to_points: raw must be 8-byte aligned");
  const FrameArgs a = {B, shift, total, rgb_bytes, depth, depth_off, rgb, rgb_off, shapes, calib};
  hipLaunchKernelGGL(frame_count_k, dim3(ntiles), dim3(kFrameThreads), 0, (hipStream_t)stream, a, tile_counts);
  hipLaunchKernelGGL(frame_scatter_k, dim3(ntiles + B + 1), dim3(kFrameThreads), 0, (hipStream_t)stream, a, ntiles,
                     tile_counts, raw, offsets);
  return check_launch("depth_to_points");
}
