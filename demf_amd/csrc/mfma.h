// MFMA operand types and the bf16 splits shared by the matrix kernels (mlp*.hip, mlp_bwd.hip, dense.hip,
// rows_gemm.hip, conv.hip): the vector aliases of the v_mfma_f32_32x32x* builtins, fp32 -> bf16 terms, and the
// chunk swizzle of the 64-byte-row LDS planes.
#pragma once
#include "common.h"

namespace demf {

using f32x16 = float __attribute__((ext_vector_type(16)));
using bf16x8 = __bf16 __attribute__((ext_vector_type(8)));
using bf16x4 = __bf16 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bf16x4 to_bf16x4(const float4& v) {
  bf16x4 r;
  r[0] = (__bf16)v.x; r[1] = (__bf16)v.y; r[2] = (__bf16)v.z; r[3] = (__bf16)v.w;
  return r;
}

// x = h + m + l with h = bf16(x), m = bf16(x - h), l = bf16(x - h - m); both differences are exact in
// fp32 and the last one fits bf16's 8 bits, so the three terms carry all 24 significand bits.
__device__ __forceinline__ float4 bf16x4_to_f32(const bf16x4& h) {
  return make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
}
__device__ __forceinline__ void split3(const float4& v, bf16x4& h, bf16x4& m, bf16x4& l) {
  h = to_bf16x4(v);
  const float4 hf = bf16x4_to_f32(h);
  const float4 r = make_float4(v.x - hf.x, v.y - hf.y, v.z - hf.z, v.w - hf.w);
  m = to_bf16x4(r);
  const float4 mf = bf16x4_to_f32(m);
  l = to_bf16x4(make_float4(r.x - mf.x, r.y - mf.y, r.z - mf.z, r.w - mf.w));
}
__device__ __forceinline__ void split3(const float4& v0, const float4& v1, bf16x8& h, bf16x8& m, bf16x8& l) {
  bf16x4 h0, m0, l0, h1, m1, l1;
  split3(v0, h0, m0, l0);
  split3(v1, h1, m1, l1);
  h = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
  m = __builtin_shufflevector(m0, m1, 0, 1, 2, 3, 4, 5, 6, 7);
  l = __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7);
}

// byte offset of 16-byte chunk `chunk` (0..3) of 64-byte row `row`.  Chunks are XOR-swizzled by bits 2-3
// of the row: a ds_read_b128 is served in lane groups {0-3, 12-15, 20-27} / {4-11, 16-19, 28-31} (+32),
// and within each group the four rows that share row & 3 (= the same 16-dword bank window) differ in
// (row >> 2) & 3, so a fragment read (lane = row, same chunk index) touches all 64 banks exactly once.
// (Measured with the earlier (row >> 1) & 3: SQ_LDS_BANK_CONFLICT = half of all LDS cycles.)
__device__ __forceinline__ int swz(int row, int chunk) { return row * 64 + ((chunk ^ ((row >> 2) & 3)) << 4); }

}  // namespace demf
