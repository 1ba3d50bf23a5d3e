// Batch assembly out of the frozen image-feature cache (demf_amd/featcache.py).
//
// The cache keeps every scene's encoder tokens - evaluated alone, on the scene's own padded shape - as consecutive
// rows of one device-resident arena (rows, C), fp32 or bf16.  A training batch needs them placed on the batch's
// canvas: level l of the batch is (H_l, W_l), a scene's own level (h_l <= H_l, w_l <= W_l) sits in its top-left
// corner, everything outside it (and every masked token) is a zero row.  demf_tokens_assemble writes ALL B * S rows
// of the (B,S,C) token tensor in one launch - a row-granular streaming copy, no LDS, no atomics.  A lane moves 4
// elements (8 when both sides are bf16 and C % 8 == 0), so the wider side of the copy is one 16-byte access per lane,
// consecutive lanes on consecutive 16 bytes: a 256-channel fp32 row is one access of a whole wave.
//
// One workgroup serves ONE scene of the batch (blockIdx.y), so the scene's table row - row0 and the own (h, w) of
// every level - is wave-uniform: it is read once per workgroup and lives in scalar registers; the per-row work is the
// level select, one 32-bit division and the copy.  A lane has ROWS rows in flight (their mask bytes, then their
// loads, then their stores): one row at a time the kernel waits for memory latency, not bandwidth.  Arena offsets are
// 64-bit (the real training set is ~9e7 rows x 256 channels, far past 2^31 elements).
#include "common.h"

namespace demf {

struct AsmLevels {
  int H[8], W[8], start[9];      // the batch canvas; start[n] = S
  int n;
};

// fp32 -> bf16, round to nearest even, NaN -> 0x7FC0: the integer form c10::BFloat16 uses, so the words are those of
// tensor.to(torch.bfloat16) whatever the denormal mode of the conversion instruction
__device__ __forceinline__ unsigned bf16_rne(unsigned u) {
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// E elements of the arena as 32-bit words: E fp32 bit patterns, or E / 2 pairs of bf16 words.  All-zero words are
// zeros in both formats.
template <int E, bool AB> struct Words { unsigned w[AB ? E / 2 : E]; };

template <int E, bool AB>
__device__ __forceinline__ Words<E, AB> load_words(const void* __restrict__ arena, long long elem, bool live) {
  constexpr int N = AB ? E / 2 : E;
  Words<E, AB> r;
#pragma unroll
  for (int i = 0; i < N; ++i) r.w[i] = 0u;
  if (live) {
    const unsigned* p = reinterpret_cast<const unsigned*>(
        reinterpret_cast<const char*>(arena) + elem * (AB ? 2 : 4));
    if constexpr (N == 4) {
      const uint4 q = *reinterpret_cast<const uint4*>(p);
      r.w[0] = q.x; r.w[1] = q.y; r.w[2] = q.z; r.w[3] = q.w;
    } else {
      static_assert(N == 2, "4 or 8 elements per lane");
      const uint2 q = *reinterpret_cast<const uint2*>(p);
      r.w[0] = q.x; r.w[1] = q.y;
    }
  }
  return r;
}

template <int E, bool AB, bool OB>
__device__ __forceinline__ void store_words(void* __restrict__ out, long long elem, const Words<E, AB>& r) {
  unsigned* o = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(out) + elem * (OB ? 2 : 4));
  if constexpr (AB == OB) {                      // a copy: the words as they are
    if constexpr ((AB ? E / 2 : E) == 4) *reinterpret_cast<uint4*>(o) = make_uint4(r.w[0], r.w[1], r.w[2], r.w[3]);
    else *reinterpret_cast<uint2*>(o) = make_uint2(r.w[0], r.w[1]);
  } else if constexpr (OB) {                     // fp32 -> bf16 (E = 4)
    static_assert(E == 4, "the converting forms move 4 elements per lane");
    *reinterpret_cast<uint2*>(o) = make_uint2(bf16_rne(r.w[0]) | (bf16_rne(r.w[1]) << 16),
                                              bf16_rne(r.w[2]) | (bf16_rne(r.w[3]) << 16));
  } else {                                       // bf16 -> fp32 (E = 4): exact
    static_assert(E == 4, "the converting forms move 4 elements per lane");
    *reinterpret_cast<uint4*>(o) = make_uint4(r.w[0] << 16, r.w[0] & 0xffff0000u, r.w[1] << 16, r.w[1] & 0xffff0000u);
  }
}

constexpr int ROWS = 4;      // rows a lane has in flight

// E elements per lane, AB / OB: bf16 arena / bf16 output.  grid (gx, B): a workgroup strides over the S rows of its
// scene, ROWS x (256 >> lpr_shift) rows at a time, 1 << lpr_shift lanes per row (>= C / E, or 256 with a lane loop).
template <int E, bool AB, bool OB>
__global__ __launch_bounds__(256) void tokens_assemble_k(int C, int S, int lpr_shift, AsmLevels lv, long long N,
                                                         long long arena_rows, const void* __restrict__ arena,
                                                         const long long* __restrict__ table,
                                                         const long long* __restrict__ indices,
                                                         const unsigned char* __restrict__ mask,
                                                         void* __restrict__ out) {
  const int b = blockIdx.y, t = threadIdx.x;
  const int cpr = C / E, lpr = 1 << lpr_shift, rpb = 256 >> lpr_shift;
  // the scene: wave-uniform, read once (scalar loads); the host has validated all of it, the guards below only keep
  // a table or index that changed underneath the call from reaching outside the arena (such a scene reads as zeros)
  const long long idx = indices[b];
  const bool known = idx >= 0 && idx < N;
  const long long* row = table + (known ? idx : 0) * (1 + 2 * lv.n);
  const long long row0 = row[0];
  int h[8], w[8], own[8];
  long long total = 0;
  bool fits = known && row0 >= 0;
#pragma unroll
  for (int l = 0; l < 8; ++l) {
    h[l] = w[l] = own[l] = 0;
    if (l < lv.n) {
      const long long hl = row[1 + 2 * l], wl = row[2 + 2 * l];
      fits = fits && hl >= 0 && wl >= 0 && hl <= lv.H[l] && wl <= lv.W[l];
      h[l] = (int)hl; w[l] = (int)wl; own[l] = (int)total;
      total += fits ? hl * wl : 0;
    }
  }
  fits = fits && row0 + total <= arena_rows;
  const unsigned char* m = mask != nullptr ? mask + (size_t)b * S : nullptr;
  const long long obase = (long long)b * S;
  const int stride = gridDim.x * rpb;
  for (int s0 = blockIdx.x * rpb + (t >> lpr_shift); s0 < S; s0 += ROWS * stride) {
    long long src[ROWS];
    bool live[ROWS];
#pragma unroll
    for (int u = 0; u < ROWS; ++u) {
      const int s = s0 + u * stride;
      const bool valid = s < S;
      int Wl = lv.W[0], st = 0, hl = h[0], wl = w[0], ow = own[0];
#pragma unroll
      for (int l = 1; l < 8; ++l)
        if (l < lv.n && s >= lv.start[l]) { Wl = lv.W[l]; st = lv.start[l]; hl = h[l]; wl = w[l]; ow = own[l]; }
      const unsigned ls = (unsigned)(s - st);
      const unsigned y = ls / (unsigned)Wl, x = ls - y * (unsigned)Wl;
      const bool masked = valid && m != nullptr && m[s];
      live[u] = valid && fits && (int)y < hl && (int)x < wl && !masked;
      src[u] = (row0 + ow + (long long)y * wl + x) * C;
    }
    for (int c = t & (lpr - 1); c < cpr; c += lpr) {
      Words<E, AB> r[ROWS];
#pragma unroll
      for (int u = 0; u < ROWS; ++u) r[u] = load_words<E, AB>(arena, src[u] + (long long)c * E, live[u]);
#pragma unroll
      for (int u = 0; u < ROWS; ++u) {
        const int s = s0 + u * stride;
        if (s < S) store_words<E, AB, OB>(out, (obase + s) * C + (long long)c * E, r[u]);
      }
    }
  }
}

}  // namespace demf


using namespace demf;

extern "C" int demf_tokens_assemble(int B, int C, int S, int L, long long N, long long arena_rows, const void* arena,
                                    int arena_bf16, const long long* table, const long long* table_host,
                                    const long long* indices, const long long* indices_host, const int* hw,
                                    const unsigned char* mask, void* out, int out_bf16, demf_stream_t stream) {
  DEMF_REQUIRE(B >= 0 && C >= 1 && S >= 1 && L >= 1 && N >= 0 && arena_rows >= 0, "tokens_assemble: bad sizes");
  DEMF_REQUIRE(L <= 8, "tokens_assemble: %d levels, at most 8", L);
  DEMF_REQUIRE(C % 4 == 0, "tokens_assemble: C = %d is not a multiple of 4", C);
  DEMF_REQUIRE(table_host && indices_host && hw, "tokens_assemble: null pointer (host table, host indices, level shapes)");
  AsmLevels lv{};
  long long rows = 0;
  for (int l = 0; l < L; ++l) {
    DEMF_REQUIRE(hw[2 * l] >= 1 && hw[2 * l + 1] >= 1, "tokens_assemble: level %d is %d x %d", l, hw[2 * l], hw[2 * l + 1]);
    lv.H[l] = hw[2 * l]; lv.W[l] = hw[2 * l + 1]; lv.start[l] = (int)rows;
    rows += (long long)hw[2 * l] * hw[2 * l + 1];
    DEMF_REQUIRE(rows <= S, "tokens_assemble: the levels hold more than S = %d tokens", S);
  }
  DEMF_REQUIRE(rows == S, "tokens_assemble: the levels hold %lld tokens, S = %d", rows, S);
  lv.start[L] = S;
  lv.n = L;
  DEMF_REQUIRE((long long)B * S < (1ll << 30), "tokens_assemble: B * S = %lld rows, at most 2^30 - 1", (long long)B * S);
  // every scene of the batch against the HOST copy of the table, before anything is launched
  for (int b = 0; b < B; ++b) {
    const long long idx = indices_host[b];
    DEMF_REQUIRE(idx >= 0 && idx < N, "tokens_assemble: index %lld (batch position %d) is outside the table of %lld scenes",
                 idx, b, N);
    const long long* row = table_host + idx * (1 + 2 * L);
    long long own = 0;
    for (int l = 0; l < L; ++l) {
      const long long h = row[1 + 2 * l], w = row[2 + 2 * l];
      DEMF_REQUIRE(h >= 0 && w >= 0 && h <= lv.H[l] && w <= lv.W[l],
                   "tokens_assemble: scene %lld level %d is %lld x %lld, larger than the batch's %d x %d", idx, l, h, w,
                   lv.H[l], lv.W[l]);
      own += h * w;
    }
    DEMF_REQUIRE(row[0] >= 0 && row[0] + own <= arena_rows,
                 "tokens_assemble: scene %lld holds rows [%lld, %lld) of an arena of %lld", idx, row[0], row[0] + own,
                 arena_rows);
  }
  if (B == 0) return DEMF_OK;
  DEMF_REQUIRE(arena && table && indices && out, "tokens_assemble: null pointer");
  DEMF_REQUIRE((uintptr_t)arena % 16 == 0 && (uintptr_t)out % 16 == 0,
               "tokens_assemble: arena and output must be 16-byte aligned");
  const int E = (arena_bf16 && out_bf16 && C % 8 == 0) ? 8 : 4;
  const int cpr = C / E;
  int shift = 0;
  while ((1 << shift) < cpr && shift < 8) ++shift;
  const int rpb = 256 >> shift;
  // workgroups per scene: every row group once, ROWS rows per lane; at most ~16 workgroups per CU over the batch
  const int want = (S + ROWS * rpb - 1) / (ROWS * rpb), cap = 4096 / B > 0 ? 4096 / B : 1;
  const dim3 grid(want < cap ? want : cap, B);
#define DEMF_ASM_LAUNCH(E_, AB_, OB_)                                                                              \
  hipLaunchKernelGGL((tokens_assemble_k<E_, AB_, OB_>), grid, dim3(256), 0, (hipStream_t)stream, C, S, shift, lv, N, \
                     arena_rows, arena, table, indices, mask, out)
  if (E == 8) DEMF_ASM_LAUNCH(8, true, true);
  else if (arena_bf16 && out_bf16) DEMF_ASM_LAUNCH(4, true, true);
  else if (arena_bf16) DEMF_ASM_LAUNCH(4, true, false);
  else if (out_bf16) DEMF_ASM_LAUNCH(4, false, true);
  else DEMF_ASM_LAUNCH(4, false, false);
#undef DEMF_ASM_LAUNCH
  return check_launch("tokens_assemble");
}
