// Device helpers that more than one shared-MLP unit inlines (all __forceinline__, no kernel here):
//   - the A-operand prologue (raw fetch + BN/ReLU or BN-backward transform): mlp_gemm_kernel, mlp_dw_body;
//   - the fused max-pool epilogue on the MFMA accumulator layout: mlp_gemm_kernel, mlp_fwd_res_kernel,
//     mlp_fwd_pc_kernel;
//   - the split-plane fragments (swizzle, pair split, MFMA chain) of the two persistent forward kernels.
#pragma once
#include "mlp_args.h"

namespace demf {

// Raw operands of one float4 of A: fetched early (kept in flight across the MFMA phase of the
// previous step) and only transformed when they are written to LDS.
template <int PRO>
struct MlpRaw {
  float4 x;                                                    // X / Y_l
  float4 g;                                                    // DY_DENSE: G ; DY_SPARSE: dP
  int4 a;                                                      // DY_SPARSE: arg
  int s;                                                       // DY_SPARSE: row's slot in its group
};
template <> struct MlpRaw<PRO_NONE> { float4 x; };
template <> struct MlpRaw<PRO_BNRELU> { float4 x; };
template <> struct MlpRaw<PRO_DY_DENSE> { float4 x, g; };

template <int PRO>
__device__ __forceinline__ void mlp_fetch(const MlpArgs& p, int row, int col, bool ok, MlpRaw<PRO>& r) {
  r.x = make_float4(0.f, 0.f, 0.f, 0.f);
  if constexpr (PRO == PRO_DY_DENSE) r.g = make_float4(0.f, 0.f, 0.f, 0.f);
  if constexpr (PRO == PRO_DY_SPARSE) {
    r.g = make_float4(0.f, 0.f, 0.f, 0.f);
    r.a = make_int4(-1, -1, -1, -1);
    r.s = 0;
  }
  if (!ok) return;
  r.x = *reinterpret_cast<const float4*>(p.X + (size_t)row * p.ldx + col);
  if constexpr (PRO == PRO_DY_DENSE) r.g = *reinterpret_cast<const float4*>(p.G + (size_t)row * p.K + col);
  if constexpr (PRO == PRO_DY_SPARSE) {
    const int rp = row / p.ns;
    r.s = row - rp * p.ns;
    r.g = *reinterpret_cast<const float4*>(p.dP + (size_t)rp * p.K + col);
    r.a = *reinterpret_cast<const int4*>(p.arg + (size_t)rp * p.K + col);
  }
}

// `vec` = the per-channel vectors (global, or the block's LDS copy); `ok` false -> zeros
template <int PRO>
__device__ __forceinline__ float4 mlp_xform(const MlpArgs& p, const float* __restrict__ vec, int col,
                                            bool ok, const MlpRaw<PRO>& r) {
  const float4 x = r.x;
  if constexpr (PRO == PRO_NONE) {
    return x;
  } else if constexpr (PRO == PRO_BNRELU) {
    if (!ok) return make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 s = *reinterpret_cast<const float4*>(vec + col);
    const float4 t = *reinterpret_cast<const float4*>(vec + p.K + col);
    float4 o;
    o.x = fmaxf(0.f, __builtin_fmaf(x.x, s.x, t.x));
    o.y = fmaxf(0.f, __builtin_fmaf(x.y, s.y, t.y));
    o.z = fmaxf(0.f, __builtin_fmaf(x.z, s.z, t.z));
    o.w = fmaxf(0.f, __builtin_fmaf(x.w, s.w, t.w));
    return o;
  } else {
    if (!ok) return make_float4(0.f, 0.f, 0.f, 0.f);
    float4 g = r.g;
    if constexpr (PRO == PRO_DY_SPARSE) {
      g.x = r.a.x == r.s ? g.x : 0.f;
      g.y = r.a.y == r.s ? g.y : 0.f;
      g.z = r.a.z == r.s ? g.z : 0.f;
      g.w = r.a.w == r.s ? g.w : 0.f;
    }
    // dY = gi*(dZ - c1 - xhat*c2) = gi*dZ + (a*y + b), dZ = g where y*scale+shift > 0
    const int K = p.K;
    const float4 sc = *reinterpret_cast<const float4*>(vec + col);
    const float4 sh = *reinterpret_cast<const float4*>(vec + K + col);
    const float4 gi = *reinterpret_cast<const float4*>(vec + 2 * K + col);
    const float4 va = *reinterpret_cast<const float4*>(vec + 3 * K + col);
    const float4 vb = *reinterpret_cast<const float4*>(vec + 4 * K + col);
    float4 o;
#define MLP_DY(m)                                                                   \
    {                                                                               \
      const float dz = __builtin_fmaf(x.m, sc.m, sh.m) > 0.f ? g.m : 0.f;           \
      o.m = __builtin_fmaf(gi.m, dz, __builtin_fmaf(va.m, x.m, vb.m));              \
    }
    MLP_DY(x) MLP_DY(y) MLP_DY(z) MLP_DY(w)
#undef MLP_DY
    return o;
  }
}

template <int PRO>
__device__ __forceinline__ float4 mlp_load_a(const MlpArgs& p, const float* __restrict__ vec,
                                             int row, int col) {
  MlpRaw<PRO> r;
  mlp_fetch<PRO>(p, row, col, true, r);
  return mlp_xform<PRO>(p, vec, col, true, r);
}

// Fused max-pool epilogue.  max_s relu(sc*y_s + sh) = relu(sc*y* + sh) with y* = max_s y_s when
// sc >= 0 and min_s y_s otherwise (sc*y + sh is monotone in y and so is its rounding), so the GEMM can
// reduce the RAW output over each group of NS rows before the batch statistics exist; the
// consumer picks max or min once the scale is known (pool_select_k).  C/D layout: a lane owns one
// column and the rows (r&3) + 8*(r>>2) + 4*(lane>>5) of each 32-row tile; the partner lane^32 owns
// the other 16 rows.  Ties resolve to the smallest row offset (first maximum, as max_pool2d).
template <int RT, int NT, int NS>
__device__ __forceinline__ void pool_epilogue(const MlpArgs& p, const f32x16 (&acc)[RT][NT], int nt,
                                              int row0, int col, int lh) {
  constexpr int GROUPS = (32 * RT) / NS;           // groups inside this wave's rows
#pragma unroll
  for (int g = 0; g < GROUPS; ++g) {
    float mx = -__builtin_inff(), mn = __builtin_inff();
    int ax = 0, an = 0;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rho_w = rt * 32 + (r & 3) + 8 * (r >> 2);      // + 4*lh, added below
        if (rho_w / NS != g) continue;                            // compile-time after unrolling
        const int rho = rho_w % NS + 4 * lh;
        const float v = acc[rt][nt][r];
        // a lane visits its rows in ascending order, so "first extremum wins" is the strict compare
        // (branch-free: one v_cmp + two v_cndmask each)
        const bool up = v > mx, dn = v < mn;
        mx = up ? v : mx; ax = up ? rho : ax;
        mn = dn ? v : mn; an = dn ? rho : an;
      }
    const float omx = __shfl_xor(mx, 32), omn = __shfl_xor(mn, 32);
    const int oax = __shfl_xor(ax, 32), oan = __shfl_xor(an, 32);
    if (omx > mx || (omx == mx && oax < ax)) { mx = omx; ax = oax; }
    if (omn < mn || (omn == mn && oan < an)) { mn = omn; an = oan; }
    const int row = row0 + g * NS;
    if (lh == 0 && row < p.R && col < p.N) {
      const size_t o = (size_t)(row / NS) * p.N + col;
      p.pmax[o] = mx; p.pmin[o] = mn; p.amax[o] = ax; p.amin[o] = an;
    }
  }
}

// NS = 64 with 32-row wave tiles: a group spans the row tiles of two neighbouring waves (2w, 2w+1).
// Each wave reduces its 32 rows, both publish through LDS, the even wave merges (its offsets are the
// smaller ones, so it wins ties) and writes.  s_pool: [wave][nt][lane&31] x {max, min, amax, amin}.
template <int NT>
__device__ __forceinline__ void pool_half_reduce(const f32x16 (&acc)[1][NT], int nt, int wave, int lr,
                                                 int lh, float4* __restrict__ s_pool) {
  float mx = -__builtin_inff(), mn = __builtin_inff();
  int ax = 0, an = 0;
  const int base = (wave & 1) * 32 + 4 * lh;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int rho = base + (r & 3) + 8 * (r >> 2);
    const float v = acc[0][nt][r];
    const bool up = v > mx, dn = v < mn;          // rows ascend: the strict compare keeps the first
    mx = up ? v : mx; ax = up ? rho : ax;
    mn = dn ? v : mn; an = dn ? rho : an;
  }
  const float omx = __shfl_xor(mx, 32), omn = __shfl_xor(mn, 32);
  const int oax = __shfl_xor(ax, 32), oan = __shfl_xor(an, 32);
  if (omx > mx || (omx == mx && oax < ax)) { mx = omx; ax = oax; }
  if (omn < mn || (omn == mn && oan < an)) { mn = omn; an = oan; }
  if (lh == 0)
    s_pool[(wave * NT + nt) * 32 + lr] =
        make_float4(mx, mn, __builtin_bit_cast(float, ax), __builtin_bit_cast(float, an));
}

// SEL: the sign of the BN scale is the sign of gamma, which IS known before the statistics: only the
// extremum the consumer will pick is tracked - the maximum of v for gamma >= 0, of -v otherwise
// (``flip`` = the lane's sign-bit mask) - at half the compare / select work and half the pooled stores.
__device__ __forceinline__ float flip_sign(float v, unsigned flip) {
  return __builtin_bit_cast(float, __builtin_bit_cast(unsigned, v) ^ flip);
}

// (`used`: this helper is inlined into kernels of three units.  Left internal, the compiler specialises its body on
// the argument ranges of the call sites ONE unit happens to contain before it inlines it - sext -> zext of the row index,
// then a longer 64-bit multiply in the pooled stores - so the same kernel came out 52-72 bytes longer next to fewer
// callers.  A symbol that must be kept is compiled from its own text alone: every unit gets the same code, at the
// price of a ~1 KB uncalled copy per instantiation in the code object.)
template <int RT, int NT, int NS>
__device__ __forceinline__ __attribute__((used)) void pool_epilogue_sel(const MlpArgs& p, const f32x16 (&acc)[RT][NT], int nt,
                                                  int row0, int col, int lh, unsigned flip) {
  constexpr int GROUPS = (32 * RT) / NS;
#pragma unroll
  for (int g = 0; g < GROUPS; ++g) {
    float mx = -__builtin_inff();
    int ax = 0;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rho_w = rt * 32 + (r & 3) + 8 * (r >> 2);
        if (rho_w / NS != g) continue;
        const int rho = rho_w % NS + 4 * lh;
        const float v = flip_sign(acc[rt][nt][r], flip);
        const bool up = v > mx;
        mx = up ? v : mx; ax = up ? rho : ax;
      }
    const float omx = __shfl_xor(mx, 32);
    const int oax = __shfl_xor(ax, 32);
    if (omx > mx || (omx == mx && oax < ax)) { mx = omx; ax = oax; }
    const int row = row0 + g * NS;
    if (lh == 0 && row < p.R && col < p.N) {
      const size_t o = (size_t)(row / NS) * p.N + col;
      p.pmax[o] = flip_sign(mx, flip); p.amax[o] = ax;
    }
  }
}

template <int NT>
__device__ __forceinline__ void pool_half_reduce_sel(const f32x16 (&acc)[1][NT], int nt, int wave, int lr,
                                                     int lh, float4* __restrict__ s_pool, unsigned flip) {
  float mx = -__builtin_inff();
  int ax = 0;
  const int base = (wave & 1) * 32 + 4 * lh;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int rho = base + (r & 3) + 8 * (r >> 2);
    const float v = flip_sign(acc[0][nt][r], flip);
    const bool up = v > mx;
    mx = up ? v : mx; ax = up ? rho : ax;
  }
  const float omx = __shfl_xor(mx, 32);
  const int oax = __shfl_xor(ax, 32);
  if (omx > mx || (omx == mx && oax < ax)) { mx = omx; ax = oax; }
  if (lh == 0) {
    float2* sp = reinterpret_cast<float2*>(s_pool);
    sp[(wave * NT + nt) * 32 + lr] = make_float2(mx, __builtin_bit_cast(float, ax));
  }
}

// ---- bf16 / fp16 planes of mlp_fwd_res_kernel and mlp_fwd_pc_kernel ---------------------------------------------------
// LDS rows are K bf16 = 128 B (K = 64); 16-byte chunk c of row r lives at chunk c ^ ((r >> 1) & 7): a
// ds_read_b128 lane group {0-3, 12-15, 20-27} / {4-11, 16-19, 28-31} then touches every bank once.
template <int KB>   // KB = bytes per row (K * 2)
__device__ __forceinline__ int fr_swz(int row, int chunk) {
  if constexpr (KB == 128) return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4);
  else return row * KB + ((chunk ^ (row & 15)) << 4);
}
using f32x2_t = float __attribute__((ext_vector_type(2)));
using bf16x2_t = __bf16 __attribute__((ext_vector_type(2)));
template <int P>
__device__ __forceinline__ void fr_split_pair(float a, float b, unsigned (&o)[P]) {
  if constexpr (P == 2) {       // two fp16 terms (csrc/common.h)
    split2_f16(a, b, o[0], o[1]);
    return;
  }
  const f32x2_t x = {a, b};
  const bf16x2_t h = __builtin_convertvector(x, bf16x2_t);
  o[0] = __builtin_bit_cast(unsigned, h);
  if constexpr (P == 3) {
    const f32x2_t r = x - __builtin_convertvector(h, f32x2_t);
    const bf16x2_t m = __builtin_convertvector(r, bf16x2_t);
    o[1] = __builtin_bit_cast(unsigned, m);
    const f32x2_t l = r - __builtin_convertvector(m, f32x2_t);
    o[2] = __builtin_bit_cast(unsigned, __builtin_convertvector(l, bf16x2_t));
  }
}
template <int P>
__device__ __forceinline__ void fr_mfma(f32x16& acc, const bf16x8 (&a)[P], const bf16x8 (&b)[P]) {
  if constexpr (P == 2) {   // fp16 terms: l.h', h.l', h.h'
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_v, a[1]), __builtin_bit_cast(f16x8_v, b[0]), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_v, a[0]), __builtin_bit_cast(f16x8_v, b[1]), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_v, a[0]), __builtin_bit_cast(f16x8_v, b[0]), acc, 0, 0, 0);
  } else if constexpr (P == 3) {   // six products of weight >= 2^-16, smallest first (as the CM = 2 path above)
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], acc, 0, 0, 0);
  } else {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], acc, 0, 0, 0);
  }
}

}  // namespace demf
