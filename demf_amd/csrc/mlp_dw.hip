// Shared-MLP weight gradients: dW_l = dY_l^T @ act(Y_{l-1}) with dY formed on the fly in the staging of the operand
// (the prologue of csrc/mlp_dev.h).  mlp_dw_body and its two kernels - one product per launch, or up to DW_GROUP_MAX
// products of one kernel variant in a grouped launch - the launch plan, and the entry points demf_mlp_gemm_bwd_dw,
// demf_mlp_gemm_bwd_dw_ld and demf_mlp_gemm_bwd_dw_group.
#include "mlp_dev.h"
#include <vector>

namespace demf {

// ---- dW(N x K) += dY(R x N)^T @ A(R x K): reduction over rows --------------------------------
// Block = 4 waves sharing a 32-row slab of dY and A in LDS per step; the NxK output is split into
// 32x32 MFMA tiles dealt round-robin to the waves (TPW tiles per wave).  Each block reduces its
// row range in registers and adds the partial with fp32 atomics.
struct DwArgs {
  int R, N, K, ldx;
  const float* Yl;     // (R x N) pre-BN output of this layer
  const float* G;      // dense upstream gradient or null
  const float* dP;     // sparse upstream gradient
  const int* arg;
  int ns;
  const float* vec;    // 5 x N backward vectors of this layer
  const float* Xp;     // (R x K) previous layer's pre-BN output, or the raw input
  const float* pvec;   // [scale|shift] of the previous layer (2K) or null (raw input)
  float* dW;           // (N x K), accumulated
  int lddw;            // row stride of dW (>= K)
  int n0, k0, NTn, NTk;  // output sub-block of a block (derived from blockIdx.y inside the kernel)
  int nsub_k;            // sub-blocks along K
  int chunk;             // 32-row slabs per claim
  int* sched;            // dynamic slab chunks: per-blockIdx.y {next chunk}, {finished}, + total; or null
  int dbg;               // DEMF_DW_DBG phase-skip bits (builds with -DDEMF_DW_PROFILE only): 1 MFMAs, 2 gather + split,
                         // 4 transform + stage, 8 flush, 16 loads
};
#ifdef DEMF_DW_PROFILE
#define DW_DBG(p, bit) ((p).dbg & (bit))
#else
#define DW_DBG(p, bit) false
#endif

#ifndef DEMF_DW_TR
#define DEMF_DW_TR 1      // transpose-read fragments from bf16 planes (0: the per-wave fp32 column gather - A/B builds)
#endif

// Waves form a 2 x 2 grid over the (<= 4 x 4) output tiles of the launch: wave (wn, wk) owns
// tiles tn = wn + 2i (i < TN), tk = wk + 2j (j < TK), so per row pair it reads TN + TK LDS
// values for TN*TK MFMAs.
// X3 (compute mode 2): the slab stays fp32 in LDS; per 16 rows a lane gathers its 8 rows of one column
// (8 ds_read_b32, conflict-free: consecutive lanes read consecutive columns), splits them into three
// bf16 terms and issues the six significant products on v_mfma_f32_32x32x16_bf16.
template <int TN, int TK, bool SPARSE, int X3 = 0>   // 0 fp32 MFMA, 1 three-term split, 2 one bf16 term
__device__ __forceinline__ void mlp_dw_body(DwArgs p, const int bx, const int by, const int gx) {
  constexpr int PROY = SPARSE ? PRO_DY_SPARSE : PRO_DY_DENSE;
  {  // this block's (<= 2TN x 2TK tiles) corner of the N x K output
    const int TNt = (p.N + 31) / 32, TKt = (p.K + 31) / 32;
    p.n0 = (by / p.nsub_k) * 2 * TN;
    p.k0 = (by % p.nsub_k) * 2 * TK;
    p.NTn = TNt - p.n0 < 2 * TN ? TNt - p.n0 : 2 * TN;
    p.NTk = TKt - p.k0 < 2 * TK ? TKt - p.k0 : 2 * TK;
  }
  extern __shared__ __attribute__((aligned(16))) float smem[];
  // staged widths are padded to the wave grid (2*TN, 2*TK tiles) so idle tiles read zeros
  constexpr int WN = 2 * TN * 32, WK = 2 * TK * 32;  // columns of dY / A staged per slab
  // TR (round 5, the bf16-MFMA modes): the slab is split ONCE by the staging threads and kept as row-major bf16
  // planes [PL][32][W + 8]; a wave's fragment - 8 consecutive ROWS of one column - is two ds_read_b64_tr_b16 per
  // plane (the 16 lanes of a group pass the addresses of a 4-row x 16-column block and receive one column each:
  // tools/ubench/tr16_probe.cpp).  Before, every wave gathered its columns from an fp32 slab with 8 ds_read_b32 and
  // split them itself - each element twice over (the two waves that share an operand), 250 of the loop's 650
  // instructions.  Same planes, same MFMA order: bit-identical results.
  constexpr bool TR = DEMF_DW_TR && X3 != 0;
  constexpr int PL = X3 == 1 ? 3 : 1;
  constexpr int ldn = TR ? WN + 8 : WN + 4, ldk = TR ? WK + 8 : WK + 4;     // row strides (bf16 / float elements)
  constexpr int PBN = 32 * ldn * 2, PBK = 32 * ldk * 2;                     // TR: bytes per plane
  float* s_dy = smem;                                // [32][WN + 4] fp32, or the dY planes
  float* s_a = TR ? reinterpret_cast<float*>(reinterpret_cast<char*>(smem) + PL * PBN) : s_dy + 32 * ldn;
  float* s_vy = TR ? reinterpret_cast<float*>(reinterpret_cast<char*>(s_a) + PL * PBK) : s_a + 32 * ldk;   // 5 x N vectors
  float* s_vx = s_vy + 5 * p.N;                      // [scale|shift] of the previous layer (2K)
  char* const p_dy = reinterpret_cast<char*>(s_dy);
  char* const p_a = reinterpret_cast<char*>(s_a);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 31, lh = lane >> 5;
  const int wn = wave >> 1, wk = wave & 1;
  for (int i = threadIdx.x; i < 5 * p.N; i += 256) s_vy[i] = p.vec[i];
  if (p.pvec)
    for (int i = threadIdx.x; i < 2 * p.K; i += 256) s_vx[i] = p.pvec[i];
  f32x16 acc[TN][TK];
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < TK; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  MlpArgs ay;  // reuse the GEMM prologue helpers
  ay.K = p.N; ay.ldx = p.N; ay.X = p.Yl; ay.G = p.G; ay.dP = p.dP; ay.arg = p.arg; ay.ns = p.ns;
  MlpArgs ax;
  ax.K = p.K; ax.ldx = p.ldx; ax.X = p.Xp;

  // per-thread slots of the 32-row slab: float4 index f = threadIdx.x + 256*j
  constexpr int qn = WN / 4, qk = WK / 4;
  MlpRaw<PROY> ry[4];
  MlpRaw<PRO_NONE> ra[4];
  // TR: a float4 (4 consecutive columns of a row) -> its PL planes, one ds_write_b64 each
  auto stage_planes = [&](char* dst, int plane_bytes, const float4& v) {
    if constexpr (X3 == 1) {
      bf16x4 h, m, l;
      split3(v, h, m, l);
      *reinterpret_cast<bf16x4*>(dst) = h;
      *reinterpret_cast<bf16x4*>(dst + plane_bytes) = m;
      *reinterpret_cast<bf16x4*>(dst + 2 * plane_bytes) = l;
    } else {
      *reinterpret_cast<bf16x4*>(dst) = to_bf16x4(v);
    }
  };
  // TR: rows 16c + 8lh .. + 7 of column col0 + lr of one plane (lane t of a 16-lane group addresses row t >> 2,
  // columns 4 (t & 3) .. + 3 of the group's 4 x 16 block)
  const int tr_off = ((lane & 15) >> 2) * 2, tr_col = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
  auto frag = [&](const char* plane, int ld, int col0, int c) {
    using v4s = short __attribute__((ext_vector_type(4)));
    using lds_v4s = v4s __attribute__((address_space(3)));
    const char* q = plane + ((16 * c + 8 * lh) * ld + col0 + tr_col) * 2 + tr_off * ld;
    const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(q));
    const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(q + 8 * ld));
    return __builtin_shufflevector(__builtin_bit_cast(bf16x4, lo), __builtin_bit_cast(bf16x4, hi), 0, 1, 2, 3, 4, 5, 6, 7);
  };
  bool oky[4], oka[4];
  auto prefetch = [&](int slab) {
    const int row0 = slab * 32;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int f = threadIdx.x + 256 * jj;
      const int r = f / qn, c = (f - r * qn) * 4;
      oky[jj] = f < 32 * qn && row0 + r < p.R && p.n0 * 32 + c < p.N && !DW_DBG(p, 16);
      mlp_fetch<PROY>(ay, row0 + r, p.n0 * 32 + c, oky[jj], ry[jj]);
      const int r2 = f / qk, c2 = (f - r2 * qk) * 4;
      oka[jj] = f < 32 * qk && row0 + r2 < p.R && p.k0 * 32 + c2 < p.K && !DW_DBG(p, 16);
      mlp_fetch<PRO_NONE>(ax, row0 + r2, p.k0 * 32 + c2, oka[jj], ra[jj]);
    }
  };
  // Rows are handed out in chunks of p.chunk 32-row slabs: the first chunk by block index, every
  // further one from a device counter per sub-block column (by), claimed a chunk ahead.
  const int nslab = (p.R + 31) / 32;
  const int nchunk = (nslab + p.chunk - 1) / p.chunk;
  __shared__ int s_next;
  const bool dyn = p.sched != nullptr;
  int claimed = 0;
  int chunk = bx, si = 0;
  if (chunk < nchunk) prefetch(chunk * p.chunk);
  while (chunk < nchunk) {
    const int slab = chunk * p.chunk + si;
    const bool last = si == p.chunk - 1 || slab + 1 >= nslab;
    if (dyn && threadIdx.x == 0) {
      if (si == 0) claimed = gx + atomicAdd(p.sched + by, 1);
      if (last) s_next = claimed;
    }
    __syncthreads();                                 // previous slab fully consumed (and s_v* ready)
    if (!DW_DBG(p, 4))
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int f = threadIdx.x + 256 * jj;
      if (f < 32 * qn) {
        const int r = f / qn, c = (f - r * qn) * 4;
        const float4 v = mlp_xform<PROY>(ay, s_vy, p.n0 * 32 + c, oky[jj], ry[jj]);
        if constexpr (TR) stage_planes(p_dy + (r * ldn + c) * 2, PBN, v);
        else *reinterpret_cast<float4*>(s_dy + r * ldn + c) = v;
      }
      if (f < 32 * qk) {
        const int r = f / qk, c = (f - r * qk) * 4;
        float4 v = ra[jj].x;
        if (p.pvec) {
          MlpRaw<PRO_BNRELU> rb;
          rb.x = v;
          v = mlp_xform<PRO_BNRELU>(ax, s_vx, p.k0 * 32 + c, oka[jj], rb);
        }
        if constexpr (TR) stage_planes(p_a + (r * ldk + c) * 2, PBK, v);
        else *reinterpret_cast<float4*>(s_a + r * ldk + c) = v;
      }
    }
    __syncthreads();
    const int next_chunk = last ? (dyn ? s_next : chunk + gx) : chunk;
    const int next_si = last ? 0 : si + 1;
    if (next_chunk < nchunk) prefetch(next_chunk * p.chunk + next_si);
    if constexpr (TR && X3 == 2) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        bf16x8 a8[TN];
#pragma unroll
        for (int i = 0; i < TN; ++i) a8[i] = frag(p_dy, ldn, (wn + 2 * i) * 32, c);
#pragma unroll
        for (int j = 0; j < TK; ++j) {
          const bf16x8 b8 = frag(p_a, ldk, (wk + 2 * j) * 32, c);
#pragma unroll
          for (int i = 0; i < TN; ++i)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a8[i], b8, acc[i][j], 0, 0, 0);
        }
      }
    } else if constexpr (TR && X3 == 1) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        bf16x8 ah[TN], am[TN], al[TN];
#pragma unroll
        for (int i = 0; i < TN; ++i) {
          ah[i] = frag(p_dy, ldn, (wn + 2 * i) * 32, c);
          am[i] = frag(p_dy + PBN, ldn, (wn + 2 * i) * 32, c);
          al[i] = frag(p_dy + 2 * PBN, ldn, (wn + 2 * i) * 32, c);
        }
#pragma unroll
        for (int j = 0; j < TK; ++j) {
          const bf16x8 bh = frag(p_a, ldk, (wk + 2 * j) * 32, c);
          const bf16x8 bm = frag(p_a + PBK, ldk, (wk + 2 * j) * 32, c);
          const bf16x8 bl = frag(p_a + 2 * PBK, ldk, (wk + 2 * j) * 32, c);
#pragma unroll
          for (int i = 0; i < TN; ++i) {
            if (DW_DBG(p, 1)) { acc[i][j][0] += (float)al[i][0] + (float)bh[0]; continue; }
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh, acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl, acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am[i], bm, acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am[i], bh, acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bm, acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh, acc[i][j], 0, 0, 0);
          }
        }
      }
    } else if constexpr (X3 == 2) {
      // compute dtype bf16: the same column gather, operands rounded to bf16, one MFMA per tile pair
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        auto gather1 = [&](const float* col, int ld) {
          const float* q = col + (16 * c + 8 * lh) * ld;
          const bf16x4 lo = to_bf16x4(make_float4(q[0], q[ld], q[2 * ld], q[3 * ld]));
          const bf16x4 hi = to_bf16x4(make_float4(q[4 * ld], q[5 * ld], q[6 * ld], q[7 * ld]));
          return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        };
        bf16x8 a8[TN];
#pragma unroll
        for (int i = 0; i < TN; ++i) a8[i] = gather1(s_dy + (wn + 2 * i) * 32 + lr, ldn);
#pragma unroll
        for (int j = 0; j < TK; ++j) {
          const bf16x8 b8 = gather1(s_a + (wk + 2 * j) * 32 + lr, ldk);
#pragma unroll
          for (int i = 0; i < TN; ++i)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a8[i], b8, acc[i][j], 0, 0, 0);
        }
      }
    } else if constexpr (X3 == 1) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        // lane supplies rows 16c + 8lh .. +7 of column lr of its tiles
        bf16x8 ah[TN], am[TN], al[TN];
        auto gather = [&](const float* col, int ld, bf16x8& h, bf16x8& m, bf16x8& l) {
          if (DW_DBG(p, 2)) { h = m = l = bf16x8{}; return; }
          const float* q = col + (16 * c + 8 * lh) * ld;
          split3(make_float4(q[0], q[ld], q[2 * ld], q[3 * ld]),
                 make_float4(q[4 * ld], q[5 * ld], q[6 * ld], q[7 * ld]), h, m, l);
        };
#pragma unroll
        for (int i = 0; i < TN; ++i) gather(s_dy + (wn + 2 * i) * 32 + lr, ldn, ah[i], am[i], al[i]);
#pragma unroll
        for (int j = 0; j < TK; ++j) {
          bf16x8 bh, bm, bl;
          gather(s_a + (wk + 2 * j) * 32 + lr, ldk, bh, bm, bl);
#pragma unroll
          for (int i = 0; i < TN; ++i) {
            if (DW_DBG(p, 1)) { acc[i][j][0] += (float)al[i][0] + (float)bh[0]; continue; }
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh, acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl, acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am[i], bm, acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am[i], bh, acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bm, acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh, acc[i][j], 0, 0, 0);
          }
        }
      }
    } else
    // A-op: dY^T -> lane supplies dY[r = 2m + lh][n = tn*32 + lr]; B-op: A[r][k = tk*32 + lr]
#pragma unroll 4
    for (int m = 0; m < 16; ++m) {
      float a[TN], b[TK];
#pragma unroll
      for (int i = 0; i < TN; ++i) a[i] = s_dy[(2 * m + lh) * ldn + (wn + 2 * i) * 32 + lr];
#pragma unroll
      for (int j = 0; j < TK; ++j) b[j] = s_a[(2 * m + lh) * ldk + (wk + 2 * j) * 32 + lr];
#pragma unroll
      for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TK; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    chunk = next_chunk;
    si = next_si;
  }
  if (dyn && threadIdx.x == 0) {
    // re-arm the counters for the next launch that is handed this set: column-lasts, then the last
    int* done = p.sched + DW_MAX_SUB;
    if (atomicAdd(done + by, 1) == gx - 1) {
      atomicExch(done + by, 0);
      atomicExch(p.sched + by, 0);
    }
  }
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < TK; ++j) {
      const int tn = wn + 2 * i, tk = wk + 2 * j;
      if (tn < p.NTn && tk < p.NTk) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int n = (p.n0 + tn) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          const int k = (p.k0 + tk) * 32 + lr;
          if (n < p.N && k < p.K && (!DW_DBG(p, 8) || acc[i][j][r] == 12345.f)) atomicAdd(p.dW + (size_t)n * p.lddw + k, acc[i][j][r]);
        }
      }
    }
}

template <int TN, int TK, bool SPARSE, int X3 = 0>
__global__ __launch_bounds__(256, 2) void mlp_dw_kernel(DwArgs p) {
  mlp_dw_body<TN, TK, SPARSE, X3>(p, (int)blockIdx.x, (int)blockIdx.y, (int)gridDim.x);
}

// Several weight-gradient launches of ONE template variant as one grid: nothing in a backward depends on a
// layer's dW, so the few-row stacks (FP modules, vote module, prediction heads: 15-20 launches of ~20 us)
// queue theirs and issue them together at the end (demf_mlp_gemm_bwd_dw_group) - the launches' ramps and tails
// overlap and the graph has that many fewer dependent nodes.
constexpr int DW_GROUP_MAX = 12;
struct DwGroup {
  int n;
  int start[DW_GROUP_MAX + 1];     // first block of job j
  int gx[DW_GROUP_MAX];            // its grid.x (row chunks); grid.y = (start[j+1] - start[j]) / gx
  DwArgs job[DW_GROUP_MAX];
};
template <int TN, int TK, bool SPARSE, int X3 = 0>
__global__ __launch_bounds__(256, 2) void mlp_dw_group_kernel(DwGroup g) {
  const int b = (int)blockIdx.x;
  int j = 0;
  while (j + 1 < g.n && b >= g.start[j + 1]) ++j;
  const int local = b - g.start[j], gx = g.gx[j];
  mlp_dw_body<TN, TK, SPARSE, X3>(g.job[j], local % gx, local / gx, gx);
}

}  // namespace demf

using namespace demf;

extern "C" int demf_mlp_gemm_bwd_dw_ld(int, int, int, int, const float*, const float*, const int*, int,
                                       const float*, const float*, const float*, const float*, float*,
                                       int, demf_stream_t);

extern "C" int demf_mlp_gemm_bwd_dw(int R, int N, int K, int ldx, const float* G, const float* dP,
                                    const int* arg, int ns, const float* Y, const float* vec6,
                                    const float* Xprev, const float* prev_scale_shift, float* dW,
                                    demf_stream_t stream) {
  return demf_mlp_gemm_bwd_dw_ld(R, N, K, ldx, G, dP, arg, ns, Y, vec6, Xprev, prev_scale_shift, dW, K,
                                 stream);
}

namespace {
struct DwPlan {
  DwArgs a;
  int gx, nsub, tn, tk, x3;      // x3: 0 fp32 MFMA, 1 three-term split, 2 bf16
  bool sparse;
  size_t lds;
};

// argument checks + launch geometry of one weight-gradient product (shared by the single and the grouped entry)
int dw_plan(int R, int N, int K, int ldx, const float* G, const float* dP, const int* arg, int ns, const float* Y,
            const float* vec6, const float* Xprev, const float* prev_scale_shift, float* dW, int lddw, bool allow_dyn,
            DwPlan& pl) {
  DEMF_REQUIRE(R >= 0 && N >= 4 && N % 4 == 0 && K >= 4 && K % 4 == 0 && ldx >= K && ldx % 4 == 0 &&
                   lddw >= K,
               "mlp_gemm_bwd_dw: bad sizes R=%d N=%d K=%d lddw=%d", R, N, K, lddw);
  pl.gx = 0;
  if (R == 0) return DEMF_OK;
  DEMF_REQUIRE(Y && vec6 && Xprev && dW && (G || (dP && arg && ns >= 1)), "mlp_gemm_bwd_dw: null pointer");
  const int TNt = cdiv(N, 32), TKt = cdiv(K, 32);
  // one launch: grid.x strides the 32-row slabs, grid.y enumerates the (<= 4x4-tile) sub-blocks
  // of the N x K output, so even a 4 k-row layer spreads over the whole chip
  int tn = TNt > 2 ? 2 : 1, tk = TKt > 2 ? 2 : 1;
  // few rows: 64 x 64 sub-blocks (4x as many blockIdx.y columns) and correspondingly fewer row chunks -
  // every block ends by adding its whole sub-block to dW with atomics, and with 128 x 128 sub-blocks x
  // R/128 chunks that flush (R/128 x N x K atomics) is most of a small launch
  // (round 5: also the 32 768-row products of the vote aggregation - they then join the grouped launch of the other
  // few-row products instead of running as two launches of their own: 292 -> 277 us for the step's 17 products,
  // tools/dw_micro.py; 5.074 -> 5.059 ms per step in situ)
  if (R <= sw().dw_small_r) tn = tk = 1;
  const int tile_ab = sw().dw_tile;       // A/B: 12 -> 64 x 128 sub-blocks, 21 -> 128 x 64, 22, 11
  if (tile_ab) { tn = TNt > 2 ? tile_ab / 10 : 1; tk = TKt > 2 ? tile_ab % 10 : 1; }
  DwArgs a{};
  a.R = R; a.N = N; a.K = K; a.ldx = ldx; a.Yl = Y; a.G = G; a.dP = dP; a.arg = arg; a.ns = ns;
  a.vec = vec6; a.Xp = Xprev; a.pvec = prev_scale_shift; a.dW = dW; a.lddw = lddw;
  a.dbg = sw().dw_dbg;
  const int nsub_n = cdiv(TNt, 2 * tn);
  a.nsub_k = cdiv(TKt, 2 * tk);
  const int nsub = nsub_n * a.nsub_k;
  // (DEMF_X3_MASK bit 2: weight-gradient launches)
  pl.x3 = (compute_bf16() && !sw().dw_f32) ? 2 : ((compute_mode() == 2 && (sw().x3_mask & 4)) ? 1 : 0);
  if (DEMF_DW_TR && pl.x3 != 0)      // bf16 planes [PL][32][W + 8] of both operands (mlp_dw_body)
    pl.lds = (size_t)(pl.x3 == 1 ? 3 : 1) * 32 * ((2 * tn * 32 + 8) + (2 * tk * 32 + 8)) * 2 + sizeof(float) * (5 * N + 2 * K);
  else
    pl.lds = sizeof(float) * (32 * ((2 * tn * 32 + 4) + (2 * tk * 32 + 4)) + 5 * N + 2 * K);
  int gx = cdiv(R, 32 * 4);
  const int tot = sw().dw_grid;
  const int cap = tot / nsub > 16 ? tot / nsub : 16;
  if (gx > cap) gx = cap;
  if (gx < 1) gx = 1;
  // dynamic chunk claims (DEMF_DW_DYN=1): measured neutral on the training step, so the default
  // stays the static slab striding (chunk = 1)
  a.chunk = 1;
  if (allow_dyn && sw().dw_dyn) {
    const int nslab = cdiv(R, 32);
    a.chunk = nslab / (gx * 4);                  // >= 4 claims per block, at most DW_CHUNK slabs each
    a.chunk = a.chunk < 1 ? 1 : (a.chunk > DW_CHUNK ? DW_CHUNK : a.chunk);
    const int nchunk = cdiv(nslab, a.chunk);
    if (gx > nchunk) gx = nchunk;
    if (nchunk > 2 * gx && nsub <= DW_MAX_SUB) a.sched = sched_slot();
  }
  pl.a = a; pl.gx = gx; pl.nsub = nsub; pl.tn = tn; pl.tk = tk; pl.sparse = G == nullptr;
  return DEMF_OK;
}

template <int X3>
void dw_launch_one(const DwPlan& pl, hipStream_t s) {
  const dim3 grid(pl.gx, pl.nsub);
#define DWV(TNv, TKv)                                                                                       \
  if (pl.sparse) hipLaunchKernelGGL((mlp_dw_kernel<TNv, TKv, true, X3>), grid, dim3(256), pl.lds, s, pl.a); \
  else hipLaunchKernelGGL((mlp_dw_kernel<TNv, TKv, false, X3>), grid, dim3(256), pl.lds, s, pl.a)
  if (pl.tn == 1 && pl.tk == 1) { DWV(1, 1); }
  else if (pl.tn == 1) { DWV(1, 2); }
  else if (pl.tk == 1) { DWV(2, 1); }
  else { DWV(2, 2); }
#undef DWV
}

template <int X3>
void dw_launch_group(const DwGroup& g, int tn, int tk, bool sparse, size_t lds, hipStream_t s) {
  const dim3 grid(g.start[g.n]);
#define DWG(TNv, TKv)                                                                                        \
  if (sparse) hipLaunchKernelGGL((mlp_dw_group_kernel<TNv, TKv, true, X3>), grid, dim3(256), lds, s, g);     \
  else hipLaunchKernelGGL((mlp_dw_group_kernel<TNv, TKv, false, X3>), grid, dim3(256), lds, s, g)
  if (tn == 1 && tk == 1) { DWG(1, 1); }
  else if (tn == 1) { DWG(1, 2); }
  else if (tk == 1) { DWG(2, 1); }
  else { DWG(2, 2); }
#undef DWG
}
}  // namespace

extern "C" int demf_mlp_gemm_bwd_dw_ld(int R, int N, int K, int ldx, const float* G, const float* dP,
                                       const int* arg, int ns, const float* Y, const float* vec6,
                                       const float* Xprev, const float* prev_scale_shift, float* dW,
                                       int lddw, demf_stream_t stream) {
  DwPlan pl;
  if (int e = dw_plan(R, N, K, ldx, G, dP, arg, ns, Y, vec6, Xprev, prev_scale_shift, dW, lddw, true, pl)) return e;
  if (pl.gx == 0) return DEMF_OK;
  hipStream_t s = (hipStream_t)stream;
  if (pl.x3 == 2) dw_launch_one<2>(pl, s);
  else if (pl.x3 == 1) dw_launch_one<1>(pl, s);
  else dw_launch_one<0>(pl, s);
  return check_launch("mlp_gemm_bwd_dw");
}

extern "C" int demf_mlp_gemm_bwd_dw_group(int n, const demf_dw_job* jobs, demf_stream_t stream) {
  DEMF_REQUIRE(n >= 0 && (n == 0 || jobs), "mlp_gemm_bwd_dw_group: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  std::vector<DwPlan> plans;
  plans.reserve(n);
  for (int i = 0; i < n; ++i) {
    const demf_dw_job& j = jobs[i];
    DwPlan pl;
    if (int e = dw_plan(j.R, j.N, j.K, j.ldx, j.G, j.dP, j.arg, j.ns, j.Y, j.vec6, j.Xprev, j.prev_scale_shift, j.dW,
                        j.lddw, false, pl))
      return e;
    if (pl.gx) plans.push_back(pl);
    if (sw().dw_trace && pl.gx)       // the step's products, one line each (tools/dw_micro.py)
      fprintf(stderr, "[dw] R=%d N=%d K=%d ldx=%d sparse=%d ns=%d bnrelu_in=%d tile=%dx%d grid=%dx%d\n", j.R, j.N, j.K, j.ldx,
              (int)pl.sparse, j.ns, j.prev_scale_shift != nullptr, pl.tn, pl.tk, pl.gx, pl.nsub);
  }
  std::vector<char> done(plans.size(), 0);
  for (size_t i = 0; i < plans.size(); ++i) {
    if (done[i]) continue;
    // every not yet issued job of the same kernel variant, DW_GROUP_MAX at a time
    DwGroup g{};
    size_t lds = 0;
    const DwPlan& f = plans[i];
    for (size_t k = i; k < plans.size() && g.n < DW_GROUP_MAX; ++k) {
      const DwPlan& q = plans[k];
      if (done[k] || q.tn != f.tn || q.tk != f.tk || q.sparse != f.sparse || q.x3 != f.x3) continue;
      g.job[g.n] = q.a; g.gx[g.n] = q.gx;
      g.start[g.n + 1] = g.start[g.n] + q.gx * q.nsub;
      lds = q.lds > lds ? q.lds : lds;
      ++g.n;
      done[k] = 1;
    }
    if (g.n == 1) {
      if (f.x3 == 2) dw_launch_one<2>(f, s);
      else if (f.x3 == 1) dw_launch_one<1>(f, s);
      else dw_launch_one<0>(f, s);
    } else if (f.x3 == 2) dw_launch_group<2>(g, f.tn, f.tk, f.sparse, lds, s);
    else if (f.x3 == 1) dw_launch_group<1>(g, f.tn, f.tk, f.sparse, lds, s);
    else dw_launch_group<0>(g, f.tn, f.tk, f.sparse, lds, s);
    if (int e = check_launch("mlp_gemm_bwd_dw_group")) return e;
  }
  return DEMF_OK;
}
