// Fused shared-MLP kernels for gfx950: 1x1 conv (GEMM) + train-mode BatchNorm + ReLU (+ max
// over neighbours), forward and backward, on point-major rows.
//
// This is the dense half of every PointSAModule the reference builds
// (demf/modeling/heads/class_agnostic_vote_head.py:383 via build_sa_module; backbone
// configs/demf/demf_votenet.py:48-62): upstream runs Conv2d -> BN2d -> ReLU as separate
// kernels over (B,C,M,ns) and materialises every intermediate.  Here a layer is ONE pass:
//
//   forward   Y_l = act_{l-1}(Y_{l-1}) @ W_l^T          act(y) = max(0, y*scale + shift)
//             - the previous layer's BN+ReLU is applied in the A-operand prologue (A is never
//               materialised), per-channel sum / sum-of-squares of Y_l are reduced in the
//               epilogue (fp32 per block, fp64 atomics across blocks) -> batch statistics;
//   tail      out = max_s act_L(Y_L)  fused with the last BN+ReLU;
//   backward  dY_l = gamma*invstd*(dZ - mean(dZ) - xhat*mean(dZ*xhat)) is formed on the fly in
//             the prologue of  dA_{l-1} = dY_l @ W_l  and of  dW_l = dY_l^T @ A_{l-1}.
//
// In this file: the generic form of that GEMM (mlp_gemm_kernel: any K <= 512, every prologue and epilogue, in the
// compute modes of csrc/launch_state.hip - fp32 MFMA, bf16 MFMA, fp32 as three bf16 terms), the dispatcher that hands
// a launch to the first special form that takes it (launch_gemm_t; the forms live in csrc/mlp_fwd_pc.hip,
// csrc/mlp_fwd_res.hip and csrc/mlp_tile.hip, declared in csrc/mlp_args.h), the forward and input-gradient entry
// points, and the first-layer kernels of an SA1-shaped stack (mlp_first_stats_k, mlp_first_finish_k).  Weight
// gradients: csrc/mlp_dw.hip.  BatchNorm launches of their own: csrc/bn.hip.
// At these skinny shapes (K,N <= 512, rows up to 1M) the kernels are HBM-bound: algorithmic bytes are
// rows*(K+N)*4 per forward layer.
//
// Fragment trick (fp32 MFMA, v_mfma_f32_32x32x2_f32): for C = A(RxK) * Bt(NxK)^T with both operands K-contiguous,
// a lane loads ONE float4 along K for A (row = lane&31) and one per column tile for Bt (row = lane&31), at
// k = k0 + 4*(lane>>5) .. +3, and feeds component m to MFMA m: MFMA m then contracts over
// k in {k0+m, k0+4+m} on both operands consistently - four MFMAs consume the two float4.
#include "mlp_dev.h"
#include <type_traits>

namespace demf {

#ifdef DEMF_MLP_PROFILE   // tools/mlp_phase_prof.py: per-phase shader cycles of block (0,0), thread 0
__device__ long long g_mlp_prof[16];
#define MP_T(k) const long long mp##k = __builtin_readcyclecounter();
#define MP_ACC(i, a, b) if (mp_on) mp_acc[i] += (b) - (a);
#else
#define MP_T(k)
#define MP_ACC(i, a, b)
#endif

// C(R x N) = pro(A)(R x K) @ Bt(N x K)^T ; NT = ceil(N/32) column tiles per wave (all of N).
// The (tile, k-step) sequence of a block is flattened so the next 32 x BK slab of A (per wave,
// prologue applied on arrival) and the next N x BK slab of Bt (shared by the 4 waves) are already
// in flight while the current ones feed the MFMAs.  A lives in a wave-private LDS region; Bt is
// staged once per step for the whole block as full 128-byte rows (fragment-shaped loads straight
// from global would cost 32 cache lines per wave-instruction).
// RT = 32-row tiles per wave (2 when the accumulators fit: twice the MFMA work per Bt fragment
// and per barrier).  The prologue's per-channel vectors are copied to LDS once per block.
// CM = 1 (bf16): the A / B slabs hold bf16 (same byte row stride as the fp32 layout, so the slab
// doubles as fp32 staging for the FIRST / RED epilogues unchanged) and a K step of 32 is two
// v_mfma_f32_32x32x16_bf16 per tile instead of sixteen v_mfma_f32_32x32x2_f32.
// CM = 2 (three-term split): the A slab stays fp32 - each wave splits the 8 floats of its own
// fragment in registers after the LDS read (its rows are private to it, so nothing is split twice) -
// and the Bt slab, which all four waves share, is split once on its way into LDS: row stride
// MLP_LD3 floats = [32 h | 32 m | 32 l] bf16 + 16 B pad (52 dwords: 8 consecutive rows still cover
// the 32 banks with their 16-byte reads).  Six bf16 MFMAs per tile and 16 columns of K.
template <int NT, int RT, int PRO, bool STATS, bool POOL = false, bool FIRST = false, bool RED = false,
          int CM = 0, bool SEL = false>
__global__ __launch_bounds__(256, 2) void mlp_gemm_kernel(MlpArgs p) {
  static_assert(!SEL || POOL, "SEL is a mode of the pooled epilogue");
  static_assert(!(STATS && RED) && !(FIRST && RED), "one column-sum epilogue at a time");
  constexpr bool BF16 = CM == 1, X3 = CM == 2;
  constexpr int LDB = X3 ? MLP_LD3 : MLP_LD;
  constexpr int WROWS = 32 * RT;          // rows per wave
  constexpr int BROWS = 4 * WROWS;        // rows per block tile
  constexpr int NVEC = PRO == PRO_NONE ? 0 : (PRO == PRO_BNRELU ? 2 : 5);
  __shared__ __attribute__((aligned(16))) float s_a[4][WROWS * MLP_LD];
  __shared__ __attribute__((aligned(16))) float s_b[NT * 32 * LDB];
  __shared__ __attribute__((aligned(16))) float s_vec[NVEC ? NVEC * MLP_MAXK : 4];
  __shared__ float s_red[(STATS || RED) ? 4 * NT * 32 * 2 : (FIRST ? 4 * NT * 32 * 10 + 16 : 1)];
  __shared__ float4 s_pool[(POOL && RT == 1) ? 4 * NT * 32 : 1];
  if constexpr (NVEC > 0) {
    // compact copy: vector v of length K lives at s_vec + v*K (same addressing as global)
    for (int i = threadIdx.x; i < NVEC * p.K; i += 256) s_vec[i] = p.vec[i];
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int lr = lane & 31, lh = lane >> 5;
  float* sa = s_a[wave];
  // few-row launches split the output columns over blockIdx.y so the chip is still filled
  // Pooled launches with two column halves use a 1-D grid in which blocks b and b+8 - the same
  // XCD under round-robin dispatch - take the two halves of the same row tiles at the same time,
  // so the second read of the A rows is an L2 hit instead of a second trip to HBM.
  int bx = blockIdx.x, gx = gridDim.x, by = blockIdx.y;
  if constexpr (POOL) {
    if (p.halves == 2) {
      by = (bx >> 3) & 1;
      bx = (bx & 7) | ((bx >> 4) << 3);
      gx >>= 1;
    }
  }
  const int cofs = by * NT * 32;
  const int ntiles = (p.R + BROWS - 1) / BROWS;
  const int ksteps = (p.K + MLP_BK - 1) / MLP_BK;
  // Persistent launches take their first tile by block index and every further one from a device
  // counter, claimed one tile ahead (the atomic's latency hides behind a whole tile): blocks that
  // run slower - e.g. while the furthest-point chain of the next batch is resident on the chip -
  // simply take fewer tiles instead of holding the launch back.  sched == null: static striding.
  // Same-address atomics serialise (~60 ns each), so the blocks are split into SCHED_GROUPS
  // groups that interleave over the XCDs and over the tile range in runs of 8; a group owns every
  // SCHED_GROUPS-th run of 8 tiles and has its own counter (32 claimants instead of 512).
  __shared__ int s_next;
  const bool dyn = p.sched != nullptr;
  const int grp = (bx >> 3) & (SCHED_GROUPS - 1);
  const int grp_first = gx / SCHED_GROUPS;          // tiles per group taken by block index
  auto group_tile = [&](int j) { return (((j >> 3) * SCHED_GROUPS + grp) << 3) + (j & 7); };
  int claimed = 0;
  float cs1[NT], cs2[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) cs1[nt] = cs2[nt] = 0.f;
  float fs[FIRST ? NT : 1][10];
  float4 fcx = make_float4(0.f, 0.f, 0.f, 0.f);
  if constexpr (FIRST) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int q = 0; q < 10; ++q) fs[nt][q] = 0.f;
  }
  f32x16 acc[RT][NT];
  unsigned selbits = 0;                            // SEL: bit nt = this lane's column of tile nt has gamma < 0
  if constexpr (SEL) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int col = cofs + nt * 32 + lr;
      if (col < p.N && p.fin.gamma[col] < 0.f) selbits |= 1u << nt;
    }
  }

  const int pr = lane >> 3, pc = (lane & 7) * 4;   // this lane's slot in a 32 x BK slab
  const int br = threadIdx.x >> 3;                  // Bt slab: row br + 32*i, cols pc..pc+3
  MlpRaw<PRO> pre[4 * RT];
  bool pok[4 * RT];
  float4 preb[NT];
  auto prefetch = [&](int tile, int ks) {
    const int k0 = ks * MLP_BK;
    const int row0 = tile * BROWS + wave * WROWS;
#pragma unroll
    for (int it = 0; it < 4 * RT; ++it) {
      const int row = row0 + it * 8 + pr, col = k0 + pc;
      pok[it] = row < p.R && col < p.K;
      mlp_fetch<PRO>(p, row, col, pok[it], pre[it]);   // raw: stays in flight until the LDS write
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int n = cofs + br + 32 * i, col = k0 + pc;
      preb[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (p.ldb > 0) {
        // transposed source: this thread's float4 runs along the OUTPUT columns of reduction row br
        const int kk = k0 + br, nn = cofs + 32 * i + pc;
        if (kk < p.K && nn < p.N) preb[i] = *reinterpret_cast<const float4*>(p.Bt + (size_t)kk * p.ldb + nn);
      } else if (n < p.N && col < p.K) {
        preb[i] = *reinterpret_cast<const float4*>(p.Bt + (size_t)n * p.K + col);
      }
    }
  };
#ifdef DEMF_MLP_PROFILE
  long long mp_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const bool mp_on = blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0;
#endif
  int tile = bx;
  if (tile < ntiles) prefetch(tile, 0);

  int ks = 0;
  while (tile < ntiles) {
    MP_T(0)
    const int k0 = ks * MLP_BK;
    const int row0 = tile * BROWS + wave * WROWS;
    const bool last_ks = ks == ksteps - 1;
    if (dyn && threadIdx.x == 0) {
      if (ks == 0) claimed = group_tile(grp_first + atomicAdd(p.sched + grp, 1));
      if (last_ks) s_next = claimed;
    }
    float* sb = s_b;
    if (ks == 0) {
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[rt][nt][r] = 0.f;
    }
    lds_barrier();                                    // everyone is done reading the old Bt slab (LDS-only
                                                      // wait: the previous tile's output stores stay in flight)
    MP_T(1) MP_ACC(0, mp0, mp1)
    if constexpr (BF16) {
      // bf16 element (row, k) lives at byte row * 4*MLP_LD + 2*k of the slab
      char* sab = reinterpret_cast<char*>(sa);
      char* sbb = reinterpret_cast<char*>(sb);
#pragma unroll
      for (int it = 0; it < 4 * RT; ++it)
        *reinterpret_cast<bf16x4*>(sab + (it * 8 + pr) * (4 * MLP_LD) + 2 * pc) =
            to_bf16x4(mlp_xform<PRO>(p, s_vec, k0 + pc, pok[it], pre[it]));
#pragma unroll
      for (int i = 0; i < NT; ++i)
        if (p.ldb > 0) {
          char* d = sbb + (32 * i + pc) * (4 * MLP_LD) + 2 * br;
          *reinterpret_cast<__bf16*>(d) = (__bf16)preb[i].x;
          *reinterpret_cast<__bf16*>(d + 4 * MLP_LD) = (__bf16)preb[i].y;
          *reinterpret_cast<__bf16*>(d + 8 * MLP_LD) = (__bf16)preb[i].z;
          *reinterpret_cast<__bf16*>(d + 12 * MLP_LD) = (__bf16)preb[i].w;
        } else {
          *reinterpret_cast<bf16x4*>(sbb + (br + 32 * i) * (4 * MLP_LD) + 2 * pc) = to_bf16x4(preb[i]);
        }
    } else if constexpr (X3) {
#pragma unroll
      for (int it = 0; it < 4 * RT; ++it)
        *reinterpret_cast<float4*>(sa + (it * 8 + pr) * MLP_LD + pc) =
            mlp_xform<PRO>(p, s_vec, k0 + pc, pok[it], pre[it]);
      // term t of element (n, k) lives at byte n * 4*MLP_LD3 + 64*t + 2*k of the Bt slab
      char* sbb = reinterpret_cast<char*>(sb);
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        bf16x4 h, m, l;
        split3(preb[i], h, m, l);
        if (p.ldb > 0) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            char* d = sbb + (32 * i + pc + e) * (4 * MLP_LD3) + 2 * br;
            *reinterpret_cast<__bf16*>(d) = h[e];
            *reinterpret_cast<__bf16*>(d + 64) = m[e];
            *reinterpret_cast<__bf16*>(d + 128) = l[e];
          }
        } else {
          char* d = sbb + (br + 32 * i) * (4 * MLP_LD3) + 2 * pc;
          *reinterpret_cast<bf16x4*>(d) = h;
          *reinterpret_cast<bf16x4*>(d + 64) = m;
          *reinterpret_cast<bf16x4*>(d + 128) = l;
        }
      }
    } else {
#pragma unroll
    for (int it = 0; it < 4 * RT; ++it)
      *reinterpret_cast<float4*>(sa + (it * 8 + pr) * MLP_LD + pc) =
          mlp_xform<PRO>(p, s_vec, k0 + pc, pok[it], pre[it]);
#pragma unroll
    for (int i = 0; i < NT; ++i)
      if (p.ldb > 0) {
        float* d = sb + (32 * i + pc) * MLP_LD + br;
        d[0] = preb[i].x; d[MLP_LD] = preb[i].y; d[2 * MLP_LD] = preb[i].z; d[3 * MLP_LD] = preb[i].w;
      } else {
        *reinterpret_cast<float4*>(sb + (br + 32 * i) * MLP_LD + pc) = preb[i];
      }
    }
    MP_T(2) MP_ACC(1, mp1, mp2)
    lds_barrier();
    MP_T(3) MP_ACC(2, mp2, mp3)
    // the pooling epilogue needs registers: on the last k-step of a tile the next tile's
    // operands are fetched after it instead of being held in flight across it
    constexpr bool DEFER = (POOL && RT == 2) || FIRST;   // epilogues that need the prefetch registers
    const bool defer_prefetch = DEFER && last_ks;
    const int next_tile = last_ks ? (dyn ? s_next : tile + gx) : tile;
    const int next_ks = last_ks ? 0 : ks + 1;
    if (next_tile < ntiles && !defer_prefetch) prefetch(next_tile, next_ks);
    MP_T(4) MP_ACC(3, mp3, mp4)
    // FIRST: the wave's 64 x 32 half tile of layer 0's output (coalesced float4 rows) and its input
    // rows are fetched before the MFMAs of the last k-step and staged through the wave's A slab
    float4 yq[(FIRST || RED) ? 2 * RT * 2 : 1];
    float4 xq = make_float4(0.f, 0.f, 0.f, 0.f);
    auto first_load = [&](int half) {
#pragma unroll
      for (int j = 0; j < 2 * RT * 2; ++j) {
        const int id = lane + 64 * j;
        const int row = row0 + (id >> 3);
        yq[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < p.R && cofs + 32 * half + 4 * (id & 7) < p.N)
          yq[j] = *reinterpret_cast<const float4*>(p.fY + (size_t)row * p.fld + p.fc0 + cofs + 32 * half + 4 * (id & 7));
      }
    };
    auto first_store = [&]() {
#pragma unroll
      for (int j = 0; j < 2 * RT * 2; ++j) {
        const int id = lane + 64 * j;
        *reinterpret_cast<float4*>(sa + (id >> 3) * MLP_LD + 4 * (id & 7)) = yq[j];
      }
    };
    if constexpr (RED) {
      if (last_ks) first_load(0);
    }
    if constexpr (FIRST) {
      if (last_ks) {
        first_load(0);
        if (lane < WROWS && row0 + lane < p.R)
          xq = *reinterpret_cast<const float4*>(p.fX + (size_t)(row0 + lane) * 4);
      }
    }
    if constexpr (BF16) {
      const char* sab = reinterpret_cast<const char*>(sa);
      const char* sbb = reinterpret_cast<const char*>(sb);
      const int kch = min(MLP_BK / 16, (p.K - k0 + 15) / 16);
      for (int c16 = 0; c16 < kch; ++c16) {
        bf16x8 a8[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
          a8[rt] = *reinterpret_cast<const bf16x8*>(sab + (rt * 32 + lr) * (4 * MLP_LD) + 2 * (c16 * 16 + 8 * lh));
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const bf16x8 b8 = *reinterpret_cast<const bf16x8*>(sbb + (nt * 32 + lr) * (4 * MLP_LD) + 2 * (c16 * 16 + 8 * lh));
#pragma unroll
          for (int rt = 0; rt < RT; ++rt)
            acc[rt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a8[rt], b8, acc[rt][nt], 0, 0, 0);
        }
      }
    } else if constexpr (X3) {
      const char* sbb = reinterpret_cast<const char*>(sb);
      const int kch = min(MLP_BK / 16, (p.K - k0 + 15) / 16);
      for (int c16 = 0; c16 < kch; ++c16) {
        bf16x8 ah[RT], am[RT], al[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          const float* src = sa + (rt * 32 + lr) * MLP_LD + c16 * 16 + 8 * lh;
          split3(*reinterpret_cast<const float4*>(src), *reinterpret_cast<const float4*>(src + 4),
                 ah[rt], am[rt], al[rt]);
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const char* src = sbb + (nt * 32 + lr) * (4 * MLP_LD3) + 2 * (c16 * 16 + 8 * lh);
          const bf16x8 bh = *reinterpret_cast<const bf16x8*>(src);
          const bf16x8 bm = *reinterpret_cast<const bf16x8*>(src + 64);
          const bf16x8 bl = *reinterpret_cast<const bf16x8*>(src + 128);
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) {
            // small terms first
            acc[rt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[rt], bh, acc[rt][nt], 0, 0, 0);
            acc[rt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[rt], bl, acc[rt][nt], 0, 0, 0);
            acc[rt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am[rt], bm, acc[rt][nt], 0, 0, 0);
            acc[rt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am[rt], bh, acc[rt][nt], 0, 0, 0);
            acc[rt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[rt], bm, acc[rt][nt], 0, 0, 0);
            acc[rt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[rt], bh, acc[rt][nt], 0, 0, 0);
          }
        }
      }
    } else {
    const int kchunks = min(MLP_BK / 8, (p.K - k0 + 7) / 8);
    for (int c8 = 0; c8 < kchunks; ++c8) {
      float4 a4[RT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
        a4[rt] = *reinterpret_cast<const float4*>(sa + (rt * 32 + lr) * MLP_LD + c8 * 8 + 4 * lh);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const float4 b4 = *reinterpret_cast<const float4*>(sb + (nt * 32 + lr) * MLP_LD + c8 * 8 + 4 * lh);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          acc[rt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[rt].x, b4.x, acc[rt][nt], 0, 0, 0);
          acc[rt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[rt].y, b4.y, acc[rt][nt], 0, 0, 0);
          acc[rt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[rt].z, b4.z, acc[rt][nt], 0, 0, 0);
          acc[rt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[rt].w, b4.w, acc[rt][nt], 0, 0, 0);
        }
      }
    }
    }
    MP_T(5) MP_ACC(4, mp4, mp5)
    if (last_ks) {
      // epilogue: C/D layout of 32x32: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        float s1 = 0.f, s2 = 0.f;
        if constexpr (FIRST) {
          const int col = cofs + nt * 32 + lr;
          const bool cok = col < p.N;
          const float sc0 = cok ? p.fss[p.fc0 + col] : 0.f, sh0 = cok ? p.fss[p.fld + p.fc0 + col] : 0.f;
          const float mu0 = cok ? p.fmi[p.fc0 + col] : 0.f, is0 = cok ? p.fmi[p.fld + p.fc0 + col] : 0.f;
          // stage this half of Y0 (and, once, the input rows in the 4 pad columns) in the A slab
          first_store();
          if (nt == 0 && lane < WROWS) *reinterpret_cast<float4*>(sa + lane * MLP_LD + MLP_BK) = xq;
          if (nt + 1 < NT) first_load(nt + 1);       // next half in flight during this one's sums
#pragma unroll
          for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int rl = rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
              if ((r & 3) == 0) __builtin_amdgcn_sched_barrier(0);   // keep the LDS reads from piling up
              if (row0 + rl < p.R && cok) {
                const float y = sa[rl * MLP_LD + lr];
                const float4 x = *reinterpret_cast<const float4*>(sa + rl * MLP_LD + MLP_BK);
                const float dz = __builtin_fmaf(y, sc0, sh0) > 0.f ? acc[rt][nt][r] : 0.f;
                fs[nt][0] += dz;
                fs[nt][1] = __builtin_fmaf(dz, (y - mu0) * is0, fs[nt][1]);
                fs[nt][2] = __builtin_fmaf(dz, x.x, fs[nt][2]);
                fs[nt][3] = __builtin_fmaf(dz, x.y, fs[nt][3]);
                fs[nt][4] = __builtin_fmaf(dz, x.z, fs[nt][4]);
                fs[nt][5] = __builtin_fmaf(dz, x.w, fs[nt][5]);
                fs[nt][6] = __builtin_fmaf(y, x.x, fs[nt][6]);
                fs[nt][7] = __builtin_fmaf(y, x.y, fs[nt][7]);
                fs[nt][8] = __builtin_fmaf(y, x.z, fs[nt][8]);
                fs[nt][9] = __builtin_fmaf(y, x.w, fs[nt][9]);
                if (nt == 0 && lr == 0 && by == 0) { fcx.x += x.x; fcx.y += x.y; fcx.z += x.z; fcx.w += x.w; }
              }
            }
        } else {
        float sc0 = 0.f, sh0 = 0.f, mu0 = 0.f, is0 = 0.f;
        if constexpr (RED) {
          const int col = cofs + nt * 32 + lr;
          if (col < p.N) {
            sc0 = p.fss[p.fc0 + col]; sh0 = p.fss[p.fld + p.fc0 + col];
            mu0 = p.fmi[p.fc0 + col]; is0 = p.fmi[p.fld + p.fc0 + col];
          }
          first_store();                             // this half of Y_{l-1} through the wave's A slab
          if (nt + 1 < NT) first_load(nt + 1);
        }
        // interior tiles of the pooled launches store unpredicated: a per-store bounds test costs an
        // exec-mask branch each; only the last row tile / a ragged column tile takes the checked path
        auto store_tile = [&](auto full_c) {
          constexpr bool FULL = decltype(full_c)::value;
#pragma unroll
          for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int row = row0 + rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
              const float v = acc[rt][nt][r];
              const bool ok = FULL || (row < p.R && cofs + nt * 32 + lr < p.N);
              if (ok) p.Y[(size_t)row * p.ldy + cofs + nt * 32 + lr] = v;
              if constexpr (RED) {
                if ((r & 3) == 0) __builtin_amdgcn_sched_barrier(0);
                if (ok) {
                  const float y = sa[(rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * MLP_LD + lr];
                  const float dz = __builtin_fmaf(y, sc0, sh0) > 0.f ? v : 0.f;
                  s1 += dz;
                  s2 = __builtin_fmaf(dz, (y - mu0) * is0, s2);
                }
              }
            }
          if constexpr (STATS) {
            // column statistics on register pairs: v_pk_add_f32 / v_pk_fma_f32 take two accumulators
            // per instruction (rows >= R are exact zeros: their A rows are zero)
            using f32x2 = float __attribute__((ext_vector_type(2)));
            f32x2 a1 = {0.f, 0.f}, a2 = {0.f, 0.f};
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
              for (int r = 0; r < 16; r += 2) {
                const f32x2 v = {acc[rt][nt][r], acc[rt][nt][r + 1]};
                a1 += v;
                a2 = __builtin_elementwise_fma(v, v, a2);
              }
            s1 += a1.x + a1.y;
            s2 += a2.x + a2.y;
          }
        };
        // (only in the pooled instantiations: duplicating the loop in the wide plain ones - up to
        // 128 accumulators live - made them 30-90 % slower)
        if constexpr (POOL) {
          if (tile * BROWS + BROWS <= p.R && cofs + NT * 32 <= p.N) store_tile(std::true_type{});
          else store_tile(std::false_type{});
        } else {
#pragma unroll
          for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int row = row0 + rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
              const float v = acc[rt][nt][r];
              if (row < p.R && cofs + nt * 32 + lr < p.N)
                p.Y[(size_t)row * p.ldy + cofs + nt * 32 + lr] = v;
              if constexpr (RED) {
                if ((r & 3) == 0) __builtin_amdgcn_sched_barrier(0);
                if (row < p.R && cofs + nt * 32 + lr < p.N) {
                  const float y = sa[(rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * MLP_LD + lr];
                  const float dz = __builtin_fmaf(y, sc0, sh0) > 0.f ? v : 0.f;
                  s1 += dz;
                  s2 = __builtin_fmaf(dz, (y - mu0) * is0, s2);
                }
              }
              if constexpr (STATS) {
                s1 += v;                   // rows >= R are exact zeros (their A rows are zero)
                s2 = __builtin_fmaf(v, v, s2);
              }
            }
        }
        }
        cs1[nt] += s1;
        cs2[nt] += s2;
        if constexpr (POOL) {
          {
            const int col = cofs + nt * 32 + lr;
            if constexpr (SEL) {
              const unsigned flip = ((selbits >> nt) & 1u) << 31;
              if (p.ns == 16) pool_epilogue_sel<RT, NT, 16>(p, acc, nt, row0, col, lh, flip);
              else if (p.ns == 32) pool_epilogue_sel<RT, NT, 32>(p, acc, nt, row0, col, lh, flip);
              else if constexpr (RT == 2) pool_epilogue_sel<RT, NT, 64>(p, acc, nt, row0, col, lh, flip);
              else pool_half_reduce_sel<NT>(acc, nt, wave, lr, lh, s_pool, flip);
            } else {
            if (p.ns == 16) pool_epilogue<RT, NT, 16>(p, acc, nt, row0, col, lh);
            else if (p.ns == 32) pool_epilogue<RT, NT, 32>(p, acc, nt, row0, col, lh);
            else if constexpr (RT == 2) pool_epilogue<RT, NT, 64>(p, acc, nt, row0, col, lh);
            else pool_half_reduce<NT>(acc, nt, wave, lr, lh, s_pool);
            }
          }
        }
      }
      if constexpr (POOL && RT == 1) {
        if (p.ns == 64) {                       // merge the two half groups of each wave pair
          lds_barrier();                        // (LDS-only: the tile's output stores keep draining)
          if ((wave & 1) == 0 && lh == 0) {
            const int grow = row0;              // first row of this wave pair's group
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
              const int col = cofs + nt * 32 + lr;
              if constexpr (SEL) {
                const float2* sp = reinterpret_cast<const float2*>(s_pool);
                const float2 a = sp[(wave * NT + nt) * 32 + lr];
                const float2 b = sp[((wave + 1) * NT + nt) * 32 + lr];
                const bool take_b = b.x > a.x;          // the even wave's offsets are the smaller ones
                if (grow < p.R && col < p.N) {
                  const unsigned flip = ((selbits >> nt) & 1u) << 31;
                  const size_t o = (size_t)(grow / 64) * p.N + col;
                  p.pmax[o] = flip_sign(take_b ? b.x : a.x, flip);
                  p.amax[o] = __builtin_bit_cast(int, take_b ? b.y : a.y);
                }
                continue;
              }
              const float4 a = s_pool[(wave * NT + nt) * 32 + lr];
              const float4 b = s_pool[((wave + 1) * NT + nt) * 32 + lr];
              float mx = a.x, mn = a.y;
              int ax = __builtin_bit_cast(int, a.z), an = __builtin_bit_cast(int, a.w);
              if (b.x > mx) { mx = b.x; ax = __builtin_bit_cast(int, b.z); }
              if (b.y < mn) { mn = b.y; an = __builtin_bit_cast(int, b.w); }
              if (grow < p.R && col < p.N) {
                const size_t o = (size_t)(grow / 64) * p.N + col;
                p.pmax[o] = mx; p.pmin[o] = mn; p.amax[o] = ax; p.amin[o] = an;
              }
            }
          }
        }
      }
      if constexpr ((POOL && RT == 2) || FIRST) {
        if (next_tile < ntiles) prefetch(next_tile, next_ks);
      }
    }
    MP_T(6) MP_ACC(5, mp5, mp6)
    tile = next_tile;
    ks = next_ks;
  }
#ifdef DEMF_MLP_PROFILE
  if (mp_on) { for (int i = 0; i < 8; ++i) atomicAdd((unsigned long long*)&g_mlp_prof[i], (unsigned long long)mp_acc[i]); atomicAdd((unsigned long long*)&g_mlp_prof[15], 1ull); }
#endif
  if (dyn) {
    // the last block out re-arms the counter pair for the next launch that uses this slot
    if (threadIdx.x == 0) {
      // (no fence: only atomics touch the counters, and an agent-scope release here would write the
      // XCD's whole L2 back once per block)
      // two-level count (512 same-address atomics with a return value would hold the last block
      // back by ~30 us): group members first, then the 16 group-lasts
      int* gdone = p.sched + SCHED_GROUPS;
      const int members = (int)(gridDim.x * gridDim.y) / SCHED_GROUPS;
      if (atomicAdd(gdone + 1 + grp, 1) == members - 1) {
        atomicExch(gdone + 1 + grp, 0);
        atomicExch(p.sched + grp, 0);
        if (atomicAdd(gdone, 1) == SCHED_GROUPS - 1) atomicExch(gdone, 0);
      }
    }
  }
  if constexpr (FIRST) {
    // lanes l and l+32 hold the same column: fold, then the 4 waves through LDS, then fp64 atomics
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int q = 0; q < 10; ++q) {
        const float v = fs[nt][q] + __shfl_xor(fs[nt][q], 32);
        if (lh == 0) s_red[((wave * NT + nt) * 10 + q) * 32 + lr] = v;
      }
    fcx.x += __shfl_xor(fcx.x, 32); fcx.y += __shfl_xor(fcx.y, 32);
    fcx.z += __shfl_xor(fcx.z, 32); fcx.w += __shfl_xor(fcx.w, 32);
    if (lane == 0) {
      float* c = s_red + 4 * NT * 32 * 10 + wave * 4;
      c[0] = fcx.x; c[1] = fcx.y; c[2] = fcx.z; c[3] = fcx.w;
    }
    __syncthreads();
    constexpr int PER = NT * 10 * 32;
    for (int i = threadIdx.x; i < PER; i += 256) {
      const float v = s_red[i] + s_red[PER + i] + s_red[2 * PER + i] + s_red[3 * PER + i];
      const int nt = i / 320, q = (i / 32) % 10, c = i & 31;
      const int col = cofs + nt * 32 + c;
      if (col < p.N) {
        // layout: g1 | g2 | P (N x 4) | Q (N x 4) | cx(4)
        const int dst = q < 2 ? q * p.N + col : (q < 6 ? 2 * p.N + col * 4 + (q - 2) : 6 * p.N + col * 4 + (q - 6));
        atomicAdd(p.fsum + dst, (double)v);
      }
    }
    if (threadIdx.x < 4 && by == 0) {
      const float* c = s_red + 4 * NT * 32 * 10;
      atomicAdd(p.fsum + 10 * p.N + threadIdx.x,
                (double)(c[threadIdx.x] + c[4 + threadIdx.x] + c[8 + threadIdx.x] + c[12 + threadIdx.x]));
    }
  }
  if constexpr (STATS || RED) {
    // lanes l and l+32 hold the same column: fold, then the 4 waves, then one fp64 atomic
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      cs1[nt] += __shfl_xor(cs1[nt], 32);
      cs2[nt] += __shfl_xor(cs2[nt], 32);
      if (lh == 0) {
        s_red[(wave * NT + nt) * 64 + lr] = cs1[nt];
        s_red[(wave * NT + nt) * 64 + 32 + lr] = cs2[nt];
      }
    }
    __syncthreads();
    // (the launch's last workgroup consumes the sums: they go to this workgroup's copy of the accumulator, bn_fin.h)
    const int lin_s = (int)(blockIdx.y * gridDim.x + blockIdx.x);
    double* sdst = p.stats;
    if constexpr (RED) {
      if (p.vfin.ticket != nullptr && p.vfin.racc != nullptr) sdst = repl_copy(p.vfin.racc, p.fld, lin_s);
    } else {
      if (p.fin.ss != nullptr && p.fin.racc != nullptr) sdst = repl_copy(p.fin.racc, p.N, lin_s);
    }
    for (int i = threadIdx.x; i < NT * 64; i += 256) {
      const float v = s_red[i] + s_red[NT * 64 + i] + s_red[2 * NT * 64 + i] + s_red[3 * NT * 64 + i];
      const int nt = i >> 6, which = (i >> 5) & 1, c = i & 31;
      if (cofs + nt * 32 + c < p.N)
        atomicAdd(sdst + which * (RED ? p.fld : p.N) + (RED ? p.fc0 : 0) + cofs + nt * 32 + c, (double)v);
    }
  }
  if constexpr (RED) {
    if (p.vfin.ticket != nullptr) {
      // layer l-1's backward vectors for this launch's columns, by its last workgroup (csrc/bn_fin.h)
      sync_drained();
      if (threadIdx.x == 0)
        s_next = last_workgroup(p.vfin.ticket, (int)(gridDim.x * gridDim.y), (int)(blockIdx.y * gridDim.x + blockIdx.x));
      __syncthreads();
      if (s_next) bn_vec_finalize(p.vfin, p.fld, p.fc0, p.N, p.stats, threadIdx.x, 256);
    }
  }
  if constexpr (STATS) {
    if (p.fin.ss != nullptr) {
      // Only atomics touch the sums and the counters, and sync_drained() waits for every wave's own
      // to be acknowledged, so no fence is needed.  Two-level exit count as above.
      sync_drained();
      if (threadIdx.x == 0) {
        const int total = (int)(gridDim.x * gridDim.y);
        const int lin = (int)(blockIdx.y * gridDim.x + blockIdx.x);
        const int ngroups = total < SCHED_GROUPS ? total : SCHED_GROUPS;
        const int g = lin % SCHED_GROUPS;
        const int members = total / SCHED_GROUPS + (g < total % SCHED_GROUPS ? 1 : 0);
        int* t = p.fin.ticket + FIN_OFF;
        int last = 0;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // own sum atomics acknowledged first (csrc/bn_fin.h)
        if (atomicAdd(t + 1 + g, 1) == members - 1) {
          atomicExch(t + 1 + g, 0);
          if (atomicAdd(t, 1) == ngroups - 1) { atomicExch(t, 0); last = 1; }
        }
        s_next = last;
      }
      __syncthreads();
      if (s_next) {
        const BnFin& f = p.fin;
        if (threadIdx.x == 0 && f.nbt != nullptr) *f.nbt += 1;
        for (int c = threadIdx.x; c < p.N; c += 256) {
          // read through the atomic unit (the sums were produced by device-scope atomics) and leave
          // the accumulator zeroed, in one exchange each
          double s1 = __builtin_bit_cast(
              double, atomicExch(reinterpret_cast<unsigned long long*>(p.stats + c), 0ull));
          double s2 = __builtin_bit_cast(
              double, atomicExch(reinterpret_cast<unsigned long long*>(p.stats + p.N + c), 0ull));
          if (f.racc != nullptr) { s1 += repl_take(f.racc, p.N, c); s2 += repl_take(f.racc, p.N, p.N + c); }
          bn_finalize_channel(c, p.N, f.count, s1, s2, f.gamma, f.beta, f.eps, f.momentum, f.rmean,
                              f.rvar, f.ss, f.mi, f.conv_bias);
        }
      }
    }
  }
}

static int mlp_grid(int R, int brows) {
  const int tiles = (R + brows - 1) / brows;
  const int cap = sw().gemm_grid;   // persistent: two 256-thread blocks per CU (256 * 2)
  return tiles < cap ? (tiles > 0 ? tiles : 1) : cap;
}

template <int PRO, bool STATS, bool POOL, bool RED, int CM>
static int launch_gemm_t(const MlpArgs& a, hipStream_t s);

template <int PRO, bool STATS, bool POOL = false, bool RED = false>
static int launch_gemm(const MlpArgs& a, hipStream_t s) {
  switch (compute_mode()) {
    case 1: return launch_gemm_t<PRO, STATS, POOL, RED, 1>(a, s);
    case 2: {
      // A/B switch: DEMF_X3_MASK bit 0 = forward launches, bit 1 = input-gradient, bit 2 = weight-gradient
      if (sw().x3_mask & (PRO >= PRO_DY_DENSE ? 2 : 1)) return launch_gemm_t<PRO, STATS, POOL, RED, 2>(a, s);
      return launch_gemm_t<PRO, STATS, POOL, RED, 0>(a, s);
    }
    default: return launch_gemm_t<PRO, STATS, POOL, RED, 0>(a, s);
  }
}

// The forms in the order they are tried: the first whose condition holds runs the launch (a tile form that cannot
// reserve its LDS passes it on).  BF16 = compute mode of the launch (0 fp32 MFMA, 1 bf16, 2 fp32 as bf16 terms).
template <int PRO, bool STATS, bool POOL, bool RED, int BF16>
static int launch_gemm_t(const MlpArgs& a, hipStream_t s) {
  if constexpr ((BF16 == 1 || BF16 == 2) && !RED && STATS && PRO == PRO_BNRELU) {
    // producer / consumer forward for 128-channel inputs (csrc/mlp_fwd_pc.hip): SA2-4 and the vote aggregation
    if (fwd_pc_takes(a, POOL)) {
      const int rc = launch_fwd_pc(a, BF16, POOL, s);
      if (rc == DEMF_OK) set_last_form(DEMF_FORM_PC);
      return rc;
    }
    // weight-resident, barrier-free forward (csrc/mlp_fwd_res.hip): 64-channel inputs, N = 64 / 128
    if (fwd_res_takes(a, POOL)) {
      const int rc = launch_fwd_res(a, BF16, POOL, s);
      if (rc == DEMF_OK) set_last_form(DEMF_FORM_RES);
      return rc;
    }
  }
  if (a.st != 0) {
    set_error("mlp_gemm: bf16 row storage (st=%d) is only built into the weight-resident forward (K = 64, "
              "N = 64 / 128, R >= 16384, bf16 compute mode)", a.st);
    return DEMF_EUNSUPPORTED;
  }
  if constexpr ((BF16 == 1 || BF16 == 2) && !POOL && !STATS && (PRO == PRO_DY_DENSE || PRO == PRO_DY_SPARSE)) {
    // few-row input-gradient launches on the tile kernel (csrc/mlp_tile.hip); A/B switch DEMF_DX_TILE
    constexpr bool SP = PRO == PRO_DY_SPARSE;
    if (dx_tile_takes(a, SP, RED)) {
      const int rc = launch_dx_tile(a, BF16, SP, RED, s);
      if (rc != LAUNCH_TRY_NEXT) { set_last_form(DEMF_FORM_TILE); return rc; }
    }
  }
  if constexpr ((BF16 == 1 || BF16 == 2) && !RED && !POOL && STATS && (PRO == PRO_BNRELU || PRO == PRO_NONE)) {
    // few-row forward layers on the 64 x 64 tile kernel (csrc/mlp_tile.hip); A/B switch DEMF_FWD_TILE
    // (measured, tools/fewrow_fwd_micro.py: 4 096 x 512 -> 256 26.3 -> 17.3 us, 8 192 x 512 -> 256 33.3 -> 23.7,
    // 2 048 x 256 -> 128 14.3 -> 10.2; at 32 768 rows mlp_gemm_kernel's 128-row tiles are level again: 43.6 vs 45.6)
    if (fwd_tile_takes(a, PRO == PRO_BNRELU)) {
      const int rc = launch_fwd_tile(a, BF16, PRO == PRO_BNRELU, s);
      if (rc != LAUNCH_TRY_NEXT) { set_last_form(DEMF_FORM_TILE); return rc; }
    }
  }
  // generic form: mlp_gemm_kernel
  set_last_form(DEMF_FORM_GENERIC);
  const dim3 block(256);
  // Two 32-row tiles per wave (256-row block tiles) while the accumulators + the raw prefetch fit
  // in 256 VGPRs: up to 4 column tiles for the forward prologues, up to 2 for the backward ones
  // (whose raw prefetch is 2-3x wider).  Backward launches are limited to 128 columns.
  // Launches with few rows (FP / vote / head layers: 4-8 k rows) would fill only a few CUs with
  // full-width tiles, so their columns are split over blockIdx.y (A is re-read; it is tiny).
  constexpr int RT2_MAX = PRO >= PRO_DY_DENSE ? 2 : 4;
  constexpr int NT_MAX = PRO >= PRO_DY_DENSE ? 4 : 8;
  const int nt = (a.N + 31) / 32;
  // (non-pooled launches wider than NT_MAX column tiles split their columns over blockIdx.y below)
  if (nt < 1 || nt > (POOL ? NT_MAX : 16)) {
    set_error("mlp_gemm: N=%d unsupported for this prologue (max %d columns per launch)", a.N,
              (POOL ? NT_MAX : 16) * 32);
    return DEMF_EUNSUPPORTED;
  }
  if constexpr (POOL) {
    // pooled epilogue: 64-row wave tiles for ns = 64 (a group must live in one wave), 32-row ones
    // otherwise; at most 2 (resp. 4) column tiles per block so that the accumulators, the
    // prefetch and the epilogue's temporaries fit in 256 VGPRs - wider outputs go to blockIdx.y
    // ns = 64: 64-row wave tiles x <= 2 column tiles (column halves co-scheduled), or - when all the
    // columns fit 4 tiles - 32-row wave tiles x 4 column tiles with the group merged across a wave pair
    const bool half64 = a.ns == 64 && nt <= 4 && !sw().pool_halves;
    const bool rt2 = a.ns == 64 && !half64;
    const int ntl = rt2 ? (nt < 2 ? nt : 2) : (nt < 4 ? nt : 4);
    const int ys = (nt + ntl - 1) / ntl;
    int gx = mlp_grid(a.R, rt2 ? 256 : 128);
    MlpArgs a2 = a;
    dim3 grid(gx, ys);
    if (ys == 2) {                       // interleaved halves: multiple of 16 blocks
      gx = ((gx + 7) / 8) * 8;
      a2.halves = 2;
      grid = dim3(2 * gx, 1);
    }
    // persistent pooled launches take their tiles dynamically too (not the interleaved-halves form,
    // whose block -> (tile, half) mapping is static)
    {
      const int brows = rt2 ? 256 : 128;
      const int tiles = (a.R + brows - 1) / brows;
      if (sw().pool_dyn && ys == 1 && tiles > gx && a.K > MLP_BK && gx % (8 * SCHED_GROUPS) == 0)
        a2.sched = sched_slot();
    }
    // SEL: only the extremum the sign of gamma selects (pmin / amin not given, gamma known)
    const bool sel = a.pmin == nullptr && a.fin.gamma != nullptr;
#define PGO(NTv, RTv)                                                                                       \
    do {                                                                                                    \
      if (sel) hipLaunchKernelGGL((mlp_gemm_kernel<NTv, RTv, PRO, STATS, true, false, false, BF16, true>), grid, block, 0, s, a2); \
      else hipLaunchKernelGGL((mlp_gemm_kernel<NTv, RTv, PRO, STATS, true, false, false, BF16>), grid, block, 0, s, a2);           \
    } while (0)
    if (rt2) { if (ntl == 1) PGO(1, 2); else PGO(2, 2); }
    else if (ntl == 1) PGO(1, 1);
    else if (ntl == 2) PGO(2, 1);
    else if (ntl == 3) PGO(3, 1);
    else PGO(4, 1);
#undef PGO
    return check_launch("mlp_gemm_pool");
  } else {
  const int tiles1 = (a.R + 127) / 128;
  // (three-term mode: more than 4 column tiles per block would not leave LDS for two blocks per CU -
  // the columns go to blockIdx.y instead of the launch falling back to the fp32 MFMA)
  if ((tiles1 < 192 && nt > 1) || nt > NT_MAX || (BF16 == 2 && nt > 4 && sw().x3_wide_split)) {
    int ysplit = (sw().split_target + tiles1 - 1) / tiles1;   // (the blocks the column split aims at)
    if (ysplit < (nt + 3) / 4) ysplit = (nt + 3) / 4;     // at most 4 column tiles per block
    if (ysplit > nt) ysplit = nt;
    const int ntl = (nt + ysplit - 1) / ysplit;          // column tiles per block
    const dim3 grid(tiles1, (nt + ntl - 1) / ntl);
    switch (ntl) {
#define SPLIT(NTv)                                                                              \
      case NTv: hipLaunchKernelGGL((mlp_gemm_kernel<NTv, 1, PRO, STATS, POOL, false, RED, BF16>), grid, block, 0, s, a); break;
      SPLIT(1) SPLIT(2) SPLIT(3) SPLIT(4)
#undef SPLIT
      default: break;
    }
    if (ntl <= 4) return check_launch("mlp_gemm");
  }
#define GO(NTv, RTv)                                                                            \
  do {                                                                                          \
    MlpArgs a3 = a;                                                                             \
    const int gxv = mlp_grid(a.R, 128 * RTv);                                                   \
    const int tilesv = (a.R + 128 * RTv - 1) / (128 * RTv);                                     \
    if (tilesv > gxv && a.K > MLP_BK && gxv % (8 * SCHED_GROUPS) == 0) a3.sched = sched_slot();                                \
    hipLaunchKernelGGL((mlp_gemm_kernel<NTv, RTv, PRO, STATS, POOL, false, RED, BF16>), dim3(gxv), block, 0, s, a3); \
  } while (0)
#define CASE(NTv)                                                                               \
  case NTv:                                                                                     \
    if constexpr (NTv <= NT_MAX && (BF16 != 2 || NTv <= 4)) {                                   \
      if constexpr (NTv <= RT2_MAX && !RED) GO(NTv, 2); else GO(NTv, 1);                        \
    }                                                                                           \
    break;
  // the split Bt slab of more than 4 column tiles would not leave room for two blocks per CU
  if constexpr (BF16 == 2) {
    if (nt > 4) return launch_gemm_t<PRO, STATS, POOL, RED, 0>(a, s);
  }
  switch (nt) {
    CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
  }
#undef CASE
#undef GO
  return check_launch("mlp_gemm");
  }
}

static int mlp_check(int R, int K, int N, int ldx) {
  DEMF_REQUIRE(R >= 0 && K >= 4 && K % 4 == 0 && K <= MLP_MAXK && N >= 1 && N <= 256 && ldx >= K &&
                   ldx % 4 == 0,
               "mlp: bad sizes R=%d K=%d N=%d ldx=%d (K%%4==0, K<=512, 1<=N<=256)", R, K, N, ldx);
  return DEMF_OK;
}

}  // namespace demf

using namespace demf;


extern "C" int demf_mlp_gemm_fwd(int R, int K, int N, int ldx, const float* X,
                                 const float* pro_scale_shift, const float* Wt, float* Y,
                                 double* stats, demf_stream_t stream) {
  if (int e = mlp_check(R, K, N, ldx)) return e;
  if (R == 0) return DEMF_OK;
  DEMF_REQUIRE(X && Wt && Y, "mlp_gemm_fwd: null pointer");
  MlpArgs a{};
  a.R = R; a.K = K; a.N = N; a.ldx = ldx; a.ldy = N; a.X = X; a.vec = pro_scale_shift; a.Bt = Wt;
  a.Y = Y; a.stats = stats;
  hipStream_t s = (hipStream_t)stream;
  if (pro_scale_shift)
    return stats ? launch_gemm<PRO_BNRELU, true>(a, s) : launch_gemm<PRO_BNRELU, false>(a, s);
  return stats ? launch_gemm<PRO_NONE, true>(a, s) : launch_gemm<PRO_NONE, false>(a, s);
}

// Same GEMM with the fused max-pool epilogue (last layer of a PointSAModule stack): besides Y
// and the statistics it emits, per group of ns rows and column, max / min of the raw output and
// their row offsets.  Supported: ns 16 / 32 / 64; anything else returns DEMF_EUNSUPPORTED (callers
// then run demf_bnrelu_maxpool_fwd on Y).
extern "C" int demf_mlp_gemm_fwd_pool(int R, int K, int N, int ldx, const float* X,
                                      const float* pro_scale_shift, const float* Wt, float* Y,
                                      double* stats, int ns, float* pmax, float* pmin, int* amax,
                                      int* amin, demf_stream_t stream) {
  if (int e = mlp_check(R, K, N, ldx)) return e;
  const bool ok = (ns == 16 || ns == 32 || ns == 64) && R % ns == 0;
  if (!ok) {
    set_error("mlp_gemm_fwd_pool: ns=%d with R=%d N=%d is not fused", ns, R, N);
    return DEMF_EUNSUPPORTED;
  }
  if (R == 0) return DEMF_OK;
  DEMF_REQUIRE(X && Wt && Y && pro_scale_shift && stats && pmax && pmin && amax && amin,
               "mlp_gemm_fwd_pool: null pointer");
  MlpArgs a{};
  a.R = R; a.K = K; a.N = N; a.ldx = ldx; a.ldy = N; a.X = X; a.vec = pro_scale_shift; a.Bt = Wt;
  a.Y = Y; a.stats = stats; a.ns = ns; a.pmax = pmax; a.pmin = pmin; a.amax = amax; a.amin = amin;
  return launch_gemm<PRO_BNRELU, true, true>(a, (hipStream_t)stream);
}

// forward launch + train-mode BN bookkeeping: in the kernel's last workgroup when a counter set is
// available, as a separate launch otherwise (DEMF_STATIC_TILES=1, DEMF_NO_FIN=1)
template <typename Launch>
static int launch_with_finalize(MlpArgs& a, BnFin fin, Launch launch, hipStream_t s) {
  fin.ticket = sw().no_fin ? nullptr : sched_slot();
  // (replicated accumulators: measured neutral on the forward launches - their workgroups do not end together (the
  //  persistent SA kernels) or the 8 x 2N exchanges of the finalize cost what the shorter queue saves (the 64 x 64-tile
  //  kernel) - so off unless DEMF_ACC_REPL_FWD=1; the row-reduction kernels of the BN backward gain 2-5 us each)
  fin.racc = fin.ticket != nullptr && a.N <= ACC_MAX_N && sw().acc_repl_fwd ? accum_slot() : nullptr;
  a.fin = fin;
  if (fin.ticket != nullptr) return launch(a);
  a.fin.ss = nullptr;                     // (gamma stays: the pooled epilogue selects by its sign)
  if (int e = launch(a)) return e;
  return launch_bn_finalize(a.N, a.stats, fin, s);     // csrc/bn.hip
}

static int fin_check(long long count, const float* gamma, const float* beta, const float* ss,
                     const float* mi, const double* stats) {
  DEMF_REQUIRE(count >= 1 && gamma && beta && ss && mi && stats, "mlp_gemm_fwd_bn: bad BN arguments");
  return DEMF_OK;
}

static int mlp_gemm_fwd_bn_impl(int R, int K, int N, int ldx, const float* X,
                                const float* pro_scale_shift, const float* Wt, float* Y,
                                double* stats, const float* gamma, const float* beta, float eps,
                                float momentum, float* running_mean, float* running_var,
                                long long* num_batches_tracked, float* scale_shift,
                                float* mean_invstd, const float* conv_bias, int st, demf_stream_t stream) {
  if (int e = mlp_check(R, K, N, ldx)) return e;
  DEMF_REQUIRE(R >= 1 && X && Wt && Y, "mlp_gemm_fwd_bn: null pointer / no rows");
  if (int e = fin_check(R, gamma, beta, scale_shift, mean_invstd, stats)) return e;
  MlpArgs a{};
  a.R = R; a.K = K; a.N = N; a.ldx = ldx; a.ldy = N; a.X = X; a.vec = pro_scale_shift; a.Bt = Wt;
  a.Y = Y; a.stats = stats; a.st = st;
  hipStream_t s = (hipStream_t)stream;
  BnFin fin{(double)R, gamma, beta, conv_bias, eps, momentum, running_mean, running_var,
            num_batches_tracked, scale_shift, mean_invstd, nullptr};
  if (pro_scale_shift)
    return launch_with_finalize(a, fin, [s](const MlpArgs& b) { return launch_gemm<PRO_BNRELU, true>(b, s); }, s);
  return launch_with_finalize(a, fin, [s](const MlpArgs& b) { return launch_gemm<PRO_NONE, true>(b, s); }, s);
}

extern "C" int demf_mlp_gemm_fwd_bn(int R, int K, int N, int ldx, const float* X,
                                    const float* pro_scale_shift, const float* Wt, float* Y,
                                    double* stats, const float* gamma, const float* beta, float eps,
                                    float momentum, float* running_mean, float* running_var,
                                    long long* num_batches_tracked, float* scale_shift,
                                    float* mean_invstd, const float* conv_bias, demf_stream_t stream) {
  return mlp_gemm_fwd_bn_impl(R, K, N, ldx, X, pro_scale_shift, Wt, Y, stats, gamma, beta, eps, momentum,
                              running_mean, running_var, num_batches_tracked, scale_shift, mean_invstd,
                              conv_bias, 0, stream);
}

// Same with the rows stored as bf16 in HBM (store_flags bit 0: X is bf16, bit 1: Y is bf16; X / Y then
// point to 2-byte elements, ldx still counts elements).  bf16 compute mode, weight-resident forward only
// (K = 64, N = 64 / 128, R >= 16384): DEMF_EUNSUPPORTED otherwise.  BASELINE configs[3].
extern "C" int demf_mlp_gemm_fwd_bn_st(int R, int K, int N, int ldx, const void* X,
                                       const float* pro_scale_shift, const float* Wt, void* Y,
                                       double* stats, const float* gamma, const float* beta, float eps,
                                       float momentum, float* running_mean, float* running_var,
                                       long long* num_batches_tracked, float* scale_shift,
                                       float* mean_invstd, const float* conv_bias, int store_flags,
                                       demf_stream_t stream) {
  DEMF_REQUIRE(store_flags >= 1 && store_flags <= 3 && pro_scale_shift, "mlp_gemm_fwd_bn_st: store_flags in 1..3, BN prologue");
  return mlp_gemm_fwd_bn_impl(R, K, N, ldx, (const float*)X, pro_scale_shift, Wt, (float*)Y, stats, gamma, beta,
                              eps, momentum, running_mean, running_var, num_batches_tracked, scale_shift,
                              mean_invstd, conv_bias, store_flags, stream);
}

static int mlp_gemm_fwd_pool_bn_impl(int R, int K, int N, int ldx, const float* X,
                                     const float* pro_scale_shift, const float* Wt, float* Y,
                                     double* stats, int ns, float* pmax, float* pmin, int* amax,
                                     int* amin, const float* gamma, const float* beta, float eps,
                                     float momentum, float* running_mean, float* running_var,
                                     long long* num_batches_tracked, float* scale_shift,
                                     float* mean_invstd, const float* conv_bias, int st,
                                     demf_stream_t stream) {
  if (int e = mlp_check(R, K, N, ldx)) return e;
  const bool ok = (ns == 16 || ns == 32 || ns == 64) && R % ns == 0 && R >= 1;
  if (!ok) {
    set_error("mlp_gemm_fwd_pool_bn: ns=%d with R=%d N=%d is not fused", ns, R, N);
    return DEMF_EUNSUPPORTED;
  }
  DEMF_REQUIRE(X && Wt && (Y || st == 4) && pro_scale_shift && pmax && amax && (pmin == nullptr) == (amin == nullptr),
               "mlp_gemm_fwd_pool_bn: null pointer");
  if (int e = fin_check(R, gamma, beta, scale_shift, mean_invstd, stats)) return e;
  MlpArgs a{};
  a.R = R; a.K = K; a.N = N; a.ldx = ldx; a.ldy = N; a.X = X; a.vec = pro_scale_shift; a.Bt = Wt;
  a.Y = Y; a.stats = stats; a.ns = ns; a.pmax = pmax; a.pmin = pmin; a.amax = amax; a.amin = amin;
  a.st = st;
  hipStream_t s = (hipStream_t)stream;
  BnFin fin{(double)R, gamma, beta, conv_bias, eps, momentum, running_mean, running_var,
            num_batches_tracked, scale_shift, mean_invstd, nullptr};
  return launch_with_finalize(a, fin, [s](const MlpArgs& b) { return launch_gemm<PRO_BNRELU, true, true>(b, s); }, s);
}

extern "C" int demf_mlp_gemm_fwd_pool_bn(int R, int K, int N, int ldx, const float* X,
                                         const float* pro_scale_shift, const float* Wt, float* Y,
                                         double* stats, int ns, float* pmax, float* pmin, int* amax,
                                         int* amin, const float* gamma, const float* beta, float eps,
                                         float momentum, float* running_mean, float* running_var,
                                         long long* num_batches_tracked, float* scale_shift,
                                         float* mean_invstd, const float* conv_bias,
                                         demf_stream_t stream) {
  return mlp_gemm_fwd_pool_bn_impl(R, K, N, ldx, X, pro_scale_shift, Wt, Y, stats, ns, pmax, pmin, amax, amin,
                                   gamma, beta, eps, momentum, running_mean, running_var,
                                   num_batches_tracked, scale_shift, mean_invstd, conv_bias, 0, stream);
}

// Pooled form with bf16 row storage (see demf_mlp_gemm_fwd_bn_st); pmin / amin must be NULL.
extern "C" int demf_mlp_gemm_fwd_pool_bn_st(int R, int K, int N, int ldx, const void* X,
                                            const float* pro_scale_shift, const float* Wt, void* Y,
                                            double* stats, int ns, float* pmax, int* amax,
                                            const float* gamma, const float* beta, float eps,
                                            float momentum, float* running_mean, float* running_var,
                                            long long* num_batches_tracked, float* scale_shift,
                                            float* mean_invstd, const float* conv_bias, int store_flags,
                                            demf_stream_t stream) {
  DEMF_REQUIRE(store_flags >= 1 && store_flags <= 4, "mlp_gemm_fwd_pool_bn_st: store_flags in 1..4");
  return mlp_gemm_fwd_pool_bn_impl(R, K, N, ldx, (const float*)X, pro_scale_shift, Wt, (float*)Y, stats, ns,
                                   pmax, nullptr, amax, nullptr, gamma, beta, eps, momentum, running_mean,
                                   running_var, num_batches_tracked, scale_shift, mean_invstd, conv_bias,
                                   store_flags, stream);
}

// ---- first layer of an SA1-shaped stack (4-float rows -> N0 channels) WITHOUT its output -----------------
// y = x.W0^T is linear in a 4-float row: the train-mode BN statistics of all N0 channels follow from the 14
// second moments of x alone,  sum y_c = w_c . sum x,   sum y_c^2 = w_c^T (sum x x^T) w_c,  taken in one pass
// over the 16-byte rows (fp32 per thread, fp64 across threads); the last workgroup turns them into
// scale / shift, mean / invstd and the running statistics (bn_finalize_channel).  The 268 MB of raw
// outputs the GEMM kernel wrote for the consumers are recomputed by them from the rows (ST bit 3 of
// mlp_fwd_res_kernel, mlp_bwd_fused_kernel).  bf16 mode: moments of the bf16-rounded rows, rounded weights.
__global__ __launch_bounds__(256) void mlp_first_stats_k(int R, int N0, const float* __restrict__ X,
                                                         const float* __restrict__ W0, double* __restrict__ mom,
                                                         BnFin fin, int bf16) {
  float m[14];
#pragma unroll
  for (int i = 0; i < 14; ++i) m[i] = 0.f;
  double acc[14];
#pragma unroll
  for (int i = 0; i < 14; ++i) acc[i] = 0.0;
  int n = 0;
  for (int r = blockIdx.x * 256 + threadIdx.x; r < R; r += gridDim.x * 256) {
    float4 x = *reinterpret_cast<const float4*>(X + (size_t)r * 4);
    if (bf16) { x.x = (float)(__bf16)x.x; x.y = (float)(__bf16)x.y; x.z = (float)(__bf16)x.z; x.w = (float)(__bf16)x.w; }
    const float v[4] = {x.x, x.y, x.z, x.w};
    int t = 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      m[i] += v[i];
#pragma unroll
      for (int j = i; j < 4; ++j) { m[t] = __builtin_fmaf(v[i], v[j], m[t]); ++t; }
    }
    if (++n == 64) {                       // fp32 partial sums of at most 64 rows, then fp64
#pragma unroll
      for (int i = 0; i < 14; ++i) { acc[i] += (double)m[i]; m[i] = 0.f; }
      n = 0;
    }
  }
#pragma unroll
  for (int i = 0; i < 14; ++i) acc[i] += (double)m[i];
  __shared__ double s_m[4][14];
  __shared__ int s_last;
#pragma unroll
  for (int i = 0; i < 14; ++i) {
    double v = acc[i];
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < 14)
    atomicAdd(mom + threadIdx.x, (s_m[0][threadIdx.x] + s_m[1][threadIdx.x]) + (s_m[2][threadIdx.x] + s_m[3][threadIdx.x]));
  sync_drained();
  if (threadIdx.x == 0) s_last = last_workgroup(fin.ticket, (int)gridDim.x, (int)blockIdx.x);
  __syncthreads();
  if (!s_last) return;
  __shared__ double s_t[14];
  if (threadIdx.x < 14)
    s_t[threadIdx.x] = __builtin_bit_cast(double, atomicExch(reinterpret_cast<unsigned long long*>(mom + threadIdx.x), 0ull));
  __syncthreads();
  if (threadIdx.x == 0 && fin.nbt != nullptr) *fin.nbt += 1;
  for (int c = threadIdx.x; c < N0; c += 256) {
    double w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float wk = W0[c * 4 + k];
      w[k] = bf16 ? (double)(float)(__bf16)wk : (double)wk;
    }
    double s1 = 0.0, s2 = 0.0;
    int t = 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      s1 += w[i] * s_t[i];
#pragma unroll
      for (int j = i; j < 4; ++j) { s2 += (i == j ? 1.0 : 2.0) * w[i] * w[j] * s_t[t]; ++t; }
    }
    bn_finalize_channel(c, N0, fin.count, s1, s2, fin.gamma, fin.beta, fin.eps, fin.momentum, fin.rmean, fin.rvar,
                        fin.ss, fin.mi, fin.conv_bias);
  }
}

// First layer of an SA1-shaped stack without its output: BN statistics + bookkeeping from the 4-float rows
// alone (mlp_first_stats_k).  ``moments``: >= 14 doubles of a zeroed accumulator, left zeroed.
extern "C" int demf_mlp_first_stats(int R, int N0, const float* X, const float* W0, double* moments,
                                    const float* gamma, const float* beta, float eps, float momentum,
                                    float* running_mean, float* running_var, long long* num_batches_tracked,
                                    float* scale_shift, float* mean_invstd, const float* conv_bias,
                                    demf_stream_t stream) {
  DEMF_REQUIRE(R >= 1 && N0 >= 1 && X && W0 && moments, "mlp_first_stats: bad arguments");
  if (int e = fin_check(R, gamma, beta, scale_shift, mean_invstd, moments)) return e;
  BnFin fin{(double)R, gamma, beta, conv_bias, eps, momentum, running_mean, running_var,
            num_batches_tracked, scale_shift, mean_invstd, sched_slot()};
  DEMF_REQUIRE(fin.ticket != nullptr, "mlp_first_stats: needs the counter ring (DEMF_STATIC_TILES=1 is set)");
  int grid = cdiv(R, 256 * 16);
  if (grid > 256) grid = 256;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(mlp_first_stats_k, dim3(grid), dim3(256), 0, (hipStream_t)stream, R, N0, X, W0, moments, fin,
                     compute_mode() == 1 ? 1 : 0);
  return check_launch("mlp_first_stats");
}

// Second layer of that stack (K = 64 -> N = 64): demf_mlp_gemm_fwd_bn with the prologue's input rebuilt from the
// 4-float rows X4 and the first layer's weight W0 (64 x 4) instead of loaded from a stored (R x 64) output;
// prev_scale_shift = the first layer's [scale|shift] from demf_mlp_first_stats.  Modes 1 / 2, R >= 16384.
extern "C" int demf_mlp_gemm_fwd_bn_x4(int R, int N, const float* X4, const float* W0,
                                       const float* prev_scale_shift, const float* Wt, float* Y, double* stats,
                                       const float* gamma, const float* beta, float eps, float momentum,
                                       float* running_mean, float* running_var, long long* num_batches_tracked,
                                       float* scale_shift, float* mean_invstd, const float* conv_bias,
                                       demf_stream_t stream) {
  const int cm = compute_mode();
  DEMF_REQUIRE((cm == 1 || cm == 2) && N == 64 && R >= 64 * 256 && X4 && W0 && prev_scale_shift && Wt && Y,
               "mlp_gemm_fwd_bn_x4: unsupported shape / mode R=%d N=%d mode=%d (or null pointer)", R, N, cm);
  if (int e = fin_check(R, gamma, beta, scale_shift, mean_invstd, stats)) return e;
  MlpArgs a{};
  a.R = R; a.K = 64; a.N = N; a.ldx = 4; a.ldy = N; a.X = X4; a.W0 = W0; a.vec = prev_scale_shift; a.Bt = Wt;
  a.Y = Y; a.stats = stats; a.st = 8;
  hipStream_t s = (hipStream_t)stream;
  BnFin fin{(double)R, gamma, beta, conv_bias, eps, momentum, running_mean, running_var,
            num_batches_tracked, scale_shift, mean_invstd, nullptr};
  return launch_with_finalize(a, fin, [s](const MlpArgs& b) { return launch_gemm<PRO_BNRELU, true>(b, s); }, s);
}

// dX(R x K) = dY(R x N) @ W(N x K), dY formed on the fly.  Wtt = W^T as (K x N) row-major.
// dX has row stride ldo >= K; K may be any multiple of 4 (handled in chunks of <= 128 columns).
struct DxReduce {            // optional: layer l-1 operands for the RED epilogue
  const float* Yprev;        // (R x K) pre-BN output of layer l-1
  const float* ss;           // [scale|shift] (2K)
  const float* mi;           // [mean|invstd] (2K)
  double* g12;               // (2K) accumulated
  const float* gamma = nullptr;   // + layer l-1's backward vectors by the last workgroup when given
  float* vec6 = nullptr;
  float* dgamma = nullptr;
  float* dbeta = nullptr;
};

static int mlp_bwd_dx_impl(bool w_direct, int R, int N, int K, int ldo, const float* G, const float* dP,
                           const int* arg, int ns, const float* Y, const float* vec6,
                           const float* Wtt, float* dX, const DxReduce* red, demf_stream_t stream) {
  DEMF_REQUIRE(R >= 0 && N >= 4 && N % 4 == 0 && K >= 1 && ldo >= K,
               "mlp_gemm_bwd_dx: bad sizes R=%d N=%d K=%d ldo=%d", R, N, K, ldo);
  if (R == 0) return DEMF_OK;
  DEMF_REQUIRE(Y && vec6 && Wtt && dX && (G || (dP && arg && ns >= 1)), "mlp_gemm_bwd_dx: null pointer");
  hipStream_t s = (hipStream_t)stream;
  // Outputs wider than 128 columns: ONE launch whose column tiles are split over blockIdx.y (every
  // block rebuilds its dY row tile, as the per-chunk launches did, but the chunks now run side by side
  // instead of as 2-4 dependent launches of one block per CU each); DEMF_DX_CHUNKS=1: chunk launches.
  const int cstep = (!sw().dx_chunks && K <= 512) ? K : 128;
  for (int c0 = 0; c0 < K; c0 += cstep) {
    // here the reduction runs over this layer's N channels and the output has K columns
    MlpArgs a{};
    a.R = R; a.K = N; a.N = (K - c0) < cstep ? (K - c0) : cstep; a.ldx = N; a.ldy = ldo; a.X = Y;
    a.G = G; a.dP = dP; a.arg = arg; a.ns = ns; a.vec = vec6;
    if (w_direct) { a.Bt = Wtt + c0; a.ldb = K; }      // Wtt is W (N x K) itself: columns c0.. of it
    else a.Bt = Wtt + (size_t)c0 * N;
    a.Y = dX + c0; a.stats = nullptr;
    int e;
    if (red) {
      a.fY = red->Yprev; a.fss = red->ss; a.fmi = red->mi; a.stats = red->g12; a.fld = K; a.fc0 = c0;
      if (red->gamma != nullptr)
        a.vfin = BnVecFin{(double)R, red->gamma, red->ss, red->mi, red->vec6, red->dgamma, red->dbeta, sched_slot(),
                          nullptr};
      if (a.vfin.ticket != nullptr && K <= ACC_MAX_N && sw().acc_repl_red) a.vfin.racc = accum_slot();
      e = G ? launch_gemm<PRO_DY_DENSE, false, false, true>(a, s)
            : launch_gemm<PRO_DY_SPARSE, false, false, true>(a, s);
    } else {
      e = G ? launch_gemm<PRO_DY_DENSE, false>(a, s) : launch_gemm<PRO_DY_SPARSE, false>(a, s);
    }
    if (e) return e;
  }
  if (red && red->gamma != nullptr && sw().static_tiles)
    // no counter ring, no last-workgroup ticket: the vectors of layer l-1 as a launch of their own (all K channels)
    return demf_bn_bwd_vectors(K, (long long)R, red->g12, red->gamma, red->ss, red->mi, red->vec6, red->dgamma,
                               red->dbeta, stream);
  return DEMF_OK;
}

extern "C" int demf_mlp_gemm_bwd_dx(int R, int N, int K, int ldo, const float* G, const float* dP,
                                    const int* arg, int ns, const float* Y, const float* vec6,
                                    const float* Wtt, float* dX, demf_stream_t stream) {
  return mlp_bwd_dx_impl(false, R, N, K, ldo, G, dP, arg, ns, Y, vec6, Wtt, dX, nullptr, stream);
}

// Same, reading the layer's weight W (N x K row-major) directly: no transposed copy per step.
extern "C" int demf_mlp_gemm_bwd_dx_w(int R, int N, int K, int ldo, const float* G, const float* dP,
                                      const int* arg, int ns, const float* Y, const float* vec6,
                                      const float* W, float* dX, demf_stream_t stream) {
  return mlp_bwd_dx_impl(true, R, N, K, ldo, G, dP, arg, ns, Y, vec6, W, dX, nullptr, stream);
}

// Same + the BN-backward sums of layer l-1 (what demf_bn_bwd_reduce(R, K, G = dX, Yprev, ...) would
// add to g12_prev) taken from the output tiles on the way out: that pass over dX and Yprev is gone.
extern "C" int demf_mlp_gemm_bwd_dx_red(int R, int N, int K, int ldo, const float* G, const float* dP,
                                        const int* arg, int ns, const float* Y, const float* vec6,
                                        const float* W, float* dX, const float* Yprev,
                                        const float* scale_shift_prev, const float* mean_invstd_prev,
                                        double* g12_prev, demf_stream_t stream) {
  DEMF_REQUIRE(K % 4 == 0 && Yprev && scale_shift_prev && mean_invstd_prev && g12_prev,
               "mlp_gemm_bwd_dx_red: bad arguments (K %% 4 == 0)");
  const DxReduce red{Yprev, scale_shift_prev, mean_invstd_prev, g12_prev};
  return mlp_bwd_dx_impl(true, R, N, K, ldo, G, dP, arg, ns, Y, vec6, W, dX, &red, stream);
}

// Same + layer l-1's backward vectors (demf_bn_bwd_vectors on g12_prev) formed by the launch's last
// workgroup: vec6_prev (5K), dgamma_prev, dbeta_prev are complete and g12_prev is zeroed on return.
extern "C" int demf_mlp_gemm_bwd_dx_red_v(int R, int N, int K, int ldo, const float* G, const float* dP,
                                          const int* arg, int ns, const float* Y, const float* vec6,
                                          const float* W, float* dX, const float* Yprev,
                                          const float* scale_shift_prev, const float* mean_invstd_prev,
                                          double* g12_prev, const float* gamma_prev, float* vec6_prev,
                                          float* dgamma_prev, float* dbeta_prev, demf_stream_t stream) {
  DEMF_REQUIRE(K % 4 == 0 && Yprev && scale_shift_prev && mean_invstd_prev && g12_prev && gamma_prev &&
                   vec6_prev && dgamma_prev && dbeta_prev,
               "mlp_gemm_bwd_dx_red_v: bad arguments (K %% 4 == 0)");
  DxReduce red{Yprev, scale_shift_prev, mean_invstd_prev, g12_prev};
  red.gamma = gamma_prev; red.vec6 = vec6_prev; red.dgamma = dgamma_prev; red.dbeta = dbeta_prev;
  return mlp_bwd_dx_impl(true, R, N, K, ldo, G, dP, arg, ns, Y, vec6, W, dX, &red, stream);
}

// ---- first layer of a stack with a 4-float input and no input gradient (SA1) --------------------
// dY0 = gi*dZ0 + a*y0 + b is linear in (dZ0, y0, 1), so layer 0's whole backward follows from raw
// sums that do not depend on the BN-backward scalars: g1 = sum dZ0, g2 = sum dZ0*xhat,
// P = dZ0^T X, Q = y0^T X, cx = colsum(X).  The dx GEMM of layer 1 takes them from its output tile
// (FIRST epilogue) instead of storing the (R x N0) gradient, which is then never written nor read:
//   dW0 = gi*P + a*Q + b*cx^T,  dgamma0 = g2,  dbeta0 = g1.
__global__ void mlp_first_finish_k(int N, double count, double* __restrict__ sums,
                                   const float* __restrict__ gamma, const float* __restrict__ mi,
                                   float* __restrict__ dW, float* __restrict__ dgamma,
                                   float* __restrict__ dbeta) {
  __shared__ double s_cx[4];
  if (threadIdx.x < 4) s_cx[threadIdx.x] = sums[10 * N + threadIdx.x];
  __syncthreads();
  const int c = threadIdx.x;
  if (c < N) {
    const double g1 = sums[c], g2 = sums[N + c];
    const double mean = mi[c], is = mi[N + c];
    const double gi = (double)gamma[c] * is;
    const double a = -gi * is * (g2 / count);
    const double b = -gi * (g1 / count) - a * mean;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      dW[c * 4 + k] = (float)(gi * sums[2 * N + c * 4 + k] + a * sums[6 * N + c * 4 + k] + b * s_cx[k]);
      sums[2 * N + c * 4 + k] = 0.0;               // consumed: the accumulator is left zeroed
      sums[6 * N + c * 4 + k] = 0.0;
    }
    sums[c] = 0.0;
    sums[N + c] = 0.0;
    dgamma[c] = (float)g2;
    dbeta[c] = (float)g1;
  }
  if (threadIdx.x < 4) sums[10 * N + threadIdx.x] = 0.0;
}

extern "C" int demf_mlp_gemm_bwd_dx_first(int R, int N, int K0, const float* G, const float* Y1,
                                          const float* vec6, const float* W1, const float* X0,
                                          const float* Y0, const float* ss0, const float* mi0,
                                          double* sums, demf_stream_t stream) {
  DEMF_REQUIRE(R >= 1 && N >= 4 && N % 4 == 0 && N <= MLP_MAXK && K0 >= 4 && K0 % 4 == 0 && K0 <= 64,
               "mlp_gemm_bwd_dx_first: bad sizes R=%d N=%d K0=%d (K0 <= 64)", R, N, K0);
  DEMF_REQUIRE(G && Y1 && vec6 && W1 && X0 && Y0 && ss0 && mi0 && sums,
               "mlp_gemm_bwd_dx_first: null pointer");
  hipStream_t s = (hipStream_t)stream;
  MlpArgs a{};
  a.R = R; a.K = N; a.N = K0; a.ldx = N; a.ldy = K0; a.X = Y1; a.G = G; a.vec = vec6;
  a.Bt = W1; a.ldb = K0; a.Y = nullptr; a.stats = nullptr;
  a.fX = X0; a.fY = Y0; a.fss = ss0; a.fmi = mi0; a.fsum = sums; a.fld = K0; a.fc0 = 0;
  // 32-row wave tiles: with 64-row ones the staged half tile + the 24 running sums do not fit next
  // to the accumulators in 256 VGPRs
  const int gx = mlp_grid(R, 128);
  const int tiles = (R + 127) / 128;
  if (tiles > gx && a.K > MLP_BK && gx % (8 * SCHED_GROUPS) == 0) a.sched = sched_slot();
#define FIRSTGO(NTv, CMv) \
  hipLaunchKernelGGL((mlp_gemm_kernel<NTv, 1, PRO_DY_DENSE, false, false, true, false, CMv>), dim3(gx), dim3(256), 0, s, a)
  const int cm = compute_mode();
  if (K0 <= 32) {
    if (cm == 1) FIRSTGO(1, 1); else if (cm == 2) FIRSTGO(1, 2); else FIRSTGO(1, 0);
  } else {
    if (cm == 1) FIRSTGO(2, 1); else if (cm == 2) FIRSTGO(2, 2); else FIRSTGO(2, 0);
  }
#undef FIRSTGO
  return check_launch("mlp_gemm_bwd_dx_first");
}

extern "C" int demf_mlp_first_finish(int N0, long long count, double* sums, const float* gamma0,
                                     const float* mean_invstd0, float* dW0, float* dgamma0,
                                     float* dbeta0, demf_stream_t stream) {
  DEMF_REQUIRE(N0 >= 1 && N0 <= 64 && count >= 1 && sums && gamma0 && mean_invstd0 && dW0 && dgamma0 &&
                   dbeta0, "mlp_first_finish: bad arguments");
  hipLaunchKernelGGL(mlp_first_finish_k, dim3(1), dim3(64), 0, (hipStream_t)stream, N0, (double)count,
                     sums, gamma0, mean_invstd0, dW0, dgamma0, dbeta0);
  return check_launch("mlp_first_finish");
}

#ifdef DEMF_MLP_PROFILE
// phases of mlp_gemm_kernel's K loop: 0 wait at the first barrier, 1 transform + LDS writes, 2 second barrier,
// 3 prefetch issue, 4 MFMA section (LDS reads + split + MFMAs), 5 epilogue + bookkeeping; [15] = launches
extern "C" int demf_mlp_prof_read(long long* out16, int reset) {
  if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(demf::g_mlp_prof), 16 * sizeof(long long)) != hipSuccess) return -1;
  if (reset) {
    long long z[16] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(demf::g_mlp_prof), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
}
#endif
