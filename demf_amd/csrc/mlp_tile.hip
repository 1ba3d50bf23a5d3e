// Few-row shared-MLP launches on 64 x 64 output tiles: the forward layers of the FP modules, the vote module, the
// vote aggregation's second layer and the prediction heads (mlp_fwd_tile_kernel), and the input-gradient launches
// of the same layers (mlp_dx_tile_kernel).  The kernels, the conditions under which the dispatcher (launch_gemm_t,
// csrc/mlp.hip) hands a launch to them, and their launchers.
#include "mlp_args.h"

namespace demf {

// ---- few-row forward layers: 64 x 64 tiles, operands split ONCE at staging, double-buffered planes (round 6) ---------
// The FP modules, the vote module, the vote aggregation's second layer and the prediction heads run this file's
// forward GEMM on 2 048 ... 32 768 rows.  mlp_gemm_kernel walks a 32-column K step in ~4 200 cycles there (DESIGN_LOG
// section 3.2: the fp32 slab goes to LDS as it is and EVERY wave splits its own fragments, two barriers per step, 24
// MFMAs = 768 issue cycles): a 2 048 x 256 -> 128 layer is 8 dependent steps = 15 us for 0.07 GFLOP.  Here a
// workgroup of 4 waves owns a 64 x 64 output tile; per 32-wide K step every thread takes 8 consecutive k of one A
// row and of one W row (two float4 each, a full 128-byte line per 4 threads), applies the BN + ReLU prologue, splits
// them into the P bf16 planes and writes ONE 16-byte chunk per plane ([row][k] planes, XOR-swizzled chunks:
// fragment reads are conflict-free); the planes are double-buffered, so a step has ONE barrier, and the global rows
// of step i + 2 / i + 3 are in flight in registers.  A wave contracts 32 x 32 x 32 per step: 12 MFMAs (P = 3) on
// fragments read as ds_read_b128.  Epilogue: column statistics (fp64 atomics, one per column per workgroup), the raw
// output, the BatchNorm bookkeeping in the last workgroup.  Column tiles of a row block run on one XCD (A read once).
// (LDS chunk swizzle: swz, csrc/mfma.h)

template <int P>
__device__ __forceinline__ void ft_split8(const float4& a, const float4& b, uint4 (&o)[P]) {
  using v2f = float __attribute__((ext_vector_type(2)));
  using v2b = __bf16 __attribute__((ext_vector_type(2)));
  const v2f x[4] = {{a.x, a.y}, {a.z, a.w}, {b.x, b.y}, {b.z, b.w}};
  unsigned w[4][P];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const v2b h = __builtin_convertvector(x[i], v2b);
    w[i][0] = __builtin_bit_cast(unsigned, h);
    if constexpr (P == 3) {
      const v2f r = x[i] - __builtin_convertvector(h, v2f);
      const v2b m = __builtin_convertvector(r, v2b);
      w[i][1] = __builtin_bit_cast(unsigned, m);
      const v2f l = r - __builtin_convertvector(m, v2f);
      w[i][2] = __builtin_bit_cast(unsigned, __builtin_convertvector(l, v2b));
    }
  }
#pragma unroll
  for (int q = 0; q < P; ++q) o[q] = make_uint4(w[0][q], w[1][q], w[2][q], w[3][q]);
}

template <int P, bool PRO>
__global__ __launch_bounds__(256, 2) void mlp_fwd_tile_kernel(MlpArgs p) {
  constexpr int PLANE = 64 * 64;                    // bytes: 64 rows x 32 k bf16
  constexpr int BUF = 2 * P * PLANE;                // A planes | W planes of one K step
  extern __shared__ __attribute__((aligned(16))) char ft_smem[];
  char* s_buf = ft_smem;                            // [2][BUF]
  float* s_vec = reinterpret_cast<float*>(ft_smem + 2 * BUF);   // [scale | shift] of the prologue (2K)
  float* s_red = s_vec + (PRO ? 2 * p.K : 0);       // [2 waves][2 stats][64 columns]
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 31, lh = lane >> 5;
  const int wm = wave & 1, wn = wave >> 1;
  int bx = blockIdx.x, by = blockIdx.y;
  {
    // all column tiles of a row block on ONE XCD, back to back (workgroups are dealt to the 8 XCDs round-robin)
    const int gx = gridDim.x, gy = gridDim.y;
    if ((gy & 7) == 0) {
      const int L = bx + gx * by;
      by = (L & 7) + 8 * (L / (8 * gx));
      bx = (L >> 3) % gx;
    }
  }
  const int m0 = by * 64, n0 = bx * 64;
  if constexpr (PRO) {
    for (int i = tid; i < 2 * p.K; i += 256) s_vec[i] = p.vec[i];
  }
  // staging map: row (tid >> 2) of the tile, k chunk (tid & 3) = 8 consecutive k
  const int srow = tid >> 2, sch = tid & 3;
  const int arow = min(m0 + srow, p.R - 1);         // rows beyond R: a valid address, zeroed in the transform
  const bool arow_ok = m0 + srow < p.R;
  const float* ga = p.X + (size_t)arow * p.ldx + 8 * sch;
  const float* gw = p.Bt + (size_t)(n0 + srow) * p.K + 8 * sch;
  const int nk = p.K / 32;
  // Register ring of FOUR K steps: a row that the layer below has just written is ~2 us away (another XCD's L2
  // or HBM), a step is ~0.5 us - with two stages every step waited for its rows.  (Stages are addressed
  // statically - the K loop is unrolled by four - or they would live in scratch.)
  float4 ra0[2], rw0[2], ra1[2], rw1[2], ra2[2], rw2[2], ra3[2], rw3[2];
  auto fetch = [&](float4 (&a4)[2], float4 (&w4)[2], int ks) {
    const float* a = ga + 32 * ks;
    const float* w = gw + 32 * ks;
    a4[0] = *reinterpret_cast<const float4*>(a);
    a4[1] = *reinterpret_cast<const float4*>(a + 4);
    w4[0] = *reinterpret_cast<const float4*>(w);
    w4[1] = *reinterpret_cast<const float4*>(w + 4);
  };
  auto commit = [&](const float4 (&a4)[2], const float4 (&w4)[2], int ks, char* buf) {
    float4 a0 = a4[0], a1 = a4[1];
    if constexpr (PRO) {
      const float4 c0 = *reinterpret_cast<const float4*>(s_vec + 32 * ks + 8 * sch);
      const float4 c1 = *reinterpret_cast<const float4*>(s_vec + 32 * ks + 8 * sch + 4);
      const float4 h0 = *reinterpret_cast<const float4*>(s_vec + p.K + 32 * ks + 8 * sch);
      const float4 h1 = *reinterpret_cast<const float4*>(s_vec + p.K + 32 * ks + 8 * sch + 4);
      a0.x = fmaxf(0.f, __builtin_fmaf(a0.x, c0.x, h0.x)); a0.y = fmaxf(0.f, __builtin_fmaf(a0.y, c0.y, h0.y));
      a0.z = fmaxf(0.f, __builtin_fmaf(a0.z, c0.z, h0.z)); a0.w = fmaxf(0.f, __builtin_fmaf(a0.w, c0.w, h0.w));
      a1.x = fmaxf(0.f, __builtin_fmaf(a1.x, c1.x, h1.x)); a1.y = fmaxf(0.f, __builtin_fmaf(a1.y, c1.y, h1.y));
      a1.z = fmaxf(0.f, __builtin_fmaf(a1.z, c1.z, h1.z)); a1.w = fmaxf(0.f, __builtin_fmaf(a1.w, c1.w, h1.w));
    }
    if (!arow_ok) { a0 = make_float4(0.f, 0.f, 0.f, 0.f); a1 = a0; }
    uint4 pa[P], pw[P];
    ft_split8<P>(a0, a1, pa);
    ft_split8<P>(w4[0], w4[1], pw);
    const int off = swz(srow, sch);
#pragma unroll
    for (int q = 0; q < P; ++q) {
      *reinterpret_cast<uint4*>(buf + q * PLANE + off) = pa[q];
      *reinterpret_cast<uint4*>(buf + (P + q) * PLANE + off) = pw[q];
    }
  };
  f32x16 acc, acc2;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc[r] = 0.f; acc2[r] = 0.f; }
  fetch(ra0, rw0, 0);
  if (nk > 1) fetch(ra1, rw1, 1);
  if (nk > 2) fetch(ra2, rw2, 2);
  if (nk > 3) fetch(ra3, rw3, 3);
  __syncthreads();                                  // the prologue vectors
  commit(ra0, rw0, 0, s_buf);
  if (nk > 4) fetch(ra0, rw0, 4);
  __syncthreads();
  // one K step: fragments of step ks out of buffer `cur`, step ks + 1 (registers an / wn) into buffer `nxt`,
  // the rows of step ks + 5 requested into the registers just freed
  auto step = [&](int ks, const char* cur, char* nxt, float4 (&an)[2], float4 (&wn4)[2]) {
    bf16x8 fa[2][P], fb[2][P];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int q = 0; q < P; ++q) {
        fa[s2][q] = *reinterpret_cast<const bf16x8*>(cur + q * PLANE + swz(wm * 32 + lr, 2 * s2 + lh));
        fb[s2][q] = *reinterpret_cast<const bf16x8*>(cur + (P + q) * PLANE + swz(wn * 32 + lr, 2 * s2 + lh));
      }
    // two accumulators (one per 16-wide half of the step): consecutive MFMAs are independent, and the staging
    // arithmetic of the NEXT step (issued below) runs on the vector ALU underneath them
    if constexpr (P == 3) {   // the six products of weight >= 2^-16, smallest first (as every three-term kernel)
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0][2], fb[0][0], acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[1][2], fb[1][0], acc2, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0][0], fb[0][2], acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[1][0], fb[1][2], acc2, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0][1], fb[0][1], acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[1][1], fb[1][1], acc2, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0][1], fb[0][0], acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[1][1], fb[1][0], acc2, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0][0], fb[0][1], acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[1][0], fb[1][1], acc2, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0][0], fb[0][0], acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[1][0], fb[1][0], acc2, 0, 0, 0);
    } else {
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0][0], fb[0][0], acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[1][0], fb[1][0], acc2, 0, 0, 0);
    }
    if (ks + 1 < nk) {
      commit(an, wn4, ks + 1, nxt);
      if (ks + 5 < nk) fetch(an, wn4, ks + 5);
    }
    if constexpr (P == 3) {
      // interleave: one MFMA, then a group of vector-ALU instructions of the staging code
#pragma unroll
      for (int i = 0; i < 12; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 9, 0);
      }
    }
    lds_barrier();
  };
  for (int ks = 0; ks < nk; ks += 4) {
    step(ks, s_buf, s_buf + BUF, ra1, rw1);                       // step 4j: stages step 4j + 1 out of ring slot 1
    if (ks + 1 < nk) step(ks + 1, s_buf + BUF, s_buf, ra2, rw2);
    if (ks + 2 < nk) step(ks + 2, s_buf, s_buf + BUF, ra3, rw3);
    if (ks + 3 < nk) step(ks + 3, s_buf + BUF, s_buf, ra0, rw0);
  }
  // ---- epilogue: C layout of 32x32: col = lr, row = (r & 3) + 8 (r >> 2) + 4 lh
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] += acc2[r];
  const int n = n0 + wn * 32 + lr;
  float cs1 = 0.f, cs2 = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
    if (m < p.R) {
      p.Y[(size_t)m * p.ldy + n] = acc[r];
      cs1 += acc[r];
      cs2 = __builtin_fmaf(acc[r], acc[r], cs2);
    }
  }
  cs1 += __shfl_xor(cs1, 32);
  cs2 += __shfl_xor(cs2, 32);
  if (lh == 0) {
    s_red[(wm * 2 + 0) * 64 + wn * 32 + lr] = cs1;
    s_red[(wm * 2 + 1) * 64 + wn * 32 + lr] = cs2;
  }
  __syncthreads();
  if (tid < 128) {
    const int which = tid >> 6, c = tid & 63;
    const float v = s_red[(0 * 2 + which) * 64 + c] + s_red[(1 * 2 + which) * 64 + c];
    double* sdst = p.fin.racc != nullptr ? repl_copy(p.fin.racc, p.N, (int)blockIdx.y) : p.stats;
    atomicAdd(sdst + (size_t)which * p.N + n0 + c, (double)v);
    // EVERY wave that issued sum atomics drains them before the barrier in front of the ticket: the barrier itself
    // does not wait for another wave's vector-memory counter (workgroup-scope release omits vmcnt(0) outside
    // threadgroup-split mode), and wave 1 carries all of this workgroup's sum of squares - taken late, the last
    // workgroup would finalise without its own 64 rows (measured: a 1e-3 shift of every gradient below the layer in
    // one run out of six) and the stragglers would land in the accumulator the finalize has just left zeroed.
  }
  // BatchNorm bookkeeping by the last workgroup (atomics only: see mlp_gemm_kernel)
  sync_drained();
  if (tid == 0) {
    const int total = (int)(gridDim.x * gridDim.y);
    const int lin = (int)(blockIdx.y * gridDim.x + blockIdx.x);
    const int ngroups = total < SCHED_GROUPS ? total : SCHED_GROUPS;
    const int g = lin % SCHED_GROUPS;
    const int members = total / SCHED_GROUPS + (g < total % SCHED_GROUPS ? 1 : 0);
    int* t = p.fin.ticket + FIN_OFF;
    int last = 0;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (atomicAdd(t + 1 + g, 1) == members - 1) {
      atomicExch(t + 1 + g, 0);
      if (atomicAdd(t, 1) == ngroups - 1) { atomicExch(t, 0); last = 1; }
    }
    s_last = last;
  }
  __syncthreads();
  if (s_last) {
    const BnFin& f = p.fin;
    if (tid == 0 && f.nbt != nullptr) *f.nbt += 1;
    for (int c = tid; c < p.N; c += 256) {
      double s1 = __builtin_bit_cast(double, atomicExch(reinterpret_cast<unsigned long long*>(p.stats + c), 0ull));
      double s2 = __builtin_bit_cast(double, atomicExch(reinterpret_cast<unsigned long long*>(p.stats + p.N + c), 0ull));
      if (f.racc != nullptr) { s1 += repl_take(f.racc, p.N, c); s2 += repl_take(f.racc, p.N, p.N + c); }
      bn_finalize_channel(c, p.N, f.count, s1, s2, f.gamma, f.beta, f.eps, f.momentum, f.rmean, f.rvar, f.ss, f.mi,
                          f.conv_bias);
    }
  }
}

bool fwd_tile_takes(const MlpArgs& a, bool pro) {
  return sw().fwd_tile && a.R <= sw().fwd_tile_max_r && a.K % 32 == 0 && a.K >= 64 && a.K <= 1024 && a.N % 64 == 0 && a.ldx % 4 == 0 &&
         a.ldb == 0 && a.ldy % 1 == 0 && a.stats != nullptr && a.fin.ss != nullptr && a.fin.ticket != nullptr &&
         ((uintptr_t)a.X % 16 == 0) && ((uintptr_t)a.Bt % 16 == 0) && (!pro || a.vec != nullptr);
}

namespace {
template <int P, bool PRO>
int fwd_tile_go(const MlpArgs& a, hipStream_t s) {
  const int lds = 2 * 2 * P * 64 * 64 + (PRO ? 2 * a.K * 4 : 0) + 2 * 2 * 64 * 4;
  static unsigned long long reserved = 0;
  if (lds > 64 * 1024 && !reserve_lds(reinterpret_cast<const void*>(&mlp_fwd_tile_kernel<P, PRO>), lds, &reserved))
    return LAUNCH_TRY_NEXT;
  const dim3 grid(a.N / 64, (a.R + 63) / 64);
  hipLaunchKernelGGL((mlp_fwd_tile_kernel<P, PRO>), grid, dim3(256), lds, s, a);
  return check_launch("mlp_fwd_tile");
}
}  // namespace

// (planes per operand: 3 bf16 terms in compute mode 2, 1 in the bf16 mode)
int launch_fwd_tile(const MlpArgs& a, int cm, bool pro, hipStream_t s) {
  if (cm == 2) return pro ? fwd_tile_go<3, true>(a, s) : fwd_tile_go<3, false>(a, s);
  return pro ? fwd_tile_go<1, true>(a, s) : fwd_tile_go<1, false>(a, s);
}


// ---- few-row INPUT-GRADIENT launches on the same tile form -------------------------------------------------------
// dX (R x Kout) = dY (R x N) . W (N x Kout) with dY = gi*dZ + a*y + b built in the staging of the A operand (dZ: the
// dense upstream gradient G, or the pooled gradient dP routed by the arg-max slot; masked by the ReLU of THIS layer),
// W read as it is: a lane takes ONE output column and 8 consecutive reduction rows of a step - 8 coalesced dword
// loads - so its split values are exactly one 16-byte chunk of the [column][reduction] planes.  RED: the output tile
// is also layer l-1's activation gradient - its BN-backward sums are taken on the way out (Y_{l-1} read per
// element), the vectors by the last workgroup (csrc/bn_fin.h).  Reduction length p.K = this layer's channels N,
// output columns p.N; p.ldb = row stride of W.
template <int P, bool SPARSE, bool RED>
__global__ __launch_bounds__(256, 2) void mlp_dx_tile_kernel(MlpArgs p) {
  constexpr int PLANE = 64 * 64;
  constexpr int BUF = 2 * P * PLANE;
  extern __shared__ __attribute__((aligned(16))) char ft_smem[];
  char* s_buf = ft_smem;                            // [2][BUF]
  float* s_vec = reinterpret_cast<float*>(ft_smem + 2 * BUF);   // scale | shift | gi | a | b of THIS layer (5 x p.K)
  float* s_red = s_vec + 5 * p.K;                   // [2 waves][2 sums][64 columns]
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 31, lh = lane >> 5;
  const int wm = wave & 1, wn = wave >> 1;
  int bx = blockIdx.x, by = blockIdx.y;
  {
    const int gx = gridDim.x, gy = gridDim.y;
    if ((gy & 7) == 0) {
      const int L = bx + gx * by;
      by = (L & 7) + 8 * (L / (8 * gx));
      bx = (L >> 3) % gx;
    }
  }
  const int m0 = by * 64, n0 = bx * 64;
  for (int i = tid; i < 5 * p.K; i += 256) s_vec[i] = p.vec[i];
  // A staging: row (tid >> 2) of the tile, 8 consecutive channels of the step
  const int srow = tid >> 2, sch = tid & 3;
  const int arow = min(m0 + srow, p.R - 1);
  const bool arow_ok = m0 + srow < p.R;
  const float* gy = p.X + (size_t)arow * p.ldx + 8 * sch;                     // Y_l
  const float* gg = SPARSE ? nullptr : p.G + (size_t)arow * p.ldx + 8 * sch;   // dense upstream gradient
  const int rp = SPARSE ? arow / p.ns : 0;
  const int slot = SPARSE ? arow - rp * p.ns : 0;
  const float* gdp = SPARSE ? p.dP + (size_t)rp * p.K + 8 * sch : nullptr;
  const int* garg = SPARSE ? p.arg + (size_t)rp * p.K + 8 * sch : nullptr;
  // B staging: output column (tid & 63), reduction rows 8 (tid >> 6) .. + 7 of the step
  const int bcol = tid & 63, bq = tid >> 6;
  const float* gw = p.Bt + (size_t)(8 * bq) * p.ldb + n0 + bcol;
  const int nk = p.K / 32;
  struct Stage { float4 y[2], g[2]; int4 a[2]; float w[8]; };
  Stage st0, st1;
  auto fetch = [&](Stage& st, int ks) {
    st.y[0] = *reinterpret_cast<const float4*>(gy + 32 * ks);
    st.y[1] = *reinterpret_cast<const float4*>(gy + 32 * ks + 4);
    if constexpr (SPARSE) {
      st.g[0] = *reinterpret_cast<const float4*>(gdp + 32 * ks);
      st.g[1] = *reinterpret_cast<const float4*>(gdp + 32 * ks + 4);
      st.a[0] = *reinterpret_cast<const int4*>(garg + 32 * ks);
      st.a[1] = *reinterpret_cast<const int4*>(garg + 32 * ks + 4);
    } else {
      st.g[0] = *reinterpret_cast<const float4*>(gg + 32 * ks);
      st.g[1] = *reinterpret_cast<const float4*>(gg + 32 * ks + 4);
    }
    const float* w = gw + (size_t)(32 * ks) * p.ldb;
#pragma unroll
    for (int e = 0; e < 8; ++e) st.w[e] = w[(size_t)e * p.ldb];
  };
  auto commit = [&](const Stage& st, int ks, char* buf) {
    const int c0 = 32 * ks + 8 * sch;
    const float y[8] = {st.y[0].x, st.y[0].y, st.y[0].z, st.y[0].w, st.y[1].x, st.y[1].y, st.y[1].z, st.y[1].w};
    const float g[8] = {st.g[0].x, st.g[0].y, st.g[0].z, st.g[0].w, st.g[1].x, st.g[1].y, st.g[1].z, st.g[1].w};
    const int ar[8] = {st.a[0].x, st.a[0].y, st.a[0].z, st.a[0].w, st.a[1].x, st.a[1].y, st.a[1].z, st.a[1].w};
    float dy[8];
    float v5[5][8];                                   // scale, shift, gi, a, b of the thread's 8 channels: float4 reads
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      const float4 lo = *reinterpret_cast<const float4*>(s_vec + q * p.K + c0);
      const float4 hi = *reinterpret_cast<const float4*>(s_vec + q * p.K + c0 + 4);
      v5[q][0] = lo.x; v5[q][1] = lo.y; v5[q][2] = lo.z; v5[q][3] = lo.w;
      v5[q][4] = hi.x; v5[q][5] = hi.y; v5[q][6] = hi.z; v5[q][7] = hi.w;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const bool on = __builtin_fmaf(y[e], v5[0][e], v5[1][e]) > 0.f;
      float dz;
      if constexpr (SPARSE) dz = (on && ar[e] == slot) ? g[e] : 0.f;
      else dz = on ? g[e] : 0.f;
      dy[e] = arow_ok ? __builtin_fmaf(v5[2][e], dz, __builtin_fmaf(v5[3][e], y[e], v5[4][e])) : 0.f;
    }
    uint4 pa[P], pw[P];
    ft_split8<P>(make_float4(dy[0], dy[1], dy[2], dy[3]), make_float4(dy[4], dy[5], dy[6], dy[7]), pa);
    ft_split8<P>(make_float4(st.w[0], st.w[1], st.w[2], st.w[3]), make_float4(st.w[4], st.w[5], st.w[6], st.w[7]), pw);
    const int offa = swz(srow, sch), offb = swz(bcol, bq);
#pragma unroll
    for (int q = 0; q < P; ++q) {
      *reinterpret_cast<uint4*>(buf + q * PLANE + offa) = pa[q];
      *reinterpret_cast<uint4*>(buf + (P + q) * PLANE + offb) = pw[q];
    }
  };
  f32x16 acc, acc2;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc[r] = 0.f; acc2[r] = 0.f; }
  fetch(st0, 0);
  if (nk > 1) fetch(st1, 1);
  __syncthreads();                                  // the layer's vectors
  commit(st0, 0, s_buf);
  if (nk > 2) fetch(st0, 2);
  __syncthreads();
  auto step = [&](int ks, const char* cur, char* nxt, Stage& sn) {
    bf16x8 fa[2][P], fb[2][P];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int q = 0; q < P; ++q) {
        fa[s2][q] = *reinterpret_cast<const bf16x8*>(cur + q * PLANE + swz(wm * 32 + lr, 2 * s2 + lh));
        fb[s2][q] = *reinterpret_cast<const bf16x8*>(cur + (P + q) * PLANE + swz(wn * 32 + lr, 2 * s2 + lh));
      }
    if constexpr (P == 3) {
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0][2], fb[0][0], acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[1][2], fb[1][0], acc2, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0][0], fb[0][2], acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[1][0], fb[1][2], acc2, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0][1], fb[0][1], acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[1][1], fb[1][1], acc2, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0][1], fb[0][0], acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[1][1], fb[1][0], acc2, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0][0], fb[0][1], acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[1][0], fb[1][1], acc2, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0][0], fb[0][0], acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[1][0], fb[1][0], acc2, 0, 0, 0);
    } else {
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0][0], fb[0][0], acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[1][0], fb[1][0], acc2, 0, 0, 0);
    }
    if (ks + 1 < nk) {
      commit(sn, ks + 1, nxt);
      if (ks + 3 < nk) fetch(sn, ks + 3);
    }
    lds_barrier();
  };
  // RED: this lane's 16 values of Y_{l-1} (the rows / column of its accumulator registers) are requested now and
  // arrive underneath the K loop instead of as 16 exposed loads behind it
  const int n = n0 + wn * 32 + lr;                  // output column of this launch
  float yprev[16];
  if constexpr (RED) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = min(m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh, p.R - 1);
      yprev[r] = p.fY[(size_t)m * p.fld + p.fc0 + n];
    }
  }
  for (int ks = 0; ks < nk; ks += 2) {
    step(ks, s_buf, s_buf + BUF, st1);
    if (ks + 1 < nk) step(ks + 1, s_buf + BUF, s_buf, st0);
  }
  // ---- epilogue
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] += acc2[r];
  float sc0 = 0.f, sh0 = 0.f, mu0 = 0.f, is0 = 0.f;
  if constexpr (RED) {
    sc0 = p.fss[p.fc0 + n]; sh0 = p.fss[p.fld + p.fc0 + n];
    mu0 = p.fmi[p.fc0 + n]; is0 = p.fmi[p.fld + p.fc0 + n];
  }
  float es1 = 0.f, es2 = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
    if (m < p.R) {
      p.Y[(size_t)m * p.ldy + n] = acc[r];
      if constexpr (RED) {
        const float y = yprev[r];
        const float dz = __builtin_fmaf(y, sc0, sh0) > 0.f ? acc[r] : 0.f;
        es1 += dz;
        es2 = __builtin_fmaf(dz, (y - mu0) * is0, es2);
      }
    }
  }
  if constexpr (RED) {
    es1 += __shfl_xor(es1, 32);
    es2 += __shfl_xor(es2, 32);
    if (lh == 0) {
      s_red[(wm * 2 + 0) * 64 + wn * 32 + lr] = es1;
      s_red[(wm * 2 + 1) * 64 + wn * 32 + lr] = es2;
    }
    __syncthreads();
    if (tid < 128) {
      const int which = tid >> 6, c = tid & 63;
      const float v = s_red[(0 * 2 + which) * 64 + c] + s_red[(1 * 2 + which) * 64 + c];
      double* sdst = p.vfin.ticket != nullptr && p.vfin.racc != nullptr ? repl_copy(p.vfin.racc, p.fld, (int)blockIdx.y) : p.stats;
      atomicAdd(sdst + (size_t)which * p.fld + p.fc0 + n0 + c, (double)v);
    }
    if (p.vfin.ticket != nullptr) {
      sync_drained();
      if (tid == 0)
        s_last = last_workgroup(p.vfin.ticket, (int)(gridDim.x * gridDim.y), (int)(blockIdx.y * gridDim.x + blockIdx.x));
      __syncthreads();
      if (s_last) bn_vec_finalize(p.vfin, p.fld, p.fc0, p.N, p.stats, tid, 256);
    }
  }
}

bool dx_tile_takes(const MlpArgs& a, bool sparse, bool red) {
  return sw().dx_tile && a.R <= sw().dx_tile_max_r && a.K % 32 == 0 && a.K >= 64 && a.K <= 1024 && a.N % 64 == 0 && a.ldx % 4 == 0 &&
         a.ldb > 0 && a.vec != nullptr && ((uintptr_t)a.X % 16 == 0) && (sparse ? (a.dP && a.arg && a.ns >= 1) : (a.G != nullptr)) &&
         (sparse ? ((uintptr_t)a.dP % 16 == 0 && (uintptr_t)a.arg % 16 == 0) : ((uintptr_t)a.G % 16 == 0)) &&
         (!red || (a.fY && a.fss && a.fmi && a.stats));
}

namespace {
template <int P, bool SPARSE, bool RED>
int dx_tile_go(const MlpArgs& a, hipStream_t s) {
  const int lds = 2 * 2 * P * 64 * 64 + 5 * a.K * 4 + 2 * 2 * 64 * 4;
  static unsigned long long reserved = 0;
  if (lds > 64 * 1024 && !reserve_lds(reinterpret_cast<const void*>(&mlp_dx_tile_kernel<P, SPARSE, RED>), lds, &reserved))
    return LAUNCH_TRY_NEXT;
  const dim3 grid(a.N / 64, (a.R + 63) / 64);
  hipLaunchKernelGGL((mlp_dx_tile_kernel<P, SPARSE, RED>), grid, dim3(256), lds, s, a);
  return check_launch("mlp_dx_tile");
}

template <int P>
int dx_tile_form(const MlpArgs& a, bool sparse, bool red, hipStream_t s) {
  if (sparse) return red ? dx_tile_go<P, true, true>(a, s) : dx_tile_go<P, true, false>(a, s);
  return red ? dx_tile_go<P, false, true>(a, s) : dx_tile_go<P, false, false>(a, s);
}
}  // namespace

int launch_dx_tile(const MlpArgs& a, int cm, bool sparse, bool red, hipStream_t s) {
  return cm == 2 ? dx_tile_form<3>(a, sparse, red, s) : dx_tile_form<1>(a, sparse, red, s);
}

}  // namespace demf
