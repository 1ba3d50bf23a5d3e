// Shared-MLP forward with the weight resident in LDS and free-running waves (mlp_fwd_res_kernel): 64-channel
// inputs, N = 64 / 128 - SA1's layers, with the bf16-storage, no-store and recompute-the-layer-below forms (ST).
// The kernel, the condition under which the dispatcher (launch_gemm_t, csrc/mlp.hip) hands a launch to it, and its
// launcher.
#include "mlp_dev.h"

namespace demf {

// ---- forward GEMM with the WEIGHT RESIDENT in LDS and free-running waves ---------------------------
// mlp_gemm_kernel (csrc/mlp.hip) restages the weight slab from L2 for every K step of every row tile and
// separates the steps with workgroup barriers: at SA1's last layer (R = 1 M rows, 64 -> 128) every
// 128-row tile costs 2 restagings + 4 barriers, the waves of a workgroup move in lockstep and the kernel
// sits at 0.50 of the HBM roof with its VALU, MFMA and memory phases in series.
// For layers whose whole weight fits LDS as split bf16 planes (N*K*2*P bytes: 48 KB for 128 x 64 in the
// three-term mode) it is staged ONCE per workgroup; after that a wave needs nobody: it walks its own
// 64-row units (two 32-row tiles), loads them as 4-channel register patches (full 256-byte rows), applies
// the previous layer's BN + ReLU, splits the result once into bf16 planes in its PRIVATE LDS slab, and
// runs the MFMAs against the resident weight planes - no workgroup barrier anywhere in the main loop, so
// the eight waves of a CU drift apart and one's loads / transform / stores overlap another's MFMAs.
// Epilogue as in mlp_gemm_kernel: raw output stored, column statistics (-> the in-kernel BN finalize by
// the last workgroup), and the max-pool over ns = 16 / 32 / 64 rows on the extremum the sign of gamma
// selects (a 64-row group = the wave's two tiles, folded in registers).

// ST (bf16 compute mode only, BASELINE configs[3]): the rows themselves live in HBM as bf16 - bit 0: the
// input rows X, bit 1: the raw output Y (statistics and pooling still see the fp32 accumulators).  A
// lane pair (columns 2c, 2c+1) swaps one register per row pair through DPP so that every lane stores one
// packed dword: half the bytes AND half the store instructions of the fp32 form.
template <int NTN, int KT, bool POOL, int CM, int ST = 0>   // N = 32*NTN, K = 32*KT (KT = 2); CM 1 bf16 / 2 three bf16 terms / 3 two fp16 terms
__global__ __launch_bounds__(64 * FR_NW, 1) void mlp_fwd_res_kernel(MlpArgs p) {
  constexpr bool XB = (ST & 1) != 0, YB = (ST & 2) != 0;
  // ST bit 2 (pooled launches): the raw output is NOT stored at all - the backward of a pooled last
  // layer can be written without it (csrc/mlp_bwd.hip mlp_bwd_pool_kernel): what leaves the kernel is the
  // column statistics and, per group and channel, the selected extremum + its row.  Channels with
  // gamma == 0 (constant activation: upstream's max-pool picks slot 0) then report slot 0 and ITS raw
  // value, which the BN backward needs for dgamma and could otherwise only gather from Y.
  constexpr bool NOY = (ST & 4) != 0;
  static_assert(!NOY || (POOL && !YB), "no-store form: pooled launches, fp32 bookkeeping");
  // ST bit 3: X holds the 4-float input rows of the layer BELOW (SA1's first layer, 4 -> K channels): that
  // layer's raw output - 256 bytes per row - is never materialised; the 16 fma per lane and row that rebuild
  // the lane's four channels of it are free next to a 16-fold cut of the bytes read.  In the bf16 mode the
  // products are taken on bf16-rounded operands, as the MFMA kernel that used to produce the rows did.
  constexpr bool XR = (ST & 8) != 0;
  static_assert(!XR || !XB, "recomputed rows have no storage type");
  constexpr int P = CM == 2 ? 3 : (CM == 3 ? 2 : 1);
  constexpr int N = NTN * 32, K = KT * 32, KB = K * 2;
  constexpr int KS = K / 16;                       // MFMA K steps
  constexpr int LPR = K / 4;                       // lanes per row of the patch load (float4 each)
  constexpr int RPI = 64 / LPR;                    // rows per load instruction
  constexpr int NLD = 32 / RPI;                    // loads per 32-row tile
  static_assert(KT == 2, "rows of 64 channels");
  extern __shared__ __attribute__((aligned(16))) char fr_smem[];
  char* s_w = fr_smem;                                       // [P][N rows x KB]
  char* s_a = s_w + P * N * KB;                              // [8 waves][P][32 rows x KB]
  float* s_vec = reinterpret_cast<float*>(s_a + FR_NW * P * 32 * KB);   // scale | shift (2K)
  float* s_red = s_vec + 2 * K;                              // [8][NTN][64]
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 31, lh = lane >> 5;
  // ---- the weight (N x K) as split planes, once ------------------------------------------------------
  for (int i = tid; i < N * (K / 4); i += 64 * FR_NW) {
    const int n = i / (K / 4), k = 4 * (i % (K / 4));
    const float4 w = *reinterpret_cast<const float4*>(p.Bt + (size_t)n * K + k);
    unsigned p0[P], p1[P];
    fr_split_pair<P>(w.x, w.y, p0);
    fr_split_pair<P>(w.z, w.w, p1);
#pragma unroll
    for (int q = 0; q < P; ++q)
      *reinterpret_cast<uint2*>(s_w + q * N * KB + fr_swz<KB>(n, k >> 3) + 2 * (k & 7)) = make_uint2(p0[q], p1[q]);
  }
  for (int i = tid; i < 2 * K; i += 64 * FR_NW) s_vec[i] = p.vec[i];
  __syncthreads();
  // lane's patch: channels 4*c4 .. +3 of rows rq + RPI*j
  const int c4 = lane % LPR, rq = lane / LPR;
  const float4 sc = *reinterpret_cast<const float4*>(s_vec + 4 * c4);
  const float4 sh = *reinterpret_cast<const float4*>(s_vec + K + 4 * c4);
  float4 w0r[XR ? 4 : 1];                              // XR: rows 4*c4 .. +3 of the lower layer's (K x 4) weight
  if constexpr (XR) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float4 w = *reinterpret_cast<const float4*>(p.W0 + (size_t)(4 * c4 + e) * 4);
      if constexpr (CM == 1) {
        w.x = (float)(__bf16)w.x; w.y = (float)(__bf16)w.y; w.z = (float)(__bf16)w.z; w.w = (float)(__bf16)w.w;
      }
      w0r[e] = w;
    }
  }
  char* my_a = s_a + wave * P * 32 * KB;
  unsigned selbits = 0, zbits = 0;
  if constexpr (POOL) {
#pragma unroll
    for (int nt = 0; nt < NTN; ++nt) {
      const float gm = p.fin.gamma[nt * 32 + lr];
      if (gm < 0.f) selbits |= 1u << nt;
      if (NOY && gm == 0.f) zbits |= 1u << nt;
    }
  }
  float cs1[NTN], cs2[NTN];
#pragma unroll
  for (int nt = 0; nt < NTN; ++nt) cs1[nt] = cs2[nt] = 0.f;
  const int ntile = (p.R + 31) / 32;
  const int nunit = (ntile + 1) / 2;
  float4 raw[NLD];
  auto fetch = [&](int tile) {
    const int row0 = tile * 32;
#pragma unroll
    for (int j = 0; j < NLD; ++j) {
      int row = row0 + rq + RPI * j;
      row = row < p.R ? row : p.R - 1;                     // valid address; zeroed by the transform
      if constexpr (XR) {
        raw[j] = *reinterpret_cast<const float4*>(p.X + (size_t)row * 4);       // the 4-float INPUT row
      } else if constexpr (XB) {
        const uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const __bf16*>(p.X) + (size_t)row * p.ldx + 4 * c4);
        raw[j] = make_float4(__builtin_bit_cast(float, u.x << 16), __builtin_bit_cast(float, u.x & 0xffff0000u),
                             __builtin_bit_cast(float, u.y << 16), __builtin_bit_cast(float, u.y & 0xffff0000u));
      } else {
        raw[j] = *reinterpret_cast<const float4*>(p.X + (size_t)row * p.ldx + 4 * c4);
      }
    }
  };
  int unit = blockIdx.x * FR_NW + wave;
  const int ustride = gridDim.x * FR_NW;
  if (unit < nunit) fetch(2 * unit);
  for (; unit < nunit; unit += ustride) {
    float pmx[NTN];
    int pax[NTN];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int tile = 2 * unit + half;
      if (tile >= ntile) break;
      const int row0 = tile * 32;
      // ---- BN + ReLU of the previous layer, split once, into the wave's private planes ---------------
      const bool tail = row0 + 32 > p.R;
#pragma unroll
      for (int j = 0; j < NLD; ++j) {
        const int rl = rq + RPI * j;
        float4 x = raw[j];
        if constexpr (XR) {                                  // the lane's four channels of the lower layer's output
          float4 r = x;
          if constexpr (CM == 1) {
            r.x = (float)(__bf16)r.x; r.y = (float)(__bf16)r.y; r.z = (float)(__bf16)r.z; r.w = (float)(__bf16)r.w;
          }
          x.x = __builtin_fmaf(r.w, w0r[0].w, __builtin_fmaf(r.z, w0r[0].z, __builtin_fmaf(r.y, w0r[0].y, r.x * w0r[0].x)));
          x.y = __builtin_fmaf(r.w, w0r[1].w, __builtin_fmaf(r.z, w0r[1].z, __builtin_fmaf(r.y, w0r[1].y, r.x * w0r[1].x)));
          x.z = __builtin_fmaf(r.w, w0r[2].w, __builtin_fmaf(r.z, w0r[2].z, __builtin_fmaf(r.y, w0r[2].y, r.x * w0r[2].x)));
          x.w = __builtin_fmaf(r.w, w0r[3].w, __builtin_fmaf(r.z, w0r[3].z, __builtin_fmaf(r.y, w0r[3].y, r.x * w0r[3].x)));
        }
        x.x = fmaxf(0.f, __builtin_fmaf(x.x, sc.x, sh.x));
        x.y = fmaxf(0.f, __builtin_fmaf(x.y, sc.y, sh.y));
        x.z = fmaxf(0.f, __builtin_fmaf(x.z, sc.z, sh.z));
        x.w = fmaxf(0.f, __builtin_fmaf(x.w, sc.w, sh.w));
        if (tail && row0 + rl >= p.R) x = make_float4(0.f, 0.f, 0.f, 0.f);
        unsigned p0[P], p1[P];
        fr_split_pair<P>(x.x, x.y, p0);
        fr_split_pair<P>(x.z, x.w, p1);
#pragma unroll
        for (int q = 0; q < P; ++q)
          *reinterpret_cast<uint2*>(my_a + q * 32 * KB + fr_swz<KB>(rl, c4 >> 1) + 8 * (c4 & 1)) =
              make_uint2(p0[q], p1[q]);
      }
      // next tile's rows in flight underneath this tile's MFMAs and epilogue
      {
        const int nxt = half == 0 ? tile + 1 : 2 * (unit + ustride);
        if (nxt < ntile && (half == 0 || unit + ustride < nunit)) fetch(nxt);
      }
      f32x16 acc[1][NTN];
#pragma unroll
      for (int nt = 0; nt < NTN; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][nt][r] = 0.f;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        bf16x8 a[P];
#pragma unroll
        for (int q = 0; q < P; ++q)
          a[q] = *reinterpret_cast<const bf16x8*>(my_a + q * 32 * KB + fr_swz<KB>(lr, 2 * s + lh));
#pragma unroll
        for (int nt = 0; nt < NTN; ++nt) {
          bf16x8 b[P];
#pragma unroll
          for (int q = 0; q < P; ++q)
            b[q] = *reinterpret_cast<const bf16x8*>(s_w + q * N * KB + fr_swz<KB>(nt * 32 + lr, 2 * s + lh));
          fr_mfma<P>(acc[0][nt], a, b);
        }
      }
      // ---- epilogue: raw output, column statistics, pooled extremum ---------------------------------
      const bool full = row0 + 32 <= p.R;
#pragma unroll
      for (int nt = 0; nt < NTN; ++nt) {
        const int col = nt * 32 + lr;
        if constexpr (NOY) {
          // (nothing to store)
        } else if constexpr (YB) {
          // lanes (2c, 2c+1): the even lane stores row r, the odd lane row r+1 of the register pair
          const bool odd = lane & 1;
          unsigned* yp = reinterpret_cast<unsigned*>(reinterpret_cast<__bf16*>(p.Y) +
                                                      (size_t)(row0 + 4 * lh) * N + (col & ~1));
#pragma unroll
          for (int r = 0; r < 16; r += 2) {
            const float send = odd ? acc[0][nt][r] : acc[0][nt][r + 1];
            const float recv = dpp_f32<0xB1>(send, send);              // quad_perm [1,0,3,2]
            const f32x2_t v = {odd ? recv : acc[0][nt][r], odd ? acc[0][nt][r + 1] : recv};
            const int rr = r + (odd ? 1 : 0);
            const int rl = (rr & 3) + 8 * (rr >> 2);
            if (full || row0 + 4 * lh + rl < p.R)
              yp[(size_t)rl * (N / 2)] = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));
          }
        } else {
        float* yp = p.Y + (size_t)(row0 + 4 * lh) * N + col;
        if (full) {
#pragma unroll
          for (int r = 0; r < 16; ++r) yp[(size_t)((r & 3) + 8 * (r >> 2)) * N] = acc[0][nt][r];
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (row0 + 4 * lh + (r & 3) + 8 * (r >> 2) < p.R) yp[(size_t)((r & 3) + 8 * (r >> 2)) * N] = acc[0][nt][r];
        }
        }
        f32x2_t a1 = {0.f, 0.f}, a2 = {0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 16; r += 2) {                    // rows >= R are exact zeros
          const f32x2_t v = {acc[0][nt][r], acc[0][nt][r + 1]};
          a1 += v;
          a2 = __builtin_elementwise_fma(v, v, a2);
        }
        cs1[nt] += a1.x + a1.y;
        cs2[nt] += a2.x + a2.y;
        if constexpr (POOL) {
          const unsigned flip = ((selbits >> nt) & 1u) << 31;
          if (p.ns == 16) pool_epilogue_sel<1, NTN, 16>(p, acc, nt, row0, col, lh, flip);
          else if (p.ns == 32) pool_epilogue_sel<1, NTN, 32>(p, acc, nt, row0, col, lh, flip);
          else {
            // ns = 64: this tile's extremum (first maximum wins: rows ascend), folded with the other half
            float mx = -__builtin_inff();
            int ax = 0;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int rho = 32 * half + 4 * lh + (r & 3) + 8 * (r >> 2);
              const float v = flip_sign(acc[0][nt][r], flip);
              const bool up = v > mx;
              mx = up ? v : mx; ax = up ? rho : ax;
            }
            if constexpr (NOY) {
              if ((zbits >> nt) & 1u) {              // gamma == 0: slot 0 of the group and its raw value
                const bool has0 = half == 0 && lh == 0;
                mx = has0 ? flip_sign(acc[0][nt][0], flip) : -__builtin_inff();
                ax = has0 ? 0 : 64;
              }
            }
            const float omx = __shfl_xor(mx, 32);
            const int oax = __shfl_xor(ax, 32);
            if (omx > mx || (omx == mx && oax < ax)) { mx = omx; ax = oax; }
            if (half == 0) { pmx[nt] = mx; pax[nt] = ax; }
            else {
              if (!(mx > pmx[nt])) { mx = pmx[nt]; ax = pax[nt]; }     // the earlier half wins ties
              if (lh == 0) {
                const size_t o = (size_t)unit * N + col;
                p.pmax[o] = flip_sign(mx, flip);
                p.amax[o] = ax;
              }
            }
          }
        }
      }
    }
  }
  // ---- column statistics: lanes l / l+32 share a column, then the 8 waves, one fp64 atomic each -------
#pragma unroll
  for (int nt = 0; nt < NTN; ++nt) {
    cs1[nt] += __shfl_xor(cs1[nt], 32);
    cs2[nt] += __shfl_xor(cs2[nt], 32);
    if (lh == 0) {
      s_red[(wave * NTN + nt) * 64 + lr] = cs1[nt];
      s_red[(wave * NTN + nt) * 64 + 32 + lr] = cs2[nt];
    }
  }
  __syncthreads();
  for (int i = tid; i < NTN * 64; i += 64 * FR_NW) {
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < FR_NW; ++w) v += s_red[w * NTN * 64 + i];
    const int nt = i >> 6, which = (i >> 5) & 1, c = i & 31;
    double* sdst = p.fin.ss != nullptr && p.fin.racc != nullptr ? repl_copy(p.fin.racc, N, (int)blockIdx.x) : p.stats;
    atomicAdd(sdst + which * N + nt * 32 + c, (double)v);
  }
  if (p.fin.ss != nullptr) {
    // train-mode BN bookkeeping by the last workgroup (as mlp_gemm_kernel: only atomics touch the sums)
    sync_drained();
    if (tid == 0) {
      const int total = (int)gridDim.x;
      const int ngroups = total < SCHED_GROUPS ? total : SCHED_GROUPS;
      const int g = (int)blockIdx.x % SCHED_GROUPS;
      const int members = total / SCHED_GROUPS + (g < total % SCHED_GROUPS ? 1 : 0);
      int* t = p.fin.ticket + FIN_OFF;
      int last = 0;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // own sum atomics acknowledged first (csrc/bn_fin.h)
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
      for (int c = tid; c < N; c += 64 * FR_NW) {
        double s1 = __builtin_bit_cast(double, atomicExch(reinterpret_cast<unsigned long long*>(p.stats + c), 0ull));
        double s2 = __builtin_bit_cast(double, atomicExch(reinterpret_cast<unsigned long long*>(p.stats + N + c), 0ull));
        if (f.racc != nullptr) { s1 += repl_take(f.racc, N, c); s2 += repl_take(f.racc, N, N + c); }
        bn_finalize_channel(c, N, f.count, s1, s2, f.gamma, f.beta, f.eps, f.momentum, f.rmean, f.rvar, f.ss,
                            f.mi, f.conv_bias);
      }
    }
  }
}

bool fwd_res_takes(const MlpArgs& a, bool pool) {
  const bool sel = !pool || (a.pmin == nullptr && a.fin.gamma != nullptr);
  return (sw().fwd_res || a.st) && a.K == 64 && (a.N == 64 || a.N == 128) && (a.ldx == 64 || (a.st == 8 && a.ldx == 4)) &&
         a.ldy == a.N && a.ldb == 0 && sel &&
         a.R >= 64 * 256 && (!pool || ((a.ns == 16 || a.ns == 32 || a.ns == 64) && a.R % 64 == 0)) &&
         (a.fin.ss == nullptr || a.fin.ticket != nullptr);
}

namespace {
struct ResGeom { int gx; size_t bytes; };

template <int NTN, bool POOL, int CM, int ST>
int res_go(const MlpArgs& a, const ResGeom& g, hipStream_t s) {
  static unsigned long long reserved = 0;      // bit per device
  if (!reserve_lds(reinterpret_cast<const void*>(&mlp_fwd_res_kernel<NTN, 2, POOL, CM, ST>), (int)g.bytes, &reserved)) {
    set_error("mlp_fwd_res: cannot reserve %zu bytes of LDS", g.bytes);
    return DEMF_ELAUNCH;
  }
  hipLaunchKernelGGL((mlp_fwd_res_kernel<NTN, 2, POOL, CM, ST>), dim3(g.gx), dim3(64 * FR_NW), g.bytes, s, a);
  return check_launch("mlp_fwd_res");
}

// kernel mode of the launch: 1 bf16, 2 three bf16 terms, 3 two fp16 terms (h2)
template <int NTN, bool POOL, int ST>
int res_mode(const MlpArgs& a, int cm, bool h2, const ResGeom& g, hipStream_t s) {
  if (cm == 2) return h2 ? res_go<NTN, POOL, 3, ST>(a, g, s) : res_go<NTN, POOL, 2, ST>(a, g, s);
  return res_go<NTN, POOL, 1, ST>(a, g, s);
}

template <bool POOL>
int res_form(const MlpArgs& a, int cm, hipStream_t s) {
  const bool h2 = cm == 2 && f16_terms();          // two fp16 terms instead of three bf16 ones
  const int P = h2 ? 2 : (cm == 2 ? 3 : 1);
  const int ntn = a.N / 32;
  const size_t bytes = (size_t)P * a.N * 128 + (size_t)FR_NW * P * 32 * 128 + sizeof(float) * (2 * 64 + FR_NW * ntn * 64);
  const int nunit = (a.R + 63) / 64;
  int gx = (nunit + FR_NW - 1) / FR_NW;
  // one 8-wave workgroup per CU, on 240 of the 256: the rest is left to the resident FPS chain of
  // the next batch (csrc/mlp_bwd.hip launch_fused has the measurements)
  if (gx > sw().persist_cus) gx = sw().persist_cus;
  const ResGeom g{gx, bytes};
  if (a.st == 0) return ntn == 2 ? res_mode<2, POOL, 0>(a, cm, h2, g, s) : res_mode<4, POOL, 0>(a, cm, h2, g, s);
  // bf16 storage: the two forms SA1 uses (fp32 rows in -> bf16 rows out; bf16 in -> bf16 out, pooled), bf16 mode only
  if constexpr (!POOL) {
    if (cm == 1 && a.st == 2 && ntn == 2) return res_go<2, false, 1, 2>(a, g, s);
    // input rows of the layer below instead of its output (either mode): SA1's second layer
    if (a.st == 8 && ntn == 2 && a.W0 != nullptr) return res_mode<2, false, 8>(a, cm, h2, g, s);
  } else {
    if (cm == 1 && a.st == 3 && ntn == 4) return res_go<4, true, 1, 3>(a, g, s);
    // no-store form (either mode): SA1's last layer, 64-row groups
    if (a.st == 4 && ntn == 4 && a.ns == 64) return res_mode<4, true, 4>(a, cm, h2, g, s);
  }
  set_error("mlp_fwd_res: bf16 storage form st=%d N=%d pool=%d mode=%d not built", a.st, a.N, (int)POOL, cm);
  return DEMF_EUNSUPPORTED;
}
}  // namespace

int launch_fwd_res(const MlpArgs& a, int cm, bool pool, hipStream_t s) {
  return pool ? res_form<true>(a, cm, s) : res_form<false>(a, cm, s);
}

}  // namespace demf
