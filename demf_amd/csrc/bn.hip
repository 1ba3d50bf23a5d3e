// Train-mode BatchNorm around the shared-MLP GEMMs, as launches of their own: statistics -> scale / shift and running
// statistics (bn_finalize_kernel), BN + ReLU + max over neighbours (bnrelu_maxpool_fwd_k), the pick between the
// pooled maxima and minima once the scale is known (pool_select_k), the two row reductions of the backward
// (bn_bwd_reduce_k, bn_bwd_reduce_dense4_k) and its per-channel vectors (bn_bwd_vectors_k), with their entry points.
// The per-channel arithmetic and the "last workgroup" bookkeeping they share with the GEMM kernels: csrc/bn_fin.h.
#include "mlp_args.h"

namespace demf {

// ---- BN statistics -> per-channel scale/shift (+ running stats, saved mean/invstd) -----------
__global__ void bn_finalize_kernel(int N, double count, double* __restrict__ stats,
                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                   float eps, float momentum, float* __restrict__ running_mean,
                                   float* __restrict__ running_var,
                                   long long* __restrict__ num_batches_tracked,
                                   float* __restrict__ ss, float* __restrict__ mi,
                                   const float* __restrict__ conv_bias) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c == 0 && num_batches_tracked != nullptr) *num_batches_tracked += 1;
  if (c >= N) return;
  const double s1 = stats[c], s2 = stats[N + c];
  stats[c] = 0.0;                                   // consumed: the accumulator is left zeroed
  stats[N + c] = 0.0;
  bn_finalize_channel(c, N, count, s1, s2, gamma, beta, eps, momentum, running_mean, running_var, ss,
                      mi, conv_bias);
}

// ---- tail: out[r,c] = max_s max(0, y[r,s,c]*scale+shift), first maximum wins -----------------
__global__ __launch_bounds__(256) void bnrelu_maxpool_fwd_k(long long RC, int ns, int C,
                                                            const float* __restrict__ y,
                                                            const float* __restrict__ ss,
                                                            float* __restrict__ out,
                                                            int* __restrict__ arg) {
  long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (; t < RC; t += stride) {
    const long long r = t / C;
    const int c = (int)(t - r * C);
    const float sc = ss[c], sh = ss[C + c];
    const float* p = y + r * ns * C + c;
    float best = fmaxf(0.f, __builtin_fmaf(p[0], sc, sh));
    int bi = 0;
    for (int s = 1; s < ns; ++s) {
      const float v = fmaxf(0.f, __builtin_fmaf(p[(size_t)s * C], sc, sh));
      if (v > best) {
        best = v;
        bi = s;
      }
    }
    out[t] = best;
    arg[t] = bi;
  }
}

// ---- tail for the fused pooling epilogue: pick max or min by the sign of the BN scale -----------
__global__ __launch_bounds__(256) void pool_select_k(long long RC, int C,
                                                     const float* __restrict__ pmax,
                                                     const float* __restrict__ pmin,
                                                     const int* __restrict__ amax,
                                                     const int* __restrict__ amin,
                                                     const float* __restrict__ ss,
                                                     float* __restrict__ out,
                                                     int* __restrict__ arg,
                                                     float* __restrict__ yraw, int slot0) {
  long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (; t < RC; t += stride) {
    const int c = (int)(t % C);
    const float sc = ss[c], sh = ss[C + c];
    const bool up = sc > 0.f || (slot0 && sc == 0.f);     // slot0: zero-scale channels carry slot 0 in pmax
    const float y = up ? pmax[t] : pmin[t];
    out[t] = fmaxf(0.f, __builtin_fmaf(y, sc, sh));
    const int a = sc == 0.f ? 0 : (up ? amax[t] : amin[t]);  // constant activation: first slot wins
    arg[t] = a;
    // the raw output AT the selected row (what the sparse BN-backward reduce would otherwise gather
    // from Y).  Zero scale: the selected row is slot 0, whose value is not among the extrema - NaN
    // tells the consumer to gather it (dgamma = sum dZ*xhat needs it even though gamma is 0).
    // (``slot0``: the producer tracked slot 0 and its raw value for zero-gamma channels itself - the no-store
    // forward, which has no Y to gather from)
    if (yraw) yraw[t] = (sc == 0.f && !slot0) ? __builtin_nanf("") : y;
  }
}

// ---- backward reductions: g1 = sum dZ, g2 = sum dZ*xhat per channel ---------------------------
// dense upstream gradient G (R x N); one block strides over rows, 256 threads = 64 col4 x 4 rows
template <bool SPARSE>
__global__ __launch_bounds__(256) void bn_bwd_reduce_k(int R, int N, int ns,
                                                       const float* __restrict__ G,
                                                       const float* __restrict__ dP,
                                                       const int* __restrict__ arg,
                                                       const float* __restrict__ Y,
                                                       const float* __restrict__ ss,
                                                       const float* __restrict__ mi,
                                                       double* __restrict__ g12,
                                                       const float* __restrict__ yraw, BnVecFin fin,
                                                       int y_bf16) {
  // thread -> one column, strided rows; columns are the fast index so reads coalesce
  __shared__ float red[2][256];
  __shared__ int s_last;
  const int cols_per_pass = N < 256 ? N : 256;
  const int rows_par = 256 / cols_per_pass;           // row lanes per block pass
  const int c_in = threadIdx.x % cols_per_pass, r_in = threadIdx.x / cols_per_pass;
  for (int cb = 0; cb < N; cb += cols_per_pass) {
    const int c = cb + c_in;
    float a1 = 0.f, a2 = 0.f;
    if (r_in < rows_par && c < N) {
      const float sc = ss[c], sh = ss[N + c], mu = mi[c], is = mi[N + c];
      if constexpr (SPARSE) {
        const int Rp = R / ns;
        for (int rp = blockIdx.x * rows_par + r_in; rp < Rp; rp += gridDim.x * rows_par) {
          // y at the arg-max row: handed over by demf_pool_select, else gathered from Y
          float y = yraw ? yraw[(size_t)rp * N + c] : __builtin_nanf("");
          if (y != y) {
            const size_t o = ((size_t)rp * ns + arg[(size_t)rp * N + c]) * N + c;
            y = y_bf16 ? (float)reinterpret_cast<const __bf16*>(Y)[o] : Y[o];
          }
          const float dz = __builtin_fmaf(y, sc, sh) > 0.f ? dP[(size_t)rp * N + c] : 0.f;
          a1 += dz;
          a2 = __builtin_fmaf(dz, (y - mu) * is, a2);
        }
      } else {
        for (int r = blockIdx.x * rows_par + r_in; r < R; r += gridDim.x * rows_par) {
          const float y = Y[(size_t)r * N + c];
          const float dz = __builtin_fmaf(y, sc, sh) > 0.f ? G[(size_t)r * N + c] : 0.f;
          a1 += dz;
          a2 = __builtin_fmaf(dz, (y - mu) * is, a2);
        }
      }
    }
    red[0][threadIdx.x] = a1;
    red[1][threadIdx.x] = a2;
    __syncthreads();
    if (threadIdx.x < cols_per_pass && cb + threadIdx.x < N) {
      float t1 = 0.f, t2 = 0.f;
      for (int j = 0; j < rows_par; ++j) {
        t1 += red[0][j * cols_per_pass + threadIdx.x];
        t2 += red[1][j * cols_per_pass + threadIdx.x];
      }
      atomicAdd(g12 + cb + threadIdx.x, (double)t1);
      atomicAdd(g12 + N + cb + threadIdx.x, (double)t2);
    }
    __syncthreads();
  }
  if (fin.ticket != nullptr) {     // this layer's backward vectors by the last workgroup (csrc/bn_fin.h)
    sync_drained();
    if (threadIdx.x == 0) s_last = last_workgroup(fin.ticket, (int)gridDim.x, (int)blockIdx.x);
    __syncthreads();
    if (s_last) bn_vec_finalize(fin, N, 0, N, g12, threadIdx.x, 256);
  }
}

// dense G, N % 4 == 0, N <= 1024: a thread owns 4 consecutive channels (float4 loads of G and Y),
// row lanes fill the rest of the block; 4 rows in flight per thread.  `rev`: rows are visited last to
// first - G has just been written front to back by the dx GEMM, so its tail is what the 256 MB
// memory-side cache still holds (measured -0.03 ms/step).
// GATHER: the pooled (sparse) form on its R/ns pooled rows - G = dP, Y = yraw (the raw output at the
// selected row, handed over by demf_pool_select); a NaN there (zero BN scale: no extremum was selected)
// sends that one value to the arg-max row of the full output Yfull, as bn_bwd_reduce_k<true> does.
template <bool GATHER>
__global__ __launch_bounds__(256) void bn_bwd_reduce_dense4_k(int R, int N,
                                                              const float* __restrict__ G,
                                                              const float* __restrict__ Y,
                                                              const float* __restrict__ ss,
                                                              const float* __restrict__ mi,
                                                              double* __restrict__ g12, int rev,
                                                              BnVecFin fin, const float* __restrict__ Yfull,
                                                              const int* __restrict__ arg, int ns, int y_bf16) {
  __shared__ float4 red[2][256];
  __shared__ int s_last;
  const int cg = N >> 2;
  const int rows_par = 256 / cg;
  const int c4 = threadIdx.x % cg, r_in = threadIdx.x / cg;
  float4 a1 = make_float4(0.f, 0.f, 0.f, 0.f), a2 = a1;
  if (r_in < rows_par) {
    const float4 sc = reinterpret_cast<const float4*>(ss)[c4];
    const float4 sh = reinterpret_cast<const float4*>(ss + N)[c4];
    const float4 mu = reinterpret_cast<const float4*>(mi)[c4];
    const float4 is = reinterpret_cast<const float4*>(mi + N)[c4];
    const int step = gridDim.x * rows_par;
    auto acc = [&](const float4& g, const float4& y) {
      const float d0 = __builtin_fmaf(y.x, sc.x, sh.x) > 0.f ? g.x : 0.f;
      const float d1 = __builtin_fmaf(y.y, sc.y, sh.y) > 0.f ? g.y : 0.f;
      const float d2 = __builtin_fmaf(y.z, sc.z, sh.z) > 0.f ? g.z : 0.f;
      const float d3 = __builtin_fmaf(y.w, sc.w, sh.w) > 0.f ? g.w : 0.f;
      a1.x += d0; a1.y += d1; a1.z += d2; a1.w += d3;
      a2.x = __builtin_fmaf(d0, (y.x - mu.x) * is.x, a2.x);
      a2.y = __builtin_fmaf(d1, (y.y - mu.y) * is.y, a2.y);
      a2.z = __builtin_fmaf(d2, (y.z - mu.z) * is.z, a2.z);
      a2.w = __builtin_fmaf(d3, (y.w - mu.w) * is.w, a2.w);
    };
    auto fix = [&](float4& y, int rr) {          // GATHER: NaN -> the value at the arg-max row
      if constexpr (GATHER) {
        auto one = [&](float& v, int c) {
          if (v != v) {
            const size_t o = ((size_t)rr * ns + arg[(size_t)rr * N + c]) * N + c;
            v = y_bf16 ? (float)reinterpret_cast<const __bf16*>(Yfull)[o] : Yfull[o];
          }
        };
        one(y.x, 4 * c4); one(y.y, 4 * c4 + 1); one(y.z, 4 * c4 + 2); one(y.w, 4 * c4 + 3);
      }
    };
    int r = blockIdx.x * rows_par + r_in;
    for (; r + 3 * step < R; r += 4 * step) {
      float4 g[4], y[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int rr = rev ? R - 1 - (r + u * step) : r + u * step;
        const size_t o = (size_t)rr * N + 4 * c4;
        g[u] = *reinterpret_cast<const float4*>(G + o);
        y[u] = *reinterpret_cast<const float4*>(Y + o);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        fix(y[u], rev ? R - 1 - (r + u * step) : r + u * step);
        acc(g[u], y[u]);
      }
    }
    for (; r < R; r += step) {
      const int rr = rev ? R - 1 - r : r;
      const size_t o = (size_t)rr * N + 4 * c4;
      float4 y = *reinterpret_cast<const float4*>(Y + o);
      fix(y, rr);
      acc(*reinterpret_cast<const float4*>(G + o), y);
    }
  }
  red[0][threadIdx.x] = a1;
  red[1][threadIdx.x] = a2;
  __syncthreads();
  if (threadIdx.x < cg) {
    float4 t1 = make_float4(0.f, 0.f, 0.f, 0.f), t2 = t1;
    for (int j = 0; j < rows_par; ++j) {
      const float4 u = red[0][j * cg + threadIdx.x], v = red[1][j * cg + threadIdx.x];
      t1.x += u.x; t1.y += u.y; t1.z += u.z; t1.w += u.w;
      t2.x += v.x; t2.y += v.y; t2.z += v.z; t2.w += v.w;
    }
    double* dst = fin.ticket != nullptr && fin.racc != nullptr ? repl_copy(fin.racc, N, (int)blockIdx.x) : g12;
    double* o1 = dst + 4 * threadIdx.x;
    double* o2 = dst + N + 4 * threadIdx.x;
    atomicAdd(o1, (double)t1.x); atomicAdd(o1 + 1, (double)t1.y);
    atomicAdd(o1 + 2, (double)t1.z); atomicAdd(o1 + 3, (double)t1.w);
    atomicAdd(o2, (double)t2.x); atomicAdd(o2 + 1, (double)t2.y);
    atomicAdd(o2 + 2, (double)t2.z); atomicAdd(o2 + 3, (double)t2.w);
  }
  if (fin.ticket != nullptr) {     // this layer's backward vectors by the last workgroup (csrc/bn_fin.h)
    sync_drained();
    if (threadIdx.x == 0) s_last = last_workgroup(fin.ticket, (int)gridDim.x, (int)blockIdx.x);
    __syncthreads();
    if (s_last) bn_vec_finalize(fin, N, 0, N, g12, threadIdx.x, 256);
  }
}

// g1,g2 -> the 5 backward vectors + dgamma, dbeta
__global__ void bn_bwd_vectors_k(int N, double count, double* __restrict__ g12,
                                 const float* __restrict__ gamma, const float* __restrict__ ss,
                                 const float* __restrict__ mi, float* __restrict__ vec,
                                 float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= N) return;
  const double g1 = g12[c], g2 = g12[N + c];
  g12[c] = 0.0;                                     // consumed: left zeroed for the next user
  g12[N + c] = 0.0;
  const double mean = mi[c], is = mi[N + c];
  const double gi = (double)gamma[c] * is;
  const double a = -gi * is * (g2 / count);
  vec[c] = ss[c];
  vec[N + c] = ss[N + c];
  vec[2 * N + c] = (float)gi;
  vec[3 * N + c] = (float)a;
  vec[4 * N + c] = (float)(-gi * (g1 / count) - a * mean);
  dgamma[c] = (float)g2;
  dbeta[c] = (float)g1;
}

int launch_bn_finalize(int N, double* stats, const BnFin& fin, hipStream_t s) {
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(cdiv(N, 256)), dim3(256), 0, s, N, fin.count, stats,
                     fin.gamma, fin.beta, fin.eps, fin.momentum, fin.rmean, fin.rvar, fin.nbt, fin.ss,
                     fin.mi, fin.conv_bias);
  return check_launch("bn_finalize");
}

}  // namespace demf

using namespace demf;

static int pool_select_impl(int Rp, int C, const float* pmax, const float* pmin, const int* amax, const int* amin,
                            const float* scale_shift, float* out, int* arg, float* yraw, int slot0,
                            demf_stream_t stream) {
  DEMF_REQUIRE(Rp >= 0 && C >= 1, "pool_select: bad sizes");
  if (Rp == 0) return DEMF_OK;
  DEMF_REQUIRE(pmax && pmin && amax && amin && scale_shift && out && arg, "pool_select: null pointer");
  const long long RC = (long long)Rp * C;
  long long g = (RC + 255) / 256;
  if (g > 2048) g = 2048;
  hipLaunchKernelGGL(pool_select_k, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, RC, C, pmax,
                     pmin, amax, amin, scale_shift, out, arg, yraw, slot0);
  return check_launch("pool_select");
}

extern "C" int demf_pool_select(int Rp, int C, const float* pmax, const float* pmin,
                                const int* amax, const int* amin, const float* scale_shift,
                                float* out, int* arg, float* yraw, demf_stream_t stream) {
  return pool_select_impl(Rp, C, pmax, pmin, amax, amin, scale_shift, out, arg, yraw, 0, stream);
}

// The same behind the no-store pooled forward (demf_mlp_gemm_fwd_pool_bn_st, store_flags = 4): channels
// with a zero BN scale arrive with slot 0 and its raw value in pmax / amax, so yraw is complete (no NaN).
extern "C" int demf_pool_select_slot0(int Rp, int C, const float* pmax, const int* amax,
                                      const float* scale_shift, float* out, int* arg, float* yraw,
                                      demf_stream_t stream) {
  return pool_select_impl(Rp, C, pmax, pmax, amax, amax, scale_shift, out, arg, yraw, 1, stream);
}

extern "C" int demf_bn_finalize(int N, long long count, double* stats, const float* gamma,
                                const float* beta, float eps, float momentum,
                                float* running_mean, float* running_var,
                                long long* num_batches_tracked, float* scale_shift,
                                float* mean_invstd, const float* conv_bias, demf_stream_t stream) {
  DEMF_REQUIRE(N >= 1 && count >= 1 && stats && gamma && beta && scale_shift && mean_invstd,
               "bn_finalize: bad arguments");
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, N,
                     (double)count, stats, gamma, beta, eps, momentum, running_mean, running_var,
                     num_batches_tracked, scale_shift, mean_invstd, conv_bias);
  return check_launch("bn_finalize");
}

extern "C" int demf_bnrelu_maxpool_fwd(int R, int ns, int C, const float* Y,
                                       const float* scale_shift, float* out, int* arg,
                                       demf_stream_t stream) {
  DEMF_REQUIRE(R >= 0 && ns >= 1 && C >= 1, "bnrelu_maxpool: bad sizes");
  if (R == 0) return DEMF_OK;
  DEMF_REQUIRE(Y && scale_shift && out && arg, "bnrelu_maxpool: null pointer");
  const long long RC = (long long)R * C;
  long long g = (RC + 255) / 256;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(bnrelu_maxpool_fwd_k, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, RC,
                     ns, C, Y, scale_shift, out, arg);
  return check_launch("bnrelu_maxpool_fwd");
}

extern "C" int demf_bn_bwd_vectors(int, long long, double*, const float*, const float*, const float*, float*,
                                   float*, float*, demf_stream_t);

static int bn_bwd_reduce_impl(int R, int N, int ns, const float* G, const float* dP,
                              const int* arg, const float* Y, const float* yraw,
                              const float* scale_shift, const float* mean_invstd, double* g12,
                              const BnVecFin& vf, demf_stream_t stream, int y_bf16 = 0) {
  DEMF_REQUIRE(R >= 0 && N >= 1, "bn_bwd_reduce: bad sizes R=%d N=%d", R, N);
  if (R == 0) return DEMF_OK;
  // (Y may be NULL in the pooled form when yraw is complete - the no-store forward, whose yraw never holds
  // the NaN that asks for a gather from Y)
  DEMF_REQUIRE((Y || (!G && yraw)) && scale_shift && mean_invstd && g12 && (G || (dP && arg && ns >= 1)),
               "bn_bwd_reduce: null pointer");
  // (a "pooled" layer with one sample per group - the row MLPs of the FP / vote / head modules - is the
  // dense case: dP is the upstream gradient of every row and the selected row is the row itself)
  if (!G && ns == 1 && !y_bf16 && N % 4 == 0 && N <= 1024 && sw().bnred_ns1_dense) G = dP;
  if (G && N % 4 == 0 && N <= 1024) {
    const int rp = 256 / (N / 4);
    // few blocks: every block ends with 2N same-address fp64 atomics, which serialise in L2
    // (~70 ns each), so 2048 blocks cost ~150 us in the tail alone
    // (with the replicated accumulators a workgroup's 2N adds queue behind an eighth of the others': one unrolled
    //  two unrolled passes of 4 row groups per workgroup, up to 1024 of them; measured on the resident step: 4 row groups
    //  4.233, 8 4.208, 16 4.208-4.218 ms; without the copies (16 per workgroup, <= 256 of them) 4.248)
    const bool repl = vf.ticket != nullptr && vf.racc != nullptr;
    int grid = cdiv(R, rp * (repl ? sw().bnred_rpb : 16));
    const int cap = sw().bnred_grid >= 0 ? sw().bnred_grid : (repl ? 1024 : 256);
    if (grid > cap) grid = cap;
    hipLaunchKernelGGL(bn_bwd_reduce_dense4_k<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, R, N, G,
                       Y, scale_shift, mean_invstd, g12, sw().bnred_rev, vf,
                       (const float*)nullptr, (const int*)nullptr, 1, 0);
    return check_launch("bn_bwd_reduce");
  }
  // pooled form with the selected rows' raw outputs at hand: the same float4 kernel over the R/ns pooled
  // rows (<= 256 blocks -> <= 256 same-address fp64 atomics per channel instead of 1 024: at SA1 the
  // sparse kernel's 31 us were mostly that tail)
  if (!G && yraw && N % 4 == 0 && N <= 1024 && R % ns == 0 && sw().bnred_pooled_dense) {
    const int Rp = R / ns, rp = 256 / (N / 4);
    const bool repl = vf.ticket != nullptr && vf.racc != nullptr;
    int grid = cdiv(Rp, rp * (repl ? sw().bnred_rpb : 16));
    const int cap = sw().bnred_grid >= 0 ? sw().bnred_grid : (repl ? 1024 : 256);
    if (grid > cap) grid = cap;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(bn_bwd_reduce_dense4_k<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, Rp, N, dP,
                       yraw, scale_shift, mean_invstd, g12, 0, vf, Y, arg, ns, y_bf16);
    return check_launch("bn_bwd_reduce");
  }
  const int rows_par = N < 256 ? 256 / N : 1;
  const int rows = G ? R : R / ns;
  // (measured on the training step, sparse form: caps of 256 / 128 / 64 / 32 blocks cost +0.04 / +0.21 /
  // +0.45 / +1.0 ms per step - the launch is bound by its dependent loads per block, not by the
  // 2N same-address fp64 atomics each block ends with)
  int grid = cdiv(rows, rows_par * (G ? 8 : sw().bnred_sparse_rpt));
  const int scap = G ? 1024 : sw().bnred_sparse_grid;
  if (grid > scap) grid = scap;
  if (grid < 1) grid = 1;
  if (G)
    hipLaunchKernelGGL((bn_bwd_reduce_k<false>), dim3(grid), dim3(256), 0, (hipStream_t)stream, R, N,
                       ns, G, dP, arg, Y, scale_shift, mean_invstd, g12, nullptr, BnVecFin{}, 0);
  else
    hipLaunchKernelGGL((bn_bwd_reduce_k<true>), dim3(grid), dim3(256), 0, (hipStream_t)stream, R, N,
                       ns, G, dP, arg, Y, scale_shift, mean_invstd, g12, yraw, vf, y_bf16);
  return check_launch("bn_bwd_reduce");
}

extern "C" int demf_bn_bwd_reduce(int R, int N, int ns, const float* G, const float* dP,
                                  const int* arg, const float* Y, const float* yraw,
                                  const float* scale_shift, const float* mean_invstd, double* g12,
                                  demf_stream_t stream) {
  return bn_bwd_reduce_impl(R, N, ns, G, dP, arg, Y, yraw, scale_shift, mean_invstd, g12, BnVecFin{}, stream);
}

// Sparse (pooled last layer) reduce + the layer's backward vectors in ONE launch: what
// demf_bn_bwd_reduce(G = NULL) followed by demf_bn_bwd_vectors does in two.
extern "C" int demf_bn_bwd_reduce_vectors(int R, int N, int ns, const float* dP, const int* arg,
                                          const float* Y, const float* yraw, const float* scale_shift,
                                          const float* mean_invstd, double* g12, const float* gamma,
                                          float* vec6, float* dgamma, float* dbeta, int y_bf16,
                                          demf_stream_t stream) {
  DEMF_REQUIRE(gamma && vec6 && dgamma && dbeta && dP && arg, "bn_bwd_reduce_vectors: null pointer");
  BnVecFin vf{(double)R, gamma, scale_shift, mean_invstd, vec6, dgamma, dbeta, sched_slot(), nullptr};
  if (vf.ticket != nullptr && N <= ACC_MAX_N) vf.racc = accum_slot();
  if (vf.ticket == nullptr) {              // DEMF_STATIC_TILES=1: no counter sets - two launches
    if (int e = bn_bwd_reduce_impl(R, N, ns, nullptr, dP, arg, Y, yraw, scale_shift, mean_invstd, g12, BnVecFin{}, stream, y_bf16)) return e;
    return demf_bn_bwd_vectors(N, R, g12, gamma, scale_shift, mean_invstd, vec6, dgamma, dbeta, stream);
  }
  return bn_bwd_reduce_impl(R, N, ns, nullptr, dP, arg, Y, yraw, scale_shift, mean_invstd, g12, vf, stream, y_bf16);
}

extern "C" int demf_bn_bwd_vectors(int N, long long count, double* g12, const float* gamma,
                                   const float* scale_shift, const float* mean_invstd, float* vec6,
                                   float* dgamma, float* dbeta, demf_stream_t stream) {
  DEMF_REQUIRE(N >= 1 && count >= 1 && g12 && gamma && scale_shift && mean_invstd && vec6 &&
                   dgamma && dbeta,
               "bn_bwd_vectors: bad arguments");
  hipLaunchKernelGGL(bn_bwd_vectors_k, dim3(cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, N,
                     (double)count, g12, gamma, scale_shift, mean_invstd, vec6, dgamma, dbeta);
  return check_launch("bn_bwd_vectors");
}
