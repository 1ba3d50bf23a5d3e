// Gradient accumulation over the micro-steps of one optimizer step (engine.Trainer(accumulate=W)).
//
// The reference forms one AdamW step from the mean gradient of 8 ranks x 16 scenes (tools/dist_train.sh:4,
// configs/_base_/datasets/sunrgbd-3d-10class.py:75); one process reaches the same step by adding the gradients of
// W forward + backward passes into the flat gradient buffer and handing AdamW grad_scale = 1 / (W * world).  The
// gradient pack of a captured micro-step therefore ADDS where the plain step's pack copies (csrc/optim.hip:
// multi_copy_k / multi_copy_sumsq_k), and the step meter's loss scalars are accumulated on the device so that the
// one row per optimizer step holds the group's mean.  HBM-bound: 3 floats of traffic per gradient word.
#include <hip/hip_runtime.h>

#include "common.h"

namespace demf {

// n segments, dst += src, in ONE launch: blockIdx.y = segment, blockIdx.x strides over its fp32 words.
// table (device, 3 x n int64): src | dst | words, as multi_copy_k's.  A null source adds nothing: dst is not written.
__global__ __launch_bounds__(256) void multi_add_k(int n, const long long* __restrict__ table) {
  const int seg = blockIdx.y;
  const float* src = reinterpret_cast<const float*>(table[seg]);
  float* dst = reinterpret_cast<float*>(table[n + seg]);
  const long long words = table[2 * n + seg];
  if (src == nullptr) return;
  const bool vec = ((table[seg] | table[n + seg]) & 15) == 0;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (vec) {
    const long long q = words >> 2;
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(dst);
    for (long long j = i; j < q; j += stride) {
      const float4 x = s4[j];
      float4 d = d4[j];
      d.x += x.x; d.y += x.y; d.z += x.z; d.w += x.w;
      d4[j] = d;
    }
    for (long long j = 4 * q + i; j < words; j += stride) dst[j] = dst[j] + src[j];
  } else {
    for (long long j = i; j < words; j += stride) dst[j] = dst[j] + src[j];
  }
}

// multi_add_k + the sum of squares of every STORED sum, added to st->sumsq exactly as multi_copy_sumsq_k adds it
// (an fp32 partial per thread, fp64 wave and workgroup reduction, one fp64 atomic per workgroup, nothing when the
// partial is 0).  A null-source segment is read and its squares counted: the norm is that of the whole accumulated
// buffer, not of this pass's share.
__global__ __launch_bounds__(256) void multi_add_sumsq_k(int n, const long long* __restrict__ table,
                                                         demf_opt_state* st) {
  __shared__ double part[4];
  const int seg = blockIdx.y;
  const float* src = reinterpret_cast<const float*>(table[seg]);
  float* dst = reinterpret_cast<float*>(table[n + seg]);
  const long long words = table[2 * n + seg];
  const bool vec = ((table[seg] | table[n + seg]) & 15) == 0;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  float acc = 0.f;
  if (src == nullptr) {
    for (long long j = i; j < words; j += stride) {
      const float x = dst[j];
      acc += x * x;
    }
  } else if (vec) {
    const long long q = words >> 2;
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(dst);
    for (long long j = i; j < q; j += stride) {
      const float4 x = s4[j];
      float4 d = d4[j];
      d.x += x.x; d.y += x.y; d.z += x.z; d.w += x.w;
      acc += d.x * d.x + d.y * d.y + d.z * d.z + d.w * d.w;
      d4[j] = d;
    }
    for (long long j = 4 * q + i; j < words; j += stride) {
      const float x = dst[j] + src[j];
      acc += x * x;
      dst[j] = x;
    }
  } else {
    for (long long j = i; j < words; j += stride) {
      const float x = dst[j] + src[j];
      acc += x * x;
      dst[j] = x;
    }
  }
  double d = (double)acc;
  for (int off = 32; off; off >>= 1) d += __shfl_xor(d, off);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) part[w] = d;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = part[0];
    for (int k = 1; k < (int)(blockDim.x >> 6); ++k) s += part[k];
    if (s != 0.0) atomicAdd(&st->sumsq, s);
  }
}

struct ScalarsAccumArgs {
  const float* s[DEMF_METER_MAX_SCALARS];
  int n;
  float* acc;
  float scale;
};

// One wave.  Lane i < n: acc[i] = acc[i] + scale * *s[i] - a rounded product, then a rounded sum (the library is
// built with -ffp-contract=off and this is no fmaf); plain stores, no atomics.
__global__ __launch_bounds__(64) void scalars_accum_k(ScalarsAccumArgs a) {
  const int lane = threadIdx.x;
  const float* p = nullptr;
#pragma unroll
  for (int i = 0; i < DEMF_METER_MAX_SCALARS; ++i)        // (a select chain: no dynamic index into the arguments)
    if (lane == i) p = a.s[i];
  if (lane < a.n) {
    const float prod = a.scale * *p;
    a.acc[lane] = a.acc[lane] + prod;
  }
}

}  // namespace demf

using namespace demf;

extern "C" int demf_multi_add(int n, const void* table, int blocks_per_segment, demf_stream_t stream) {
  DEMF_REQUIRE(n >= 0 && n <= 65535 && blocks_per_segment >= 1, "multi_add: bad arguments");
  if (n == 0) return DEMF_OK;
  DEMF_REQUIRE(table != nullptr, "multi_add: null table");
  hipLaunchKernelGGL(multi_add_k, dim3(blocks_per_segment, n), dim3(256), 0, (hipStream_t)stream, n,
                     (const long long*)table);
  return check_launch("multi_add");
}

extern "C" int demf_multi_add_sumsq(int n, const void* table, int blocks_per_segment, void* opt_state,
                                    demf_stream_t stream) {
  DEMF_REQUIRE(n >= 0 && n <= 65535 && blocks_per_segment >= 1, "multi_add_sumsq: bad arguments");
  if (n == 0) return DEMF_OK;
  DEMF_REQUIRE(table != nullptr && opt_state != nullptr, "multi_add_sumsq: null pointer");
  hipLaunchKernelGGL(multi_add_sumsq_k, dim3(blocks_per_segment, n), dim3(256), 0, (hipStream_t)stream, n,
                     (const long long*)table, (demf_opt_state*)opt_state);
  return check_launch("multi_add_sumsq");
}

extern "C" int demf_scalars_accum(int n, const float* const* scalars, float* acc, float scale,
                                  demf_stream_t stream) {
  DEMF_REQUIRE(n >= 1 && n <= DEMF_METER_MAX_SCALARS, "scalars_accum: n=%d scalars (1..%d supported)", n,
               DEMF_METER_MAX_SCALARS);
  DEMF_REQUIRE(scalars != nullptr && acc != nullptr, "scalars_accum: null pointer");
  ScalarsAccumArgs a;
  for (int i = 0; i < DEMF_METER_MAX_SCALARS; ++i) {
    DEMF_REQUIRE(i >= n || scalars[i] != nullptr, "scalars_accum: null pointer (scalar %d)", i);
    a.s[i] = i < n ? scalars[i] : nullptr;
  }
  a.n = n;
  a.acc = acc;
  a.scale = scale;
  hipLaunchKernelGGL(scalars_accum_k, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
  return check_launch("scalars_accum");
}
