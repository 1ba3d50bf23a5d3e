// Step meter: one 64-byte record per optimizer step in a device-resident ring, so that a training loop can log
// its loss terms, gradient norm and clip coefficient without waiting for the GPU at every step (mmcv's
// TextLoggerHook reads them with .item(), a host sync per step).  The launch sits between the point where the
// squared gradient norm is complete in the optimizer's device state (demf_multi_copy_sumsq / demf_sumsq_f32) and
// the demf_adamw_state_f32 launch that consumes and clears it (csrc/optim.hip), in the step's stream or as a node
// of its hipGraph.  A row is a pure function of the step's inputs: no running sums, no cursor, no atomics - a
// replayed or resumed step count overwrites its own row, and a capture warm-up that runs no update writes nothing.
#include <hip/hip_runtime.h>

#include "common.h"

namespace demf {

struct MeterArgs {
  const float* s[DEMF_METER_MAX_SCALARS];
  int n;
  const demf_opt_state* st;
  float grad_scale, max_norm;
  unsigned* ring;
  int rows;
};

__device__ __forceinline__ bool non_finite(float v) { return !(fabsf(v) <= 3.402823466e+38f); }

// One wave.  Lane w < 16 produces word w of the row and the 16 lanes store the row as one 64-byte line; lanes
// 6 .. 6 + n - 1 each load one scalar, the ballot of their non-finite tests is the flag word.
__global__ __launch_bounds__(64) void step_meter_k(MeterArgs a) {
  const int lane = threadIdx.x;
  const int k = lane - DEMF_METER_HEAD_WORDS;
  const float* p = nullptr;
#pragma unroll
  for (int i = 0; i < DEMF_METER_MAX_SCALARS; ++i)        // (a select chain: no dynamic index into the arguments)
    if (k == i) p = a.s[i];
  const bool mine = k >= 0 && k < a.n;
  const float v = mine ? *p : 0.f;
  const unsigned long long bad = __ballot(mine && non_finite(v));
  const long long t = a.st->t;
  // the expressions of adamw_state_k, term by term
  const float norm = (float)sqrt(a.st->sumsq);
  const float grad_norm = norm * a.grad_scale;
  float clip = 1.f;
  if (a.max_norm > 0.f) {
    const float c = a.max_norm / (norm * a.grad_scale + 1e-6f);
    clip = c < 1.f ? c : 1.f;
  }
  unsigned flags = (unsigned)(bad >> DEMF_METER_HEAD_WORDS) & ((1u << DEMF_METER_MAX_SCALARS) - 1u);
  if (non_finite(grad_norm)) flags |= DEMF_METER_FLAG_GRAD_NORM;
  unsigned w;
  switch (lane) {
    case 0: w = (unsigned)((unsigned long long)t & 0xffffffffull); break;
    case 1: w = (unsigned)((unsigned long long)t >> 32); break;
    case 2: w = flags; break;
    case 3: w = __builtin_bit_cast(unsigned, a.st->lr_factor); break;
    case 4: w = __builtin_bit_cast(unsigned, grad_norm); break;
    case 5: w = __builtin_bit_cast(unsigned, clip); break;
    default: w = __builtin_bit_cast(unsigned, v); break;
  }
  long long row = t % (long long)a.rows;
  if (row < 0) row += a.rows;
  if (lane < DEMF_METER_ROW_WORDS) a.ring[(size_t)row * DEMF_METER_ROW_WORDS + lane] = w;
}

}  // namespace demf

using namespace demf;

extern "C" int demf_step_meter(int n, const float* const* scalars, const void* opt_state, float grad_scale,
                               float max_norm, void* ring, int rows, demf_stream_t stream) {
  DEMF_REQUIRE(n >= 1 && n <= DEMF_METER_MAX_SCALARS, "step_meter: n=%d scalars (1..%d supported)", n,
               DEMF_METER_MAX_SCALARS);
  DEMF_REQUIRE(rows >= 1, "step_meter: ring of %d rows", rows);
  DEMF_REQUIRE(scalars != nullptr && opt_state != nullptr && ring != nullptr, "step_meter: null pointer");
  MeterArgs a;
  for (int i = 0; i < DEMF_METER_MAX_SCALARS; ++i) {
    DEMF_REQUIRE(i >= n || scalars[i] != nullptr, "step_meter: null pointer (scalar %d)", i);
    a.s[i] = i < n ? scalars[i] : nullptr;
  }
  a.n = n;
  a.st = (const demf_opt_state*)opt_state;
  a.grad_scale = grad_scale;
  a.max_norm = max_norm;
  a.ring = (unsigned*)ring;
  a.rows = rows;
  hipLaunchKernelGGL(step_meter_k, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
  return check_launch("step_meter");
}
