// Process- and thread-wide launch state of libdemf_hip.so, used by every family of matrix kernels:
//   - the compute mode of the dense kernels (process default + a per-thread stack of contexts) and the
//     two-fp16-term switch: compute_mode(), compute_bf16(), f16_terms() of csrc/common.h, with their entry points
//     demf_set_compute_dtype / demf_set_f16_terms / demf_ctx_push / demf_ctx_pop / demf_get_compute_dtype and the
//     *_ctx wrappers that run one call under a context;
//   - the two device rings launches draw from: self-resetting counter sets (sched_slot) and zeroed blocks of
//     replicated accumulators (accum_slot), declared in csrc/bn_fin.h.  The rings live HERE, next to the functions
//     that resolve their address; kernels only ever receive the pointers.
// No kernel in this unit.
#include "mlp_args.h"
#include <atomic>

namespace demf {

// Compute mode of the dense kernels (demf_set_compute_dtype):
//   0 = fp32 MFMA (v_mfma_f32_32x32x2_f32, the reference's precision);
//   1 = bf16 MFMA with fp32 accumulate (v_mfma_f32_32x32x16_bf16): operands are rounded to bf16 (RNE,
//       v_cvt_pk_bf16_f32) on their way into LDS, AFTER the fp32 prologue (BN + ReLU / BN-backward);
//       everything stored to memory, every statistic, index and loss stays fp32.  BASELINE configs[3];
//   2 = fp32 operands split into three bf16 terms each (x = h + m + l exactly: 3 x 8 significand
//       bits) and the six products h.h, h.m, m.h, m.m, h.l, l.h accumulated in fp32 on the bf16 MFMA
//       (the dropped m.l, l.m, l.l terms are <= 2^-23 relative - the rounding of one fp32 FMA).
//       On gfx950 the bf16 MFMA runs 16x the fp32 one, so six of them cost 3/8 of the native fp32
//       issue time at fp32-grade results (tests/test_gpu_split.py measures both against fp64).
// Until demf_set_compute_dtype is called the mode is 2, or 0 with DEMF_F32_NATIVE=1 in the environment.
static std::atomic<int> g_compute_mode{-1};
// demf_ctx_push / demf_ctx_pop: the calling THREAD's mode for the calls in between (a stack, so library code
// may nest them); -1 = the process default below.  Two host threads driving two models in different modes do
// not see each other's setting.
constexpr int CTX_DEPTH = 8;
static thread_local int tl_mode_stack[CTX_DEPTH];
static thread_local int tl_mode_top = 0;
int compute_mode() {
  if (tl_mode_top > 0 && tl_mode_stack[tl_mode_top - 1] >= 0) return tl_mode_stack[tl_mode_top - 1];
  int m = g_compute_mode.load(std::memory_order_relaxed);
  if (m < 0) {
    m = sw().f32_native ? 0 : 2;
    g_compute_mode.store(m);
  }
  return m;
}
bool compute_bf16() { return compute_mode() == 1; }
// (demf_set_f16_terms; until it is called: on, or off with DEMF_F16_TERMS=0 in the environment)
static std::atomic<int> g_f16_terms{-1};
bool f16_terms() {
  int on = g_f16_terms.load(std::memory_order_relaxed);
  if (on < 0) {
    on = sw().f16_terms != 0;
    g_f16_terms.store(on);
  }
  return on && compute_mode() == 2;
}

// Counter sets {next tile per group, finished blocks} of the dynamically scheduled persistent
// launches.  A launch takes the next set of a ring; the last block of the launch leaves it zeroed, so
// a captured launch can be replayed with the set it was given.  Launches that share a set are
// 1024 launches apart on the calling thread's stream order (the MLP path is single-stream).
// (Both rings start on a 128-byte line, so a 256-byte counter set covers two lines and a copy of the accumulators
// whole ones.  The 326-kernel unit they used to live in happened to place them so; alone in a unit they landed 16 bytes
// into a line, and the step measured 0.4 % slower in 8 of 8 alternating pairs.)
constexpr int SCHED_SLOTS = 1024;
__device__ __attribute__((aligned(128))) int g_tile_sched[SCHED_INTS * SCHED_SLOTS];
int* sched_slot() {
  static int* base = nullptr;
  static std::atomic<unsigned> next{0};
  if (base == nullptr) {
    void* ptr = nullptr;
    if (hipGetSymbolAddress(&ptr, HIP_SYMBOL(g_tile_sched)) != hipSuccess) return nullptr;
    base = (int*)ptr;
  }
  if (sw().static_tiles) return nullptr;     // A/B switch
  return base + SCHED_INTS * (next.fetch_add(1) % SCHED_SLOTS);
}

// Blocks of zeroed doubles for the replicated accumulators (csrc/bn_fin.h): as the counter sets, the next block of a
// ring; the launch's last workgroup leaves it zeroed.
constexpr int ACC_SLOTS = 128;
__device__ __attribute__((aligned(128))) double g_accum_ring[(size_t)ACC_SLOT_DOUBLES * ACC_SLOTS];
double* accum_slot() {
  static double* base = nullptr;
  static std::atomic<unsigned> next{0};
  if (base == nullptr) {
    void* ptr = nullptr;
    if (hipGetSymbolAddress(&ptr, HIP_SYMBOL(g_accum_ring)) != hipSuccess) return nullptr;
    base = (double*)ptr;
  }
  if (!sw().acc_repl) return nullptr;     // A/B switch
  return base + (size_t)ACC_SLOT_DOUBLES * (next.fetch_add(1) % ACC_SLOTS);
}

}  // namespace demf

using namespace demf;

extern "C" int demf_set_compute_dtype(int mode) {
  DEMF_REQUIRE(mode >= 0 && mode <= 2, "set_compute_dtype: 0 = fp32, 1 = bf16, 2 = fp32 as three bf16 terms");
  g_compute_mode.store(mode);
  return DEMF_OK;
}

extern "C" int demf_set_f16_terms(int on) {
  g_f16_terms.store(on ? 1 : 0);
  return DEMF_OK;
}

extern "C" int demf_ctx_push(const demf_ctx* ctx) {
  DEMF_REQUIRE(ctx != nullptr, "ctx_push: null context");
  DEMF_REQUIRE(ctx->compute_mode >= -1 && ctx->compute_mode <= 2,
               "ctx_push: compute_mode -1 (process default), 0 fp32, 1 bf16, 2 fp32 as three bf16 terms");
  DEMF_REQUIRE(tl_mode_top < CTX_DEPTH, "ctx_push: more than %d nested contexts on this thread", CTX_DEPTH);
  tl_mode_stack[tl_mode_top++] = ctx->compute_mode;
  return DEMF_OK;
}

extern "C" int demf_ctx_pop(void) {
  DEMF_REQUIRE(tl_mode_top > 0, "ctx_pop: no context pushed on this thread");
  --tl_mode_top;
  return DEMF_OK;
}

extern "C" int demf_get_compute_dtype(void) { return compute_mode(); }

namespace {
struct CtxScope {          // the *_ctx entry points: the context for exactly one call
  bool pushed;
  explicit CtxScope(const demf_ctx* c) : pushed(c != nullptr && demf_ctx_push(c) == DEMF_OK) {}
  ~CtxScope() { if (pushed) demf_ctx_pop(); }
};
}  // namespace

extern "C" int demf_mlp_gemm_fwd(int, int, int, int, const float*, const float*, const float*, float*, double*,
                                 demf_stream_t);
extern "C" int demf_mlp_gemm_fwd_ctx(const demf_ctx* ctx, int R, int K, int N, int ldx, const float* X,
                                     const float* pro_scale_shift, const float* Wt, float* Y, double* stats,
                                     demf_stream_t stream) {
  DEMF_REQUIRE(ctx != nullptr, "mlp_gemm_fwd_ctx: null context");
  CtxScope scope(ctx);
  if (!scope.pushed) return DEMF_EINVAL;
  return demf_mlp_gemm_fwd(R, K, N, ldx, X, pro_scale_shift, Wt, Y, stats, stream);
}

extern "C" int demf_gemm_f32(const demf_gemm_desc*, demf_stream_t);
extern "C" int demf_gemm_f32_ctx(const demf_ctx* ctx, const demf_gemm_desc* desc, demf_stream_t stream) {
  DEMF_REQUIRE(ctx != nullptr, "gemm_f32_ctx: null context");
  CtxScope scope(ctx);
  if (!scope.pushed) return DEMF_EINVAL;
  return demf_gemm_f32(desc, stream);
}

extern "C" int demf_gemm_group_f32(const demf_gemm_desc*, int, demf_stream_t);
extern "C" int demf_gemm_group_f32_ctx(const demf_ctx* ctx, const demf_gemm_desc* descs, int n, demf_stream_t stream) {
  DEMF_REQUIRE(ctx != nullptr, "gemm_group_f32_ctx: null context");
  CtxScope scope(ctx);
  if (!scope.pushed) return DEMF_EINVAL;
  return demf_gemm_group_f32(descs, n, stream);
}
