// What the shared-MLP translation units agree on: the kernel argument block (MlpArgs), the prologue codes, the tile
// and scheduling constants, and - per kernel family that lives in a unit of its own - the two host functions the
// dispatcher (launch_gemm_t, csrc/mlp.hip) calls: a predicate "this form takes the launch" and its launcher.
//
//   csrc/mlp.hip          mlp_gemm_kernel (generic form), the dispatcher, forward / dX entry points, first-layer kernels
//   csrc/mlp_fwd_pc.hip   producer / consumer forward for 128-channel inputs
//   csrc/mlp_fwd_res.hip  weight-resident, barrier-free forward for 64-channel inputs
//   csrc/mlp_tile.hip     few-row forward and input-gradient launches on 64 x 64 tiles
//   csrc/mlp_dw.hip       weight gradients
//   csrc/bn.hip           BatchNorm finalize / pool select / backward reductions
//   csrc/mlp_dev.h        device helpers more than one of them inlines (prologue, pooled epilogue, plane fragments)
#pragma once
#include "common.h"
#include "bn_fin.h"
#include "mfma.h"

namespace demf {

constexpr int MLP_BK = 32;        // K step staged per iteration
constexpr int SCHED_GROUPS = 16;  // counters per dynamically scheduled persistent launch
constexpr int DW_CHUNK = 16;      // 32-row slabs per claim of the weight-gradient kernel
constexpr int DW_MAX_SUB = 32;    // blockIdx.y columns with their own counter
constexpr int SCHED_INTS = 2 * DW_MAX_SUB;   // ints per counter set (>= 2*SCHED_GROUPS + 1)
constexpr int MLP_LD = MLP_BK + 4;  // LDS row stride (floats), +16 B pad
constexpr int MLP_LD3 = 3 * (MLP_BK / 2) + 4;   // Bt row stride of compute mode 2: three bf16 terms
constexpr int MLP_MAXK = 512;
constexpr int FR_NW = 8;          // waves per workgroup of the weight-resident forward (mlp_fwd_res_kernel)
constexpr int PC_K = 128, PC_KB = 256, PC_ROWS = 64;

enum { PRO_NONE = 0, PRO_BNRELU = 1, PRO_DY_DENSE = 2, PRO_DY_SPARSE = 3 };

// per-channel vectors of the backward prologue ("vec5"), struct-of-arrays of length n each:
//   [0] scale  [1] shift  (z = y*scale + shift, ReLU mask)   [2] gi = gamma*invstd
//   [3] a = -gi*invstd*mean(dZ*xhat)   [4] b = -gi*mean(dZ) - a*mean     (dY = gi*dZ + a*y + b)
// (BnFin, bn_finalize_channel: csrc/bn_fin.h)
struct MlpArgs {
  int R, K, N;                 // rows, reduction length, output columns
  int ldx;                     // row stride of X (floats)
  int ldy;                     // row stride of Y (floats)
  const float* X;              // PRO_NONE/BNRELU: input rows; PRO_DY_*: Y_l (pre-BN output)
  const float* G;              // PRO_DY_DENSE: upstream gradient dA_l (R x K)
  const float* dP;             // PRO_DY_SPARSE: pooled gradient (R/ns x K)
  const int* arg;              //                and arg-max slot (R/ns x K)
  int ns;
  const float* vec;            // BNRELU: [scale|shift] (2K);  DY: 5 vectors of length K
  const float* Bt;             // (N x K) row-major; or, with ldb > 0, the (K x >=N) matrix whose
  int ldb;                     // TRANSPOSE is the B operand (row stride ldb): W itself for dX = dY.W
  float* Y;                    // (R x N) output
  double* stats;               // optional (2N): column sum, column sum of squares
  // optional fused pooling epilogue (forward, last layer): per group of ns consecutive rows and
  // column, the max / min of the raw output and the row offset where each is attained
  float* pmax;                 // (R/ns x N) or null
  float* pmin;
  int* amax;
  int* amin;
  int halves;                  // pooled launches: 2 = two column halves interleaved in a 1-D grid
  int st;                      // bf16 STORAGE of the rows (weight-resident forward only): bit 0 X, bit 1 Y
  // FIRST epilogue (backward of a stack whose first layer has a 4-float input and no input
  // gradient): the output tile IS the gradient of layer 0's activation; instead of storing it, the
  // raw sums of layer 0's whole backward are taken from it (see mlp_first_finish_k)
  const float* W0;             // weight-resident forward, ST bit 3: (K x 4) weight of the layer BELOW, whose raw
                               // output is recomputed from its 4-float input rows X instead of being loaded
  const float* fX;             // (R x 4) input rows of layer 0
  const float* fY;             // (R x N) pre-BN output of layer 0
  const float* fss;            // layer 0 [scale|shift] (2N)
  const float* fmi;            // layer 0 [mean|invstd] (2N)
  double* fsum;                // g1(N) | g2(N) | P(N x 4) | Q(N x 4) | cx(4), accumulated
  // RED epilogue (dx GEMM of layer l): besides storing dX = the gradient of layer l-1's activation,
  // layer l-1's BN-backward sums (sum dZ, sum dZ*xhat) are taken from the tile -> stats; the layer
  // l-1 operands are addressed with row stride / vector length fld and column offset fc0
  int fld, fc0;
  int* sched;                  // persistent launches: SCHED_GROUPS tile counters, 1 + SCHED_GROUPS exit counters, or null
  BnFin fin;                   // STATS launches: in-kernel finalize when fin.ss != null
  BnVecFin vfin;               // RED launches: layer l-1's backward vectors by the last workgroup (ticket != null)
};

// ---- kernel families in their own units ----------------------------------------------------------------------------
// *_takes: exactly the condition under which the dispatcher hands the launch to the form.  launch_*: LDS size, the
// one-time LDS reservation (latched per kernel instantiation and device), the instantiation switch, check_launch.
// cm = compute mode of the launch (1 bf16, 2 fp32 as bf16 terms - f16_terms() then picks two fp16 terms instead).
bool fwd_pc_takes(const MlpArgs& a, bool pool);
int launch_fwd_pc(const MlpArgs& a, int cm, bool pool, hipStream_t s);
bool fwd_res_takes(const MlpArgs& a, bool pool);
int launch_fwd_res(const MlpArgs& a, int cm, bool pool, hipStream_t s);
// The tile launchers answer LAUNCH_TRY_NEXT when the device cannot reserve the LDS the form needs: nothing was
// launched and no error is set - the dispatcher goes on to the next form.
constexpr int LAUNCH_TRY_NEXT = -1000;
bool fwd_tile_takes(const MlpArgs& a, bool pro);                       // pro: BN + ReLU prologue (a.vec)
int launch_fwd_tile(const MlpArgs& a, int cm, bool pro, hipStream_t s);
bool dx_tile_takes(const MlpArgs& a, bool sparse, bool red);
int launch_dx_tile(const MlpArgs& a, int cm, bool sparse, bool red, hipStream_t s);
// the stand-alone finalize behind a STATS launch that had no counter set (bn_finalize_kernel, csrc/bn.hip)
int launch_bn_finalize(int N, double* stats, const BnFin& fin, hipStream_t s);

}  // namespace demf
