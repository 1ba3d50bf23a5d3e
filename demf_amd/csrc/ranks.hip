// Rank merges: what a data-parallel run does with the per-rank device state AFTER the transport has gathered it.
// Both entry points take already-gathered device arrays (rank-major, W slabs of one shape) and contain no
// communication, so a single process can test them; demf_amd/ranks.py puts the collective in front.
//
//   demf_store_concat  W DetectionStores (the arrays demf_detect_pack appends to) -> one store in rank order.  The
//                      scene counts are the host's, the row counts the device's: the grid covers the worst case
//                      (every rank full) and workgroups whose share lies beyond the rows that exist leave at once.
//   demf_meter_merge   W step-meter rings (csrc/meter.hip's row layout) -> one ring whose scalars are the mean over
//                      ranks, taken in fp64 in ascending rank order.
//
// Neither kernel has atomics or a cursor: every destination word has exactly one writer, so a merge is bit-identical
// from run to run.
#include <hip/hip_runtime.h>

#include "common.h"

namespace demf {

// DEMF_RANKS_MAX bounds W of either merge: the per-rank tables travel in the kernel arguments
constexpr int CONCAT_THREADS = 256;
constexpr int CONCAT_MAX_BLOCKS = 1024;   // workgroups per rank; a workgroup strides over its rank's words

struct ConcatArgs {
  int n[DEMF_RANKS_MAX];      // scenes of rank r
  int first[DEMF_RANKS_MAX];  // scenes of the ranks before r
  int W, S, R;                // ranks, per-rank scene capacity, per-rank row capacity
  int total_scenes;
  const int* src_off;      // (W, S+1)
  const int* src_state;    // (W, 2)
  const unsigned* src_boxes;   // (W, R, 7) as words
  const unsigned* src_scores;  // (W, R)
  const unsigned* src_labels;  // (W, R)
  int max_rows;
  unsigned* boxes;
  unsigned* scores;
  unsigned* labels;
  int* scene_off;
  int* state;
};

// grid (P, W), 256 threads.  Every workgroup reads the W row counts (lane q of the first wave: scene_off[q][n_q]),
// takes the exclusive prefix for its own rank from LDS and copies a strided share of the rank's words.
__global__ __launch_bounds__(CONCAT_THREADS) void store_concat_k(ConcatArgs a) {
  __shared__ int rows_s[DEMF_RANKS_MAX];
  __shared__ int flag_s[DEMF_RANKS_MAX];
  const int tid = threadIdx.x;
  const int r = blockIdx.y;
  if (tid < DEMF_RANKS_MAX) {
    int rows = 0, flag = 0;
    if (tid < a.W) {
      rows = a.src_off[(size_t)tid * (a.S + 1) + a.n[tid]];
      if (rows < 0) rows = 0;                         // (a negative cursor reads as an empty rank)
      flag = a.src_state[2 * tid + 1] != 0;
    }
    rows_s[tid] = rows;
    flag_s[tid] = flag;
  }
  __syncthreads();
  long long base = 0;
  for (int q = 0; q < r; ++q) base += rows_s[q];
  const int rows_r = rows_s[r];
  // rows of this rank that exist (not beyond its capacity) and have a place (below max_rows) in the destination
  long long room = (long long)a.max_rows - base;
  if (room < 0) room = 0;
  long long copy = rows_r < a.R ? rows_r : a.R;
  if (copy > room) copy = room;

  const long long stride = (long long)gridDim.x * CONCAT_THREADS;
  const long long start = (long long)blockIdx.x * CONCAT_THREADS + tid;
  // scene offsets of this rank: global scene first[r] + i
  for (long long i = start; i < a.n[r]; i += stride) {
    const long long v = base + a.src_off[(size_t)r * (a.S + 1) + i];
    a.scene_off[a.first[r] + i] = (int)v;
  }
  if (r == 0 && blockIdx.x == 0 && tid == 0) {
    long long total = 0;
    int over = 0;
    for (int q = 0; q < a.W; ++q) {
      total += rows_s[q];
      over |= flag_s[q];
    }
    if (total > (long long)a.max_rows) over = 1;
    a.scene_off[a.total_scenes] = (int)total;
    a.state[0] = (int)total;
    a.state[1] = over;
  }
  if (start >= copy * 7) return;                      // (the worst-case grid: nothing of this rank is left for us)
  const unsigned* sb = a.src_boxes + (size_t)r * a.R * 7;
  unsigned* db = a.boxes + (size_t)base * 7;
  for (long long i = start; i < copy * 7; i += stride) db[i] = sb[i];
  const unsigned* ss = a.src_scores + (size_t)r * a.R;
  const unsigned* sl = a.src_labels + (size_t)r * a.R;
  unsigned* ds = a.scores + (size_t)base;
  unsigned* dl = a.labels + (size_t)base;
  for (long long i = start; i < copy; i += stride) {
    ds[i] = ss[i];
    dl[i] = sl[i];
  }
}

// One thread per word of the merged ring (16 consecutive lanes = one 64-byte row).
__global__ __launch_bounds__(256) void meter_merge_k(int W, int rows, const unsigned* rings, unsigned* out) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)rows * DEMF_METER_ROW_WORDS) return;
  const int w = (int)(idx % DEMF_METER_ROW_WORDS);
  const size_t row0 = (size_t)(idx - w);              // first word of the row in rank 0's ring
  const size_t slab = (size_t)rows * DEMF_METER_ROW_WORDS;
  const unsigned mine0 = rings[row0 + w];
  if (W == 1) {                                       // a copy, bit for bit
    out[idx] = mine0;
    return;
  }
  const unsigned t_lo = rings[row0], t_hi = rings[row0 + 1];
  bool agree = true;
  unsigned ored = 0;
  double sum = 0.0;
  for (int r = 0; r < W; ++r) {
    const unsigned* p = rings + (size_t)r * slab + row0;
    agree = agree && p[0] == t_lo && p[1] == t_hi;
    const unsigned v = p[w];
    ored |= v;
    sum += (double)__builtin_bit_cast(float, v);
  }
  unsigned res;
  if (!agree) res = w < 2 ? 0xffffffffu : 0u;         // the row of an empty ring: stamp -1, every other word 0
  else if (w == 2) res = ored;
  else if (w < DEMF_METER_HEAD_WORDS) res = mine0;    // stamp, lr_factor, grad_norm, clip: rank 0's
  else res = __builtin_bit_cast(unsigned, (float)(sum / (double)W));
  out[idx] = res;
}

}  // namespace demf

using namespace demf;

extern "C" int demf_store_concat(int W, const int* counts, int S, int R, const int* src_scene_off,
                                 const int* src_state, const float* src_boxes, const float* src_scores,
                                 const int* src_labels, int max_scenes, int max_rows, float* boxes, float* scores,
                                 int* labels, int* scene_off, int* state, demf_stream_t stream) {
  DEMF_REQUIRE(W >= 1 && S >= 1 && R >= 0 && max_scenes >= 1 && max_rows >= 0,
               "store_concat: bad sizes (W=%d S=%d R=%d max_scenes=%d max_rows=%d)", W, S, R, max_scenes, max_rows);
  if (W > DEMF_RANKS_MAX) {
    set_error("store_concat: W=%d ranks (at most %d supported)", W, DEMF_RANKS_MAX);
    return DEMF_EUNSUPPORTED;
  }
  DEMF_REQUIRE(counts != nullptr && src_scene_off != nullptr && src_state != nullptr && scene_off != nullptr &&
                   state != nullptr,
               "store_concat: null pointer");
  DEMF_REQUIRE(R == 0 || (src_boxes != nullptr && src_scores != nullptr && src_labels != nullptr),
               "store_concat: null pointer (source rows)");
  DEMF_REQUIRE(max_rows == 0 || R == 0 || (boxes != nullptr && scores != nullptr && labels != nullptr),
               "store_concat: null pointer (destination rows)");
  DEMF_REQUIRE((long long)R * 7 < (1ll << 31) && (long long)max_rows * 7 < (1ll << 33),
               "store_concat: too many rows for the offsets (R=%d max_rows=%d)", R, max_rows);
  ConcatArgs a;
  long long scenes = 0;
  for (int r = 0; r < DEMF_RANKS_MAX; ++r) {
    const int n = r < W ? counts[r] : 0;
    DEMF_REQUIRE(n >= 0 && n <= S, "store_concat: rank %d holds %d scenes, its capacity is %d", r, n, S);
    a.n[r] = n;
    a.first[r] = (int)scenes;
    scenes += n;
    DEMF_REQUIRE(scenes <= max_scenes, "store_concat: %lld scenes do not fit the destination's %d", scenes,
                 max_scenes);
  }
  a.W = W;
  a.S = S;
  a.R = R;
  a.total_scenes = (int)scenes;
  a.src_off = src_scene_off;
  a.src_state = src_state;
  a.src_boxes = (const unsigned*)src_boxes;
  a.src_scores = (const unsigned*)src_scores;
  a.src_labels = (const unsigned*)src_labels;
  a.max_rows = max_rows;
  a.boxes = (unsigned*)boxes;
  a.scores = (unsigned*)scores;
  a.labels = (unsigned*)labels;
  a.scene_off = scene_off;
  a.state = state;
  const long long words = (long long)R * 7 > S ? (long long)R * 7 : S;
  long long P = (words + CONCAT_THREADS * 4 - 1) / (CONCAT_THREADS * 4);    // ~4 words of the widest array a thread
  if (P < 1) P = 1;
  if (P > CONCAT_MAX_BLOCKS) P = CONCAT_MAX_BLOCKS;
  hipLaunchKernelGGL(store_concat_k, dim3((unsigned)P, (unsigned)W), dim3(CONCAT_THREADS), 0, (hipStream_t)stream, a);
  return check_launch("store_concat");
}

extern "C" int demf_meter_merge(int W, int rows, const void* rings, void* out, demf_stream_t stream) {
  DEMF_REQUIRE(W >= 1 && rows >= 1, "meter_merge: bad sizes (W=%d rows=%d)", W, rows);
  if (W > DEMF_RANKS_MAX) {
    set_error("meter_merge: W=%d ranks (at most %d supported)", W, DEMF_RANKS_MAX);
    return DEMF_EUNSUPPORTED;
  }
  DEMF_REQUIRE(rings != nullptr && out != nullptr, "meter_merge: null pointer");
  DEMF_REQUIRE((long long)W * rows * DEMF_METER_ROW_WORDS < (1ll << 31), "meter_merge: %d rings of %d rows", W, rows);
  const int blocks = cdiv(rows * DEMF_METER_ROW_WORDS, 256);
  hipLaunchKernelGGL(meter_merge_k, dim3(blocks), dim3(256), 0, (hipStream_t)stream, W, rows, (const unsigned*)rings,
                     (unsigned*)out);
  return check_launch("meter_merge");
}
