// Grid arithmetic of the one-launch backward over (column chunk x row range) - demf_mlp_bwd_fused_wide,
// csrc/mlp_bwd.hip.  Plain integer code shared by the launch, the kernel and a host-only check
// (tests/host/wide_map_check.cpp), so it includes nothing and compiles as C++ or HIP.
//
// A layer whose input has nchunk x 128 channels is walked by nchunk x gpc workgroups: workgroup
// (chunk c, member w) takes the 32-row slabs w, w + gpc, w + 2 gpc, ... of column chunk c.  Block ids are
// laid out in runs of `rw` members: [run 0: chunk 0 members 0..rw-1 | chunk 1 members 0..rw-1 | ...][run 1: ...],
// with rw = 8 whenever there are at least 8 members per chunk.  Workgroups go to the 8 XCDs round-robin by
// block id, so the nchunk workgroups that walk the SAME slabs (members w of every chunk, block ids 8 apart)
// share an XCD and therefore an L2: the second and later reads of the slab's dY operands (Y_l, G) hit there -
// as the forward's co-scheduled column halves do (csrc/mlp.hip, `halves`).
#pragma once

#if defined(__HIPCC__)
#define DEMF_WM_HD __host__ __device__ __forceinline__
#else
#define DEMF_WM_HD static inline
#endif

namespace demf {

struct WideBlock {
  int chunk;    // column chunk of this workgroup
  int first;    // its first slab
  int stride;   // distance between its slabs = workgroups per chunk
};

// workgroups per chunk: at most cap / nchunk and at most one per slab; a multiple of 8 from 8 up (full runs)
DEMF_WM_HD int wide_members(int nslab, int nchunk, int cap) {
  int g = cap / nchunk;
  if (g > nslab) g = nslab;
  if (g < 1) g = 1;
  if (g >= 8) g -= g % 8;
  return g;
}

// members per run of block ids
DEMF_WM_HD int wide_run(int gpc) { return gpc >= 8 ? 8 : gpc; }

// block id (0 .. nchunk * gpc) -> its chunk and slab sequence
DEMF_WM_HD WideBlock wide_block(int block, int nchunk, int gpc) {
  const int rw = wide_run(gpc);
  const int run = block / (rw * nchunk), within = block % (rw * nchunk);
  WideBlock b;
  b.chunk = within / rw;
  b.first = run * rw + within % rw;
  b.stride = gpc;
  return b;
}

}  // namespace demf
