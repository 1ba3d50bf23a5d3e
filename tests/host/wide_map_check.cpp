// Stand-alone host check of csrc/wide_map.h: the block -> (column chunk, slab sequence) mapping and the grid-size
// arithmetic of demf_mlp_bwd_fused_wide.  Built with -fsanitize=address,undefined and run by
// tests/test_wide_map_host.py (no GPU, nothing loaded into Python).  For every (nslab, nchunk, cap):
//   * the grid holds nchunk x members blocks, members <= max(1, cap / nchunk), members <= nslab (no idle block);
//   * every (chunk, slab) pair is visited by exactly one block;
//   * the nchunk blocks that walk the same slabs have ids a run width apart - 8 whenever a chunk has >= 8 members,
//     i.e. they land on the same XCD under the round-robin block -> XCD assignment.
#include <cstdio>
#include <vector>

#include "../../demf_amd/csrc/wide_map.h"

int main() {
  const int nslabs[] = {1, 7, 8, 9, 119, 120, 121, 513, 1024, 8192};
  const int nchunks[] = {2, 3, 4};
  const int caps[] = {8, 240, 256};
  int bad = 0, cases = 0;
  for (int nslab : nslabs)
    for (int nchunk : nchunks)
      for (int cap : caps) {
        ++cases;
        const int gpc = demf::wide_members(nslab, nchunk, cap);
        const int want_max = cap / nchunk > 1 ? cap / nchunk : 1;
        if (gpc < 1 || gpc > nslab || gpc > want_max || (gpc >= 8 && gpc % 8 != 0) ||
            (gpc < 8 && gpc != (want_max < nslab ? want_max : nslab))) {
          std::printf("members: nslab %d nchunk %d cap %d -> %d\n", nslab, nchunk, cap, gpc);
          ++bad;
          continue;
        }
        const int rw = demf::wide_run(gpc);
        if (rw != (gpc >= 8 ? 8 : gpc)) { std::printf("run width %d for %d members\n", rw, gpc); ++bad; }
        std::vector<int> seen((size_t)nchunk * nslab, 0);
        std::vector<int> owner((size_t)nchunk * gpc, -1);      // (chunk, first slab) -> block id
        for (int b = 0; b < nchunk * gpc; ++b) {
          const demf::WideBlock wb = demf::wide_block(b, nchunk, gpc);
          if (wb.chunk < 0 || wb.chunk >= nchunk || wb.first < 0 || wb.first >= gpc || wb.stride != gpc) {
            std::printf("block %d of (%d, %d, %d): chunk %d first %d stride %d\n", b, nslab, nchunk, cap, wb.chunk,
                        wb.first, wb.stride);
            ++bad;
            continue;
          }
          if (owner[(size_t)wb.chunk * gpc + wb.first] != -1) { std::printf("two blocks on one sequence\n"); ++bad; }
          owner[(size_t)wb.chunk * gpc + wb.first] = b;
          for (int s = wb.first; s < nslab; s += wb.stride) ++seen[(size_t)wb.chunk * nslab + s];
        }
        for (int c = 0; c < nchunk; ++c)
          for (int s = 0; s < nslab; ++s)
            if (seen[(size_t)c * nslab + s] != 1) {
              std::printf("(%d, %d, %d): chunk %d slab %d visited %d times\n", nslab, nchunk, cap, c, s,
                          seen[(size_t)c * nslab + s]);
              ++bad;
            }
        for (int c = 1; c < nchunk; ++c)
          for (int w = 0; w < gpc; ++w) {
            const int d = owner[(size_t)c * gpc + w] - owner[(size_t)(c - 1) * gpc + w];
            if (d != rw) {
              std::printf("(%d, %d, %d): member %d of chunks %d / %d is %d blocks apart, not %d\n", nslab, nchunk, cap,
                          w, c - 1, c, d, rw);
              ++bad;
            }
          }
      }
  std::printf("wide_map_check: %d cases, %d failures\n", cases, bad);
  return bad ? 1 : 0;
}
