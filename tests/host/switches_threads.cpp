// Stand-alone host program for tests/test_switch_table_host.py: eight threads take their first look at the switch
// table (csrc/switches.h) at once - the use the thread-local compute-mode stack promises - and every one of them must
// see the same, fully parsed table.  Built together with csrc/switches.hip (host code only) under -fsanitize=thread.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <thread>
#include <vector>

#include "../../demf_amd/csrc/switches.h"
#include "../../include/demf_hip.h"

int main() {
  setenv("DEMF_FWD_RES", "0", 1);
  setenv("DEMF_PERSIST_CUS", "256", 1);
  unsetenv("DEMF_PERSIST_CUS_BWD");
  constexpr int T = 8;
  std::atomic<int> ready{0}, bad{0};
  std::vector<std::thread> threads;
  for (int t = 0; t < T; ++t)
    threads.emplace_back([&] {
      ready.fetch_add(1);
      while (ready.load() < T) {}          // all eight reach the first call together
      const demf::Switches& s = demf::sw();
      if (s.fwd_res != 0 || s.persist_cus != 256 || s.persist_cus_bwd != 256 || s.fwd_pc != 1) bad.fetch_add(1);
      const char* name = nullptr;
      int value = 0, dflt = 0, n = 0;
      while (demf_switch_at(n, &name, &value, &dflt) == DEMF_OK) {
        if (!strcmp(name, "DEMF_FWD_RES") && (value != 0 || dflt != 1)) bad.fetch_add(1);
        ++n;
      }
      if (n < 60 || &s != &demf::sw()) bad.fetch_add(1);
    });
  for (auto& th : threads) th.join();
  printf("%d threads, %d failures\n", T, bad.load());
  return bad.load() ? 1 : 0;
}
