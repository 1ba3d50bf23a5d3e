// The one definition of the switch table (csrc/switches.h): the only place in the library that reads the environment.
// Host code only - no HIP call, so tests/host/switches_threads.cpp builds it into a stand-alone program.
#include <stdlib.h>

#include "../../include/demf_hip.h"
#include "switches.h"

namespace demf {

namespace {
struct Entry { const char* name; int dflt; int Switches::*field; };
#define DEMF_SW_ENTRY(field, name, dflt, meaning) {name, dflt, &Switches::field},
constexpr Entry TABLE[] = {DEMF_SWITCHES(DEMF_SW_ENTRY)};
#undef DEMF_SW_ENTRY
constexpr int COUNT = sizeof(TABLE) / sizeof(TABLE[0]);

Switches read_environment() {
  Switches s;
  for (const Entry& e : TABLE) {
    const char* v = getenv(e.name);
    s.*e.field = v ? atoi(v) : e.dflt;
  }
  // the fused backwards' block count: its own variable, else the forwards', else that one's default
  if (!getenv("DEMF_PERSIST_CUS_BWD")) s.persist_cus_bwd = s.persist_cus;
  return s;
}
}  // namespace

const Switches& sw() {
  static const Switches s = read_environment();
  return s;
}

}  // namespace demf

extern "C" int demf_switch_at(int index, const char** name, int* value, int* dflt) {
  if (index < 0 || index >= demf::COUNT) return DEMF_EINVAL;
  const demf::Entry& e = demf::TABLE[index];
  if (name) *name = e.name;
  if (value) *value = demf::sw().*e.field;
  if (dflt) *dflt = e.dflt;
  return DEMF_OK;
}
