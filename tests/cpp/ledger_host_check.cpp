// The host side of the rumour ledger (include/serf_sim_ledger.h, serf_amd/host/serf.hpp) as a stand-alone program for a sanitizer build
// (-fsanitize=address,undefined on the host, run on a machine without a GPU or with one): the five calls' argument paths with a null
// handle and, where there is no device, with the handle sim_create refuses; the wrapper's sample type.  Prints "ok" and exits 0.
#include <cstdio>
#include <vector>

#include "../../serf_amd/host/serf.hpp"

#define EXPECT(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

int main() {
  const std::vector<sim_ledger_entry> e = {{SIM_K_EVENT, 0x77u, 3}, {SIM_K_LEAVE, 5, 2}, {SIM_K_SUSPECT, 9, 0}};
  std::vector<uint64_t> out(SIM_LEDGER_HEADER_WORDS + e.size() * SIM_LEDGER_ENTRY_WORDS, 77);
  uint32_t taken = 5, dropped = 6, got = 7;
  EXPECT(sim_ledger_version() == SIM_LEDGER_VERSION);
  // a null handle: SIM_EINVAL, nothing written
  EXPECT(sim_ledger_start(nullptr, e.data(), (uint32_t)e.size(), 0, 1, 8) == SIM_EINVAL);
  EXPECT(sim_ledger_start(nullptr, nullptr, 0, 0, 0, 0) == SIM_EINVAL);
  EXPECT(sim_ledger_count(nullptr, &taken, &dropped) == SIM_EINVAL && taken == 5 && dropped == 6);
  EXPECT(sim_ledger_count(nullptr, nullptr, nullptr) == SIM_EINVAL);
  EXPECT(sim_ledger_read(nullptr, 0, 1, out.data(), out.size(), &got) == SIM_EINVAL && got == 7);
  EXPECT(sim_ledger_read(nullptr, 0, 0, nullptr, 0, nullptr) == SIM_EINVAL);
  EXPECT(sim_ledger_stop(nullptr) == SIM_EINVAL);
  EXPECT(sim_ledger_now(nullptr, e.data(), (uint32_t)e.size(), out.data()) == SIM_EINVAL);
  EXPECT(sim_ledger_now(nullptr, nullptr, 0, nullptr) == SIM_EINVAL);
  for (uint64_t w : out) EXPECT(w == 77);
  // the wrapper: a cluster the library refuses (no device) throws before any ledger call; one it grants takes the five calls
  try {
    serf::Cluster cl(serf::Options::lan(64));
    cl.ledger_start(e, 0, 1, 4);
    cl.step(2);
    EXPECT(cl.ledger_count().first == 2);
    const auto s = cl.ledger_read();
    EXPECT(s.size() == 2 && s[1].entries.size() == e.size() && s[1].header[2] == e.size());
    EXPECT(cl.ledger_now(e).entries.size() == e.size());
    cl.ledger_stop();
  } catch (const serf::Error& err) {
    std::fprintf(stderr, "no handle: %s\n", err.what());
  }
  serf::Cluster::LedgerSample s;
  s.entries.resize(2);
  EXPECT(sizeof(s.entries[0]) == 8 * SIM_LEDGER_ENTRY_WORDS && sizeof(s.header) == 8 * SIM_LEDGER_HEADER_WORDS);
  std::puts("ok");
  return 0;
}
