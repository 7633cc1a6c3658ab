// The rumour ledger (include/serf_sim_ledger.h) through serf::Cluster (serf_amd/host/serf.hpp): node 11 sends one user event, node 7
// crashes; a ledger of the event and of the SUSPECT and DEAD records about node 7, behind every tick, is read once at the end and
// printed, one line per sample, then ledger_now() once with the event alone.
// Output:  <tick> <running> <n> <queued> <in flight> <packets>  <event: reach holders queued transmits in-flight fresh>  <queued SUSPECT> <queued DEAD>
//          ...   now <tick> <running> <n> <reach> <queued> <in flight>   sent <the sum of the event's in-flight column>
#include <cstdio>
#include <cstdlib>

#include "../../serf_amd/host/serf.hpp"

int main(int argc, char** argv) {
  const uint32_t n = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 4096, ticks = argc > 2 ? (uint32_t)std::atoi(argv[2]) : 160;
  try {
    serf::Cluster cl(serf::Options::lan(n).with_view_slots(64));
    const uint32_t key = 0x4C454447u;
    const uint64_t ltime = cl.node(11).stats().event_time;  // the Lamport time the origin is about to give it
    cl.crash(7, 3);
    const std::vector<sim_ledger_entry> entries = {{SIM_K_EVENT, key, ltime}, {SIM_K_SUSPECT, 7, 0}, {SIM_K_DEAD, 7, 0}};
    cl.ledger_start(entries, 0, 1, ticks);
    cl.node(11).user_event(key, 64, false);
    cl.step(ticks);                   // one call; nothing is read while it runs
    const auto cnt = cl.ledger_count();
    if (cnt.first != ticks || cnt.second != 0) { std::fprintf(stderr, "taken %u dropped %u\n", cnt.first, cnt.second); return 1; }
    unsigned long long sent = 0;
    for (const auto& s : cl.ledger_read()) {
      if (s.entries.size() != 3 || s.entries[0].id != ((uint64_t)key | ((uint64_t)SIM_K_EVENT << 32)) || s.entries[0].val != ltime) return 1;
      const auto& e = s.entries[0];
      std::printf("%llu %llu %llu %llu %llu %llu  %llu %llu %llu %llu %llu %llu  %llu %llu\n", (unsigned long long)s.header[0],
                  (unsigned long long)s.header[1], (unsigned long long)s.header[2], (unsigned long long)s.header[3],
                  (unsigned long long)s.header[4], (unsigned long long)s.header[5], (unsigned long long)e.reach, (unsigned long long)e.holders,
                  (unsigned long long)e.queued, (unsigned long long)e.transmits, (unsigned long long)e.in_flight, (unsigned long long)e.fresh,
                  (unsigned long long)s.entries[1].queued, (unsigned long long)s.entries[2].queued);
      sent += e.in_flight;
    }
    const auto now = cl.ledger_now({entries[0]});
    std::printf("now %llu %llu %llu %llu %llu %llu\n", (unsigned long long)now.header[0], (unsigned long long)now.header[1],
                (unsigned long long)now.header[2], (unsigned long long)now.entries[0].reach, (unsigned long long)now.entries[0].queued,
                (unsigned long long)now.entries[0].in_flight);
    std::printf("sent %llu\n", sent);
    cl.ledger_stop();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
