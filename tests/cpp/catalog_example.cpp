// The rumour catalogue (include/serf_sim_catalog.h) through serf::Cluster (serf_amd/host/serf.hpp): node 11 sends one user event, node 7
// crashes — nobody names the SUSPECT and DEAD records the cluster makes about it.  A catalogue behind every tick is read once at the
// end: a line per sample, a line per registry record, then catalog_now() once, and the ledger on what the catalogue found.
// Output:  <tick> <running> <live> <overflow> <new> <died> <revived> <registry> <lost> <queued> <in flight>
//          ...   id <kind> <key> <val> <first seen> <last seen> <samples> <revivals> <peak queued> <copies>
//          ...   now <tick> <live> <rows>   ledger <entries> <mismatches>
#include <cstdio>
#include <cstdlib>

#include "../../serf_amd/host/serf.hpp"

int main(int argc, char** argv) {
  const uint32_t n = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 4096, ticks = argc > 2 ? (uint32_t)std::atoi(argv[2]) : 160;
  try {
    serf::Cluster cl(serf::Options::lan(n).with_view_slots(64));
    const uint32_t key = 0x43415441u;
    cl.crash(7, 3);
    cl.catalog_start(SIM_CATALOG_KINDS, 64, 0, 1, ticks);
    cl.node(11).user_event(key, 64, false);
    cl.step(ticks / 2);
    const auto mid = cl.catalog_live();     // the live table behind the latest tick, and the GPU's own ledger on the same identities
    std::vector<sim_ledger_entry> entries;
    for (const auto& e : mid)
      if (entries.size() < SIM_LEDGER_MAX) entries.push_back({(uint32_t)(e.id >> 32), (uint32_t)e.id, e.val});
    unsigned bad = 0;
    if (!entries.empty()) {
      const auto led = cl.ledger_now(entries);
      for (size_t i = 0; i < entries.size(); ++i)
        bad += led.entries[i].holders != mid[i].holders || led.entries[i].queued != mid[i].queued || led.entries[i].in_flight != mid[i].in_flight;
    }
    cl.step(ticks - ticks / 2);       // nothing is read while it runs
    const auto cnt = cl.catalog_count();
    if (cnt.first != ticks || cnt.second != 0) { std::fprintf(stderr, "taken %u dropped %u\n", cnt.first, cnt.second); return 1; }
    for (const auto& s : cl.catalog_read())
      std::printf("%llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)s.w[0], (unsigned long long)s.w[1],
                  (unsigned long long)s.w[2], (unsigned long long)s.w[3], (unsigned long long)s.w[4], (unsigned long long)s.w[5],
                  (unsigned long long)s.w[6], (unsigned long long)s.w[7], (unsigned long long)s.w[8], (unsigned long long)s.w[9],
                  (unsigned long long)s.w[10]);
    for (const auto& r : cl.catalog_list())
      std::printf("id %u %u %llu %u %u %u %u %u %llu\n", r.kind(), r.key(), (unsigned long long)r.val, r.first_seen, r.last_seen, r.samples,
                  r.revivals, r.peak_queued, (unsigned long long)r.in_flight_sum);
    const auto now = cl.catalog_now();
    std::printf("now %llu %llu %zu\n", (unsigned long long)now.sample.w[0], (unsigned long long)now.sample.w[2], now.live.size());
    std::printf("ledger %zu %u\n", entries.size(), bad);
    cl.catalog_stop();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
