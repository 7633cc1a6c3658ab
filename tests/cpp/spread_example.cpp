// The spread map (include/serf_sim_spread.h) through serf::Cluster (serf_amd/host/serf.hpp): three user events from three nodes under
// packet loss, a node that crashes; the map latched behind every tick is read once at the end and printed.
// Output:  counts <taken> <dropped>
//          sample <the last sample's 8 + 8 n words>
//          summary <its 40 words>              for every entry
//          unreached <entry> <total> <the first ids>      for every entry
//          top <its 8 words>                   for the eight worst running nodes by missed entries
//          map <entry 0's arrivals of nodes 0 .. 15>
#include <cstdio>
#include <cstdlib>

#include "../../serf_amd/host/serf.hpp"

static void words(const char* pre, const uint64_t* w, size_t n) {
  std::printf("%s", pre);
  for (size_t i = 0; i < n; ++i) std::printf(" %llu", (unsigned long long)w[i]);
  std::printf("\n");
}

int main(int argc, char** argv) {
  const uint32_t n = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 512, ticks = argc > 2 ? (uint32_t)std::atoi(argv[2]) : 40;
  try {
    serf::Cluster cl(serf::Options::lan(n).with_view_slots(64).with_packet_loss(0.25));
    std::vector<sim_spread_entry> entries;
    for (uint32_t i = 0; i < 3; ++i)  // (an event's Lamport time is its origin's event clock when it is sent)
      entries.push_back(sim_spread_entry{SIM_K_EVENT, 0x5A000000u + i, cl.node(5 + 100 * i).stats().event_time});
    entries.push_back(sim_spread_entry{SIM_K_JOIN, n - 1, 1});
    cl.crash(n / 2, 6);
    cl.spread_start(entries, 0, 1, ticks);
    for (uint32_t i = 0; i < 3; ++i) cl.node(5 + 100 * i).user_event(0x5A000000u + i, 64);
    cl.step(ticks);                   // one call; nothing is read while it runs
    const auto cnt = cl.spread_count();
    std::printf("counts %u %u\n", cnt.first, cnt.second);
    const auto samples = cl.spread_read();
    if (samples.size() != cnt.first || samples.empty()) return 1;
    std::vector<uint64_t> last(samples.back().header, samples.back().header + SIM_SPREAD_HEADER_WORDS);
    for (const auto& e : samples.back().entries) {
      const uint64_t w[8] = {e.id, e.val, e.latched, e.reached, e.reached_up, e.holds, e.first, e.last};
      last.insert(last.end(), w, w + 8);
    }
    words("sample", last.data(), last.size());
    for (const auto& s : cl.spread_summary(2)) words("summary", reinterpret_cast<const uint64_t*>(&s), SIM_SPREAD_SUMMARY_WORDS);
    for (uint32_t e = 0; e < entries.size(); ++e) {
      const auto un = cl.spread_unreached(e, 4);
      std::printf("unreached %u %u", e, un.second);
      for (uint32_t id : un.first) std::printf(" %u", id);
      std::printf("\n");
    }
    for (const auto& r : cl.spread_late(8, SIM_SPREAD_BY_MISSED).top) words("top", r.w, SIM_SPREAD_NODE_WORDS);
    std::printf("map");
    for (uint32_t a : cl.spread_map(0, 0, n < 16 ? n : 16)) std::printf(" %u", a);
    std::printf("\n");
    cl.spread_stop();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
