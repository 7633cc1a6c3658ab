// The traffic meter (include/serf_sim_traffic.h) through serf::Cluster (serf_amd/host/serf.hpp): three user events from three nodes
// under packet loss, a node that crashes; the map accumulated behind every tick is read once at the end and printed.
// Output:  counts <taken> <dropped>
//          sample <the last sample's 64 words>
//          summary <its 40 words>              for tx_units and rx_units, bins of 16 units
//          top <id> <running> <its 8 columns>  for the eight nodes the most units were addressed to
//          node <its 8 columns>                for nodes 0 .. 15
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
    cl.crash(n / 2, 6);
    cl.traffic_start(0, 1, ticks);
    for (uint32_t i = 0; i < 3; ++i) cl.node(5 + 100 * i).user_event(0x5A000000u + i, 64);
    cl.step(ticks);                   // one call; nothing is read while it runs
    const auto cnt = cl.traffic_count();
    std::printf("counts %u %u\n", cnt.first, cnt.second);
    const auto samples = cl.traffic_read();
    if (samples.size() != cnt.first || samples.empty()) return 1;
    words("sample", samples.back().w, SIM_TRAFFIC_WORDS);
    for (uint32_t column : {SIM_TRAFFIC_TX_UNITS, SIM_TRAFFIC_RX_UNITS}) {
      const auto s = cl.traffic_summary(column, 16);
      words("summary", reinterpret_cast<const uint64_t*>(&s), SIM_TRAFFIC_SUMMARY_WORDS);
    }
    for (const auto& r : cl.traffic_top(8, SIM_TRAFFIC_RX_UNITS)) {
      std::printf("top %u %u", r.id, r.running);
      for (uint32_t c : r.node.col) std::printf(" %u", c);
      std::printf("\n");
    }
    for (const auto& r : cl.traffic_nodes(0, n < 16 ? n : 16)) {
      std::printf("node");
      for (uint32_t c : r.col) std::printf(" %u", c);
      std::printf("\n");
    }
    cl.traffic_stop();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
