// The rumour tree (include/serf_sim_tree.h) through serf::Cluster (serf_amd/host/serf.hpp): three user events from three nodes under
// packet loss, a node that crashes; the tree latched behind every tick is read once at the end and printed.
// Output:  counts <taken> <dropped>
//          sample <the last sample's 8 + 8 n words>
//          summary <its 72 words>                          for every entry
//          top <id> <running> <arrival> <parent> <hop> <children>    for the eight nodes with the most children in entry 0's tree
//          path <entry> <total> <the ids>                  for every entry: the chain of the last node
//          link <arrival> <parent> <hop> <children>        for nodes 0 .. 15 of entry 0
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
    std::vector<sim_tree_entry> entries;
    for (uint32_t i = 0; i < 3; ++i)  // (an event's Lamport time is its origin's event clock when it is sent)
      entries.push_back(sim_tree_entry{SIM_K_EVENT, 0x5A000000u + i, cl.node(5 + 100 * i).stats().event_time});
    cl.crash(n / 2, 6);
    cl.tree_start(entries, 0, ticks);
    for (uint32_t i = 0; i < 3; ++i) cl.node(5 + 100 * i).user_event(0x5A000000u + i, 64);
    cl.step(ticks);                   // one call; nothing is read while it runs
    const auto cnt = cl.tree_count();
    std::printf("counts %u %u\n", cnt.first, cnt.second);
    const auto samples = cl.tree_read();
    if (samples.size() != cnt.first || samples.empty()) return 1;
    std::vector<uint64_t> last(samples.back().header, samples.back().header + SIM_TREE_HEADER_WORDS);
    for (const auto& e : samples.back().entries) {
      const uint64_t w[8] = {e.id, e.val, e.latched, e.new_orphans, e.reached, e.orphans, e.copies, e.fresh};
      last.insert(last.end(), w, w + 8);
    }
    words("sample", last.data(), last.size());
    for (const auto& s : cl.tree_summary()) words("summary", reinterpret_cast<const uint64_t*>(&s), SIM_TREE_SUMMARY_WORDS);
    for (const auto& r : cl.tree_top(0, 8))
      std::printf("top %u %u %u %u %u %u\n", r.id, r.running, r.link.arrival, r.link.parent, r.link.hop, r.link.children);
    for (uint32_t e = 0; e < entries.size(); ++e) {
      const auto p = cl.tree_path(e, n - 1);
      std::printf("path %u %u", e, p.second);
      for (uint32_t id : p.first) std::printf(" %u", id);
      std::printf("\n");
    }
    for (const auto& l : cl.tree_links(0, 0, n < 16 ? n : 16)) std::printf("link %u %u %u %u\n", l.arrival, l.parent, l.hop, l.children);
    cl.tree_stop();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
