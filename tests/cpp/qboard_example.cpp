// The query board (include/serf_sim_qboard.h) through serf::Cluster (serf_amd/host/serf.hpp): two queries under packet loss — one to
// everybody with relays, one to four nodes by id — and an id nobody schedules; a node that crashes.  The board sampled behind every
// tick is read once at the end and printed.
// Output:  counts <taken> <dropped>
//          sample <the last sample's 8 + 16 n words>
//          now <a stateless sample's 8 + 16 n words>          of the same ids, in reverse order
//          silent <entry> <which> <total> <the first eight ids>   for every entry, acks and responses
//          top <the record's 8 words>                          the eight nodes with the most silent acks
//          node <the record's 8 words>                         for nodes 0 .. 15
#include <cstdio>
#include <cstdlib>

#include "../../serf_amd/host/serf.hpp"

static void words(const char* pre, const uint64_t* w, size_t n) {
  std::printf("%s", pre);
  for (size_t i = 0; i < n; ++i) std::printf(" %llu", (unsigned long long)w[i]);
  std::printf("\n");
}
static void sample(const char* pre, const serf::Cluster::QBoardSample& s) {
  std::vector<uint64_t> w(s.header, s.header + SIM_QBOARD_HEADER_WORDS);
  for (const auto& e : s.entries) {
    const uint64_t r[SIM_QBOARD_ENTRY_WORDS] = {e.id | (uint64_t)e.state << 32, e.origin | (uint64_t)e.flags << 32, e.deadline, e.acks, e.responses,
                                               e.eligible, e.answered, e.responded, e.silent, e.new_acks, e.new_responses,
                                               e.t_first, e.t_half, e.t_90, e.t_99, e.t_all};
    w.insert(w.end(), r, r + SIM_QBOARD_ENTRY_WORDS);
  }
  words(pre, w.data(), w.size());
}

int main(int argc, char** argv) {
  const uint32_t n = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 512, ticks = argc > 2 ? (uint32_t)std::atoi(argv[2]) : 40;
  try {
    serf::Cluster cl(serf::Options::lan(n).with_view_slots(64).with_packet_loss(0.25));
    const std::vector<uint32_t> ids = {0x51, 0x52, 0x53};
    cl.qboard_start(ids, 0, 1, ticks);  // the ids first, then the queries: none of them runs yet
    cl.node(5).query(0x51, SIM_F_ACK | SIM_F_RESPOND | (2u << 8));
    cl.node(105).query(0x52, SIM_F_ACK, {1, 2, 3, n / 2}, 0xFFFFFFFFu);
    cl.crash(n / 2, 6);
    cl.step(ticks);                     // one call; nothing is read while it runs
    const auto cnt = cl.qboard_count();
    std::printf("counts %u %u\n", cnt.first, cnt.second);
    const auto samples = cl.qboard_read();
    if (samples.size() != cnt.first || samples.empty()) return 1;
    sample("sample", samples.back());
    sample("now", cl.qboard_now({0x53, 0x52, 0x51}));
    for (uint32_t e = 0; e < ids.size(); ++e)
      for (uint32_t which = 0; which < 2; ++which) {
        const auto s = cl.qboard_silent(e, which, 8);
        std::printf("silent %u %u %u", e, which, s.second);
        for (uint32_t id : s.first) std::printf(" %u", id);
        std::printf("\n");
      }
    for (const auto& r : cl.qboard_top(8, SIM_QBOARD_BY_SILENT_ACK).top) words("top", r.w, SIM_QBOARD_NODE_WORDS);
    for (const auto& r : cl.qboard_nodes(0, n < 16 ? n : 16)) words("node", r.w, SIM_QBOARD_NODE_WORDS);
    cl.qboard_stop();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
