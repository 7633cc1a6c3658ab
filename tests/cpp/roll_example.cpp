// The observer roll (include/serf_sim_roll.h) through serf::Cluster (serf_amd/host/serf.hpp): two nodes crash, one leaves; a roll
// behind every tick, ranked by the stopped members an observer still holds Alive, is read once at the end and printed, one line per
// sample, then roll_now() once with every node's record.
// Output:  <tick> <running> <subjects> <listed> <rank_by> <current> <sum stale> <holders of a stopped Alive> <their sum> <first listed id>
//          ...   now <same ten>   nodes <records> <running among them> <sum of their stale_alive>
#include <cstdio>
#include <cstdlib>

#include "../../serf_amd/host/serf.hpp"

static void line(const char* pre, const serf::Cluster::RollSample& s) {
  const sim_roll_header& h = s.header;
  std::printf("%s%llu %llu %llu %llu %llu %llu %llu %llu %llu %lld\n", pre, (unsigned long long)h.w[0], (unsigned long long)h.w[1],
              (unsigned long long)h.w[2], (unsigned long long)(h.w[3] & 0xFFFFFFFFu), (unsigned long long)(h.w[3] >> 32), (unsigned long long)h.w[4],
              (unsigned long long)h.w[5], (unsigned long long)h.w[12], (unsigned long long)h.w[13],
              s.top.empty() ? -1ll : (long long)(s.top[0].w[0] & 0xFFFFFFFFu));
}

int main(int argc, char** argv) {
  const uint32_t n = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 4096, ticks = argc > 2 ? (uint32_t)std::atoi(argv[2]) : 160;
  try {
    serf::Cluster cl(serf::Options::lan(n).with_view_slots(64));
    cl.crash(7, 3);
    cl.crash(n / 2, 9);
    cl.roll_start(0, 1, ticks, 4, SIM_ROLL_BY_MISSED);
    cl.step(20);
    cl.node(11).leave();
    cl.step(ticks - 20);              // one call; nothing is read while it runs
    const auto cnt = cl.roll_count();
    if (cnt.first != ticks || cnt.second != 0) { std::fprintf(stderr, "taken %u dropped %u\n", cnt.first, cnt.second); return 1; }
    const auto samples = cl.roll_read();
    for (const auto& s : samples) {
      if (s.top.size() != (s.header.w[3] & 0xFFFFFFFFu) || s.top.size() > 4) return 1;
      line("", s);
    }
    const auto now = cl.roll_now(4, SIM_ROLL_BY_MISSED, true);
    line("now ", now);
    unsigned long long running = 0, missed = 0;
    for (const auto& r : now.nodes) { running += r.w[0] >> 32; missed += r.w[5]; }
    std::printf("nodes %zu %llu %llu\n", now.nodes.size(), running, missed);
    cl.roll_stop();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
