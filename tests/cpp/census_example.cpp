// The membership census (include/serf_sim_census.h) through serf::Cluster (serf_amd/host/serf.hpp): two nodes crash, one leaves;
// a census behind every tick is read once at the end and printed, one line per sample, then census_now() once.
// Output:  <tick> <running> <subjects> <stored> <settled> <stopped-but-Alive> <fully detected>   ...   now <same seven>
#include <cstdio>
#include <cstdlib>

#include "../../serf_amd/host/serf.hpp"

static void line(const char* pre, const sim_census_header& h) {
  std::printf("%s%llu %llu %llu %llu %llu %llu %llu\n", pre, (unsigned long long)h.w[0], (unsigned long long)h.w[1], (unsigned long long)h.w[2],
              (unsigned long long)h.w[3], (unsigned long long)h.w[4], (unsigned long long)h.w[9], (unsigned long long)h.w[11]);
}

int main(int argc, char** argv) {
  const uint32_t n = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 4096, ticks = argc > 2 ? (uint32_t)std::atoi(argv[2]) : 160;
  try {
    serf::Cluster cl(serf::Options::lan(n).with_view_slots(64));
    cl.crash(7, 3);
    cl.crash(n / 2, 9);
    cl.census_start(0, 1, ticks, 2);  // two records a sample: the third subject shows in the header only
    cl.step(20);
    cl.node(11).leave();
    cl.step(ticks - 20);              // one call; nothing is read while it runs
    const auto cnt = cl.census_count();
    if (cnt.first != ticks || cnt.second != 0) { std::fprintf(stderr, "taken %u dropped %u\n", cnt.first, cnt.second); return 1; }
    const auto samples = cl.census_read();
    for (const auto& s : samples) {
      if (s.subjects.size() != s.header.w[3]) return 1;
      line("", s.header);
    }
    const auto now = cl.census_now(64);
    line("now ", now.header);
    for (const auto& r : now.subjects)
      std::printf("subject %u slot %u running %llu failed %llu left %llu\n", (unsigned)(r.w[0] & 0xFFFFFFFFu), (unsigned)(r.w[0] >> 32),
                  (unsigned long long)r.w[1], (unsigned long long)r.w[6], (unsigned long long)r.w[5]);
    cl.census_stop();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
