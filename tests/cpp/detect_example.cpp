// The detection log (include/serf_sim_detect.h) through serf::Cluster (serf_amd/host/serf.hpp): two nodes crash, one of them comes
// back, one member leaves; a log behind every tick is read once at the end and printed.
// Output:  counts <taken> <dropped> <written> <lost>
//          header <the last sample's 64 words>
//          episode <its 8 words>     for every log record, then     open <its 8 words>     for every episode still open
#include <cstdio>
#include <cstdlib>

#include "../../serf_amd/host/serf.hpp"

static void words(const char* pre, const uint64_t* w, unsigned n) {
  std::printf("%s", pre);
  for (unsigned i = 0; i < n; ++i) std::printf(" %llu", (unsigned long long)w[i]);
  std::printf("\n");
}

int main(int argc, char** argv) {
  const uint32_t n = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 4096, ticks = argc > 2 ? (uint32_t)std::atoi(argv[2]) : 160;
  try {
    serf::Cluster cl(serf::Options::lan(n).with_view_slots(64));
    cl.crash(7, 3);
    cl.crash(n / 2, 9);
    cl.revive(7, 60);
    cl.detect_start(0, 1, ticks, 64);
    cl.step(20);
    cl.node(11).leave();
    cl.step(ticks - 20);              // one call; nothing is read while it runs
    const auto cnt = cl.detect_count();
    const auto lc = cl.detect_log_count();
    std::printf("counts %u %u %llu %llu\n", cnt.first, cnt.second, (unsigned long long)lc.first, (unsigned long long)lc.second);
    const auto hdr = cl.detect_read();
    if (hdr.size() != cnt.first || hdr.empty()) return 1;
    words("header", hdr.back().w, SIM_DETECT_WORDS);
    for (const auto& e : cl.detect_log()) words("episode", e.w, SIM_DETECT_EPISODE_WORDS);
    for (const auto& e : cl.detect_open()) words("open", e.w, SIM_DETECT_EPISODE_WORDS);
    cl.detect_stop();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
