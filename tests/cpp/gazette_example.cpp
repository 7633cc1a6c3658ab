// The member gazette (include/serf_sim_gazette.h) through serf::Cluster (serf_amd/host/serf.hpp): two nodes crash, one leaves; a
// gazette behind every tick is read once at the end and printed, one line per sample, then the totals of both maps and the three
// subjects the most observers announced Failed.
// Output:  <tick> <running> <slots> <fresh> <join> <leave> <failed> <reap> <flap> <suspected> <cleared> <nodes with events> <subjects with events>
//          ...   nodes <rows> <sum of failed> <sum of leave> <largest peak>   subjects <rows> <sum of failed> <sum of leave>
//          top <id> <failed> <peak>   (three lines)
#include <cstdio>
#include <cstdlib>

#include "../../serf_amd/host/serf.hpp"

int main(int argc, char** argv) {
  const uint32_t n = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 4096, ticks = argc > 2 ? (uint32_t)std::atoi(argv[2]) : 160;
  try {
    serf::Cluster cl(serf::Options::lan(n).with_view_slots(64));
    cl.crash(7, 3);
    cl.crash(n / 2, 9);
    cl.gazette_start(0, 1, ticks, 60);
    cl.step(20);
    cl.node(11).leave();
    cl.step(ticks - 20);              // one call; nothing is read while it runs
    const auto cnt = cl.gazette_count();
    if (cnt.first != ticks || cnt.second != 0) { std::fprintf(stderr, "taken %u dropped %u\n", cnt.first, cnt.second); return 1; }
    for (const auto& s : cl.gazette_read()) {
      std::printf("%llu %llu %llu %llu", (unsigned long long)s.w[0], (unsigned long long)s.w[1], (unsigned long long)s.w[2], (unsigned long long)s.w[3]);
      for (int k = 45; k < 52; ++k) std::printf(" %llu", (unsigned long long)s.w[k]);
      std::printf(" %llu %llu\n", (unsigned long long)s.w[52], (unsigned long long)s.w[55]);
    }
    unsigned long long failed = 0, leave = 0, peak = 0;
    const auto nodes = cl.gazette_nodes();
    for (const auto& r : nodes) { failed += r.c[SIM_GAZETTE_FAILED]; leave += r.c[SIM_GAZETTE_LEAVE]; peak = r.c[SIM_GAZETTE_PEAK] > peak ? r.c[SIM_GAZETTE_PEAK] : peak; }
    std::printf("nodes %zu %llu %llu %llu\n", nodes.size(), failed, leave, peak);
    failed = leave = 0;
    const auto subj = cl.gazette_subjects();
    for (const auto& r : subj) { failed += r.c[SIM_GAZETTE_FAILED]; leave += r.c[SIM_GAZETTE_LEAVE]; }
    std::printf("subjects %zu %llu %llu\n", subj.size(), failed, leave);
    for (const auto& r : cl.gazette_top(SIM_GAZETTE_MAP_SUBJECTS, SIM_GAZETTE_FAILED, 3))
      std::printf("top %llu %u %u\n", (unsigned long long)r.id, r.row.c[SIM_GAZETTE_FAILED], r.row.c[SIM_GAZETTE_PEAK]);
    cl.gazette_stop();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
