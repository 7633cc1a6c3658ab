/*
 * serf_sim_detect.h — detection log on the device: for every member that owns a view slot, the episodes in which it was down
 * (when the crash was first suspected, when half, 99 % and all of the running nodes knew) and the episodes in which it ran
 * and was accused (how far the accusation got, whether it was refuted), judged behind the sampled ticks without a host poll
 * and without naming a subject in advance.
 *
 * The sixth extension of include/serf_sim.h, in the style of include/serf_sim_census.h: exported by the HIP library
 * (libserf_sim.so) only, with a version of its own (sim_detect_version), not part of SIM_ABI_VERSION.  The CPU oracle has no
 * detection log: it is the checker — every word below is a pure fold over the census records (include/serf_sim_census.h) of
 * the sampled ticks (tests/detect_model.py over tests/census_model.py).
 *
 * The trackers (include/serf_sim_track.h) latch the same ticks for subjects registered beforehand, SIM_TRACK_MAX at a time;
 * the census shows the state at a sampled tick but not when an accusation began or how it ended.  The detection log is the
 * census with memory: behind every sampled tick the census's count and fold kernels produce every allocated slot's record on
 * scratch of the log's own, and one more kernel runs a small state machine per view slot over them — at most one open episode
 * a slot, with the trackers' latches — writes a header of cumulative figures and appends every episode that closed to a log
 * on the device, in (sample, ascending slot) order.  A churn run is one sim_step(h, n) and one read of the log.  The log adds
 * no protocol state: digests, events, dumps and checkpoint images do not know it, and a handle that never started one
 * allocates, launches and synchronises nothing for it.
 *
 * Checkpoints: sim_snapshot holds no detection log, sim_restore leaves a running one as it is (sampling rule: as the
 * census's).  Its episodes go on being judged by the samples taken afterwards; a slot whose subject is gone or another one
 * behind the restore closes ABANDONED.  A dropped sample is an evaluation not made.
 *
 * Out of scope: sharded handles (SIM_ESTATE from every call, as the census); subjects without a view slot.
 *
 * EVALUATION.  Behind a sampled tick every view slot a below the highest slot bound the log has seen since it started is
 * evaluated, in ascending order, on the census's inputs for that tick: now = sim_tick after the tick, R = running nodes, and
 * for a slot with a subject (a below the current bound and subject_of[a] a node) its census record w: run = w[1] & 1,
 * failed = w[6], left = w[5], susp = w[8] + w[9], gone = failed + left.  Per slot the log keeps the subject, prev_run, a
 * `done` flag and at most one open episode.  In order:
 *   1. Subject change.  The stored subject differs from the slot's subject now, or there is none now: an open episode closes
 *      ABANDONED, the state is cleared.  No subject now: the slot is done for this sample.  Otherwise the state is FRESH for
 *      the rest of this evaluation.
 *   2. The subject runs.  An open DOWN episode closes RETURNED; `done` is cleared.  With susp > 0 || failed > 0: unless an
 *      ACCUSED episode is open one opens (opened = now; flag AFTER_RETURN when a DOWN episode closed just above); then
 *      first_failed latches now when failed > 0, peak = max(peak, failed), peak_susp = max(peak_susp, susp), evaluated += 1.
 *      With both 0 an open ACCUSED episode closes CLEARED.
 *   3. The subject is stopped.  With no DOWN episode open, `done` clear and the state fresh or prev_run == 1: an open ACCUSED
 *      episode closes STOPPED and a DOWN episode opens (opened = now; flag CENSORED when the state is fresh and this is the
 *      log's first sample: the subject may have stopped long before).  On the open DOWN episode, each latched once, those on
 *      `gone` only while R > 0 (the trackers' rules): first_suspect when susp > 0 || failed > 0, first_failed when failed > 0,
 *      half when 2 gone >= R, p99 when 100 gone >= 99 R, all when gone == R; peak = max(peak, gone), peak_susp = max(peak_susp,
 *      susp), evaluated += 1.  When `all` has latched the episode closes DETECTED and `done` is set: a subject that stays
 *      down opens nothing more until it has been seen running.
 *   4. prev_run = run.
 * A slot closes at most two episodes in one evaluation (ABANDONED or STOPPED, then DETECTED), logged in that order.
 */
#ifndef SERF_SIM_DETECT_H
#define SERF_SIM_DETECT_H

#include <stddef.h>

#include "serf_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIM_DETECT_VERSION 1u
#define SIM_DETECT_WORDS 64u               /* a sample's header: 64 x uint64_t = 512 bytes */
#define SIM_DETECT_EPISODE_WORDS 8u        /* an episode: 8 x uint64_t = 64 bytes */
#define SIM_DETECT_MAX_SAMPLES (1u << 20)
#define SIM_DETECT_MAX_LOG (1u << 24)
#define SIM_DETECT_NEVER 0xFFFFFFFFu       /* a tick that has not been latched; `closed` of an open episode */

enum { SIM_DETECT_DOWN = 1, SIM_DETECT_ACCUSED = 2 };                                   /* kind */
enum { SIM_DETECT_OPEN = 0, SIM_DETECT_DETECTED = 1, SIM_DETECT_RETURNED = 2, SIM_DETECT_CLEARED = 3, SIM_DETECT_STOPPED = 4,
       SIM_DETECT_ABANDONED = 5 };                                                       /* outcome */
enum { SIM_DETECT_F_CENSORED = 1, SIM_DETECT_F_AFTER_RETURN = 2 };                      /* flags */

/* One episode (low 32 bits | high 32 bits):
 *   0   subject | slot
 *   1   kind | outcome << 8 | flags << 16   |   0
 *   2   opened | closed (SIM_DETECT_NEVER while open)
 *   3   first_suspect (ACCUSED: = opened) | first_failed
 *   4   half | p99                  (ACCUSED: SIM_DETECT_NEVER)
 *   5   all (ACCUSED: SIM_DETECT_NEVER) | evaluated
 *   6   peak       DOWN: the most observers that held the subject Failed or Left; ACCUSED: Failed
 *   7   peak_susp  the most observers that held it Suspect or Dead
 * All ticks are values of sim_tick AFTER the sampled tick, as the trackers' latches. */
typedef struct sim_detect_episode { uint64_t w[SIM_DETECT_EPISODE_WORDS]; } sim_detect_episode;

/* One sample = one header; every cumulative word counts since sim_detect_start and includes what the log lost.
 *   0-2     sim_tick after the tick, running nodes, subjects (allocated slots)
 *   3, 4    open DOWN / open ACCUSED episodes after this evaluation
 *   5       episodes closed by this evaluation
 *   6, 7    log records written / lost so far
 *   8-12    episodes closed so far by outcome 1 .. 5
 *   13      ACCUSED episodes closed so far with first_failed != SIM_DETECT_NEVER (false declarations)
 *   14, 15  DOWN / ACCUSED episodes opened so far
 *   16-31   histogram of first_suspect - opened over the DETECTED episodes that are not CENSORED
 *   32-47   histogram of all - opened over the same episodes
 *   48-63   histogram of closed - opened over the CLEARED episodes
 * The bin of x is x == 0 ? 0 : min(15, 1 + floor(log2 x)); a DETECTED episode whose first_suspect never latched (every
 * observer holds the subject Left, nobody Suspect, Dead or Failed) counts in bin 15 of words 16-31. */
typedef struct sim_detect_header { uint64_t w[SIM_DETECT_WORDS]; } sim_detect_header;

/* Errors of all calls: SIM_EINVAL for null pointers, period == 0, capacity == 0 or > SIM_DETECT_MAX_SAMPLES, log_capacity == 0
 * or > SIM_DETECT_MAX_LOG, a read beyond what was taken / written (or into a buffer that is too small); SIM_ESTATE on a sharded
 * handle, between sim_step_begin and sim_step_end, for a start while a log is running and for a read / open / stop without
 * one; SIM_ENOMEM when the buffers cannot be allocated.  A call that fails changes nothing. */

/* A sample is taken behind tick t (the tick during which sim_tick was t) when t >= first_tick, (t - first_tick) % period
 * == 0 and fewer than `capacity` samples have been taken; one that is due with the buffer full is dropped and counted.
 * A first_tick that has passed already means "now" (the handle's tick).  The log keeps the first log_capacity episodes that
 * close — always the exact prefix — and counts the later ones as lost. */
int sim_detect_start(sim_handle*, uint32_t first_tick, uint32_t period, uint32_t capacity, uint32_t log_capacity);
/* Samples taken / dropped so far: the host knows every sampled tick in advance, so this waits for nothing.  Both are 0
 * on a handle without a detection log. */
int sim_detect_count(const sim_handle*, uint32_t* taken, uint32_t* dropped);
/* Waits for the handle's stream, then copies the headers of samples first .. first + n - 1 (first + n <= taken) into
 * out[cap_words] (n * SIM_DETECT_WORDS <= cap_words); *n_out = n. */
int sim_detect_read(sim_handle*, uint32_t first, uint32_t n, uint64_t* out, size_t cap_words, uint32_t* n_out);
/* Waits for the handle's stream: log records written / lost so far.  Both are 0 on a handle without a detection log. */
int sim_detect_log_count(sim_handle*, uint64_t* written, uint64_t* lost);
/* Waits for the handle's stream, then copies log records first .. first + n - 1 (first + n <= written, n <= cap) into
 * out[cap]; *n_out = n. */
int sim_detect_log_read(sim_handle*, uint64_t first, uint32_t n, sim_detect_episode* out, uint32_t cap, uint32_t* n_out);
/* Waits for the handle's stream: the episodes still open, in ascending slot order, closed = SIM_DETECT_NEVER and outcome 0,
 * into out[cap] (SIM_EINVAL when there are more than cap; out may be null when cap == 0); *n_out = how many. */
int sim_detect_open(sim_handle*, sim_detect_episode* out, uint32_t cap, uint32_t* n_out);
/* Frees the buffers; samples, log and open episodes are gone. */
int sim_detect_stop(sim_handle*);
uint32_t sim_detect_version(void);

#ifdef __cplusplus
}
#endif
#endif
