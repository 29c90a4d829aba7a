// group_check.cpp — the host side of the replication groups under AddressSanitizer + UBSan
// (make asan, tests/test_group_stats.py): fognet_rep_metrics' floor rule against the plain 128-bit
// quotient over the edge cases and seeded random values, the host twins (add_rep, merge, job) against
// each other on any split of the records, and fognet_write_sca_groups through its paths.
// Usage: group_check <scratch dir>.  No GPU, no library: linked with stats_host.cpp and io.cpp.
#include <inttypes.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "fognet_hip.h"
#include "fognet_io.h"

static int g_fail = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                                   \
    }                                                             \
  } while (0)

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static fognet_rep_stats blank() {
  fognet_rep_stats s;
  memset(&s, 0, sizeof s);
  s.queue_min_raw = s.resp_min_ticks = s.abort_tick = INT64_MAX;
  s.queue_max_raw = s.resp_max_ticks = s.last_tick = INT64_MIN;
  s.abort_task = -1;
  return s;
}

// floor(n / d), d > 0, by the language's truncating division
static bool floor_ref(__int128 n, int64_t d, int64_t* q) {
  __int128 t = n / d;
  if (n % d != 0 && n < 0) t -= 1;
  if (t < (__int128)INT64_MIN || t > (__int128)INT64_MAX) return false;
  *q = (int64_t)t;
  return true;
}

static void check_queue_mean(__int128 sum, int64_t n) {
  fognet_rep_stats s = blank();
  s.n_qtime = n;
  s.queue_sum_lo = (uint64_t)(unsigned __int128)sum;
  s.queue_sum_hi = (uint64_t)((unsigned __int128)sum >> 64);
  int64_t v[FOGNET_REP_METRICS];
  uint32_t def = 0, ovf = 0;
  fognet_rep_metrics(&s, v, &def, &ovf);
  const uint32_t bit = 1u << FOGNET_METRIC_QUEUE_MEAN;
  if (n <= 0) {
    CHECK(!(def & bit) && !(ovf & bit) && v[FOGNET_METRIC_QUEUE_MEAN] == INT64_MIN);
    return;
  }
  int64_t q = 0;
  const bool fits = floor_ref(sum, n, &q);
  CHECK(((def & bit) != 0) == fits && ((ovf & bit) != 0) == !fits);
  CHECK(v[FOGNET_METRIC_QUEUE_MEAN] == (fits ? q : INT64_MIN));
}

static void check_resp_mean(unsigned __int128 sum, int64_t n) {
  fognet_rep_stats s = blank();
  s.n_tasks = n;
  s.resp_sum_lo = (uint64_t)sum;
  s.resp_sum_hi = (uint64_t)(sum >> 64);
  int64_t v[FOGNET_REP_METRICS];
  uint32_t def = 0, ovf = 0;
  fognet_rep_metrics(&s, v, &def, &ovf);
  const uint32_t bit = 1u << FOGNET_METRIC_RESP_MEAN;
  const unsigned __int128 q = sum / (unsigned __int128)n;
  const bool fits = q <= (unsigned __int128)INT64_MAX;
  CHECK(((def & bit) != 0) == fits && ((ovf & bit) != 0) == !fits);
  CHECK(v[FOGNET_METRIC_RESP_MEAN] == (fits ? (int64_t)q : INT64_MIN));
}

static void check_energy(double e, bool fits, int64_t want) {
  fognet_rep_stats s = blank();
  s.energy_j = e;
  int64_t v[FOGNET_REP_METRICS];
  uint32_t def = 0, ovf = 0;
  fognet_rep_metrics(&s, v, &def, &ovf);
  const uint32_t bit = 1u << FOGNET_METRIC_ENERGY_UJ;
  CHECK(((def & bit) != 0) == fits && ((ovf & bit) != 0) == !fits);
  CHECK(v[FOGNET_METRIC_ENERGY_UJ] == (fits ? want : INT64_MIN));
}

static fognet_rep_stats random_rep() {
  fognet_rep_stats s = blank();
  s.status = rnd() % 8 == 0 ? (int32_t)(1 + rnd() % 10) : FOGNET_OK;
  if (rnd() % 8 == 0) s.abort_tick = (int64_t)(rnd() >> 4);
  s.n_tasks = (int64_t)(rnd() % 5000);
  s.n_queued = (int64_t)(rnd() % (uint64_t)(s.n_tasks + 1));
  s.n_started = s.n_tasks - s.n_queued;
  s.events = s.n_tasks * 14;
  s.n_qtime = s.n_queued;
  s.n_qtime_overflow = (int64_t)(rnd() % 2);
  s.last_tick = (int64_t)(rnd() >> 8);
  s.queue_min_raw = (int64_t)rnd();
  s.queue_max_raw = (int64_t)rnd();
  s.resp_min_ticks = (int64_t)rnd();
  s.resp_max_ticks = (int64_t)rnd();
  s.queue_sum_lo = rnd(), s.queue_sum_hi = rnd() % 4 == 0 ? ~(uint64_t)0 : rnd() >> 40;
  s.queue_sq_lo = rnd(), s.queue_sq_hi = rnd(), s.queue_sq_top = rnd();
  s.resp_sum_lo = rnd(), s.resp_sum_hi = rnd() % 3 == 0 ? rnd() >> 58 : 0u, s.resp_sq_lo = rnd(), s.resp_sq_hi = rnd();
  s.max_pending = (int32_t)(rnd() % 4096);
  s.busy_s = (int64_t)(rnd() >> 20);
  s.energy_j = (double)(rnd() >> 20) * 1e-3;
  return s;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: group_check <scratch dir>\n");
    return 2;
  }
  const std::string dir = argv[1];

  // ---- the floor rule: edge cases, then random values
  const __int128 two127 = (__int128)1 << 126;
  const __int128 kSums[] = {0, 1, -1, 7, -7, -8, INT64_MAX, (__int128)INT64_MAX + 1, INT64_MIN, (__int128)INT64_MIN - 1,
                            -two127 - two127 /* -2^127 */, two127 + (two127 - 1) /* 2^127 - 1 */, -two127, two127};
  const int64_t kDiv[] = {-1, 0, 1, 2, 3, 7, 1000000, INT64_MAX, INT64_MAX - 1, (int64_t)1 << 62, ((int64_t)1 << 62) + 1};
  for (const __int128 s : kSums)
    for (const int64_t d : kDiv) {
      check_queue_mean(s, d);
      if (d > 0) check_resp_mean((unsigned __int128)s, d);
    }
  for (int i = 0; i < 2000000; ++i) {
    const unsigned shift = (unsigned)(rnd() % 128);
    const unsigned __int128 raw = (((unsigned __int128)rnd() << 64) | rnd()) >> shift;
    const __int128 sum = rnd() % 2 ? (__int128)raw : -(__int128)(raw >> 1) - 1;
    const int64_t d = (int64_t)(((rnd() >> 1) >> (rnd() % 63)) | 1u);
    check_queue_mean(sum, d);
    check_resp_mean(raw, d);
  }

  // ---- toInt64(energy_j * 1e6)
  check_energy(0.0, true, 0);
  check_energy(-0.0, true, 0);
  check_energy(1.5, true, 1500000);
  check_energy(2.5e-6, true, 3);    // the product lands exactly on .5: floor(x + 0.5) rounds up
  check_energy(0.5e-6, true, 1);
  check_energy(-0.5e-6, true, 0);
  check_energy(-12.25, true, -12250000);
  check_energy(9.2e12, true, (int64_t)floor(9.2e12 * 1e6 + 0.5));
  check_energy(9.3e12, false, 0);
  check_energy(-9.3e12, false, 0);
  check_energy(NAN, false, 0);
  check_energy(INFINITY, false, 0);
  check_energy(-INFINITY, false, 0);

  // ---- add_rep / merge / job: any split of the records merges to the whole
  std::vector<fognet_rep_stats> reps;
  for (int i = 0; i < 300; ++i) reps.push_back(random_rep());
  fognet_group_stats whole;
  fognet_group_stats_init(&whole);
  for (const fognet_rep_stats& s : reps) fognet_group_stats_add_rep(&whole, &s);
  for (int parts = 1; parts <= 7; ++parts) {
    std::vector<fognet_group_stats> part((size_t)parts);
    for (fognet_group_stats& p : part) fognet_group_stats_init(&p);
    for (size_t i = 0; i < reps.size(); ++i) fognet_group_stats_add_rep(&part[rnd() % (uint64_t)parts], &reps[i]);
    fognet_group_stats acc;
    fognet_group_stats_init(&acc);
    for (const fognet_group_stats& p : part) fognet_group_stats_merge(&acc, &p);
    CHECK(memcmp(&acc, &whole, sizeof acc) == 0);
  }
  fognet_group_stats empty;
  fognet_group_stats_init(&empty);
  CHECK(empty.n_reps == 0 && empty.queue.min_raw == INT64_MAX && empty.across[8].max_raw == INT64_MIN);
  fognet_job_stats job;
  fognet_group_stats_job(&whole, &job);
  CHECK(job.n_reps == 300 && job.n_failed == whole.n_failed && job.n_tasks == whole.n_tasks);
  CHECK(job.n_qtime == whole.queue.count && job.busy_s == (int64_t)whole.across[FOGNET_METRIC_BUSY_S].sum_lo);
  fognet_group_stats_job(&empty, &job);
  CHECK(job.n_reps == 0 && job.max_pending == 0 && job.last_tick == INT64_MIN && job.energy_j == 0.0);
  // null arguments are ignored
  fognet_group_stats_init(NULL);
  fognet_group_stats_add_rep(NULL, &reps[0]);
  fognet_group_stats_add_rep(&whole, NULL);
  fognet_group_stats_merge(&whole, NULL);
  fognet_group_stats_job(NULL, &job);
  fognet_rep_metrics(NULL, NULL, NULL, NULL);

  // ---- the writer
  const std::string path = dir + "/groups.sca";
  CHECK(fognet_write_sca_groups(path.c_str(), "run", "Net", 1, &whole, NULL, 0) == FOGNET_OK);
  fognet_group_stats three[3] = {whole, empty, whole};
  three[2].across[FOGNET_METRIC_MAX_PENDING].overflow = 4;  // (a metric that loses nothing by itself)
  const char* names[3] = {"Net.a", "Net.b", "Net.c"};
  CHECK(fognet_write_sca_groups(path.c_str(), "run", "Net", 3, three, names, 1) == FOGNET_OK);
  CHECK(fognet_write_sca_groups(path.c_str(), "run", "Net", 3, three, NULL, 1) == FOGNET_OK);
  CHECK(fognet_write_sca_groups(path.c_str(), "run", "Net", 0, NULL, NULL, 1) == FOGNET_OK);
  const char* holes[3] = {"Net.a", NULL, "Net.c"};
  CHECK(fognet_write_sca_groups(path.c_str(), "run", "Net", 3, three, holes, 1) == FOGNET_ERR_ARG);
  CHECK(fognet_write_sca_groups(path.c_str(), "run", "Net", 2, NULL, NULL, 1) == FOGNET_ERR_ARG);
  CHECK(fognet_write_sca_groups(NULL, "run", "Net", 1, &whole, NULL, 0) == FOGNET_ERR_ARG);
  CHECK(fognet_write_sca_groups((dir + "/no/such/dir/x.sca").c_str(), "run", "Net", 1, &whole, NULL, 0) == FOGNET_ERR_ARG);
  FILE* f = fopen(path.c_str(), "r");
  CHECK(f != NULL);
  if (f) {
    int stats = 0, lost = 0;
    char line[512];
    while (fgets(line, sizeof line, f)) {
      if (strncmp(line, "statistic ", 10) == 0) ++stats;
      if (strstr(line, "maxPending replications lost")) ++lost;
    }
    fclose(f);
    CHECK(stats == 7 * FOGNET_REP_METRICS && lost == 2);
  }

  if (g_fail) {
    fprintf(stderr, "group_check: %d failures\n", g_fail);
    return 1;
  }
  printf("group_check: all checks passed\n");
  return 0;
}
