// stats_check.cpp — the host side of the seven statistics records (stats_host.cpp) under
// AddressSanitizer + UBSan (make asan, tests/test_stats_host.py).  For the job, node, user, window,
// queue, compare and group records, on seeded random records that are rich in edge values: the
// empty record is the identity of the merge, the merge is commutative and associative byte for byte
// and equals a restatement written here from fognet_hip.h's field comments (whole 128-bit adds, a
// 192-bit add by comparison), carries and wraps land where two's complement puts them, and a null
// argument is ignored.  Then one replication added to a job against the same added to a group.
// Usage: stats_check.  No GPU, no library: linked with stats_host.cpp only.
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "fognet_hip.h"

typedef unsigned __int128 u128;

static int g_fail = 0;
static const char* g_what = "";
#define CHECK(c)                                                                \
  do {                                                                          \
    if (!(c)) {                                                                 \
      fprintf(stderr, "%s:%d: %s: CHECK(%s)\n", __FILE__, __LINE__, g_what, #c); \
      ++g_fail;                                                                 \
    }                                                                           \
  } while (0)

static uint64_t g_state = 0x243F6A8885A308D3ull;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// ---------------------------------------------------------------- random records
static uint64_t r_u64() {  // a limb: the values around a carry come up often
  const uint64_t pick = rnd() % 6, bits = rnd() % 64;
  switch (pick) {
    case 0: return 0;
    case 1: return ~(uint64_t)0;
    case 2: return 1;
    case 3: return (uint64_t)1 << 63;
    default: return rnd() >> bits;
  }
}
static int64_t r_i64() { return (int64_t)r_u64(); }  // any value, negative ones included
static int64_t r_count() {                           // non-negative, INT64_MAX among them
  const uint64_t pick = rnd() % 6, bits = 1 + rnd() % 63;
  return pick == 0 ? INT64_MAX : pick == 1 ? 0 : pick == 2 ? 1 : (int64_t)(rnd() >> bits);
}
static double r_energy() { return (double)(rnd() >> 24); }  // whole numbers below 2^40: their sums are exact

static fognet_moments r_moments() {
  fognet_moments m;
  m.count = r_count(), m.min_raw = r_i64(), m.max_raw = r_i64();
  m.sum_lo = r_u64(), m.sum_hi = r_u64(), m.sq_lo = r_u64(), m.sq_hi = r_u64(), m.sq_top = r_u64();
  m.overflow = r_count();
  return m;
}

static fognet_job_stats r_job() {
  fognet_job_stats s;
  memset(&s, 0, sizeof s);
  s.n_reps = r_count(), s.n_failed = r_count(), s.n_tasks = r_count(), s.n_queued = r_count(), s.n_started = r_count();
  s.last_tick = r_i64();
  s.queue_min_raw = r_i64(), s.queue_max_raw = r_i64(), s.resp_min_ticks = r_i64(), s.resp_max_ticks = r_i64();
  for (int l = 0; l < 3; ++l) s.queue_sum[l] = r_u64(), s.queue_sq[l] = r_u64(), s.resp_sum[l] = r_u64(), s.resp_sq[l] = r_u64();
  s.events = r_count(), s.max_pending = r_count(), s.busy_s = r_count();
  s.energy_j = r_energy();
  s.n_qtime = r_count(), s.n_qtime_overflow = r_count(), s.n_ref_aborted = r_count();
  return s;
}

static fognet_node_stats r_node() {
  fognet_node_stats s;
  memset(&s, 0, sizeof s);
  s.n_tasks = r_count(), s.n_queued = r_count(), s.n_started = r_count(), s.n_lost = r_count(), s.busy_s = r_count();
  s.last_tick = r_i64();
  s.queue = r_moments(), s.resp = r_moments();
  return s;
}

static fognet_user_stats r_user() {
  fognet_user_stats s;
  s.delay = r_moments(), s.latency = r_moments(), s.latencyH1 = r_moments(), s.taskTime = r_moments();
  return s;
}

static fognet_window_stats r_window() {
  fognet_window_stats s;
  memset(&s, 0, sizeof s);
  s.n_publish = r_count(), s.n_complete = r_count();
  s.busy_lo = r_u64(), s.busy_hi = r_u64(), s.insys_lo = r_u64(), s.insys_hi = r_u64();
  s.queue = r_moments(), s.delay = r_moments(), s.latency = r_moments(), s.latencyH1 = r_moments(), s.taskTime = r_moments();
  return s;
}

static fognet_queue_stats r_queue() {
  fognet_queue_stats s;
  memset(&s, 0, sizeof s);
  s.n_enq = r_count(), s.max_len = r_count();
  s.observed_lo = r_u64(), s.observed_hi = r_u64(), s.area_lo = r_u64(), s.area_hi = r_u64();
  for (int q = 0; q < FOGNET_QUEUE_LEVELS_MAX; ++q) s.time_ge[q][0] = r_u64(), s.time_ge[q][1] = r_u64();
  return s;
}

static fognet_compare_stats r_compare() {
  fognet_compare_stats s;
  memset(&s, 0, sizeof s);
  s.status_a = (int32_t)(rnd() % 12), s.status_b = (int32_t)(rnd() % 12);
  s.n_reps = r_count(), s.n_pairs = r_count(), s.n_moved = r_count();
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) s.trans[i][j] = r_count();
  s.n_done_both = r_count(), s.n_done_only_a = r_count(), s.n_done_only_b = r_count(), s.n_done_neither = r_count();
  s.n_better = r_count(), s.n_equal = r_count(), s.n_worse = r_count();
  s.rep_better = r_count(), s.rep_equal = r_count(), s.rep_worse = r_count();
  s.d_start = r_moments(), s.d_service = r_moments(), s.d_resp = r_moments();
  return s;
}

static fognet_group_stats r_group() {
  fognet_group_stats s;
  memset(&s, 0, sizeof s);
  s.n_reps = r_count(), s.n_failed = r_count(), s.n_ref_aborted = r_count();
  s.n_tasks = r_count(), s.n_queued = r_count(), s.n_started = r_count(), s.events = r_count();
  s.queue = r_moments(), s.resp = r_moments();
  for (int k = 0; k < FOGNET_REP_METRICS; ++k) s.across[k] = r_moments();
  return s;
}

// ---------------------------------------------------------------- the merge, restated from the header
static int64_t x_add(int64_t a, int64_t b) { return (int64_t)(uint64_t)((__int128)a + (__int128)b); }  // wraps
static int64_t x_min(int64_t a, int64_t b) { return a < b ? a : b; }
static int64_t x_max(int64_t a, int64_t b) { return a > b ? a : b; }
static void x_add128(uint64_t& lo, uint64_t& hi, uint64_t blo, uint64_t bhi) {
  const u128 s = (((u128)hi << 64) | lo) + (((u128)bhi << 64) | blo);
  lo = (uint64_t)s, hi = (uint64_t)(s >> 64);
}
static void x_add192(uint64_t& lo, uint64_t& hi, uint64_t& top, uint64_t blo, uint64_t bhi, uint64_t btop) {
  const u128 a = ((u128)hi << 64) | lo, s = a + (((u128)bhi << 64) | blo);
  lo = (uint64_t)s, hi = (uint64_t)(s >> 64), top = top + btop + (s < a ? 1u : 0u);
}
static void x_add192(uint64_t a[3], const uint64_t b[3]) { x_add192(a[0], a[1], a[2], b[0], b[1], b[2]); }

static fognet_moments x_moments(fognet_moments a, const fognet_moments& b) {
  a.count = x_add(a.count, b.count), a.overflow = x_add(a.overflow, b.overflow);
  a.min_raw = x_min(a.min_raw, b.min_raw), a.max_raw = x_max(a.max_raw, b.max_raw);
  x_add128(a.sum_lo, a.sum_hi, b.sum_lo, b.sum_hi);
  x_add192(a.sq_lo, a.sq_hi, a.sq_top, b.sq_lo, b.sq_hi, b.sq_top);
  return a;
}

static fognet_job_stats x_job(fognet_job_stats a, const fognet_job_stats& b) {
  a.n_reps = x_add(a.n_reps, b.n_reps), a.n_failed = x_add(a.n_failed, b.n_failed), a.n_tasks = x_add(a.n_tasks, b.n_tasks);
  a.n_queued = x_add(a.n_queued, b.n_queued), a.n_started = x_add(a.n_started, b.n_started);
  a.events = x_add(a.events, b.events), a.busy_s = x_add(a.busy_s, b.busy_s);
  a.n_qtime = x_add(a.n_qtime, b.n_qtime), a.n_qtime_overflow = x_add(a.n_qtime_overflow, b.n_qtime_overflow);
  a.n_ref_aborted = x_add(a.n_ref_aborted, b.n_ref_aborted);
  a.last_tick = x_max(a.last_tick, b.last_tick), a.max_pending = x_max(a.max_pending, b.max_pending);
  a.queue_min_raw = x_min(a.queue_min_raw, b.queue_min_raw), a.queue_max_raw = x_max(a.queue_max_raw, b.queue_max_raw);
  a.resp_min_ticks = x_min(a.resp_min_ticks, b.resp_min_ticks), a.resp_max_ticks = x_max(a.resp_max_ticks, b.resp_max_ticks);
  a.energy_j = a.energy_j + b.energy_j;
  x_add192(a.queue_sum, b.queue_sum), x_add192(a.queue_sq, b.queue_sq);
  x_add192(a.resp_sum, b.resp_sum), x_add192(a.resp_sq, b.resp_sq);
  return a;
}

static fognet_node_stats x_node(fognet_node_stats a, const fognet_node_stats& b) {
  a.n_tasks = x_add(a.n_tasks, b.n_tasks), a.n_queued = x_add(a.n_queued, b.n_queued);
  a.n_started = x_add(a.n_started, b.n_started), a.n_lost = x_add(a.n_lost, b.n_lost), a.busy_s = x_add(a.busy_s, b.busy_s);
  a.last_tick = x_max(a.last_tick, b.last_tick);
  a.queue = x_moments(a.queue, b.queue), a.resp = x_moments(a.resp, b.resp);
  return a;
}

static fognet_user_stats x_user(fognet_user_stats a, const fognet_user_stats& b) {
  a.delay = x_moments(a.delay, b.delay), a.latency = x_moments(a.latency, b.latency);
  a.latencyH1 = x_moments(a.latencyH1, b.latencyH1), a.taskTime = x_moments(a.taskTime, b.taskTime);
  return a;
}

static fognet_window_stats x_window(fognet_window_stats a, const fognet_window_stats& b) {
  a.n_publish = x_add(a.n_publish, b.n_publish), a.n_complete = x_add(a.n_complete, b.n_complete);
  x_add128(a.busy_lo, a.busy_hi, b.busy_lo, b.busy_hi);
  x_add128(a.insys_lo, a.insys_hi, b.insys_lo, b.insys_hi);
  a.queue = x_moments(a.queue, b.queue), a.delay = x_moments(a.delay, b.delay), a.latency = x_moments(a.latency, b.latency);
  a.latencyH1 = x_moments(a.latencyH1, b.latencyH1), a.taskTime = x_moments(a.taskTime, b.taskTime);
  return a;
}

static fognet_queue_stats x_queue(fognet_queue_stats a, const fognet_queue_stats& b) {
  a.n_enq = x_add(a.n_enq, b.n_enq), a.max_len = x_max(a.max_len, b.max_len);
  x_add128(a.observed_lo, a.observed_hi, b.observed_lo, b.observed_hi);
  x_add128(a.area_lo, a.area_hi, b.area_lo, b.area_hi);
  for (int q = 0; q < FOGNET_QUEUE_LEVELS_MAX; ++q) x_add128(a.time_ge[q][0], a.time_ge[q][1], b.time_ge[q][0], b.time_ge[q][1]);
  return a;
}

static fognet_compare_stats x_compare(fognet_compare_stats a, const fognet_compare_stats& b) {  // (a's statuses stay)
  a.n_reps = x_add(a.n_reps, b.n_reps), a.n_pairs = x_add(a.n_pairs, b.n_pairs), a.n_moved = x_add(a.n_moved, b.n_moved);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) a.trans[i][j] = x_add(a.trans[i][j], b.trans[i][j]);
  a.n_done_both = x_add(a.n_done_both, b.n_done_both), a.n_done_only_a = x_add(a.n_done_only_a, b.n_done_only_a);
  a.n_done_only_b = x_add(a.n_done_only_b, b.n_done_only_b), a.n_done_neither = x_add(a.n_done_neither, b.n_done_neither);
  a.n_better = x_add(a.n_better, b.n_better), a.n_equal = x_add(a.n_equal, b.n_equal), a.n_worse = x_add(a.n_worse, b.n_worse);
  a.rep_better = x_add(a.rep_better, b.rep_better), a.rep_equal = x_add(a.rep_equal, b.rep_equal);
  a.rep_worse = x_add(a.rep_worse, b.rep_worse);
  a.d_start = x_moments(a.d_start, b.d_start), a.d_service = x_moments(a.d_service, b.d_service);
  a.d_resp = x_moments(a.d_resp, b.d_resp);
  return a;
}

static fognet_group_stats x_group(fognet_group_stats a, const fognet_group_stats& b) {
  a.n_reps = x_add(a.n_reps, b.n_reps), a.n_failed = x_add(a.n_failed, b.n_failed);
  a.n_ref_aborted = x_add(a.n_ref_aborted, b.n_ref_aborted), a.n_tasks = x_add(a.n_tasks, b.n_tasks);
  a.n_queued = x_add(a.n_queued, b.n_queued), a.n_started = x_add(a.n_started, b.n_started), a.events = x_add(a.events, b.events);
  a.queue = x_moments(a.queue, b.queue), a.resp = x_moments(a.resp, b.resp);
  for (int k = 0; k < FOGNET_REP_METRICS; ++k) a.across[k] = x_moments(a.across[k], b.across[k]);
  return a;
}

// ---------------------------------------------------------------- the checks of one record type
// own: leading bytes that a merge leaves to the accumulator (the compare record's two statuses)
template <class T, class Gen, class Ref>
static void check_record(const char* name, void (*init)(T*), void (*merge)(T*, const T*), Gen gen, Ref ref, size_t own,
                         int n) {
  g_what = name;
  const auto same = [own](const T& x, const T& y) {
    return memcmp((const char*)&x + own, (const char*)&y + own, sizeof(T) - own) == 0;
  };
  const auto merged = [merge](T a, const T& b) {
    merge(&a, &b);
    return a;
  };
  T empty, zero;
  memset(&empty, 0xA5, sizeof empty);  // (init writes every byte)
  memset(&zero, 0, sizeof zero);
  init(&empty);
  CHECK(memcmp(&empty, &zero, own) == 0);
  for (int i = 0; i < n; ++i) {
    const T a = gen(), b = gen(), c = gen();
    const T ea = merged(empty, a);
    CHECK(same(ea, a) && memcmp(&ea, &empty, own) == 0);  // identity
    const T ab = merged(a, b);
    CHECK(same(ab, merged(b, a)));                            // commutative
    CHECK(same(merged(ab, c), merged(a, merged(b, c))));      // associative
    const T want = ref(a, b);
    CHECK(memcmp(&ab, &want, sizeof ab) == 0);                // the header's rule, a's own bytes kept
  }
  init(nullptr);
  T x = gen();
  const T keep = x;
  merge(nullptr, &x);
  merge(&x, nullptr);
  CHECK(memcmp(&x, &keep, sizeof x) == 0);
}

// ---------------------------------------------------------------- carries and wraps, by hand
static void check_carries() {
  g_what = "carries";
  const uint64_t ones = ~(uint64_t)0;
  {  // moments inside a node record
    fognet_node_stats a, b;
    fognet_node_stats_init(&a), fognet_node_stats_init(&b);
    a.n_tasks = INT64_MAX, b.n_tasks = 1;
    a.queue.count = INT64_MAX, b.queue.count = 1;
    a.queue.sum_lo = ones, a.queue.sum_hi = 5, b.queue.sum_lo = 1;                      // lo = 2^64 - 1 plus 1
    a.queue.sq_lo = ones, a.queue.sq_hi = ones, a.queue.sq_top = 7, b.queue.sq_lo = 1;  // hi = 2^64 - 1 with a carry in
    a.resp.sum_lo = ones, a.resp.sum_hi = ones, b.resp.sum_lo = ones, b.resp.sum_hi = ones;  // -1 + -1
    a.resp.overflow = INT64_MAX, b.resp.overflow = INT64_MAX;
    fognet_node_stats_merge(&a, &b);
    CHECK(a.n_tasks == INT64_MIN && a.queue.count == INT64_MIN && a.resp.overflow == -2);
    CHECK(a.queue.sum_lo == 0 && a.queue.sum_hi == 6);
    CHECK(a.queue.sq_lo == 0 && a.queue.sq_hi == 0 && a.queue.sq_top == 8);
    CHECK(a.resp.sum_lo == ones - 1 && a.resp.sum_hi == ones);  // -2
  }
  {  // the window record's 128-bit sums wrap modulo 2^128
    fognet_window_stats a, b;
    fognet_window_stats_init(&a), fognet_window_stats_init(&b);
    a.busy_lo = ones, a.busy_hi = ones, b.busy_lo = 1;
    a.insys_lo = (uint64_t)1 << 63, a.insys_hi = 2, b.insys_lo = (uint64_t)1 << 63, b.insys_hi = ones;  // + a negative sum
    a.n_publish = INT64_MAX, b.n_publish = 1;
    fognet_window_stats_merge(&a, &b);
    CHECK(a.busy_lo == 0 && a.busy_hi == 0 && a.insys_lo == 0 && a.insys_hi == 2 && a.n_publish == INT64_MIN);
  }
  {  // the queue record's
    fognet_queue_stats a, b;
    fognet_queue_stats_init(&a), fognet_queue_stats_init(&b);
    a.time_ge[7][0] = ones, a.time_ge[7][1] = 3, b.time_ge[7][0] = 2;
    a.area_lo = ones, a.area_hi = ones, b.area_lo = ones, b.area_hi = ones;
    a.n_enq = INT64_MAX, b.n_enq = 1, a.max_len = 4, b.max_len = 9;
    fognet_queue_stats_merge(&a, &b);
    CHECK(a.time_ge[7][0] == 1 && a.time_ge[7][1] == 4 && a.area_lo == ones - 1 && a.area_hi == ones);
    CHECK(a.n_enq == INT64_MIN && a.max_len == 9 && a.time_ge[6][0] == 0 && a.time_ge[6][1] == 0);
  }
  {  // the job record's three limbs
    fognet_job_stats a, b;
    fognet_job_stats_init(&a), fognet_job_stats_init(&b);
    for (int l = 0; l < 3; ++l) a.queue_sum[l] = b.queue_sum[l] = ones;  // -1 + -1
    a.resp_sq[0] = ones, a.resp_sq[1] = ones, a.resp_sq[2] = 1, b.resp_sq[0] = 1;
    a.resp_sum[0] = ones, a.resp_sum[1] = 0, b.resp_sum[0] = 1;
    a.queue_sq[2] = ones, b.queue_sq[2] = 2;                             // the top limb wraps
    a.n_reps = INT64_MAX, b.n_reps = 1, a.busy_s = INT64_MAX, b.busy_s = INT64_MAX;
    fognet_job_stats_merge(&a, &b);
    CHECK(a.queue_sum[0] == ones - 1 && a.queue_sum[1] == ones && a.queue_sum[2] == ones);
    CHECK(a.resp_sq[0] == 0 && a.resp_sq[1] == 0 && a.resp_sq[2] == 2);
    CHECK(a.resp_sum[0] == 0 && a.resp_sum[1] == 1 && a.resp_sum[2] == 0 && a.queue_sq[2] == 1);
    CHECK(a.n_reps == INT64_MIN && a.busy_s == -2);
  }
  {  // the counts that merge as a run of words
    fognet_compare_stats a, b;
    fognet_compare_stats_init(&a), fognet_compare_stats_init(&b);
    a.status_a = 3, a.status_b = 4, b.status_a = 5, b.status_b = 6;
    a.n_reps = INT64_MAX, b.n_reps = 1, a.trans[2][2] = INT64_MAX, b.trans[2][2] = 1, a.rep_worse = INT64_MAX, b.rep_worse = 2;
    fognet_compare_stats_merge(&a, &b);
    CHECK(a.status_a == 3 && a.status_b == 4);
    CHECK(a.n_reps == INT64_MIN && a.trans[2][2] == INT64_MIN && a.rep_worse == INT64_MIN + 1 && a.d_start.count == 0);
    fognet_group_stats g, h;
    fognet_group_stats_init(&g), fognet_group_stats_init(&h);
    g.n_reps = INT64_MAX, h.n_reps = 1, g.events = INT64_MAX, h.events = INT64_MAX;
    fognet_group_stats_merge(&g, &h);
    CHECK(g.n_reps == INT64_MIN && g.events == -2 && g.queue.count == 0 && g.queue.min_raw == INT64_MAX);
  }
}

// ---------------------------------------------------------------- one replication added
static fognet_rep_stats r_rep() {
  fognet_rep_stats s;
  memset(&s, 0, sizeof s);
  s.status = rnd() % 6 == 0 ? (int32_t)(1 + rnd() % 10) : FOGNET_OK;
  s.abort_tick = rnd() % 6 == 0 ? (int64_t)(rnd() >> 4) : INT64_MAX;
  s.abort_task = -1;
  s.n_tasks = (int64_t)(rnd() % 5000);
  s.n_queued = (int64_t)(rnd() % (uint64_t)(s.n_tasks + 1));
  s.n_started = s.n_tasks - s.n_queued;
  s.events = s.n_tasks * 14;
  s.n_qtime = s.n_queued;
  s.n_qtime_overflow = (int64_t)(rnd() % 2);
  s.last_tick = rnd() % 8 == 0 ? INT64_MIN : (int64_t)(rnd() >> 8);
  s.queue_min_raw = r_i64(), s.queue_max_raw = r_i64(), s.resp_min_ticks = r_i64(), s.resp_max_ticks = r_i64();
  s.queue_sum_lo = rnd(), s.queue_sum_hi = rnd() % 3 == 0 ? ~(uint64_t)0 : rnd() >> 40;  // negative sums among them
  s.queue_sq_lo = r_u64(), s.queue_sq_hi = r_u64(), s.queue_sq_top = r_u64();
  s.resp_sum_lo = r_u64(), s.resp_sum_hi = rnd() >> 58, s.resp_sq_lo = r_u64(), s.resp_sq_hi = r_u64();
  s.max_pending = (int32_t)(rnd() % 4096);
  s.busy_s = (int64_t)(rnd() >> 20);
  s.energy_j = r_energy();
  return s;
}

static void check_add_rep() {
  g_what = "add_rep";
  fognet_job_stats job;
  fognet_group_stats group;
  fognet_job_stats_init(&job);
  fognet_group_stats_init(&group);
  double energy = 0.0;
  for (int i = 0; i < 2000; ++i) {
    const fognet_rep_stats s = r_rep();
    // the record by itself, from fognet_rep_stats' and fognet_job_stats' field comments
    fognet_job_stats one;
    fognet_job_stats_init(&one);
    fognet_job_stats_add_rep(&one, &s);
    const bool aborted = (s.status == FOGNET_OK || s.status == FOGNET_REF_ABORTED) && s.abort_tick != INT64_MAX;
    CHECK(one.n_reps == 1 && one.n_failed == (s.status != FOGNET_OK) && one.n_ref_aborted == aborted);
    if (s.status != FOGNET_OK) {
      fognet_job_stats want;
      fognet_job_stats_init(&want);
      want.n_reps = 1, want.n_failed = 1, want.n_ref_aborted = aborted;
      CHECK(memcmp(&one, &want, sizeof one) == 0);
    } else {
      CHECK(one.n_tasks == s.n_tasks && one.n_queued == s.n_queued && one.n_started == s.n_started && one.events == s.events);
      CHECK(one.last_tick == s.last_tick && one.max_pending == s.max_pending && one.busy_s == s.busy_s);
      CHECK(one.energy_j == s.energy_j && one.n_qtime == s.n_qtime && one.n_qtime_overflow == s.n_qtime_overflow);
      CHECK(one.queue_min_raw == s.queue_min_raw && one.queue_max_raw == s.queue_max_raw);
      CHECK(one.resp_min_ticks == s.resp_min_ticks && one.resp_max_ticks == s.resp_max_ticks);
      CHECK(one.queue_sum[0] == s.queue_sum_lo && one.queue_sum[1] == s.queue_sum_hi);
      CHECK(one.queue_sum[2] == ((s.queue_sum_hi >> 63) ? ~(uint64_t)0 : 0u));  // sign-extended
      CHECK(one.queue_sq[0] == s.queue_sq_lo && one.queue_sq[1] == s.queue_sq_hi && one.queue_sq[2] == s.queue_sq_top);
      CHECK(one.resp_sum[0] == s.resp_sum_lo && one.resp_sum[1] == s.resp_sum_hi && one.resp_sum[2] == 0);
      CHECK(one.resp_sq[0] == s.resp_sq_lo && one.resp_sq[1] == s.resp_sq_hi && one.resp_sq[2] == 0);
      energy = energy + s.energy_j;
    }
    // adding to an accumulator is merging the record by itself
    fognet_job_stats via = job;
    fognet_job_stats_merge(&via, &one);
    fognet_job_stats_add_rep(&job, &s);
    CHECK(memcmp(&via, &job, sizeof job) == 0);
    fognet_group_stats_add_rep(&group, &s);
  }
  CHECK(job.energy_j == energy);
  // the group as a job record: the same integers (sums inside 128 bits here); its energy comes from
  // rounded microjoules and is not compared
  fognet_job_stats gj;
  fognet_group_stats_job(&group, &gj);
  gj.energy_j = job.energy_j;
  CHECK(memcmp(&gj, &job, sizeof job) == 0);
  // null arguments are ignored
  const fognet_job_stats keep = job;
  const fognet_rep_stats s = r_rep();
  fognet_job_stats_add_rep(nullptr, &s);
  fognet_job_stats_add_rep(&job, nullptr);
  CHECK(memcmp(&job, &keep, sizeof job) == 0);
}

int main() {
  const int n = 4000;
  check_record<fognet_job_stats>("job", fognet_job_stats_init, fognet_job_stats_merge, r_job, x_job, 0, n);
  check_record<fognet_node_stats>("node", fognet_node_stats_init, fognet_node_stats_merge, r_node, x_node, 0, n);
  check_record<fognet_user_stats>("user", fognet_user_stats_init, fognet_user_stats_merge, r_user, x_user, 0, n);
  check_record<fognet_window_stats>("window", fognet_window_stats_init, fognet_window_stats_merge, r_window, x_window, 0, n);
  check_record<fognet_queue_stats>("queue", fognet_queue_stats_init, fognet_queue_stats_merge, r_queue, x_queue, 0, n);
  check_record<fognet_compare_stats>("compare", fognet_compare_stats_init, fognet_compare_stats_merge, r_compare, x_compare,
                                     offsetof(fognet_compare_stats, n_reps), n);
  check_record<fognet_group_stats>("group", fognet_group_stats_init, fognet_group_stats_merge, r_group, x_group, 0, n);
  check_carries();
  check_add_rep();
  if (g_fail) {
    fprintf(stderr, "stats_check: %d failures\n", g_fail);
    return 1;
  }
  printf("stats_check: all checks passed\n");
  return 0;
}
