// stats_host.cpp — the host side of every statistics record of fognet_hip.h: the empty record and
// the exact merge of the job, node, user, window, queue, compare and group records, one replication
// added to a job or a group, the metrics of one record and the group as a job record.
// Plain host C++ (no HIP runtime), so a sanitizer build of a stand-alone program links it as it is
// (tests/c/stats_check.cpp, tests/c/group_check.cpp).
// Every integer addition goes through uint64_t: defined for every input, and the two's-complement
// wrap that the device reductions produce.
#include <stddef.h>
#include <string.h>

#include "group_metrics.h"

namespace {

void add64(int64_t& a, int64_t b) { a = (int64_t)((uint64_t)a + (uint64_t)b); }
void take_min(int64_t& a, int64_t b) { a = b < a ? b : a; }
void take_max(int64_t& a, int64_t b) { a = b > a ? b : a; }

// a[0 .. n) += b[0 .. n), a run of contiguous counts
void add_counts(int64_t* a, const int64_t* b, int n) {
  for (int w = 0; w < n; ++w) add64(a[w], b[w]);
}

// (hi, lo) += (bhi, blo) modulo 2^128; the carry out of hi
uint64_t add128(uint64_t& lo, uint64_t& hi, uint64_t blo, uint64_t bhi) {
  unsigned __int128 s = (unsigned __int128)lo + blo;
  lo = (uint64_t)s;
  s = (unsigned __int128)hi + bhi + (uint64_t)(s >> 64);
  hi = (uint64_t)s;
  return (uint64_t)(s >> 64);
}

// a += b modulo 2^192, limbs [0] = least significant
void add192(uint64_t a[3], const uint64_t b[3]) { a[2] = a[2] + b[2] + add128(a[0], a[1], b[0], b[1]); }

void moments_init(fognet_moments* m) {
  memset(m, 0, sizeof *m);
  m->min_raw = INT64_MAX;
  m->max_raw = INT64_MIN;
}

// a += b: counts add, extrema combine, the sums modulo 2^128 / 2^192
void moments_merge(fognet_moments* a, const fognet_moments* b) {
  add64(a->count, b->count);
  add64(a->overflow, b->overflow);
  take_min(a->min_raw, b->min_raw);
  take_max(a->max_raw, b->max_raw);
  add128(a->sum_lo, a->sum_hi, b->sum_lo, b->sum_hi);
  a->sq_top = a->sq_top + b->sq_top + add128(a->sq_lo, a->sq_hi, b->sq_lo, b->sq_hi);
}

// the queueTime and response moments of one replication's record (resp: 128 bits of squares, nothing lost)
void rep_moments(const fognet_rep_stats& s, fognet_moments& queue, fognet_moments& resp) {
  queue = fognet_moments{s.n_qtime,     s.queue_min_raw, s.queue_max_raw, s.queue_sum_lo,     s.queue_sum_hi,
                         s.queue_sq_lo, s.queue_sq_hi,   s.queue_sq_top,  s.n_qtime_overflow};
  resp = fognet_moments{s.n_tasks, s.resp_min_ticks, s.resp_max_ticks, s.resp_sum_lo, s.resp_sum_hi,
                        s.resp_sq_lo, s.resp_sq_hi, 0u, 0};
}

// a job record's queue_* / resp_* fields and n_qtime* from pooled moments: queue_sum's top limb is the
// two's complement sign extension of the 128-bit sum, resp_sum's is 0
void job_set_moments(fognet_job_stats* j, const fognet_moments& queue, const fognet_moments& resp) {
  j->queue_min_raw = queue.min_raw;
  j->queue_max_raw = queue.max_raw;
  j->n_qtime = queue.count;
  j->n_qtime_overflow = queue.overflow;
  j->resp_min_ticks = resp.min_raw;
  j->resp_max_ticks = resp.max_raw;
  j->queue_sum[0] = queue.sum_lo;
  j->queue_sum[1] = queue.sum_hi;
  j->queue_sum[2] = (int64_t)queue.sum_hi < 0 ? ~(uint64_t)0 : 0u;
  j->queue_sq[0] = queue.sq_lo;
  j->queue_sq[1] = queue.sq_hi;
  j->queue_sq[2] = queue.sq_top;
  j->resp_sum[0] = resp.sum_lo;
  j->resp_sum[1] = resp.sum_hi;
  j->resp_sum[2] = 0u;
  j->resp_sq[0] = resp.sq_lo;
  j->resp_sq[1] = resp.sq_hi;
  j->resp_sq[2] = resp.sq_top;
}

// counted under FOGNET_FLAG_REF_ABORT too (status FOGNET_REF_ABORTED), like the device reductions
bool ref_aborted(const fognet_rep_stats& s) {
  return (s.status == FOGNET_OK || s.status == FOGNET_REF_ABORTED) && s.abort_tick != INT64_MAX;
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------- job record
void fognet_job_stats_init(fognet_job_stats* s) {
  if (!s) return;
  memset(s, 0, sizeof *s);
  s->queue_min_raw = s->resp_min_ticks = INT64_MAX;
  s->queue_max_raw = s->resp_max_ticks = s->last_tick = INT64_MIN;
}

void fognet_job_stats_merge(fognet_job_stats* a, const fognet_job_stats* b) {
  if (!a || !b) return;
  add64(a->n_reps, b->n_reps);
  add64(a->n_failed, b->n_failed);
  add64(a->n_tasks, b->n_tasks);
  add64(a->n_queued, b->n_queued);
  add64(a->n_started, b->n_started);
  add64(a->events, b->events);
  take_max(a->last_tick, b->last_tick);
  take_min(a->queue_min_raw, b->queue_min_raw);
  take_max(a->queue_max_raw, b->queue_max_raw);
  add64(a->n_qtime, b->n_qtime);
  add64(a->n_qtime_overflow, b->n_qtime_overflow);
  add64(a->n_ref_aborted, b->n_ref_aborted);
  take_min(a->resp_min_ticks, b->resp_min_ticks);
  take_max(a->resp_max_ticks, b->resp_max_ticks);
  take_max(a->max_pending, b->max_pending);
  add64(a->busy_s, b->busy_s);
  a->energy_j = a->energy_j + b->energy_j;
  add192(a->queue_sum, b->queue_sum);
  add192(a->queue_sq, b->queue_sq);
  add192(a->resp_sum, b->resp_sum);
  add192(a->resp_sq, b->resp_sq);
}

void fognet_job_stats_add_rep(fognet_job_stats* a, const fognet_rep_stats* s) {
  if (!a || !s) return;
  add64(a->n_reps, 1);
  if (ref_aborted(*s)) add64(a->n_ref_aborted, 1);
  if (s->status != FOGNET_OK) {
    add64(a->n_failed, 1);
    return;
  }
  fognet_job_stats b;
  fognet_job_stats_init(&b);
  b.n_tasks = s->n_tasks;
  b.n_queued = s->n_queued;
  b.n_started = s->n_started;
  b.events = s->events;
  b.last_tick = s->last_tick;
  b.max_pending = s->max_pending;
  b.busy_s = s->busy_s;
  b.energy_j = s->energy_j;
  fognet_moments queue, resp;
  rep_moments(*s, queue, resp);
  job_set_moments(&b, queue, resp);
  fognet_job_stats_merge(a, &b);
}

// ---------------------------------------------------------------- node, user, window, queue, compare records
void fognet_node_stats_init(fognet_node_stats* s) {
  if (!s) return;
  memset(s, 0, sizeof *s);
  s->last_tick = INT64_MIN;
  moments_init(&s->queue);
  moments_init(&s->resp);
}

void fognet_node_stats_merge(fognet_node_stats* a, const fognet_node_stats* b) {
  if (!a || !b) return;
  add64(a->n_tasks, b->n_tasks);
  add64(a->n_queued, b->n_queued);
  add64(a->n_started, b->n_started);
  add64(a->n_lost, b->n_lost);
  add64(a->busy_s, b->busy_s);
  take_max(a->last_tick, b->last_tick);
  moments_merge(&a->queue, &b->queue);
  moments_merge(&a->resp, &b->resp);
}

void fognet_user_stats_init(fognet_user_stats* s) {
  if (!s) return;
  moments_init(&s->delay);
  moments_init(&s->latency);
  moments_init(&s->latencyH1);
  moments_init(&s->taskTime);
}

void fognet_user_stats_merge(fognet_user_stats* a, const fognet_user_stats* b) {
  if (!a || !b) return;
  moments_merge(&a->delay, &b->delay);
  moments_merge(&a->latency, &b->latency);
  moments_merge(&a->latencyH1, &b->latencyH1);
  moments_merge(&a->taskTime, &b->taskTime);
}

void fognet_window_stats_init(fognet_window_stats* s) {
  if (!s) return;
  memset(s, 0, sizeof *s);
  moments_init(&s->queue);
  moments_init(&s->delay);
  moments_init(&s->latency);
  moments_init(&s->latencyH1);
  moments_init(&s->taskTime);
}

void fognet_window_stats_merge(fognet_window_stats* a, const fognet_window_stats* b) {
  if (!a || !b) return;
  add64(a->n_publish, b->n_publish);
  add64(a->n_complete, b->n_complete);
  add128(a->busy_lo, a->busy_hi, b->busy_lo, b->busy_hi);
  add128(a->insys_lo, a->insys_hi, b->insys_lo, b->insys_hi);
  moments_merge(&a->queue, &b->queue);
  moments_merge(&a->delay, &b->delay);
  moments_merge(&a->latency, &b->latency);
  moments_merge(&a->latencyH1, &b->latencyH1);
  moments_merge(&a->taskTime, &b->taskTime);
}

void fognet_queue_stats_init(fognet_queue_stats* s) {
  if (s) memset(s, 0, sizeof *s);
}

void fognet_queue_stats_merge(fognet_queue_stats* a, const fognet_queue_stats* b) {
  if (!a || !b) return;
  add64(a->n_enq, b->n_enq);
  take_max(a->max_len, b->max_len);
  add128(a->observed_lo, a->observed_hi, b->observed_lo, b->observed_hi);
  add128(a->area_lo, a->area_hi, b->area_lo, b->area_hi);
  for (int q = 0; q < FOGNET_QUEUE_LEVELS_MAX; ++q)
    add128(a->time_ge[q][0], a->time_ge[q][1], b->time_ge[q][0], b->time_ge[q][1]);
}

void fognet_compare_stats_init(fognet_compare_stats* s) {
  if (!s) return;
  memset(s, 0, sizeof *s);  // (statuses FOGNET_OK)
  moments_init(&s->d_start);
  moments_init(&s->d_service);
  moments_init(&s->d_resp);
}

void fognet_compare_stats_merge(fognet_compare_stats* a, const fognet_compare_stats* b) {
  if (!a || !b) return;
  // the 22 counts from n_reps to rep_worse (a's statuses stay)
  static_assert(offsetof(fognet_compare_stats, d_start) - offsetof(fognet_compare_stats, n_reps) == 22 * sizeof(int64_t),
                "the counts are contiguous");
  add_counts(&a->n_reps, &b->n_reps, 22);
  moments_merge(&a->d_start, &b->d_start);
  moments_merge(&a->d_service, &b->d_service);
  moments_merge(&a->d_resp, &b->d_resp);
}

// ---------------------------------------------------------------- replication groups
void fognet_rep_metrics(const fognet_rep_stats* rep, int64_t value[FOGNET_REP_METRICS], uint32_t* defined,
                        uint32_t* overflowed) {
  if (!rep || !value) return;
  const fognet::RepMetrics m = fognet::rep_metrics(*rep);
  for (int k = 0; k < FOGNET_REP_METRICS; ++k) value[k] = m.v[k];
  if (defined) *defined = m.defined;
  if (overflowed) *overflowed = m.overflowed;
}

void fognet_group_stats_init(fognet_group_stats* s) {
  if (!s) return;
  memset(s, 0, sizeof *s);
  moments_init(&s->queue);
  moments_init(&s->resp);
  for (int k = 0; k < FOGNET_REP_METRICS; ++k) moments_init(&s->across[k]);
}

void fognet_group_stats_merge(fognet_group_stats* a, const fognet_group_stats* b) {
  if (!a || !b) return;
  static_assert(offsetof(fognet_group_stats, queue) == 7 * sizeof(int64_t), "the counts are contiguous");
  add_counts(&a->n_reps, &b->n_reps, 7);
  moments_merge(&a->queue, &b->queue);
  moments_merge(&a->resp, &b->resp);
  for (int k = 0; k < FOGNET_REP_METRICS; ++k) moments_merge(&a->across[k], &b->across[k]);
}

void fognet_group_stats_add_rep(fognet_group_stats* a, const fognet_rep_stats* s) {
  if (!a || !s) return;
  fognet_group_stats b;
  fognet_group_stats_init(&b);
  b.n_reps = 1;
  if (ref_aborted(*s)) b.n_ref_aborted = 1;
  if (s->status != FOGNET_OK) {
    b.n_failed = 1;
  } else {
    b.n_tasks = s->n_tasks;
    b.n_queued = s->n_queued;
    b.n_started = s->n_started;
    b.events = s->events;
    rep_moments(*s, b.queue, b.resp);
    const fognet::RepMetrics m = fognet::rep_metrics(*s);
    for (int k = 0; k < FOGNET_REP_METRICS; ++k) {
      fognet_moments& x = b.across[k];
      x.overflow = (m.overflowed >> k) & 1u;
      if (!((m.defined >> k) & 1u)) continue;
      const int64_t v = m.v[k];
      const unsigned __int128 mag = v < 0 ? (unsigned __int128)0 - (unsigned __int128)(__int128)v : (unsigned __int128)v;
      const unsigned __int128 sq = mag * mag;
      x.count = 1;
      x.min_raw = x.max_raw = v;
      x.sum_lo = (uint64_t)v;
      x.sum_hi = v < 0 ? ~(uint64_t)0 : 0u;
      x.sq_lo = (uint64_t)sq;
      x.sq_hi = (uint64_t)(sq >> 64);
    }
  }
  fognet_group_stats_merge(a, &b);
}

void fognet_group_stats_job(const fognet_group_stats* g, fognet_job_stats* out) {
  if (!g || !out) return;
  memset(out, 0, sizeof *out);
  out->n_reps = g->n_reps;
  out->n_failed = g->n_failed;
  out->n_ref_aborted = g->n_ref_aborted;
  out->n_tasks = g->n_tasks;
  out->n_queued = g->n_queued;
  out->n_started = g->n_started;
  out->events = g->events;
  out->last_tick = g->across[FOGNET_METRIC_MAKESPAN].max_raw;
  const int64_t pend = g->across[FOGNET_METRIC_MAX_PENDING].max_raw;
  out->max_pending = pend > 0 ? pend : 0;  // (the job's maximum starts at 0)
  out->busy_s = (int64_t)g->across[FOGNET_METRIC_BUSY_S].sum_lo;
  job_set_moments(out, g->queue, g->resp);
  const fognet_moments& e = g->across[FOGNET_METRIC_ENERGY_UJ];
  const __int128 uj = (__int128)(((unsigned __int128)e.sum_hi << 64) | e.sum_lo);
  out->energy_j = (double)uj * 1e-6;
}

}  // extern "C"
