// group_host.cpp — the host twins of the replication-group pass (fognet_hip.h "Replication groups"):
// the metrics of one record, the empty group record, one replication added, the exact merge, and
// the group as a job record.  Plain host C++ (no HIP runtime), so a sanitizer build of a stand-alone
// program links it as it is (tests/c/group_check.cpp).
#include <stddef.h>
#include <string.h>

#include "group_metrics.h"

static void moments_init_host(fognet_moments* m) {
  memset(m, 0, sizeof *m);
  m->min_raw = INT64_MAX;
  m->max_raw = INT64_MIN;
}

// a += b: counts add, extrema combine, the sums modulo 2^128 / 2^192
static void moments_merge_host(fognet_moments* a, const fognet_moments* b) {
  a->count = (int64_t)((uint64_t)a->count + (uint64_t)b->count);
  a->overflow = (int64_t)((uint64_t)a->overflow + (uint64_t)b->overflow);
  if (b->min_raw < a->min_raw) a->min_raw = b->min_raw;
  if (b->max_raw > a->max_raw) a->max_raw = b->max_raw;
  unsigned __int128 c = (unsigned __int128)a->sum_lo + b->sum_lo;
  a->sum_lo = (uint64_t)c;
  a->sum_hi = a->sum_hi + b->sum_hi + (uint64_t)(c >> 64);
  c = (unsigned __int128)a->sq_lo + b->sq_lo;
  a->sq_lo = (uint64_t)c;
  c = (unsigned __int128)a->sq_hi + b->sq_hi + (uint64_t)(c >> 64);
  a->sq_hi = (uint64_t)c;
  a->sq_top = a->sq_top + b->sq_top + (uint64_t)(c >> 64);
}

extern "C" {

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
  moments_init_host(&s->queue);
  moments_init_host(&s->resp);
  for (int k = 0; k < FOGNET_REP_METRICS; ++k) moments_init_host(&s->across[k]);
}

void fognet_group_stats_merge(fognet_group_stats* a, const fognet_group_stats* b) {
  if (!a || !b) return;
  static_assert(offsetof(fognet_group_stats, queue) == 7 * sizeof(int64_t), "the counts are contiguous");
  int64_t* const aw = &a->n_reps;
  const int64_t* const bw = &b->n_reps;
  for (int w = 0; w < 7; ++w) aw[w] = (int64_t)((uint64_t)aw[w] + (uint64_t)bw[w]);
  moments_merge_host(&a->queue, &b->queue);
  moments_merge_host(&a->resp, &b->resp);
  for (int k = 0; k < FOGNET_REP_METRICS; ++k) moments_merge_host(&a->across[k], &b->across[k]);
}

void fognet_group_stats_add_rep(fognet_group_stats* a, const fognet_rep_stats* s) {
  if (!a || !s) return;
  fognet_group_stats b;
  fognet_group_stats_init(&b);
  b.n_reps = 1;
  if ((s->status == FOGNET_OK || s->status == FOGNET_REF_ABORTED) && s->abort_tick != INT64_MAX) b.n_ref_aborted = 1;
  if (s->status != FOGNET_OK) {
    b.n_failed = 1;
  } else {
    b.n_tasks = s->n_tasks;
    b.n_queued = s->n_queued;
    b.n_started = s->n_started;
    b.events = s->events;
    // the member's own moments, as fognet_job_stats_add_rep takes them
    b.queue = fognet_moments{s->n_qtime,     s->queue_min_raw, s->queue_max_raw, s->queue_sum_lo,      s->queue_sum_hi,
                             s->queue_sq_lo, s->queue_sq_hi,   s->queue_sq_top,  s->n_qtime_overflow};
    b.resp = fognet_moments{s->n_tasks, s->resp_min_ticks, s->resp_max_ticks, s->resp_sum_lo, s->resp_sum_hi,
                            s->resp_sq_lo, s->resp_sq_hi, 0u, 0};
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
  memset(out, 0, sizeof *out);  // (every field is set below but the top limbs, which stay 0)
  out->n_reps = g->n_reps;
  out->n_failed = g->n_failed;
  out->n_ref_aborted = g->n_ref_aborted;
  out->n_tasks = g->n_tasks;
  out->n_queued = g->n_queued;
  out->n_started = g->n_started;
  out->events = g->events;
  out->last_tick = g->across[FOGNET_METRIC_MAKESPAN].max_raw;
  out->queue_min_raw = g->queue.min_raw;
  out->queue_max_raw = g->queue.max_raw;
  out->n_qtime = g->queue.count;
  out->n_qtime_overflow = g->queue.overflow;
  out->resp_min_ticks = g->resp.min_raw;
  out->resp_max_ticks = g->resp.max_raw;
  const int64_t pend = g->across[FOGNET_METRIC_MAX_PENDING].max_raw;
  out->max_pending = pend > 0 ? pend : 0;  // (the job's maximum starts at 0)
  out->busy_s = (int64_t)g->across[FOGNET_METRIC_BUSY_S].sum_lo;
  out->queue_sum[0] = g->queue.sum_lo;
  out->queue_sum[1] = g->queue.sum_hi;
  out->queue_sum[2] = (int64_t)g->queue.sum_hi < 0 ? ~(uint64_t)0 : 0u;
  out->queue_sq[0] = g->queue.sq_lo;
  out->queue_sq[1] = g->queue.sq_hi;
  out->queue_sq[2] = g->queue.sq_top;
  out->resp_sum[0] = g->resp.sum_lo;
  out->resp_sum[1] = g->resp.sum_hi;
  out->resp_sq[0] = g->resp.sq_lo;
  out->resp_sq[1] = g->resp.sq_hi;
  out->resp_sq[2] = g->resp.sq_top;
  const fognet_moments& e = g->across[FOGNET_METRIC_ENERGY_UJ];
  const __int128 uj = (__int128)(((unsigned __int128)e.sum_hi << 64) | e.sum_lo);
  out->energy_j = (double)uj * 1e-6;
}

}  // extern "C"
