// group_metrics.h — the per-replication metrics of fognet_hip.h "Replication groups", stated once
// for the device pass (group_stats.hip) and the host twins (stats_host.cpp): nine exact integers formed
// from one fognet_rep_stats, each defined or not, each fitting int64 or counted as lost.
#pragma once
#include <math.h>
#include <stdint.h>

#include "fognet_hip.h"

// (stats_host.cpp is plain host C++: no HIP runtime there)
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FOGNET_HD __host__ __device__
#else
#define FOGNET_HD
#endif

namespace fognet {

struct RepMetrics {
  int64_t v[FOGNET_REP_METRICS];  // INT64_MIN where the bit of `defined` is clear
  uint32_t defined;               // bit m: v[m] is a value the moments take
  uint32_t overflowed;            // bit m: the metric is defined and does not fit int64
};

// floor(n / d) of an unsigned 128-bit n and d > 0; false where it does not fit int64
FOGNET_HD inline bool floor_div_u128(unsigned __int128 n, uint64_t d, int64_t& q) {
  uint64_t q64;
  if ((uint64_t)(n >> 64) == 0u) {  // the common case: one 64-bit division
    q64 = (uint64_t)n / d;
  } else {
    const unsigned __int128 qq = n / d;
    if ((qq >> 63) != 0u) return false;
    q64 = (uint64_t)qq;
  }
  if ((q64 >> 63) != 0u) return false;
  q = (int64_t)q64;
  return true;
}

// floor(n / d) towards minus infinity of a signed 128-bit n and d > 0 (-7 / 2 -> -4)
FOGNET_HD inline bool floor_div_i128(__int128 n, uint64_t d, int64_t& q) {
  if (n >= 0) return floor_div_u128((unsigned __int128)n, d, q);
  const unsigned __int128 mag = (unsigned __int128)0 - (unsigned __int128)n;  // (2^127 for the minimum)
  unsigned __int128 qm;
  if ((uint64_t)(mag >> 64) == 0u) qm = (uint64_t)mag / d;
  else qm = mag / d;
  const unsigned __int128 rem = mag - qm * d;
  const unsigned __int128 up = qm + (rem != 0u ? 1u : 0u);  // -ceil(mag / d)
  if (up > ((unsigned __int128)1 << 63)) return false;
  q = (int64_t)((uint64_t)0 - (uint64_t)up);
  return true;
}

// toInt64(energy_j * 1e6): one multiply, then floor(x + 0.5), each rounded on its own
FOGNET_HD inline bool energy_to_uj(double e, int64_t& uj) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double x = e * 1e6;
  const double f = floor(x + 0.5);
  const bool ok = fabs(f) < 0x1p63;  // (false for a NaN)
  uj = ok ? (int64_t)f : 0;
  return ok;
}

// (the status is the caller's business: only an OK replication's metrics reach the moments)
FOGNET_HD inline RepMetrics rep_metrics(const fognet_rep_stats& s) {
  RepMetrics m;
  m.defined = m.overflowed = 0u;
  for (int k = 0; k < FOGNET_REP_METRICS; ++k) m.v[k] = INT64_MIN;
  auto take = [&](int k, bool fits, int64_t v) {
    if (fits) {
      m.v[k] = v;
      m.defined |= 1u << k;
    } else {
      m.overflowed |= 1u << k;
    }
  };
  int64_t q = 0;
  if (s.n_tasks > 0) {
    const unsigned __int128 rs = ((unsigned __int128)s.resp_sum_hi << 64) | s.resp_sum_lo;
    const bool fits = floor_div_u128(rs, (uint64_t)s.n_tasks, q);
    take(FOGNET_METRIC_RESP_MEAN, fits, q);
    take(FOGNET_METRIC_RESP_MAX, true, s.resp_max_ticks);
    const bool pfits = floor_div_i128((__int128)s.n_queued * 1000000, (uint64_t)s.n_tasks, q);
    take(FOGNET_METRIC_QUEUED_PPM, pfits, q);
  }
  if (s.n_qtime > 0) {
    const __int128 qs = (__int128)(((unsigned __int128)s.queue_sum_hi << 64) | s.queue_sum_lo);
    const bool fits = floor_div_i128(qs, (uint64_t)s.n_qtime, q);
    take(FOGNET_METRIC_QUEUE_MEAN, fits, q);
    take(FOGNET_METRIC_QUEUE_MAX, true, s.queue_max_raw);
  }
  if (s.last_tick != INT64_MIN) take(FOGNET_METRIC_MAKESPAN, true, s.last_tick);
  take(FOGNET_METRIC_BUSY_S, true, s.busy_s);
  take(FOGNET_METRIC_MAX_PENDING, true, (int64_t)s.max_pending);
  const bool efits = energy_to_uj(s.energy_j, q);
  take(FOGNET_METRIC_ENERGY_UJ, efits, q);
  return m;
}

}  // namespace fognet
