// stats_atomics.h — what the keyed statistics passes share (node_stats.hip keyed by
// node, per_user_stats.hip keyed by user): integer atomic updates of fognet_moments
// records in LDS or HBM, and the exact merge of two such records.  Every update is a
// 64-bit integer atomic: sums take their carries from the value the atomic add returns,
// extrema are integer min/max, so a record does not depend on the order of its updates.
#pragma once
#include "replay_common.h"

namespace fognet {

// *p += v; returns the carry out of the word (from the value the add replaced).
__device__ __forceinline__ uint64_t atomic_add_carry(uint64_t* p, uint64_t v) {
  if (v == 0u) return 0u;
  const uint64_t old = (uint64_t)atomicAdd((unsigned long long*)p, (unsigned long long)v);
  return old + v < old ? 1u : 0u;
}
__device__ __forceinline__ void atomic_add(void* p, uint64_t v) {
  if (v != 0u) (void)atomicAdd((unsigned long long*)p, (unsigned long long)v);
}
// Multi-limb sums: each word's wrap-arounds are carried into the next word by the
// update that caused them, so the final value is the sum modulo 2^128 / 2^192 in any order.
__device__ __forceinline__ void atomic_add128(uint64_t* lo, uint64_t* hi, uint64_t vlo, uint64_t vhi) {
  atomic_add(hi, vhi + atomic_add_carry(lo, vlo));
}
__device__ __forceinline__ void atomic_add192(uint64_t* lo, uint64_t* hi, uint64_t* top, uint64_t vlo, uint64_t vhi,
                                              uint64_t vtop) {
  const uint64_t mid = vhi + atomic_add_carry(lo, vlo);
  const uint64_t c_mid = mid < vhi ? 1u : 0u;  // vhi + carry itself wrapped (to 0)
  atomic_add(top, vtop + c_mid + atomic_add_carry(hi, mid));
}
__device__ __forceinline__ void atomic_min_i64(int64_t* p, int64_t v) { (void)atomicMin((long long*)p, (long long)v); }
__device__ __forceinline__ void atomic_max_i64(int64_t* p, int64_t v) { (void)atomicMax((long long*)p, (long long)v); }

__device__ __forceinline__ void commit_moments(fognet_moments* m, uint64_t n, uint64_t ovf, int64_t mn, int64_t mx,
                                               uint64_t s_lo, uint64_t s_hi, uint64_t q_lo, uint64_t q_hi,
                                               uint64_t q_top) {
  atomic_add(&m->overflow, ovf);
  if (n == 0u) return;
  atomic_add(&m->count, n);
  atomic_min_i64(&m->min_raw, mn);
  atomic_max_i64(&m->max_raw, mx);
  atomic_add128(&m->sum_lo, &m->sum_hi, s_lo, s_hi);
  atomic_add192(&m->sq_lo, &m->sq_hi, &m->sq_top, q_lo, q_hi, q_top);
}

// the exact merge of two records (the job reductions)
__device__ __forceinline__ void moments_merge(fognet_moments& a, const fognet_moments& b) {
  a.count += b.count;
  a.overflow += b.overflow;
  a.min_raw = min(a.min_raw, b.min_raw);
  a.max_raw = max(a.max_raw, b.max_raw);
  add128(a.sum_lo, a.sum_hi, b.sum_lo, b.sum_hi);
  add192(a.sq_lo, a.sq_hi, a.sq_top, b.sq_lo, b.sq_hi, b.sq_top);
}

}  // namespace fognet
