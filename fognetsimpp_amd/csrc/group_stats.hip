// group_stats.hip — replication groups (fognet_reduce_groups_dev): the job reduction keyed by the
// replication's place in the job, and per group the moments of nine per-replication metrics across
// its replications.  fognet_hip.h "Replication groups" states the record, group_metrics.h the
// metrics.
//
// The pass reads the [R] records alone, 200 B per replication, one replication per lane in a
// grid-stride loop.  A replication is eleven "signals" to its group: the pooled queueTime and
// response moments it already carries, and one value of each defined metric.  They are taken one at
// a time in a rolled loop (eleven Sigs through one butterfly would be some 150 VGPR pairs).  A
// wavefront whose members all name one group -- G = 1, contiguous groups -- merges each signal in a
// butterfly and commits once; otherwise every member commits on its own.  Up to
// FOGNET_GROUP_LDS_MAX groups the accumulators are the workgroup's LDS copy, whose non-empty records
// are added to the caller's at the end; above, the caller's records themselves, which a clear
// kernel has set to the empty record.  Every update is one of signals.h's integer atomics, so a
// record does not depend on their order.
#include "group_metrics.h"
#include "signals.h"

namespace fognet {

namespace {

struct GroupOps {
  using Rec = fognet_group_stats;
  static constexpr int kHeadWords = 7;
  static __device__ __forceinline__ uint64_t head_empty(int) { return 0u; }
};
constexpr int kRecWords = rec_words<GroupOps>();
constexpr int kSignals = 2 + FOGNET_REP_METRICS;
static_assert(sizeof(fognet_group_stats) == 848 && kRecWords == 106, "fognet_group_stats is 106 words");
static_assert(offsetof(fognet_group_stats, n_reps) == 0 && offsetof(fognet_group_stats, events) == 6 * 8 &&
                  offsetof(fognet_group_stats, queue) == GroupOps::kHeadWords * 8 &&
                  offsetof(fognet_group_stats, resp) == (GroupOps::kHeadWords + kMomWords) * 8 &&
                  offsetof(fognet_group_stats, across) == (GroupOps::kHeadWords + 2 * kMomWords) * 8,
              "the record's layout (fognet_hip.h): 7 counts, then queue, resp and across[9]");
static_assert(FOGNET_GROUP_LDS_MAX * sizeof(fognet_group_stats) <= 64 * 1024, "the LDS copy fits a workgroup's 64 KiB");

struct GroupArgs {
  const fognet_rep_stats* stats;
  const int32_t* group_of;  // nullable: every replication in group 0
  int32_t R, G;
  fognet_group_stats* out;
  int64_t* metrics;      // [R][FOGNET_REP_METRICS], nullable
  uint32_t* defined;     // [R], nullable
  int64_t* n_ungrouped;  // [1], nullable
};

// One signal's share of a replication, of a wavefront or of a record: count, lost, moments.
struct Part {
  uint64_t n, ovf;
  Sig s;
};

__device__ __forceinline__ Part part_identity() { return Part{0u, 0u, sig_identity()}; }

__device__ __forceinline__ int64_t metric_at(const RepMetrics& m, int k) {
  switch (k) {
    case 0: return m.v[0];
    case 1: return m.v[1];
    case 2: return m.v[2];
    case 3: return m.v[3];
    case 4: return m.v[4];
    case 5: return m.v[5];
    case 6: return m.v[6];
    case 7: return m.v[7];
    default: return m.v[8];
  }
}

// Signal k of an OK replication: 0 its queueTime moments, 1 its response moments (both merged as
// the job reduction merges them, whatever the counts say), 2 + m the one value of metric m.
__device__ __forceinline__ Part part_of(const fognet_rep_stats& s, const RepMetrics& m, int k) {
  if (k == 0)
    return Part{(uint64_t)s.n_qtime, (uint64_t)s.n_qtime_overflow,
                Sig{s.queue_min_raw, s.queue_max_raw, s.queue_sum_lo, s.queue_sum_hi, s.queue_sq_lo, s.queue_sq_hi,
                    s.queue_sq_top}};
  if (k == 1)
    return Part{(uint64_t)s.n_tasks, 0u,
                Sig{s.resp_min_ticks, s.resp_max_ticks, s.resp_sum_lo, s.resp_sum_hi, s.resp_sq_lo, s.resp_sq_hi, 0u}};
  const int b = k - 2;
  Part p = part_identity();
  if ((m.defined >> b) & 1u) {
    p.n = 1u;
    sig_add(p.s, metric_at(m, b));
  }
  p.ovf = (m.overflowed >> b) & 1u;
  return p;
}

// butterfly over the 64 lanes (all active): every lane ends with the wavefront's part
__device__ __forceinline__ void wave_merge_part(Part& p) {
#pragma unroll 1
  for (int x = kWave / 2; x > 0; x >>= 1) {
    const uint64_t on = shfl_xor_u64(p.n, x), oo = shfl_xor_u64(p.ovf, x);
    const Sig os = sig_shfl_xor(p.s, x);
    p.n += on;
    p.ovf += oo;
    sig_merge(p.s, os);
  }
}

// (commit_sig returns at a count of 0; a pooled signal is merged whatever its count says)
__device__ __forceinline__ void commit_part(fognet_moments* m, const Part& p) {
  atomic_add(&m->count, p.n);
  atomic_add(&m->overflow, p.ovf);
  if (p.s.mn != INT64_MAX) atomic_min_i64(&m->min_raw, p.s.mn);
  if (p.s.mx != INT64_MIN) atomic_max_i64(&m->max_raw, p.s.mx);
  atomic_add128(&m->sum_lo, &m->sum_hi, p.s.s_lo, p.s.s_hi);
  atomic_add192(&m->sq_lo, &m->sq_hi, &m->sq_top, p.s.q_lo, p.s.q_hi, p.s.q_top);
}

__device__ __forceinline__ fognet_moments* signal_of(fognet_group_stats* rec, int k) {
  return &rec->queue + k;  // queue, resp, across[0 .. 8]: contiguous (the static_assert above)
}

__global__ __launch_bounds__(kPassThreads) void group_clear_kernel(uint64_t* out, size_t words, int64_t* n_ungrouped) {
  const size_t stride = (size_t)gridDim.x * kPassThreads;
  for (size_t w = (size_t)blockIdx.x * kPassThreads + threadIdx.x; w < words; w += stride)
    out[w] = empty_word<GroupOps>((int)(w % kRecWords));
  if (n_ungrouped && blockIdx.x == 0 && threadIdx.x == 0) *n_ungrouped = 0;
}

template <bool kLds>
__global__ __launch_bounds__(kPassThreads) void group_kernel(GroupArgs P) {
  extern __shared__ uint64_t s_acc[];  // kLds: the workgroup's G records
  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1);
  if (kLds) {
    for (int w = tid; w < P.G * kRecWords; w += kPassThreads) s_acc[w] = empty_word<GroupOps>(w % kRecWords);
    __syncthreads();
  }
  fognet_group_stats* const acc = kLds ? reinterpret_cast<fognet_group_stats*>(s_acc) : P.out;
  const int64_t stride = (int64_t)gridDim.x * kPassThreads;
  // (the bound is a wavefront's first replication: its 64 lanes take every round together)
  for (int64_t base = (int64_t)blockIdx.x * kPassThreads + (tid - lane); base < P.R; base += stride) {
    const int64_t r = base + lane;
    const bool in = r < P.R;
    const fognet_rep_stats s = P.stats[in ? r : base];  // (a lane past R reloads the wavefront's first record, unused)
    int32_t g = 0;
    if (in && P.group_of) g = P.group_of[r];
    const bool member = in && (uint32_t)g < (uint32_t)P.G;
    const bool ok = s.status == FOGNET_OK;
    const RepMetrics m = rep_metrics(s);
    if (in && P.metrics) {
#pragma unroll
      for (int k = 0; k < FOGNET_REP_METRICS; ++k) P.metrics[r * FOGNET_REP_METRICS + k] = ok ? m.v[k] : INT64_MIN;
    }
    if (in && P.defined) P.defined[r] = ok ? m.defined : 0u;
    const uint64_t lost = __ballot(in && !member);
    if (lane == 0 && P.n_ungrouped && lost != 0u) atomic_add(P.n_ungrouped, (uint64_t)__popcll(lost));
    const uint64_t members = __ballot(member);
    if (members == 0u) continue;
    const int32_t g0 = __shfl(g, __ffsll((long long)members) - 1, kWave);
    const bool one_group = __ballot(member && g != g0) == 0u;
    // the seven counts, under fognet_job_stats' rules
    const bool aborts = (ok || s.status == FOGNET_REF_ABORTED) && s.abort_tick != INT64_MAX;
    const bool adds = member && ok;
    uint64_t head[GroupOps::kHeadWords] = {member ? 1u : 0u,
                                           member && !ok ? 1u : 0u,
                                           member && aborts ? 1u : 0u,
                                           adds ? (uint64_t)s.n_tasks : 0u,
                                           adds ? (uint64_t)s.n_queued : 0u,
                                           adds ? (uint64_t)s.n_started : 0u,
                                           adds ? (uint64_t)s.events : 0u};
    if (one_group) {  // (wave-uniform) one butterfly per signal, one commit by lane 0
      fognet_group_stats* const rec = acc + g0;
#pragma unroll
      for (int w = 0; w < GroupOps::kHeadWords; ++w) {
        for (int x = kWave / 2; x > 0; x >>= 1) head[w] += shfl_xor_u64(head[w], x);
        if (lane == 0) atomic_add(reinterpret_cast<uint64_t*>(rec) + w, head[w]);
      }
#pragma unroll 1
      for (int k = 0; k < kSignals; ++k) {
        Part p = part_identity();
        if (adds) p = part_of(s, m, k);
        wave_merge_part(p);
        if (lane == 0) commit_part(signal_of(rec, k), p);
      }
    } else if (member) {
      fognet_group_stats* const rec = acc + g;
#pragma unroll
      for (int w = 0; w < GroupOps::kHeadWords; ++w) atomic_add(reinterpret_cast<uint64_t*>(rec) + w, head[w]);
      if (ok) {
#pragma unroll 1
        for (int k = 0; k < kSignals; ++k) commit_part(signal_of(rec, k), part_of(s, m, k));
      }
    }
  }
  if (kLds) {
    // the workgroup's non-empty records, added to the caller's: one thread per (record, head or signal)
    __syncthreads();
    for (int i = tid; i < P.G * (1 + kSignals); i += kPassThreads) {
      const int g = i / (1 + kSignals), k = i % (1 + kSignals) - 1;
      fognet_group_stats* const src = acc + g;
      if (src->n_reps == 0) continue;  // no member of g in this workgroup
      if (k < 0) {
        for (int w = 0; w < GroupOps::kHeadWords; ++w)
          atomic_add(reinterpret_cast<uint64_t*>(P.out + g) + w, reinterpret_cast<const uint64_t*>(src)[w]);
      } else {
        const fognet_moments& q = *signal_of(src, k);
        commit_part(signal_of(P.out + g, k), Part{(uint64_t)q.count, (uint64_t)q.overflow,
                                                  Sig{q.min_raw, q.max_raw, q.sum_lo, q.sum_hi, q.sq_lo, q.sq_hi, q.sq_top}});
      }
    }
  }
}

}  // namespace

hipError_t launch_reduce_groups(const fognet_rep_stats* stats, int32_t R, const int32_t* group_of, int32_t G,
                                fognet_group_stats* out, int64_t* metrics, uint32_t* defined, int64_t* n_ungrouped,
                                bool force_hbm, hipStream_t s) {
  const size_t words = (size_t)G * kRecWords;
  const size_t clear_blocks = (words + kPassThreads - 1) / kPassThreads;
  hipLaunchKernelGGL(group_clear_kernel, dim3((unsigned)(clear_blocks < 4096 ? clear_blocks : 4096)), dim3(kPassThreads), 0,
                     s, reinterpret_cast<uint64_t*>(out), words, n_ungrouped);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || R <= 0) return e;
  const GroupArgs p{stats, group_of, R, G, out, metrics, defined, n_ungrouped};
  // two workgroups per CU at most: each flushes up to FOGNET_GROUP_LDS_MAX records at its end
  const int64_t need = ((int64_t)R + kPassThreads - 1) / kPassThreads;
  const dim3 grid((unsigned)(need < 512 ? need : 512));
  if (G <= FOGNET_GROUP_LDS_MAX && !force_hbm)
    hipLaunchKernelGGL(group_kernel<true>, grid, dim3(kPassThreads), (size_t)G * sizeof(fognet_group_stats), s, p);
  else
    hipLaunchKernelGGL(group_kernel<false>, grid, dim3(kPassThreads), 0, s, p);
  return hipGetLastError();
}

}  // namespace fognet
