// quantiles.hip — exact quantiles of the five recorded signals of a finished replay, per
// replication (fognet_quantiles_dev) and of the job's pooled population
// (fognet_job_quantiles_dev).  Which values a publish emits is signals.h's emission rule;
// fognet_hip.h ("Quantiles") states the populations and the nearest-rank rule.
//
// The pass is a radix select over the order-preserving key raw ^ 2^63, most significant byte
// first.  No value is ever stored: every round streams the replication's rows again
// (signals.h's stream_rows; 33 B per task, 34 under EXT_HIER, 29 with U = 0), forms the values
// with emissions() and counts the next byte of the members whose higher bytes equal the prefix
// of a (signal, rank).  A pick then walks the 256 counts to the byte that holds the rank,
// subtracts the counts below it and extends the prefix.  After the eighth byte the prefix is
// the key of the rank's value.  Every count is an integer atomic, so two runs are
// byte-identical.
//
// Two things decide the time.
//   Colliding bytes.  Real populations are narrow: the high bytes of a signal are shared by
//   all 64 lanes of a step, and every delay of a user is one value.  Where the counting lanes
//   of a signal agree on the counter (one ballot against the first lane's byte), one lane adds
//   their number; otherwise each adds its own.  Ranks whose prefixes are equal share one
//   histogram (the first of them owns it), so round one counts once per signal.  Measured at C3
//   (DESIGN.md §8f): the shared histograms are worth 7% at three ranks and 22 to 37% at eight, the
//   one add per wavefront 0 to 8% (the LDS atomic unit takes a wave on one counter well).
//   Rounds that decide nothing.  A first pass takes each signal's size, minimum and maximum.
//   The leading bytes that the two extrema share are shared by every member, so the select of
//   a signal starts behind them; a signal whose extrema are equal is finished.  A round in
//   which no signal takes part streams nothing.  FOGNET_QUANTILES=full starts every signal at
//   byte 0; the results are identical.
//
// Per replication: one kPassThreads workgroup runs the extent pass and all rounds in one
// launch, counters (32-bit: a replication's population is below 2 T) and select state in LDS.
// Per job: the same row kernel, one phase per launch, with the job's select state read from
// the workspace (QuantWs); it adds the non-zero bins of its LDS counters to the workspace's
// [5][Q][256] table of 64-bit counters, and a one-workgroup pick kernel after it extends the
// prefixes and clears the table.
#include "signals.h"

namespace fognet {

namespace {

constexpr int kQSignals = FOGNET_QUANTILE_SIGNALS;
constexpr int kQMax = FOGNET_QUANTILE_MAX;
constexpr int kBins = 256;
constexpr int kRounds = 8;
constexpr uint64_t kSignBit = (uint64_t)1 << 63;
// The two ways of sharing counter updates, each measured against a timing build without it
// (DESIGN.md §8f): one add per wavefront where its lanes agree on the counter, and one histogram for
// the ranks whose prefixes are equal.
#ifndef FOGNET_QUANTILE_WAVE_SUM
#define FOGNET_QUANTILE_WAVE_SUM 1
#endif
#ifndef FOGNET_QUANTILE_SHARE_HISTOGRAMS
#define FOGNET_QUANTILE_SHARE_HISTOGRAMS 1
#endif

// The select of one population set: five signals, up to kQMax ranks each.
struct QState {
  uint64_t prefix[kQSignals][kQMax];  // the key bytes found so far, in place; the bytes below them 0
  uint64_t rank[kQSignals][kQMax];    // 1-based, among the members that share the prefix
  uint64_t n[kQSignals];              // the population's size
  uint64_t kmin[kQSignals], kmax[kQSignals];  // its extreme keys
  int32_t start[kQSignals];           // the first round the signal takes part in; kRounds: finished
  uint32_t own[kQSignals];            // bit q: rank q owns a histogram (no rank before it has its prefix)
  uint8_t hist_of[kQSignals][kQMax];  // the rank whose histogram rank q reads
};
static_assert(sizeof(QState) == kQuantStateBytes, "workspace.h's size of the job's select state");
static_assert(kQSignals * kQMax * kBins * sizeof(uint32_t) + sizeof(QState) + 256 <= 65536, "counters and state fit in LDS");

struct QuantArgs : UserLinks {
  int64_t* value;         // per replication [R][5][Q]; job [5][Q]
  int64_t* count;         // per replication [R][5]; job [5]
  int64_t* n_unassigned;  // [R], nullable (per replication only)
  uint64_t* table;        // job: [5][Q][256] counters of the round
  QState* job;            // job: the select state
  int32_t ppm[kQMax];
  int32_t Q;
  int32_t full;           // every signal starts at round 0
};

// the bytes of a key above round d's
__device__ __forceinline__ uint64_t mask_above(int d) { return d == 0 ? 0u : ~(uint64_t)0 << (64 - 8 * d); }

// ---------------------------------------------------------------- the values of a publish
// Up to six values: f(signal, has, key), in a fixed order, called by the whole wave.
template <class F>
__device__ __forceinline__ void each_value(const ReplayArgs& A, const QuantArgs& P, const Row& cur, bool decided,
                                           size_t nbase, size_t lbase, uint32_t& unassigned, F&& f) {
  const uint32_t u = (uint32_t)cur.user;
  const bool user = decided && u < (uint32_t)P.U;  // the publish has a user: its user-side values exist
  unassigned += (uint32_t)__popcll(ballot(decided && !user));
  const Emissions e = emissions(
      A, cur, [&](int k) { return A.dl[nbase + k]; }, [&](int k) { return A.ul[nbase + k]; },
      user ? P.ul[lbase + u] : 0, user ? P.dl[lbase + u] : 0);
  int64_t raw = 0;
  bool has = decided && e.queued && qtime_raw(e.queue_start, e.queue_enq, raw);
  f(0, has, (uint64_t)raw ^ kSignBit);
  f(1, user, (uint64_t)e.delay ^ kSignBit);
  const bool first = user && e.first != kAckNone && ms_raw(e.first_d, raw);  // one value, latency or latencyH1
  const uint64_t key_first = (uint64_t)raw ^ kSignBit;
  f(2, first && e.first == kAckLatency, key_first);
  has = user && ms_raw(e.puback_d, raw);
  f(3, has, (uint64_t)raw ^ kSignBit);
  f(3, first && e.first == kAckLatencyH1, key_first);
  has = user && e.completed && ms_raw(e.done_d, raw);
  f(4, has, (uint64_t)raw ^ kSignBit);
}

template <class F>
__device__ __forceinline__ void each_row(const ReplayArgs& A, const QuantArgs& P, int r, uint32_t& unassigned, F&& f) {
  const size_t nbase = (size_t)r * (size_t)A.node_stride, lbase = (size_t)r * (size_t)P.link_stride;
  const int U = P.U;
  auto load = [&](size_t o) {
    return U > 0 ? load_row<kColStart | kColUser | kColEsc>(A, P.user_of, o)
                 : load_row<kColStart | kColEsc>(A, nullptr, o);  // (U = 0: user_of may be NULL)
  };
  stream_rows(A, r, decided_tasks(A, r), load, [&](const Row& cur, int, bool decided) {
    each_value(A, P, cur, decided, nbase, lbase, unassigned, f);
  });
}

// ---------------------------------------------------------------- the extent pass
// size and extreme keys of the five populations into st (LDS atomics)
__device__ __forceinline__ void extent_pass(const ReplayArgs& A, const QuantArgs& P, int r, QState& st,
                                            unsigned long long* s_unassigned) {
  const int lane = (int)threadIdx.x & (kWave - 1);
  uint32_t n[kQSignals], unassigned = 0u;
  uint64_t mn[kQSignals], mx[kQSignals];
#pragma unroll
  for (int s = 0; s < kQSignals; ++s) n[s] = 0u, mn[s] = ~(uint64_t)0, mx[s] = 0u;
  each_row(A, P, r, unassigned, [&](int s, bool has, uint64_t key) {
    if (has) {
      n[s] += 1u;
      mn[s] = key < mn[s] ? key : mn[s];
      mx[s] = key > mx[s] ? key : mx[s];
    }
  });
#pragma unroll
  for (int s = 0; s < kQSignals; ++s) {
    const uint32_t total = wave_sum_u32(n[s]);
    const uint64_t lo = wave_min_u64(mn[s]), hi = ~wave_min_u64(~mx[s]);
    if (lane == 0 && total != 0u) {
      (void)atomicAdd((unsigned long long*)&st.n[s], (unsigned long long)total);
      (void)atomicMin((unsigned long long*)&st.kmin[s], (unsigned long long)lo);
      (void)atomicMax((unsigned long long*)&st.kmax[s], (unsigned long long)hi);
    }
  }
  if (lane == 0 && unassigned != 0u) (void)atomicAdd(s_unassigned, (unsigned long long)unassigned);
}

__device__ __forceinline__ void state_clear(QState& st, int tid) {
  if (tid < kQSignals) st.n[tid] = 0u, st.kmin[tid] = ~(uint64_t)0, st.kmax[tid] = 0u, st.start[tid] = kRounds, st.own[tid] = 0u;
  if (tid < kQSignals * kQMax) {
    st.prefix[tid / kQMax][tid % kQMax] = 0u, st.rank[tid / kQMax][tid % kQMax] = 0u;
    st.hist_of[tid / kQMax][tid % kQMax] = 0;
  }
}

// which ranks own a histogram: the first of every set of equal prefixes (one thread per signal)
__device__ __forceinline__ void share_histograms(QState& st, int Q, int s) {
  uint32_t own = 0u;
  for (int q = 0; q < Q; ++q) {
    int h = q;
    for (int p = 0; p < q; ++p)
      if (FOGNET_QUANTILE_SHARE_HISTOGRAMS && st.prefix[s][p] == st.prefix[s][q]) {
        h = p;
        break;
      }
    st.hist_of[s][q] = (uint8_t)h;
    if (h == q) own |= 1u << q;
  }
  st.own[s] = own;
}

// From the extents to the ranks and the first round of every signal (one thread per signal).
// k = max(1, ceil(n * ppm / 10^6)); n * ppm stays below 2^60.
__device__ __forceinline__ void plan(QState& st, const QuantArgs& P, int s) {
  const uint64_t n = st.n[s];
  const uint64_t diff = st.kmin[s] ^ st.kmax[s];
  const int common = n == 0u || diff == 0u ? kRounds : __clzll((long long)diff) / 8;  // bytes shared by every member
  const int start = n == 0u ? kRounds : P.full ? 0 : common;
  st.start[s] = start;
  for (int q = 0; q < P.Q; ++q) {
    const uint64_t k = (n * (uint64_t)P.ppm[q] + 999999u) / 1000000u;
    st.rank[s][q] = k < 1u ? 1u : k;
    st.prefix[s][q] = st.kmin[s] & mask_above(start);  // (start 8: the whole key)
  }
  share_histograms(st, P.Q, s);
}

__device__ __forceinline__ bool takes_part(const QState& st, int s, int d) { return d >= st.start[s]; }

__device__ __forceinline__ bool round_runs(const QState& st, int d) {
  bool any = false;
  for (int s = 0; s < kQSignals; ++s) any = any || takes_part(st, s, d);
  return any;
}

// ---------------------------------------------------------------- one round's counts
// byte d of the members under each owning rank's prefix into cnt [5][Q][256] (LDS)
__device__ __forceinline__ void count_pass(const ReplayArgs& A, const QuantArgs& P, int r, const QState& st, int d,
                                           uint32_t* cnt) {
  const int lane = (int)threadIdx.x & (kWave - 1);
  const int Q = P.Q, shift = 56 - 8 * d;
  const uint64_t above = mask_above(d);
  uint32_t own[kQSignals];  // (wave-uniform; 0: the signal sits this round out)
#pragma unroll
  for (int s = 0; s < kQSignals; ++s)
    own[s] = (uint32_t)__builtin_amdgcn_readfirstlane((int)(takes_part(st, s, d) ? st.own[s] : 0u));
  uint32_t unassigned = 0u;
  each_row(A, P, r, unassigned, [&](int s, bool has, uint64_t key) {
    const uint32_t idx = (uint32_t)(key >> shift) & (kBins - 1);
    for (uint32_t m = own[s]; m != 0u; m &= m - 1u) {
      const int q = __ffs((int)m) - 1;
      const bool in = has && (key & above) == st.prefix[s][q];
      const uint64_t act = ballot(in);
      if (act == 0u) continue;
      uint32_t* const c = cnt + ((size_t)s * Q + q) * kBins;
      const int leader = __ffsll((long long)act) - 1;
      const uint32_t idx0 = readlane_u32(idx, leader);
      if (FOGNET_QUANTILE_WAVE_SUM && ballot(in && idx != idx0) == 0u) {  // the lanes agree on the counter: one add of their number
        if (lane == leader) (void)atomicAdd(&c[idx0], (uint32_t)__popcll(act));
      } else if (in) {
        (void)atomicAdd(&c[idx], 1u);
      }
    }
  });
}

// rank q of signal s walks its histogram (counts c [256]) to the byte of round d
template <class Count>
__device__ __forceinline__ void pick(QState& st, int s, int q, int d, const Count* c) {
  const uint64_t k = st.rank[s][q];
  uint64_t below = 0u;
  int b = 0;
  for (; b < kBins - 1; ++b) {
    const uint64_t here = (uint64_t)c[b];
    if (k <= below + here) break;
    below += here;
  }
  st.rank[s][q] = k - below;
  st.prefix[s][q] |= (uint64_t)b << (56 - 8 * d);
}

// value [5][Q], count [5] of a finished select (tid < 5 * Q)
__device__ __forceinline__ void write_results(const QState& st, int Q, int tid, int64_t* value, int64_t* count) {
  if (tid >= kQSignals * Q) return;
  const int s = tid / Q, q = tid % Q;
  value[tid] = st.n[s] == 0u ? INT64_MAX : (int64_t)(st.prefix[s][q] ^ kSignBit);
  if (q == 0) count[s] = (int64_t)st.n[s];
}

// ---------------------------------------------------------------- the row kernel
// kJob = false: replication blockIdx.x whole (phase unused).  kJob: one phase of the job's select
// over replication blockIdx.x: -1 the extents, d >= 0 round d's counts.
template <bool kJob>
__global__ __launch_bounds__(kPassThreads) void quantile_rows_kernel(ReplayArgs A, QuantArgs P, int phase) {
  extern __shared__ uint32_t s_cnt[];  // [5][Q][256]
  __shared__ QState st;
  __shared__ unsigned long long s_unassigned;
  const int r = blockIdx.x, tid = (int)threadIdx.x, Q = P.Q;
  const int words = kQSignals * Q * kBins;
  if (kJob) {
    if (A.out_stats[r].status != FOGNET_OK) return;  // (the job reductions' rule)
  } else if (!rep_ok(A, r)) {  // (nothing of its rows, users or links is read)
    if (tid < kQSignals * Q) P.value[(size_t)r * kQSignals * Q + tid] = INT64_MAX;
    if (tid < kQSignals) P.count[(size_t)r * kQSignals + tid] = 0;
    if (tid == 0 && P.n_unassigned) P.n_unassigned[r] = 0;
    return;
  }
  if (kJob && phase >= 0) {
    uint64_t* const dst = reinterpret_cast<uint64_t*>(&st);
    const uint64_t* const src = reinterpret_cast<const uint64_t*>(P.job);
    for (int w = tid; w < (int)(sizeof(QState) / 8); w += kPassThreads) dst[w] = src[w];
  } else {
    state_clear(st, tid);
  }
  if (tid == 0) s_unassigned = 0u;
  __syncthreads();
  if (!kJob || phase < 0) {
    extent_pass(A, P, r, st, &s_unassigned);
    __syncthreads();
    if (kJob) {
      if (tid < kQSignals && st.n[tid] != 0u) {
        (void)atomicAdd((unsigned long long*)&P.job->n[tid], (unsigned long long)st.n[tid]);
        (void)atomicMin((unsigned long long*)&P.job->kmin[tid], (unsigned long long)st.kmin[tid]);
        (void)atomicMax((unsigned long long*)&P.job->kmax[tid], (unsigned long long)st.kmax[tid]);
      }
      return;
    }
    if (tid < kQSignals) plan(st, P, tid);
    __syncthreads();
  }
  for (int d = kJob ? phase : 0; d < (kJob ? phase + 1 : kRounds); ++d) {
    if (!round_runs(st, d)) continue;  // (uniform: st is not written since the last barrier)
    for (int w = tid; w < words; w += kPassThreads) s_cnt[w] = 0u;
    __syncthreads();
    count_pass(A, P, r, st, d, s_cnt);
    __syncthreads();
    if (kJob) {
      for (int w = tid; w < words; w += kPassThreads)
        if (s_cnt[w] != 0u) (void)atomicAdd((unsigned long long*)&P.table[w], (unsigned long long)s_cnt[w]);
      return;
    }
    if (tid < kQSignals * Q && takes_part(st, tid / Q, d))
      pick(st, tid / Q, tid % Q, d, s_cnt + (size_t)(tid / Q * Q + st.hist_of[tid / Q][tid % Q]) * kBins);
    __syncthreads();
    if (tid < kQSignals) share_histograms(st, Q, tid);
    __syncthreads();
  }
  if (!kJob) {
    write_results(st, Q, tid, P.value + (size_t)r * kQSignals * Q, P.count + (size_t)r * kQSignals);
    if (tid == 0 && P.n_unassigned) P.n_unassigned[r] = (int64_t)s_unassigned;
  }
}

// ---------------------------------------------------------------- the job's pick kernel
// One workgroup between the row launches.  phase -2: clear the state and the table; -1: plan from
// the extents; d >= 0: extend the prefixes by round d's byte and clear the table; the last round
// writes the results.
__global__ __launch_bounds__(kPassThreads) void quantile_pick_kernel(QuantArgs P, int phase) {
  __shared__ QState st;
  __shared__ uint64_t s_tab[kQMax * kBins];
  const int tid = (int)threadIdx.x, Q = P.Q;
  const int words = kQSignals * Q * kBins;
  uint64_t* const mem = reinterpret_cast<uint64_t*>(P.job);
  uint64_t* const loc = reinterpret_cast<uint64_t*>(&st);
  if (phase == -2) {
    state_clear(st, tid);
    for (int w = tid; w < words; w += kPassThreads) P.table[w] = 0u;
  } else {
    for (int w = tid; w < (int)(sizeof(QState) / 8); w += kPassThreads) loc[w] = mem[w];
  }
  __syncthreads();
  if (phase == -1) {
    if (tid < kQSignals) plan(st, P, tid);
  } else if (phase >= 0 && round_runs(st, phase)) {
    for (int s = 0; s < kQSignals; ++s) {
      if (!takes_part(st, s, phase)) continue;  // (uniform; its part of the table stayed zero)
      uint64_t* const t = P.table + (size_t)s * Q * kBins;
      for (int w = tid; w < Q * kBins; w += kPassThreads) {
        s_tab[w] = t[w];
        t[w] = 0u;
      }
      __syncthreads();
      if (tid < Q) pick(st, s, tid, phase, s_tab + (size_t)st.hist_of[s][tid] * kBins);
      __syncthreads();
    }
    if (tid < kQSignals) share_histograms(st, Q, tid);
  }
  __syncthreads();
  for (int w = tid; w < (int)(sizeof(QState) / 8); w += kPassThreads) mem[w] = loc[w];
  if (phase == kRounds - 1 && P.value) write_results(st, Q, tid, P.value, P.count);
}

QuantArgs quant_args(const UserLinks& users, const int32_t* ppm, int32_t Q, bool full) {
  QuantArgs p{};
  static_cast<UserLinks&>(p) = users;
  for (int q = 0; q < Q; ++q) p.ppm[q] = ppm[q];
  p.Q = Q, p.full = full ? 1 : 0;
  return p;
}

}  // namespace

size_t quantiles_table_count(int32_t Q) { return (size_t)kQSignals * (size_t)Q * kBins; }

hipError_t launch_quantiles(const ReplayArgs& a, const UserLinks& users, const int32_t* ppm, int32_t Q, int64_t* value,
                            int64_t* count, int64_t* n_unassigned, bool full, hipStream_t s) {
  if (a.R <= 0) return hipSuccess;
  QuantArgs p = quant_args(users, ppm, Q, full);
  p.value = value, p.count = count, p.n_unassigned = n_unassigned;
  const size_t lds = quantiles_table_count(Q) * sizeof(uint32_t);
  hipLaunchKernelGGL(quantile_rows_kernel<false>, dim3(a.R), dim3(kPassThreads), lds, s, a, p, 0);
  return hipGetLastError();
}

hipError_t launch_job_quantiles(const ReplayArgs& a, const UserLinks& users, const int32_t* ppm, int32_t Q,
                                int64_t* value, int64_t* count, const QuantWs& w, bool full, hipStream_t s) {
  QuantArgs p = quant_args(users, ppm, Q, full);
  p.value = value, p.count = count, p.n_unassigned = nullptr;
  p.table = w.table, p.job = reinterpret_cast<QState*>(w.state);
  const size_t lds = quantiles_table_count(Q) * sizeof(uint32_t);
  // -2 clears, -1 takes the extents, then the eight rounds; a round that no signal takes part in
  // costs two launches that return at once (which rounds run is known on the device only)
  for (int phase = -2; phase < kRounds; ++phase) {
    if (phase >= -1 && a.R > 0)
      hipLaunchKernelGGL(quantile_rows_kernel<true>, dim3(a.R), dim3(kPassThreads), lds, s, a, p, phase);
    hipLaunchKernelGGL(quantile_pick_kernel, dim3(1), dim3(kPassThreads), 0, s, p, phase);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace fognet
