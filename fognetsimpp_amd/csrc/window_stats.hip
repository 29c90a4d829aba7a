// window_stats.hip — the statistics of a finished replay per window of sim time
// (fognet_window_stats_dev) and their job reduction (fognet_reduce_window_stats_dev): the five
// recorded signals, the publishes and the completions binned by the time of each event, and the
// two time averages of a queueing study, node-ticks of service (busy) and task-ticks in the
// system (insys), as the part of every task's interval that lies in each window.  Which events a
// publish has, with which times and values, is signals.h's emission rule; fognet_hip.h states
// what the record holds.
//
// The pass is a reduction keyed by window over the replay's per-task arrays (33 B per task; 34
// under EXT_HIER; 29 with U = 0), streamed by one workgroup per replication (signals.h's
// stream_rows).  The accumulators are one fognet_window_stats per window with two cover-count
// deltas beside it: in LDS up to kWinLdsMax windows, above that the caller's records and the
// context's workspace (signals.h's keyed frame).  Every update is an integer atomic, so the
// records do not depend on the order of the updates and two runs are byte-identical.
//
// Point events.  A task has up to seven events at up to six times, so each goes to its own
// window: the index is an exact division by the run-time window length (win_div: a reciprocal estimate, then
// one exact correction step).  Trace order is nearly time order, so the 64 tasks of a step mostly
// share one window per signal: a signal whose emitting lanes agree on the window, and are at
// least the layout's threshold, is summed across the wave (wave_merge2, two signals per
// butterfly) and committed once; otherwise every lane commits its own.
//
// Intervals.  [a, b) is clipped to the covered range; its partial end windows add their ticks
// to the record's 128-bit sum directly, and the windows it covers whole are counted by a
// difference array: +1 at wa + 1, -1 at wb.  After the row loop a workgroup scan over w (chunks
// of kPassThreads with a carry) turns the deltas into cover counts, and cover * window_tick is
// added in 128 bits.  The cost per task does not depend on how many windows it spans.
#include "signals.h"

namespace fognet {

namespace {

constexpr int kWinThreads = kPassThreads;
// 408 B of record + 16 B of deltas per window; the limit is the header's, measured: the most
// windows whose records fit the 64 KiB of LDS a workgroup may ask for (62 KiB, two workgroups per CU)
constexpr int kWinLdsMax = FOGNET_WINDOW_LDS_WINDOWS;
static_assert((size_t)kWinLdsMax * 424 + 88 <= 65536, "the records and deltas of kWinLdsMax windows fit in LDS");
// The fewest emitting lanes of a signal that are summed across the wave when their windows agree,
// per layout; above kWave none is.  Measured: on the caller's records the summing
// is worth a factor of 2.3 to 2.5 at C3, the same from 4, 8, 16 or 32 lanes on; in LDS it gains 3%
// there at 137 VGPRs instead of 54, and is left out.
#ifndef FOGNET_WINDOW_REDUCE_LDS
#define FOGNET_WINDOW_REDUCE_LDS (kWave + 1)
#endif
#ifndef FOGNET_WINDOW_REDUCE_HBM
#define FOGNET_WINDOW_REDUCE_HBM 8
#endif

// fognet_window_stats as signals.h takes a record: two counts and two 128-bit sums, then five fognet_moments
struct WindowOps {
  using Rec = fognet_window_stats;
  static constexpr int kHeadWords = 6;
  static __device__ __forceinline__ uint64_t head_empty(int) { return 0u; }
  static __device__ __forceinline__ void merge(Rec& a, const Rec& b) {
    a.n_publish += b.n_publish;
    a.n_complete += b.n_complete;
    add128(a.busy_lo, a.busy_hi, b.busy_lo, b.busy_hi);
    add128(a.insys_lo, a.insys_hi, b.insys_lo, b.insys_hi);
    moments_merge(a.queue, b.queue);
    moments_merge(a.delay, b.delay);
    moments_merge(a.latency, b.latency);
    moments_merge(a.latencyH1, b.latencyH1);
    moments_merge(a.taskTime, b.taskTime);
  }
};
constexpr int kWRecWords = rec_words<WindowOps>();
static_assert(sizeof(fognet_window_stats) == 408 && kWRecWords == 51, "fognet_window_stats is 51 words");
static_assert(offsetof(fognet_window_stats, queue) == 6 * 8, "the head is six words");

using MomentsOf = fognet_moments fognet_window_stats::*;
using CountOf = int64_t fognet_window_stats::*;

// ---------------------------------------------------------------- windows
struct WindowArgs : UserLinks {
  fognet_window_stats* out;  // [R][W]
  int64_t* n_outside;        // [R][2], nullable
  int64_t* n_unassigned;     // [R], nullable
  int64_t* ws_delta;         // [R][W][2] the cover-count deltas of the layout without LDS
  int64_t t0, d, span;       // the covered range [t0, t0 + span), span = W * d
  double inv_d;              // 1 / d, rounded
  int32_t W;
};

// x / d and x % d for 0 <= x <= span: the quotient is at most 2^20 and the estimate's relative
// error below 2^-50, so the estimate is off by at most one, which the exact remainder shows.
__device__ __forceinline__ int32_t win_div(const WindowArgs& P, int64_t x, int64_t& rem) {
  int64_t q = (int64_t)((double)x * P.inv_d);
  int64_t r = (int64_t)((uint64_t)x - (uint64_t)q * (uint64_t)P.d);
  if (r < 0) {
    --q;
    r += P.d;
  } else if (r >= P.d) {
    ++q;
    r -= P.d;
  }
  rem = r;
  return (int32_t)q;
}

// the window of a point event at tick `at`: -1 before the range, W at or past its end
__device__ __forceinline__ int32_t window_of(const WindowArgs& P, int64_t at) {
  const int64_t x = at - P.t0;
  if (x < 0) return -1;
  if (x >= P.span) return P.W;
  int64_t rem;
  return win_div(P, x, rem);
}

// ---------------------------------------------------------------- point events
// the lanes `in` agree on their window (and are enough to be summed): `leader` is the first of them
template <int kThr>
__device__ __forceinline__ bool agree(bool in, int32_t w, int& leader) {
  if (kThr > kWave) return false;
  const uint64_t act = ballot(in);
  if (__popcll(act) < kThr) return false;  // (kThr >= 1: an empty set is never summed)
  leader = __ffsll((long long)act) - 1;
  const int32_t w0 = (int32_t)readlane_u32((uint32_t)w, leader);
  return ballot(in && w != w0) == 0u;
}

__device__ __forceinline__ Sig sig_of(bool emits, int64_t raw) {
  Sig s = sig_identity();
  if (emits) sig_add(s, raw);
  return s;
}

// Two signals of the step: in*: the lane has this event, inside the range, in window w*; ok*: its
// value is in the simtime_t range (else a lost emission, counted in the window's overflow).
template <int kThr>
__device__ __forceinline__ void point_pair(fognet_window_stats* acc, int lane, MomentsOf ma, bool in_a, int32_t wa,
                                           bool ok_a, int64_t raw_a, MomentsOf mb, bool in_b, int32_t wb, bool ok_b,
                                           int64_t raw_b) {
  int lead_a = 0, lead_b = 0;
  const bool sum_a = agree<kThr>(in_a, wa, lead_a), sum_b = agree<kThr>(in_b, wb, lead_b);
  if (sum_a || sum_b) {  // (wave-uniform)
    Sig a = sig_of(sum_a && in_a && ok_a, raw_a), b = sig_of(sum_b && in_b && ok_b, raw_b);
    NoHead none;
    wave_merge2(a, b, none);
    const uint64_t n_a = (uint64_t)__popcll(ballot(in_a && ok_a)), o_a = (uint64_t)__popcll(ballot(in_a && !ok_a));
    const uint64_t n_b = (uint64_t)__popcll(ballot(in_b && ok_b)), o_b = (uint64_t)__popcll(ballot(in_b && !ok_b));
    if (sum_a && lane == lead_a) commit_sig(&(acc[wa].*ma), n_a, o_a, a);
    if (sum_b && lane == lead_b) commit_sig(&(acc[wb].*mb), n_b, o_b, b);
  }
  if (in_a && !sum_a) commit_sig(&(acc[wa].*ma), ok_a ? 1u : 0u, ok_a ? 0u : 1u, sig_of(ok_a, raw_a));
  if (in_b && !sum_b) commit_sig(&(acc[wb].*mb), ok_b ? 1u : 0u, ok_b ? 0u : 1u, sig_of(ok_b, raw_b));
}

template <int kThr>
__device__ __forceinline__ void point_count(fognet_window_stats* acc, int lane, CountOf m, bool in, int32_t w) {
  int leader = 0;
  if (agree<kThr>(in, w, leader)) {
    const uint64_t n = (uint64_t)__popcll(ballot(in));  // (by the whole wave, before the leader goes alone)
    if (lane == leader) atomic_add(&(acc[w].*m), n);
  } else if (in) {
    atomic_add(&(acc[w].*m), 1u);
  }
}

// ---------------------------------------------------------------- intervals
// ticks into the 128-bit sum at `lo` of window w's record: summed across the wave where the lanes agree
template <int kThr>
__device__ __forceinline__ void edge_add(fognet_window_stats* acc, int lane, uint64_t fognet_window_stats::*lo, bool in,
                                         int32_t w, uint64_t v) {
  int leader = 0;
  if (agree<kThr>(in, w, leader)) {
    // 64 values below 2^62: the halves' sums stay below 2^38
    const uint64_t s_lo = wave_sum_u64(in ? v & 0xFFFFFFFFu : 0u), s_hi = wave_sum_u64(in ? v >> 32 : 0u);
    uint64_t t_lo = s_lo, t_hi = 0u;
    add128(t_lo, t_hi, s_hi << 32, s_hi >> 32);
    if (lane == leader) atomic_add128(&(acc[w].*lo), &(acc[w].*lo) + 1, t_lo, t_hi);
  } else if (in && v != 0u) {
    atomic_add128(&(acc[w].*lo), &(acc[w].*lo) + 1, v, 0u);
  }
}

// [a, b) into the sum at `lo` and the cover deltas delta[2 * w + which]
template <int kThr>
__device__ __forceinline__ void interval_add(const WindowArgs& P, fognet_window_stats* acc, int64_t* delta, int lane,
                                             uint64_t fognet_window_stats::*lo, int which, bool has, int64_t a, int64_t b) {
  // clipped to the range, relative to t0: 0 <= xa < xb <= span where anything is left
  const int64_t xa = (a > P.t0 ? a : P.t0) - P.t0;
  const int64_t xb = b - P.t0 < P.span ? b - P.t0 : P.span;
  const bool in = has && xa < xb;
  int64_t ra = 0, rb = 0;
  int32_t wa = 0, wb = 0;
  if (in) {
    wa = win_div(P, xa, ra);
    wb = win_div(P, xb, rb);  // (xb == span: window W with nothing in it, never indexed)
  }
  const bool one = wa == wb;
  edge_add<kThr>(acc, lane, lo, in, wa, (uint64_t)(one ? xb - xa : P.d - ra));
  edge_add<kThr>(acc, lane, lo, in && !one && rb > 0, wb, (uint64_t)rb);
  if (in && wa + 1 < wb) {  // the windows wa + 1 .. wb - 1 lie in it whole
    atomic_add(&delta[2 * (size_t)(wa + 1) + which], 1u);
    if (wb < P.W) atomic_add(&delta[2 * (size_t)wb + which], ~(uint64_t)0);
  }
}

// ---------------------------------------------------------------- the pass
// kLds: the records and the deltas live in LDS
template <bool kLds>
__global__ __launch_bounds__(kWinThreads) void window_stats_kernel(ReplayArgs A, WindowArgs P) {
  extern __shared__ uint64_t s_mem[];  // kLds: [W] records, [W][2] deltas
  __shared__ unsigned long long s_cnt[3];  // events before the range, at or past its end; unassigned publishes
  __shared__ int64_t s_scan[2][kPassWaves];
  const int r = blockIdx.x;
  const int W = P.W, U = P.U;
  const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x / kWave;
  fognet_window_stats* const row = P.out + (size_t)r * (size_t)W;
  fognet_window_stats* const acc = kLds ? reinterpret_cast<fognet_window_stats*>(s_mem) : row;
  int64_t* const delta = kLds ? reinterpret_cast<int64_t*>(s_mem + (size_t)W * kWRecWords)
                              : P.ws_delta + (size_t)r * (size_t)W * 2;
  if (!keyed_begin<WindowOps, kLds>(A, r, row, W, s_mem)) {  // (nothing of its rows, users or links is read)
    if (threadIdx.x < 2 && P.n_outside) P.n_outside[2 * (size_t)r + threadIdx.x] = 0;
    if (threadIdx.x == 0 && P.n_unassigned) P.n_unassigned[r] = 0;
    return;
  }
  if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0u;
  for (int i = threadIdx.x; i < 2 * W; i += kWinThreads) delta[i] = 0;
  keyed_ready<kLds>();
  constexpr int kThr = kLds ? FOGNET_WINDOW_REDUCE_LDS : FOGNET_WINDOW_REDUCE_HBM;
  const size_t nbase = (size_t)r * (size_t)A.node_stride, lbase = (size_t)r * (size_t)P.link_stride;
  uint32_t before = 0u, after = 0u, unassigned = 0u;  // per wavefront (uniform)
  // the window of an event this lane has; counts it where it lies outside the range
  auto place = [&](bool has, int64_t at, int32_t& w) {
    w = has ? window_of(P, at) : 0;
    before += (uint32_t)__popcll(ballot(has && w < 0));
    after += (uint32_t)__popcll(ballot(has && w >= W));
    return has && w >= 0 && w < W;
  };
  auto load = [&](size_t o) {
    return U > 0 ? load_row<kColStart | kColUser | kColEsc>(A, P.user_of, o)
                 : load_row<kColStart | kColEsc>(A, nullptr, o);  // (U = 0: user_of may be NULL)
  };
  stream_rows(A, r, decided_tasks(A, r), load, [&](const Row& cur, int, bool decided) {
    const uint32_t u = (uint32_t)cur.user;
    const bool user = decided && u < (uint32_t)U;  // the publish has a user: its user-side events exist
    unassigned += (uint32_t)__popcll(ballot(decided && !user));
    const Emissions e = emissions(
        A, cur, [&](int k) { return A.dl[nbase + k]; }, [&](int k) { return A.ul[nbase + k]; },
        user ? P.ul[lbase + u] : 0, user ? P.dl[lbase + u] : 0);
    const bool completed = decided && e.completed;
    int32_t w_t, w_x, w_y;
    // at arrive_tick: the publish itself and the broker's delay
    const bool in_t = place(decided, cur.t, w_t);
    point_count<kThr>(acc, lane, &fognet_window_stats::n_publish, in_t, w_t);
    before += (uint32_t)__popcll(ballot(user && w_t < 0));  // (delay: a second event of the same tick)
    after += (uint32_t)__popcll(ballot(user && w_t >= W));
    int64_t raw_x = 0, raw_y = 0;
    bool ok_x = user && ms_raw(e.puback_d, raw_x);
    const bool in_p = place(user, e.puback_at, w_x);
    point_pair<kThr>(acc, lane, &fognet_window_stats::delay, in_t && user, w_t, true, e.delay,
                     &fognet_window_stats::latencyH1, in_p, w_x, ok_x, raw_x);
    // the node's first ack: latency or latencyH1 by its kind, one time for both
    const bool first = user && e.first != kAckNone;
    ok_x = first && ms_raw(e.first_d, raw_x);
    const bool in_f = place(first, e.first_at, w_x);
    point_pair<kThr>(acc, lane, &fognet_window_stats::latency, in_f && e.first == kAckLatency, w_x, ok_x, raw_x,
                     &fognet_window_stats::latencyH1, in_f && e.first == kAckLatencyH1, w_x, ok_x, raw_x);
    // taskTime at the completion ack's arrival, queueTime at the service start
    const bool tt = user && completed, qt = decided && e.queued;
    ok_x = tt && ms_raw(e.done_d, raw_x);
    const bool ok_y = qt && qtime_raw(e.queue_start, e.queue_enq, raw_y);
    const bool in_d = place(tt, e.done_at, w_x), in_q = place(qt, e.queue_start, w_y);
    point_pair<kThr>(acc, lane, &fognet_window_stats::taskTime, in_d, w_x, ok_x, raw_x, &fognet_window_stats::queue,
                     in_q, w_y, ok_y, raw_y);
    const bool in_c = place(completed, cur.done, w_x);
    point_count<kThr>(acc, lane, &fognet_window_stats::n_complete, in_c, w_x);
    interval_add<kThr>(P, acc, delta, lane, &fognet_window_stats::busy_lo, 0, completed, cur.start, cur.done);
    interval_add<kThr>(P, acc, delta, lane, &fognet_window_stats::insys_lo, 1, completed, e.queue_enq, cur.done);
  });
  if (lane == 0) {
    if (before != 0u) (void)atomicAdd(&s_cnt[0], (unsigned long long)before);
    if (after != 0u) (void)atomicAdd(&s_cnt[1], (unsigned long long)after);
    if (unassigned != 0u) (void)atomicAdd(&s_cnt[2], (unsigned long long)unassigned);
  }
  if (!kLds) __threadfence();  // every delta is in memory before the scan reads it
  __syncthreads();
  if (threadIdx.x < 2 && P.n_outside) P.n_outside[2 * (size_t)r + threadIdx.x] = (int64_t)s_cnt[threadIdx.x];
  if (threadIdx.x == 0 && P.n_unassigned) P.n_unassigned[r] = (int64_t)s_cnt[2];
  // inclusive scan of the deltas over w, kWinThreads windows per round with a carry; the cover
  // counts stay below 2^31 (T) and window_tick below 2^62, so the product fits 128 bits
  int64_t carry[2] = {0, 0};
  for (int w0 = 0; w0 < W; w0 += kWinThreads) {
    const int w = w0 + (int)threadIdx.x;
    int64_t c[2] = {0, 0};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (w < W)
        c[k] = kLds ? delta[2 * (size_t)w + k]
                    : (int64_t)__hip_atomic_load(&delta[2 * (size_t)w + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      c[k] = wave_scan_add_i64(c[k]);
      if (lane == kWave - 1) s_scan[k][wave] = c[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      int64_t total = 0;
#pragma unroll
      for (int j = 0; j < kPassWaves; ++j) {
        if (j < wave) c[k] += s_scan[k][j];
        total += s_scan[k][j];
      }
      c[k] += carry[k];
      carry[k] += total;
      if (w < W && c[k] != 0) {
        uint64_t* const lo = k == 0 ? &acc[w].busy_lo : &acc[w].insys_lo;
        atomic_add128(lo, lo + 1, (uint64_t)c[k] * (uint64_t)P.d, __umul64hi((uint64_t)c[k], (uint64_t)P.d));
      }
    }
    __syncthreads();  // (s_scan is rewritten by the next round)
  }
  keyed_end<WindowOps, kLds>(row, W, s_mem);
}

}  // namespace

size_t window_stats_delta_count(int32_t R, int32_t W, bool force_hbm) {
  return W > kWinLdsMax || force_hbm ? (size_t)R * (size_t)W * 2 : 0;
}

hipError_t launch_window_stats(const ReplayArgs& a, const UserLinks& users, int64_t t0, int64_t window, int32_t W,
                               fognet_window_stats* out, int64_t* n_outside, int64_t* n_unassigned, int64_t* ws_delta,
                               bool force_hbm, hipStream_t s) {
  if (a.R <= 0 || (W <= 0 && !n_outside && !n_unassigned)) return hipSuccess;
  WindowArgs p{};
  static_cast<UserLinks&>(p) = users;
  p.out = out, p.n_outside = n_outside, p.n_unassigned = n_unassigned, p.ws_delta = ws_delta;
  p.t0 = t0, p.d = window, p.span = (int64_t)W * window, p.inv_d = 1.0 / (double)window, p.W = W;
  if (W <= kWinLdsMax && !force_hbm) {
    const size_t lds = (size_t)W * (kWRecWords + 2) * sizeof(uint64_t);
    hipLaunchKernelGGL(window_stats_kernel<true>, dim3(a.R), dim3(kWinThreads), lds, s, a, p);
  } else {
    hipLaunchKernelGGL(window_stats_kernel<false>, dim3(a.R), dim3(kWinThreads), 0, s, a, p);
  }
  return hipGetLastError();
}

hipError_t launch_reduce_window_stats(const fognet_window_stats* in, const fognet_rep_stats* stats, int32_t R, int32_t W,
                                      fognet_window_stats* out, hipStream_t s) {
  return launch_reduce<WindowOps>(in, stats, R, W, out, s);
}

}  // namespace fognet
