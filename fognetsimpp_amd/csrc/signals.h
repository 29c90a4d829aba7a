// signals.h — what the passes over a finished replay share (user_stats.hip, node_stats.hip,
// per_user_stats.hip, signal_vectors.hip, window_stats.hip, compare_stats.hip), each stated once: which replications and tasks a
// pass reads, the per-task row and the loop that streams it, the emission rule of a decided
// publish, the moments of one signal with their wave merge and atomic commit, the empty
// record, the frame of a pass keyed by node or user, and the job reduction of its records.
//
// The reference's acks: the broker's own status-4 pubAck at the publish
// (BrokerBaseApp3.cc:145-150), the node's status 5/4 at the task's arrival
// (ComputeBrokerApp3.cc:284-289, 310-313) and status 6 at its completion (:228-233); node
// acks reach the broker one uplink later and are relayed (BrokerBaseApp3.cc:164-198) to the
// user, one user downlink later.  The user emits (simTime() - created) * 1000 for each
// (mqttApp2.cc:252-291; raw simtime_t values, fognet_hip.h "Reference signal values"),
// created = the publish's send time = its broker arrival - the user uplink; the node emits
// queueTime at the service start of a task it had queued (ComputeBrokerApp3.cc:238).  Acks
// carry no state back into the decision loop, so every signal is a closed form of the replay
// outputs; tests/oracle_lib restates them as real FES events.
#pragma once
#include <type_traits>

#include "replay_common.h"

namespace fognet {

constexpr int kPassThreads = 256;  // one workgroup per replication
constexpr int kPassWaves = kPassThreads / kWave;

// ---------------------------------------------------------------- replications and rows
// A failed replication is not read (its rows are undefined, fognet_hip.h "Buffers").
__device__ __forceinline__ bool rep_ok(const ReplayArgs& A, int r) {
  const int32_t s = A.out_stats[r].status;
  return s == FOGNET_OK || s == FOGNET_REF_ABORTED;
}

__device__ __forceinline__ int decided_tasks(const ReplayArgs& A, int r) {
  const int64_t n64 = A.out_stats[r].n_tasks;  // decided tasks (written by the replay)
  return (int)(n64 < 0 ? 0 : n64 > A.T ? A.T : n64);
}

// One task of a finished replay.  arrive, done, node and status (21 B) are always read; a
// pass names the further columns it streams, and the fields of the others stay 0.
enum : unsigned { kColStart = 1u, kColReq = 2u, kColUser = 4u, kColEsc = 8u };
struct Row {
  int64_t t, start, done;
  int32_t req, node, user;
  uint32_t status;
  uint32_t esc;  // EXT_HIER: the parent took the decision (the task reached its node a hop later)
};

// (A.out_esc: the replay's escalation flags, bound by capi.hip under EXT_HIER only)
template <unsigned kCols>
__device__ __forceinline__ Row load_row(const ReplayArgs& A, const int32_t* user_of, size_t o) {
  Row x{};
  x.t = A.arrive[o];
  x.done = A.out_done[o];
  x.node = A.out_node[o];
  x.status = (uint32_t)A.out_status[o];
  if (kCols & kColStart) x.start = A.out_start[o];
  if (kCols & kColReq) x.req = A.req[o];
  if (kCols & kColUser) x.user = user_of[o];
  if ((kCols & kColEsc) && A.out_esc) x.esc = (uint32_t)A.out_esc[o];
  return x;
}

// A kPassThreads workgroup streams replication r's first n tasks, coalesced: 64 tasks per
// wavefront and step, the next step's loads in flight while f(row, task, task < n) handles
// this one.  Lanes past n reload the chunk's first task (in bounds, unused).  The row is whatever
// load(offset) returns (compare_stats.hip streams the rows of two replays as one); T: tasks per replication.
template <class Load, class F>
__device__ __forceinline__ void stream_rows(int T, int r, int n, Load&& load, F&& f) {
  using RowT = decltype(load((size_t)0));
  const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x / kWave;
  const size_t tbase = (size_t)r * (size_t)T;
  const int chunks = (n + kWave - 1) / kWave;
  auto offset_of = [&](int c) { return tbase + (size_t)(c * kWave + lane < n ? c * kWave + lane : c * kWave); };
  RowT cur{};
  if (wave < chunks) cur = load(offset_of(wave));
  for (int c = wave; c < chunks; c += kPassWaves) {
    RowT nxt = cur;
    if (c + kPassWaves < chunks) nxt = load(offset_of(c + kPassWaves));
    const int i = c * kWave + lane;
    f(cur, i, i < n);
    cur = nxt;
  }
}
template <class Load, class F>
__device__ __forceinline__ void stream_rows(const ReplayArgs& A, int r, int n, Load&& load, F&& f) {
  stream_rows(A.T, r, n, load, f);
}

// ---------------------------------------------------------------- the emission rule
// (a decided publish's node lies in [0, N); an index outside it reads node 0's links)
__device__ __forceinline__ int link_node(const ReplayArgs& A, int32_t node) {
  return (uint32_t)node < (uint32_t)A.N ? node : 0;
}

enum AckKind { kAckNone, kAckLatency, kAckLatencyH1 };

// What one decided publish emits: times in ticks, `_d` the ticks since the publish was created.
// A user-side value is ms_raw(_d), a queueTime qtime_raw(queue_start, queue_enq); either can
// leave the simtime_t range, which the moments passes count and the vectors drop.
struct Emissions {
  int64_t delay;                 // at the broker (BrokerBaseApp3.cc:143), at t: a simtime_t (s)
  int64_t puback_at, puback_d;   // the broker's own pubAck, status 4 -> latencyH1
  int64_t first_at, first_d;     // the node's ack, sent at the task's arrival
  AckKind first;                 // status 5 "task assigned" -> latency, 4 "task queued" -> latencyH1,
                                 // 9: the task reached a crashed node, which sends no ack
  int64_t done_at, done_d;       // status 6 -> taskTime
  bool completed;                // (done -1: never completed)
  int64_t queue_start, queue_enq;
  bool queued;                   // queueTime, at the service start of a task the node had queued
};

// dl_of / ul_of: the links of a node in [0, N); uu / ud: the links of the publish's user.
template <class DlOf, class UlOf>
__device__ __forceinline__ Emissions emissions(const ReplayArgs& A, const Row& x, DlOf&& dl_of, UlOf&& ul_of,
                                               int64_t uu, int64_t ud) {
  const int k = link_node(A, x.node);
  // the task reaches its node at t + dl_k, the parent's hop later where it was escalated
  const int64_t at_node = x.t + dl_of(k) + (x.esc ? A.hier_up : 0);
  const int64_t created = x.t - uu;
  const int64_t relay = ul_of(k) + ud;  // node -> broker -> user
  Emissions e;
  e.delay = uu;
  e.puback_at = x.t + ud;
  e.puback_d = e.puback_at - created;
  e.first_at = at_node + relay;
  e.first_d = e.first_at - created;
  e.first = x.status == 5u ? kAckLatency : x.status == 4u ? kAckLatencyH1 : kAckNone;
  e.done_at = x.done + relay;
  e.done_d = e.done_at - created;
  e.completed = x.done >= 0;
  e.queue_start = x.start;
  e.queue_enq = at_node;
  e.queued = k == x.node && x.status == 4u && x.start >= 0;
  return e;
}

// ---------------------------------------------------------------- integer atomics
// Every update of a record in LDS or HBM is a 64-bit integer atomic: sums take their carries
// from the value the atomic add returns, extrema are integer min/max, so a record does not
// depend on the order of its updates.
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

// ---------------------------------------------------------------- the moments of one signal
// extrema, 128-bit sum and 192-bit sum of squares of raw emitted values; the count and the
// lost emissions travel beside it (a byte each of a pass's packed count word)
struct Sig {
  int64_t mn, mx;
  uint64_t s_lo, s_hi, q_lo, q_hi, q_top;
};

__device__ __forceinline__ Sig sig_identity() { return Sig{INT64_MAX, INT64_MIN, 0u, 0u, 0u, 0u, 0u}; }

__device__ __forceinline__ void sig_add(Sig& s, int64_t raw) {
  s.mn = min(s.mn, raw);
  s.mx = max(s.mx, raw);
  add_moment_signed(s.s_lo, s.s_hi, s.q_lo, s.q_hi, s.q_top, raw);
}

__device__ __forceinline__ void sig_merge(Sig& a, const Sig& b) {
  a.mn = min(a.mn, b.mn);
  a.mx = max(a.mx, b.mx);
  add128(a.s_lo, a.s_hi, b.s_lo, b.s_hi);
  add192(a.q_lo, a.q_hi, a.q_top, b.q_lo, b.q_hi, b.q_top);
}

__device__ __forceinline__ Sig sig_shfl_xor(const Sig& a, int m) {
  return Sig{(int64_t)shfl_xor_u64((uint64_t)a.mn, m), (int64_t)shfl_xor_u64((uint64_t)a.mx, m),
             shfl_xor_u64(a.s_lo, m), shfl_xor_u64(a.s_hi, m), shfl_xor_u64(a.q_lo, m), shfl_xor_u64(a.q_hi, m),
             shfl_xor_u64(a.q_top, m)};
}

// Butterfly over the 64 lanes (all active) of two signals: every lane ends with the totals.
// head: the caller's further words, a type with shfl_xor(m) and merge(other), taken through the
// same rounds (every word of a round is fetched from lane ^ m before any is merged).
struct NoHead {
  __device__ __forceinline__ NoHead shfl_xor(int) const { return NoHead{}; }
  __device__ __forceinline__ void merge(const NoHead&) {}
};
template <class Head>
__device__ __forceinline__ void wave_merge2(Sig& a, Sig& b, Head& head) {
#pragma unroll 1
  for (int m = kWave / 2; m > 0; m >>= 1) {
    const Head oh = head.shfl_xor(m);
    const Sig oa = sig_shfl_xor(a, m), ob = sig_shfl_xor(b, m);
    head.merge(oh);
    sig_merge(a, oa);
    sig_merge(b, ob);
  }
}
// its twin over three signals (compare_stats.hip)
template <class Head>
__device__ __forceinline__ void wave_merge3(Sig& a, Sig& b, Sig& c, Head& head) {
#pragma unroll 1
  for (int m = kWave / 2; m > 0; m >>= 1) {
    const Head oh = head.shfl_xor(m);
    const Sig oa = sig_shfl_xor(a, m), ob = sig_shfl_xor(b, m), oc = sig_shfl_xor(c, m);
    head.merge(oh);
    sig_merge(a, oa);
    sig_merge(b, ob);
    sig_merge(c, oc);
  }
}

__device__ __forceinline__ void commit_sig(fognet_moments* m, uint64_t n, uint64_t ovf, const Sig& s) {
  atomic_add(&m->overflow, ovf);
  if (n == 0u) return;
  atomic_add(&m->count, n);
  atomic_min_i64(&m->min_raw, s.mn);
  atomic_max_i64(&m->max_raw, s.mx);
  atomic_add128(&m->sum_lo, &m->sum_hi, s.s_lo, s.s_hi);
  atomic_add192(&m->sq_lo, &m->sq_hi, &m->sq_top, s.q_lo, s.q_hi, s.q_top);
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

// ---------------------------------------------------------------- records
// A record type is described by an Ops: Rec; kHeadWords, the words before its fognet_moments,
// which fill the rest; head_empty(w), the empty record's head word w; merge(a, b), exact.
constexpr int kMomWords = (int)(sizeof(fognet_moments) / sizeof(uint64_t));
static_assert(sizeof(fognet_moments) == 72 && offsetof(fognet_moments, min_raw) == 8 &&
                  offsetof(fognet_moments, max_raw) == 16,
              "empty_word's indices");

template <class Ops>
constexpr int rec_words() {
  static_assert((sizeof(typename Ops::Rec) / 8 - Ops::kHeadWords) % kMomWords == 0, "a head, then fognet_moments");
  return (int)(sizeof(typename Ops::Rec) / sizeof(uint64_t));
}

// word w of the empty record (fognet_hip.h): every min_raw INT64_MAX, max_raw INT64_MIN, the rest 0
template <class Ops>
__device__ __forceinline__ uint64_t empty_word(int w) {
  if (w < Ops::kHeadWords) return Ops::head_empty(w);
  const int f = (w - Ops::kHeadWords) % kMomWords;
  return f == 1 ? (uint64_t)INT64_MAX : f == 2 ? (uint64_t)INT64_MIN : 0u;
}

// the empty record as a value: its words are compile-time constants, copied whole
template <class Ops>
__device__ __forceinline__ typename Ops::Rec empty_record() {
  uint64_t w[rec_words<Ops>()];
#pragma unroll
  for (int i = 0; i < rec_words<Ops>(); ++i) w[i] = empty_word<Ops>(i);
  typename Ops::Rec rec;
  __builtin_memcpy(&rec, w, sizeof rec);
  return rec;
}

// A pass keyed by node or user keeps one record per key: in LDS (kLds, at s_mem, copied to the
// caller's row at the end) or in the caller's row itself.  keyed_begin sets them to the empty
// record and says whether the replication is read at all: of a failed one the caller's row gets
// the empty records and the workgroup returns.  The caller then fills its own LDS, calls
// keyed_ready, accumulates with atomics, and ends with keyed_end.
template <class Ops, bool kLds>
__device__ __forceinline__ bool keyed_begin(const ReplayArgs& A, int r, typename Ops::Rec* row, int keys,
                                            uint64_t* s_mem) {
  const bool ok = rep_ok(A, r);
  uint64_t* const acc_w = !kLds || !ok ? reinterpret_cast<uint64_t*>(row) : s_mem;
  const size_t words = (size_t)keys * rec_words<Ops>();
  for (size_t w = threadIdx.x; w < words; w += kPassThreads) acc_w[w] = empty_word<Ops>((int)(w % rec_words<Ops>()));
  return ok;
}

template <bool kLds>
__device__ __forceinline__ void keyed_ready() {
  if (!kLds) __threadfence();  // the empty records are in memory before any atomic update of them
  __syncthreads();
}

// (kLds: the copy-out, behind a barrier of its own; the caller's rows need nothing more)
template <class Ops, bool kLds>
__device__ __forceinline__ void keyed_end(typename Ops::Rec* row, int keys, const uint64_t* s_mem) {
  if (!kLds) return;
  __syncthreads();
  uint64_t* const dst = reinterpret_cast<uint64_t*>(row);
  const size_t words = (size_t)keys * rec_words<Ops>();
  for (size_t w = threadIdx.x; w < words; w += kPassThreads) dst[w] = s_mem[w];
}

// Job reduction: workgroup j merges column j of the [R][K] records of the replications that
// ran to their end; its threads stride over the replications, then a tree in LDS.  An Ops with
// included(rec) names its own records instead (a record that carries the statuses it depends on:
// no stats array is read).
constexpr int kReduceThreads = 128;

template <class Ops, class = void>
struct ops_names_included : std::false_type {};
template <class Ops>
struct ops_names_included<Ops, std::void_t<decltype(&Ops::included)>> : std::true_type {};

template <class Ops>
__global__ __launch_bounds__(kReduceThreads) void record_reduce_kernel(const typename Ops::Rec* in,
                                                                const fognet_rep_stats* stats, int32_t R, int32_t K,
                                                                typename Ops::Rec* out) {
  using Rec = typename Ops::Rec;
  __shared__ Rec sh[kReduceThreads];
  const int j = blockIdx.x;
  Rec a = empty_record<Ops>();
  for (int r = threadIdx.x; r < R; r += kReduceThreads) {
    const Rec& x = in[(size_t)r * (size_t)K + (size_t)j];
    if constexpr (ops_names_included<Ops>::value) {
      if (Ops::included(x)) Ops::merge(a, x);
    } else {
      if (stats[r].status == FOGNET_OK) Ops::merge(a, x);
    }
  }
  sh[threadIdx.x] = a;
  __syncthreads();
  for (int w = kReduceThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) Ops::merge(sh[threadIdx.x], sh[threadIdx.x + w]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[j] = sh[0];
}

template <class Ops>
inline hipError_t launch_reduce(const typename Ops::Rec* in, const fognet_rep_stats* stats, int32_t R, int32_t K,
                                typename Ops::Rec* out, hipStream_t s) {
  if (K <= 0) return hipSuccess;
  hipLaunchKernelGGL(record_reduce_kernel<Ops>, dim3(K), dim3(kReduceThreads), 0, s, in, stats, R, K, out);
  return hipGetLastError();
}

}  // namespace fognet
