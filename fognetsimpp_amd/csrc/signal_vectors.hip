// signal_vectors.hip — the recorded signals of a finished replay as ordered vectors
// (fognet_signal_vectors_dev): what the reference records with `vector` per fog node
// (queueTime, ComputeBrokerApp3.ned:45-46), at the broker (delay, BrokerBaseApp3.ned:32-33)
// and per user module (latency, latencyH1, taskTime, mqttApp2.ned:49-54).  The rows are the
// emissions node_stats.hip and per_user_stats.hip count: all three take them from signals.h's
// emission rule.  Their order is the one fognet_hip.h states ("Signal vectors").
//
// One CSR per replication over V = N + 1 + 3U vectors, in three kernels on the caller's stream:
//   count  one 256-thread workgroup per replication streams the per-task rows (33 B per task,
//          coalesced, 64 tasks per wavefront and step, the next step's loads in flight) and
//          counts the rows of every vector with integer atomics: in LDS up to kVecLdsMax
//          vectors, above that in the caller's offset row; an exclusive scan turns the counts
//          into offsets;
//   place  the same stream again; every emission takes the next slot of its vector's segment
//          from an atomic cursor (LDS up to kVecLdsMax vectors, else the workspace), so the
//          position within the segment is arbitrary at this point (but for the broker's delay
//          vector of a replication without unassigned publishes: row i is task i's, placed at i);
//   order  one workgroup per (replication, vector) sorts its segment with a bitonic network: a
//          segment of up to kVecSortLdsMax rows in LDS; a longer one in chunks of that many rows,
//          the network's steps inside a chunk in LDS and its wider steps over the segment in HBM.
// A row is (time, value, task).  The tie words of the order (the tick the node sent the ack and
// the tick its sending event was inserted) are not stored: where two rows of a user vector have
// the same time, and only there, they are recomputed from the two tasks' per-task outputs.  The
// one thing a row cannot say of itself is whether a latencyH1 row is the broker's own pubAck or
// the node's "task queued" ack (both can carry the same time, value and task): between place and
// order, bit 31 of such a row's task marks the relayed ack; the order kernel clears it.
//
// The network is the all-ascending form (a flip step, then half-cleaners): a compare-exchange
// only ever moves the smaller row to the lower index, so the positions past the segment's end
// act as +infinity without being stored or touched, and any segment length sorts in place.
// The key is total apart from rows equal in every word, so the result does not depend on where
// the cursors put the rows.
#include "signals.h"

namespace fognet {

namespace {

constexpr int kVecThreads = kPassThreads;
constexpr int kVecLdsMax = 8192;       // one 32-bit count or cursor per vector: 32 KiB of LDS
constexpr int kVecSortThreads = 1024;  // one compare-exchange per thread and step at kVecSortLdsMax rows
constexpr int kVecSortLdsMax = 2048;   // 20 B per row (time, value, task): 40 KiB of the 64 KiB a workgroup may take
constexpr int kVecSortForcedChunk = 64; // FOGNET_VEC_SORT=hbm: small segments take the HBM steps as well
constexpr uint32_t kRelayedBit = 0x80000000u;

struct VecArgs : UserLinks {
  int32_t r0, Rv, V;
  int64_t cap;             // rows per replication in time / value / task
  int64_t* offset;         // [Rv][V + 1]
  int64_t* time;           // [Rv][cap]
  int64_t* value;          // [Rv][cap]
  int32_t* task;           // [Rv][cap]
  int64_t* n_unassigned;   // [Rv], nullable
  uint32_t* cursor;        // [Rv][V] workspace (V > kVecLdsMax or forced)
  int32_t sort_chunk;      // rows of a segment sorted together in LDS (a power of two, <= kVecSortLdsMax)
};

// The rows of one decided publish, signals.h's emissions with a value in the simtime_t range:
// f(vector, time, value, relayed-ack mark).  A publish of no known user has its queueTime row alone.
template <class F>
__device__ __forceinline__ void for_each_emission(const ReplayArgs& A, const VecArgs& P, size_t nbase, size_t lbase,
                                                  const Row& x, F&& f) {
  const int N = A.N, U = P.U;
  const uint32_t u = (uint32_t)x.user;
  const bool known = u < (uint32_t)U;
  const Emissions e = emissions(
      A, x, [&](int k) { return A.dl[nbase + k]; }, [&](int k) { return A.ul[nbase + k]; },
      known ? P.ul[lbase + u] : 0, known ? P.dl[lbase + u] : 0);
  int64_t raw;
  if (e.queued && qtime_raw(e.queue_start, e.queue_enq, raw)) f(x.node, e.queue_start, raw, 0u);
  if (!known) return;
  f(N, x.t, e.delay, 0u);
  const int v_lat = N + 1 + (int)u, v_h1 = v_lat + U, v_tt = v_h1 + U;
  if (ms_raw(e.puback_d, raw)) f(v_h1, e.puback_at, raw, 0u);
  if (e.first != kAckNone && ms_raw(e.first_d, raw))
    f(e.first == kAckLatency ? v_lat : v_h1, e.first_at, raw, e.first == kAckLatency ? 0u : kRelayedBit);
  if (e.completed && ms_raw(e.done_d, raw)) f(v_tt, e.done_at, raw, 0u);
}

// the per-task columns of the count and place kernels (33 B per task; never the escalation flags)
__device__ __forceinline__ Row load_vec_row(const ReplayArgs& A, const VecArgs& P, size_t o) {
  return load_row<kColStart | kColUser>(A, P.user_of, o);
}

// a count the workgroup's atomics left in the caller's row (read where the atomics were performed)
__device__ __forceinline__ int64_t load_count(const int64_t* p) {
  return (int64_t)__hip_atomic_load((const unsigned long long*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------- count
// kLds: the counts live in LDS; else in the caller's offset row, scanned in place
template <bool kLds>
__global__ __launch_bounds__(kVecThreads) void vec_count_kernel(ReplayArgs A, VecArgs P) {
  extern __shared__ uint32_t s_cnt[];  // kLds: [V]
  __shared__ int64_t s_part[kVecThreads];
  __shared__ unsigned long long s_unassigned;
  const int q = blockIdx.x, r = P.r0 + q, V = P.V;
  int64_t* const off = P.offset + (size_t)q * ((size_t)V + 1);
  if (!rep_ok(A, r)) {  // a failed replication: all-zero offsets, nothing of its rows is read
    for (int v = threadIdx.x; v <= V; v += kVecThreads) off[v] = 0;
    if (threadIdx.x == 0 && P.n_unassigned) P.n_unassigned[q] = 0;
    return;
  }
  if (threadIdx.x == 0) s_unassigned = 0u;
  if (kLds) {
    for (int v = threadIdx.x; v < V; v += kVecThreads) s_cnt[v] = 0u;
  } else {
    for (int v = threadIdx.x; v < V; v += kVecThreads) off[v] = 0;
    __threadfence();  // the zeroes are in memory before any atomic update of them
  }
  __syncthreads();
  const size_t nbase = (size_t)r * (size_t)A.node_stride, lbase = (size_t)r * (size_t)P.link_stride;
  uint32_t unassigned = 0u;  // per wavefront (uniform)
  auto load = [&](size_t o) { return load_vec_row(A, P, o); };
  stream_rows(A, r, decided_tasks(A, r), load, [&](const Row& x, int, bool decided) {
    unassigned += (uint32_t)__popcll(ballot(decided && (uint32_t)x.user >= (uint32_t)P.U));
    if (!decided) return;
    for_each_emission(A, P, nbase, lbase, x, [&](int v, int64_t, int64_t, uint32_t) {
      if (kLds)
        (void)atomicAdd(&s_cnt[v], 1u);
      else
        (void)atomicAdd((unsigned long long*)&off[v], 1ull);
    });
  });
  if (((int)threadIdx.x & (kWave - 1)) == 0 && unassigned != 0u)
    (void)atomicAdd(&s_unassigned, (unsigned long long)unassigned);
  __syncthreads();
  if (threadIdx.x == 0 && P.n_unassigned) P.n_unassigned[q] = (int64_t)s_unassigned;
  // exclusive scan: every thread owns one run of consecutive vectors
  const int per = (V + kVecThreads - 1) / kVecThreads;
  const int v0 = min((int)threadIdx.x * per, V), v1 = min(v0 + per, V);
  int64_t sum = 0;
  for (int v = v0; v < v1; ++v) sum += kLds ? (int64_t)s_cnt[v] : load_count(&off[v]);
  s_part[threadIdx.x] = sum;
  __syncthreads();  // (and every count is read before any offset is written over it)
  int64_t before = 0, total = 0;
  for (int t = 0; t < kVecThreads; ++t) {
    const int64_t p = s_part[t];
    before += t < (int)threadIdx.x ? p : 0;
    total += p;
  }
  for (int v = v0; v < v1; ++v) {
    const int64_t c = kLds ? (int64_t)s_cnt[v] : load_count(&off[v]);
    off[v] = before;
    before += c;
  }
  if (threadIdx.x == 0) off[V] = total;
}

// ---------------------------------------------------------------- place
// kLds: the cursors live in LDS; else in the workspace (zeroed here: no dependence on what it held)
template <bool kLds>
__global__ __launch_bounds__(kVecThreads) void vec_place_kernel(ReplayArgs A, VecArgs P) {
  extern __shared__ uint32_t s_cur[];  // kLds: [V]
  const int q = blockIdx.x, r = P.r0 + q, V = P.V;
  if (!rep_ok(A, r)) return;
  const int64_t* const off = P.offset + (size_t)q * ((size_t)V + 1);
  uint32_t* const cur = kLds ? s_cur : P.cursor + (size_t)q * (size_t)V;
  for (int v = threadIdx.x; v < V; v += kVecThreads) cur[v] = 0u;
  if (!kLds) __threadfence();
  __syncthreads();
  const size_t nbase = (size_t)r * (size_t)A.node_stride, lbase = (size_t)r * (size_t)P.link_stride;
  const size_t base = (size_t)q * (size_t)P.cap;
  const int n = decided_tasks(A, r);
  // Every decided publish of a known user emits one delay row, and the vector is in task order: where no
  // publish is unassigned, row i is task i's and needs neither a cursor nor the order stage.
  const bool delay_dense = off[A.N + 1] - off[A.N] == (int64_t)n;
  auto load = [&](size_t o) { return load_vec_row(A, P, o); };
  stream_rows(A, r, n, load, [&](const Row& x, int i, bool decided) {
    if (!decided) return;
    for_each_emission(A, P, nbase, lbase, x, [&](int v, int64_t time, int64_t value, uint32_t mark) {
      const int64_t slot = off[v] + (v == A.N && delay_dense ? (int64_t)i : (int64_t)atomicAdd(&cur[v], 1u));
      if (slot >= off[v + 1] || slot >= P.cap) return;  // (never: count and place see the same emissions)
      P.time[base + (size_t)slot] = time;
      P.value[base + (size_t)slot] = value;
      P.task[base + (size_t)slot] = (int32_t)((uint32_t)i | mark);
    });
  });
}

// ---------------------------------------------------------------- order
enum VecKind { kByTask = 0, kLatency = 1, kLatencyH1 = 2, kTaskTime = 3 };

struct SortRow {
  int64_t time, value;
  uint32_t task;  // (latencyH1: bit 31 marks the relayed ack)
};

struct SortCtx {
  const ReplayArgs* A;
  size_t tbase, nbase;
  int kind;
};

// the tie words of a user-vector row: (tick the node sent the ack, tick its sending event was inserted);
// the broker's own pubAck precedes every relayed ack of its tick
__device__ __forceinline__ void tie_words(const SortCtx& c, uint32_t task, int64_t& sent, int64_t& inserted) {
  const ReplayArgs& A = *c.A;
  // (a row's task is one of the replication's T by construction; the clamp keeps the gather in bounds regardless)
  const size_t o = c.tbase + (size_t)min(task & ~kRelayedBit, (uint32_t)A.T - 1u);
  if (c.kind == kTaskTime) {  // the completion ack: sent at done, by the RELEASERESOURCE timer armed at start
    sent = A.out_done[o];
    inserted = A.out_start[o];
  } else if (c.kind == kLatencyH1 && !(task & kRelayedBit)) {
    sent = -1;
    inserted = 0;
  } else {  // the node's first ack: sent at the task's arrival, an event created at the decision
    const int32_t k = A.out_node[o];
    const int64_t t = A.arrive[o];
    sent = t + A.dl[c.nbase + (size_t)link_node(A, k)];
    inserted = t;
  }
}

__device__ __forceinline__ bool row_less(const SortCtx& c, const SortRow& a, const SortRow& b) {
  if (c.kind == kByTask) return a.task < b.task;
  if (a.time != b.time) return a.time < b.time;
  int64_t sa, ia, sb, ib;
  tie_words(c, a.task, sa, ia);
  tie_words(c, b.task, sb, ib);
  if (sa != sb) return sa < sb;
  if (ia != ib) return ia < ib;
  return (a.task & ~kRelayedBit) < (b.task & ~kRelayedBit);
}

// the pair of compare-exchange p in the step of distance j inside blocks of k (flip: the block's first step)
__device__ __forceinline__ void pair_of(uint32_t p, uint32_t k, uint32_t j, uint32_t& lo, uint32_t& hi) {
  const uint32_t blk = p / j, in = p % j;
  lo = blk * 2u * j + in;
  hi = 2u * j == k ? blk * k + (k - 1u - in) : lo + j;
}

// One compare-exchange step (block k, distance j) over the m rows of a chunk in LDS.
__device__ __forceinline__ void lds_step(const SortCtx& c, uint32_t m, uint32_t pairs, uint32_t k, uint32_t j,
                                         int64_t* s_time, int64_t* s_value, uint32_t* s_task) {
  for (uint32_t p = threadIdx.x; p < pairs; p += kVecSortThreads) {
    uint32_t lo, hi;
    pair_of(p, k, j, lo, hi);
    if (hi >= m) continue;  // +infinity stays where it is
    const SortRow a{s_time[lo], s_value[lo], s_task[lo]}, b{s_time[hi], s_value[hi], s_task[hi]};
    if (row_less(c, b, a)) {
      s_time[lo] = b.time, s_value[lo] = b.value, s_task[lo] = b.task;
      s_time[hi] = a.time, s_value[hi] = a.value, s_task[hi] = a.task;
    }
  }
}

// Workgroup (q, v) sorts vector v of replication q.  The segment is cut into chunks of C rows (C a power of
// two, at most kVecSortLdsMax): every step whose pairs lie inside an aligned chunk -- all of them up to block
// size C, and the distances below C of the larger blocks -- runs on the chunk in LDS, one load and one store
// per run of such steps; the steps of distance C and more run over the segment in HBM, where the workgroup's
// barrier orders them.  A segment of up to C rows is one chunk and never leaves LDS.
__global__ __launch_bounds__(kVecSortThreads) void vec_sort_kernel(ReplayArgs A, VecArgs P) {
  __shared__ int64_t s_time[kVecSortLdsMax];
  __shared__ int64_t s_value[kVecSortLdsMax];
  __shared__ uint32_t s_task[kVecSortLdsMax];
  const int V = P.V, N = A.N, U = P.U;
  const int q = (int)(blockIdx.x / (uint32_t)V), v = (int)(blockIdx.x % (uint32_t)V), r = P.r0 + q;
  const int64_t* const off = P.offset + (size_t)q * ((size_t)V + 1);
  const int64_t o0 = off[v];
  const uint32_t n = (uint32_t)(off[v + 1] - o0);
  if (n == 0u) return;
  if (v == N && (int64_t)n == (int64_t)decided_tasks(A, r)) return;  // the dense delay vector was placed in order
  SortCtx c{&A, (size_t)r * (size_t)A.T, (size_t)r * (size_t)A.node_stride,
            v <= N ? kByTask : v < N + 1 + U ? kLatency : v < N + 1 + 2 * U ? kLatencyH1 : kTaskTime};
  int64_t* const g_time = P.time + (size_t)q * (size_t)P.cap + (size_t)o0;
  int64_t* const g_value = P.value + (size_t)q * (size_t)P.cap + (size_t)o0;
  uint32_t* const g_task = reinterpret_cast<uint32_t*>(P.task + (size_t)q * (size_t)P.cap + (size_t)o0);
  uint32_t pow2 = 1u;
  while (pow2 < n) pow2 <<= 1;
  const uint32_t tid = threadIdx.x, C = (uint32_t)P.sort_chunk;
  // the chunks' runs of steps: blocks k_first .. k_last, of each the distances from min(k / 2, C / 2) down
  auto chunks = [&](uint32_t k_first, uint32_t k_last, bool last) {
    for (uint32_t base = 0u; base < n; base += C) {
      const uint32_t m = min(C, n - base);
      for (uint32_t i = tid; i < m; i += kVecSortThreads) {
        s_time[i] = g_time[base + i];
        s_value[i] = g_value[base + i];
        s_task[i] = g_task[base + i];
      }
      for (uint32_t k = k_first; k <= k_last; k <<= 1)
        for (uint32_t j = min(k >> 1, C >> 1); j > 0u; j >>= 1) {
          __syncthreads();
          lds_step(c, m, C >> 1, k, j, s_time, s_value, s_task);
        }
      __syncthreads();
      const uint32_t keep = last ? ~kRelayedBit : ~0u;  // the finished rows carry the task alone
      for (uint32_t i = tid; i < m; i += kVecSortThreads) {
        g_time[base + i] = s_time[i];
        g_value[base + i] = s_value[i];
        g_task[base + i] = s_task[i] & keep;
      }
      __syncthreads();  // the chunk is in memory, and LDS is free, before anything else touches either
    }
  };
  chunks(2u, min(C, pow2), pow2 <= C);
  for (uint32_t k = 2u * C; k <= pow2 && k != 0u; k <<= 1) {
    for (uint32_t j = k >> 1; j >= C; j >>= 1) {  // the wide steps, over the segment in HBM
      for (uint32_t p = tid; p < pow2 / 2u; p += kVecSortThreads) {
        uint32_t lo, hi;
        pair_of(p, k, j, lo, hi);
        if (hi >= n) continue;
        const SortRow a{g_time[lo], 0, g_task[lo]}, b{g_time[hi], 0, g_task[hi]};
        if (row_less(c, b, a)) {
          const int64_t va = g_value[lo], vb = g_value[hi];
          g_time[lo] = b.time, g_value[lo] = vb, g_task[lo] = b.task;
          g_time[hi] = a.time, g_value[hi] = va, g_task[hi] = a.task;
        }
      }
      __syncthreads();
    }
    chunks(k, k, k == pow2);
  }
}

}  // namespace

int32_t signal_vectors_lds_max() { return kVecLdsMax; }
int32_t signal_vectors_sort_lds_max() { return kVecSortLdsMax; }

hipError_t launch_signal_vectors(const ReplayArgs& a, const UserLinks& users, int32_t r0, int32_t Rv,
                                 const fognet_signal_vectors& vec, int64_t* n_unassigned, uint32_t* cursor,
                                 bool force_hbm, int stages, hipStream_t s) {
  if (Rv <= 0) return hipSuccess;
  const int32_t V = a.N + 1 + 3 * users.U;
  const VecArgs p{users, r0, Rv, V, vec.cap, vec.offset, vec.time, vec.value, vec.task, n_unassigned, cursor,
                  force_hbm ? kVecSortForcedChunk : kVecSortLdsMax};
  const bool lds = V <= kVecLdsMax && !force_hbm;
  const size_t lds_bytes = lds ? (size_t)V * sizeof(uint32_t) : 0;
  if (lds)
    hipLaunchKernelGGL(vec_count_kernel<true>, dim3(Rv), dim3(kVecThreads), lds_bytes, s, a, p);
  else
    hipLaunchKernelGGL(vec_count_kernel<false>, dim3(Rv), dim3(kVecThreads), 0, s, a, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || stages < 2 || a.T <= 0) return e;
  if (lds)
    hipLaunchKernelGGL(vec_place_kernel<true>, dim3(Rv), dim3(kVecThreads), lds_bytes, s, a, p);
  else
    hipLaunchKernelGGL(vec_place_kernel<false>, dim3(Rv), dim3(kVecThreads), 0, s, a, p);
  e = hipGetLastError();
  if (e != hipSuccess || stages < 3) return e;
  hipLaunchKernelGGL(vec_sort_kernel, dim3((uint32_t)((size_t)Rv * (size_t)V)), dim3(kVecSortThreads), 0, s, a, p);
  return hipGetLastError();
}

}  // namespace fognet
