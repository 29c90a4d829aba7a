// queue_stats.hip — queue-length statistics of a finished replay (fognet_queue_stats_dev) and
// their job reduction (fognet_reduce_queue_stats_dev): per fog node the longest `requests`
// vector (ComputeBrokerApp3.cc:309 push_back, :246 erase), its time integral and the time it
// held each of up to FOGNET_QUEUE_LEVELS_MAX lengths or more, over a caller's range of sim time.
// fognet_hip.h "Queue-length statistics" states the model once.
//
// No event is sorted.  A node's queued tasks (status 4) are FIFO in trace order, because at_node =
// arrive + dl_k is nondecreasing along a node's tasks, so with element j of a node (0-based) holding
//   at_j     the tick it was enqueued,
//   leave_j  the tick it was dequeued (its start_tick; down_tick of a node that crashed first),
//   prev_j   the start_tick of the task served just before it, whose completion dequeued it,
// every quantity is a closed form of one element and its neighbours:
//   D_j   the dequeues before enqueue j = #{l < j : (leave_l, prev_l) < (at_j, t_j)}, t_j = at_j -
//         dl_k (the same-tick rule: the enqueue comes first iff t_j <= prev_l); both keys are
//         nondecreasing in l, so D_j is one binary search over [0, j);
//   L right after enqueue j = j + 1 - D_j;
//   L >= k between at_j and at_{j+1} exactly while element j + 1 - k has not left;
//   the area is the sum of the elements' [at_j, leave_j).
//
// Three launches on the caller's stream:
//   count    one workgroup per replication counts the queued tasks of every node with integer
//            atomics (LDS up to kCountLdsMax nodes, else the workspace row) and scans the counts
//            into offsets: one CSR per replication.  A failed replication gets zero offsets and
//            none of its rows is read.
//   build    one wavefront per replication walks the trace in tiles of 64 tasks, as
//            replay_assigned.hip's chain kernel does: the lanes of one node come from one ballot
//            per bit of the node index, a task's stable rank from the node's cursor plus the
//            queued lanes before it, prev from the nearest earlier lane of the node or the node's
//            carried last start.  The carries (12 B per node) live in LDS up to kBuildLdsMax
//            nodes, else in the workspace.
//   measure  one workgroup per replication, one thread per element; the records are committed per
//            node with signals.h's keyed frame and node_stats.hip's group-by-node wave summing (a
//            node's elements are contiguous, so most of a wavefront shares a node).  Records live
//            in LDS up to kNodeLdsMax nodes, above that in the caller's rows.
// Every update is one of signals.h's integer atomics, so a record does not depend on their order.
#include "signals.h"

namespace fognet {

namespace {

constexpr int kCountLdsMax = 8192;  // one 32-bit count per node: 32 KiB
constexpr int kBuildLdsMax = 2048;  // 12 B of carry per node: 24 KiB per wavefront
constexpr int kNodeLdsMax = 256;    // 176 B of record per node: 44 KiB
constexpr int kGroupReduce = 8;
constexpr int kLevels = FOGNET_QUEUE_LEVELS_MAX;

// fognet_queue_stats as signals.h takes a record: all head words, the empty record all zero
struct QueueOps {
  using Rec = fognet_queue_stats;
  static constexpr int kHeadWords = (int)(sizeof(fognet_queue_stats) / sizeof(uint64_t));
  static __device__ __forceinline__ uint64_t head_empty(int) { return 0u; }
  static __device__ __forceinline__ void merge(Rec& a, const Rec& b) {
    a.n_enq += b.n_enq;
    a.max_len = max(a.max_len, b.max_len);
    add128(a.observed_lo, a.observed_hi, b.observed_lo, b.observed_hi);
    add128(a.area_lo, a.area_hi, b.area_lo, b.area_hi);
#pragma unroll
    for (int q = 0; q < kLevels; ++q) add128(a.time_ge[q][0], a.time_ge[q][1], b.time_ge[q][0], b.time_ge[q][1]);
  }
};
constexpr int kRecWords = rec_words<QueueOps>();
static_assert(sizeof(fognet_queue_stats) == 176 && kRecWords == 22, "fognet_queue_stats is 22 words");
static_assert(offsetof(fognet_queue_stats, max_len) == 8 && offsetof(fognet_queue_stats, observed_lo) == 16 &&
                  offsetof(fognet_queue_stats, area_lo) == 32 && offsetof(fognet_queue_stats, time_ge) == 48,
              "the record's layout (fognet_hip.h)");

struct QueueArgs {
  QueueWs w;
  int64_t t0, t1;          // the observed range [t0, t1)
  int64_t level[kLevels];  // strictly ascending, >= 1; level[q >= Q] unused
  int32_t Q;
  int32_t carry_hbm;       // the build kernel's carries live in the workspace (the count kernel initialises them)
};

__device__ __forceinline__ uint32_t shfl_u32(uint32_t v, int src) { return (uint32_t)__shfl((int)v, src, kWave); }
__device__ __forceinline__ int64_t shfl_i64(int64_t v, int src) {
  const uint32_t lo = shfl_u32((uint32_t)(uint64_t)v, src), hi = shfl_u32((uint32_t)((uint64_t)v >> 32), src);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// ---------------------------------------------------------------- count
// kLds: the counts live in LDS; else in the replication's offset row, scanned in place
template <bool kLds>
__global__ __launch_bounds__(kPassThreads) void queue_count_kernel(ReplayArgs A, QueueArgs P) {
  extern __shared__ uint32_t s_cnt[];  // kLds: [N]
  __shared__ uint32_t s_part[kPassThreads];
  const int r = blockIdx.x, N = A.N, tid = threadIdx.x;
  uint32_t* const off = P.w.off + (size_t)r * ((size_t)N + 1);
  if (!rep_ok(A, r)) {  // no element: the other two kernels have nothing to walk
    for (int v = tid; v <= N; v += kPassThreads) off[v] = 0u;
    return;
  }
  const int n = decided_tasks(A, r);
  const size_t tbase = (size_t)r * (size_t)A.T;
  for (int v = tid; v < N; v += kPassThreads) {
    if (kLds)
      s_cnt[v] = 0u;
    else
      off[v] = 0u;
    if (P.carry_hbm) {
      const size_t c = (size_t)r * (size_t)N + (size_t)v;
      P.w.c_start[c] = -1;
      P.w.c_rank[c] = 0u;
    }
  }
  if (!kLds) __threadfence();  // the zeroes are in memory before any atomic update of them
  __syncthreads();
  for (int i = tid; i < n; i += kPassThreads) {
    const uint32_t k = (uint32_t)A.out_node[tbase + i];
    if (A.out_status[tbase + i] == 4u && k < (uint32_t)N) {
      if (kLds)
        (void)atomicAdd(&s_cnt[k], 1u);
      else
        (void)atomicAdd(&off[k], 1u);
    }
  }
  __syncthreads();
  // exclusive scan: every thread owns one run of consecutive nodes (assigned_count_kernel's)
  auto count_of = [&](int v) -> uint32_t {
    return kLds ? s_cnt[v] : __hip_atomic_load(&off[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  const int per = (N + kPassThreads - 1) / kPassThreads;
  const int v0 = min(tid * per, N), v1 = min(v0 + per, N);
  uint32_t sum = 0u;
  for (int v = v0; v < v1; ++v) sum += count_of(v);
  s_part[tid] = sum;
  __syncthreads();  // (and every count is read before any offset is written over it)
  uint32_t before = 0u, total = 0u;
  for (int t = 0; t < kPassThreads; ++t) {
    const uint32_t p = s_part[t];
    before += t < tid ? p : 0u;
    total += p;
  }
  for (int v = v0; v < v1; ++v) {
    const uint32_t c = count_of(v);
    off[v] = before;
    before += c;
  }
  if (tid == 0) off[N] = total;
}

// ---------------------------------------------------------------- build
// kLds: the nodes' carries live in LDS; else in the workspace
template <bool kLds>
__global__ __launch_bounds__(kWave) void queue_build_kernel(ReplayArgs A, QueueArgs P) {
  extern __shared__ __align__(8) unsigned char s_dyn[];  // kLds: the carries
  const int r = blockIdx.x, lane = threadIdx.x, N = A.N, T = A.T;
  if (!rep_ok(A, r)) return;
  const int n = decided_tasks(A, r);
  const size_t tbase = (size_t)r * (size_t)T, nbase = (size_t)r * (size_t)A.node_stride;
  // what node k carries from tile to tile
  int64_t* c_start;  // start_tick of the last task sent to it (-1: none yet, or that task never started)
  uint32_t* c_rank;  // its queued tasks so far: the next element of its segment
  if constexpr (kLds) {
    c_start = reinterpret_cast<int64_t*>(s_dyn);
    c_rank = reinterpret_cast<uint32_t*>(s_dyn + (size_t)8 * (size_t)N);
    for (int j = lane; j < N; j += kWave) {
      c_start[j] = -1;
      c_rank[j] = 0u;
    }
  } else {
    c_start = P.w.c_start + (size_t)r * (size_t)N;
    c_rank = P.w.c_rank + (size_t)r * (size_t)N;
  }
  __syncthreads();
  const uint32_t* const off = P.w.off + (size_t)r * ((size_t)N + 1);
  int64_t* const e_at = P.w.at + tbase;
  int64_t* const e_leave = P.w.leave + tbase;
  int64_t* const e_prev = P.w.prev + tbase;
  int32_t* const e_node = P.w.node + tbase;
  const int nbits = N > 1 ? 32 - __clz(N - 1) : 0;  // bits of a node index
  const uint64_t lt = ((uint64_t)1 << lane) - 1u;   // the lanes before this one

  for (int c0 = 0; c0 < n; c0 += kWave) {
    const int i = c0 + lane;
    const size_t o = tbase + (size_t)(i < n ? i : c0);  // past the end: reload the tile's first task (in bounds, unused)
    const int64_t t = A.arrive[o], start = A.out_start[o];
    const uint32_t k = (uint32_t)A.out_node[o], status = A.out_status[o];
    const bool in = i < n && k < (uint32_t)N;  // (a decided publish's node lies in [0, N))
    const uint32_t ku = in ? k : 0u;
    const int64_t dl_k = A.dl[nbase + ku];
    const int64_t down_k = A.down ? A.down[nbase + ku] : kNever;
    const uint32_t off_k = off[ku], cr = c_rank[ku];
    const int64_t cs = c_start[ku];

    // the lanes of the same node: all of them (the task served before), and the queued ones (ranks)
    uint64_t m_all = ballot(in);
    for (int b = 0; b < nbits; ++b) {
      const bool bit = (ku >> b) & 1u;
      const uint64_t bb = ballot(in && bit);
      m_all &= bit ? bb : ~bb;
    }
    if (!in) m_all = 0u;
    const bool queued = in && status == 4u;
    const uint64_t m_q = m_all & ballot(queued);
    const uint32_t rank = cr + (uint32_t)__popcll(m_q & lt);
    const uint64_t prevs = m_all & lt;
    const int pred = prevs ? 63 - __clzll((long long)prevs) : -1;  // the task served just before, if in this tile
    const int64_t start_up = shfl_i64(start, pred >= 0 ? pred : lane);
    if (queued) {
      const int64_t at = t + dl_k;
      // (rows of the segment lie inside the replication's T elements; the clamp keeps the stores so regardless)
      const uint32_t row = min(off_k + rank, (uint32_t)(T - 1));
      e_at[row] = at;
      // a queued task that never starts waits until its node crashes (only a crash keeps it from starting)
      e_leave[row] = start >= 0 ? start : (down_k != kNever && down_k > at ? down_k : at);
      e_prev[row] = pred >= 0 ? start_up : cs;
      e_node[row] = (int32_t)ku;
    }
    // the carries, by the node's last lane of the tile
    if (in && (m_all >> lane) == 1u) {
      c_start[ku] = start;
      c_rank[ku] = cr + (uint32_t)__popcll(m_q);
    }
    if (!kLds) __threadfence_block();  // the next tile reads them back
  }
}

// ---------------------------------------------------------------- measure
// the ticks of [a, b) inside [t0, t1)
__device__ __forceinline__ uint64_t clipped(int64_t a, int64_t b, int64_t t0, int64_t t1) {
  const int64_t lo = max(a, t0), hi = min(b, t1);
  return hi > lo ? (uint64_t)(hi - lo) : 0u;
}

// The contribution of one element, or of a group of at most 64 of one node.  The intervals that one
// node's elements add to a level are disjoint, so ge[q] stays below 2^62; the area takes 128 bits.
struct Part {
  uint64_t enq;
  int64_t mx;
  uint64_t area_lo, area_hi;
  uint64_t ge[kLevels];
};

__device__ __forceinline__ Part part_identity() { return Part{0u, 0, 0u, 0u, {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}}; }

// every lane (all active) ends with the wave's total
__device__ __forceinline__ Part wave_merge(Part a) {
#pragma unroll 1
  for (int m = kWave / 2; m > 0; m >>= 1) {
    Part b;
    b.enq = shfl_xor_u64(a.enq, m);
    b.mx = (int64_t)shfl_xor_u64((uint64_t)a.mx, m);
    b.area_lo = shfl_xor_u64(a.area_lo, m);
    b.area_hi = shfl_xor_u64(a.area_hi, m);
#pragma unroll
    for (int q = 0; q < kLevels; ++q) b.ge[q] = shfl_xor_u64(a.ge[q], m);
    a.enq += b.enq;
    a.mx = max(a.mx, b.mx);
    add128(a.area_lo, a.area_hi, b.area_lo, b.area_hi);
#pragma unroll
    for (int q = 0; q < kLevels; ++q) a.ge[q] += b.ge[q];
  }
  return a;
}

__device__ __forceinline__ void commit(fognet_queue_stats* d, const Part& p) {
  atomic_add(&d->n_enq, p.enq);
  if (p.enq != 0u) atomic_max_i64(&d->max_len, p.mx);
  atomic_add128(&d->area_lo, &d->area_hi, p.area_lo, p.area_hi);
#pragma unroll
  for (int q = 0; q < kLevels; ++q) atomic_add128(&d->time_ge[q][0], &d->time_ge[q][1], p.ge[q], 0u);
}

// kLds: the accumulators live in LDS
template <bool kLds>
__global__ __launch_bounds__(kPassThreads) void queue_measure_kernel(ReplayArgs A, QueueArgs P, fognet_queue_stats* out) {
  extern __shared__ uint64_t s_mem[];  // kLds: [N] records
  const int r = blockIdx.x, N = A.N, T = A.T;
  const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x / kWave;
  fognet_queue_stats* const row = out + (size_t)r * (size_t)N;
  fognet_queue_stats* const acc = kLds ? reinterpret_cast<fognet_queue_stats*>(s_mem) : row;
  if (!keyed_begin<QueueOps, kLds>(A, r, row, N, s_mem)) return;
  keyed_ready<kLds>();
  const int64_t t0 = P.t0, t1 = P.t1;
  for (int j = threadIdx.x; j < N; j += kPassThreads) atomic_add(&acc[j].observed_lo, (uint64_t)(t1 - t0));
  const size_t tbase = (size_t)r * (size_t)T, nbase = (size_t)r * (size_t)A.node_stride;
  const uint32_t* const off = P.w.off + (size_t)r * ((size_t)N + 1);
  const int64_t* const e_at = P.w.at + tbase;
  const int64_t* const e_leave = P.w.leave + tbase;
  const int64_t* const e_prev = P.w.prev + tbase;
  const int32_t* const e_node = P.w.node + tbase;
  const uint32_t total = min(off[N], (uint32_t)T);  // (the count kernel's total: at most the decided tasks)
  const uint32_t chunks = (total + kWave - 1) / kWave;
  for (uint32_t c = wave; c < chunks; c += kPassWaves) {
    const uint32_t e = c * kWave + lane;
    bool valid = e < total;
    uint32_t k = 0u;
    Part p = part_identity();
    if (valid) {
      k = min((uint32_t)e_node[e], (uint32_t)(N - 1));
      // the node's segment [s0, s1) holds e (the build kernel placed it by these offsets; checked regardless)
      const uint32_t s0 = off[k], s1 = min(off[k + 1], total);
      valid = s0 <= e && e < s1;
      if (valid) {
        const uint32_t j = e - s0, m = s1 - s0;
        const int64_t at = e_at[e], leave = e_leave[e];
        const int64_t tj = at - A.dl[nbase + k];  // the publish's tick at the broker: when the arrival was inserted
        const int64_t next_at = j + 1u < m ? e_at[e + 1u] : kNever;
        // D_j: the first l in [0, j) whose dequeue does not precede this enqueue
        uint32_t lo = 0u, hi = j;
        while (lo < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          const int64_t lv = e_leave[s0 + mid], pv = e_prev[s0 + mid];
          if (lv < at || (lv == at && pv < tj))
            lo = mid + 1u;
          else
            hi = mid;
        }
        if (t0 <= at && at < t1) {
          p.enq = 1u;
          p.mx = (int64_t)(j + 1u - lo);
        }
        p.area_lo = clipped(at, leave, t0, t1);
#pragma unroll
        for (int q = 0; q < kLevels; ++q) {
          if (q < P.Q && P.level[q] <= (int64_t)j + 1) {
            const uint32_t idx = j + 1u - (uint32_t)P.level[q];  // the element whose leaving ends L >= level
            p.ge[q] = clipped(at, min(next_at, e_leave[s0 + idx]), t0, t1);
          }
        }
      }
    }
    // group the wave's elements by node (node_stats.hip)
    bool self = false;  // this lane's element commits itself
    uint64_t todo = ballot(valid);
    while (todo != 0u) {
      const int leader = __ffsll((long long)todo) - 1;
      const uint32_t k0 = readlane_u32(k, leader);
      const bool mine = valid && k == k0;
      const uint64_t grp = ballot(mine);
      todo &= ~grp;
      if (__popcll(grp) < kGroupReduce) {
        self = self || mine;
      } else {
        const Part g = wave_merge(mine ? p : part_identity());
        if (lane == leader) commit(&acc[k0], g);
      }
    }
    if (self) commit(&acc[k], p);
  }
  keyed_end<QueueOps, kLds>(row, N, s_mem);
}

}  // namespace

int32_t queue_stats_lds_max() { return kNodeLdsMax; }
int32_t queue_stats_build_lds_max() { return kBuildLdsMax; }

hipError_t launch_queue_stats(const ReplayArgs& a, const QueueWs& w, const int64_t* level, int32_t Q, int64_t t0,
                              int64_t t1, fognet_queue_stats* out, bool force_hbm, int stages, hipStream_t s) {
  if (a.R <= 0 || a.N <= 0) return hipSuccess;
  const bool carry_lds = a.N <= kBuildLdsMax && !force_hbm;
  QueueArgs p{};
  p.w = w;
  p.t0 = t0;
  p.t1 = t1;
  p.Q = Q;
  for (int q = 0; q < kLevels; ++q) p.level[q] = q < Q ? level[q] : INT64_MAX;
  p.carry_hbm = carry_lds ? 0 : 1;
  if (a.N <= kCountLdsMax && !force_hbm)
    hipLaunchKernelGGL(queue_count_kernel<true>, dim3(a.R), dim3(kPassThreads), (size_t)a.N * sizeof(uint32_t), s, a, p);
  else
    hipLaunchKernelGGL(queue_count_kernel<false>, dim3(a.R), dim3(kPassThreads), 0, s, a, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (carry_lds)
    hipLaunchKernelGGL(queue_build_kernel<true>, dim3(a.R), dim3(kWave), (size_t)a.N * 12u, s, a, p);
  else
    hipLaunchKernelGGL(queue_build_kernel<false>, dim3(a.R), dim3(kWave), 0, s, a, p);
  e = hipGetLastError();
  if (e != hipSuccess || stages < 2) return e;
  if (a.N <= kNodeLdsMax && !force_hbm)
    hipLaunchKernelGGL(queue_measure_kernel<true>, dim3(a.R), dim3(kPassThreads),
                       (size_t)a.N * kRecWords * sizeof(uint64_t), s, a, p, out);
  else
    hipLaunchKernelGGL(queue_measure_kernel<false>, dim3(a.R), dim3(kPassThreads), 0, s, a, p, out);
  return hipGetLastError();
}

hipError_t launch_reduce_queue_stats(const fognet_queue_stats* in, const fognet_rep_stats* stats, int32_t R, int32_t N,
                                     fognet_queue_stats* out, hipStream_t s) {
  return launch_reduce<QueueOps>(in, stats, R, N, out, s);
}

}  // namespace fognet
