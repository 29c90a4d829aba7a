// node_stats.hip — per-node statistics of a finished replay (fognet_node_stats_dev) and
// their job reduction (fognet_reduce_node_stats_dev): what the reference records per
// ComputeBroker module (queueTime, ComputeBrokerApp3.ned:45-46) plus the node's task
// counts, service seconds and responses.
//
// The pass is a reduction keyed by node over the replay's per-task arrays (33 B per
// task; 34 under EXT_HIER, whose escalated tasks are enqueued a hop later).  One
// workgroup per replication streams them coalesced, 64 tasks per wavefront and
// step.  The accumulators are one fognet_node_stats per node: in LDS up to
// kNodeLdsMax nodes (copied to the caller's records at the end), above that the caller's
// records themselves, set to the empty record first.  Every update is an integer atomic:
// sums take their carries from the value the atomic add returns, extrema are integer
// min/max, so the records do not depend on the order of the updates.
//
// Under REF_V3 the stale view herds most of a 64-task step onto one node (DESIGN.md
// §3.4): per-task atomics on one record would serialise.  Each wavefront therefore
// groups its 64 tasks by node (leader's node, ballot); a group of kGroupReduce tasks or
// more is summed in registers across the wave and committed once by its leader, the
// tasks of smaller groups commit themselves (at most kGroupReduce - 1 updates meet on
// one record, and a step has at most 64 / kGroupReduce summed groups).
#include "stats_atomics.h"

namespace fognet {

namespace {

constexpr int kNodeThreads = 256;  // 160 VGPRs: three workgroups (and their LDS) per CU
constexpr int kNodeWaves = kNodeThreads / kWave;
constexpr int kNodeLdsMax = 256;  // 192 B of record + 16 B of parameters per node: 52 KiB
constexpr int kGroupReduce = 8;
constexpr int kRecWords = (int)(sizeof(fognet_node_stats) / sizeof(uint64_t));
static_assert(sizeof(fognet_node_stats) == 192 && kRecWords == 24, "fognet_node_stats is 24 words");

// word w of the empty record (fognet_hip.h): the maxima (last_tick, queue.max_raw,
// resp.max_raw) INT64_MIN, the minima INT64_MAX, everything else 0
__device__ __forceinline__ uint64_t empty_word(int w) {
  return (w == 5 || w == 8 || w == 17) ? (uint64_t)INT64_MIN : (w == 7 || w == 16) ? (uint64_t)INT64_MAX : 0u;
}
static_assert(offsetof(fognet_node_stats, last_tick) == 5 * 8 && offsetof(fognet_node_stats, queue.min_raw) == 7 * 8 &&
                  offsetof(fognet_node_stats, queue.max_raw) == 8 * 8 &&
                  offsetof(fognet_node_stats, resp.min_raw) == 16 * 8 &&
                  offsetof(fognet_node_stats, resp.max_raw) == 17 * 8,
              "empty_word's indices");

// The contribution of one task, or of a group of at most 64: the seven counts
// (each <= 64) share one word, a byte each.
struct Part {
  uint64_t cnt;  // bytes: tasks, queued, started, lost, queue.count, queue.overflow, resp.count
  uint64_t busy;
  int64_t last, qmin, qmax, rmin, rmax;
  uint64_t qs_lo, qs_hi, qq_lo, qq_hi, qq_top, rs_lo, rs_hi, rq_lo, rq_hi, rq_top;
};
enum { kCTasks = 0, kCQueued = 8, kCStarted = 16, kCLost = 24, kCQn = 32, kCQovf = 40, kCRn = 48 };

__device__ __forceinline__ Part part_identity() {
  Part p = {};
  p.qmin = p.rmin = INT64_MAX;
  p.last = p.qmax = p.rmax = INT64_MIN;
  return p;
}

__device__ __forceinline__ void part_merge(Part& a, const Part& b) {
  a.cnt += b.cnt;
  a.busy += b.busy;
  a.last = max(a.last, b.last);
  a.qmin = min(a.qmin, b.qmin);
  a.qmax = max(a.qmax, b.qmax);
  a.rmin = min(a.rmin, b.rmin);
  a.rmax = max(a.rmax, b.rmax);
  add128(a.qs_lo, a.qs_hi, b.qs_lo, b.qs_hi);
  add192(a.qq_lo, a.qq_hi, a.qq_top, b.qq_lo, b.qq_hi, b.qq_top);
  add128(a.rs_lo, a.rs_hi, b.rs_lo, b.rs_hi);
  add192(a.rq_lo, a.rq_hi, a.rq_top, b.rq_lo, b.rq_hi, b.rq_top);
}

// Butterfly over the 64 lanes (all active): every lane ends with the total.
__device__ __forceinline__ Part wave_merge(Part a) {
#pragma unroll 1
  for (int m = kWave / 2; m > 0; m >>= 1) {
    Part b;
    b.cnt = shfl_xor_u64(a.cnt, m);
    b.busy = shfl_xor_u64(a.busy, m);
    b.last = (int64_t)shfl_xor_u64((uint64_t)a.last, m);
    b.qmin = (int64_t)shfl_xor_u64((uint64_t)a.qmin, m);
    b.qmax = (int64_t)shfl_xor_u64((uint64_t)a.qmax, m);
    b.rmin = (int64_t)shfl_xor_u64((uint64_t)a.rmin, m);
    b.rmax = (int64_t)shfl_xor_u64((uint64_t)a.rmax, m);
    b.qs_lo = shfl_xor_u64(a.qs_lo, m);
    b.qs_hi = shfl_xor_u64(a.qs_hi, m);
    b.qq_lo = shfl_xor_u64(a.qq_lo, m);
    b.qq_hi = shfl_xor_u64(a.qq_hi, m);
    b.qq_top = shfl_xor_u64(a.qq_top, m);
    b.rs_lo = shfl_xor_u64(a.rs_lo, m);
    b.rs_hi = shfl_xor_u64(a.rs_hi, m);
    b.rq_lo = shfl_xor_u64(a.rq_lo, m);
    b.rq_hi = shfl_xor_u64(a.rq_hi, m);
    b.rq_top = shfl_xor_u64(a.rq_top, m);
    part_merge(a, b);
  }
  return a;
}

// ---------------------------------------------------------------- atomic commit (stats_atomics.h)
__device__ __forceinline__ void commit(fognet_node_stats* d, const Part& p) {
  atomic_add(&d->n_tasks, (p.cnt >> kCTasks) & 0xFFu);
  atomic_add(&d->n_queued, (p.cnt >> kCQueued) & 0xFFu);
  atomic_add(&d->n_started, (p.cnt >> kCStarted) & 0xFFu);
  atomic_add(&d->n_lost, (p.cnt >> kCLost) & 0xFFu);
  atomic_add(&d->busy_s, p.busy);
  const uint64_t rn = (p.cnt >> kCRn) & 0xFFu;
  if (rn != 0u) atomic_max_i64(&d->last_tick, p.last);
  commit_moments(&d->queue, (p.cnt >> kCQn) & 0xFFu, (p.cnt >> kCQovf) & 0xFFu, p.qmin, p.qmax, p.qs_lo, p.qs_hi,
                 p.qq_lo, p.qq_hi, p.qq_top);
  commit_moments(&d->resp, rn, 0u, p.rmin, p.rmax, p.rs_lo, p.rs_hi, p.rq_lo, p.rq_hi, p.rq_top);
}

// ---------------------------------------------------------------- the pass
struct TaskRow {
  int64_t t, start, done;
  int32_t req, node;
  uint32_t status;
  uint32_t esc;  // EXT_HIER: the parent took the decision (the task reached its node a hop later)
};

// (A.out_esc: the replay's escalation flags, passed by capi.hip under EXT_HIER only)
__device__ __forceinline__ TaskRow load_task(const ReplayArgs& A, size_t o) {
  return TaskRow{A.arrive[o], A.out_start[o], A.out_done[o], A.req[o], A.out_node[o], (uint32_t)A.out_status[o],
                 A.out_esc ? (uint32_t)A.out_esc[o] : 0u};
}

// kLds: the accumulators, the nodes' downlinks and their MIPS dividers live in LDS
template <bool kLds>
__global__ __launch_bounds__(kNodeThreads) void node_stats_kernel(ReplayArgs A, fognet_node_stats* out) {
  extern __shared__ uint64_t s_mem[];  // kLds: [N] records, [N] dl, [N] UDiv
  const int r = blockIdx.x;
  const int N = A.N;
  const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x / kWave;
  fognet_node_stats* const row = out + (size_t)r * (size_t)N;
  fognet_node_stats* const acc = kLds ? reinterpret_cast<fognet_node_stats*>(s_mem) : row;
  int64_t* const s_dl = reinterpret_cast<int64_t*>(s_mem + (size_t)N * kRecWords);
  UDiv* const s_div = reinterpret_cast<UDiv*>(s_mem + (size_t)N * (kRecWords + 1));
  const int32_t rep_status = A.out_stats[r].status;
  const bool ok = rep_status == FOGNET_OK || rep_status == FOGNET_REF_ABORTED;
  // a failed replication: N empty records, nothing of its rows is read
  const bool direct = !kLds || !ok;
  uint64_t* const acc_w = direct ? reinterpret_cast<uint64_t*>(row) : s_mem;
  const size_t words = (size_t)N * kRecWords;
  for (size_t w = threadIdx.x; w < words; w += kNodeThreads) acc_w[w] = empty_word((int)(w % kRecWords));
  if (!ok) return;
  const size_t nbase = (size_t)r * (size_t)A.node_stride;
  if (kLds) {
    for (int j = threadIdx.x; j < N; j += kNodeThreads) {
      s_dl[j] = A.dl[nbase + j];
      s_div[j] = udiv_magic((uint32_t)A.mips[nbase + j]);
    }
  } else {
    __threadfence();  // the empty records are in memory before any atomic update of them
  }
  __syncthreads();
  const size_t tbase = (size_t)r * (size_t)A.T;
  int64_t n64 = A.out_stats[r].n_tasks;  // decided tasks (written by the replay)
  const int n = (int)(n64 < 0 ? 0 : n64 > A.T ? A.T : n64);
  const int chunks = (n + kWave - 1) / kWave;
  // lanes past n reload the chunk's first task (in bounds, unused)
  auto offset_of = [&](int c) { return tbase + (size_t)(c * kWave + lane < n ? c * kWave + lane : c * kWave); };
  TaskRow cur{};
  if (wave < chunks) cur = load_task(A, offset_of(wave));
  for (int c = wave; c < chunks; c += kNodeWaves) {
    TaskRow nxt = cur;  // the next chunk's loads are in flight while this one is accumulated
    if (c + kNodeWaves < chunks) nxt = load_task(A, offset_of(c + kNodeWaves));
    const uint32_t k = (uint32_t)cur.node;
    const bool valid = c * kWave + lane < n && k < (uint32_t)N;
    Part p = part_identity();
    if (valid) {
      const int64_t dl_k = kLds ? s_dl[k] : A.dl[nbase + k];
      p.cnt = (uint64_t)1 << kCTasks;
      if (cur.status == 4u) p.cnt += (uint64_t)1 << kCQueued;
      if (cur.status == 5u) p.cnt += (uint64_t)1 << kCStarted;
      if (cur.status == 9u) p.cnt += (uint64_t)1 << kCLost;
      if (cur.done >= 0) {  // completed
        const uint32_t mips_k = kLds ? 0u : (uint32_t)A.mips[nbase + k];
        p.busy = kLds ? udiv((uint32_t)cur.req, s_div[k]) : (mips_k ? (uint32_t)cur.req / mips_k : 0u);
        p.last = cur.done;
        const int64_t resp = cur.done - cur.t;
        p.cnt += (uint64_t)1 << kCRn;
        p.rmin = p.rmax = resp;
        add_moment_signed(p.rs_lo, p.rs_hi, p.rq_lo, p.rq_hi, p.rq_top, resp);
      }
      if (cur.status == 4u && cur.start >= 0) {  // queueTime emission (ComputeBrokerApp3.cc:238)
        int64_t raw;
        if (qtime_raw(cur.start, cur.t + dl_k + (cur.esc ? A.hier_up : 0), raw)) {
          p.cnt += (uint64_t)1 << kCQn;
          p.qmin = p.qmax = raw;
          add_moment_signed(p.qs_lo, p.qs_hi, p.qq_lo, p.qq_hi, p.qq_top, raw);
        } else {
          p.cnt += (uint64_t)1 << kCQovf;
        }
      }
    }
    // group the wave's tasks by node
    bool self = false;  // this lane's task commits itself
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
    cur = nxt;
  }
  if (kLds) {
    __syncthreads();
    uint64_t* const dst = reinterpret_cast<uint64_t*>(row);
    for (size_t w = threadIdx.x; w < words; w += kNodeThreads) dst[w] = s_mem[w];
  }
}

// ---------------------------------------------------------------- job reduction
constexpr int kNodeReduceThreads = 128;

__device__ __forceinline__ void node_merge(fognet_node_stats& a, const fognet_node_stats& b) {
  a.n_tasks += b.n_tasks;
  a.n_queued += b.n_queued;
  a.n_started += b.n_started;
  a.n_lost += b.n_lost;
  a.busy_s += b.busy_s;
  a.last_tick = max(a.last_tick, b.last_tick);
  moments_merge(a.queue, b.queue);
  moments_merge(a.resp, b.resp);
}

__device__ __forceinline__ fognet_node_stats node_empty() {
  fognet_node_stats s = {};
  s.last_tick = s.queue.max_raw = s.resp.max_raw = INT64_MIN;
  s.queue.min_raw = s.resp.min_raw = INT64_MAX;
  return s;
}

// Workgroup j merges column j of the [R][N] records: its threads stride over the
// replications, then a tree in LDS.
__global__ __launch_bounds__(kNodeReduceThreads) void node_reduce_kernel(const fognet_node_stats* in,
                                                                         const fognet_rep_stats* stats, int32_t R,
                                                                         int32_t N, fognet_node_stats* out) {
  __shared__ fognet_node_stats sh[kNodeReduceThreads];
  const int j = blockIdx.x;
  fognet_node_stats a = node_empty();
  for (int r = threadIdx.x; r < R; r += kNodeReduceThreads)
    if (stats[r].status == FOGNET_OK) node_merge(a, in[(size_t)r * (size_t)N + (size_t)j]);
  sh[threadIdx.x] = a;
  __syncthreads();
  for (int w = kNodeReduceThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) node_merge(sh[threadIdx.x], sh[threadIdx.x + w]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[j] = sh[0];
}

}  // namespace

int32_t node_stats_lds_max() { return kNodeLdsMax; }

hipError_t launch_node_stats(const ReplayArgs& a, fognet_node_stats* out, bool force_hbm, hipStream_t s) {
  if (a.R <= 0 || a.N <= 0) return hipSuccess;
  if (a.N <= kNodeLdsMax && !force_hbm) {
    const size_t lds = (size_t)a.N * (kRecWords + 2) * sizeof(uint64_t);
    hipLaunchKernelGGL(node_stats_kernel<true>, dim3(a.R), dim3(kNodeThreads), lds, s, a, out);
  } else {
    hipLaunchKernelGGL(node_stats_kernel<false>, dim3(a.R), dim3(kNodeThreads), 0, s, a, out);
  }
  return hipGetLastError();
}

hipError_t launch_reduce_node_stats(const fognet_node_stats* in, const fognet_rep_stats* stats, int32_t R, int32_t N,
                                    fognet_node_stats* out, hipStream_t s) {
  if (N <= 0) return hipSuccess;
  hipLaunchKernelGGL(node_reduce_kernel, dim3(N), dim3(kNodeReduceThreads), 0, s, in, stats, R, N, out);
  return hipGetLastError();
}

}  // namespace fognet
