// node_stats.hip — per-node statistics of a finished replay (fognet_node_stats_dev) and
// their job reduction (fognet_reduce_node_stats_dev): what the reference records per
// ComputeBroker module (queueTime, ComputeBrokerApp3.ned:45-46) plus the node's task
// counts, service seconds and responses.
//
// The pass is a reduction keyed by node over the replay's per-task arrays (33 B per
// task; 34 under EXT_HIER, whose escalated tasks are enqueued a hop later), streamed by
// one workgroup per replication (signals.h's stream_rows); when a queueTime is emitted,
// and with which two ticks, is signals.h's emission rule.  The accumulators are one
// fognet_node_stats per node: in LDS up to kNodeLdsMax nodes, above that the caller's
// records themselves (signals.h's keyed frame).  Every update is an integer atomic
// (signals.h), so the records do not depend on the order of the updates.
//
// Under REF_V3 the stale view herds most of a 64-task step onto one node (DESIGN.md
// §3.4): per-task atomics on one record would serialise.  Each wavefront therefore
// groups its 64 tasks by node (leader's node, ballot); a group of kGroupReduce tasks or
// more is summed in registers across the wave and committed once by its leader, the
// tasks of smaller groups commit themselves (at most kGroupReduce - 1 updates meet on
// one record, and a step has at most 64 / kGroupReduce summed groups).
#include "signals.h"

namespace fognet {

namespace {

constexpr int kNodeThreads = kPassThreads;  // 160 VGPRs: three workgroups (and their LDS) per CU
constexpr int kNodeLdsMax = 256;  // 192 B of record + 16 B of parameters per node: 52 KiB
constexpr int kGroupReduce = 8;

// fognet_node_stats as signals.h takes a record: four counts, busy_s and last_tick, then queue and resp
struct NodeOps {
  using Rec = fognet_node_stats;
  static constexpr int kHeadWords = 6;
  static __device__ __forceinline__ uint64_t head_empty(int w) { return w == 5 ? (uint64_t)INT64_MIN : 0u; }  // last_tick
  static __device__ __forceinline__ void merge(Rec& a, const Rec& b) {
    a.n_tasks += b.n_tasks;
    a.n_queued += b.n_queued;
    a.n_started += b.n_started;
    a.n_lost += b.n_lost;
    a.busy_s += b.busy_s;
    a.last_tick = max(a.last_tick, b.last_tick);
    moments_merge(a.queue, b.queue);
    moments_merge(a.resp, b.resp);
  }
};
constexpr int kRecWords = rec_words<NodeOps>();
static_assert(sizeof(fognet_node_stats) == 192 && kRecWords == 24, "fognet_node_stats is 24 words");
static_assert(offsetof(fognet_node_stats, last_tick) == 5 * 8 && offsetof(fognet_node_stats, queue.min_raw) == 7 * 8 &&
                  offsetof(fognet_node_stats, queue.max_raw) == 8 * 8 &&
                  offsetof(fognet_node_stats, resp.min_raw) == 16 * 8 &&
                  offsetof(fognet_node_stats, resp.max_raw) == 17 * 8,
              "empty_word's indices");

// The contribution of one task, or of a group of at most 64: the seven counts
// (each <= 64) share one word, a byte each.
struct PartHead {
  uint64_t cnt;  // bytes: tasks, queued, started, lost, queue.count, queue.overflow, resp.count
  uint64_t busy;
  int64_t last;
  __device__ __forceinline__ PartHead shfl_xor(int m) const {
    return PartHead{shfl_xor_u64(cnt, m), shfl_xor_u64(busy, m), (int64_t)shfl_xor_u64((uint64_t)last, m)};
  }
  __device__ __forceinline__ void merge(const PartHead& b) {
    cnt += b.cnt;
    busy += b.busy;
    last = max(last, b.last);
  }
};
struct Part : PartHead {
  Sig queue, resp;
};
enum { kCTasks = 0, kCQueued = 8, kCStarted = 16, kCLost = 24, kCQn = 32, kCQovf = 40, kCRn = 48 };

__device__ __forceinline__ Part part_identity() { return Part{{0u, 0u, INT64_MIN}, sig_identity(), sig_identity()}; }

// every lane (all active) ends with the wave's total
__device__ __forceinline__ Part wave_merge(Part a) {
  wave_merge2(a.queue, a.resp, static_cast<PartHead&>(a));
  return a;
}

__device__ __forceinline__ void commit(fognet_node_stats* d, const Part& p) {
  atomic_add(&d->n_tasks, (p.cnt >> kCTasks) & 0xFFu);
  atomic_add(&d->n_queued, (p.cnt >> kCQueued) & 0xFFu);
  atomic_add(&d->n_started, (p.cnt >> kCStarted) & 0xFFu);
  atomic_add(&d->n_lost, (p.cnt >> kCLost) & 0xFFu);
  atomic_add(&d->busy_s, p.busy);
  const uint64_t rn = (p.cnt >> kCRn) & 0xFFu;
  if (rn != 0u) atomic_max_i64(&d->last_tick, p.last);
  commit_sig(&d->queue, (p.cnt >> kCQn) & 0xFFu, (p.cnt >> kCQovf) & 0xFFu, p.queue);
  commit_sig(&d->resp, rn, 0u, p.resp);
}

// ---------------------------------------------------------------- the pass
// kLds: the accumulators, the nodes' downlinks and their MIPS dividers live in LDS
template <bool kLds>
__global__ __launch_bounds__(kNodeThreads) void node_stats_kernel(ReplayArgs A, fognet_node_stats* out) {
  extern __shared__ uint64_t s_mem[];  // kLds: [N] records, [N] dl, [N] UDiv
  const int r = blockIdx.x;
  const int N = A.N;
  const int lane = (int)threadIdx.x & (kWave - 1);
  fognet_node_stats* const row = out + (size_t)r * (size_t)N;
  fognet_node_stats* const acc = kLds ? reinterpret_cast<fognet_node_stats*>(s_mem) : row;
  int64_t* const s_dl = reinterpret_cast<int64_t*>(s_mem + (size_t)N * kRecWords);
  UDiv* const s_div = reinterpret_cast<UDiv*>(s_mem + (size_t)N * (kRecWords + 1));
  if (!keyed_begin<NodeOps, kLds>(A, r, row, N, s_mem)) return;
  const size_t nbase = (size_t)r * (size_t)A.node_stride;
  if (kLds) {
    for (int j = threadIdx.x; j < N; j += kNodeThreads) {
      s_dl[j] = A.dl[nbase + j];
      s_div[j] = udiv_magic((uint32_t)A.mips[nbase + j]);
    }
  }
  keyed_ready<kLds>();
  auto load = [&](size_t o) { return load_row<kColStart | kColReq | kColEsc>(A, nullptr, o); };
  stream_rows(A, r, decided_tasks(A, r), load, [&](const Row& cur, int, bool decided) {
    const uint32_t k = (uint32_t)cur.node;
    const bool valid = decided && k < (uint32_t)N;
    Part p = part_identity();
    if (valid) {
      // of the node's own signal the rule needs the downlink alone (read first: the load is in flight below)
      const Emissions e = emissions(
          A, cur, [&](int j) { return kLds ? s_dl[j] : A.dl[nbase + j]; }, [](int) { return (int64_t)0; }, 0, 0);
      p.cnt = (uint64_t)1 << kCTasks;
      if (cur.status == 4u) p.cnt += (uint64_t)1 << kCQueued;
      if (cur.status == 5u) p.cnt += (uint64_t)1 << kCStarted;
      if (cur.status == 9u) p.cnt += (uint64_t)1 << kCLost;
      if (cur.done >= 0) {  // completed
        const uint32_t mips_k = kLds ? 0u : (uint32_t)A.mips[nbase + k];
        p.busy = kLds ? udiv((uint32_t)cur.req, s_div[k]) : (mips_k ? (uint32_t)cur.req / mips_k : 0u);
        p.last = cur.done;
        p.cnt += (uint64_t)1 << kCRn;
        sig_add(p.resp, cur.done - cur.t);
      }
      if (e.queued) {
        int64_t raw;
        if (qtime_raw(e.queue_start, e.queue_enq, raw)) {
          p.cnt += (uint64_t)1 << kCQn;
          sig_add(p.queue, raw);
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
  });
  keyed_end<NodeOps, kLds>(row, N, s_mem);
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
  return launch_reduce<NodeOps>(in, stats, R, N, out, s);
}

}  // namespace fognet
