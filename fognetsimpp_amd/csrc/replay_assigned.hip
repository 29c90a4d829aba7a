// replay_assigned.hip — the node model under a caller's decisions (fognet_replay_assigned_dev,
// fognet_run_assigned_dev): task i of a replication goes to node assign[i], and the pass fills
// status, start_tick, done_tick and the replay fields of the record.  With the node given, the
// broker's view no longer matters: every fog node is a FIFO single server over the tasks sent
// to it (fognet_hip.h "Assigned replay" states the model), so its completions obey
//   done = max(a, done_p) + s = f(done_p),  f: x -> max(x + A, B) with (A, B) = (s, a + s),
// and these functions compose associatively: (A1, B1) then (A2, B2) = (A1 + A2, max(B1 + A2, B2)).
// A node's chain is a segmented inclusive scan in trace order over its tasks.
//
// Two kernels on the caller's stream:
//   count  one 256-thread workgroup per replication checks the node parameters and the trace
//          (every precondition of fognet_batch_in, and assign inside [0, N)), counts the tasks of
//          every node with integer atomics (in LDS up to kAsgCountLdsMax nodes, else in the
//          workspace row) and scans the counts into offsets: node k's completion adverts are
//          rows [off[k], off[k + 1]) of the replication's advert row in the workspace;
//   chain  one wavefront per replication walks the trace in tiles of 64 tasks, task c0 + lane
//          in each lane, so every per-task row is read and written coalesced and nothing is
//          sorted.  Inside a tile the lanes of one node are found with one ballot per bit of the
//          node index (a lane's mask of equal keys); the scan over those scattered lanes is six
//          rounds of pointer jumping to the previous lane of the same node.  What a node
//          carries from tile to tile is its last completion and service time, its task count,
//          its service seconds and a cursor into its adverts: 28 B per node, in LDS up to
//          FOGNET_ASSIGNED_LDS_NODES nodes, else in the workspace.  One wavefront runs the tiles
//          in order, so no result depends on the order of any atomic.
// max_pending: task i sees 1 + its rank on its node - the adverts of that node that reached the
// broker before arrive[i].  A node's adverts are nondecreasing in its FIFO order (tasks that
// never complete hold kNever), so that number is a binary search in the node's advert row
// between the carried cursor (arrivals are nondecreasing) and the task's own rank.
//
// Composed scan elements can pass the int64 range before a result does (a service time is up
// to 2^31 - 1 s = 2^71 ticks): sums saturate at kSat = 2^62, which keeps every comparison with
// the 2^61 bound and with down_tick exact, and never wrap.  The chain is integer arithmetic
// only; the statistics of fognet_run_assigned_dev are the accumulators of replay_common.h
// (acc_task, the wide kernel's), whose queueTime values follow the reference's doubles.
#include "replay_common.h"

namespace fognet {

namespace {

constexpr int kAsgThreads = 256;
constexpr int kAsgCountLdsMax = 8192;                 // one 32-bit count per node: 32 KiB of LDS
constexpr int kAsgLdsMax = FOGNET_ASSIGNED_LDS_NODES; // 28 B of carry per node: 28 KiB per wavefront
constexpr uint64_t kSat = (uint64_t)1 << 62;
static_assert(FOGNET_ASSIGNED_TILE == kWave, "one task per lane and tile");

struct AsgArgs {
  const int32_t* assign;  // [R][T]
  AssignedWs w;
  int32_t carry_hbm;      // the carries live in the workspace (the count kernel initialises them)
};

// x + y for x, y <= kSat, saturated at kSat
__device__ __forceinline__ uint64_t sat_add(uint64_t x, uint64_t y) {
  const uint64_t s = x + y;
  return s < kSat ? s : kSat;
}

__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, kWave);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, kWave);
  return ((uint64_t)hi << 32) | lo;
}

// ---------------------------------------------------------------- count
// kLds: the counts live in LDS; else in the replication's offset row, scanned in place
template <bool kLds>
__global__ __launch_bounds__(kAsgThreads) void assigned_count_kernel(ReplayArgs A, AsgArgs P) {
  extern __shared__ uint32_t s_cnt[];  // kLds: [N]
  __shared__ uint32_t s_part[kAsgThreads];
  __shared__ int s_bad;
  const int r = blockIdx.x, N = A.N, T = A.T, tid = threadIdx.x;
  uint32_t* const off = P.w.off + (size_t)r * ((size_t)N + 1);
  const size_t tbase = (size_t)r * (size_t)T, nbase = (size_t)r * (size_t)A.node_stride;
  if (tid == 0) s_bad = 0;
  if (kLds) {
    for (int v = tid; v < N; v += kAsgThreads) s_cnt[v] = 0u;
  } else {
    for (int v = tid; v < N; v += kAsgThreads) off[v] = 0u;
    __threadfence();  // the zeroes are in memory before any atomic update of them
  }
  __syncthreads();
  bool bad = false;
  // the node parameters (fognet_batch_in's preconditions, as the replay kernels check them)
  const int64_t arrive0 = T > 0 ? A.arrive[tbase] : kNever;
  for (int j = tid; j < N; j += kAsgThreads) {
    const int32_t m = A.mips[nbase + j];
    const int64_t d = A.dl[nbase + j], u = A.ul[nbase + j], ia = A.init[nbase + j];
    const int64_t dn = A.down ? A.down[nbase + j] : kNever;
    bad |= (m <= 0) | (d < 0) | (u < 0) | (d > kMaxTick) | (u > kMaxTick) | (ia < u) | (ia >= arrive0);
    bad |= dn != kNever && (dn < ia || dn > kMaxTick);
    if (P.carry_hbm) {
      const size_t c = (size_t)r * (size_t)N + (size_t)j;
      P.w.c_done[c] = -1;
      P.w.c_busy[c] = 0u;
      P.w.c_S[c] = 0u;
      P.w.c_rank[c] = 0u;
      P.w.c_head[c] = 0u;
    }
  }
  // the trace and the assignment
  for (int i = tid; i < T; i += kAsgThreads) {
    const int64_t t = A.arrive[tbase + i], before = A.arrive[tbase + (i > 0 ? i - 1 : 0)];
    const int32_t rq = A.req[tbase + i], k = P.assign[tbase + i];
    const bool in = (uint32_t)k < (uint32_t)N;
    bad |= (t < before) | (rq < 0) | (t > kMaxTick) | !in;
    if (in) {
      if (kLds)
        (void)atomicAdd(&s_cnt[k], 1u);
      else
        (void)atomicAdd(&off[k], 1u);
    }
  }
  if (bad) s_bad = 1;  // (every writer stores the same value)
  __syncthreads();
  if (tid == 0) P.w.bad[r] = s_bad;
  // exclusive scan: every thread owns one run of consecutive nodes
  auto count_of = [&](int v) -> uint32_t {
    return kLds ? s_cnt[v] : __hip_atomic_load(&off[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  const int per = (N + kAsgThreads - 1) / kAsgThreads;
  const int v0 = min(tid * per, N), v1 = min(v0 + per, N);
  uint32_t sum = 0u;
  for (int v = v0; v < v1; ++v) sum += count_of(v);
  s_part[tid] = sum;
  __syncthreads();  // (and every count is read before any offset is written over it)
  uint32_t before = 0u, total = 0u;
  for (int t = 0; t < kAsgThreads; ++t) {
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

// ---------------------------------------------------------------- chain
// the record of a replication refused before its first decision (fognet_hip.h "Buffers")
template <bool kStats>
__device__ __forceinline__ void write_refused(fognet_rep_stats* S) {
  S->n_tasks = 0;
  S->max_pending = 0;
  S->status = FOGNET_ERR_ARG;
  S->events = 0;
  if (kStats) write_rep_stats(S, acc_identity(), abort_none(), false);
}

// kLds: the nodes' carries live in LDS; else in the workspace.  kStats: fognet_run_assigned_dev
// (the whole record, the histogram and the energy model as well).
template <bool kLds, bool kStats>
__global__ __launch_bounds__(kWave) void assigned_chain_kernel(ReplayArgs A, AsgArgs P) {
  extern __shared__ __align__(16) unsigned char s_dyn[];  // kLds: the carries
  __shared__ uint32_t s_hist[FOGNET_HIST_METRICS * FOGNET_HIST_BINS];
  __shared__ double s_e[kWave];
  const int r = blockIdx.x, lane = threadIdx.x, N = A.N, T = A.T;
  fognet_rep_stats* const S = A.out_stats + r;
  if (P.w.bad[r] != 0) {  // refused by the count kernel: nothing of its rows is touched
    if (lane == 0) write_refused<kStats>(S);
    return;
  }
  const size_t tbase = (size_t)r * (size_t)T, nbase = (size_t)r * (size_t)A.node_stride;
  // what node k carries from tile to tile
  int64_t* c_done;    // completion of its last queued task, before any crash cuts it (-1: no task yet)
  uint64_t* c_busy;   // its service seconds so far (kept for the energy model only)
  uint32_t* c_S;      // service seconds of that last task
  uint32_t* c_rank;   // tasks sent to it so far
  uint32_t* c_head;   // its adverts known to have reached the broker: rows [0, head) of its advert segment
  if constexpr (kLds) {
    c_done = reinterpret_cast<int64_t*>(s_dyn);
    c_busy = reinterpret_cast<uint64_t*>(s_dyn) + N;
    c_S = reinterpret_cast<uint32_t*>(s_dyn + (size_t)16 * (size_t)N);
    c_rank = c_S + N;
    c_head = c_rank + N;
    for (int j = lane; j < N; j += kWave) {
      c_done[j] = -1;
      c_busy[j] = 0u;
      c_S[j] = 0u;
      c_rank[j] = 0u;
      c_head[j] = 0u;
    }
  } else {
    const size_t c = (size_t)r * (size_t)N;
    c_done = P.w.c_done + c;
    c_busy = P.w.c_busy + c;
    c_S = P.w.c_S + c;
    c_rank = P.w.c_rank + c;
    c_head = P.w.c_head + c;
  }
  if (kStats)
    for (int h = lane; h < FOGNET_HIST_METRICS * FOGNET_HIST_BINS; h += kWave) s_hist[h] = 0u;
  __syncthreads();
  const uint32_t* const off = P.w.off + (size_t)r * ((size_t)N + 1);
  int64_t* const adv = P.w.adv + tbase;
  const int nbits = N > 1 ? 32 - __clz(N - 1) : 0;  // bits of a node index
  const bool energy = kStats && A.p_busy != nullptr;
  const bool hist = kStats && A.hist != nullptr;
  const uint64_t lt = ((uint64_t)1 << lane) - 1u;  // the lanes before this one

  Acc acc = acc_identity();
  AbortPt ab = abort_none();
  uint32_t max_pend = 0u;
  int n_short = 0;    // this lane's tasks that never complete (node-down)
  bool range = false; // a tick of this lane's tasks reached the replay's bound

  // the next tile's rows are loaded before the current tile is worked on
  int64_t nt = 0;
  int32_t nrq = 0, nk = 0;
  if (lane < T) {
    nt = A.arrive[tbase + lane];
    nrq = A.req[tbase + lane];
    nk = P.assign[tbase + lane];
  }
  for (int c0 = 0; c0 < T; c0 += kWave) {
    const int i = c0 + lane;
    const bool valid = i < T;
    const int64_t t = nt;
    const int32_t rq = nrq, k = nk;
    if (i + kWave < T) {
      nt = A.arrive[tbase + i + kWave];
      nrq = A.req[tbase + i + kWave];
      nk = P.assign[tbase + i + kWave];
    }
    // (the count kernel saw every index inside [0, N); the clamp keeps the gathers in bounds regardless)
    const uint32_t ku = valid ? min((uint32_t)k, (uint32_t)(N - 1)) : 0u;
    const int32_t mips_k = A.mips[nbase + ku];
    const int64_t dl_k = A.dl[nbase + ku], ul_k = A.ul[nbase + ku];
    const int64_t down_k = A.down ? A.down[nbase + ku] : kNever;
    const uint32_t off_k = off[ku];
    const int64_t cd = c_done[ku];
    const uint32_t cS = c_S[ku], cr = c_rank[ku], ch = c_head[ku];
    const uint64_t cC = energy ? c_busy[ku] : 0u;

    const uint32_t Sv = (uint32_t)rq / (uint32_t)max(mips_k, 1);  // requiredMIPS / MIPS (ComputeBrokerApp3.cc:276)
    const int64_t a = t + dl_k;
    const bool live = valid && a < down_k;  // else lost: it reaches a crashed node and takes no place in the queue

    // the lanes of the same node: all of them (ranks, adverts), and the live ones (the queue)
    uint64_t m_all = ballot(valid);
    for (int b = 0; b < nbits; ++b) {
      const bool bit = (ku >> b) & 1u;
      const uint64_t bb = ballot(valid && bit);
      m_all &= bit ? bb : ~bb;
    }
    if (!valid) m_all = 0u;
    const uint64_t m = live ? m_all & ballot(live) : 0u;
    const uint32_t rank = cr + (uint32_t)__popcll(m_all & lt);  // among the tasks sent to the node
    const bool last_all = valid && (m_all >> lane) == 1u;
    const bool last_live = live && (m >> lane) == 1u;
    const uint64_t prevs = m & lt;
    const int pred = prevs ? 63 - __clzll((long long)prevs) : -1;  // the task it queues behind, if in this tile

    // segmented inclusive scan by pointer jumping: after round j the lane holds the composition of the
    // last min(2^j, its position + 1) elements of its node's run in the tile, and p the lane before them
    const uint64_t sT = Sv >= kChainSCap ? kSat : (uint64_t)ticks_of(Sv);
    uint64_t fa = live ? sT : 0u, fb = live ? sat_add((uint64_t)a, sT) : 0u, fc = live ? (uint64_t)Sv : 0u;
    int p = pred;
    for (int round = 0; round < 6 && ballot(p >= 0) != 0u; ++round) {
      const int src = p >= 0 ? p : lane;
      const uint64_t pa = shfl_u64(fa, src), pb = shfl_u64(fb, src);
      const uint64_t pc = energy ? shfl_u64(fc, src) : 0u;
      const int pp = __shfl(p, src, kWave);
      if (p >= 0) {
        const uint64_t through = sat_add(pb, fa);
        fb = through > fb ? through : fb;
        fa = sat_add(pa, fa);
        fc += pc;
        p = pp;
      }
    }
    const bool has_carry = cd >= 0;
    const uint64_t over = sat_add(has_carry ? (uint64_t)cd : 0u, fa);
    const uint64_t done_u = over > fb ? over : fb;  // before any crash cuts it
    const int src = pred >= 0 ? pred : lane;
    const uint64_t done_up = shfl_u64(done_u, src);
    const uint32_t S_up = (uint32_t)__shfl((int)Sv, src, kWave);
    const bool has_prev = pred >= 0 || has_carry;
    const int64_t prev_done = pred >= 0 ? (int64_t)done_up : cd;
    const uint32_t prev_S = pred >= 0 ? S_up : cS;
    const int64_t start_u = has_prev && prev_done > a ? prev_done : a;

    // the task's outputs: the crash precedes its tick's events and cancels the timer
    uint32_t status = FOGNET_TASK_LOST;
    int64_t start = -1, done = -1;
    if (live) {
      status = has_prev ? arrival_status(prev_done, min(prev_S, kChainSCap), a, dl_k) : 5u;
      if (start_u < down_k) {
        start = start_u;
        if ((int64_t)done_u < down_k) done = (int64_t)done_u;
        // a task that starts arms its timer: a completion past the bound is refused there
        range |= Sv >= kChainSCap || done_u > (uint64_t)kMaxTick;
      }
      range |= a > kMaxTick;
    }
    if (valid) {
      const size_t o = tbase + (size_t)i;
      A.out_node[o] = k;
      A.out_status[o] = (uint8_t)status;
      A.out_start[o] = start;
      A.out_done[o] = done;
      // its completion advert, in its node's segment (a task that never completes stays pending)
      const uint32_t row = min(off_k + rank, (uint32_t)(T - 1));
      adv[row] = done >= 0 ? done + ul_k : kNever;
    }
    __threadfence_block();  // the tile's adverts are written before any lane searches them

    // pending tasks of its node as the broker counts them at this publish: the first row of its segment
    // at or after the carried cursor that is not before arrive[i] (bisection; a gallop from the cursor
    // with the outputs stored after the search measured 20 % slower at C5 and the driver's shape)
    uint32_t lo = ch, hi = rank;
    if (valid) {
      const int64_t* const seg = adv + off_k;
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        // (rows of the segment lie inside the advert row; the clamp keeps the load so regardless)
        const uint32_t row = min(off_k + mid, (uint32_t)(T - 1)) - off_k;
        if (seg[row] < t)
          lo = mid + 1u;
        else
          hi = mid;
      }
      max_pend = max(max_pend, 1u + rank - lo);
    }

    // the carries, by the node's last lane of the tile
    if (last_all) {
      c_rank[ku] = rank + 1u;
      c_head[ku] = lo;
    }
    if (last_live) {
      c_done[ku] = (int64_t)done_u;
      c_S[ku] = Sv;
      if (energy) c_busy[ku] = cC + fc;
    }
    if (!kLds) __threadfence_block();  // the next tile reads them back

    if (valid && done < 0) n_short += 1;
    if (kStats && valid) {
      if (done >= 0) {
        acc_task(acc, ab, t, a, start, done, Sv, status, i, hist ? s_hist : nullptr);
        if (hist) atomicAdd(&s_hist[FOGNET_HIST_BINS + hist_bin(done - t)], 1u);
      } else {
        // node-down: acked at arrival (status 4/5) or lost; a queued task that started before
        // the crash still emitted its queueTime (ComputeBrokerApp3.cc:238)
        if (status == 5u) acc.n5 += 1u;
        if (status == 4u) {
          acc.n4 += 1u;
          if (start >= 0) acc_qtime(acc, ab, start, a, i, hist ? s_hist : nullptr);
        }
      }
    }
  }

  if (ballot(range) != 0u) {  // refused as a whole: its rows are undefined, nothing reaches hist
    if (lane == 0) write_refused<kStats>(S);
    return;
  }
  const uint32_t mp = ~wave_min_u32(~max_pend);
  int shorts = n_short;
  for (int w = kWave / 2; w > 0; w >>= 1) shorts += __shfl_xor(shorts, w, kWave);
  if (kStats) {
    acc = wave_merge(acc);
    ab = wave_min_abort(ab);
  }
  if (lane == 0) {
    S->n_tasks = T;
    S->max_pending = (int32_t)mp;
    S->status = FOGNET_OK;
    // initial adverts + publish, arrival, release, advert per task (publish, arrival for a
    // task a crash keeps from completing): the count replay_wide.hip states at its record write
    S->events = 2 * (int64_t)N + 4 * (int64_t)T - 2 * (int64_t)shorts;
    if (kStats) write_rep_stats(S, acc, ab, A.ref_abort);
  }
  if constexpr (kStats) {
    __syncthreads();  // every lane's histogram counts are in LDS
    if (hist)
      for (int h = lane; h < FOGNET_HIST_METRICS * FOGNET_HIST_BINS; h += kWave)
        if (s_hist[h]) atomicAdd((unsigned long long*)&A.hist[h], (unsigned long long)s_hist[h]);
    if (energy) {  // fognet_rep_stats.energy_j, in node order
      const int64_t H = T > 0 ? acc.last : 0;
      double* const row = A.out_energy ? A.out_energy + (size_t)r * (size_t)N : nullptr;
      const double sum = energy_sum_wave<8>(c_busy, 1, A.p_busy + nbase, A.p_idle + nbase, N, H, row, lane, s_e);
      if (lane == 0) S->energy_j = sum;
    }
  }
}

template <bool kLds>
void launch_chain(const ReplayArgs& a, const AsgArgs& p, bool stats, size_t lds_bytes, hipStream_t s) {
  if (stats)
    hipLaunchKernelGGL((assigned_chain_kernel<kLds, true>), dim3(a.R), dim3(kWave), lds_bytes, s, a, p);
  else
    hipLaunchKernelGGL((assigned_chain_kernel<kLds, false>), dim3(a.R), dim3(kWave), lds_bytes, s, a, p);
}

}  // namespace

int32_t replay_assigned_lds_max() { return kAsgLdsMax; }

hipError_t launch_replay_assigned(const ReplayArgs& a, const int32_t* assign, const AssignedWs& w, bool stats,
                                  bool force_hbm, int stages, hipStream_t s) {
  if (a.R <= 0) return hipSuccess;
  const bool carry_lds = a.N <= kAsgLdsMax && !force_hbm;
  const AsgArgs p{assign, w, carry_lds ? 0 : 1};
  if (a.N <= kAsgCountLdsMax && !force_hbm)
    hipLaunchKernelGGL(assigned_count_kernel<true>, dim3(a.R), dim3(kAsgThreads), (size_t)a.N * sizeof(uint32_t), s, a,
                       p);
  else
    hipLaunchKernelGGL(assigned_count_kernel<false>, dim3(a.R), dim3(kAsgThreads), 0, s, a, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || stages < 2) return e;
  if (carry_lds)
    launch_chain<true>(a, p, stats, (size_t)a.N * 28u, s);
  else
    launch_chain<false>(a, p, stats, 0, s);
  return hipGetLastError();
}

}  // namespace fognet
