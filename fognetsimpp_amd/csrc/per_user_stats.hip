// per_user_stats.hip — the user-side signals of a finished replay per publishing user
// (fognet_per_user_stats_dev) and their job reduction (fognet_reduce_user_stats_dev): what
// the reference records per user module (latency, latencyH1, taskTime, mqttApp2.ned:49-54)
// plus each user's share of the broker's delay.  The signals and their emission rule are
// user_stats.hip's; task i's links are those of user_of[i].
//
// The pass is a reduction keyed by user over the replay's per-task arrays (25 B per task;
// 26 under EXT_HIER).  One workgroup per replication streams them coalesced, 64 tasks per
// wavefront and step.  The accumulators are one fognet_user_stats per user: in LDS up to
// kUserLdsMax users, with the replication's user links beside them (copied to the caller's
// records at the end), above that the caller's records themselves, set to the empty record
// first.  Every update is an integer atomic (stats_atomics.h), so the records do not depend
// on the order of the updates.
//
// mqttApp2's users publish in turn: a 64-task step holds about min(U, 64) users with 64 / U
// tasks each, and one user per replication puts all 64 lanes on one record.  Each wavefront
// groups its 64 tasks by user (one ballot per bit of the user index gives every lane the lanes
// that share its user); a group at or above the layout's threshold is summed in registers across
// the wave, two signals per round, in a leader/ballot walk over those groups, and committed
// once by its leader; the tasks of smaller groups commit themselves.  The thresholds are
// measurements: 8 for the caller's records in HBM, none for the records in LDS.
#include "stats_atomics.h"

namespace fognet {

namespace {

constexpr int kPuThreads = 256;
constexpr int kPuWaves = kPuThreads / kWave;
constexpr int kUserLdsMax = 128;  // 288 B of record + 16 B of links per user: 38 KiB, four workgroups per CU
// The smallest group that is summed across the wave before it is committed, per layout; above
// kWave no group is.  Measured: LDS atomics take 64 lanes on one record better
// than the butterfly does (and the kernel without it needs fewer registers), global atomics do not.
#ifndef FOGNET_USER_GROUP_REDUCE_LDS
#define FOGNET_USER_GROUP_REDUCE_LDS (kWave + 1)
#endif
#ifndef FOGNET_USER_GROUP_REDUCE_HBM
#define FOGNET_USER_GROUP_REDUCE_HBM 8
#endif
constexpr int kMomWords = (int)(sizeof(fognet_moments) / sizeof(uint64_t));
constexpr int kURecWords = (int)(sizeof(fognet_user_stats) / sizeof(uint64_t));
static_assert(sizeof(fognet_moments) == 72 && sizeof(fognet_user_stats) == 288 && kURecWords == 36,
              "fognet_user_stats is four fognet_moments of nine words");
static_assert(offsetof(fognet_moments, min_raw) == 8 && offsetof(fognet_moments, max_raw) == 16, "empty_word's indices");

// word w of the empty record: every signal's min_raw INT64_MAX, max_raw INT64_MIN, the rest 0
__device__ __forceinline__ uint64_t empty_word(int w) {
  const int f = w % kMomWords;
  return f == 1 ? (uint64_t)INT64_MAX : f == 2 ? (uint64_t)INT64_MIN : 0u;
}

// extrema, 128-bit sum and 192-bit sum of squares of one signal's raw values
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

// The contribution of one task, or of a group of at most 64.  A task emits one delay, one
// or two latencyH1 (the broker's pubAck, plus the node's "task queued" ack), at most one
// latency and at most one taskTime: a group holds at most 128 latencyH1 emissions and 64 of
// every other kind, so the seven counts share one word, a byte each.
struct UPart {
  uint64_t cnt;  // bytes: delay.count, latency.count/.overflow, latencyH1.count/.overflow, taskTime.count/.overflow
  Sig delay, lat, h1, tt;
};
enum { kCDn = 0, kCLn = 8, kCLovf = 16, kCHn = 24, kCHovf = 32, kCTn = 40, kCTovf = 48 };

// emit(signal, (simTime() - created) * 1000): an overflowing product is a lost emission
__device__ __forceinline__ void emit_ms(Sig& s, uint64_t& cnt, int sh_n, int sh_ovf, int64_t d) {
  int64_t raw;
  if (ms_raw(d, raw)) {
    cnt += (uint64_t)1 << sh_n;
    sig_add(s, raw);
  } else {
    cnt += (uint64_t)1 << sh_ovf;
  }
}

// Butterfly over the 64 lanes (all active) of two signals: every lane ends with the totals.
__device__ __forceinline__ void wave_merge2(Sig& a, Sig& b) {
#pragma unroll 1
  for (int m = kWave / 2; m > 0; m >>= 1) {
    const Sig oa = sig_shfl_xor(a, m), ob = sig_shfl_xor(b, m);
    sig_merge(a, oa);
    sig_merge(b, ob);
  }
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int m = kWave / 2; m > 0; m >>= 1) v += shfl_xor_u64(v, m);
  return v;
}

__device__ __forceinline__ void commit_sig(fognet_moments* m, uint64_t n, uint64_t ovf, const Sig& s) {
  commit_moments(m, n, ovf, s.mn, s.mx, s.s_lo, s.s_hi, s.q_lo, s.q_hi, s.q_top);
}

__device__ __forceinline__ void commit(fognet_user_stats* d, const UPart& p) {
  commit_sig(&d->delay, (p.cnt >> kCDn) & 0xFFu, 0u, p.delay);
  commit_sig(&d->latency, (p.cnt >> kCLn) & 0xFFu, (p.cnt >> kCLovf) & 0xFFu, p.lat);
  commit_sig(&d->latencyH1, (p.cnt >> kCHn) & 0xFFu, (p.cnt >> kCHovf) & 0xFFu, p.h1);
  commit_sig(&d->taskTime, (p.cnt >> kCTn) & 0xFFu, (p.cnt >> kCTovf) & 0xFFu, p.tt);
}

// ---------------------------------------------------------------- the pass
struct UserRow {
  int64_t t, done;
  int32_t node, user;
  uint32_t status;
  uint32_t esc;  // EXT_HIER: the parent took the decision (the node ack leaves a hop later)
};

__device__ __forceinline__ UserRow load_row(const ReplayArgs& A, const int32_t* user_of, size_t o) {
  return UserRow{A.arrive[o], A.out_done[o], A.out_node[o], user_of[o], (uint32_t)A.out_status[o],
                 A.out_esc ? (uint32_t)A.out_esc[o] : 0u};
}

struct UserArgs {
  const int32_t* user_of;  // [R][T]
  const int64_t* ul;       // [R|1][U] user -> broker
  const int64_t* dl;       // [R|1][U] broker -> user
  int32_t U, link_stride;
  fognet_user_stats* out;  // [R][U]
  int64_t* n_unassigned;   // [R], nullable
};

// kLds: the accumulators and the replication's user links live in LDS
template <bool kLds>
__global__ __launch_bounds__(kPuThreads) void per_user_stats_kernel(ReplayArgs A, UserArgs P) {
  extern __shared__ uint64_t s_mem[];  // kLds: [U] records, [U] ul, [U] dl
  __shared__ unsigned long long s_unassigned;
  const int r = blockIdx.x;
  const int U = P.U;
  const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x / kWave;
  fognet_user_stats* const row = P.out + (size_t)r * (size_t)U;
  fognet_user_stats* const acc = kLds ? reinterpret_cast<fognet_user_stats*>(s_mem) : row;
  int64_t* const s_ul = reinterpret_cast<int64_t*>(s_mem + (size_t)U * kURecWords);
  int64_t* const s_dl = s_ul + U;
  const int32_t rep_status = A.out_stats[r].status;
  const bool ok = rep_status == FOGNET_OK || rep_status == FOGNET_REF_ABORTED;
  // a failed replication: U empty records, nothing of its rows, its users or its links is read
  const bool direct = !kLds || !ok;
  uint64_t* const acc_w = direct ? reinterpret_cast<uint64_t*>(row) : s_mem;
  const size_t words = (size_t)U * kURecWords;
  for (size_t w = threadIdx.x; w < words; w += kPuThreads) acc_w[w] = empty_word((int)(w % kURecWords));
  if (!ok) {
    if (threadIdx.x == 0 && P.n_unassigned) P.n_unassigned[r] = 0;
    return;
  }
  if (threadIdx.x == 0) s_unassigned = 0u;
  const size_t lbase = (size_t)r * (size_t)P.link_stride;
  if (kLds) {
    for (int u = threadIdx.x; u < U; u += kPuThreads) {
      s_ul[u] = P.ul[lbase + u];
      s_dl[u] = P.dl[lbase + u];
    }
  } else {
    __threadfence();  // the empty records are in memory before any atomic update of them
  }
  __syncthreads();
  const size_t tbase = (size_t)r * (size_t)A.T;
  const size_t nbase = (size_t)r * (size_t)A.node_stride;
  int64_t n64 = A.out_stats[r].n_tasks;  // decided tasks (written by the replay)
  const int n = (int)(n64 < 0 ? 0 : n64 > A.T ? A.T : n64);
  const int chunks = (n + kWave - 1) / kWave;
  // lanes past n reload the chunk's first task (in bounds, unused)
  auto offset_of = [&](int c) { return tbase + (size_t)(c * kWave + lane < n ? c * kWave + lane : c * kWave); };
  constexpr int kGroupReduce = kLds ? FOGNET_USER_GROUP_REDUCE_LDS : FOGNET_USER_GROUP_REDUCE_HBM;
  uint32_t unassigned = 0u;  // per wavefront (uniform)
  const int key_bits = U > 1 ? 32 - __clz(U - 1) : 0;  // the bits in which two users below U can differ
  UserRow cur{};
  if (wave < chunks) cur = load_row(A, P.user_of, offset_of(wave));
  for (int c = wave; c < chunks; c += kPuWaves) {
    UserRow nxt = cur;  // the next chunk's loads are in flight while this one is accumulated
    if (c + kPuWaves < chunks) nxt = load_row(A, P.user_of, offset_of(c + kPuWaves));
    const uint32_t u = (uint32_t)cur.user;
    const bool decided = c * kWave + lane < n;
    const bool valid = decided && u < (uint32_t)U;
    unassigned += (uint32_t)__popcll(ballot(decided && !valid));
    UPart p{0u, sig_identity(), sig_identity(), sig_identity(), sig_identity()};
    if (valid) {
      const int64_t uu = kLds ? s_ul[u] : P.ul[lbase + u];
      const int64_t ud = kLds ? s_dl[u] : P.dl[lbase + u];
      // (a decided publish's node lies in [0, N); an index outside it reads node 0's links)
      const size_t k = nbase + (size_t)((uint32_t)cur.node < (uint32_t)A.N ? cur.node : 0);
      const int64_t created = cur.t - uu;
      const int64_t relay = A.ul[k] + ud;  // node -> broker -> user
      p.cnt = (uint64_t)1 << kCDn;         // delay: at the broker (:143), a simtime_t (s)
      sig_add(p.delay, uu);
      emit_ms(p.h1, p.cnt, kCHn, kCHovf, cur.t + ud - created);  // broker pubAck status 4 -> latencyH1
      // node ack sent at the task's arrival: t + dl_k, the parent's hop later for an escalated task
      const int64_t at_arrival = cur.t + A.dl[k] + (cur.esc ? A.hier_up : 0) + relay - created;
      if (cur.status == 5u)
        emit_ms(p.lat, p.cnt, kCLn, kCLovf, at_arrival);  // "task assigned" -> latency
      else if (cur.status == 4u)
        emit_ms(p.h1, p.cnt, kCHn, kCHovf, at_arrival);  // "task queued" -> latencyH1
      // (status 9: the task reached a crashed node, which sends no ack)
      if (cur.done >= 0) emit_ms(p.tt, p.cnt, kCTn, kCTovf, cur.done + relay - created);  // status 6 -> taskTime
    }
    // group the wave's tasks by user: `same` = the valid lanes that hold this lane's user, one ballot
    // per bit of the key, so finding the groups costs log2(U) steps however many users the step holds
    bool large = false;
    uint64_t same = 0u;
    if (kGroupReduce <= kWave) {
      same = ballot(valid);
      for (int b = 0; b < key_bits; ++b) {
        const bool bit = ((u >> b) & 1u) != 0u;
        const uint64_t m = ballot(bit);
        same &= bit ? m : ~m;
      }
      large = valid && __popcll(same) >= kGroupReduce;
    }
    const bool self = valid && !large;  // this lane's task commits itself
    // the leader/ballot walk over the groups that are summed (at most 64 / kGroupReduce)
    uint64_t todo = kGroupReduce <= kWave ? ballot(large && lane == __ffsll((long long)same) - 1) : 0u;
    while (todo != 0u) {
      const int leader = __ffsll((long long)todo) - 1;
      todo &= todo - 1u;
      const uint32_t u0 = readlane_u32(u, leader);
      const bool mine = (((uint64_t)readlane_i64((int64_t)same, leader) >> lane) & 1u) != 0u;
      UPart g;
      g.cnt = wave_sum_u64(mine ? p.cnt : 0u);
      g.delay = mine ? p.delay : sig_identity();
      g.lat = mine ? p.lat : sig_identity();
      wave_merge2(g.delay, g.lat);
      g.h1 = mine ? p.h1 : sig_identity();
      g.tt = mine ? p.tt : sig_identity();
      wave_merge2(g.h1, g.tt);
      if (lane == leader) commit(&acc[u0], g);
    }
    if (self) commit(&acc[u], p);
    cur = nxt;
  }
  if (lane == 0 && unassigned != 0u) (void)atomicAdd(&s_unassigned, (unsigned long long)unassigned);
  __syncthreads();
  if (threadIdx.x == 0 && P.n_unassigned) P.n_unassigned[r] = (int64_t)s_unassigned;
  if (kLds) {
    uint64_t* const dst = reinterpret_cast<uint64_t*>(row);
    for (size_t w = threadIdx.x; w < words; w += kPuThreads) dst[w] = s_mem[w];
  }
}

// ---------------------------------------------------------------- job reduction
constexpr int kUserReduceThreads = 128;

__device__ __forceinline__ void user_merge(fognet_user_stats& a, const fognet_user_stats& b) {
  moments_merge(a.delay, b.delay);
  moments_merge(a.latency, b.latency);
  moments_merge(a.latencyH1, b.latencyH1);
  moments_merge(a.taskTime, b.taskTime);
}

__device__ __forceinline__ fognet_user_stats user_empty() {
  fognet_user_stats s = {};
  s.delay.min_raw = s.latency.min_raw = s.latencyH1.min_raw = s.taskTime.min_raw = INT64_MAX;
  s.delay.max_raw = s.latency.max_raw = s.latencyH1.max_raw = s.taskTime.max_raw = INT64_MIN;
  return s;
}

// Workgroup u merges column u of the [R][U] records: its threads stride over the
// replications, then a tree in LDS (36 KiB).
__global__ __launch_bounds__(kUserReduceThreads) void user_reduce_kernel(const fognet_user_stats* in,
                                                                         const fognet_rep_stats* stats, int32_t R,
                                                                         int32_t U, fognet_user_stats* out) {
  __shared__ fognet_user_stats sh[kUserReduceThreads];
  const int u = blockIdx.x;
  fognet_user_stats a = user_empty();
  for (int r = threadIdx.x; r < R; r += kUserReduceThreads)
    if (stats[r].status == FOGNET_OK) user_merge(a, in[(size_t)r * (size_t)U + (size_t)u]);
  sh[threadIdx.x] = a;
  __syncthreads();
  for (int w = kUserReduceThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) user_merge(sh[threadIdx.x], sh[threadIdx.x + w]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[u] = sh[0];
}

}  // namespace

int32_t per_user_stats_lds_max() { return kUserLdsMax; }

hipError_t launch_per_user_stats(const ReplayArgs& a, const int32_t* user_of, int32_t U, int32_t link_stride,
                                 const int64_t* user_ul, const int64_t* user_dl, fognet_user_stats* out,
                                 int64_t* n_unassigned, bool force_hbm, hipStream_t s) {
  if (a.R <= 0 || (U <= 0 && !n_unassigned)) return hipSuccess;
  const UserArgs p{user_of, user_ul, user_dl, U, link_stride, out, n_unassigned};
  if (U <= kUserLdsMax && !force_hbm) {
    const size_t lds = (size_t)U * (kURecWords + 2) * sizeof(uint64_t);
    hipLaunchKernelGGL(per_user_stats_kernel<true>, dim3(a.R), dim3(kPuThreads), lds, s, a, p);
  } else {
    hipLaunchKernelGGL(per_user_stats_kernel<false>, dim3(a.R), dim3(kPuThreads), 0, s, a, p);
  }
  return hipGetLastError();
}

hipError_t launch_reduce_user_stats(const fognet_user_stats* in, const fognet_rep_stats* stats, int32_t R, int32_t U,
                                    fognet_user_stats* out, hipStream_t s) {
  if (U <= 0) return hipSuccess;
  hipLaunchKernelGGL(user_reduce_kernel, dim3(U), dim3(kUserReduceThreads), 0, s, in, stats, R, U, out);
  return hipGetLastError();
}

}  // namespace fognet
