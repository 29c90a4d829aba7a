// per_user_stats.hip — the user-side signals of a finished replay per publishing user
// (fognet_per_user_stats_dev) and their job reduction (fognet_reduce_user_stats_dev): what
// the reference records per user module (latency, latencyH1, taskTime, mqttApp2.ned:49-54)
// plus each user's share of the broker's delay.  The signals and their emission rule are
// signals.h's; task i's links are those of user_of[i].
//
// The pass is a reduction keyed by user over the replay's per-task arrays (25 B per task;
// 26 under EXT_HIER), streamed by one workgroup per replication (signals.h's stream_rows).
// The accumulators are one fognet_user_stats per user: in LDS up to kUserLdsMax users, with
// the replication's user links beside them, above that the caller's records themselves
// (signals.h's keyed frame).  Every update is an integer atomic (signals.h), so the records
// do not depend on the order of the updates.
//
// mqttApp2's users publish in turn: a 64-task step holds about min(U, 64) users with 64 / U
// tasks each, and one user per replication puts all 64 lanes on one record.  Each wavefront
// groups its 64 tasks by user (one ballot per bit of the user index gives every lane the lanes
// that share its user); a group at or above the layout's threshold is summed in registers across
// the wave, two signals per round, in a leader/ballot walk over those groups, and committed
// once by its leader; the tasks of smaller groups commit themselves.  The thresholds are
// measurements: 8 for the caller's records in HBM, none for the records in LDS.
#include "signals.h"

namespace fognet {

namespace {

constexpr int kPuThreads = kPassThreads;
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

// fognet_user_stats as signals.h takes a record: four fognet_moments, no head
struct UserOps {
  using Rec = fognet_user_stats;
  static constexpr int kHeadWords = 0;
  static __device__ __forceinline__ uint64_t head_empty(int) { return 0u; }
  static __device__ __forceinline__ void merge(Rec& a, const Rec& b) {
    moments_merge(a.delay, b.delay);
    moments_merge(a.latency, b.latency);
    moments_merge(a.latencyH1, b.latencyH1);
    moments_merge(a.taskTime, b.taskTime);
  }
};
constexpr int kURecWords = rec_words<UserOps>();
static_assert(sizeof(fognet_user_stats) == 288 && kURecWords == 36, "fognet_user_stats is four fognet_moments of nine words");

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

__device__ __forceinline__ void commit(fognet_user_stats* d, const UPart& p) {
  commit_sig(&d->delay, (p.cnt >> kCDn) & 0xFFu, 0u, p.delay);
  commit_sig(&d->latency, (p.cnt >> kCLn) & 0xFFu, (p.cnt >> kCLovf) & 0xFFu, p.lat);
  commit_sig(&d->latencyH1, (p.cnt >> kCHn) & 0xFFu, (p.cnt >> kCHovf) & 0xFFu, p.h1);
  commit_sig(&d->taskTime, (p.cnt >> kCTn) & 0xFFu, (p.cnt >> kCTovf) & 0xFFu, p.tt);
}

// ---------------------------------------------------------------- the pass
struct UserArgs : UserLinks {
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
  const int lane = (int)threadIdx.x & (kWave - 1);
  fognet_user_stats* const row = P.out + (size_t)r * (size_t)U;
  fognet_user_stats* const acc = kLds ? reinterpret_cast<fognet_user_stats*>(s_mem) : row;
  int64_t* const s_ul = reinterpret_cast<int64_t*>(s_mem + (size_t)U * kURecWords);
  int64_t* const s_dl = s_ul + U;
  if (!keyed_begin<UserOps, kLds>(A, r, row, U, s_mem)) {  // (nothing of its users or its links is read either)
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
  }
  keyed_ready<kLds>();
  const size_t nbase = (size_t)r * (size_t)A.node_stride;
  constexpr int kGroupReduce = kLds ? FOGNET_USER_GROUP_REDUCE_LDS : FOGNET_USER_GROUP_REDUCE_HBM;
  uint32_t unassigned = 0u;  // per wavefront (uniform)
  const int key_bits = U > 1 ? 32 - __clz(U - 1) : 0;  // the bits in which two users below U can differ
  auto load = [&](size_t o) { return load_row<kColUser | kColEsc>(A, P.user_of, o); };
  stream_rows(A, r, decided_tasks(A, r), load, [&](const Row& cur, int, bool decided) {
    const uint32_t u = (uint32_t)cur.user;
    const bool valid = decided && u < (uint32_t)U;
    unassigned += (uint32_t)__popcll(ballot(decided && !valid));
    UPart p{0u, sig_identity(), sig_identity(), sig_identity(), sig_identity()};
    if (valid) {
      const Emissions e = emissions(
          A, cur, [&](int k) { return A.dl[nbase + k]; }, [&](int k) { return A.ul[nbase + k]; },
          kLds ? s_ul[u] : P.ul[lbase + u], kLds ? s_dl[u] : P.dl[lbase + u]);
      p.cnt = (uint64_t)1 << kCDn;
      sig_add(p.delay, e.delay);
      emit_ms(p.h1, p.cnt, kCHn, kCHovf, e.puback_d);
      if (e.first == kAckLatency) emit_ms(p.lat, p.cnt, kCLn, kCLovf, e.first_d);
      else if (e.first == kAckLatencyH1) emit_ms(p.h1, p.cnt, kCHn, kCHovf, e.first_d);
      if (e.completed) emit_ms(p.tt, p.cnt, kCTn, kCTovf, e.done_d);
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
      NoHead none;
      g.cnt = wave_sum_u64(mine ? p.cnt : 0u);
      g.delay = mine ? p.delay : sig_identity();
      g.lat = mine ? p.lat : sig_identity();
      wave_merge2(g.delay, g.lat, none);
      g.h1 = mine ? p.h1 : sig_identity();
      g.tt = mine ? p.tt : sig_identity();
      wave_merge2(g.h1, g.tt, none);
      if (lane == leader) commit(&acc[u0], g);
    }
    if (self) commit(&acc[u], p);
  });
  if (lane == 0 && unassigned != 0u) (void)atomicAdd(&s_unassigned, (unsigned long long)unassigned);
  __syncthreads();
  if (threadIdx.x == 0 && P.n_unassigned) P.n_unassigned[r] = (int64_t)s_unassigned;
  keyed_end<UserOps, kLds>(row, U, s_mem);
}

}  // namespace

int32_t per_user_stats_lds_max() { return kUserLdsMax; }

hipError_t launch_per_user_stats(const ReplayArgs& a, const UserLinks& users, fognet_user_stats* out,
                                 int64_t* n_unassigned, bool force_hbm, hipStream_t s) {
  const int32_t U = users.U;
  if (a.R <= 0 || (U <= 0 && !n_unassigned)) return hipSuccess;
  const UserArgs p{users, out, n_unassigned};
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
  return launch_reduce<UserOps>(in, stats, R, U, out, s);
}

}  // namespace fognet
