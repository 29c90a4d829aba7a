// user_stats.hip — the user-side signals of the offload loop, computed on the
// device from a finished replay (fognet_user_stats_dev): one
// record per replication, the links of every publish's user given per replication or
// per task.  The signals and their emission rule are signals.h's; under EXT_HIER the
// rule needs the replay's escalation flags (capi.hip refuses that policy without them).
//
// Memory-bound: one 256-thread workgroup per replication, its threads stride over the
// tasks (21 B per task, 22 under EXT_HIER, plus the links), then a tree in LDS per signal.
#include "signals.h"

namespace fognet {

namespace {

constexpr int kUserThreads = 256;
constexpr int kSignals = 4;  // delay, latency, latencyH1, taskTime

// one signal of one thread: its moments, its emissions and the ones lost
struct Tally {
  Sig s;
  uint64_t n, ovf;
};

__device__ __forceinline__ void tally(Tally& m, int64_t raw) {
  m.n += 1u;
  sig_add(m.s, raw);
}

// emit(signal, (simTime() - created) * 1000) (mqttApp2.cc:260,272,282); an
// overflowing product throws and mqttApp2's catch drops the emission
__device__ __forceinline__ void tally_ms(Tally& m, int64_t d) {
  int64_t raw;
  if (ms_raw(d, raw)) tally(m, raw);
  else m.ovf += 1u;
}

__device__ __forceinline__ void tally_merge(Tally& a, const Tally& b) {
  a.n += b.n;
  a.ovf += b.ovf;
  sig_merge(a.s, b.s);
}

__global__ __launch_bounds__(kUserThreads) void user_stats_kernel(ReplayArgs A, const int64_t* uul, const int64_t* udl,
                                                                  int32_t per_task, fognet_user_stats* out) {
  __shared__ Tally sh[kUserThreads];
  const int r = blockIdx.x;
  const size_t tbase = (size_t)r * (size_t)A.T;
  const size_t nbase = (size_t)r * (size_t)A.node_stride;
  // a failed replication: the empty record, nothing of its rows or links is read
  const int n = rep_ok(A, r) ? decided_tasks(A, r) : 0;
  Tally m[kSignals];
  for (int s = 0; s < kSignals; ++s) m[s] = Tally{sig_identity(), 0u, 0u};
  for (int i = threadIdx.x; i < n; i += kUserThreads) {
    const size_t o = tbase + (size_t)i;
    const Row x = load_row<kColEsc>(A, nullptr, o);
    const size_t uo = per_task ? o : (size_t)r;
    const Emissions e = emissions(
        A, x, [&](int k) { return A.dl[nbase + k]; }, [&](int k) { return A.ul[nbase + k]; }, uul[uo], udl[uo]);
    tally(m[0], e.delay);
    tally_ms(m[2], e.puback_d);
    if (e.first == kAckLatency) tally_ms(m[1], e.first_d);
    else if (e.first == kAckLatencyH1) tally_ms(m[2], e.first_d);
    if (e.completed) tally_ms(m[3], e.done_d);
  }
  fognet_moments* dst[kSignals] = {&out[r].delay, &out[r].latency, &out[r].latencyH1, &out[r].taskTime};
  for (int s = 0; s < kSignals; ++s) {
    sh[threadIdx.x] = m[s];
    __syncthreads();
    for (int w = kUserThreads / 2; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w) tally_merge(sh[threadIdx.x], sh[threadIdx.x + w]);
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      const Tally& b = sh[0];
      const Sig& v = b.s;
      *dst[s] = fognet_moments{(int64_t)b.n, v.mn, v.mx, v.s_lo, v.s_hi, v.q_lo, v.q_hi, v.q_top, (int64_t)b.ovf};
    }
    __syncthreads();
  }
}

}  // namespace

hipError_t launch_user_stats(const ReplayArgs& a, const int64_t* user_ul, const int64_t* user_dl, int32_t per_task,
                             fognet_user_stats* out, hipStream_t s) {
  if (a.R <= 0) return hipSuccess;
  hipLaunchKernelGGL(user_stats_kernel, dim3(a.R), dim3(kUserThreads), 0, s, a, user_ul, user_dl, per_task, out);
  return hipGetLastError();
}

}  // namespace fognet
