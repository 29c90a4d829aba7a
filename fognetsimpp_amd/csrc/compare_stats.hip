// compare_stats.hip — paired comparison of two replays of the same traces (fognet_compare_dev)
// and its job reduction (fognet_reduce_compare_dev).  fognet_hip.h "Paired comparison" states
// the record once: per task B minus A of the start, the service and the completion, how many
// tasks moved to another node or changed their status, and which run won.
//
// The publish tick cancels in every difference, so the pass reads no trace column and no link:
// node, status, start and done of both runs, 42 B per task, streamed by one workgroup per
// replication (signals.h's stream_rows over a row that holds both sides).  Nothing is keyed:
// each lane keeps the three signals and its counts in registers, a wavefront merges them in one
// butterfly and commits once into the workgroup's record in LDS, which is then copied to the
// caller's row.  The two histogram rows are counted in LDS and flushed with 64-bit atomics.
// Every update is one of signals.h's integer atomics, so a record does not depend on their order.
#include "signals.h"

namespace fognet {

namespace {

// fognet_compare_stats as signals.h takes a record: the statuses (one word), 22 counts, then
// d_start, d_service and d_resp.  The job reduction merges the records that name both runs OK.
struct CompareOps {
  using Rec = fognet_compare_stats;
  static constexpr int kHeadWords = 23;
  static __device__ __forceinline__ uint64_t head_empty(int) { return 0u; }  // (statuses FOGNET_OK)
  static __device__ __forceinline__ bool included(const Rec& x) {
    return x.status_a == FOGNET_OK && x.status_b == FOGNET_OK;
  }
  static __device__ __forceinline__ void merge(Rec& a, const Rec& b) {  // (a's statuses stay)
    int64_t* const aw = &a.n_reps;
    const int64_t* const bw = &b.n_reps;
#pragma unroll
    for (int w = 0; w < kHeadWords - 1; ++w) aw[w] = (int64_t)((uint64_t)aw[w] + (uint64_t)bw[w]);
    moments_merge(a.d_start, b.d_start);
    moments_merge(a.d_service, b.d_service);
    moments_merge(a.d_resp, b.d_resp);
  }
};
constexpr int kRecWords = rec_words<CompareOps>();
static_assert(FOGNET_OK == 0, "the empty record's statuses are its zero words");
static_assert(sizeof(fognet_compare_stats) == 400 && kRecWords == 50, "fognet_compare_stats is 50 words");
static_assert(offsetof(fognet_compare_stats, n_reps) == 8 && offsetof(fognet_compare_stats, trans) == 4 * 8 &&
                  offsetof(fognet_compare_stats, rep_worse) == 22 * 8 &&
                  offsetof(fognet_compare_stats, d_start) == CompareOps::kHeadWords * 8 &&
                  offsetof(fognet_compare_stats, d_resp.min_raw) == (CompareOps::kHeadWords + 2 * kMomWords + 1) * 8,
              "the record's layout (fognet_hip.h): 22 int64 counts from n_reps on, then the moments");

struct CompareArgs {
  int32_t R, T;
  const int32_t *node_a, *node_b;
  const uint8_t *status_a, *status_b;
  const int64_t *start_a, *start_b, *done_a, *done_b;
  const fognet_rep_stats *stats_a, *stats_b;
  int64_t* hist;  // [2][FOGNET_HIST_BINS], added to (nullable)
};

// one task of both replays
struct PairRow {
  int64_t start_a, done_a, start_b, done_b;
  int32_t node_a, node_b;
  uint32_t status_a, status_b;
};

// A lane's counts: at most ceil(T / kPassThreads) tasks each, a wavefront's total below T < 2^31.
enum { kCMoved = 0, kCTrans = 1, kCBoth = 10, kCOnlyA, kCOnlyB, kCNeither, kCBetter, kCEqual, kCWorse, kCounts };
struct Counts {
  uint32_t c[kCounts];
  __device__ __forceinline__ Counts shfl_xor(int m) const {
    Counts o;
#pragma unroll
    for (int k = 0; k < kCounts; ++k) o.c[k] = (uint32_t)__shfl_xor((int)c[k], m, kWave);
    return o;
  }
  __device__ __forceinline__ void merge(const Counts& b) {
#pragma unroll
    for (int k = 0; k < kCounts; ++k) c[k] += b.c[k];
  }
};
static_assert(offsetof(fognet_compare_stats, n_moved) == (3 + kCMoved) * 8 &&
                  offsetof(fognet_compare_stats, n_done_both) == (3 + kCBoth) * 8 &&
                  offsetof(fognet_compare_stats, n_worse) == (3 + kCWorse) * 8,
              "Counts is the record's words from n_moved to n_worse, in order");

// index of a task status in trans (fognet_hip.h); 3: none
__device__ __forceinline__ uint32_t status_index(uint32_t s) { return s == 5u ? 0u : s == 4u ? 1u : s == 9u ? 2u : 3u; }

__device__ __forceinline__ bool compared(int32_t s) { return s == FOGNET_OK || s == FOGNET_REF_ABORTED; }

// (four waves per SIMD: at most 128 VGPRs, which the three signals, the counts and two rows in flight fit without a spill)
__global__ __launch_bounds__(kPassThreads, 4) void compare_kernel(CompareArgs P, fognet_compare_stats* out) {
  __shared__ uint64_t s_rec[kRecWords];
  __shared__ uint32_t s_hist[2 * FOGNET_HIST_BINS];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1);
  const int32_t st_a = P.stats_a[r].status, st_b = P.stats_b[r].status;
  const bool both = compared(st_a) && compared(st_b);
  const bool hist = P.hist != nullptr && st_a == FOGNET_OK && st_b == FOGNET_OK;  // the job rule
  for (int w = tid; w < kRecWords; w += kPassThreads) s_rec[w] = empty_word<CompareOps>(w);
  for (int b = tid; b < 2 * FOGNET_HIST_BINS; b += kPassThreads) s_hist[b] = 0u;
  __syncthreads();
  fognet_compare_stats* const acc = reinterpret_cast<fognet_compare_stats*>(s_rec);
  int n = 0;
  if (both) {  // (wave-uniform; of a replication that is not compared no row is read)
    const int64_t na = P.stats_a[r].n_tasks, nb = P.stats_b[r].n_tasks, n64 = na < nb ? na : nb;
    n = (int)(n64 < 0 ? 0 : n64 > P.T ? P.T : n64);
    Sig d_start = sig_identity(), d_service = sig_identity(), d_resp = sig_identity();
    Counts cnt{};
    auto load = [&](size_t o) {
      return PairRow{P.start_a[o], P.done_a[o], P.start_b[o], P.done_b[o], P.node_a[o], P.node_b[o],
                     (uint32_t)P.status_a[o], (uint32_t)P.status_b[o]};
    };
    stream_rows(P.T, r, n, load, [&](const PairRow& x, int, bool pair) {
      if (!pair) return;
      cnt.c[kCMoved] += x.node_a != x.node_b ? 1u : 0u;
      const uint32_t ia = status_index(x.status_a), ib = status_index(x.status_b);
      const uint32_t cell = ia < 3u && ib < 3u ? ia * 3u + ib : 9u;
#pragma unroll
      for (uint32_t k = 0; k < 9u; ++k) cnt.c[kCTrans + k] += cell == k ? 1u : 0u;
      const bool fa = x.done_a >= 0, fb = x.done_b >= 0;
      cnt.c[kCBoth] += fa && fb ? 1u : 0u;
      cnt.c[kCOnlyA] += fa && !fb ? 1u : 0u;
      cnt.c[kCOnlyB] += !fa && fb ? 1u : 0u;
      cnt.c[kCNeither] += !fa && !fb ? 1u : 0u;
      if (fa && fb) {
        // B minus A, modulo 2^64
        const int64_t ds = (int64_t)((uint64_t)x.start_b - (uint64_t)x.start_a);
        const int64_t dr = (int64_t)((uint64_t)x.done_b - (uint64_t)x.done_a);
        const int64_t dv = (int64_t)((uint64_t)dr - (uint64_t)ds);  // (done_b - start_b) - (done_a - start_a)
        sig_add(d_start, ds);
        sig_add(d_service, dv);
        sig_add(d_resp, dr);
        cnt.c[kCBetter] += dr < 0 ? 1u : 0u;
        cnt.c[kCEqual] += dr == 0 ? 1u : 0u;
        cnt.c[kCWorse] += dr > 0 ? 1u : 0u;
        if (hist && dr != 0) {  // dr = the difference of two ticks >= 0: |dr| < 2^63
          const int64_t mag = dr < 0 ? (int64_t)((uint64_t)0 - (uint64_t)dr) : dr;
          (void)atomicAdd(&s_hist[(dr < 0 ? 0 : FOGNET_HIST_BINS) + hist_bin(mag)], 1u);
        }
      }
    });
    // one butterfly and one commit per wavefront (every lane is active here)
    wave_merge3(d_start, d_service, d_resp, cnt);
    if (lane == 0) {
      uint64_t* const words = s_rec + 3;  // n_moved .. n_worse
#pragma unroll
      for (int k = 0; k < kCounts; ++k) atomic_add(&words[k], cnt.c[k]);
      const uint64_t m = cnt.c[kCBoth];
      commit_sig(&acc->d_start, m, 0u, d_start);
      commit_sig(&acc->d_service, m, 0u, d_service);
      commit_sig(&acc->d_resp, m, 0u, d_resp);
    }
  }
  __syncthreads();
  if (tid == 0) {
    acc->status_a = st_a;
    acc->status_b = st_b;
    if (both) {
      acc->n_reps = 1;
      acc->n_pairs = n;
      // the sign of the signed 128-bit d_resp sum
      const uint64_t lo = acc->d_resp.sum_lo, hi = acc->d_resp.sum_hi;
      const bool neg = (int64_t)hi < 0, zero = (lo | hi) == 0u;
      acc->rep_better = neg ? 1 : 0;
      acc->rep_equal = zero ? 1 : 0;
      acc->rep_worse = !neg && !zero ? 1 : 0;
    }
  }
  __syncthreads();
  uint64_t* const dst = reinterpret_cast<uint64_t*>(out + r);
  for (int w = tid; w < kRecWords; w += kPassThreads) dst[w] = s_rec[w];
  if (hist)
    for (int b = tid; b < 2 * FOGNET_HIST_BINS; b += kPassThreads) atomic_add(&P.hist[b], (uint64_t)s_hist[b]);
}

}  // namespace

hipError_t launch_compare(const CompareIn& in, fognet_compare_stats* out, int64_t* hist, hipStream_t s) {
  if (in.R <= 0) return hipSuccess;
  CompareArgs p{};
  p.R = in.R, p.T = in.T;
  p.node_a = in.a->node, p.status_a = in.a->status, p.start_a = in.a->start_tick, p.done_a = in.a->done_tick;
  p.node_b = in.b->node, p.status_b = in.b->status, p.start_b = in.b->start_tick, p.done_b = in.b->done_tick;
  p.stats_a = in.a->stats, p.stats_b = in.b->stats;
  p.hist = hist;
  hipLaunchKernelGGL(compare_kernel, dim3(in.R), dim3(kPassThreads), 0, s, p, out);
  return hipGetLastError();
}

hipError_t launch_reduce_compare(const fognet_compare_stats* in, int32_t R, fognet_compare_stats* out, hipStream_t s) {
  return launch_reduce<CompareOps>(in, nullptr, R, 1, out, s);
}

}  // namespace fognet
