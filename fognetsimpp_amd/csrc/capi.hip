// capi.hip — host implementation of the libfognet_hip C ABI (include/fognet_hip.h).
// Pure host C++ around the gfx950 kernels; there is no CPU compute path: every
// decision is evaluated on the device, and the library refuses to create a
// context without a gfx950 GPU.
#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "internal.h"

struct fognet_ctx {
  int device = -1;
  int cus = 256;  // compute units (generated-mode launch size)
  hipStream_t stream = nullptr;  // private stream for the host-buffer entry points
  fognet::RingWord* ring = nullptr;
  size_t ring_bytes = 0;
  // partial job records of a multi-block reduction (fognet_reduce_stats_dev)
  void* red = nullptr;
  size_t red_bytes = 0;
  // scratch for the v2 scalar decision
  void* scratch = nullptr;
  size_t scratch_bytes = 0;
  // mapped, coherent host memory for fognet_decide / fognet_decide_window:
  // inputs the kernel reads and results it writes without copies
  void* host_stage = nullptr;
  void* host_stage_dev = nullptr;
  size_t host_stage_bytes = 0;
  // EXT_HIER path choice (fognet_hier_path_stats): the hand-over count of the last region pass,
  // copied back into pinned memory on the launch stream and read once its event has passed
  // One measurement at a time: the count is paired with the shape and stream of the
  // launch it measured, and its decision applies only to later launches of that same shape and stream.
  struct HierShape {
    int32_t R, T, N;
    void* stream;
    bool operator==(const HierShape& o) const { return R == o.R && T == o.T && N == o.N && stream == o.stream; }
  };
  int32_t* hier_host = nullptr;  // [0] handed-over replications of the measured launch
  hipEvent_t hier_ev = nullptr;
  bool hier_pending = false;
  HierShape hier_pend_shape{};  // the launch being measured
  bool hier_seq = false;  // the last measured region pass (of hier_seq_shape) handed most replications over
  HierShape hier_seq_shape{};
  int hier_seq_runs = 0;  // launches sent straight to the sequential replay since that measurement
  int64_t hier_region_launches = 0, hier_seq_launches = 0;
  std::string err;
};

namespace {

constexpr int kDefaultRing = 2048;
// Workspace slots of the wide kernel when it replays the replications the
// register kernel hands over (at most one wave per SIMD of the chip).
constexpr int32_t kWideFallbackSlots = 1024;

using fognet::align256;

int fail(fognet_ctx* c, int rc, const std::string& msg) {
  if (c) c->err = msg;
  return rc;
}

int hip_fail(fognet_ctx* c, hipError_t e, const char* what) {
  return fail(c, FOGNET_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

int ensure(fognet_ctx* c, void** p, size_t* have, size_t want, const char* what) {
  if (*have >= want) return FOGNET_OK;
  if (*p) {
    (void)hipFree(*p);
    *p = nullptr;
    *have = 0;
  }
  hipError_t e = hipMalloc(p, want);
  if (e != hipSuccess) {
    *p = nullptr;
    return fail(c, e == hipErrorOutOfMemory ? FOGNET_ERR_OOM : FOGNET_ERR_DEVICE,
                std::string("hipMalloc ") + what + ": " + hipGetErrorString(e));
  }
  *have = want;
  return FOGNET_OK;
}

int ensure_host(fognet_ctx* c, size_t want) {
  if (c->host_stage_bytes >= want) return FOGNET_OK;
  if (c->host_stage) {
    (void)hipHostFree(c->host_stage);
    c->host_stage = c->host_stage_dev = nullptr;
    c->host_stage_bytes = 0;
  }
  want = want < 4096 ? 4096 : want;
  hipError_t e = hipHostMalloc(&c->host_stage, want, hipHostMallocMapped | hipHostMallocCoherent);
  if (e == hipSuccess) e = hipHostGetDevicePointer(&c->host_stage_dev, c->host_stage, 0);
  if (e != hipSuccess) {
    if (c->host_stage) (void)hipHostFree(c->host_stage);
    c->host_stage = c->host_stage_dev = nullptr;
    return fail(c, FOGNET_ERR_OOM, std::string("hipHostMalloc decide stage: ") + hipGetErrorString(e));
  }
  c->host_stage_bytes = want;
  return FOGNET_OK;
}

int set_device(fognet_ctx* c) {
  hipError_t e = hipSetDevice(c->device);
  return e == hipSuccess ? FOGNET_OK : hip_fail(c, e, "hipSetDevice");
}

// The job reduction of keyed records, recs [R][K] into out [K] (fognet_reduce_{node,queue,window,user}_stats_dev):
// `negative` and `what` are the entry point's own texts.
template <class Rec>
int reduce_keyed(fognet_ctx* c, const Rec* recs, const fognet_rep_stats* stats, int32_t R, int32_t K, Rec* out,
                 void* stream, hipError_t (*launch)(const Rec*, const fognet_rep_stats*, int32_t, int32_t, Rec*, hipStream_t),
                 const char* negative, const char* what) {
  if (!c) return FOGNET_ERR_ARG;
  if (R < 0 || K < 0) return fail(c, FOGNET_ERR_ARG, negative);
  if (K == 0) return FOGNET_OK;
  if (!out || (R > 0 && (!recs || !stats))) return fail(c, FOGNET_ERR_ARG, "null pointer");
  const int rc = set_device(c);
  if (rc) return rc;
  const hipError_t e = launch(recs, stats, R, K, out, (hipStream_t)stream);
  return e == hipSuccess ? FOGNET_OK : hip_fail(c, e, what);
}

// Validates a batch descriptor; fills the kernel argument block except pointers to outputs.
// generated: fognet_run_generated_dev (no trace or node-parameter arrays)
int prepare(fognet_ctx* c, const fognet_batch_in* in, fognet::ReplayArgs* a, bool generated = false) {
  if (!in) return fail(c, FOGNET_ERR_ARG, "null batch");
  if (in->R < 0 || in->T < 0 || in->N < 0) return fail(c, FOGNET_ERR_ARG, "negative R/T/N");
  if (in->N == 0) return fail(c, FOGNET_ERR_NO_NODES, "N == 0 (BrokerBaseApp3.cc:268 reads brokers[0])");
  if (in->N > fognet::kWideBigMaxNodes)
    return fail(c, FOGNET_ERR_UNSUPPORTED, "N > 1048576 (the wide replay kernel's active-group mask: 16 words per lane)");
  if (in->policy == FOGNET_POLICY_EXT_HIER && in->N > fognet::kWideMaxNodes)
    return fail(c, FOGNET_ERR_UNSUPPORTED, "EXT_HIER with N > 65536 (more than 64 regions of 1,024 nodes)");
  if (in->policy != FOGNET_POLICY_REF_V3 && in->policy != FOGNET_POLICY_EXT_LAT && in->policy != FOGNET_POLICY_EXT_HIER)
    return fail(c, FOGNET_ERR_UNSUPPORTED, "unknown policy");
  if (in->policy == FOGNET_POLICY_EXT_HIER) {
    if (!generated && in->R > 0 && in->T > 0 && !in->region) return fail(c, FOGNET_ERR_ARG, "EXT_HIER needs the region array");
    if (in->hier_threshold_s < 0 || in->hier_up_tick < 0 || in->hier_up_tick >= ((int64_t)1 << 50))
      return fail(c, FOGNET_ERR_ARG, "EXT_HIER: threshold >= 0 and 0 <= up latency < 2^50 ticks");
  }
  if ((in->p_busy_w == nullptr) != (in->p_idle_w == nullptr))
    return fail(c, FOGNET_ERR_ARG, "p_busy_w and p_idle_w must both be given or both be null");
  if (in->down_tick && in->p_busy_w)
    return fail(c, FOGNET_ERR_UNSUPPORTED, "the power model assumes nodes that stay up (down_tick with p_busy_w)");
  if (in->node_stride != 0 && in->node_stride != in->N)
    return fail(c, FOGNET_ERR_ARG, "node_stride must be 0 or N");
  if (in->flags & ~FOGNET_FLAG_REF_ABORT) return fail(c, FOGNET_ERR_ARG, "unknown flags");
  int q = in->ring_capacity ? in->ring_capacity : kDefaultRing;
  if (q < 2 || (q & (q - 1)) != 0 || q > (1 << 15)) return fail(c, FOGNET_ERR_ARG, "ring_capacity must be a power of two in [2, 2^15]");
  int qlog = 0;
  while ((1 << qlog) < q) ++qlog;
  if (!generated && in->R > 0 && in->T > 0 && (!in->arrive_tick || !in->req_mips))
    return fail(c, FOGNET_ERR_ARG, "null trace arrays");
  if (!generated && in->R > 0 && (!in->mips || !in->dl_tick || !in->ul_tick || !in->init_adv_tick))
    return fail(c, FOGNET_ERR_ARG, "null node parameter arrays");
  memset(a, 0, sizeof *a);
  a->R = in->R;
  a->T = in->T;
  a->N = in->N;
  a->node_stride = in->node_stride;
  a->q_log2 = qlog;
  // busy (a sum of at most Q pending service times) must stay below 2^24 s
  // (the replay kernel's 32-bit view key is busy << 8 | node), and service
  // times stay below 2^16 s (18.2 h) so its run scan cannot overflow
  // (replay.hip, kMaxTick).  Q = 1024: at most 16383 s per task.
  const uint64_t by_ring = 0xFFFFFFull / (uint64_t)q;
  a->max_s = (uint32_t)(by_ring < 0xFFFFull ? by_ring : 0xFFFFull);
  a->arrive = in->arrive_tick;
  a->req = in->req_mips;
  a->mips = in->mips;
  a->dl = in->dl_tick;
  a->ul = in->ul_tick;
  a->init = in->init_adv_tick;
  a->policy = in->policy;
  a->p_busy = in->p_busy_w;
  a->p_idle = in->p_idle_w;
  a->down = in->down_tick;
  a->ref_abort = (in->flags & FOGNET_FLAG_REF_ABORT) ? 1 : 0;
  if (in->policy == FOGNET_POLICY_EXT_HIER) {
    a->region = in->region;
    a->hier_up = in->hier_up_tick;
    a->hier_thr = in->hier_threshold_s;
  }
  return FOGNET_OK;
}

// The environment switches, each read once in every call (the parity tests flip them between calls to
// check that each path ran).  FOGNET_REPLAY_KERNEL=wide: the wide replay kernel (replay_wide.hip),
// which N > 256 takes anyway, for any N.
// FOGNET_REPLAY_STATS=inloop: the statistics of a fused replay come from in-loop accumulators
// (replay_inl_kernel, 3 waves/SIMD) instead of the epilogue's re-read of the outputs (replay_kernel,
// 4 waves/SIMD); the records are identical (the parity tests run both).  Not the default: at C3 (4,096
// replications, all resident at 4 waves/SIMD) it measured 20.9 ms/launch against 14.1 ms, the fourth
// wave per SIMD being worth more than the re-read.
// FOGNET_HIER_REGIONS=0: EXT_HIER replays run on the sequential wide kernel only; =only: the region pass
// without the sequential hand-over (a replication it cannot finish keeps an internal status).
// FOGNET_HIER_RESUME=0: an escalated replication is replayed by the sequential kernel from the start (and
// with FOGNET_HIER_REGIONS unset hier_skip_regions chooses between the two paths); default: it continues
// from its first escalated publish (replay_region.hip)
bool env_is(const char* name, const char* value) {
  const char* f = getenv(name);
  return f != nullptr && strcmp(f, value) == 0;
}

bool use_wide(int32_t N) {
  return N > fognet::kWave * fognet::kMaxNodesPerLane || env_is("FOGNET_REPLAY_KERNEL", "wide");
}

// Workspace slots of the hand-over launch: the wide kernel walks the hand-over
// list with a grid stride, so fewer slots than handed-over replications are
// still exact.  At most kWideFallbackSlots, and no more than fit in the ring
// workspace the register kernel needs anyway (floor 1), so a replay that never
// hands over allocates nothing extra.
int32_t fallback_slots(int32_t R, int32_t T, int32_t N, size_t ring_bytes, bool gen, int policy) {
  int32_t slots = R < kWideFallbackSlots ? R : kWideFallbackSlots;
  const size_t per = fognet::replay_wide_workspace_bytes(1, T, N, gen, policy);
  const size_t fit = per ? ring_bytes / per : (size_t)slots;
  if ((size_t)slots > fit) slots = fit < 1 ? 1 : (int32_t)fit;
  return slots;
}

// Sizes a layout of workspace.h (parts: the walk over its part list, returning the total), grows
// the context's one workspace allocation to hold it and sets the parts' pointers.
template <class Parts>
int carve(fognet_ctx* c, const char* what, Parts parts) {
  fognet::WsCursor size{nullptr};
  const int rc = ensure(c, (void**)&c->ring, &c->ring_bytes, parts(size), what);
  fognet::WsCursor bind{reinterpret_cast<unsigned char*>(c->ring)};
  if (rc == FOGNET_OK) parts(bind);
  return rc;
}

// The wide kernel on its own: workgroup r replays replication r.
int run_wide(fognet_ctx* c, const fognet::ReplayArgs& a, hipStream_t s) {
  const size_t ws = fognet::replay_wide_workspace_bytes(a.R, a.T, a.N, a.gen_on != 0, a.policy);
  const int rc = ensure(c, (void**)&c->ring, &c->ring_bytes, ws, "wide replay workspace");
  if (rc) return rc;
  const hipError_t e = fognet::launch_replay_wide(a, c->ring, a.R, s);
  return e == hipSuccess ? FOGNET_OK : hip_fail(c, e, "wide replay launch");
}

// Automatic EXT_HIER path choice (restart mode, FOGNET_HIER_REGIONS unset): after a region pass that
// handed most replications over, this many launches go straight to the sequential replay before a
// region pass measures again
constexpr int kHierReprobe = 15;

// Takes in the last region pass's hand-over count, if it has reached the host (never waited for),
// and says whether this launch skips the region pass.
bool hier_skip_regions(fognet_ctx* c, const fognet_ctx::HierShape& shape) {
  if (c->hier_pending && hipEventQuery(c->hier_ev) == hipSuccess) {
    c->hier_pending = false;
    c->hier_seq = 2 * (int64_t)c->hier_host[0] > (int64_t)c->hier_pend_shape.R;
    c->hier_seq_shape = c->hier_pend_shape;
    c->hier_seq_runs = 0;
  }
  if (c->hier_seq && !(c->hier_seq_shape == shape)) c->hier_seq = false;  // another job: measure it
  if (c->hier_seq && c->hier_seq_runs < kHierReprobe) {
    ++c->hier_seq_runs;  // most replications escalated: the region pass would only be replayed again
    return true;
  }
  c->hier_seq = false;  // (measure again)
  return false;
}

// The hand-over count of the region pass just launched back to the host, asynchronously.  While a
// measurement is in flight, later launches are not measured: its pinned slot and event stay paired
// with the launch that issued them.
int hier_measure(fognet_ctx* c, const fognet_ctx::HierShape& shape, const int32_t* count, hipStream_t s) {
  if (c->hier_pending) return FOGNET_OK;
  if (!c->hier_host && hipHostMalloc((void**)&c->hier_host, sizeof(int32_t), hipHostMallocDefault) != hipSuccess)
    c->hier_host = nullptr;
  if (!c->hier_ev && hipEventCreateWithFlags(&c->hier_ev, hipEventDisableTiming) != hipSuccess) c->hier_ev = nullptr;
  if (!c->hier_host || !c->hier_ev) return FOGNET_OK;
  c->hier_pend_shape = shape;
  hipError_t e = hipMemcpyAsync(c->hier_host, count, sizeof(int32_t), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipEventRecord(c->hier_ev, s);
  if (e != hipSuccess) return hip_fail(c, e, "hand-over count copy");
  c->hier_pending = true;
  return FOGNET_OK;
}

// EXT_HIER by region: one wavefront per (replication, region) while no region escalates (replay_region.hip),
// the statistics pass, then the sequential wide kernel for the replications some region handed back, with one
// workspace slot each up to kWideFallbackSlots (an escalation-heavy job replays its hand-overs side by side, as
// the sequential-only path does).  only: FOGNET_HIER_REGIONS=only; measure (nullable): for the automatic choice
int run_regions(fognet_ctx* c, fognet::ReplayArgs& a, int32_t B, bool resume, bool only,
                const fognet_ctx::HierShape* measure, hipStream_t s) {
  const int32_t slots = a.R < kWideFallbackSlots ? a.R : kWideFallbackSlots;
  const size_t fb = fognet::replay_wide_workspace_bytes(slots, a.T, a.N, false, a.policy);
  fognet::ReplayWs h;
  fognet::RegionWs w;
  const int rc = carve(c, "region replay workspace", [&](fognet::WsCursor& v) {
    return fognet::region_ws(h, w, a.R, a.T, a.N, B, fb, resume, v);
  });
  if (rc) return rc;
  w.pass = 1;
  w.B = B;
  a.wide_count = h.count;
  a.wide_list = only ? nullptr : h.list;
  hipError_t e = hipMemsetAsync(a.wide_count, 0, sizeof(int32_t), s);
  if (e != hipSuccess) return hip_fail(c, e, "hand-over counter");
  e = fognet::launch_replay_region(a, w, resume && !only, s);
  if (e != hipSuccess) return hip_fail(c, e, "region replay launch");
  if (only) return FOGNET_OK;
  e = fognet::launch_replay_wide(a, h.body, slots, s, resume ? &w : nullptr);
  if (e != hipSuccess) return hip_fail(c, e, "wide hand-over launch");
  return measure ? hier_measure(c, *measure, a.wide_count, s) : FOGNET_OK;
}

// The register kernel (replay.hip), then the wide kernel for the replications it handed over
// (usually none: every workgroup leaves at once).
int run_register(fognet_ctx* c, fognet::ReplayArgs& a, bool stats_only, hipStream_t s) {
  const size_t ring_bytes = (size_t)a.R * (size_t)a.N * ((size_t)1 << a.q_log2) * sizeof(fognet::RingWord);
  const int32_t slots = fallback_slots(a.R, a.T, a.N, ring_bytes, false, a.policy);
  const size_t fb_bytes = fognet::replay_wide_workspace_bytes(slots, a.T, a.N, false, a.policy);
  const bool scratch_out = stats_only && !a.inloop;  // the fused statistics epilogue reads the outputs back
  fognet::ReplayWs w;
  const int rc = carve(c, "ring workspace", [&](fognet::WsCursor& v) {
    return fognet::register_ws(w, a.R, ring_bytes, fb_bytes, scratch_out ? (size_t)a.R * (size_t)a.T : 0, v);
  });
  if (rc) return rc;
  a.wide_count = w.count;
  a.wide_list = w.list;
  a.ring = reinterpret_cast<fognet::RingWord*>(w.body);
  if (scratch_out) {
    a.scratch_out = 1;
    a.out_node = w.out_node;
    a.out_status = w.out_status;
    a.out_start = w.out_start;
    a.out_done = w.out_done;
  }
  hipError_t e = hipMemsetAsync(a.wide_count, 0, sizeof(int32_t), s);
  if (e != hipSuccess) return hip_fail(c, e, "hand-over counter");
  if (!a.inloop) {  // replay_kernel's progress board: every slot empty
    a.board = w.board;
    e = hipMemsetAsync(a.board, 0xFF, fognet::kBoardWords * sizeof(uint32_t), s);
    if (e != hipSuccess) return hip_fail(c, e, "progress board");
  }
  e = fognet::launch_replay(a, s);
  if (e != hipSuccess) return hip_fail(c, e, "replay launch");
  // The wide kernel accumulates its statistics inline; in a replay-only call the statistics stage that
  // follows recomputes them for every replication from the per-task outputs, so the hand-over must not
  // add its histogram and energy as well
  fognet::ReplayArgs hw = a;
  if (!a.fuse_stats) {
    hw.hist = nullptr;
    hw.out_energy = nullptr;
  }
  e = fognet::launch_replay_wide(hw, w.body, slots, s);
  return e == hipSuccess ? FOGNET_OK : hip_fail(c, e, "wide hand-over launch");
}

int run_rep_stats(fognet_ctx* c, const fognet::ReplayArgs& a, hipStream_t s) {
  const hipError_t e = fognet::launch_rep_stats(a, s);
  return e == hipSuccess ? FOGNET_OK : hip_fail(c, e, "stats launch");
}

// which: 1 replay, 2 statistics, 3 both (fused).  Validation and routing only.
int stage(fognet_ctx* c, const fognet_batch_in* in, fognet_batch_out* out, void* stream, int which) {
  if (!c || !out) return FOGNET_ERR_ARG;
  fognet::ReplayArgs a;
  int rc = prepare(c, in, &a);
  if (rc) return rc;
  if (!out->stats) return fail(c, FOGNET_ERR_ARG, "stats output is required (per-replication status)");
  const int n_null = !out->node + !out->status + !out->start_tick + !out->done_tick;
  if (n_null != 0 && n_null != 4)
    return fail(c, FOGNET_ERR_ARG, "per-task outputs: give all four arrays, or none (statistics only)");
  const bool stats_only = n_null == 4 && a.T > 0;
  if (stats_only && which != 3)
    return fail(c, FOGNET_ERR_UNSUPPORTED, "statistics-only replays run through fognet_run_batch_dev");
  if (stats_only && out->escalated)
    return fail(c, FOGNET_ERR_ARG, "escalated is a per-task output: a statistics-only out has none");
  if (a.R == 0) return FOGNET_OK;
  rc = set_device(c);
  if (rc) return rc;
  a.out_node = out->node;
  a.out_status = out->status;
  a.out_start = out->start_tick;
  a.out_done = out->done_tick;
  a.out_stats = out->stats;
  a.out_energy = out->node_energy_j;
  a.hist = out->hist;
  if (a.out_energy && !a.p_busy) return fail(c, FOGNET_ERR_ARG, "node_energy_j needs the power model (p_busy_w/p_idle_w)");
  const hipStream_t s = (hipStream_t)stream;
  // the escalation flags: written by the EXT_HIER replay paths; no other policy escalates
  if (a.policy == FOGNET_POLICY_EXT_HIER) {
    a.out_esc = out->escalated;
  } else if (out->escalated && (which & 1) && a.T > 0) {
    const hipError_t e = hipMemsetAsync(out->escalated, 0, (size_t)a.R * (size_t)a.T, s);
    if (e != hipSuccess) return hip_fail(c, e, "escalated clear");
  }
  if (use_wide(a.N) || a.down || a.policy == FOGNET_POLICY_EXT_HIER) {  // (regions: the wide kernel's groups)
    // crashes are only modelled by the wide kernel; it accumulates the statistics while it replays, so the
    // statistics-only stage has nothing left to do
    if (!(which & 1)) return FOGNET_OK;
    a.no_task_out = stats_only ? 1 : 0;
    const int32_t B = (a.N + FOGNET_HIER_REGION_NODES - 1) / FOGNET_HIER_REGION_NODES;
    const bool hier_split = a.policy == FOGNET_POLICY_EXT_HIER && !a.down && !stats_only && a.T > 0 && B >= 2;
    const char* const mode = getenv("FOGNET_HIER_REGIONS");
    bool regions = hier_split && (mode == nullptr || strcmp(mode, "0") != 0);
    // resume: the region pass is never wasted and is always taken
    const bool resume = regions && !env_is("FOGNET_HIER_RESUME", "0");
    const bool automatic = regions && mode == nullptr && !resume;
    const fognet_ctx::HierShape shape{a.R, a.T, a.N, stream};
    if (automatic && hier_skip_regions(c, shape)) regions = false;
    if (hier_split) ++(regions ? c->hier_region_launches : c->hier_seq_launches);
    if (!regions) return run_wide(c, a, s);
    const bool only = mode != nullptr && strcmp(mode, "only") == 0;
    return run_regions(c, a, B, resume, only, automatic ? &shape : nullptr, s);
  }
  // both stages: the replay kernel runs the statistics pass as its epilogue
  a.fuse_stats = which == 3 ? 1 : 0;
  if (a.fuse_stats) which = 1;
  // statistics accumulated in the loop (replay_inl_kernel) where the node tails hold exact totals
  a.inloop = a.fuse_stats && (uint64_t)a.T * (uint64_t)a.max_s < (1ull << 32) && env_is("FOGNET_REPLAY_STATS", "inloop");
  if (a.inloop) a.no_task_out = stats_only ? 1 : 0;
  if (which & 1) rc = run_register(c, a, stats_only, s);
  if (rc == FOGNET_OK && (which & 2)) rc = run_rep_stats(c, a, s);
  return rc;
}

}  // namespace

extern "C" {

int fognet_abi_version(void) { return FOGNET_ABI_VERSION; }

const char* fognet_status_string(int s) {
  switch (s) {
    case FOGNET_OK: return "ok";
    case FOGNET_ERR_ARG: return "invalid argument";
    case FOGNET_ERR_NO_NODES: return "no fog nodes registered";
    case FOGNET_ERR_DIV0: return "advertised MIPS of node 0 is zero";
    case FOGNET_ERR_STATE: return "self-message already scheduled";
    case FOGNET_ERR_DEVICE: return "HIP device error";
    case FOGNET_ERR_OOM: return "out of device memory";
    case FOGNET_ERR_CAPACITY: return "capacity exceeded";
    case FOGNET_ERR_UNSUPPORTED: return "unsupported configuration";
    case FOGNET_REF_ABORTED: return "the reference run aborts (queueTime simtime overflow)";
    case FOGNET_ERR_INTERNAL: return "internal invariant check failed";
  }
  return "unknown status";
}

int fognet_create(fognet_ctx** out, int hip_device) {
  if (!out) return FOGNET_ERR_ARG;
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) return FOGNET_ERR_DEVICE;
  if (hip_device < 0 || hip_device >= n) return FOGNET_ERR_ARG;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, hip_device) != hipSuccess) return FOGNET_ERR_DEVICE;
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return FOGNET_ERR_DEVICE;
  fognet_ctx* c = new (std::nothrow) fognet_ctx();
  if (!c) return FOGNET_ERR_OOM;
  c->device = hip_device;
  if (prop.multiProcessorCount > 0) c->cus = prop.multiProcessorCount;
  if (hipSetDevice(hip_device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return FOGNET_ERR_DEVICE;
  }
  *out = c;
  return FOGNET_OK;
}

void fognet_destroy(fognet_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->ring) (void)hipFree(c->ring);
  if (c->scratch) (void)hipFree(c->scratch);
  if (c->red) (void)hipFree(c->red);
  if (c->host_stage) (void)hipHostFree(c->host_stage);
  if (c->hier_ev) (void)hipEventSynchronize(c->hier_ev), (void)hipEventDestroy(c->hier_ev);
  if (c->hier_host) (void)hipHostFree(c->hier_host);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

int fognet_hier_path_stats(const fognet_ctx* c, int64_t* region_launches, int64_t* sequential_launches) {
  if (!c) return FOGNET_ERR_ARG;
  if (region_launches) *region_launches = c->hier_region_launches;
  if (sequential_launches) *sequential_launches = c->hier_seq_launches;
  return FOGNET_OK;
}

const char* fognet_last_error(const fognet_ctx* c) { return c ? c->err.c_str() : "null context"; }

int fognet_sync(fognet_ctx* c) {
  if (!c) return FOGNET_ERR_ARG;
  int rc = set_device(c);
  if (rc) return rc;
  hipError_t e = hipDeviceSynchronize();
  return e == hipSuccess ? FOGNET_OK : hip_fail(c, e, "hipDeviceSynchronize");
}

int fognet_decide_batch_dev(fognet_ctx* c, int policy, int64_t m, int32_t n, const double* adv_busy,
                            const int32_t* adv_mips, const int32_t* req, int32_t* out_node, int32_t* out_status,
                            void* stream) {
  if (!c) return FOGNET_ERR_ARG;
  if (policy != FOGNET_POLICY_REF_V3) return fail(c, FOGNET_ERR_UNSUPPORTED, "unknown policy");
  if (m < 0) return fail(c, FOGNET_ERR_ARG, "m < 0");
  if (m > 0 && (!out_node || (n > 0 && (!adv_busy || !adv_mips || !req))))
    return fail(c, FOGNET_ERR_ARG, "null pointer");
  int rc = set_device(c);
  if (rc) return rc;
  hipError_t e = fognet::launch_decide(m, n, n, adv_busy, adv_mips, req, out_node, out_status, (hipStream_t)stream);
  return e == hipSuccess ? FOGNET_OK : hip_fail(c, e, "decide launch");
}

int fognet_decide(fognet_ctx* c, int policy, int32_t n, const double* adv_busy, const int32_t* adv_mips,
                  int32_t req_mips, int32_t* out_node) {
  if (!c || !out_node) return FOGNET_ERR_ARG;
  if (policy != FOGNET_POLICY_REF_V3) return fail(c, FOGNET_ERR_UNSUPPORTED, "fognet_decide: policy REF_V3 only");
  if (n <= 0) return fail(c, FOGNET_ERR_NO_NODES, "n <= 0 (BrokerBaseApp3.cc:268 reads brokers[0])");
  if (!adv_busy || !adv_mips) return fail(c, FOGNET_ERR_ARG, "null view");
  int rc = set_device(c);
  if (rc) return rc;
  // result words at the stage's start; a view too large for the kernel arguments follows them and is
  // moved to device scratch by one DMA copy (the kernel would read it over the link at one wave's pace)
  const size_t far = n > fognet::kDecideArgNodes ? (size_t)n * sizeof(double) : 0;
  rc = ensure_host(c, 256 + far);
  if (rc) return rc;
  if (far) {
    rc = ensure(c, &c->scratch, &c->scratch_bytes, far, "decide scratch");
    if (rc) return rc;
  }
  fognet::DecideArgs a;
  a.n = n;
  a.mips0 = adv_mips[0];  // the policy reads brokers[0]->getMips() only (BrokerBaseApp3.cc:268,273)
  a.req = req_mips;
  a.pad = 0;
  unsigned char* const h = static_cast<unsigned char*>(c->host_stage);
  unsigned char* const d = static_cast<unsigned char*>(c->host_stage_dev);
  if (far) memcpy(h + 256, adv_busy, far);
  else memcpy(a.busy, adv_busy, (size_t)n * sizeof(double));
  volatile int32_t* res = reinterpret_cast<volatile int32_t*>(h);
  res[0] = -1;
  res[1] = FOGNET_ERR_DEVICE;
  hipError_t e = hipSuccess;
  if (far && (e = hipMemcpyAsync(c->scratch, h + 256, far, hipMemcpyHostToDevice, c->stream)) != hipSuccess)
    return hip_fail(c, e, "decide copy-in");
  e = fognet::launch_decide_args(a, static_cast<const double*>(c->scratch), reinterpret_cast<int32_t*>(d), c->stream);
  if (e != hipSuccess) return hip_fail(c, e, "decide launch");
  if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return hip_fail(c, e, "decide sync");
  if (res[1] != FOGNET_OK) return fail(c, res[1], fognet_status_string(res[1]));
  *out_node = res[0];
  return FOGNET_OK;
}

int fognet_decide_window(fognet_ctx* c, int policy, int32_t n, const double* adv_busy, const int32_t* adv_mips,
                         int32_t m, const int32_t* req_mips, int32_t* out_node) {
  if (!c || m < 0 || (m > 0 && (!out_node || !req_mips))) return fail(c, FOGNET_ERR_ARG, "decide_window: bad argument");
  if (policy != FOGNET_POLICY_REF_V3) return fail(c, FOGNET_ERR_UNSUPPORTED, "decide_window: policy REF_V3 only");
  if (m == 0) return FOGNET_OK;
  if (n <= 0) return fail(c, FOGNET_ERR_NO_NODES, "n <= 0 (BrokerBaseApp3.cc:268 reads brokers[0])");
  if (!adv_busy || !adv_mips) return fail(c, FOGNET_ERR_ARG, "null view");
  int rc = set_device(c);
  if (rc) return rc;
  // stage: [node m][status m][mips0][req m][busy n], 256-B aligned parts
  const size_t o_st = align256((size_t)m * 4), o_m0 = o_st + align256((size_t)m * 4), o_rq = o_m0 + 256;
  const size_t o_b = o_rq + align256((size_t)m * 4), total = o_b + (size_t)n * sizeof(double);
  rc = ensure_host(c, total);
  if (rc) return rc;
  unsigned char* const h = static_cast<unsigned char*>(c->host_stage);
  unsigned char* const d = static_cast<unsigned char*>(c->host_stage_dev);
  memcpy(h + o_m0, adv_mips, sizeof(int32_t));
  memcpy(h + o_rq, req_mips, (size_t)m * 4);
  memcpy(h + o_b, adv_busy, (size_t)n * sizeof(double));
  const double* view = reinterpret_cast<const double*>(d + o_b);  // small views: read in place over the link
  hipError_t e = hipSuccess;
  if (n > fognet::kDecideArgNodes) {
    rc = ensure(c, &c->scratch, &c->scratch_bytes, (size_t)n * sizeof(double), "decide scratch");
    if (rc) return rc;
    if ((e = hipMemcpyAsync(c->scratch, h + o_b, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream)) !=
        hipSuccess)
      return hip_fail(c, e, "decide_window copy-in");
    view = static_cast<const double*>(c->scratch);
  }
  e = fognet::launch_decide(m, n, 0, view,
                                       reinterpret_cast<const int32_t*>(d + o_m0), reinterpret_cast<const int32_t*>(d + o_rq),
                                       reinterpret_cast<int32_t*>(d), reinterpret_cast<int32_t*>(d + o_st), c->stream);
  if (e != hipSuccess) return hip_fail(c, e, "decide_window launch");
  if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return hip_fail(c, e, "decide_window sync");
  memcpy(out_node, h, (size_t)m * 4);
  const int32_t* st = reinterpret_cast<const int32_t*>(h + o_st);
  for (int32_t i = 0; i < m; ++i)
    if (st[i] != FOGNET_OK) {
      char buf[96];
      snprintf(buf, sizeof buf, "request %d: %s", i, fognet_status_string(st[i]));
      return fail(c, st[i], buf);
    }
  return FOGNET_OK;
}

int fognet_decide_v2_batch_dev(fognet_ctx* c, int64_t m, int32_t n, const int32_t* adv_mips, const int32_t* local_mips,
                               const int32_t* req, int32_t* out_node, int32_t* out_action, void* stream) {
  if (!c) return FOGNET_ERR_ARG;
  if (m < 0 || n < 0) return fail(c, FOGNET_ERR_ARG, "m < 0 or n < 0");
  if (m > 0 && (!out_node || !out_action || !local_mips || !req || (n > 0 && !adv_mips)))
    return fail(c, FOGNET_ERR_ARG, "null pointer");
  int rc = set_device(c);
  if (rc) return rc;
  hipError_t e = fognet::launch_decide_v2(m, n, adv_mips, local_mips, req, out_node, out_action, (hipStream_t)stream);
  return e == hipSuccess ? FOGNET_OK : hip_fail(c, e, "decide_v2 launch");
}

int fognet_decide_v2(fognet_ctx* c, int32_t n, const int32_t* adv_mips, int32_t local_mips, int32_t req_mips,
                     int32_t* out_node, int32_t* out_action) {
  if (!c || !out_node || !out_action) return FOGNET_ERR_ARG;
  if (n < 0) return fail(c, FOGNET_ERR_ARG, "n < 0");
  if (n > 0 && !adv_mips) return fail(c, FOGNET_ERR_ARG, "null view");
  int rc = set_device(c);
  if (rc) return rc;
  const size_t nm = (size_t)n * sizeof(int32_t);
  const size_t off_s = (nm + 255) & ~(size_t)255, off_o = off_s + 256, total = off_o + 256;
  rc = ensure(c, &c->scratch, &c->scratch_bytes, total, "decide scratch");
  if (rc) return rc;
  char* s = (char*)c->scratch;
  const int32_t scal[2] = {local_mips, req_mips};
  hipError_t e;
  if ((n > 0 && (e = hipMemcpyAsync(s, adv_mips, nm, hipMemcpyHostToDevice, c->stream)) != hipSuccess) ||
      (e = hipMemcpyAsync(s + off_s, scal, sizeof scal, hipMemcpyHostToDevice, c->stream)) != hipSuccess)
    return hip_fail(c, e, "decide_v2 copy-in");
  e = fognet::launch_decide_v2(1, n, (const int32_t*)s, (const int32_t*)(s + off_s), (const int32_t*)(s + off_s) + 1,
                               (int32_t*)(s + off_o), (int32_t*)(s + off_o) + 1, c->stream);
  if (e != hipSuccess) return hip_fail(c, e, "decide_v2 launch");
  int32_t res[2] = {-1, 0};
  if ((e = hipMemcpyAsync(res, s + off_o, sizeof res, hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
      (e = hipStreamSynchronize(c->stream)) != hipSuccess)
    return hip_fail(c, e, "decide_v2 copy-out");
  *out_node = res[0];
  *out_action = res[1];
  return FOGNET_OK;
}

int fognet_run_generated_dev(fognet_ctx* c, const fognet_gen_params* p, int64_t r0, const fognet_batch_in* in,
                             fognet_batch_out* out, void* stream) {
  if (!c || !p || !in || !out) return FOGNET_ERR_ARG;
  if (in->arrive_tick || in->req_mips || in->mips || in->dl_tick || in->ul_tick || in->init_adv_tick || in->down_tick ||
      in->region)
    return fail(c, FOGNET_ERR_ARG, "generated replay: the trace and node-parameter arrays must be NULL (generated)");
  // (EXT_HIER: each publish's region from the mobility model of fa.mobility_regions, computed in the
  // kernel, replication by replication on the sequential wide kernel)
  if (out->node || out->status || out->start_tick || out->done_tick || out->escalated)
    return fail(c, FOGNET_ERR_ARG, "generated replay: statistics only (per-task arrays must be NULL)");
  if (!out->stats) return fail(c, FOGNET_ERR_ARG, "stats output is required (per-replication status)");
  if (r0 < 0 || p->req_lo < 0 || p->req_hi < p->req_lo) return fail(c, FOGNET_ERR_ARG, "bad r0 or req range");
  if (in->R > 0 && (!p->mean_gap_ticks || !p->lat_scale)) return fail(c, FOGNET_ERR_ARG, "null generator parameters");
  // the register kernel's in-loop statistics take per-node totals from the node tails' 32-bit
  // cumulative service (MIPS >= 1000): past 2^32 service seconds per replication the wide kernel
  // (64-bit cumulative sums) replays the generated traces instead
  const bool long_run = in->T > 0 && (uint64_t)in->T * (uint64_t)(p->req_hi / 1000) >= (1ull << 32);
  fognet::ReplayArgs a;
  int rc = prepare(c, in, &a, true);
  if (rc) return rc;
  if (a.R == 0) return FOGNET_OK;
  rc = set_device(c);
  if (rc) return rc;
  a.gen_on = 1;
  a.gen_r0 = r0;
  a.gen = *p;
  a.no_task_out = 1;
  a.out_stats = out->stats;
  a.out_energy = out->node_energy_j;
  a.hist = out->hist;
  if (a.out_energy && !a.p_busy) return fail(c, FOGNET_ERR_ARG, "node_energy_j needs the power model (p_busy_w/p_idle_w)");
  const hipStream_t s = (hipStream_t)stream;
  if (use_wide(a.N) || long_run || a.policy == FOGNET_POLICY_EXT_HIER) return run_wide(c, a, s);
  // the rings of the resident workgroups, reused by the wide hand-over
  const int64_t resident = (int64_t)c->cus * fognet::kGenWavesPerCu;
  a.gen_slots = (int32_t)(a.R < resident ? a.R : resident);
  const size_t ring_bytes = (size_t)a.gen_slots * (size_t)a.N * ((size_t)1 << a.q_log2) * sizeof(fognet::RingWord);
  const int32_t slots = fallback_slots(a.R, a.T, a.N, ring_bytes, true, a.policy);
  const size_t fb_bytes = fognet::replay_wide_workspace_bytes(slots, a.T, a.N, true, a.policy);
  fognet::ReplayWs w;
  rc = carve(c, "ring workspace", [&](fognet::WsCursor& v) {
    return fognet::generated_ws(w, a.R, ring_bytes, fb_bytes, v);
  });
  if (rc) return rc;
  a.wide_count = w.count;
  a.wide_list = w.list;
  a.ring = reinterpret_cast<fognet::RingWord*>(w.body);
  a.queue = w.count + 1;
  hipError_t e = hipMemsetAsync(w.count, 0, 2 * sizeof(int32_t), s);
  if (e != hipSuccess) return hip_fail(c, e, "hand-over and work counters");
  e = fognet::launch_replay(a, s);
  if (e != hipSuccess) return hip_fail(c, e, "replay launch");
  e = fognet::launch_replay_wide(a, w.body, slots, s);
  return e == hipSuccess ? FOGNET_OK : hip_fail(c, e, "wide hand-over launch");
}

int fognet_replay_dev(fognet_ctx* c, const fognet_batch_in* in, fognet_batch_out* out, void* stream) {
  return stage(c, in, out, stream, 1);
}

int fognet_rep_stats_dev(fognet_ctx* c, const fognet_batch_in* in, fognet_batch_out* out, void* stream) {
  return stage(c, in, out, stream, 2);
}

int fognet_run_batch_dev(fognet_ctx* c, const fognet_batch_in* in, fognet_batch_out* out, void* stream) {
  return stage(c, in, out, stream, 3);
}

// The assigned replay (replay_assigned.hip).  stats: fognet_run_assigned_dev.
static int run_assigned(fognet_ctx* c, const fognet_batch_in* in, const int32_t* assign, fognet_batch_out* out,
                        void* stream, bool stats) {
  if (!c || !out) return FOGNET_ERR_ARG;
  if (!in) return fail(c, FOGNET_ERR_ARG, "null batch");
  if (in->N > fognet::kWideBigMaxNodes)
    return fail(c, FOGNET_ERR_UNSUPPORTED, "assigned replay: N > 1048576 (the limit of every replay here)");
  // no broker decides: what only a decision reads is not read
  fognet_batch_in b = *in;
  b.policy = FOGNET_POLICY_REF_V3;
  b.ring_capacity = 0;
  b.region = nullptr;
  b.hier_up_tick = 0;
  b.hier_threshold_s = 0;
  fognet::ReplayArgs a;
  int rc = prepare(c, &b, &a);
  if (rc) return rc;
  if (a.R > 0 && !out->stats) return fail(c, FOGNET_ERR_ARG, "stats output is required (per-replication status)");
  const bool tasks = a.R > 0 && a.T > 0;
  if (tasks && (!out->node || !out->status || !out->start_tick || !out->done_tick))
    return fail(c, FOGNET_ERR_ARG, "assigned replay: all four per-task arrays are required (no statistics-only out)");
  if (tasks && !assign) return fail(c, FOGNET_ERR_ARG, "assigned replay: null assign");
  if (stats && out->node_energy_j && !a.p_busy)
    return fail(c, FOGNET_ERR_ARG, "node_energy_j needs the power model (p_busy_w/p_idle_w)");
  if (a.R == 0) return FOGNET_OK;
  if ((rc = set_device(c))) return rc;
  a.out_node = out->node;
  a.out_status = out->status;
  a.out_start = out->start_tick;
  a.out_done = out->done_tick;
  a.out_stats = out->stats;
  if (stats) {
    a.out_energy = out->node_energy_j;
    a.hist = out->hist;
  }
  const hipStream_t s = (hipStream_t)stream;
  if (out->escalated && tasks) {  // nobody escalates
    const hipError_t e = hipMemsetAsync(out->escalated, 0, (size_t)a.R * (size_t)a.T, s);
    if (e != hipSuccess) return hip_fail(c, e, "escalated clear");
  }
  // FOGNET_ASSIGNED=hbm: counts and carries in the workspace for every N (the layout of
  // N > replay_assigned_lds_max()), so small tests run both layouts on the same traces
  const bool force_hbm = env_is("FOGNET_ASSIGNED", "hbm");
  const bool carry_hbm = force_hbm || a.N > fognet::replay_assigned_lds_max();
  fognet::AssignedWs w;
  rc = carve(c, "assigned replay workspace", [&](fognet::WsCursor& v) {
    return fognet::assigned_ws(w, (size_t)a.R, (size_t)a.T, (size_t)a.N, carry_hbm ? (size_t)a.R * (size_t)a.N : 0, v);
  });
  if (rc) return rc;
  // FOGNET_ASSIGNED_STAGES=1 (timing only): stop after the validation + count kernel; nothing is written then
  const int stages = env_is("FOGNET_ASSIGNED_STAGES", "1") ? 1 : 2;
  const hipError_t e = fognet::launch_replay_assigned(a, assign, w, stats, force_hbm, stages, s);
  return e == hipSuccess ? FOGNET_OK : hip_fail(c, e, "assigned replay launch");
}

int fognet_replay_assigned_dev(fognet_ctx* c, const fognet_batch_in* in, const int32_t* assign, fognet_batch_out* out,
                               void* stream) {
  return run_assigned(c, in, assign, out, stream, false);
}

int fognet_run_assigned_dev(fognet_ctx* c, const fognet_batch_in* in, const int32_t* assign, fognet_batch_out* out,
                            void* stream) {
  return run_assigned(c, in, assign, out, stream, true);
}

int fognet_run_batch(fognet_ctx* c, const fognet_batch_in* in, fognet_batch_out* out) {
  if (!c || !in || !out) return FOGNET_ERR_ARG;
  fognet::ReplayArgs chk;
  int rc = prepare(c, in, &chk);
  if (rc) return rc;
  rc = set_device(c);
  if (rc) return rc;
  const size_t R = (size_t)in->R, RT = R * (size_t)in->T, N = (size_t)in->N;
  const size_t NRN = (in->node_stride ? R : 1) * N;
  const size_t HB = FOGNET_HIST_METRICS * FOGNET_HIST_BINS * sizeof(int64_t);
  // One device buffer per present host array (an absent optional one stays null): src is copied in
  // before the launch, dst copied out after it; hist is both, because it is added to.
  struct Buf { const void* src; void* dst; size_t bytes; bool present; void* dev; };
  enum { kRegion, kArrive, kReq, kMips, kDl, kUl, kInit, kPBusy, kPIdle, kDown,
         kNode, kStatus, kStart, kDone, kStats, kEnergy, kHist, kEsc, kBufs };
  const bool rg = in->policy == FOGNET_POLICY_EXT_HIER && in->region != nullptr;
  Buf b[kBufs] = {
      {in->region, nullptr, RT * 4, rg},
      {in->arrive_tick, nullptr, RT * 8, true},
      {in->req_mips, nullptr, RT * 4, true},
      {in->mips, nullptr, NRN * 4, true},
      {in->dl_tick, nullptr, NRN * 8, true},
      {in->ul_tick, nullptr, NRN * 8, true},
      {in->init_adv_tick, nullptr, NRN * 8, true},
      {in->p_busy_w, nullptr, NRN * 8, in->p_busy_w != nullptr},
      {in->p_idle_w, nullptr, NRN * 8, in->p_busy_w != nullptr},
      {in->down_tick, nullptr, NRN * 8, in->down_tick != nullptr},
      {nullptr, out->node, RT * 4, out->node != nullptr},  // (statistics only: no per-task outputs)
      {nullptr, out->status, RT * 1, out->status != nullptr},
      {nullptr, out->start_tick, RT * 8, out->start_tick != nullptr},
      {nullptr, out->done_tick, RT * 8, out->done_tick != nullptr},
      {nullptr, out->stats, R * sizeof(fognet_rep_stats), true},
      {nullptr, out->node_energy_j, R * N * 8, out->node_energy_j != nullptr},
      {out->hist, out->hist, HB, out->hist != nullptr},
      {nullptr, out->escalated, RT * 1, out->escalated != nullptr},
  };
  rc = [&]() -> int {
    hipError_t e;
    for (Buf& x : b) {
      if (!x.present) continue;
      const bool region = &x == &b[kRegion];
      if ((e = hipMalloc(&x.dev, x.bytes ? x.bytes : 8)) != hipSuccess)
        return hip_fail(c, e, region ? "region copy-in" : "hipMalloc batch");
      if (x.src && x.bytes && (e = hipMemcpyAsync(x.dev, x.src, x.bytes, hipMemcpyHostToDevice, c->stream)) != hipSuccess)
        return hip_fail(c, e, region ? "region copy-in" : "copy-in");
    }
    fognet_batch_in din = *in;
    din.region = (const int32_t*)b[kRegion].dev;
    din.arrive_tick = (const int64_t*)b[kArrive].dev;
    din.req_mips = (const int32_t*)b[kReq].dev;
    din.mips = (const int32_t*)b[kMips].dev;
    din.dl_tick = (const int64_t*)b[kDl].dev;
    din.ul_tick = (const int64_t*)b[kUl].dev;
    din.init_adv_tick = (const int64_t*)b[kInit].dev;
    din.p_busy_w = (const double*)b[kPBusy].dev;
    din.p_idle_w = (const double*)b[kPIdle].dev;
    din.down_tick = (const int64_t*)b[kDown].dev;
    fognet_batch_out dout = {(int32_t*)b[kNode].dev, (uint8_t*)b[kStatus].dev, (int64_t*)b[kStart].dev,
                             (int64_t*)b[kDone].dev, (fognet_rep_stats*)b[kStats].dev, (double*)b[kEnergy].dev,
                             (int64_t*)b[kHist].dev, (uint8_t*)b[kEsc].dev};
    const int rc_run = fognet_run_batch_dev(c, &din, &dout, c->stream);
    if (rc_run) return rc_run;
    for (Buf& x : b)
      if (x.dev && x.dst && x.bytes &&
          (e = hipMemcpyAsync(x.dst, x.dev, x.bytes, hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
        return hip_fail(c, e, "copy-out");
    e = hipStreamSynchronize(c->stream);
    return e == hipSuccess ? FOGNET_OK : hip_fail(c, e, "batch sync");
  }();
  for (Buf& x : b)  // on every exit
    if (x.dev) (void)hipFree(x.dev);
  if (rc) return rc;
  if (out->stats)
    for (size_t r = 0; r < R; ++r)
      if (out->stats[r].status != FOGNET_OK) {
        char buf[96];
        snprintf(buf, sizeof buf, "replication %zu: %s", r, fognet_status_string(out->stats[r].status));
        return fail(c, out->stats[r].status, buf);
      }
  return FOGNET_OK;
}

// ---------------------------------------------------------------- passes over a finished replay
// What the five passes share of their entry points; each keeps its own checks, in its own order, between them.
struct PassSpec {
  bool need_start;    // the pass reads start_tick as well as node, status and done_tick
  bool hier_refused;  // EXT_HIER: refused outright; else only without fognet_batch_out.escalated
  const char* hier_msg;
};
#define FOGNET_NEEDS_ESCALATED \
  "the per-task outputs do not say which tasks were escalated (replay with fognet_batch_out.escalated)"

static int pass_begin(fognet_ctx* c, const fognet_batch_in* in, const fognet_batch_out* out, const PassSpec& p,
                      fognet::ReplayArgs* a) {
  if (!c || !out) return FOGNET_ERR_ARG;
  if (in && in->policy == FOGNET_POLICY_EXT_HIER && (p.hier_refused || !out->escalated))
    return fail(c, FOGNET_ERR_UNSUPPORTED, p.hier_msg);
  return prepare(c, in, a);
}

// (a statistics-only out has no per-task outputs)
static bool has_task_outputs(const fognet::ReplayArgs& a, const fognet_batch_out* out, const PassSpec& p) {
  return a.T <= 0 || (out->node && out->status && out->done_tick && (!p.need_start || out->start_tick));
}

// the device, and the replay's outputs as the pass's inputs
static int pass_bind(fognet_ctx* c, const fognet_batch_out* out, const PassSpec& p, fognet::ReplayArgs* a) {
  a->out_node = out->node, a->out_status = out->status, a->out_done = out->done_tick, a->out_stats = out->stats;
  if (p.need_start) a->out_start = out->start_tick;
  if (!p.hier_refused && a->policy == FOGNET_POLICY_EXT_HIER) a->out_esc = out->escalated;  // (else never read)
  return set_device(c);
}

int fognet_user_stats_dev(fognet_ctx* c, const fognet_batch_in* in, const fognet_batch_out* out, const int64_t* user_ul,
                          const int64_t* user_dl, int32_t user_per_task, fognet_user_stats* user_stats, void* stream) {
  static const PassSpec spec = {false, false, "user signals under EXT_HIER: the acks of an escalated task leave its "
                                              "node hier_up_tick later, and " FOGNET_NEEDS_ESCALATED};
  fognet::ReplayArgs a;
  int rc = pass_begin(c, in, out, spec, &a);
  if (rc) return rc;
  if (user_per_task != 0 && user_per_task != 1) return fail(c, FOGNET_ERR_ARG, "user_per_task must be 0 or 1");
  if (a.R == 0) return FOGNET_OK;
  if (!user_ul || !user_dl || !user_stats || !out->stats || !has_task_outputs(a, out, spec))
    return fail(c, FOGNET_ERR_ARG, "null pointer");
  if ((rc = pass_bind(c, out, spec, &a))) return rc;
  hipError_t e = fognet::launch_user_stats(a, user_ul, user_dl, user_per_task, user_stats, (hipStream_t)stream);
  return e == hipSuccess ? FOGNET_OK : hip_fail(c, e, "user stats launch");
}

int fognet_node_stats_dev(fognet_ctx* c, const fognet_batch_in* in, const fognet_batch_out* out,
                          fognet_node_stats* node_stats, void* stream) {
  static const PassSpec spec = {true, false, "node statistics under EXT_HIER: an escalated task reaches its node "
                                             "hier_up_tick later, and " FOGNET_NEEDS_ESCALATED};
  fognet::ReplayArgs a;
  int rc = pass_begin(c, in, out, spec, &a);
  if (rc) return rc;
  if (a.R == 0) return FOGNET_OK;
  if (!out->stats) return fail(c, FOGNET_ERR_ARG, "null stats");
  if (!has_task_outputs(a, out, spec))
    return fail(c, FOGNET_ERR_ARG, "node statistics need the per-task outputs (a statistics-only out has none)");
  if (!node_stats) return fail(c, FOGNET_ERR_ARG, "null node_stats");
  if ((rc = pass_bind(c, out, spec, &a))) return rc;
  // FOGNET_NODE_STATS=hbm: the accumulators are the caller's records for every N (the layout of
  // N > node_stats_lds_max()), so small tests run both layouts on the same traces
  const hipError_t e = fognet::launch_node_stats(a, node_stats, env_is("FOGNET_NODE_STATS", "hbm"), (hipStream_t)stream);
  return e == hipSuccess ? FOGNET_OK : hip_fail(c, e, "node stats launch");
}

int fognet_reduce_node_stats_dev(fognet_ctx* c, const fognet_node_stats* node_stats, const fognet_rep_stats* stats,
                                 int32_t R, int32_t N, fognet_node_stats* out, void* stream) {
  return reduce_keyed(c, node_stats, stats, R, N, out, stream, fognet::launch_reduce_node_stats, "negative R/N",
                      "node reduce launch");
}

// (of `in` only R and T are read: no prepare(), which checks the trace and the policy)
int fognet_compare_dev(fognet_ctx* c, const fognet_batch_in* in, const fognet_batch_out* out_a,
                       const fognet_batch_out* out_b, fognet_compare_stats* cmp, int64_t* hist, void* stream) {
  if (!c) return FOGNET_ERR_ARG;
  if (!in || !out_a || !out_b) return fail(c, FOGNET_ERR_ARG, "null batch");
  if (in->R < 0 || in->T < 0) return fail(c, FOGNET_ERR_ARG, "negative R/T");
  if (in->R == 0) return FOGNET_OK;
  if (!out_a->stats || !out_b->stats) return fail(c, FOGNET_ERR_ARG, "null stats");
  for (const fognet_batch_out* o : {out_a, out_b})
    if (in->T > 0 && (!o->node || !o->status || !o->start_tick || !o->done_tick))
      return fail(c, FOGNET_ERR_ARG, "the comparison needs the per-task outputs of both replays (a statistics-only out has none)");
  if (!cmp) return fail(c, FOGNET_ERR_ARG, "null cmp");
  const int rc = set_device(c);
  if (rc) return rc;
  const hipError_t e = fognet::launch_compare(fognet::CompareIn{in->R, in->T, out_a, out_b}, cmp, hist, (hipStream_t)stream);
  return e == hipSuccess ? FOGNET_OK : hip_fail(c, e, "compare launch");
}

int fognet_reduce_compare_dev(fognet_ctx* c, const fognet_compare_stats* cmp, int32_t R, fognet_compare_stats* out,
                              void* stream) {
  if (!c) return FOGNET_ERR_ARG;
  if (R < 0) return fail(c, FOGNET_ERR_ARG, "negative R");
  if (!out || (R > 0 && !cmp)) return fail(c, FOGNET_ERR_ARG, "null pointer");
  const int rc = set_device(c);
  if (rc) return rc;
  const hipError_t e = fognet::launch_reduce_compare(cmp, R, out, (hipStream_t)stream);
  return e == hipSuccess ? FOGNET_OK : hip_fail(c, e, "compare reduce launch");
}

int fognet_reduce_groups_dev(fognet_ctx* c, const fognet_rep_stats* stats, int32_t R, const int32_t* group_of, int32_t G,
                             fognet_group_stats* out, int64_t* metrics, uint32_t* defined, int64_t* n_ungrouped,
                             void* stream) {
  if (!c) return FOGNET_ERR_ARG;
  if (R < 0) return fail(c, FOGNET_ERR_ARG, "negative R");
  if (G <= 0) return fail(c, FOGNET_ERR_ARG, "G must be positive");
  if (!out || (R > 0 && !stats)) return fail(c, FOGNET_ERR_ARG, "null pointer");
  const int rc = set_device(c);
  if (rc) return rc;
  // FOGNET_GROUP_STATS=hbm: the accumulators are the caller's records for every G (the layout above
  // FOGNET_GROUP_LDS_MAX groups), so small tests run both layouts on the same records
  const hipError_t e = fognet::launch_reduce_groups(stats, R, group_of, G, out, metrics, defined, n_ungrouped,
                                                    env_is("FOGNET_GROUP_STATS", "hbm"), (hipStream_t)stream);
  return e == hipSuccess ? FOGNET_OK : hip_fail(c, e, "group reduce launch");
}

int fognet_per_user_stats_dev(fognet_ctx* c, const fognet_batch_in* in, const fognet_batch_out* out,
                              const int32_t* user_of, int32_t U, int32_t link_stride, const int64_t* user_ul,
                              const int64_t* user_dl, fognet_user_stats* per_user, int64_t* n_unassigned, void* stream) {
  static const PassSpec spec = {false, false, "per-user signals under EXT_HIER: the acks of an escalated task leave "
                                              "its node hier_up_tick later, and " FOGNET_NEEDS_ESCALATED};
  fognet::ReplayArgs a;
  int rc = pass_begin(c, in, out, spec, &a);
  if (rc) return rc;
  if (U < 0) return fail(c, FOGNET_ERR_ARG, "negative U");
  if (link_stride != 0 && link_stride != U) return fail(c, FOGNET_ERR_ARG, "link_stride must be 0 or U");
  if (a.R == 0) return FOGNET_OK;
  if (!out->stats) return fail(c, FOGNET_ERR_ARG, "null stats");
  if (!has_task_outputs(a, out, spec))
    return fail(c, FOGNET_ERR_ARG, "per-user signals need the per-task outputs (a statistics-only out has none)");
  if (a.T > 0 && !user_of && (U > 0 || n_unassigned)) return fail(c, FOGNET_ERR_ARG, "null user_of");
  if (U > 0 && (!per_user || !user_ul || !user_dl)) return fail(c, FOGNET_ERR_ARG, "null per_user or user links");
  if ((rc = pass_bind(c, out, spec, &a))) return rc;
  // FOGNET_USER_STATS=hbm: the accumulators are the caller's records for every U (the layout of
  // U > per_user_stats_lds_max()), so small tests run both layouts on the same traces
  const fognet::UserLinks users{user_of, user_ul, user_dl, U, link_stride};
  const hipError_t e = fognet::launch_per_user_stats(a, users, per_user, n_unassigned, env_is("FOGNET_USER_STATS", "hbm"),
                                                     (hipStream_t)stream);
  return e == hipSuccess ? FOGNET_OK : hip_fail(c, e, "per-user stats launch");
}

int fognet_window_stats_dev(fognet_ctx* c, const fognet_batch_in* in, const fognet_batch_out* out,
                            const int32_t* user_of, int32_t U, int32_t link_stride, const int64_t* user_ul,
                            const int64_t* user_dl, int64_t t0, int64_t window, int32_t W, fognet_window_stats* win,
                            int64_t* n_outside, int64_t* n_unassigned, void* stream) {
  static const PassSpec spec = {true, false, "window statistics under EXT_HIER: an escalated task reaches its node, "
                                             "and sends its acks, hier_up_tick later, and " FOGNET_NEEDS_ESCALATED};
  static_assert(FOGNET_WINDOW_MAX == 1 << 20, "the message below");
  fognet::ReplayArgs a;
  int rc = pass_begin(c, in, out, spec, &a);
  if (rc) return rc;
  if (U < 0) return fail(c, FOGNET_ERR_ARG, "negative U");
  if (link_stride != 0 && link_stride != U) return fail(c, FOGNET_ERR_ARG, "link_stride must be 0 or U");
  if (window < 1 || t0 < 0 || W < 0) return fail(c, FOGNET_ERR_ARG, "window_tick >= 1, t0_tick >= 0 and W >= 0");
  if (W > FOGNET_WINDOW_MAX) return fail(c, FOGNET_ERR_UNSUPPORTED, "window statistics: W > 1048576 windows");
  const int64_t kEnd = (int64_t)1 << 62;  // (W <= 2^20: the quotient cannot wrap)
  if (W > 0 && (window > kEnd / W || t0 > kEnd - (int64_t)W * window))
    return fail(c, FOGNET_ERR_ARG, "t0_tick + W * window_tick must not pass 2^62");
  if (t0 > kEnd) return fail(c, FOGNET_ERR_ARG, "t0_tick + W * window_tick must not pass 2^62");
  if (a.R == 0) return FOGNET_OK;
  if (!out->stats) return fail(c, FOGNET_ERR_ARG, "null stats");
  if (!has_task_outputs(a, out, spec))
    return fail(c, FOGNET_ERR_ARG, "window statistics need the per-task outputs, start_tick included");
  if (W > 0 && !win) return fail(c, FOGNET_ERR_ARG, "null win");
  if (a.T > 0 && U > 0 && !user_of) return fail(c, FOGNET_ERR_ARG, "null user_of");
  if (U > 0 && (!user_ul || !user_dl)) return fail(c, FOGNET_ERR_ARG, "null user links");
  if ((rc = pass_bind(c, out, spec, &a))) return rc;
  // FOGNET_WINDOW_STATS=hbm: the accumulators are the caller's records and the workspace for every W
  // (the layout of W > FOGNET_WINDOW_LDS_WINDOWS), so small tests run both layouts on the same traces
  const bool force_hbm = env_is("FOGNET_WINDOW_STATS", "hbm");
  const size_t delta_n = fognet::window_stats_delta_count(a.R, W, force_hbm);
  fognet::WindowWs w{};
  if (delta_n > 0) {
    fognet::WsCursor measure{nullptr};
    rc = ensure(c, (void**)&c->ring, &c->ring_bytes, fognet::window_stats_ws(w, delta_n, measure), "window cover counts");
    if (rc) return rc;
    fognet::WsCursor carve{reinterpret_cast<unsigned char*>(c->ring)};
    (void)fognet::window_stats_ws(w, delta_n, carve);
  }
  const fognet::UserLinks users{user_of, user_ul, user_dl, U, link_stride};
  const hipError_t e = fognet::launch_window_stats(a, users, t0, window, W, win, n_outside, n_unassigned, w.delta,
                                                   force_hbm, (hipStream_t)stream);
  return e == hipSuccess ? FOGNET_OK : hip_fail(c, e, "window stats launch");
}

// fognet_quantiles_dev (job = false) and fognet_job_quantiles_dev
static int run_quantiles(fognet_ctx* c, const fognet_batch_in* in, const fognet_batch_out* out, const int32_t* user_of,
                         int32_t U, int32_t link_stride, const int64_t* user_ul, const int64_t* user_dl,
                         const int32_t* ppm, int32_t Q, int64_t* value, int64_t* count, int64_t* n_unassigned,
                         void* stream, bool job) {
  static const PassSpec spec = {true, false, "quantiles under EXT_HIER: an escalated task reaches its node, and sends "
                                             "its acks, hier_up_tick later, and " FOGNET_NEEDS_ESCALATED};
  static_assert(FOGNET_QUANTILE_MAX == 8, "the message below");
  fognet::ReplayArgs a;
  int rc = pass_begin(c, in, out, spec, &a);
  if (rc) return rc;
  if (Q < 1 || Q > FOGNET_QUANTILE_MAX) return fail(c, FOGNET_ERR_ARG, "quantiles: 1 <= Q <= 8 ranks per call");
  for (int32_t q = 0; ppm && q < Q; ++q)
    if (ppm[q] < 0 || ppm[q] > 1000000) return fail(c, FOGNET_ERR_ARG, "quantiles: a rank is a ppm in [0, 1000000]");
  if (U < 0) return fail(c, FOGNET_ERR_ARG, "negative U");
  if (link_stride != 0 && link_stride != U) return fail(c, FOGNET_ERR_ARG, "link_stride must be 0 or U");
  if (a.R == 0 && (!job || !ppm || !value || !count)) return FOGNET_OK;
  if (!ppm || !value || !count) return fail(c, FOGNET_ERR_ARG, "null ppm, value or count");
  if (a.R > 0) {
    if (!out->stats) return fail(c, FOGNET_ERR_ARG, "null stats");
    if (!has_task_outputs(a, out, spec))
      return fail(c, FOGNET_ERR_ARG, "quantiles need the per-task outputs, start_tick included");
    if (U > 0 && (!user_ul || !user_dl)) return fail(c, FOGNET_ERR_ARG, "null user links");
    if (a.T > 0 && U > 0 && !user_of) return fail(c, FOGNET_ERR_ARG, "null user_of");
  }
  if ((rc = pass_bind(c, out, spec, &a))) return rc;
  // FOGNET_QUANTILES=full: no round is skipped, so small tests run both ways on the same replays
  const bool full = env_is("FOGNET_QUANTILES", "full");
  const fognet::UserLinks users{user_of, user_ul, user_dl, U, link_stride};
  hipError_t e;
  if (job) {
    fognet::QuantWs w;
    rc = carve(c, "job quantile counters", [&](fognet::WsCursor& v) {
      return fognet::quantiles_ws(w, fognet::quantiles_table_count(Q), v);
    });
    if (rc) return rc;
    e = fognet::launch_job_quantiles(a, users, ppm, Q, value, count, w, full, (hipStream_t)stream);
  } else {
    e = fognet::launch_quantiles(a, users, ppm, Q, value, count, n_unassigned, full, (hipStream_t)stream);
  }
  return e == hipSuccess ? FOGNET_OK : hip_fail(c, e, "quantiles launch");
}

int fognet_quantiles_dev(fognet_ctx* c, const fognet_batch_in* in, const fognet_batch_out* out, const int32_t* user_of,
                         int32_t U, int32_t link_stride, const int64_t* user_ul, const int64_t* user_dl,
                         const int32_t* ppm, int32_t Q, int64_t* value, int64_t* count, int64_t* n_unassigned,
                         void* stream) {
  return run_quantiles(c, in, out, user_of, U, link_stride, user_ul, user_dl, ppm, Q, value, count, n_unassigned, stream,
                       false);
}

int fognet_job_quantiles_dev(fognet_ctx* c, const fognet_batch_in* in, const fognet_batch_out* out,
                             const int32_t* user_of, int32_t U, int32_t link_stride, const int64_t* user_ul,
                             const int64_t* user_dl, const int32_t* ppm, int32_t Q, int64_t* value, int64_t* count,
                             void* stream) {
  return run_quantiles(c, in, out, user_of, U, link_stride, user_ul, user_dl, ppm, Q, value, count, nullptr, stream, true);
}

#undef FOGNET_NEEDS_ESCALATED

// replications [r0, r0 + Rr) of a pass's argument block: every [R][..] array moved to row r0
static fognet::ReplayArgs slice_reps(const fognet::ReplayArgs& a, int32_t r0, int32_t Rr) {
  fognet::ReplayArgs b = a;
  const size_t t = (size_t)r0 * (size_t)a.T, nd = (size_t)r0 * (size_t)a.node_stride;
  b.R = Rr;
  if (t != 0) b.arrive += t, b.req += t, b.out_node += t, b.out_status += t, b.out_start += t, b.out_done += t;
  if (nd != 0) {
    b.mips += nd, b.dl += nd, b.ul += nd, b.init += nd;
    if (b.down) b.down += nd;
  }
  b.out_stats += r0;
  return b;
}

int fognet_queue_stats_dev(fognet_ctx* c, const fognet_batch_in* in, const fognet_batch_out* out, const int64_t* level,
                           int32_t Q, int64_t t0, int64_t t1, fognet_queue_stats* qs, void* stream) {
  static const PassSpec spec = {true, true, "queue-length statistics under EXT_HIER: an escalated task arrives a hop "
                                            "later, so a node's FIFO order is no longer trace order, and where that "
                                            "arrival stands among the events of its tick is builder-defined"};
  static_assert(FOGNET_QUEUE_LEVELS_MAX == 8, "the message below");
  fognet::ReplayArgs a;
  int rc = pass_begin(c, in, out, spec, &a);
  if (rc) return rc;
  if (Q < 1 || Q > FOGNET_QUEUE_LEVELS_MAX) return fail(c, FOGNET_ERR_ARG, "queue statistics: 1 <= Q <= 8 levels per call");
  if (!level) return fail(c, FOGNET_ERR_ARG, "null level");
  for (int32_t q = 0; q < Q; ++q)
    if (level[q] < 1 || (q > 0 && level[q] <= level[q - 1]))
      return fail(c, FOGNET_ERR_ARG, "queue statistics: levels are >= 1 and strictly ascending");
  if (t0 < 0 || t1 < t0 || t1 > ((int64_t)1 << 62))
    return fail(c, FOGNET_ERR_ARG, "queue statistics: 0 <= t0_tick <= t1_tick <= 2^62");
  if (a.R == 0) return FOGNET_OK;
  if (!out->stats) return fail(c, FOGNET_ERR_ARG, "null stats");
  if (!has_task_outputs(a, out, spec))
    return fail(c, FOGNET_ERR_ARG, "queue statistics need the per-task outputs, start_tick included");
  if (!qs) return fail(c, FOGNET_ERR_ARG, "null qs");
  if ((rc = pass_bind(c, out, spec, &a))) return rc;
  // FOGNET_QUEUE_STATS=hbm: counts, carries and accumulators in the workspace and the caller's records for
  // every N (the layouts of large N), so small tests run both on the same traces
  const bool force_hbm = env_is("FOGNET_QUEUE_STATS", "hbm");
  const bool carry_hbm = force_hbm || a.N > fognet::queue_stats_build_lds_max();
  // rounds: as many replications as keep a round's elements within kRoundBytes (at least one)
  constexpr size_t kRoundBytes = (size_t)1 << 30;
  const size_t per_rep = (size_t)a.T * fognet::kQueueElementBytes;
  size_t round = per_rep ? kRoundBytes / per_rep : (size_t)a.R;
  if (const char* f = getenv("FOGNET_QUEUE_ROUND")) {
    const long v = atol(f);
    if (v > 0) round = (size_t)v;
  }
  const int32_t Rr = (int32_t)(round < 1 ? 1 : round > (size_t)a.R ? (size_t)a.R : round);
  fognet::QueueWs w;
  rc = carve(c, "queue statistics workspace", [&](fognet::WsCursor& v) {
    return fognet::queue_stats_ws(w, (size_t)Rr, (size_t)a.T, (size_t)a.N, carry_hbm ? (size_t)Rr * (size_t)a.N : 0, v);
  });
  if (rc) return rc;
  // FOGNET_QUEUE_STAGES=1 (timing only): stop after count + build; nothing is written then
  const int stages = env_is("FOGNET_QUEUE_STAGES", "1") ? 1 : 2;
  for (int32_t r0 = 0; r0 < a.R; r0 += Rr) {  // (stream order: a round's kernels are done with the workspace before the next)
    const int32_t n = a.R - r0 < Rr ? a.R - r0 : Rr;
    const hipError_t e = fognet::launch_queue_stats(slice_reps(a, r0, n), w, level, Q, t0, t1,
                                                    qs + (size_t)r0 * (size_t)a.N, force_hbm, stages, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(c, e, "queue statistics launch");
  }
  return FOGNET_OK;
}

int fognet_reduce_queue_stats_dev(fognet_ctx* c, const fognet_queue_stats* qs, const fognet_rep_stats* stats, int32_t R,
                                  int32_t N, fognet_queue_stats* out, void* stream) {
  return reduce_keyed(c, qs, stats, R, N, out, stream, fognet::launch_reduce_queue_stats, "negative R/N",
                      "queue reduce launch");
}

int fognet_reduce_window_stats_dev(fognet_ctx* c, const fognet_window_stats* win, const fognet_rep_stats* stats,
                                   int32_t R, int32_t W, fognet_window_stats* out, void* stream) {
  return reduce_keyed(c, win, stats, R, W, out, stream, fognet::launch_reduce_window_stats, "negative R/W",
                      "window reduce launch");
}

int fognet_signal_vectors_dev(fognet_ctx* c, const fognet_batch_in* in, const fognet_batch_out* out,
                              const int32_t* user_of, int32_t U, int32_t link_stride, const int64_t* user_ul,
                              const int64_t* user_dl, int32_t r0, int32_t Rv, const fognet_signal_vectors* vec,
                              int64_t* n_unassigned, void* stream) {
  static const PassSpec spec = {true, true, "signal vectors under EXT_HIER: where an escalated task's acks stand among "
                                            "the acks of their tick is builder-defined, and no recording of the "
                                            "reference pins it"};
  fognet::ReplayArgs a;
  int rc = pass_begin(c, in, out, spec, &a);
  if (rc) return rc;
  if (U < 0) return fail(c, FOGNET_ERR_ARG, "negative U");
  if (link_stride != 0 && link_stride != U) return fail(c, FOGNET_ERR_ARG, "link_stride must be 0 or U");
  if (r0 < 0 || Rv < 0 || (int64_t)r0 + Rv > a.R) return fail(c, FOGNET_ERR_ARG, "[r0, r0 + Rv) must lie in [0, R)");
  if (Rv == 0) return FOGNET_OK;
  if (!out->stats) return fail(c, FOGNET_ERR_ARG, "null stats");
  if (!has_task_outputs(a, out, spec))
    return fail(c, FOGNET_ERR_ARG, "signal vectors need the per-task outputs, start_tick included");
  if (a.T > 0 && !user_of) return fail(c, FOGNET_ERR_ARG, "null user_of");
  if (U > 0 && (!user_ul || !user_dl)) return fail(c, FOGNET_ERR_ARG, "null user links");
  if (!vec || !vec->offset || (a.T > 0 && (!vec->time || !vec->value || !vec->task)))
    return fail(c, FOGNET_ERR_ARG, "null vec or vec arrays");
  if (vec->cap < 6 * (int64_t)a.T) return fail(c, FOGNET_ERR_ARG, "vec->cap must be at least 6 * T");
  const int64_t V = (int64_t)a.N + 1 + 3 * (int64_t)U;
  if (a.T >= (1 << 28) || V * Rv >= ((int64_t)1 << 31))
    return fail(c, FOGNET_ERR_UNSUPPORTED, "signal vectors: T >= 2^28 or Rv * V >= 2^31");
  if ((rc = pass_bind(c, out, spec, &a))) return rc;
  fognet::VecWs w{};
  fognet::WsCursor measure{nullptr};
  rc = ensure(c, (void**)&c->ring, &c->ring_bytes, fognet::signal_vectors_ws(w, (size_t)Rv, (size_t)V, measure),
              "signal vector cursors");
  if (rc) return rc;
  fognet::WsCursor carve{reinterpret_cast<unsigned char*>(c->ring)};
  (void)fognet::signal_vectors_ws(w, (size_t)Rv, (size_t)V, carve);
  // FOGNET_VEC_SORT=hbm: every segment is sorted in HBM and the counters live in HBM (the layouts of
  // large segments and of V > signal_vectors_lds_max()), so small tests run both on the same traces.
  // FOGNET_VEC_STAGES=1 / 2: stop after the count / place stage (tools/time_signal_vectors.py).
  const int stages = env_is("FOGNET_VEC_STAGES", "1") ? 1 : env_is("FOGNET_VEC_STAGES", "2") ? 2 : 3;
  const fognet::UserLinks users{user_of, user_ul, user_dl, U, link_stride};
  const hipError_t e = fognet::launch_signal_vectors(a, users, r0, Rv, *vec, n_unassigned, w.cursor,
                                                     env_is("FOGNET_VEC_SORT", "hbm"), stages, (hipStream_t)stream);
  return e == hipSuccess ? FOGNET_OK : hip_fail(c, e, "signal vectors launch");
}

int fognet_reduce_user_stats_dev(fognet_ctx* c, const fognet_user_stats* user_stats, const fognet_rep_stats* stats,
                                 int32_t R, int32_t U, fognet_user_stats* out, void* stream) {
  return reduce_keyed(c, user_stats, stats, R, U, out, stream, fognet::launch_reduce_user_stats, "negative R/U",
                      "user reduce launch");
}

int fognet_run_v2_dev(fognet_ctx* c, const fognet_v2_in* in, fognet_v2_out* out, void* stream) {
  if (!c || !in || !out) return FOGNET_ERR_ARG;
  if (in->R < 0 || in->T < 0 || in->N < 0) return fail(c, FOGNET_ERR_ARG, "negative R/T/N");
  if (in->N > FOGNET_V2_MAX_NODES)
    return fail(c, FOGNET_ERR_UNSUPPORTED, "the v2 replay keeps at most 256 nodes per lane: N <= 16384");
  if (in->node_stride != 0 && in->node_stride != in->N) return fail(c, FOGNET_ERR_ARG, "node_stride must be 0 or N");
  const int q = in->queue_capacity ? in->queue_capacity : 256;
  if (q < 2 || (q & (q - 1)) != 0 || q > (1 << 16)) return fail(c, FOGNET_ERR_ARG, "queue_capacity must be a power of two in [2, 2^16]");
  int qlog = 0;
  while ((1 << qlog) < q) ++qlog;
  if (in->R == 0) return FOGNET_OK;
  if (!in->broker_mips || !in->required_time_s || !in->stop_tick || (in->T > 0 && (!in->arrive_tick || !in->req_mips)) ||
      (in->N > 0 && (!in->mips || !in->dl_tick || !in->ul_tick || !in->first_adv_tick)))
    return fail(c, FOGNET_ERR_ARG, "null input array");
  if (!out->stats || (in->T > 0 && (!out->node || !out->status || !out->start_tick || !out->done_tick)))
    return fail(c, FOGNET_ERR_ARG, "null output array");
  int rc = set_device(c);
  if (rc) return rc;
  rc = ensure(c, (void**)&c->ring, &c->ring_bytes, fognet::replay_v2_workspace_bytes(in->R, in->T, in->N, qlog),
              "v2 replay workspace");
  if (rc) return rc;
  hipError_t e = fognet::launch_replay_v2(*in, *out, c->ring, qlog, (hipStream_t)stream);
  return e == hipSuccess ? FOGNET_OK : hip_fail(c, e, "v2 replay launch");
}

int fognet_reduce_stats_dev(fognet_ctx* c, const fognet_rep_stats* stats, int32_t R, fognet_job_stats* out,
                            void* stream) {
  if (!c || !out || (R > 0 && !stats) || R < 0) return FOGNET_ERR_ARG;
  int rc = set_device(c);
  if (rc) return rc;
  const int32_t np = fognet::reduce_stats_parts(R);
  if (np > 0) {
    rc = ensure(c, &c->red, &c->red_bytes, (size_t)np * sizeof(fognet_job_stats), "reduction partials");
    if (rc) return rc;
  }
  hipError_t e = fognet::launch_reduce_stats(stats, R, out, static_cast<fognet_job_stats*>(c->red),
                                             (hipStream_t)stream);
  return e == hipSuccess ? FOGNET_OK : hip_fail(c, e, "reduce launch");
}

int fognet_gen_trace_dev(fognet_ctx* c, const fognet_gen_params* p, int64_t r0, int32_t R, int32_t T, int32_t N,
                         int64_t* arrive_tick, int32_t* req_mips, int32_t* mips, int64_t* dl_tick, int64_t* ul_tick,
                         int64_t* init_adv_tick, void* stream) {
  if (!c || !p) return FOGNET_ERR_ARG;
  if (R < 0 || T < 0 || N <= 0 || r0 < 0) return fail(c, FOGNET_ERR_ARG, "bad sizes");
  if (p->req_lo < 0 || p->req_hi < p->req_lo) return fail(c, FOGNET_ERR_ARG, "bad req range");
  if (R > 0 && (!p->mean_gap_ticks || !p->lat_scale || !mips || !dl_tick || !ul_tick || !init_adv_tick ||
                (T > 0 && (!arrive_tick || !req_mips))))
    return fail(c, FOGNET_ERR_ARG, "null pointer");
  int rc = set_device(c);
  if (rc) return rc;
  hipError_t e = fognet::launch_gen_trace(*p, r0, R, T, N, arrive_tick, req_mips, mips, dl_tick, ul_tick,
                                          init_adv_tick, (hipStream_t)stream);
  return e == hipSuccess ? FOGNET_OK : hip_fail(c, e, "tracegen launch");
}

}  // extern "C"

// ---------------------------------------------------------------- RCCL stats exchange
// RCCL's C API, resolved with dlsym on first use (no link-time dependency).
namespace {

typedef struct {
  char internal[FOGNET_COMM_ID_BYTES];
} RcclId;
typedef void* RcclComm;
enum { kRcclInt8 = 0, kRcclUint8 = 1, kRcclInt64 = 4, kRcclSum = 0 };

struct Rccl {
  int (*get_unique_id)(RcclId*) = nullptr;
  int (*comm_init_rank)(RcclComm*, int, RcclId, int) = nullptr;
  int (*comm_destroy)(RcclComm) = nullptr;
  int (*all_gather)(const void*, void*, size_t, int, RcclComm, hipStream_t) = nullptr;
  int (*all_reduce)(const void*, void*, size_t, int, int, RcclComm, hipStream_t) = nullptr;
  const char* (*error_string)(int) = nullptr;
  bool ok = false;
  std::string why;
};

Rccl& rccl() {
  static Rccl r = [] {
    Rccl x;
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) {
      x.why = std::string("cannot load librccl: ") + dlerror();
      return x;
    }
    x.get_unique_id = reinterpret_cast<decltype(x.get_unique_id)>(dlsym(h, "ncclGetUniqueId"));
    x.comm_init_rank = reinterpret_cast<decltype(x.comm_init_rank)>(dlsym(h, "ncclCommInitRank"));
    x.comm_destroy = reinterpret_cast<decltype(x.comm_destroy)>(dlsym(h, "ncclCommDestroy"));
    x.all_gather = reinterpret_cast<decltype(x.all_gather)>(dlsym(h, "ncclAllGather"));
    x.all_reduce = reinterpret_cast<decltype(x.all_reduce)>(dlsym(h, "ncclAllReduce"));
    x.error_string = reinterpret_cast<decltype(x.error_string)>(dlsym(h, "ncclGetErrorString"));
    x.ok = x.get_unique_id && x.comm_init_rank && x.comm_destroy && x.all_gather && x.all_reduce && x.error_string;
    if (!x.ok) x.why = "librccl lacks the NCCL collective API";
    return x;
  }();
  return r;
}

int rccl_fail(fognet_ctx* c, int e, const char* what) {
  return fail(c, FOGNET_ERR_DEVICE, std::string(what) + ": " + rccl().error_string(e));
}

}  // namespace

struct fognet_comm {
  RcclComm comm = nullptr;
  int32_t world = 0, rank = 0;
  int device = -1;
  void* buf = nullptr;  // [world] job records
};

extern "C" {

int fognet_comm_unique_id(uint8_t id[FOGNET_COMM_ID_BYTES]) {
  if (!id) return FOGNET_ERR_ARG;
  Rccl& r = rccl();
  if (!r.ok) return FOGNET_ERR_UNSUPPORTED;
  RcclId x;
  if (r.get_unique_id(&x) != 0) return FOGNET_ERR_DEVICE;
  memcpy(id, x.internal, FOGNET_COMM_ID_BYTES);
  return FOGNET_OK;
}

int fognet_comm_create(fognet_ctx* c, int32_t world, int32_t rank, const uint8_t id[FOGNET_COMM_ID_BYTES],
                       fognet_comm** out) {
  if (!c || !out || !id || world <= 0 || rank < 0 || rank >= world) return fail(c, FOGNET_ERR_ARG, "comm: bad world/rank");
  *out = nullptr;
  Rccl& r = rccl();
  if (!r.ok) return fail(c, FOGNET_ERR_UNSUPPORTED, r.why);
  int rc = set_device(c);
  if (rc) return rc;
  fognet_comm* m = new fognet_comm;
  m->world = world;
  m->rank = rank;
  m->device = c->device;
  RcclId x;
  memcpy(x.internal, id, FOGNET_COMM_ID_BYTES);
  const int e = r.comm_init_rank(&m->comm, world, x, rank);
  if (e != 0) {
    delete m;
    return rccl_fail(c, e, "ncclCommInitRank");
  }
  const hipError_t he = hipMalloc(&m->buf, (size_t)world * sizeof(fognet_job_stats));
  if (he != hipSuccess) {
    r.comm_destroy(m->comm);
    delete m;
    return hip_fail(c, he, "hipMalloc comm buffer");
  }
  *out = m;
  return FOGNET_OK;
}

void fognet_comm_destroy(fognet_comm* m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  if (m->comm) rccl().comm_destroy(m->comm);
  if (m->buf) (void)hipFree(m->buf);
  delete m;
}

int fognet_allreduce_stats(fognet_ctx* c, fognet_comm* m, fognet_job_stats* inout, int64_t* hist, void* stream) {
  if (!c || !m || !inout) return fail(c, FOGNET_ERR_ARG, "allreduce_stats: null argument");
  if (m->device != c->device) return fail(c, FOGNET_ERR_ARG, "allreduce_stats: comm and context on different devices");
  int rc = set_device(c);
  if (rc) return rc;
  Rccl& r = rccl();
  hipStream_t s = (hipStream_t)stream;
  const size_t sz = sizeof(fognet_job_stats);
  unsigned char* const buf = static_cast<unsigned char*>(m->buf);
  hipError_t he = hipMemcpyAsync(buf + (size_t)m->rank * sz, inout, sz, hipMemcpyHostToDevice, s);
  if (he != hipSuccess) return hip_fail(c, he, "allreduce_stats copy-in");
  int e = r.all_gather(buf + (size_t)m->rank * sz, buf, sz, kRcclUint8, m->comm, s);  // in place
  if (e != 0) return rccl_fail(c, e, "ncclAllGather");
  if (hist) {
    e = r.all_reduce(hist, hist, (size_t)FOGNET_HIST_METRICS * FOGNET_HIST_BINS, kRcclInt64, kRcclSum, m->comm, s);
    if (e != 0) return rccl_fail(c, e, "ncclAllReduce");
  }
  std::string recs((size_t)m->world * sz, '\0');
  he = hipMemcpyAsync(&recs[0], buf, recs.size(), hipMemcpyDeviceToHost, s);
  if (he == hipSuccess) he = hipStreamSynchronize(s);
  if (he != hipSuccess) return hip_fail(c, he, "allreduce_stats copy-out");
  fognet_job_stats acc;
  fognet_job_stats_init(&acc);
  for (int32_t k = 0; k < m->world; ++k) {  // rank order: exact and identical on every rank
    fognet_job_stats rec;
    memcpy(&rec, recs.data() + (size_t)k * sz, sz);
    fognet_job_stats_merge(&acc, &rec);
  }
  *inout = acc;
  return FOGNET_OK;
}

}  // extern "C"
