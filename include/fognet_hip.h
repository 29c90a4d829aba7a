/*
 * fognet_hip.h — C ABI of libfognet_hip, the MI355X (gfx950) engine for
 * FogNetSim++'s offload-decision hot path.
 *
 * Reference interfaces replaced (paths relative to the FogNetSim++ tree):
 *   - the broker's allocation argmin, BrokerBaseApp3::sendPubAck(status=false),
 *     src/mqttapp/BrokerBaseApp3.cc:265-304 (decision core :267-281)
 *       -> fognet_decide / fognet_decide_batch_dev;
 *   - the v2 broker's local-first / "max-MIPS" forward, BrokerBaseApp2.cc:180-192
 *     and :235-286 -> fognet_decide_v2 / fognet_decide_v2_batch_dev;
 *   - the fog node's task arrival, ComputeBrokerApp3::processPacket,
 *     src/mqttapp/ComputeBrokerApp3.cc:269-320, its completion + advertisement,
 *     ComputeBrokerApp3::releaseResource / advertiseMIPS, :224-256 / :205-222,
 *     and the broker's view update on each advertisement,
 *     BrokerBaseApp3.cc:123-130 -> fognet_run_batch[_dev] (R independent
 *     trace replays of the whole decide -> queue -> complete -> advertise loop);
 *   - the queueTime statistic (ComputeBrokerApp3.cc:238, ComputeBrokerApp3.ned:45-46)
 *     -> fognet_rep_stats, reduced on the device (fognet_reduce_stats_dev);
 *   - the ack relay and the users' latency signals (BrokerBaseApp3.cc:143,
 *     164-198; mqttApp2.cc:252-291) -> fognet_user_stats_dev.
 *
 * Conventions
 *   - Every entry point returns a fognet_status; no exception crosses the ABI.
 *     fognet_last_error() gives the message of the last failure on a context.
 *   - The caller owns every buffer.  *_dev entry points take device pointers
 *     (hipMalloc'd, or torch.cuda tensors) and enqueue on the given hipStream_t
 *     (NULL = default stream); the others take host pointers and copy.
 *   - Streams.  A *_dev call only enqueues: every kernel, clear and copy it
 *     issues goes to hip_stream and to no other stream, and the call returns
 *     without waiting for the device.  The one exception is a call that has to
 *     grow the context's workspace (the first job of a size larger than any
 *     before it on that context): it frees the old allocation, which waits
 *     for the device.  The calls on one context share that workspace, so
 *     consecutive *_dev calls on one context must be ordered with respect to
 *     each other: enqueue them on one stream, or order the streams with
 *     events (a statistics or reduction pass after its replay likewise).
 *     Contexts share nothing; two contexts may run on two streams at once.
 *     The host-pointer entry points (fognet_decide, fognet_decide_window,
 *     fognet_decide_v2, fognet_run_batch) run on a private non-blocking
 *     stream of the context and return once their results are in the caller's
 *     memory.  The decisions wait for that stream alone, not for the
 *     caller's streams; fognet_run_batch frees its staging buffers before
 *     it returns, which waits for the whole device.  fognet_run_batch
 *     uses the workspace as well: do not call it while a *_dev job of the
 *     same context is executing.  (A job that is enqueued but still waits
 *     behind other work of its stream is unaffected: every job initialises
 *     what it reads of the workspace when it starts.)
 *   - A fognet_ctx is not thread-safe; use one per host thread (OMNeT++'s
 *     sequential kernel is single-threaded anyway).
 *   - Deterministic: identical inputs give bit-identical outputs.
 *   - Time is OMNeT++ 4.6 simtime_t raw int64 at scale 1e-12 s ("ticks").
 */
#ifndef FOGNET_HIP_H
#define FOGNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FOGNET_ABI_VERSION 10
#define FOGNET_TICKS_PER_SECOND 1000000000000LL

/* Latency histograms (device-side statistics, summed over replications; the
 * only data the multi-GPU path all-reduces over RCCL together with energy).
 * Metric 0 = queueTime (ComputeBrokerApp3.cc:238, queued tasks only): q = the
 * whole part of the recorded value in ms (the emitted raw simtime_t * 1e-12,
 * see "Reference signal values" below); metric 1 = response (completion tick -
 * publish tick at the broker): q = ticks / 10^9 whole milliseconds.  A value
 * falls in bin 0 if q < 1, else min(63, floor(log2 q) + 1): bin b >= 1 holds
 * [2^(b-1), 2^b) ms. */
#define FOGNET_HIST_METRICS 2
#define FOGNET_HIST_BINS 64

typedef int64_t fognet_tick;
typedef struct fognet_ctx fognet_ctx;

typedef enum fognet_status {
    FOGNET_OK = 0,
    FOGNET_ERR_ARG = 1,         /* invalid argument / precondition (see fognet_run_batch)            */
    FOGNET_ERR_NO_NODES = 2,    /* n == 0: BrokerBaseApp3.cc:268 reads brokers[0] first (UB)           */
    FOGNET_ERR_DIV0 = 3,        /* advertised MIPS of node 0 is 0: BrokerBaseApp3.cc:268 SIGFPE        */
    FOGNET_ERR_STATE = 4,       /* scheduleAt on a scheduled selfMsg (ComputeBrokerApp3.cc:301): the
                                   reference's cRuntimeError is swallowed by processPacket's catch
                                   (:277,317), leaving the node busy with no completion pending;
                                   unreachable under the fognet_batch_in preconditions            */
    FOGNET_ERR_DEVICE = 5,      /* HIP runtime failure or no gfx950 device                             */
    FOGNET_ERR_OOM = 6,
    FOGNET_ERR_CAPACITY = 7,    /* v2 queue_capacity exceeded; a decision whose smallest advertised busy
                                   time is 2^32 - 1 s or more (the view keeps 32 bits, saturated: larger
                                   values only lose); EXT_LAT: an advertised busy time of 2^24 s or more */
    FOGNET_ERR_UNSUPPORTED = 8, /* configuration not implemented (e.g. N > 2^20, unknown policy)     */
    FOGNET_REF_ABORTED = 9,     /* replication status under FOGNET_FLAG_REF_ABORT: the reference run ends
                                   at a queueTime emission that overflows (ComputeBrokerApp3.cc:238; see
                                   "Reference signal values"); outputs are still written in full     */
    FOGNET_ERR_INTERNAL = 10    /* an internal invariant check of the replay failed (a library bug)   */
} fognet_status;

/* fognet_batch_in.flags */
#define FOGNET_FLAG_REF_ABORT 1 /* a replication the reference would abort (abort_tick set) gets status
                                   FOGNET_REF_ABORTED, so job reductions count it as failed, as the
                                   reference records no result for it; without the flag its status is
                                   FOGNET_OK and the continuation past the abort is the extension's */

typedef enum fognet_policy {
    FOGNET_POLICY_REF_V2 = 2,   /* BrokerBaseApp2: local-first, then the LAST node whose advertised MIPS
                                   exceeds node 0's, forwarded only if MIPSRequired < its MIPS
                                   (fognet_decide_v2; needs the broker's own MIPS)                 */
    FOGNET_POLICY_REF_V3 = 1,   /* BrokerBaseApp3: argmin(busy_j + req / mips_0), int division,
                                   strict '<' (ties -> lowest index), stale advertised view      */
    FOGNET_POLICY_EXT_LAT = 16, /* north-star cost, NOT in the reference (parity vs the oracle's
                                   restatement only): argmin over j of
                                   dl_j + adv_busy_j * 1e12 + (req / mips_j) * 1e12 ticks
                                   (int division by the node's OWN MIPS, exact int64 ticks,
                                   ties -> lowest index); same stale view and node model      */
    FOGNET_POLICY_EXT_HIER = 32 /* hierarchical brokers with mobility handoff (BASELINE.json C5), NOT
                                   in the reference (one flat broker, BrokerBaseApp3.cc:271-279):
                                   the nodes form regions of FOGNET_HIER_REGION_NODES consecutive
                                   indices, each with a regional broker; publish t reaches the
                                   broker of region[t] (the user's region when it publishes: a
                                   handoff changes it).  That broker applies BrokerBaseApp3's rule
                                   inside its region: the smallest (advertised busy, index).  If
                                   that busy exceeds hier_threshold_s the task is escalated to the
                                   parent broker, which applies the rule over ALL nodes, and
                                   reaches its node hier_up_tick later (the extra hop).  Adverts
                                   reach every broker with the node's uplink latency.  A direct
                                   task can reach a node before an escalated task decided earlier
                                   (it overtakes it inside the hop): the node serves in arrival
                                   order; any number of escalated tasks may be in flight at once
                                   (the node FIFO takes any length, ComputeBrokerApp3.cc:305-309).
                                   A replication that fails (status != OK) leaves the per-task
                                   outputs of escalated tasks still in flight at the error
                                   unwritten, like every task after the error.  Which tasks the
                                   parent decided is the optional output fognet_batch_out.escalated;
                                   fognet_user_stats_dev and fognet_node_stats_dev need it under
                                   this policy (they add the hop to those tasks' arrival).     */
} fognet_policy;

/* Region size of FOGNET_POLICY_EXT_HIER (node r * 1024 .. r * 1024 + 1023 form region r). */
#define FOGNET_HIER_REGION_NODES 1024

/* Outcome of one BrokerBaseApp2 decision (BrokerBaseApp2.cc:180-192, 235-286). */
typedef enum fognet_v2_action {
    FOGNET_V2_LOCAL = 3,     /* MIPSRequired < the broker's own MIPS: served locally (pubAck status 3)  */
    FOGNET_V2_FORWARD = 4,   /* pubAck status 4 + FognetMsgTask to *out_node                            */
    FOGNET_V2_DROPPED = 5,   /* pubAck status 4, MIPSRequired >= the chosen node's MIPS: no task sent   */
    FOGNET_V2_NO_NODES = 6   /* no compute broker registered: "no compute resource available" puback   */
} fognet_v2_action;

/* Reference signal values.  The reference emits its latency signals as
 * simtime_t values (OMNeT++ 4.6, scale 1e-12: a raw int64 t, recorded as the
 * double dbl() = t * 1e-12), and computes them with SimTime's double round
 * trips: SimTime(double d) = toInt64(1e12 * d), SimTime * double =
 * toInt64(t * d), toInt64(x) = floor(x + 0.5), a cRuntimeError outside int64.
 * The statistics keep exact moments of those RAW emitted values ("raw"):
 *   queueTime  (simTime() - SimTime(queueStartTime)) * 1000, queueStartTime =
 *              simTime().dbl() of the enqueue, a double (ComputeBrokerApp3.cc:238,
 *              306, Request.cc:26): raw = toInt64((double)(now -
 *              toInt64(1e12 * (a * 1e-12))) * 1000.0) for a task enqueued at tick a
 *              and started at tick now (the recorded value, raw * 1e-12, is in ms;
 *              it can be a few ulps off the exact tick difference, even negative
 *              for a task queued and started in the same tick);
 *   latency / latencyH1 / taskTime  (simTime() - timeCreated) * 1000 with
 *              timeCreated a simtime_t (mqttApp2.cc:260,272,282): raw = toInt64(d * 1000.0);
 *   delay      simTime() - creationTime (BrokerBaseApp3.cc:143): raw = d ticks (s).
 * An emission whose product leaves the int64 range (a queue time above ~9223 s)
 * throws in the reference.  At the user signals the exception is swallowed by
 * mqttApp2's catch and the emission is lost (fognet_moments.overflow).  At
 * queueTime it ENDS THE REFERENCE RUN: ComputeBrokerApp3::releaseResource emits
 * at ComputeBrokerApp3.cc:238 before it dequeues the next task (:240-250) and
 * nothing up to handleMessageWhenUp (:84-86) catches, so OMNeT++ stops at that
 * RELEASERESOURCE event.  The engine reports that point per replication
 * (fognet_rep_stats.abort_tick / abort_task) and, as a builder-defined
 * EXTENSION of the reference, keeps replaying past it: the emission is counted
 * (n_qtime_overflow) and left out of the moments and histograms, and the node
 * dequeues its next task as if the emit had returned.  What the reference
 * defines of an aborted replication is the prefix before that event: every
 * publish with arrive_tick <= abort_tick is decided (trace publishes precede
 * same-tick dynamic events), and every arrival, start and
 * completion at a tick < abort_tick has happened.  Everything later, and every
 * statistic that includes it, is the extension's.  Signed sums are two's
 * complement. */

/* Per-replication statistics.  Exact integer moments, split into uint64 limbs
 * ([lo, hi, top] = bits 0-63, 64-127, 128-191) so results are bit-reproducible. */
typedef struct fognet_rep_stats {
    int64_t n_tasks;          /* decisions made                                                   */
    int64_t n_queued;         /* node acks with status 4 ("task queued", :310-313)                 */
    int64_t n_started;        /* node acks with status 5                                          */
    int64_t last_tick;        /* latest RELEASERESOURCE tick (makespan)                           */
    int64_t queue_min_raw, queue_max_raw;     /* queueTime emissions: raw values (see above)       */
    int64_t resp_min_ticks, resp_max_ticks;   /* over all tasks: done - arrival at broker          */
    uint64_t queue_sum_lo, queue_sum_hi;      /* signed 128-bit sum of queueTime raw values        */
    uint64_t queue_sq_lo, queue_sq_hi;        /* bits 0-127 of the sum of their squares            */
    uint64_t resp_sum_lo, resp_sum_hi, resp_sq_lo, resp_sq_hi;
    int64_t events;           /* reference FES events this replay stands for (2N + 4 per task)    */
    int32_t max_pending;      /* max tasks assigned to one node whose completion advert had not
                                 reached the broker yet (ring occupancy)                          */
    int32_t status;           /* fognet_status of this replication                                */
    int64_t busy_s;           /* sum of service seconds (req / MIPS) over all tasks               */
    double energy_j;          /* node energy (builder-defined, not in the reference; 0 when no
                                 power model): sum over j in index order of
                                 P_busy_j * B_j + P_idle_j * ((H - B_j * 1e12) / 1e12), with
                                 B_j = node j's service seconds, H = last_tick (0 if no task);
                                 IEEE fp64, no fused multiply-add                                 */
    uint64_t queue_sq_top;    /* bits 128-191 of the queueTime sum of squares                     */
    int64_t n_qtime;          /* queueTime emissions in the moments (queued tasks that started)   */
    int64_t n_qtime_overflow; /* queueTime emissions the reference cannot make (simtime overflow) */
    /* The reference's abort point (see "Reference signal values"): the RELEASERESOURCE
     * tick at which the first overflowing queueTime emission throws and the index of the
     * task it would have started; INT64_MAX / -1 when the reference run completes.
     * Several overflowing emissions at that tick (different nodes): abort_task is the LOWEST
     * task index among them.  The reference, run under a stand-in kernel, throws at the one
     * whose RELEASERESOURCE timer was inserted first (FES order: the node whose running
     * service started earlier), which can be a higher index: in the recording
     * overflow_same_tick_high_first (tests/golden/ref_v3_edges.json) it throws at task 5
     * while task 3 overflows at the same tick, and this field is 3.  The tick, and so the
     * reference-defined prefix, are the same either way; the oracle's stop-at-abort mode
     * names the reference's task. */
    int64_t abort_tick;
    int64_t abort_task;
} fognet_rep_stats;

/* Job-level statistics: the exact sum of any set of fognet_rep_stats.  Sums
 * are 192-bit integers (limbs [0] = least significant; queue_sum two's
 * complement), so combining is associative and the integer fields do not
 * depend on how replications were sharded over GPUs.  Mean/stddev in ms:
 * queueTime sum * 1e-12 / n_qtime, response sum / n_tasks / 1e9, etc. */
typedef struct fognet_job_stats {
    int64_t n_reps, n_failed;
    int64_t n_tasks, n_queued, n_started;
    int64_t last_tick;
    int64_t queue_min_raw, queue_max_raw, resp_min_ticks, resp_max_ticks;
    uint64_t queue_sum[3], queue_sq[3], resp_sum[3], resp_sq[3];
    int64_t events;
    int64_t max_pending;
    int64_t busy_s;
    double energy_j;          /* fp64 sum over replications: fixed tree order on one device, rank
                                 order across GPUs; differs from another sharding's sum by
                                 rounding only (within 1e-9 relative)                            */
    int64_t n_qtime, n_qtime_overflow;
    int64_t n_ref_aborted;    /* replications the reference would have aborted (abort_tick set),
                                 status OK or FOGNET_REF_ABORTED (the latter also in n_failed) */
} fognet_job_stats;

/* R trace replays of T tasks over N fog nodes, SoA, row-major [R][T] / [R|1][N]. */
typedef struct fognet_batch_in {
    int32_t R, T, N;
    int32_t policy;           /* fognet_policy                                                    */
    int32_t node_stride;      /* 0: node params shared by all replications; N: one row each       */
    int32_t ring_capacity;    /* per-node pending-task ring of the register-resident replay kernel
                                 (N <= 256), power of two in [2, 2^15] (0 = default 2048).  Not a
                                 limit on the inputs: a replication with a node past it (or with a
                                 service time past min(2^24 / ring_capacity, 255) s, or a task
                                 reaching its node past 2^56 ticks, the 8-B ring entry's ranges) is
                                 replayed again from the start by the wide kernel, whose per-node
                                 chains are unbounded, inside the same call.  Only sizes the
                                 workspace (8 B per entry) and the common path.                  */
    const int64_t *arrive_tick;   /* [R][T] publish arrival at the broker, nondecreasing          */
    const int32_t *req_mips;      /* [R][T] MqttMsgPublish.MIPSRequired, >= 0                      */
    const int32_t *mips;          /* [R|1][N] node MIPS (> 0), CONNECT order = index order         */
    const int64_t *dl_tick;       /* [R|1][N] broker -> node delivery latency (>= 0)               */
    const int64_t *ul_tick;       /* [R|1][N] node -> broker delivery latency (>= 0)               */
    const int64_t *init_adv_tick; /* [R|1][N] arrival of the node's first advert at the broker;
                                     ul <= init_adv < arrive[0] (all adverts land before task 0)  */
    const double *p_busy_w;       /* [R|1][N] node power while serving, W (nullable: no energy)   */
    const double *p_idle_w;       /* [R|1][N] node power while idle, W (null iff p_busy_w is)     */
    /* Node-down extension (not one of the reference's scenarios): [R|1][N] tick at which
     * node j crashes (INT64_MAX = never; otherwise init_adv_tick <= down < 2^61), nullable.
     * INET lifecycle, ComputeBrokerApp3::handleNodeCrash (ComputeBrokerApp3.cc:423-427):
     * the node's RELEASERESOURCE timer is cancelled and the host drops arriving tasks;
     * the broker keeps its last advert.  The crash precedes every model event of its
     * tick.  Replays with crashes run on the wide kernel; not combinable with the power
     * model (ERR_UNSUPPORTED); not stored in trace files (fognet_io.h). */
    const int64_t *down_tick;
    /* FOGNET_POLICY_EXT_HIER only (ignored otherwise): [R][T] region of each publish's
     * regional broker (0 <= region < ceil(N / FOGNET_HIER_REGION_NODES)), the busy seconds
     * above which a regional broker escalates, the extra latency of an escalated task. */
    const int32_t *region;
    int64_t hier_up_tick;
    int32_t hier_threshold_s;
    int32_t flags;            /* FOGNET_FLAG_* (0: none)                                           */
} fognet_batch_in;

/* Per-task status (fognet_batch_out.status). */
typedef enum fognet_task_status {
    FOGNET_TASK_QUEUED = 4,   /* node ack "task queued"   (ComputeBrokerApp3.cc:304-313)       */
    FOGNET_TASK_STARTED = 5,  /* node ack "task assigned" (ComputeBrokerApp3.cc:282-301)       */
    FOGNET_TASK_LOST = 9      /* reached a crashed node (down_tick): no ack, never served       */
} fognet_task_status;

typedef struct fognet_batch_out {
    int32_t *node;            /* [R][T] chosen node                                               */
    uint8_t *status;          /* [R][T] fognet_task_status: 5 started on arrival, 4 queued, 9 lost */
    int64_t *start_tick;      /* [R][T] service start (-1: never started, node-down only)         */
    int64_t *done_tick;       /* [R][T] completion (RELEASERESOURCE) tick (-1: never, node-down)  */
    fognet_rep_stats *stats;  /* [R], required.  node/status/start_tick/done_tick: all four, or all
                                 NULL for a statistics-only replay (fognet_run_batch_dev /
                                 fognet_run_batch only): the caller gets the records and the
                                 histogram; N > 256 (wide kernel) then writes nothing per task,
                                 N <= 256 keeps the per-task outputs in the context's workspace
                                 for its fused statistics pass                                 */
    double *node_energy_j;    /* [R][N] per-node energy (nullable; needs the power model)         */
    int64_t *hist;            /* [FOGNET_HIST_METRICS][FOGNET_HIST_BINS] job histogram, ADDED to
                                 (the caller zeroes it; nullable)                                 */
    uint8_t *escalated;       /* [R][T] nullable (needs the four per-task arrays: FOGNET_ERR_ARG with a
                                 statistics-only out).  FOGNET_POLICY_EXT_HIER: 1 for a decided task
                                 whose decision the parent broker took (its region's minimum above
                                 hier_threshold_s), whether or not the chosen node lies in the
                                 publish's own region and also when that node has crashed (status
                                 9); else 0.  Other policies: filled with 0.  Last member: a caller
                                 that zeroes the struct or initialises only the members above
                                 passes NULL and sees no change.                                  */
} fognet_batch_out;

/* Buffers.  What every *_dev entry point asks of, and leaves in, the caller's arrays
 * (tests/test_buffer_contract_gpu.py holds the library to each sentence):
 *   Alignment.  Every pointer needs only the natural alignment of its element type
 *     (8 B for int64 / double / the record structs, 4 B for int32, 1 B for status and
 *     escalated).
 *   Bounds.  Nothing outside [R][T] / [R|1][N] / [R] / [m] / hist is read or written,
 *     whatever T % 64, R % 4 (the v2 wavefronts) or R % 4096 (the reduction) are.
 *   Initialisation.  No output needs initialising, and none depends on what it held
 *     before the call, except hist, which is ADDED to (the caller zeroes it once).
 *   A failed replication (stats[r].status other than FOGNET_OK / FOGNET_REF_ABORTED) never
 *     touches its neighbours.  Its per-task rows and its node_energy_j row are undefined.
 *     Its record is written in full: status, and n_tasks, events and max_pending up to the
 *     failure; the other fields (and what it added to hist) cover the n_tasks publishes
 *     decided before the failure and are no result.  A replication refused before its first
 *     decision (n_tasks = 0: every precondition on the node parameters, and a bad publish
 *     in a chunk the replay checks before it decides) therefore has the empty-set values
 *     used throughout this header: counts and sums 0, energy_j 0.0, minima INT64_MAX,
 *     maxima (last_tick too) INT64_MIN, abort_tick = INT64_MAX, abort_task = -1.
 *     (fognet_replay_dev alone writes only the four fields named at its declaration;
 *     fognet_rep_stats_dev completes the record.)  Likewise fognet_v2_stats (every count 0
 *     for a replication refused before its first event).  fognet_user_stats_dev reads
 *     nothing of a failed replication's rows, wherever it failed: its fognet_user_stats
 *     holds the count == 0 values of fognet_moments in all four signals.
 *   The per-node records (fognet_node_stats_dev's [R][N], fognet_reduce_node_stats_dev's [N])
 *     obey every sentence above: 8-B alignment, nothing outside [R][N] / [N] touched, no
 *     initialisation needed; a failed replication's row is N empty records.
 *   The per-user records (fognet_per_user_stats_dev's [R][U], fognet_reduce_user_stats_dev's
 *     [U]) and n_unassigned [R] likewise: 8-B alignment (user_of: 4 B), nothing outside
 *     [R][U] / [U] / [R] touched, no initialisation needed; a failed replication's row is U
 *     empty records and its n_unassigned is 0.
 *   The signal vectors (fognet_signal_vectors_dev's offset [Rv][V + 1], time / value / task
 *     [Rv][cap], n_unassigned [Rv]) likewise: 8-B alignment (task: 4 B), nothing outside them
 *     touched, no initialisation needed; rows at and past offset[V] keep what they held; a
 *     failed replication's offsets are all 0 and none of its rows is written.
 *   The window records (fognet_window_stats_dev's [R][W], fognet_reduce_window_stats_dev's [W]),
 *     n_outside [R][2] and n_unassigned [R] likewise: 8-B alignment, nothing outside them
 *     touched, no initialisation needed; a failed replication's row is W empty records and
 *     its n_outside and n_unassigned are 0.
 *   escalated likewise: 1-B alignment, nothing outside [R][T] touched, no initialisation
 *     needed; a failed replication's row is undefined, like its other per-task rows.
 *   The assignment (fognet_replay_assigned_dev's and fognet_run_assigned_dev's assign [R][T])
 *     likewise: 4-B alignment, nothing outside [R][T] read; it is never written, unless the caller
 *     passes the same pointer as out->node, which then holds the same values afterwards.
 *   The group records (fognet_reduce_groups_dev's out [G], metrics [R][FOGNET_REP_METRICS], defined
 *     [R], n_ungrouped [1], group_of [R]) likewise: 8-B alignment (defined and group_of: 4 B), nothing
 *     outside them or stats [R] touched, no initialisation needed; a failed replication's metrics
 *     row is all INT64_MIN and its defined word 0. */

/* count / min / max / exact signed 128-bit sum and 192-bit sum of squares of a
 * signal's raw emitted values (min_raw = INT64_MAX, max_raw = INT64_MIN when
 * count == 0); overflow: emissions lost to the simtime_t range (see above). */
typedef struct fognet_moments {
    int64_t count, min_raw, max_raw;
    uint64_t sum_lo, sum_hi, sq_lo, sq_hi, sq_top;
    int64_t overflow;
} fognet_moments;

/* User-side signals of one replication, as raw emitted
 * values (see "Reference signal values"): delay in ticks (s), the others the
 * raw simtime_t of (simTime() - created) * 1000 (recorded value raw * 1e-12 ms):
 *   delay      broker `delay` (BrokerBaseApp3.cc:143): publish arrival at the
 *              broker - creation at the user, every publish
 *   latency    mqttApp2 on the relayed status-5 ack ("task assigned",
 *              mqttApp2.cc:257-265)
 *   latencyH1  on status-4 acks (mqttApp2.cc:269-277): the broker's own pubAck
 *              (BrokerBaseApp3.cc:145-150) for every publish, plus the node's
 *              relayed "task queued" ack
 *   taskTime   on the relayed status-6 ack ("performed", mqttApp2.cc:279-291)
 * Acks travel node -> broker (ul_k), are relayed to the request's user
 * (BrokerBaseApp3.cc:164-198) and arrive one user downlink later.  Message
 * ids are assumed unique (the reference matches them with strcmp). */
typedef struct fognet_user_stats {
    fognet_moments delay, latency, latencyH1, taskTime;
} fognet_user_stats;

/* Statistics of ONE fog node in one replication (or, reduced, in one job): what the
 * reference records per ComputeBroker module (ComputeBrokerApp3.ned:45-46).  A task is
 * COMPLETED when its done_tick >= 0 (a node-down task that never completes has -1 and adds
 * nothing to busy_s, resp or last_tick; a status-4 task with start_tick >= 0 still emits
 * its queueTime).  Empty record: counts and sums 0, min_raw = INT64_MAX, max_raw =
 * last_tick = INT64_MIN.  The exact merge of a replication's N records is its
 * fognet_rep_stats: n_tasks, n_queued, n_started, busy_s sum; last_tick is the maximum;
 * queue.{count, overflow} are n_qtime / n_qtime_overflow; the queue and resp limbs and
 * extrema are the record's queue_* / resp_* (resp_sq_{lo,hi}: bits 0-127 of resp.sq). */
typedef struct fognet_node_stats {
    int64_t n_tasks;     /* decided publishes whose chosen node is this one                   */
    int64_t n_queued;    /* ... with status 4                                                  */
    int64_t n_started;   /* ... with status 5                                                  */
    int64_t n_lost;      /* ... with status 9 (node-down)                                      */
    int64_t busy_s;      /* service seconds req / MIPS_k (int division) of its COMPLETED tasks */
    int64_t last_tick;   /* latest completion tick on this node; INT64_MIN if none             */
    fognet_moments queue;/* this module's queueTime emissions, raw values ("Reference signal
                            values"): status-4 tasks that started, enqueued at arrive + dl_k
                            (+ hier_up_tick for an escalated task), started at start_tick;
                            overflow = emissions the reference throws on                       */
    fognet_moments resp; /* done_tick - arrive_tick (ticks) of its completed tasks; overflow 0  */
} fognet_node_stats;     /* 192 B, 8-B aligned */

/* ---- v2 model replay: BrokerBaseApp2 + ComputeBrokerApp2,
 * the modules simulations/example/wirelessNet.ini:56,62 select.  The broker
 * keeps its own MIPS pool with a single RELEASERESOURCE timer
 * (BrokerBaseApp2.cc:205-233, 382-406) and forwards to the LAST node whose
 * advertised MIPS exceeds node 0's (:235-271); a node reserves MIPS for
 * requiredTime and runs a 10-ms advert/release timer (ComputeBrokerApp2.cc:
 * 202-318).  Deadlines are doubles compared with simTime().dbl() = ticks *
 * 1e-12, exactly as the reference does (their rounding decides releases). */
#define FOGNET_V2_MAX_NODES 16384 /* node j on lane j % 64, slot j / 64 (up to 256 per lane) */
/* Device workspace of a v2 replay (fognet_run_v2_dev, allocated and kept by the context): 64 B per
 * (replication, node slot, queue entry) plus R * T B, i.e. R * S * queue_capacity * 64 B with S = N
 * rounded up to 64 x a power of two -- at N = 4096 and the default capacity 256, 64 MiB per replication
 * (128 MiB at N = 8192, 256 MiB at N = 16384).  Above 256 nodes (NPL >= 8) each node's record lives in
 * per-lane scratch memory. */

typedef enum fognet_v2_task_status {
    FOGNET_V2_ST_LOCAL = 3,      /* reserved in the broker's own pool (pubAck 3)                   */
    FOGNET_V2_ST_FORWARDED = 4,  /* task sent, still in flight when the run stopped                */
    FOGNET_V2_ST_DROPPED = 5,    /* MIPSRequired >= the chosen node's advertised MIPS: no task sent */
    FOGNET_V2_ST_NO_NODES = 6,   /* no compute broker registered                                   */
    FOGNET_V2_ST_ACCEPTED = 7,   /* reserved at the node (ComputeBrokerApp2.cc:269-295)             */
    FOGNET_V2_ST_REJECTED = 8    /* MIPSRequired >= the node's remaining MIPS (:299-306)            */
} fognet_v2_task_status;

typedef struct fognet_v2_in {
    int32_t R, T, N;              /* N <= FOGNET_V2_MAX_NODES                                      */
    int32_t node_stride;          /* 0: node parameters shared; N: one row per replication         */
    int32_t queue_capacity;       /* per-node capacity of each message queue and of the
                                     reservation list, power of two (0 = default 256)              */
    int32_t pad;
    const int64_t *arrive_tick;   /* [R][T] publish arrival at the broker, nondecreasing           */
    const int32_t *req_mips;      /* [R][T] MIPSRequired                                           */
    const int32_t *broker_mips;   /* [R] BrokerBaseApp2 par("MIPS")                                */
    const double *required_time_s;/* [R] MqttMsgPublish.requiredTime (mqttApp2.cc:372: 0.01)      */
    const int64_t *stop_tick;     /* [R] sim-time-limit: events at >= stop are not run (<= 2^53)   */
    const int32_t *mips;          /* [R|1][N] ComputeBrokerApp2 par("MIPS")                        */
    const int64_t *dl_tick;       /* [R|1][N] broker -> node latency                               */
    const int64_t *ul_tick;       /* [R|1][N] node -> broker latency                               */
    const int64_t *first_adv_tick;/* [R|1][N] first ADVERTISEMIPS firing (CONNACK + 0.01 s)        */
} fognet_v2_in;

typedef struct fognet_v2_stats {
    int64_t n_tasks, n_local, n_forwarded, n_accepted, n_rejected, n_dropped, n_no_nodes;
    int64_t n_released_broker;    /* broker timer releases (BrokerBaseApp2.cc:382-406)            */
    int64_t n_inflated;           /* ... of forwarded requests, credited to the broker's own pool  */
    int64_t n_released_node;      /* node releases (ComputeBrokerApp2.cc:222-245)                 */
    int64_t n_relayed;            /* status-6 acks that found their request at the broker         */
    int64_t events;               /* events processed (cancelled timers excluded)                  */
    int64_t node_mips_final_sum;
    int32_t broker_mips_final;
    int32_t status;               /* fognet_status of the replication                              */
} fognet_v2_stats;

typedef struct fognet_v2_out {
    int32_t *node;                /* [R][T] chosen node, -1: served locally / no node              */
    uint8_t *status;              /* [R][T] fognet_v2_task_status (0: not published before stop)  */
    int64_t *start_tick;          /* [R][T] reservation tick, -1 if never reserved                 */
    int64_t *done_tick;           /* [R][T] release tick of the reservation, -1 if not released    */
    fognet_v2_stats *stats;       /* [R]                                                           */
} fognet_v2_out;

/* R v2 replays on the device (device pointers; enqueued on hip_stream). */
int fognet_run_v2_dev(fognet_ctx *ctx, const fognet_v2_in *in, fognet_v2_out *out, void *hip_stream);

/* Synthetic trace recipe, generated on the device.
 * Replication r uses Philox4x32-10 key (seed, r); see DESIGN.md §Trace generator. */
typedef struct fognet_gen_params {
    uint32_t seed;
    int32_t req_lo, req_hi;       /* req ~ U_int[req_lo, req_hi]                                  */
    int32_t pad;
    const double *mean_gap_ticks; /* [R] exponential inter-arrival mean per replication (device)  */
    const int64_t *lat_scale;     /* [R] latency multiplier per replication (device)              */
} fognet_gen_params;

int fognet_abi_version(void);
const char *fognet_status_string(int status);

/* Context: binds a HIP device (gfx950 required), owns the replay workspace. */
int fognet_create(fognet_ctx **out, int hip_device);
void fognet_destroy(fognet_ctx *ctx);
const char *fognet_last_error(const fognet_ctx *ctx);

/* Scalar drop-in for BrokerBaseApp3.cc:267-281 (the OMNeT++ adapter's call,
 * INTEGRATION.md §1): host arrays of the broker's advertised view
 * (Broker::busyTime, Broker::MIPS in CONNECT order); evaluated on the device
 * with the reference's exact fp64 arithmetic.  policy: FOGNET_POLICY_REF_V3.
 * One kernel launch per call (views of <= 256 nodes travel in the kernel
 * arguments, larger ones in one DMA copy; the result is written to mapped
 * host memory) and one stream synchronisation. */
int fognet_decide(fognet_ctx *ctx, int policy, int32_t n, const double *adv_busy,
                  const int32_t *adv_mips, int32_t req_mips, int32_t *out_node);

/* The publishes of one window decided together: m requests against ONE view
 * (the broker's view only changes when an advert arrives, BrokerBaseApp3.cc:
 * 123-130, so every publish between two adverts sees the same view).  Equals
 * m fognet_decide calls on that view; one launch, one synchronisation.
 * out_node [m] (host).  Returns the first failing request's status. */
int fognet_decide_window(fognet_ctx *ctx, int policy, int32_t n, const double *adv_busy,
                         const int32_t *adv_mips, int32_t m, const int32_t *req_mips, int32_t *out_node);

/* M independent decisions, device pointers: adv_busy/adv_mips [M][n], req [M],
 * out_node [M], out_status [M] (fognet_status per query, nullable). */
int fognet_decide_batch_dev(fognet_ctx *ctx, int policy, int64_t m, int32_t n,
                            const double *adv_busy, const int32_t *adv_mips, const int32_t *req,
                            int32_t *out_node, int32_t *out_status, void *hip_stream);

/* Drop-in for the v2 broker's allocation (BrokerBaseApp2.cc:180-192 and
 * sendPubAck(status=false) :235-286): host arrays of the advertised MIPS view
 * adv_mips[n] (Broker::MIPS, updated by adverts :128-136), the broker's own
 * remaining MIPS (par MIPS minus local reservations) and MIPSRequired.
 * *out_action: fognet_v2_action; *out_node: chosen node, -1 for LOCAL/NO_NODES.
 * Evaluated on the device. */
int fognet_decide_v2(fognet_ctx *ctx, int32_t n, const int32_t *adv_mips, int32_t local_mips,
                     int32_t req_mips, int32_t *out_node, int32_t *out_action);

/* M independent v2 decisions, device pointers: adv_mips [M][n], local_mips [M],
 * req [M], out_node [M], out_action [M]. */
int fognet_decide_v2_batch_dev(fognet_ctx *ctx, int64_t m, int32_t n, const int32_t *adv_mips,
                               const int32_t *local_mips, const int32_t *req, int32_t *out_node,
                               int32_t *out_action, void *hip_stream);

/* Batched replay engine.  *_dev: every pointer in in/out is a device pointer
 * (the structs themselves are host memory).  Returns FOGNET_OK once enqueued;
 * per-replication failures are reported in stats[r].status. */
int fognet_run_batch_dev(fognet_ctx *ctx, const fognet_batch_in *in, fognet_batch_out *out,
                         void *hip_stream);
/* The two stages fognet_run_batch_dev enqueues, exposed so callers can time or
 * overlap them: the replay kernel (decisions, node queues, adverts; fills
 * node/status/start/done and stats[r].{status,n_tasks,max_pending,events}) and
 * the statistics pass over its outputs (the remaining stats fields). */
int fognet_replay_dev(fognet_ctx *ctx, const fognet_batch_in *in, fognet_batch_out *out, void *hip_stream);
int fognet_rep_stats_dev(fognet_ctx *ctx, const fognet_batch_in *in, fognet_batch_out *out, void *hip_stream);
/* Host-buffer variant: copies in, replays, copies out, synchronises.  Returns
 * the first non-OK replication status, if any. */
int fognet_run_batch(fognet_ctx *ctx, const fognet_batch_in *in, fognet_batch_out *out);

/* Assigned replay: the node model under the CALLER's decisions.  Task i of replication r goes
 * to node assign[r][i] (device, [R][T]); no broker decides, so policy, ring_capacity, region and
 * the hier_* fields of `in` are not read.  Read: R, T, N, node_stride, arrive_tick, req_mips,
 * mips, dl_tick, ul_tick, init_adv_tick (its preconditions only), flags, and p_busy_w / p_idle_w /
 * down_tick as fognet_run_batch_dev reads them.
 * The node model (ComputeBrokerApp3.cc:269-320), with k = assign[i],
 * s = (req_i / mips_k) * 10^12 ticks (int division), a = arrive_i + dl_k and p the previous task
 * of the trace on node k: the first task on a node has status 5 and start = a; otherwise start =
 * max(a, done_p), and status is 5 iff a > done_p, or a == done_p and dl_k < s_p (the completion's
 * timer was then inserted before the arrival event), else 4; done = start + s.
 * down_tick: a task with a >= down_k has status 9, start = done = -1 and takes no place in the
 * queue; a computed start >= down_k becomes -1, and so does a computed done >= down_k (the crash
 * precedes its tick's events and cancels the timer).
 * stats[r].max_pending: the maximum over tasks of 1 + the earlier tasks on the same node whose
 * completion advert (done + ul_k) has not reached the broker strictly before arrive_i (a task that
 * never completes stays pending); stats[r].events: 2N + 4 per task, 2 for a task that never
 * completes.
 * Written: all four per-task arrays (required; out->node receives the assignment and may be the
 * same pointer as assign), escalated (if given: 0), stats[r].{status, n_tasks, max_pending,
 * events}; fognet_run_assigned_dev completes the record, hist and node_energy_j as
 * fognet_run_batch_dev does.  Afterwards the same `in` with policy = FOGNET_POLICY_REF_V3 serves
 * fognet_node_stats_dev, fognet_per_user_stats_dev, fognet_user_stats_dev and
 * fognet_signal_vectors_dev.
 * A replication with a bad input is refused as a whole, before its first decision: status
 * FOGNET_ERR_ARG and the empty-set record (n_tasks = 0, events = 0; "Buffers" above); its
 * neighbours are untouched.  Bad inputs: an assign entry outside [0, N), decreasing arrive_tick,
 * negative req, mips <= 0, the init_adv_tick / down_tick preconditions of fognet_batch_in, an
 * arrival past 2^61 ticks, and a task that starts with a service time of 2^22 s or more or a
 * completion past 2^61 ticks (intermediate sums saturate, they never wrap).
 * Refused calls: a statistics-only `out`, a NULL assign with R * T > 0, NULL stats
 * (FOGNET_ERR_ARG); N > 2^20, the power model together with down_tick (FOGNET_ERR_UNSUPPORTED).
 * R = 0 and T = 0 succeed.  Both calls only enqueue and use the context's workspace (8 B per
 * task, 4 B per replication and node; 28 B more per replication and node above
 * FOGNET_ASSIGNED_LDS_NODES nodes).  The trace is walked in tiles of FOGNET_ASSIGNED_TILE tasks.
 * FOGNET_ASSIGNED=hbm (environment, testing): the per-node counts and carries live in the
 * workspace for every N, as they do above FOGNET_ASSIGNED_LDS_NODES nodes; the results are
 * identical.  FOGNET_ASSIGNED_STAGES=1 (timing only): stop after the validation and count stage;
 * no output is written then. */
#define FOGNET_ASSIGNED_TILE 64
#define FOGNET_ASSIGNED_LDS_NODES 1024
int fognet_replay_assigned_dev(fognet_ctx *ctx, const fognet_batch_in *in, const int32_t *assign,
                               fognet_batch_out *out, void *hip_stream);
int fognet_run_assigned_dev(fognet_ctx *ctx, const fognet_batch_in *in, const int32_t *assign,
                            fognet_batch_out *out, void *hip_stream);

/* User-side signals from a finished replay (fognet_replay_dev or
 * fognet_run_batch_dev on the same stream): device pointers in `in` (trace,
 * node parameters) and `out` (node, status, done_tick, stats) plus the
 * publishing users' links user_ul_tick (user -> broker) and user_dl_tick
 * (broker -> user): [R] (one user per replication, user_per_task = 0) or
 * [R][T] (per task, = 1).  Writes user_stats [R] (device): record r covers
 * replication r's first stats[r].n_tasks publishes; a failed replication (status
 * other than FOGNET_OK / FOGNET_REF_ABORTED) gets the count == 0 record in all four
 * signals, and none of its per-task rows or link entries is read (a
 * FOGNET_REF_ABORTED one keeps its full record).  The signals are a closed form of
 * the per-task outputs that holds where every node ack leaves at arrive_tick +
 * dl_k: FOGNET_POLICY_REF_V3 and FOGNET_POLICY_EXT_LAT, with or without down_tick.
 * FOGNET_POLICY_EXT_HIER with out->escalated (the replay's flags): the node ack of task
 * i leaves at arrive_tick + dl_k + in->hier_up_tick * escalated[i] (the hop; the broker's
 * own pubAck, delay and taskTime, which goes by done_tick, do not move).  Refused:
 * FOGNET_POLICY_EXT_HIER with out->escalated NULL (FOGNET_ERR_UNSUPPORTED, before
 * anything else is checked and with nothing written: an escalated task reaches its
 * node hier_up_tick later, so do its acks, and the other per-task outputs do not say
 * which tasks were escalated).  The policy is the caller's word: EXT_HIER outputs passed
 * under another policy are computed as if no task had been escalated (escalated is
 * not read then). */
int fognet_user_stats_dev(fognet_ctx *ctx, const fognet_batch_in *in, const fognet_batch_out *out,
                          const int64_t *user_ul_tick, const int64_t *user_dl_tick, int32_t user_per_task,
                          fognet_user_stats *user_stats, void *hip_stream);

/* Per-node statistics from a finished replay (fognet_run_batch_dev, or fognet_replay_dev
 * followed by fognet_rep_stats_dev, on the same stream): device pointers in `in`
 * (arrive_tick, req_mips, mips, dl_tick) and `out` (node, status, start_tick, done_tick,
 * stats[r].{n_tasks,status}).  Writes node_stats [R][N] (device): row r holds the records
 * of replication r's nodes over its first stats[r].n_tasks publishes; a failed
 * replication (status other than FOGNET_OK / FOGNET_REF_ABORTED) gets N empty records
 * and nothing of its per-task rows is read.  FOGNET_POLICY_REF_V3 and
 * FOGNET_POLICY_EXT_LAT, with or without down_tick; FOGNET_POLICY_EXT_HIER with
 * out->escalated (the replay's flags): task i is enqueued at arrive_tick + dl_k +
 * in->hier_up_tick * escalated[i].  Refused: FOGNET_POLICY_EXT_HIER with out->escalated
 * NULL (FOGNET_ERR_UNSUPPORTED: an escalated task reaches its node hier_up_tick later, and
 * the other per-task outputs do not say which tasks were escalated), a statistics-only
 * `out` (FOGNET_ERR_ARG) and a NULL node_stats with R * N > 0 (FOGNET_ERR_ARG).  Under the
 * other policies escalated is not read.
 * FOGNET_NODE_STATS=hbm (environment, testing): the accumulators are the caller's
 * records for every N, as they are above 256 nodes; the results are identical. */
int fognet_node_stats_dev(fognet_ctx *ctx, const fognet_batch_in *in, const fognet_batch_out *out,
                          fognet_node_stats *node_stats, void *hip_stream);
/* Job reduction of the per-node records (device pointers): out[j] = the exact merge of
 * node_stats[r][j] over the replications with stats[r].status == FOGNET_OK
 * (fognet_reduce_stats_dev's rule: REF_ABORTED and failed ones contribute nothing).
 * Any R; R = 0 gives N empty records.  Needs no workspace. */
int fognet_reduce_node_stats_dev(fognet_ctx *ctx, const fognet_node_stats *node_stats,
                                 const fognet_rep_stats *stats, int32_t R, int32_t N,
                                 fognet_node_stats *out, void *hip_stream);
/* Host-side identity and exact merge (ranks combine their [N] records after an all-gather). */
void fognet_node_stats_init(fognet_node_stats *s);
void fognet_node_stats_merge(fognet_node_stats *acc, const fognet_node_stats *other);

/* Per-user signals of a finished replay (fognet_run_batch_dev or fognet_replay_dev on the
 * same stream): device pointers in `in` (arrive_tick, dl_tick, ul_tick) and `out` (node,
 * status, done_tick, stats[r].{n_tasks,status}), the publishing user of every trace entry
 * user_of [R][T] (device; fognet_gen_trace_mqtt's user_of) and the users' links
 * user_ul_tick / user_dl_tick [U] shared by all replications (link_stride = 0) or [R][U]
 * (link_stride = U).  Writes per_user [R][U] (device): record [r][u] covers the publishes
 * i < stats[r].n_tasks of replication r with user_of[r][i] == u.  The four signals and
 * their emission rule are fognet_user_stats_dev's, task i's links being
 * user_ul_tick[user_of[i]] and user_dl_tick[user_of[i]]: delay for every publish, the
 * broker's own pubAck into latencyH1 for every publish, the node ack at arrive_tick + dl_k
 * + in->hier_up_tick * escalated[i] into latency (status 5) or latencyH1 (status 4),
 * taskTime where done_tick >= 0; an emission whose product leaves the simtime_t range
 * counts in overflow.  A user without a publish gets the count == 0 record.
 * Defining invariant: the exact merge (fognet_user_stats_merge) of a replication's U records
 * equals, bit for bit, fognet_user_stats_dev's record of that replication with
 * user_per_task = 1 and the per-task links expanded from user_of.
 * FOGNET_POLICY_REF_V3 and FOGNET_POLICY_EXT_LAT, with or without down_tick;
 * FOGNET_POLICY_EXT_HIER with out->escalated (the replay's flags).  Refused:
 * FOGNET_POLICY_EXT_HIER with out->escalated NULL (FOGNET_ERR_UNSUPPORTED, before anything
 * else is checked and with nothing written); a statistics-only `out`, a NULL per_user or
 * NULL links with R * U > 0, a NULL user_of with R * T > 0, U < 0 and a link_stride other
 * than 0 or U (FOGNET_ERR_ARG).  Under the other policies escalated is not read.
 * A failed replication (status other than FOGNET_OK / FOGNET_REF_ABORTED) gets U count == 0
 * records and n_unassigned[r] = 0; nothing of its per-task rows, its user_of row or its link
 * row is read (a FOGNET_REF_ABORTED one keeps its full records).
 * A decided publish whose user_of lies outside [0, U) adds to no record and touches nothing
 * out of bounds; n_unassigned [R] (device, nullable) receives their number per replication.
 * U = 0 writes nothing but n_unassigned.
 * FOGNET_USER_STATS=hbm (environment, testing): the accumulators are the caller's records
 * for every U, as they are above 128 users; the results are identical. */
int fognet_per_user_stats_dev(fognet_ctx *ctx, const fognet_batch_in *in, const fognet_batch_out *out,
                              const int32_t *user_of, int32_t U, int32_t link_stride,
                              const int64_t *user_ul_tick, const int64_t *user_dl_tick,
                              fognet_user_stats *per_user, int64_t *n_unassigned, void *hip_stream);
/* Job reduction of user records (device pointers): out[u] = the exact merge of
 * user_stats[r][u] over the replications with stats[r].status == FOGNET_OK
 * (fognet_reduce_node_stats_dev's rule: REF_ABORTED and failed ones contribute nothing).
 * Any R; R = 0 gives U empty records.  Needs no workspace.  With U = 1 it reduces the [R]
 * records of fognet_user_stats_dev. */
int fognet_reduce_user_stats_dev(fognet_ctx *ctx, const fognet_user_stats *user_stats,
                                 const fognet_rep_stats *stats, int32_t R, int32_t U,
                                 fognet_user_stats *out, void *hip_stream);
/* Host-side identity (the count == 0 record in all four signals) and exact merge, field by
 * field (ranks combine their [U] records after an all-gather). */
void fognet_user_stats_init(fognet_user_stats *s);
void fognet_user_stats_merge(fognet_user_stats *acc, const fognet_user_stats *other);

/* Signal vectors.  The reference records its five signals with `record=stats, vector`; the
 * vector half lists every emission with its time, in the order the module made them.  One
 * replication has V = N + 1 + 3U vectors, in this order: the N nodes' queueTime, the broker's
 * delay, U x latency, U x latencyH1, U x taskTime.  Its rows are the emissions that
 * fognet_node_stats_dev and fognet_per_user_stats_dev count: over the replication's first
 * stats[r].n_tasks publishes, with the same emission rule; an emission that overflows the
 * simtime_t range is no row (the records count it in `overflow`), and a publish whose user_of
 * lies outside [0, U) gives no user-side row and no delay row (n_unassigned counts them).
 * Time, value and order of the rows (k the task's node, u its user, the links as above):
 *   queueTime, node k   time start_tick, value the raw queueTime; in task order (the server is
 *                       FIFO, so the times are nondecreasing).
 *   delay, broker       time arrive_tick, value user_ul[u]; in task order.
 *   latencyH1 / latency / taskTime, user u   value the raw (time - created) * 1000, the time
 *                       arrive + dl_u for the broker's own pubAck (latencyH1), arrive + dl_k +
 *                       ul_k + dl_u for the node's first ack (status 5: latency, 4: latencyH1),
 *                       done + ul_k + dl_u for the completion ack (taskTime); ascending by
 *     1. the time;
 *     2. the broker's own pubAck before any relayed ack (publishes precede dynamic events at
 *        the broker's tick);
 *     3. among relayed acks, the tick at which the node sent it (time - dl_u - ul_k);
 *     4. the tick at which the sending event was inserted: arrive_tick[i] for the first ack
 *        (the task's arrival event, created at the decision), start_tick[i] for the completion
 *        ack (the RELEASERESOURCE timer, armed at the service start);
 *     5. a first ack before a completion ack;
 *     6. the task index.
 * This is the FES order of the reference; tests/test_signal_vectors.py holds it to every
 * relayed ack of the reference's own recorded runs.  The key is total (rows equal in all of it
 * are equal in every column), so the output does not depend on how rows were placed before
 * ordering.
 * The CSR of one replication: offset [V + 1] (offset[0] = 0; vector v's rows are
 * [offset[v], offset[v + 1])), and per row its time (ticks), its raw value (the units of the
 * records: fognet_moments) and the index of the task that caused it. */
typedef struct fognet_signal_vectors {
    int64_t cap;      /* rows per replication in time / value / task: at least 6 * T (one queueTime,
                         one delay, one latency, two latencyH1 and one taskTime per task at most)  */
    int64_t *offset;  /* [Rv][V + 1]                                                            */
    int64_t *time;    /* [Rv][cap]                                                              */
    int64_t *value;   /* [Rv][cap]                                                              */
    int32_t *task;    /* [Rv][cap]                                                              */
} fognet_signal_vectors;

/* The signal vectors of replications [r0, r0 + Rv) of a finished replay, ordered, on the device.
 * in, out, user_of, U, link_stride and the links: as fognet_per_user_stats_dev ([R][T] /
 * [R|1][U], indexed by the job's replication r); out->start_tick is needed as well.  vec (host
 * struct of device pointers) and n_unassigned [Rv] (device, nullable) are indexed by r - r0.
 * Rows at and past offset[V] are not written, and nothing depends on what the buffers held; two
 * runs are byte-identical.  A failed replication (status other than FOGNET_OK /
 * FOGNET_REF_ABORTED) gets all-zero offsets and n_unassigned 0; nothing of its rows, its links
 * or its user_of row is read.  FOGNET_POLICY_REF_V3 and FOGNET_POLICY_EXT_LAT, with or without
 * down_tick.  Refused: FOGNET_POLICY_EXT_HIER (FOGNET_ERR_UNSUPPORTED, before anything else is
 * checked and with nothing written: the place of an escalated task's acks in the order is
 * builder-defined, and no recording pins it); a statistics-only `out` or one without start_tick,
 * NULL vec or vec arrays, vec->cap < 6 * T, NULL links with U > 0, NULL user_of with T > 0,
 * U < 0, a link_stride other than 0 or U, r0 < 0, Rv < 0 or r0 + Rv > R (FOGNET_ERR_ARG);
 * T >= 2^28 or Rv * V >= 2^31 (FOGNET_ERR_UNSUPPORTED).  Uses the context's workspace (4 B per
 * replication and vector).
 * FOGNET_VEC_SORT=hbm (environment, testing): every segment above 64 rows is sorted as segments
 * above 2,048 rows are (in chunks, the sorting network's wider steps over the segment in HBM),
 * and the row counters live in the caller's offset row and the workspace, as they do above 8,192
 * vectors; the results are identical.  FOGNET_VEC_STAGES=1 / 2 (timing
 * only): stop after the count / the place stage; the rows are then unordered or unwritten. */
int fognet_signal_vectors_dev(fognet_ctx *ctx, const fognet_batch_in *in, const fognet_batch_out *out,
                              const int32_t *user_of, int32_t U, int32_t link_stride,
                              const int64_t *user_ul_tick, const int64_t *user_dl_tick, int32_t r0, int32_t Rv,
                              const fognet_signal_vectors *vec, int64_t *n_unassigned, void *hip_stream);

/* Time-window statistics.  Window w of a call covers the ticks [t0_tick + w * window_tick,
 * t0_tick + (w + 1) * window_tick), w in [0, W); the covered range is their union.  One record
 * holds what happened in one window of one replication (or, reduced, of one job).
 * Point events fall into the window of their own tick.  The emissions of the five signals, their
 * times and their values are the rows of "Signal vectors" above, with the same emission rule and
 * the same links; only two things are added here: n_publish falls at arrive_tick and n_complete
 * at done_tick, and under FOGNET_POLICY_EXT_HIER the node's first ack of an escalated task leaves
 * hier_up_tick later, as in fognet_per_user_stats_dev.  An emission whose value leaves the
 * simtime_t range is no row there; here it counts in `overflow` of the window of its time, as in
 * the other records.
 * Intervals are clipped to the covered range, and each window receives the ticks of the interval
 * that lie in it; an interval of length zero adds nothing.  Over a range that covers a
 * replication whole, the busy sums add up to 10^12 * busy_s and the records merge
 * (fognet_window_stats_merge) into the merge of its node records' queue and its user records'
 * four signals.
 * Empty record: as the other records (counts and sums 0, every min_raw INT64_MAX, max_raw
 * INT64_MIN). */
typedef struct fognet_window_stats {
    int64_t  n_publish;            /* decided publishes with arrive_tick in the window                   */
    int64_t  n_complete;           /* completed tasks (done_tick >= 0) with done_tick in the window      */
    uint64_t busy_lo, busy_hi;     /* node-ticks of service inside the window: the part of [start_tick,
                                      done_tick) of every completed task that lies in it (128-bit)       */
    uint64_t insys_lo, insys_hi;   /* task-ticks in the system inside the window: the part of [at_node,
                                      done_tick) of every completed task, at_node = arrive + dl_k
                                      (+ hier_up_tick where escalated), the tick it was enqueued         */
    fognet_moments queue, delay, latency, latencyH1, taskTime;
} fognet_window_stats;             /* 408 B, 8-B aligned */

/* Window statistics of a finished replay, on the device.  in, out, user_of, U, link_stride and
 * the links: as fognet_per_user_stats_dev; out->start_tick is needed as well.  Writes win [R][W]
 * (device): record [r][w] covers window w over replication r's first stats[r].n_tasks publishes.
 * n_outside [R][2] (device, nullable): the point events of replication r before t0_tick ([r][0])
 * and at or past t0_tick + W * window_tick ([r][1]); they add to no record.  A point event is
 * each of n_publish and n_complete and each emission of the five signals, lost ones included.
 * Intervals are clipped and counted nowhere.
 * A publish whose user_of lies outside [0, U) has no user-side event (delay, latency, latencyH1,
 * taskTime); it still counts in n_publish, n_complete, busy, insys and queue, and in
 * n_unassigned [R] (device, nullable).  With U = 0, user_of and the links may be NULL.
 * A failed replication (status other than FOGNET_OK / FOGNET_REF_ABORTED) gets W empty records
 * and zeros in n_outside and n_unassigned; nothing of its rows, its user_of row or its links is
 * read (a FOGNET_REF_ABORTED one keeps its records).
 * FOGNET_POLICY_REF_V3 and FOGNET_POLICY_EXT_LAT, with or without down_tick, the outputs of
 * fognet_run_assigned_dev among them; FOGNET_POLICY_EXT_HIER with out->escalated (a window needs
 * the times of an escalated task's acks, not their order inside a tick).  Refused:
 * FOGNET_POLICY_EXT_HIER with out->escalated NULL (FOGNET_ERR_UNSUPPORTED, before anything else
 * is checked and with nothing written); a statistics-only `out` or one without start_tick, a
 * NULL win with R * W > 0, window_tick < 1, t0_tick < 0, W < 0, t0_tick + W * window_tick above
 * 2^62, U < 0, a link_stride other than 0 or U, NULL links with U > 0, a NULL user_of with U > 0
 * and R * T > 0 (FOGNET_ERR_ARG); W > FOGNET_WINDOW_MAX (FOGNET_ERR_UNSUPPORTED).  R = 0, T = 0
 * and W = 0 succeed; W = 0 writes only n_outside and n_unassigned.
 * The records are exact integers in any order of the updates, so two runs are byte-identical.
 * Up to FOGNET_WINDOW_LDS_WINDOWS windows the pass needs no workspace; above, the context's
 * workspace holds 16 B per replication and window (the cover counts of the two intervals).
 * FOGNET_WINDOW_STATS=hbm (environment, testing): the accumulators are the caller's records and
 * the workspace for every W, as they are above FOGNET_WINDOW_LDS_WINDOWS; the results are
 * identical. */
#define FOGNET_WINDOW_MAX (1 << 20)
#ifndef FOGNET_WINDOW_LDS_WINDOWS /* (a timing build of the library may set another limit) */
#define FOGNET_WINDOW_LDS_WINDOWS 150
#endif
int fognet_window_stats_dev(fognet_ctx *ctx, const fognet_batch_in *in, const fognet_batch_out *out,
                            const int32_t *user_of, int32_t U, int32_t link_stride,
                            const int64_t *user_ul_tick, const int64_t *user_dl_tick,
                            int64_t t0_tick, int64_t window_tick, int32_t W,
                            fognet_window_stats *win, int64_t *n_outside, int64_t *n_unassigned,
                            void *hip_stream);
/* Job reduction of the window records (device pointers): out[w] = the exact merge of win[r][w]
 * over the replications with stats[r].status == FOGNET_OK (fognet_reduce_node_stats_dev's rule).
 * Any R; R = 0 gives W empty records.  Needs no workspace. */
int fognet_reduce_window_stats_dev(fognet_ctx *ctx, const fognet_window_stats *win,
                                   const fognet_rep_stats *stats, int32_t R, int32_t W,
                                   fognet_window_stats *out, void *hip_stream);
/* Host-side identity (the empty record) and exact merge, field by field (ranks combine their [W]
 * records after an all-gather). */
void fognet_window_stats_init(fognet_window_stats *s);
void fognet_window_stats_merge(fognet_window_stats *acc, const fognet_window_stats *other);

/* Quantiles.  Exact quantiles of the five recorded signals, in fognet_window_stats order: queue,
 * delay, latency, latencyH1, taskTime.
 * Populations.  A signal's population is the set of rows that "Signal vectors" above defines for
 * it, under FOGNET_POLICY_EXT_HIER the emissions that fognet_window_stats_dev counts: over the
 * replication's first stats[r].n_tasks publishes, with the same emission rule and the same links.
 * An emission whose value leaves the simtime_t range is no member, so a population's size n is the
 * `count` of the matching fognet_moments, not count + overflow.  A publish whose user_of lies
 * outside [0, U) has no user-side member (delay, latency, latencyH1, taskTime); it keeps its
 * queueTime member and counts in n_unassigned.
 * Rank rule: nearest rank, in integers only.  A rank is asked for as ppm in [0, 1000000]; of a
 * population of n > 0 raw values the result is the k-th smallest, k = max(1, ceil(n * ppm /
 * 1000000)), 1-based (n * ppm stays below 2^60).  ppm = 0 is the minimum, ppm = 1000000 the
 * maximum, and the median of four values is the second smallest.  The result is a member of the
 * population: a raw int64 in the units of fognet_moments, never interpolated, with no floating
 * point on the way.  For n = 0 it is INT64_MAX, the empty record's min_raw. */
#define FOGNET_QUANTILE_SIGNALS 5
#define FOGNET_QUANTILE_MAX 8 /* ranks per call */
/* Quantiles per replication, on the device.  in, out, user_of, U, link_stride and the links: as
 * fognet_window_stats_dev (with U = 0, user_of and the links may be NULL); out->start_tick is
 * needed.  ppm [Q] (host): the ranks, which may repeat and come in any order.  Writes value
 * [R][5][Q] (device; value[r][s][q] answers ppm[q] for signal s), count [R][5] (device; the
 * populations' sizes) and n_unassigned [R] (device, nullable).
 * A failed replication (status other than FOGNET_OK / FOGNET_REF_ABORTED) gets counts 0, values
 * INT64_MAX and n_unassigned 0; nothing of its rows, its user_of row or its links is read (a
 * FOGNET_REF_ABORTED one keeps its results).
 * FOGNET_POLICY_REF_V3 and FOGNET_POLICY_EXT_LAT, with or without down_tick, the outputs of
 * fognet_run_assigned_dev among them; FOGNET_POLICY_EXT_HIER with out->escalated (a quantile needs
 * the values of an escalated task's acks, not their order inside a tick).  Refused:
 * FOGNET_POLICY_EXT_HIER with out->escalated NULL (FOGNET_ERR_UNSUPPORTED, before anything else is
 * checked and with nothing written); Q < 1 or Q > FOGNET_QUANTILE_MAX, a ppm outside [0, 10^6],
 * NULL ppm, value or count with R > 0, a statistics-only `out` or one without start_tick, U < 0, a
 * link_stride other than 0 or U, NULL links with U > 0, a NULL user_of with U > 0 and R * T > 0
 * (FOGNET_ERR_ARG).  R = 0 and T = 0 succeed.
 * The pass is a radix select over the key raw ^ 2^63, a byte per round, that never stores a value:
 * every round streams the rows again.  The counts are integers in any order of the updates, so
 * two runs are byte-identical; nothing depends on what the output buffers held, and nothing
 * outside them is written.  Needs no workspace.
 * FOGNET_QUANTILES=full (environment, read at the call; testing): all eight rounds run for every
 * signal; by default the rounds of the leading bytes that a population's minimum and maximum share
 * are skipped.  The results are identical. */
int fognet_quantiles_dev(fognet_ctx *ctx, const fognet_batch_in *in, const fognet_batch_out *out,
                         const int32_t *user_of, int32_t U, int32_t link_stride,
                         const int64_t *user_ul_tick, const int64_t *user_dl_tick,
                         const int32_t *ppm, int32_t Q, int64_t *value, int64_t *count,
                         int64_t *n_unassigned, void *hip_stream);
/* Quantiles of the job: of each signal's population pooled over the replications with
 * stats[r].status == FOGNET_OK (fognet_reduce_node_stats_dev's rule: a FOGNET_REF_ABORTED or
 * failed replication contributes nothing, and nothing of a failed one is read).  Arguments,
 * policies and refusals as fognet_quantiles_dev; writes value [5][Q] and count [5] (device).
 * The result is no function of the per-replication results.  R = 0 gives five empty populations.
 * Uses the context's workspace (8 B per signal, rank and byte value, and the select's state;
 * ordering of calls on one context: "Streams" in the Conventions above); nothing depends on what
 * the workspace held. */
int fognet_job_quantiles_dev(fognet_ctx *ctx, const fognet_batch_in *in, const fognet_batch_out *out,
                             const int32_t *user_of, int32_t U, int32_t link_stride,
                             const int64_t *user_ul_tick, const int64_t *user_dl_tick,
                             const int32_t *ppm, int32_t Q, int64_t *value, int64_t *count,
                             void *hip_stream);

/* Queue-length statistics.  For fog node k of replication r, L(t) is the length of its `requests`
 * vector (ComputeBrokerApp3.cc:309 push_back, :246 erase): the tasks waiting, the one in service
 * not among them.
 * A decided task enters the queue when it reaches its node, at_node = arrive_tick + dl_k, and is
 * answered status 4; it leaves at its start_tick.  A status-5 or status-9 task never enters.  Under
 * down_tick a queued task that never starts (start_tick = -1) leaves at down_tick[k]; the crash
 * precedes every model event of its tick, so such a task takes part in no tie.
 * Same-tick order (it changes only the maximum): the FES order of DESIGN.md §3.3.  Take the dequeue
 * at tick x caused by the completion of the task served just before it, which started at
 * prev_start, and an enqueue at tick x of a publish that reached the broker at t = x - dl_k.  The
 * enqueue comes first iff t <= prev_start: the arrival event was then inserted no later than the
 * RELEASERESOURCE timer, and at equal insertion ticks the pre-inserted publish ran first.
 * A call observes the ticks [t0_tick, t1_tick) and takes up to FOGNET_QUEUE_LEVELS_MAX strictly
 * ascending levels level[q] >= 1.  The empty record, given to a failed replication, is all zero.
 * Everything is an exact integer in any order of the updates, so two runs are byte-identical. */
#define FOGNET_QUEUE_LEVELS_MAX 8
typedef struct fognet_queue_stats {
    int64_t  n_enq;       /* enqueues with t0 <= at_node < t1                                  */
    int64_t  max_len;     /* largest L right after one of those enqueues (0: none).  A length
                             carried into the range from before t0 is no enqueue of the range. */
    uint64_t observed_lo, observed_hi;  /* t1 - t0 of every replication merged into the record */
    uint64_t area_lo, area_hi;          /* integral of L over the range: the part of [at_node,
                                           leave) of every queued task that lies in it         */
    uint64_t time_ge[FOGNET_QUEUE_LEVELS_MAX][2]; /* ticks of the range with L >= level[q]
                                                     (lo, hi); q >= Q: 0                       */
} fognet_queue_stats;                   /* 176 B, 8-B aligned */

/* Queue-length statistics of a finished replay, on the device.  in (arrive_tick, dl_tick,
 * down_tick) and out (node, status, start_tick, stats[r].{n_tasks,status}): device pointers, as
 * fognet_node_stats_dev.  level [Q] (host).  Writes qs [R][N] (device): record [r][k] covers node k
 * over replication r's first stats[r].n_tasks publishes.
 * A failed replication (status other than FOGNET_OK / FOGNET_REF_ABORTED) gets N empty records and
 * none of its rows is read (a FOGNET_REF_ABORTED one keeps its records).
 * FOGNET_POLICY_REF_V3 and FOGNET_POLICY_EXT_LAT, with or without down_tick, the outputs of
 * fognet_run_assigned_dev among them.  Refused, before anything is written:
 * FOGNET_POLICY_EXT_HIER, with or without out->escalated (FOGNET_ERR_UNSUPPORTED: an escalated task
 * arrives a hop later, so a node's FIFO order is no longer trace order, and the place of that
 * arrival within its tick is the unpinned order that keeps the signal vectors from EXT_HIER); a
 * statistics-only `out` or one without start_tick, Q < 1 or Q > FOGNET_QUEUE_LEVELS_MAX, a level
 * below 1 or levels not strictly ascending, t0_tick < 0, t1_tick < t0_tick, t1_tick > 2^62, NULL
 * level, NULL qs with R * N > 0 (FOGNET_ERR_ARG).  R = 0, T = 0 and t1_tick = t0_tick succeed.
 * Uses the context's workspace (28 B per task, 4 B per replication and node; 12 B more per
 * replication and node above 2,048 nodes); a job whose elements pass 1 GiB runs its replications in
 * rounds (ordering of calls on one context: "Streams" in the Conventions above).  Nothing depends
 * on what the workspace or qs held.
 * FOGNET_QUEUE_STATS=hbm (environment, testing): the counts, carries and accumulators live in the
 * workspace and the caller's records for every N, as they do above 256 nodes (records), 2,048
 * (carries) and 8,192 (counts); the results are identical.  FOGNET_QUEUE_ROUND=<n> (testing): n
 * replications per round.  FOGNET_QUEUE_STAGES=1 (timing only): stop before the measure kernel; no
 * output is written then. */
int fognet_queue_stats_dev(fognet_ctx *ctx, const fognet_batch_in *in, const fognet_batch_out *out,
                           const int64_t *level, int32_t Q, int64_t t0_tick, int64_t t1_tick,
                           fognet_queue_stats *qs, void *hip_stream);
/* Job reduction of the queue records (device pointers): out[k] = the exact merge of qs[r][k] over
 * the replications with stats[r].status == FOGNET_OK (fognet_reduce_node_stats_dev's rule): sums,
 * and the maximum of max_len.  Any R; R = 0 gives N empty records.  Needs no workspace. */
int fognet_reduce_queue_stats_dev(fognet_ctx *ctx, const fognet_queue_stats *qs,
                                  const fognet_rep_stats *stats, int32_t R, int32_t N,
                                  fognet_queue_stats *out, void *hip_stream);
/* Host-side identity (the empty record) and exact merge. */
void fognet_queue_stats_init(fognet_queue_stats *s);
void fognet_queue_stats_merge(fognet_queue_stats *acc, const fognet_queue_stats *other);

/* Paired comparison of two replays of the same traces, A and B (two policies, a policy against
 * fognet_run_assigned_dev, ...): task i of replication r is the same publish in both, so every
 * difference below is B minus A of one task, and the publish tick arrive_tick cancels in all of
 * them.  That both outputs belong to the same traces is the caller's word.
 * Pairs: replication r is COMPARED iff stats_a[r].status and stats_b[r].status are each FOGNET_OK
 * or FOGNET_REF_ABORTED; its pairs are the task indices i < n_pairs = min(n_tasks of A, n_tasks of
 * B), clamped to [0, T].  n_moved and trans count over all pairs.  A status byte outside {5, 4, 9}
 * counts in no cell of trans; the node values are compared and never used as an index.
 * Signals: over the pairs COMPLETED in both runs (done_tick >= 0 on both sides), in ticks,
 *   d_start   = start_b - start_a
 *   d_service = (done_b - start_b) - (done_a - start_a)
 *   d_resp    = done_b - done_a            (per pair d_resp = d_start + d_service)
 * each computed modulo 2^64 (outputs of a replay stay below 2^61 ticks, so nothing wraps); signed
 * values with two's complement sums, like queue_sum; overflow is always 0.  A negative d_resp
 * means the task finished earlier under B: "better".
 * Replications: a compared replication has n_reps = 1 and exactly one of rep_better / rep_equal /
 * rep_worse = 1, by the sign of its signed 128-bit d_resp sum (< 0: better; no completed pair:
 * equal).  A replication that is not compared gets the EMPTY record -- counts 0, the three empty
 * fognet_moments, n_reps = 0 -- which still carries the two statuses; none of its rows is read, on
 * either side.
 * Everything is an exact integer in any order of the updates, so two runs are byte-identical. */
/* index of a task status in trans: 0 = started (5), 1 = queued (4), 2 = lost (9) */
typedef struct fognet_compare_stats {
    int32_t status_a, status_b;   /* stats[r].status of the two replications (a job record: FOGNET_OK) */
    int64_t n_reps;               /* replications in the record */
    int64_t n_pairs;              /* publishes decided in both: min(n_tasks_a, n_tasks_b), clamped to [0, T] */
    int64_t n_moved;              /* pairs with node_a != node_b */
    int64_t trans[3][3];          /* pairs by (status in A, status in B) */
    int64_t n_done_both, n_done_only_a, n_done_only_b, n_done_neither;   /* done_tick >= 0 */
    int64_t n_better, n_equal, n_worse;        /* of n_done_both: d_resp < 0, == 0, > 0 */
    int64_t rep_better, rep_equal, rep_worse;  /* replications by the sign of their d_resp sum */
    fognet_moments d_start, d_service, d_resp; /* over the n_done_both pairs, ticks, B minus A */
} fognet_compare_stats;           /* 400 B, 8-B aligned */

/* The comparison of two finished replays, on the device.  Of `in` only R and T are read: no trace
 * column, link or policy field, so the pass serves every fognet_batch_out the library produces
 * (REF_V3, EXT_LAT, EXT_HIER with or without out->escalated, fognet_run_assigned_dev, with or
 * without down_tick).  out_a and out_b (device pointers): node, status, start_tick, done_tick and
 * stats[r].{n_tasks,status} of each; out_a == out_b is allowed.  Writes cmp [R] (device), one
 * record per replication.  hist (device, [2][FOGNET_HIST_BINS] int64, ADDED to, nullable): row 0
 * takes the completed pairs with d_resp < 0, row 1 those with d_resp > 0, each binned by
 * |d_resp| with the rule of histogram metric 1 (whole milliseconds, log2 bins); only replications
 * with both statuses == FOGNET_OK add to it (the job rule), so its rows sum to the job record's
 * n_better / n_worse.
 * Refused, before anything is written (FOGNET_ERR_ARG): negative R or T, and with R > 0 a
 * statistics-only out on either side (T > 0), NULL stats, NULL cmp.  R = 0 and T = 0 succeed.
 * The call only enqueues on hip_stream and needs no workspace; nothing depends on what cmp held,
 * and nothing outside cmp [R] and hist is written. */
int fognet_compare_dev(fognet_ctx *ctx, const fognet_batch_in *in, const fognet_batch_out *out_a,
                       const fognet_batch_out *out_b, fognet_compare_stats *cmp /* [R] */,
                       int64_t *hist /* [2][FOGNET_HIST_BINS], ADDED to, nullable */, void *hip_stream);
/* Job reduction (device pointers): *out = the exact merge of the records cmp[r] whose status_a and
 * status_b are both FOGNET_OK (the record carries its statuses, so no stats array is passed); its
 * own statuses are FOGNET_OK and n_reps is the number merged.  Any R; R = 0 gives the empty
 * record.  Needs no workspace. */
int fognet_reduce_compare_dev(fognet_ctx *ctx, const fognet_compare_stats *cmp, int32_t R,
                              fognet_compare_stats *out, void *hip_stream);
/* Host-side identity (the empty record, statuses FOGNET_OK) and exact merge: counts and moments
 * add field by field, extrema combine; acc's statuses are left alone. */
void fognet_compare_stats_init(fognet_compare_stats *s);
void fognet_compare_stats_merge(fognet_compare_stats *acc, const fognet_compare_stats *other);

/* Exact reduction of R per-replication stats (device pointers) into one job
 * record (device pointer).  Replications with status != OK count in n_failed
 * and contribute nothing else.  R > 4096 reduces through partial records in
 * the context's workspace (ordering of calls on one context: "Streams" in
 * the Conventions above). */
int fognet_reduce_stats_dev(fognet_ctx *ctx, const fognet_rep_stats *stats, int32_t R,
                            fognet_job_stats *out, void *hip_stream);
/* Host-side exact merge (used to combine per-GPU records after an all-gather):
 * *acc = *acc (+) *other.  fognet_job_stats_init() sets the identity. */
void fognet_job_stats_init(fognet_job_stats *s);
void fognet_job_stats_merge(fognet_job_stats *acc, const fognet_job_stats *other);
/* Host-side exact accumulate of one replication (what fognet_reduce_stats_dev
 * does per replication; energy is added in call order): for callers of the
 * host-buffer fognet_run_batch. */
void fognet_job_stats_add_rep(fognet_job_stats *acc, const fognet_rep_stats *rep);

/* Replication groups: the job reduction keyed by the replication's place in the job (a sweep point,
 * a scenario, a shard) and, per group, the spread of per-replication metrics ACROSS replications --
 * the method of independent replications: each run's mean, and the mean and standard deviation of
 * those over the runs.  The pass reads the [R] records alone, so it serves every replay that fills
 * fognet_rep_stats: materialised, assigned, EXT_HIER and generated (not the v2 model, whose
 * fognet_v2_stats hold counts only).
 * Metrics of one replication, exact integers from its record (fognet_rep_metrics); floor is towards
 * minus infinity (-7 / 2 -> -4):
 *   0 RESP_MEAN    floor(resp_sum / n_tasks), ticks (resp_sum: unsigned 128 bit)    iff n_tasks > 0
 *   1 RESP_MAX     resp_max_ticks                                                   iff n_tasks > 0
 *   2 QUEUE_MEAN   floor(queue_sum / n_qtime), raw (queue_sum: signed 128 bit)      iff n_qtime > 0
 *   3 QUEUE_MAX    queue_max_raw                                                    iff n_qtime > 0
 *   4 QUEUED_PPM   floor(n_queued * 10^6 / n_tasks) (signed 128-bit product)        iff n_tasks > 0
 *   5 MAKESPAN     last_tick                                                        iff last_tick != INT64_MIN
 *   6 BUSY_S       busy_s                                                           always
 *   7 MAX_PENDING  max_pending                                                      always
 *   8 ENERGY_UJ    toInt64(energy_j * 1e6): one IEEE multiply, then floor(x + 0.5) with its own
 *                  rounding (no fused multiply-add), "Reference signal values"      always
 * Only a replication with status == FOGNET_OK has metrics (fognet_reduce_stats_dev's rule).  A
 * defined metric whose value does not fit int64 (a NaN or out-of-range energy: toInt64's
 * |floor(x + 0.5)| < 2^63; a quotient of inconsistent caller-made records) counts in that metric's
 * `overflow` and stays out of its moments; an undefined metric adds nothing.
 * Every field of the group record is an integer updated with integer atomics or merged exactly, so
 * a record does not depend on the order of its updates: the same call gives the same bytes twice,
 * and sharding over GPUs changes nothing.  No fp64 sum is kept: the group's energy is
 * across[FOGNET_METRIC_ENERGY_UJ].sum, in microjoules. */
#define FOGNET_REP_METRICS 9
enum {
    FOGNET_METRIC_RESP_MEAN = 0, FOGNET_METRIC_RESP_MAX, FOGNET_METRIC_QUEUE_MEAN, FOGNET_METRIC_QUEUE_MAX,
    FOGNET_METRIC_QUEUED_PPM, FOGNET_METRIC_MAKESPAN, FOGNET_METRIC_BUSY_S, FOGNET_METRIC_MAX_PENDING,
    FOGNET_METRIC_ENERGY_UJ
};
typedef struct fognet_group_stats {
    int64_t n_reps, n_failed, n_ref_aborted;    /* fognet_job_stats' rules, over the group's members */
    int64_t n_tasks, n_queued, n_started, events;   /* sums over the OK members */
    fognet_moments queue;   /* pooled over tasks: count = sum of n_qtime, overflow = sum of n_qtime_overflow,
                               min/max, sum (signed, modulo 2^128) and sq (192 bit) merged from the OK
                               members' records                                                       */
    fognet_moments resp;    /* pooled: count = sum of n_tasks, overflow 0                             */
    fognet_moments across[FOGNET_REP_METRICS];  /* over the group's OK replications, one value each */
} fognet_group_stats;       /* 848 B, 8-B aligned: 7 words, then 11 fognet_moments */

#define FOGNET_GROUP_LDS_MAX 64   /* groups whose records a workgroup keeps in LDS (64 x 848 B) */
/* out[g] (device, [G]) = the group record of the replications r with group_of[r] == g (device, [R]
 * int32; NULL: every replication in group 0).  A replication with group_of[r] outside [0, G) is in
 * no group and is counted in *n_ungrouped (device, nullable).  A failed replication counts in its
 * group's n_reps and n_failed, and in n_ref_aborted under fognet_job_stats' rule (status OK or
 * FOGNET_REF_ABORTED, abort_tick set); it adds nothing else.
 * metrics (device, [R][FOGNET_REP_METRICS] int64, nullable) and defined (device, [R] uint32,
 * nullable) take fognet_rep_metrics of every replication, grouped or not: bit m of defined[r] says
 * that metrics[r][m] is a value the moments take; every other entry (an undefined or overflowed
 * metric, the whole row of a failed replication) is INT64_MIN with its bit clear.  They are there for
 * what the moments cannot give, such as quantiles across replications on the host.
 * Any R; R = 0 gives G empty records (every count and sum 0, min_raw INT64_MAX, max_raw INT64_MIN)
 * and *n_ungrouped = 0.  G <= 0, a NULL out, or NULL stats with R > 0: FOGNET_ERR_ARG, nothing
 * written.  The call only enqueues on hip_stream and needs no workspace.  Up to
 * FOGNET_GROUP_LDS_MAX groups each workgroup accumulates in LDS and adds its non-empty records to
 * out at its end; above, the accumulators are out itself.  FOGNET_GROUP_STATS=hbm (environment,
 * testing) forces the latter for every G; the results are identical. */
int fognet_reduce_groups_dev(fognet_ctx *ctx, const fognet_rep_stats *stats, int32_t R,
                             const int32_t *group_of, int32_t G, fognet_group_stats *out,
                             int64_t *metrics, uint32_t *defined, int64_t *n_ungrouped, void *hip_stream);
/* The metrics of one record (host): value[m] and bit m of *defined for a metric the moments take,
 * bit m of *overflowed for a defined metric that does not fit int64 (value[m] = INT64_MIN, as for
 * an undefined one).  The status is not looked at.  defined / overflowed: nullable. */
void fognet_rep_metrics(const fognet_rep_stats *rep, int64_t value[FOGNET_REP_METRICS], uint32_t *defined,
                        uint32_t *overflowed);
/* Host twins, exact: the empty record, one replication added (what the device pass does per
 * member), and the merge of two records (ranks, shards, groups folded together). */
void fognet_group_stats_init(fognet_group_stats *s);
void fognet_group_stats_add_rep(fognet_group_stats *acc, const fognet_rep_stats *rep);
void fognet_group_stats_merge(fognet_group_stats *acc, const fognet_group_stats *other);
/* The group as a job record: every integer field equals what fognet_reduce_stats_dev gives for the
 * group's members alone (last_tick, max_pending and busy_s from across[]; queue_sum's top limb is
 * the sign of the 128-bit pooled sum and resp_sum's is 0, which is the job's value while the group's
 * sums stay inside 128 bits, 2^64 tasks of 2^63 ticks); energy_j = (double)(sum of microjoules) * 1e-6. */
void fognet_group_stats_job(const fognet_group_stats *g, fognet_job_stats *out);

/* Device trace generator: fills arrive/req [R][T] and node params [R][N]
 * (replications r0 .. r0+R-1 of the recipe; r0 lets GPUs shard one job). */
int fognet_gen_trace_dev(fognet_ctx *ctx, const fognet_gen_params *p, int64_t r0, int32_t R,
                         int32_t T, int32_t N, int64_t *arrive_tick, int32_t *req_mips,
                         int32_t *mips, int64_t *dl_tick, int64_t *ul_tick, int64_t *init_adv_tick,
                         void *hip_stream);

/* Generated replay ("traces are generated in-kernel ...
 * only stats and histograms are written"): replications r0 .. r0 + R - 1 of
 * the fognet_gen_trace_dev recipe (p; mean_gap_ticks / lat_scale indexed by the
 * local replication 0 .. R-1) are replayed with each 64-publish chunk of the
 * trace and the node parameters computed inside the replay kernel; no trace
 * and no per-task output ever reaches memory.  Results equal
 * fognet_gen_trace_dev + fognet_run_batch_dev on the same replications.
 *   in:  R, T, N, policy, ring_capacity, p_busy_w/p_idle_w, node_stride (and
 *        hier_threshold_s / hier_up_tick for EXT_HIER); every trace/node-parameter
 *        pointer, down_tick and region must be NULL.  EXT_HIER: publish i's regional
 *        broker follows the builder-defined mobility model of the Python mirror's
 *        mobility_regions with its defaults (256 users, user i mod 256 starts in
 *        region (i mod 256) mod B, moves +1 (even) / -1 (odd) every 30/45/60/75 s
 *        (user mod 4) from the first publish), computed in the kernel; EXT_HIER and
 *        replays with T * (req_hi / 1000) >= 2^32 run on the wide kernel.
 *   out: stats [R] (required), hist (added to), node_energy_j (nullable);
 *        node/status/start_tick/done_tick must be NULL. */
int fognet_run_generated_dev(fognet_ctx *ctx, const fognet_gen_params *p, int64_t r0,
                             const fognet_batch_in *in, fognet_batch_out *out, void *hip_stream);

/* Synchronise the context's device. */
int fognet_sync(fognet_ctx *ctx);

/* EXT_HIER with N > 1024 (more than one region), fognet_run_batch[_dev]: the path each
 * launch took (diagnostic).  A launch first replays every (replication, region) pair on
 * its own wavefront and hands a replication with any escalation to the sequential
 * replay, which continues it from its first escalated publish (region_launches); or it
 * runs the sequential replay for every replication (sequential_launches).  Both give
 * identical results.  FOGNET_HIER_REGIONS (environment): unset or "1" -- the region pass;
 * "0" -- always sequential; "only" -- the region pass without the hand-over (testing: a
 * handed-over replication then reports FOGNET_ERR_UNSUPPORTED).  FOGNET_HIER_RESUME=0: the
 * sequential replay restarts a handed-over replication from its first publish, and with
 * FOGNET_HIER_REGIONS unset the path is chosen per launch: while the last region pass
 * whose hand-over count has reached the host (copied back asynchronously, read without
 * waiting) handed more than half of its replications over, the next launches go straight
 * to the sequential replay, with a region pass again every 16th launch to re-measure. */
int fognet_hier_path_stats(const fognet_ctx *ctx, int64_t *region_launches, int64_t *sequential_launches);

/* ---- Multi-GPU statistics exchange over RCCL (xGMI), SURVEY.md §8(b)
 * `fognet_allreduce_stats` and §8(e): replications are sharded over ranks (one
 * process per GPU) and this end-of-run exchange is the only collective.  RCCL
 * is loaded on first use (librccl.so.1; a copy already in the process, e.g.
 * PyTorch's, is reused).  Rank 0 creates the id; the caller moves its bytes to
 * the other ranks (MPI, a shared file, a TCP store ...).  Collective calls:
 * every rank calls fognet_comm_create / fognet_allreduce_stats in the same order. */
#define FOGNET_COMM_ID_BYTES 128
typedef struct fognet_comm fognet_comm;
int fognet_comm_unique_id(uint8_t id[FOGNET_COMM_ID_BYTES]);
int fognet_comm_create(fognet_ctx *ctx, int32_t world, int32_t rank, const uint8_t id[FOGNET_COMM_ID_BYTES],
                       fognet_comm **out);
void fognet_comm_destroy(fognet_comm *comm);
/* *inout (host): this rank's job record in, the job record of all ranks out:
 * the records are all-gathered and merged in rank order with
 * fognet_job_stats_merge, so the result is exact and identical on every rank
 * (energy: fp64 sum in rank order).  hist (device pointer to
 * [FOGNET_HIST_METRICS][FOGNET_HIST_BINS] int64, nullable): summed in place.
 * Enqueued on hip_stream; returns after the exchange completed. */
int fognet_allreduce_stats(fognet_ctx *ctx, fognet_comm *comm, fognet_job_stats *inout, int64_t *hist,
                           void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* FOGNET_HIP_H */
