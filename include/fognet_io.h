/*
 * fognet_io.h — host-side formats on either side of the offload-decision path
 * (SURVEY.md §8(f) rows 1 and 3).  Pure host C++ in libfognet_hip: no GPU and
 * no fognet_ctx needed, so an OMNeT++ build, a trace exporter or a CPU test
 * can call these without a device.
 *
 *   - Binary SoA trace files ("FOGNTRC1"): the inputs of fognet_run_batch
 *     (node parameters in CONNECT order + the broker-side publish trace), so
 *     the same bytes feed the GPU engine, the CPU oracle and a reference run.
 *   - OMNeT++ 4.6 result files: `.sca` (scalar/statistic/field/bin lines as in
 *     simulations/example/results/General-0.sca:4957-4967) and `.vec`
 *     (vector declarations + data lines, General-0.vec / General-0.vci) from
 *     the engine's job record, histogram and per-task outputs.
 *   - The reference's task source, mqttApp2::sendMqttData
 *     (src/mqttapp/mqttApp2.cc:353-409): glibc rand() stream shared by every
 *     user in event order, MIPSRequired = 200 + rand() % 701.
 *
 * Errors: fognet_status codes (fognet_hip.h); the message of the last failure
 * on the calling thread is fognet_io_last_error().
 */
#ifndef FOGNET_IO_H
#define FOGNET_IO_H

#include <stdint.h>

#include "fognet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FOGNET_TRACE_MAGIC "FOGNTRC1"
#define FOGNET_TRACE_VERSION 1
#define FOGNET_TRACE_HEADER_BYTES 256
#define FOGNET_TRACE_ALIGN 64

/* Trace file layout (little endian):
 *   header (FOGNET_TRACE_HEADER_BYTES): magic[8], u32 version, u32 header_bytes,
 *     i32 R, T, N, node_stride (0: node parameters shared, N: one row per
 *     replication), u32 flags, u32 reserved, u64 payload_bytes, u64 checksum
 *     (FNV-1a 64 over the payload), char note[FOGNET_TRACE_NOTE_BYTES]
 *     (free text, NUL padded), zero padding;
 *   payload, each section starting at a multiple of FOGNET_TRACE_ALIGN from
 *     the file start, in this order (NR = node_stride ? R : 1):
 *     mips i32 [NR][N], dl_tick i64 [NR][N], ul_tick i64 [NR][N],
 *     init_adv_tick i64 [NR][N], node_id i32 [NR][N] (flag NODE_ID),
 *     p_busy_w f64 [NR][N], p_idle_w f64 [NR][N] (flag POWER),
 *     arrive_tick i64 [R][T], req_mips i32 [R][T]. */
#define FOGNET_TRACE_NOTE_BYTES 160
#define FOGNET_TRACE_FLAG_POWER 1u    /* p_busy_w / p_idle_w sections present            */
#define FOGNET_TRACE_FLAG_NODE_ID 2u  /* node_id section present (module ids, .sca names) */

typedef struct fognet_trace_info {
    int32_t R, T, N, node_stride;
    uint32_t flags;
    uint32_t version;
    uint64_t payload_bytes;
    uint64_t checksum;
    char note[FOGNET_TRACE_NOTE_BYTES];
} fognet_trace_info;

const char *fognet_io_last_error(void);

/* Write in (host pointers; policy and ring_capacity are not stored) to path.
 * node_id: [NR][N] module ids (nullable: not stored).  note: nullable. */
int fognet_trace_write(const char *path, const fognet_batch_in *in, const int32_t *node_id, const char *note);

/* Read and validate the header (magic, version, sizes, file length). */
int fognet_trace_info_read(const char *path, fognet_trace_info *info);

/* Read the whole trace into caller buffers sized from fognet_trace_info:
 * out->arrive_tick .. init_adv_tick are required; out->p_busy_w/p_idle_w
 * and node_id are filled when non-null and present (FOGNET_ERR_ARG when
 * non-null but absent).  R/T/N/node_stride of *out are set from the file.
 * The checksum is verified (FOGNET_ERR_ARG on mismatch). */
int fognet_trace_read(const char *path, fognet_batch_in *out, int32_t *node_id);

/* OMNeT++ .sca of one job record.  run_id: "run" line (e.g.
 * "General-0-20260101-00:00:00-1"); network: module path prefix (e.g.
 * "FogNet").  Writes, under <network>.broker.udpApp[0] and
 * <network>.fogNodes.udpApp[0]: scalars (decisions, queued, started,
 * replications, failed replications, busy seconds, energy J, makespan s),
 * `queueTime:stats` and `response:stats` (ms; count/mean/stddev/sum/sqrsum/
 * min/max computed from the exact integer sums, printed %.14g like
 * OMNeT++), and when hist != NULL `queueTime:histogram` /
 * `response:histogram` with the FOGNET_HIST_BINS bins (lower bound ms). */
int fognet_write_sca(const char *path, const char *run_id, const char *network, const fognet_job_stats *job,
                     const int64_t *hist /* [FOGNET_HIST_METRICS][FOGNET_HIST_BINS], nullable */);

/* OMNeT++ .sca blocks of per-node records (host; fognet_node_stats_dev /
 * fognet_reduce_node_stats_dev, fognet_hip.h): per module
 * <network>.fogNode[<node_id or index>].udpApp[0] (fognet_write_vec's naming) the
 * scalars tasks, tasks queued, tasks started, tasks lost and busy seconds, then
 * `queueTime:stats` and `response:stats` with fognet_write_sca's fields and
 * formatting (a node without a task writes them with count 0).  append != 0: the
 * blocks are appended to the existing file fognet_write_sca wrote, without a
 * second version/run header; otherwise the file is created with one.
 * node_id: [N], nullable (index names). */
int fognet_write_sca_nodes(const char *path, const char *run_id, const char *network, int32_t N,
                           const fognet_node_stats *nodes, const int32_t *node_id, int append);

/* OMNeT++ .sca scalars of per-node queue records (host; fognet_queue_stats_dev /
 * fognet_reduce_queue_stats_dev, fognet_hip.h "Queue-length statistics"): qs [N], level [Q] the
 * levels of the call that made them.  Per module <network>.fogNode[<node_id or index>].udpApp[0]
 * (fognet_write_sca_nodes' naming, so the lines join that block) the scalars
 *   queueLength:max, queueLength:enqueued, queueLength:timeavg = area / observed, and per level
 *   queueLength:ge<level> = time_ge / observed,
 * the counts as integers, the shares %.14g from the 128-bit sums (-nan where observed is 0).
 * append and node_id: as fognet_write_sca_nodes. */
int fognet_write_sca_queue(const char *path, const char *run_id, const char *network, int32_t N,
                           const fognet_queue_stats *qs, const int64_t *level, int32_t Q,
                           const int32_t *node_id, int append);

/* OMNeT++ .sca block of a paired comparison (host; the job record of fognet_reduce_compare_dev and
 * fognet_compare_dev's hist, fognet_hip.h "Paired comparison").  Under one module (nullable:
 * <network>.compare) the scalars, as integers,
 *   compare:replications, compare:pairs, compare:moved, compare:better, compare:equal,
 *   compare:worse, compare:doneOnlyA, compare:doneOnlyB, compare:repsBetter, compare:repsEqual,
 *   compare:repsWorse and the nine compare:status<a>to<b> with a, b in 5, 4, 9 (trans, row-major),
 * then startDiff:stats, serviceDiff:stats and responseDiff:stats in ms (ticks / 10^9) with
 * fognet_write_sca's fields and formatting, from the exact sums (count 0: -nan).  hist
 * ([2][FOGNET_HIST_BINS], nullable): responseDiff:earlier:histogram (d_resp < 0) and
 * responseDiff:later:histogram (d_resp > 0) over |d_resp| in fognet_write_sca's bin format;
 * `field count` is the row's total, and the moments of one side alone are not recorded (-nan).
 * append: as fognet_write_sca_nodes. */
int fognet_write_sca_compare(const char *path, const char *run_id, const char *network, const char *module,
                             const fognet_compare_stats *job, const int64_t *hist, int append);

/* OMNeT++ .sca blocks of replication groups (host; fognet_reduce_groups_dev's records, fognet_hip.h
 * "Replication groups").  Per group one module -- module[g] (nullable array of G names), else
 * <network>.replications when G == 1 and <network>.group[g] otherwise -- with the scalars
 *   replications, "failed replications", "replications the reference aborts"
 * and one statistic per metric over the group's OK replications (count, mean and stddev are what
 * an interval needs; no t-quantile table is shipped):
 *   respMean:replications, respMax:replications       ms (ticks / 10^9)
 *   queueMean:replications, queueMax:replications     ms (raw * 10^-12)
 *   queuedShare:replications                          a fraction (ppm / 10^6)
 *   makespan:replications                             s
 *   busySeconds:replications, maxPending:replications
 *   energy:replications                               J
 * with fognet_write_sca's fields and %.14g formatting, from the exact sums (count 0: -nan).  Each
 * is followed by the scalar "<metric> replications lost" where its overflow > 0.
 * append: as fognet_write_sca_nodes. */
int fognet_write_sca_groups(const char *path, const char *run_id, const char *network, int32_t G,
                            const fognet_group_stats *groups, const char *const *module, int append);

/* OMNeT++ .sca blocks of per-user records (host; fognet_per_user_stats_dev /
 * fognet_reduce_user_stats_dev, fognet_hip.h): per module
 * <network>.<user_module[u] or "user[u]">.udpApp[0] the statistics `latency:stats`,
 * `latencyH1:stats` and `taskTime:stats` in ms (raw * 1e-12) with fognet_write_sca's
 * fields and formatting, computed from the exact sums (a user without an emission
 * writes them with count 0), each followed by a scalar "<signal> emissions lost" where
 * its overflow > 0.  Then one `delay:stats` (s) under <network>.broker.udpApp[0] from the
 * exact merge of the U records' delay: it is the broker module's signal
 * (BrokerBaseApp3.cc:143), not a user module's.  append != 0: the blocks are appended to
 * the existing file fognet_write_sca wrote, without a second version/run header;
 * otherwise the file is created with one.  user_module: [U] names, nullable. */
int fognet_write_sca_users(const char *path, const char *run_id, const char *network, int32_t U,
                           const fognet_user_stats *users, const char *const *user_module, int append);

/* OMNeT++ .vec of one replication's per-task outputs (host arrays of length
 * T): vector `queueTime:vector` of every fog node module
 * <network>.fogNode[<node_id or index>].udpApp[0] (value ms, emitted at the
 * task's service start, queued tasks only: ComputeBrokerApp3.cc:238) and
 * `decision:vector` of <network>.broker.udpApp[0] (chosen node index at the
 * publish tick).  Columns "TV" (time, value): the engine has no OMNeT++ event
 * numbers.  Times print as exact decimal seconds (12 fractional digits,
 * trailing zeros trimmed).  node_id: nullable (index names). */
int fognet_write_vec(const char *path, const char *run_id, const char *network, int32_t T, int32_t N,
                     const int64_t *arrive_tick, const int64_t *dl_tick /* [N] */, const int32_t *node,
                     const uint8_t *status, const int64_t *start_tick, const int32_t *node_id);

/* OMNeT++ .vec vectors of the user-side signals of ONE replication (host copies of
 * fognet_signal_vectors_dev's CSR, fognet_hip.h "Signal vectors"): `delay:vector` under
 * <network>.broker.udpApp[0] (value s) and, per module <network>.<user_module[u] or
 * "user[u]">.udpApp[0] (fognet_write_sca_users' names), `latency:vector`, `latencyH1:vector`
 * and `taskTime:vector` (value ms), each with fognet_write_vec's three attr lines, columns
 * "TV", exact decimal times and values raw * 1e-12; rows in the CSR's order.
 * offset: the replication's offset row FROM THE delay VECTOR ON, &offset[N]: 3U + 2 entries
 * (delay, U x latency, U x latencyH1, U x taskTime), indexing the replication's time and
 * value arrays.  Vector ids: id_base for delay, id_base + 1 + 3u + {0, 1, 2} for user u's
 * latency, latencyH1, taskTime (after fognet_write_vec: id_base = N + 1).  A vector without a
 * row is declared and has no data line.  append != 0: the vectors are appended to the file
 * fognet_write_vec wrote, without a second version/run header; otherwise the file is created
 * with one.  user_module: [U] names, nullable. */
int fognet_write_vec_users(const char *path, const char *run_id, const char *network, int32_t U, int32_t id_base,
                           const int64_t *offset, const int64_t *time, const int64_t *value,
                           const char *const *user_module, int append);

/* OMNeT++ .vec vectors of a job's window records (host; fognet_window_stats_dev /
 * fognet_reduce_window_stats_dev, fognet_hip.h): job [W], the exact merge over `replications`
 * replications of N nodes, window w covering [t0_tick + w * window_tick, t0_tick + (w + 1) *
 * window_tick).  Fourteen vectors with ids from id_base, "TV" columns, one row per window at
 * the window's END time (exact decimal seconds, values %.14g):
 *   <network>.fogNodes.udpApp[0]  utilisation:window = busy / (N * window_tick * replications),
 *                                 tasksInSystem:window = insys / (window_tick * replications),
 *                                 completions:window, queueTime:window(mean) (ms),
 *                                 queueTime:window(count)
 *   <network>.broker.udpApp[0]    publishes:window, delay:window(mean) (s), delay:window(count)
 *   <network>.users.udpApp[0]     latency, latencyH1, taskTime: each :window(mean) (ms) and
 *                                 :window(count)
 * The counts are the job's totals; a mean comes from the exact sum (as fognet_write_sca's), and a
 * window whose count is 0 has no row in a mean vector.  append: as fognet_write_vec_users. */
int fognet_write_vec_windows(const char *path, const char *run_id, const char *network, int32_t N, int32_t W,
                             int64_t t0_tick, int64_t window_tick, int64_t replications,
                             const fognet_window_stats *job, int32_t id_base, int append);

/* OMNeT++ .sca scalars of a job's quantiles (host copies of fognet_job_quantiles_dev's results,
 * fognet_hip.h "Quantiles"): ppm [Q] the ranks, value [5][Q] and count [5] in the order queue,
 * delay, latency, latencyH1, taskTime.  One line per signal and rank, in that order,
 *   scalar <module[s]> "<signal>:p<percent>" <value>
 * with the signals named queueTime, delay, latency, latencyH1, taskTime, the percent printed
 * exactly from the ppm without trailing zeros (p50, p99.9, p99.9999) and the value in the recorded
 * units of the statistic's min / max fields (raw * 1e-12, %.14g).  A signal whose count is 0
 * writes no line.  module: [5] module paths, nullable: fognet_write_vec_windows' modules
 * (<network>.fogNodes.udpApp[0], <network>.broker.udpApp[0], 3 x <network>.users.udpApp[0]).
 * append != 0: the lines are appended to an existing file without a second version/run header. */
int fognet_write_sca_quantiles(const char *path, const char *run_id, const char *network,
                               const char *const *module /* [5] */, int32_t Q, const int32_t *ppm,
                               const int64_t *value /* [5][Q] */, const int64_t *count /* [5] */, int append);

/* The reference task source (mqttApp2.cc:198-409 with the ini keys of
 * simulations/example/wirelessNet.ini:48-52), restated as a small event
 * simulation of U users and the broker's CONNECT handling:
 *   START(u) at start_tick[u] (mqttApp2::processStart/processSend): sends
 *     CONNECT (reaches the broker at +uplink_tick[u]) and arms the MQTTDATA
 *     timer at start + interval_tick[u] (if < stop_tick);
 *   CONNECT at the broker (BrokerBaseApp3.cc:99-121): the CONNACK reaches
 *     the user downlink_tick[u] later (downlink_tick[u] < 0: never);
 *   CONNACK at the user (processConSubAck, :319-325): publishes at once;
 *   MQTTDATA (sendMqttData, :353-409): publishes.
 * A publish draws MIPSRequired = req_base + rand() % req_span from ONE glibc
 * rand() stream seeded by srand(seed) (the TYPE_3 additive feedback
 * generator of glibc random_r.c, shared by every user in event order) and,
 * if now + interval < stop_tick, cancels and re-arms the user's timer at
 * now + interval.  Events are processed in OMNeT++ FES order (tick,
 * insertion sequence); the START events are inserted first, in user order.
 * Each publish reaches the broker uplink_tick[u] after it is sent; the trace
 * is ordered by (broker arrival tick, send order), the broker's FES order.
 * Writes at most cap publishes; *out_T = publishes generated
 * (FOGNET_ERR_CAPACITY if > cap, with the first cap written).  user_of
 * (nullable): publishing user of each trace entry. */
int fognet_gen_trace_mqtt(uint32_t seed, int32_t U, const int64_t *start_tick, const int64_t *interval_tick,
                          const int64_t *uplink_tick, const int64_t *downlink_tick, int64_t stop_tick,
                          int32_t req_base, int32_t req_span, int32_t cap, int64_t *arrive_tick,
                          int32_t *req_mips, int32_t *user_of, int32_t *out_T);

#ifdef __cplusplus
}
#endif
#endif /* FOGNET_IO_H */
