// workspace.h — the layouts of the replay workspaces that capi.hip carves out of a context's one
// grow-only allocation.  Host-only C++17 (no HIP): each layout is one ordered list of its parts,
// and both its size and its pointers come from a cursor's walk over that list.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "fognet_hip.h"

namespace fognet {

// Element sizes of the parts whose types live with the kernels (internal.h ties each to its struct
// with a static_assert), and the parts of fixed size.
constexpr size_t kWideEntryBytes = 40, kWideNodeBytes = 64, kRegionRecBytes = 16;
constexpr size_t kBoardWords = (size_t)1 << 17;  // 8 XCC x 8 SE x 2 SH x 16 CU x 4 SIMD x 16 slots
constexpr size_t kRegionResumeBytes = 192;       // >= sizeof(Acc) + sizeof(AbortPt) (replay_common.h)

constexpr size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Walks a layout: every part starts 256-B aligned, after the one before it.  base == nullptr only
// measures; otherwise each part's pointer is set as well.
struct WsCursor {
  unsigned char* base;
  size_t off = 0;  // where the next part starts
  size_t end = 0;  // where the last part's elements ended (before padding)
  template <class T>
  void operator()(T*& p, size_t count) {
    if (base) p = reinterpret_cast<T*>(base + off);
    end = off + count * sizeof(T);
    off = align256(end);
  }
};

// The parts that are not fields of a kernel-side struct.
struct ReplayWs {
  int32_t* count;   // hand-over counter at byte 0; generated: count[1] is the work counter
  int32_t* list;    // [R] hand-over list, at byte 256
  uint32_t* board;  // [kBoardWords] replay_kernel's progress board
  // the register kernel's pending-task rings and, once that kernel is done (stream order), the workspace of
  // the wide kernel's replay of the handed-over replications (its own layout: wide_ws, replay_wide.hip)
  unsigned char* body;
  // [R][T] per-task outputs of a statistics-only replay, which the fused statistics epilogue reads back
  int32_t* out_node;
  uint8_t* out_status;
  int64_t *out_start, *out_done;
};

// Register replay: [counter | list | board | body | out_node, out_status, out_start, out_done].
// The board is there even when the in-loop kernel does not use it, and the outputs hold RT = 0
// elements unless the replay is statistics-only with the epilogue's re-read.  Returns the total.
inline size_t register_ws(ReplayWs& w, size_t R, size_t ring_bytes, size_t fb_bytes, size_t RT, WsCursor& v) {
  v(w.count, 64), v(w.list, R), v(w.board, kBoardWords), v(w.body, ring_bytes > fb_bytes ? ring_bytes : fb_bytes);
  v(w.out_node, RT), v(w.out_status, RT), v(w.out_start, RT), v(w.out_done, RT);
  return v.off;
}

// Generated replay: [hand-over counter, work counter | list | body]: no board, the rings in body are
// those of the resident workgroups (gen_slots) only, and the total is not padded.
inline size_t generated_ws(ReplayWs& w, size_t R, size_t ring_bytes, size_t fb_bytes, WsCursor& v) {
  v(w.count, 64), v(w.list, R), v(w.body, ring_bytes > fb_bytes ? ring_bytes : fb_bytes);
  return v.end;
}

// Region replay (EXT_HIER, replay_region.hip; W: RegionWs, whose fields say what each part holds):
// [counter | list | first escalations | region records | segment offsets | dispatch keys | dispatch
// order | resume records | node tails || entries | node records | busy view | region-sorted trace |
// inv | region-sorted outputs | s_idx] + the hand-over launch's wide workspace of fb_bytes in w.body.
// With resume the wide kernel reads the region state, so its workspace lies after everything; without,
// it overlaps the second half from the entries on, which is safe in stream order: the hand-over launch
// follows the finish kernel, the last reader of the node records and the sorted outputs.
template <class W>
size_t region_ws(ReplayWs& h, W& w, size_t R, size_t T, size_t N, size_t B, size_t fb_bytes, bool resume, WsCursor& v) {
  const size_t RT = R * T, RB = R * B;
  v(h.count, 64), v(h.list, R), v(w.esc, R), v(w.rec, RB), v(w.seg, R * (B + 1)), v(w.okey, RB), v(w.perm, RB);
  v(w.pacc, R * kRegionResumeBytes), v(w.tails, R * N * 2);
  const size_t o_e = v.off;
  v(w.e, RT), v(w.nd, R * N), v(w.vb, RB * FOGNET_HIER_REGION_NODES), v(w.s_arr, RT), v(w.s_req, RT), v(w.inv, RT);
  v(w.o_node, RT), v(w.o_status, RT), v(w.o_start, RT), v(w.o_done, RT), v(w.s_idx, RT);
  const size_t o_end = v.off;
  if (!resume) v.off = o_e;
  v(h.body, fb_bytes);
  return resume || v.end > o_end ? v.end : o_end;
}

// Signal vectors (signal_vectors.hip): [cursors].  One 32-bit cursor per (replication, vector) of the
// place kernel, which zeroes its replication's row itself; used only above the kernel's LDS capacity
// (or when the HBM layouts are forced), but sized for every call so the layout has one form.
struct VecWs {
  uint32_t* cursor;  // [Rv][V] rows placed so far in each vector's segment
};

inline size_t signal_vectors_ws(VecWs& w, size_t Rv, size_t V, WsCursor& v) {
  v(w.cursor, Rv * V);
  return v.off;
}

// Window statistics (window_stats.hip): [deltas].  Two cover-count deltas (busy, insys) per
// (replication, window): the difference arrays of the windows that an interval covers whole,
// zeroed by the kernel itself.  delta_n = R * W * 2 above the kernel's LDS capacity or when the
// workspace layout is forced, else 0 (the deltas then live in LDS beside the records).
struct WindowWs {
  int64_t* delta;  // [R][W][2]
};

inline size_t window_stats_ws(WindowWs& w, size_t delta_n, WsCursor& v) {
  v(w.delta, delta_n);
  return v.off;
}

// Job quantiles (quantiles.hip): [table | state].  table: the round's [5][Q][256] 64-bit counters,
// which every replication's workgroup adds its bins to and the pick kernel clears; state: the job's
// select state (quantiles.hip's QState: prefixes, ranks, extents and which ranks share a histogram),
// read by the row launches and rewritten by the pick launches between them.  Both are cleared by the
// call's first launch, so nothing depends on what the workspace held.
constexpr size_t kQuantStateBytes = 840;
struct QuantWs {
  uint64_t* table;  // [5][Q][256]
  uint64_t* state;  // [kQuantStateBytes / 8]
};

inline size_t quantiles_ws(QuantWs& w, size_t table_n, WsCursor& v) {
  v(w.table, table_n), v(w.state, kQuantStateBytes / 8);
  return v.off;
}

// Assigned replay (replay_assigned.hip): [refusal flags | node offsets | advert rows || carries].
// off: the exclusive scan of the tasks per node, one row of N + 1 per replication; adv: every
// task's completion advert tick, grouped by node in trace order (row off[k] + rank); the five
// carry arrays hold what a node carries from tile to tile where it does not fit in LDS (carry_n
// = R * N above the kernel's LDS capacity or when the workspace layout is forced, else 0).
struct AssignedWs {
  int32_t* bad;      // [R] 1: refused by the validation pass
  uint32_t* off;     // [R][N + 1]
  int64_t* adv;      // [R][T]
  int64_t* c_done;   // [R][N] the carries (replay_assigned.hip says what each holds)
  uint64_t* c_busy;
  uint32_t *c_S, *c_rank, *c_head;
};

inline size_t assigned_ws(AssignedWs& w, size_t R, size_t T, size_t N, size_t carry_n, WsCursor& v) {
  v(w.bad, R), v(w.off, R * (N + 1)), v(w.adv, R * T);
  v(w.c_done, carry_n), v(w.c_busy, carry_n), v(w.c_S, carry_n), v(w.c_rank, carry_n), v(w.c_head, carry_n);
  return v.off;
}

// Queue-length statistics (queue_stats.hip): [node offsets | elements || carries].  off: the
// exclusive scan of the queued tasks per node, one row of N + 1 per replication; the elements of a
// replication (at most T: its queued tasks) are four columns grouped by node in FIFO order (row
// off[k] + rank): the tick the task was enqueued, the tick it left, the start of the task served
// before it, and its node; the two carry arrays hold what a node carries from tile to tile of the
// build kernel where it does not fit in LDS (carry_n = R * N above that kernel's LDS capacity or
// when the workspace layout is forced, else 0).  R: the replications of one round.
struct QueueWs {
  uint32_t* off;     // [R][N + 1]
  int64_t* at;       // [R][T]
  int64_t* leave;    // [R][T]
  int64_t* prev;     // [R][T]
  int32_t* node;     // [R][T]
  int64_t* c_start;  // [R][N] the carries (queue_stats.hip says what each holds)
  uint32_t* c_rank;
};

constexpr size_t kQueueElementBytes = 28;

inline size_t queue_stats_ws(QueueWs& w, size_t R, size_t T, size_t N, size_t carry_n, WsCursor& v) {
  v(w.off, R * (N + 1)), v(w.at, R * T), v(w.leave, R * T), v(w.prev, R * T), v(w.node, R * T);
  v(w.c_start, carry_n), v(w.c_rank, carry_n);
  return v.off;
}

}  // namespace fognet
