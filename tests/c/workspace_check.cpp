// workspace_check.cpp — the replay workspace layouts of fognetsimpp_amd/csrc/workspace.h: for every
// layout, at the shapes below, the parts are 256-B aligned, follow each other in the declared order
// without overlap and hold their elements, the total is where the last part ends, and the offsets
// and totals equal the literal values the library has always used (any change of them moves device
// memory under kernels that do not know).  Stand-alone: no HIP, no GPU.
#include <stdio.h>

#include <vector>

#include "fognet_hip.h"
#include "workspace.h"

namespace {

using fognet::align256;

int failures = 0;
#define CHECK(cond, ...)                     \
  do {                                       \
    if (!(cond)) {                           \
      printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      printf(__VA_ARGS__);                   \
      printf("\n");                          \
      ++failures;                            \
    }                                        \
  } while (0)

// RegionWs (internal.h) as far as the layout goes: the same field names, elements of the same sizes
// (internal.h asserts its structs' sizes against the same constants).
struct Entry {
  unsigned char b[fognet::kWideEntryBytes];
};
struct Node {
  unsigned char b[fognet::kWideNodeBytes];
};
struct Rec {
  unsigned char b[fognet::kRegionRecBytes];
};
struct RegionWs {
  Entry* e;
  Node* nd;
  Rec* rec;
  uint32_t* vb;
  int32_t *esc, *s_idx;
  unsigned char* pacc;
  int32_t* seg;
  int64_t* s_arr;
  int32_t *s_req, *inv, *o_node;
  uint8_t* o_status;
  int64_t *o_start, *o_done, *tails;
  uint32_t* okey;
  int32_t* perm;
};

// one part as the check expects it: the field the layout bound, and the bytes its elements need
struct Part {
  const void* p;
  size_t bytes;
};

// Measures a layout, then binds it over a real allocation of that size (walk(cursor) returns the total).
template <class Walk>
size_t measure_and_bind(const char* what, Walk walk, std::vector<unsigned char>& mem) {
  fognet::WsCursor size{nullptr};
  const size_t total = walk(size);
  mem.assign(total, 0);
  fognet::WsCursor bind{mem.data()};
  const size_t again = walk(bind);
  CHECK(again == total, "%s: measured %zu, bound %zu", what, total, again);
  return total;
}

// The parts, in the declared order, lie at the literal offsets `want`, each 256-B aligned and ending
// before the next begins; the last one ends within `total`.
void check_parts(const char* what, const std::vector<unsigned char>& mem, const std::vector<Part>& parts,
                 const std::vector<size_t>& want, size_t total) {
  CHECK(parts.size() == want.size(), "%s: %zu parts, %zu offsets", what, parts.size(), want.size());
  for (size_t i = 0; i < parts.size() && i < want.size(); ++i) {
    const size_t off = (size_t)((const unsigned char*)parts[i].p - mem.data());
    CHECK(off == want[i], "%s part %zu: offset %zu, expected %zu", what, i, off, want[i]);
    CHECK(off % 256 == 0, "%s part %zu: offset %zu not 256-B aligned", what, i, off);
    const size_t next = i + 1 < parts.size() ? (size_t)((const unsigned char*)parts[i + 1].p - mem.data()) : total;
    CHECK(off + parts[i].bytes <= next, "%s part %zu: [%zu, +%zu) runs into the next part at %zu", what, i, off,
          parts[i].bytes, next);
  }
}

// (R, N, ring, T); fb: the hand-over launch's wide workspace for the slots that fit (smaller than the
// rings in the first shape, larger in the second)
void check_register(size_t R, size_t N, size_t ring, size_t T, size_t fb, bool outputs, const std::vector<size_t>& offsets,
                    size_t want_total) {
  char what[96];
  snprintf(what, sizeof what, "register (%zu, %zu, %zu, %zu) outputs=%d", R, N, ring, T, (int)outputs);
  fognet::ReplayWs w{};
  std::vector<unsigned char> mem;
  const size_t ring_bytes = R * N * ring * 8, RT = outputs ? R * T : 0;
  const size_t total = measure_and_bind(
      what, [&](fognet::WsCursor& v) { return fognet::register_ws(w, R, ring_bytes, fb, RT, v); }, mem);
  check_parts(what, mem,
              {{w.count, 4}, {w.list, R * 4}, {w.board, fognet::kBoardWords * 4}, {w.body, ring_bytes > fb ? ring_bytes : fb},
               {w.out_node, RT * 4}, {w.out_status, RT}, {w.out_start, RT * 8}, {w.out_done, RT * 8}},
              offsets, total);
  // (the total is the end of the last part, padded like every part)
  CHECK(total == align256(offsets.back() + RT * 8), "%s: total %zu is not the last part's end", what, total);
  CHECK(total == want_total, "%s: total %zu, expected %zu", what, total, want_total);
}

void check_generated(size_t R, size_t slots, size_t N, size_t ring, size_t fb, size_t want_total) {
  char what[96];
  snprintf(what, sizeof what, "generated (%zu, %zu, %zu, %zu) fb=%zu", R, slots, N, ring, fb);
  fognet::ReplayWs w{};
  std::vector<unsigned char> mem;
  const size_t ring_bytes = slots * N * ring * 8, body = ring_bytes > fb ? ring_bytes : fb;
  const size_t total = measure_and_bind(
      what, [&](fognet::WsCursor& v) { return fognet::generated_ws(w, R, ring_bytes, fb, v); }, mem);
  // hand-over counter @0 and work counter @4 in the first part
  check_parts(what, mem, {{w.count, 8}, {w.list, R * 4}, {w.body, body}}, {0, 256, 40448}, total);
  CHECK(total == 40448 + body, "%s: total %zu is not the last part's end", what, total);
  CHECK(total == want_total, "%s: total %zu, expected %zu", what, total, want_total);
  CHECK(w.board == nullptr && w.out_node == nullptr, "%s: no board, no outputs", what);
}

// (R, T, N); fb: the wide workspace of min(R, 1024) slots (larger than the second half in the first
// shape, smaller in the second); offsets: the 20 parts before the wide workspace
void check_region(size_t R, size_t T, size_t N, size_t fb, bool resume, const std::vector<size_t>& offsets, size_t want_wide,
                  size_t want_total) {
  char what[96];
  snprintf(what, sizeof what, "region (%zu, %zu, %zu) resume=%d", R, T, N, (int)resume);
  const size_t B = (N + FOGNET_HIER_REGION_NODES - 1) / FOGNET_HIER_REGION_NODES, RT = R * T, RB = R * B;
  fognet::ReplayWs h{};
  RegionWs w{};
  std::vector<unsigned char> mem;
  const size_t total = measure_and_bind(
      what, [&](fognet::WsCursor& v) { return fognet::region_ws(h, w, R, T, N, B, fb, resume, v); }, mem);
  const size_t o_e = offsets[9], o_end = align256(offsets[19] + RT * 4), body = o_end - o_e;
  check_parts(what, mem,
              {{h.count, 4}, {h.list, R * 4}, {w.esc, R * 4}, {w.rec, RB * 16}, {w.seg, R * (B + 1) * 4}, {w.okey, RB * 4},
               {w.perm, RB * 4}, {w.pacc, R * fognet::kRegionResumeBytes}, {w.tails, R * N * 16}, {w.e, RT * 40},
               {w.nd, R * N * 64}, {w.vb, RB * 1024 * 4}, {w.s_arr, RT * 8}, {w.s_req, RT * 4}, {w.inv, RT * 4},
               {w.o_node, RT * 4}, {w.o_status, RT}, {w.o_start, RT * 8}, {w.o_done, RT * 8}, {w.s_idx, RT * 4}},
              offsets, o_end);
  const size_t o_wide = (size_t)(h.body - mem.data());
  CHECK(o_wide == want_wide && o_wide % 256 == 0, "%s: wide workspace at %zu, expected %zu", what, o_wide, want_wide);
  if (resume) {
    CHECK(o_wide == o_e + body, "%s: wide workspace at %zu, not after the second half (%zu)", what, o_wide, o_e + body);
    CHECK(total == o_wide + fb, "%s: total %zu", what, total);
  } else {
    CHECK(o_wide == o_e, "%s: wide workspace at %zu, not over the entries (%zu)", what, o_wide, o_e);
    CHECK(total == o_e + (body > fb ? body : fb), "%s: total %zu", what, total);
  }
  CHECK(total == want_total, "%s: total %zu, expected %zu", what, total, want_total);
}

}  // namespace

int main() {
  check_register(3, 5, 2048, 65, 71168, false, {0, 256, 512, 524800, 770560, 770560, 770560, 770560}, 770560);
  check_register(3, 5, 2048, 65, 71168, true, {0, 256, 512, 524800, 770560, 771584, 771840, 773632}, 775424);
  check_register(8, 256, 4, 2000, 126912, false, {0, 256, 512, 524800, 651776, 651776, 651776, 651776}, 651776);
  check_register(8, 256, 4, 2000, 126912, true, {0, 256, 512, 524800, 651776, 715776, 731904, 859904}, 987904);
  check_generated(10000, 3072, 256, 4, 25089152, 25206272);
  check_generated(10000, 3072, 256, 4, 25178169, 25218617);  // the wide workspace larger: the total is not padded
  const std::vector<size_t> small = {0,      256,    512,    768,    1024,   1280,   1536,   1792,   2560,   101376,
                                     124416, 518912, 555776, 560384, 562688, 564992, 567296, 568064, 572672, 577280};
  check_region(3, 191, 2054, 653312, false, small, 101376, 754688);
  check_region(3, 191, 2054, 653312, true, small, 579584, 1232896);
  const std::vector<size_t> large = {0,       256,     512,     768,     1536,     1792,     2048,     2304,     3072,     643072,
                                     5885952, 8445952, 8609792, 9658368, 10182656, 10706944, 11231232, 11362304, 12410880, 13459456};
  check_region(4, 32768, 10000, 9466368, false, large, 643072, 13983744);
  check_region(4, 32768, 10000, 9466368, true, large, 13983744, 23450112);
  if (failures) {
    printf("workspace: %d checks failed\n", failures);
    return 1;
  }
  printf("workspace: all checks passed\n");
  return 0;
}
