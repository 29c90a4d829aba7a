// io_windows_check.cpp — stand-alone driver of fognet_write_vec_windows (io.cpp) for the host
// sanitizer build (`make asan`): a new file and an appended one, a window without an emission,
// utilisation and tasks in system from sums that need the high limbs, no window at all, and the
// error paths.  The records come from the host identity and merge of fognet_window_stats, which
// are checked for their values here but are NOT sanitised here: they run from the library as it
// ships (stats_check.cpp instruments them); only io.cpp and this file are instrumented.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "fognet_io.h"

static int failures = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);     \
      ++failures;                                                 \
    }                                                             \
  } while (0)

static std::string slurp(const std::string& path) {
  std::string s;
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return s;
  char buf[4096];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, n);
  fclose(f);
  return s;
}

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  // identity and merge
  fognet_window_stats e;
  memset(&e, 0x5A, sizeof e);
  fognet_window_stats_init(&e);
  CHECK(e.n_publish == 0 && e.busy_hi == 0 && e.queue.min_raw == INT64_MAX && e.taskTime.max_raw == INT64_MIN);
  fognet_window_stats a = e, b = e;
  a.n_publish = 3, a.n_complete = 2, a.busy_lo = ~(uint64_t)0, a.insys_lo = 5, a.insys_hi = 1;
  a.delay = fognet_moments{2, 1000000000, 3000000000LL, 4000000000ULL, 0, 10000000000000000000ULL, 0, 0, 0};
  b.n_publish = 1, b.busy_lo = 2, b.insys_lo = ~(uint64_t)0;
  b.delay = fognet_moments{1, 5, 5, 5, 0, 25, 0, 0, 1};
  b.latency = fognet_moments{1, -7, -7, (uint64_t)-7, ~(uint64_t)0, 49, 0, 0, 0};  // a negative sum
  fognet_window_stats m = a;
  fognet_window_stats_merge(&m, &b);
  CHECK(m.n_publish == 4 && m.n_complete == 2 && m.busy_lo == 1 && m.busy_hi == 1 && m.insys_lo == 4 && m.insys_hi == 2);
  CHECK(m.delay.count == 3 && m.delay.min_raw == 5 && m.delay.max_raw == 3000000000LL && m.delay.overflow == 1);
  CHECK(m.latency.count == 1 && (int64_t)m.latency.sum_lo == -7 && m.latency.sum_hi == ~(uint64_t)0);
  fognet_window_stats n = e;
  fognet_window_stats_merge(&n, &m);
  CHECK(memcmp(&n, &m, sizeof m) == 0);  // the identity
  fognet_window_stats_merge(nullptr, &m), fognet_window_stats_merge(&m, nullptr), fognet_window_stats_init(nullptr);
  // the writer
  std::vector<fognet_window_stats> job = {m, e, a};
  const std::string p = dir + "/windows.vec";
  CHECK(fognet_write_vec_windows(p.c_str(), "run-1", "Net", 5, 3, 0, 2500000000000LL, 4, job.data(), 0, 0) == FOGNET_OK);
  const std::string fresh = slurp(p);
  CHECK(fresh.compare(0, 10, "version 2\n") == 0);
  CHECK(fresh.find("vector 0  Net.fogNodes.udpApp[0]  utilisation:window  TV\n") != std::string::npos);
  CHECK(fresh.find("vector 13  Net.users.udpApp[0]  taskTime:window(count)  TV\n") != std::string::npos);
  // utilisation = busy / (N * window * replications) with busy = 2^64 + 1 (the high limb alone carries it), 0, 2^64 - 1
  CHECK(fresh.find("\n0\t2.5\t368934.88147419\n0\t5\t0\n0\t7.5\t368934.88147419\n") != std::string::npos);
  // tasks in system = insys / (window * replications) with insys = 2 * 2^64 + 4, 0, 2^64 + 5
  CHECK(fresh.find("\n1\t2.5\t3689348.8147419\n1\t5\t0\n1\t7.5\t1844674.407371\n") != std::string::npos);
  CHECK(fresh.find("\n2\t2.5\t2\n2\t5\t0\n2\t7.5\t2\n") != std::string::npos);  // completions
  CHECK(fresh.find("\n5\t2.5\t4\n5\t5\t0\n5\t7.5\t3\n") != std::string::npos);  // publishes, at each window's end
  CHECK(fresh.find("\n7\t2.5\t3\n7\t5\t0\n7\t7.5\t2\n") != std::string::npos);  // delay counts
  CHECK(fresh.find("\n6\t5\t") == std::string::npos);                           // no mean where nothing was emitted
  CHECK(fresh.find("\n8\t2.5\t-7e-12\n") != std::string::npos);                 // latency mean (ms) from the exact sum
  const std::string q = dir + "/job_windows.vec";
  const int64_t z = 0;
  const int32_t zn = 0;
  const uint8_t zs = 5;
  CHECK(fognet_write_vec(q.c_str(), "run-1", "Net", 1, 1, &z, &z, &zn, &zs, &z, nullptr) == FOGNET_OK);
  const std::string before = slurp(q);
  CHECK(fognet_write_vec_windows(q.c_str(), "run-1", "Net", 5, 3, 0, 2500000000000LL, 4, job.data(), 2, 1) == FOGNET_OK);
  const std::string after = slurp(q);
  CHECK(after.compare(0, before.size(), before) == 0 && after.find("version 2", 1) == std::string::npos);
  CHECK(after.find("vector 2  Net.fogNodes.udpApp[0]  utilisation:window  TV\n") != std::string::npos);
  CHECK(after.find("vector 15  Net.users.udpApp[0]  taskTime:window(count)  TV\n") != std::string::npos);
  CHECK(fognet_write_vec_windows(p.c_str(), "r", "Net", 5, 0, 0, 1, 1, nullptr, 0, 0) == FOGNET_OK);  // no window: no row
  CHECK(slurp(p).find("\n0\t") == std::string::npos);
  CHECK(fognet_write_vec_windows((dir + "/no/such/dir.vec").c_str(), "r", "Net", 5, 3, 0, 1, 1, job.data(), 0, 0) == FOGNET_ERR_ARG);
  CHECK(strstr(fognet_io_last_error(), "cannot open") != nullptr);
  CHECK(fognet_write_vec_windows(p.c_str(), "r", "Net", 5, 3, 0, 1, 1, nullptr, 0, 0) == FOGNET_ERR_ARG);
  CHECK(fognet_write_vec_windows(nullptr, "r", "Net", 5, 3, 0, 1, 1, job.data(), 0, 0) == FOGNET_ERR_ARG);
  CHECK(fognet_write_vec_windows(p.c_str(), "r", "Net", 0, 3, 0, 1, 1, job.data(), 0, 0) == FOGNET_ERR_ARG);
  CHECK(fognet_write_vec_windows(p.c_str(), "r", "Net", 5, 3, 0, 0, 1, job.data(), 0, 0) == FOGNET_ERR_ARG);
  CHECK(fognet_write_vec_windows(p.c_str(), "r", "Net", 5, 3, -1, 1, 1, job.data(), 0, 0) == FOGNET_ERR_ARG);
  CHECK(fognet_write_vec_windows(p.c_str(), "r", "Net", 5, 3, 0, 1, 0, job.data(), 0, 0) == FOGNET_ERR_ARG);
  CHECK(fognet_write_vec_windows(p.c_str(), "r", "Net", 5, 3, 0, (int64_t)1 << 61, 1, job.data(), 0, 0) == FOGNET_ERR_ARG);
  if (failures) return 1;
  puts("io_windows_check: all checks passed");
  return 0;
}
