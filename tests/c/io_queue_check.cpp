// io_queue_check.cpp — stand-alone driver of fognet_write_sca_queue (io.cpp) for the host
// sanitizer build (`make asan`): a new file and an appended one, named and indexed modules,
// 128-bit sums, an unobserved record, every number of levels, and the error paths.
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
  std::vector<fognet_queue_stats> qs(3);
  memset(qs.data(), 0, qs.size() * sizeof(fognet_queue_stats));
  fognet_queue_stats& a = qs[0];
  a.n_enq = 12345, a.max_len = 41;
  a.observed_lo = 0, a.observed_hi = 4;  // 2^66 ticks observed (a merged job)
  a.area_lo = 0, a.area_hi = 6;          // time average 1.5
  a.time_ge[0][0] = 0, a.time_ge[0][1] = 4;
  a.time_ge[1][0] = 0, a.time_ge[1][1] = 1;
  a.time_ge[7][0] = 1;
  qs[1].observed_lo = 1000;              // observed, never queued
  const int64_t level[8] = {1, 2, 3, 4, 5, 6, 7, 1000000000000LL};
  const int32_t ids[3] = {7, 3, 11};
  const std::string p = dir + "/queue.sca";
  CHECK(fognet_write_sca_queue(p.c_str(), "run-1", "Net", 3, qs.data(), level, 8, nullptr, 0) == FOGNET_OK);
  const std::string fresh = slurp(p);
  CHECK(fresh.compare(0, 10, "version 2\n") == 0);
  CHECK(fresh.find("scalar Net.fogNode[0].udpApp[0] \tqueueLength:max \t41\n") != std::string::npos);
  CHECK(fresh.find("scalar Net.fogNode[0].udpApp[0] \tqueueLength:enqueued \t12345\n") != std::string::npos);
  CHECK(fresh.find("scalar Net.fogNode[0].udpApp[0] \tqueueLength:timeavg \t1.5\n") != std::string::npos);
  CHECK(fresh.find("scalar Net.fogNode[0].udpApp[0] \tqueueLength:ge1 \t1\n") != std::string::npos);
  CHECK(fresh.find("scalar Net.fogNode[0].udpApp[0] \tqueueLength:ge2 \t0.25\n") != std::string::npos);
  CHECK(fresh.find("scalar Net.fogNode[0].udpApp[0] \tqueueLength:ge1000000000000 \t") != std::string::npos);
  CHECK(fresh.find("scalar Net.fogNode[1].udpApp[0] \tqueueLength:timeavg \t0\n") != std::string::npos);
  CHECK(fresh.find("scalar Net.fogNode[2].udpApp[0] \tqueueLength:timeavg \t-nan\n") != std::string::npos);  // nothing observed
  for (int32_t Q = 0; Q <= 8; ++Q)
    CHECK(fognet_write_sca_queue(p.c_str(), "run-1", "Net", 3, qs.data(), level, Q, nullptr, 0) == FOGNET_OK);
  fognet_job_stats job;
  memset(&job, 0, sizeof job);
  const std::string q = dir + "/job_queue.sca";
  CHECK(fognet_write_sca(q.c_str(), "run-1", "Net", &job, nullptr) == FOGNET_OK);
  const std::string before = slurp(q);
  CHECK(fognet_write_sca_queue(q.c_str(), "run-1", "Net", 3, qs.data(), level, 2, ids, 1) == FOGNET_OK);
  const std::string after = slurp(q);
  CHECK(after.compare(0, before.size(), before) == 0);
  CHECK(after.find("version 2", 1) == std::string::npos);
  CHECK(after.find("Net.fogNode[11].udpApp[0]") != std::string::npos && after.find("Net.fogNode[0]") == std::string::npos);
  CHECK(after.find("queueLength:ge3") == std::string::npos);
  CHECK(fognet_write_sca_queue(q.c_str(), "run-1", "Net", 0, nullptr, level, 2, nullptr, 1) == FOGNET_OK);  // N = 0: nothing added
  CHECK(slurp(q) == after);
  CHECK(fognet_write_sca_queue((dir + "/no/such/dir.sca").c_str(), "r", "Net", 3, qs.data(), level, 2, nullptr, 0) == FOGNET_ERR_ARG);
  CHECK(strstr(fognet_io_last_error(), "cannot open") != nullptr);
  CHECK(fognet_write_sca_queue(p.c_str(), "r", "Net", 3, nullptr, level, 2, nullptr, 0) == FOGNET_ERR_ARG);
  CHECK(fognet_write_sca_queue(p.c_str(), "r", "Net", 3, qs.data(), nullptr, 2, nullptr, 0) == FOGNET_ERR_ARG);
  CHECK(fognet_write_sca_queue(p.c_str(), "r", "Net", 3, qs.data(), level, 9, nullptr, 0) == FOGNET_ERR_ARG);
  CHECK(fognet_write_sca_queue(nullptr, "r", "Net", 3, qs.data(), level, 2, nullptr, 0) == FOGNET_ERR_ARG);
  if (failures) return 1;
  puts("io_queue_check: all checks passed");
  return 0;
}
