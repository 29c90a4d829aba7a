// io_nodes_check.cpp — stand-alone driver of fognet_write_sca_nodes (io.cpp) for the host
// sanitizer build (`make asan`): a new file and an appended one, named and indexed
// modules, an empty node, sums that need the top limbs, and the error paths.
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

static fognet_node_stats empty_node() {
  fognet_node_stats s;
  memset(&s, 0, sizeof s);
  s.last_tick = s.queue.max_raw = s.resp.max_raw = INT64_MIN;
  s.queue.min_raw = s.resp.min_raw = INT64_MAX;
  return s;
}

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  std::vector<fognet_node_stats> nodes(3, empty_node());
  fognet_node_stats& a = nodes[0];
  a.n_tasks = 9, a.n_queued = 6, a.n_started = 2, a.n_lost = 1, a.busy_s = 123, a.last_tick = 77;
  a.queue = fognet_moments{5, -1000, INT64_MAX - 5, ~(uint64_t)0, 1, ~(uint64_t)0, ~(uint64_t)0, 3, 2};
  a.resp = fognet_moments{3, 5, 1000000000000LL, 1000000000012LL, 0, 1, 54210, 0, 0};
  nodes[2].queue = fognet_moments{1, -7, -7, (uint64_t)-7, ~(uint64_t)0, 49, 0, 0, 0};  // a negative sum
  const int32_t ids[3] = {7, 3, 11};
  const std::string p = dir + "/nodes.sca";
  CHECK(fognet_write_sca_nodes(p.c_str(), "run-1", "Net", 3, nodes.data(), nullptr, 0) == FOGNET_OK);
  const std::string fresh = slurp(p);
  CHECK(fresh.compare(0, 10, "version 2\n") == 0);
  CHECK(fresh.find("scalar Net.fogNode[0].udpApp[0] \ttasks \t9\n") != std::string::npos);
  CHECK(fresh.find("statistic Net.fogNode[1].udpApp[0] \tqueueTime:stats\nfield count 0\n") != std::string::npos);
  CHECK(fresh.find("statistic Net.fogNode[2].udpApp[0] \tresponse:stats\nfield count 0\n") != std::string::npos);
  fognet_job_stats job;
  memset(&job, 0, sizeof job);
  const std::string q = dir + "/job_nodes.sca";
  CHECK(fognet_write_sca(q.c_str(), "run-1", "Net", &job, nullptr) == FOGNET_OK);
  const std::string before = slurp(q);
  CHECK(fognet_write_sca_nodes(q.c_str(), "run-1", "Net", 3, nodes.data(), ids, 1) == FOGNET_OK);
  const std::string after = slurp(q);
  CHECK(after.compare(0, before.size(), before) == 0);
  CHECK(after.find("version 2", 1) == std::string::npos);
  CHECK(after.find("Net.fogNode[11].udpApp[0]") != std::string::npos && after.find("Net.fogNode[0]") == std::string::npos);
  CHECK(fognet_write_sca_nodes(q.c_str(), "run-1", "Net", 0, nullptr, nullptr, 1) == FOGNET_OK);  // N = 0: nothing added
  CHECK(slurp(q) == after);
  CHECK(fognet_write_sca_nodes((dir + "/no/such/dir.sca").c_str(), "r", "Net", 3, nodes.data(), nullptr, 0) == FOGNET_ERR_ARG);
  CHECK(strstr(fognet_io_last_error(), "cannot open") != nullptr);
  CHECK(fognet_write_sca_nodes(p.c_str(), "r", "Net", 3, nullptr, nullptr, 0) == FOGNET_ERR_ARG);
  CHECK(fognet_write_sca_nodes(nullptr, "r", "Net", 3, nodes.data(), nullptr, 0) == FOGNET_ERR_ARG);
  if (failures) return 1;
  puts("io_nodes_check: all checks passed");
  return 0;
}
