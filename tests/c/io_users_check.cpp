// io_users_check.cpp — stand-alone driver of fognet_write_sca_users (io.cpp) for the host
// sanitizer build (`make asan`): a new file and an appended one, named and indexed
// modules, a user without an emission, sums that need the top limbs, lost emissions, the
// broker's delay as the merge of the users' shares, and the error paths.
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

static fognet_user_stats empty_user() {
  fognet_user_stats s;
  memset(&s, 0, sizeof s);
  s.delay.min_raw = s.latency.min_raw = s.latencyH1.min_raw = s.taskTime.min_raw = INT64_MAX;
  s.delay.max_raw = s.latency.max_raw = s.latencyH1.max_raw = s.taskTime.max_raw = INT64_MIN;
  return s;
}

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  std::vector<fognet_user_stats> users(3, empty_user());
  users[0].delay = fognet_moments{2, 1000000000, 1000000000, 2000000000, 0, 2000000000000000000ULL, 0, 0, 0};
  users[0].latencyH1 = fognet_moments{5, 1000, INT64_MAX - 5, ~(uint64_t)0, 1, ~(uint64_t)0, ~(uint64_t)0, 3, 2};
  users[0].taskTime = fognet_moments{1, 7, 7, 7, 0, 49, 0, 0, 0};
  users[2].delay = fognet_moments{1, 5000000000LL, 5000000000LL, 5000000000ULL, 0, 6553255926290448384ULL, 1, 0, 0};
  users[2].latency = fognet_moments{1, -7, -7, (uint64_t)-7, ~(uint64_t)0, 49, 0, 0, 0};  // a negative sum
  const char* names[3] = {"user[3]", "usr[0]", "gw"};
  const std::string p = dir + "/users.sca";
  CHECK(fognet_write_sca_users(p.c_str(), "run-1", "Net", 3, users.data(), nullptr, 0) == FOGNET_OK);
  const std::string fresh = slurp(p);
  CHECK(fresh.compare(0, 10, "version 2\n") == 0);
  CHECK(fresh.find("statistic Net.user[0].udpApp[0] \tlatencyH1:stats\nfield count 5\n") != std::string::npos);
  CHECK(fresh.find("scalar Net.user[0].udpApp[0] \t\"latencyH1 emissions lost\" \t2\n") != std::string::npos);
  CHECK(fresh.find("\"latency emissions lost\"") == std::string::npos);
  CHECK(fresh.find("statistic Net.user[1].udpApp[0] \ttaskTime:stats\nfield count 0\n") != std::string::npos);
  CHECK(fresh.find("statistic Net.broker.udpApp[0] \tdelay:stats\nfield count 3\n") != std::string::npos);
  CHECK(fresh.find("Net.user[0].udpApp[0] \tdelay:stats") == std::string::npos);
  fognet_job_stats job;
  memset(&job, 0, sizeof job);
  const std::string q = dir + "/job_users.sca";
  CHECK(fognet_write_sca(q.c_str(), "run-1", "Net", &job, nullptr) == FOGNET_OK);
  const std::string before = slurp(q);
  CHECK(fognet_write_sca_users(q.c_str(), "run-1", "Net", 3, users.data(), names, 1) == FOGNET_OK);
  const std::string after = slurp(q);
  CHECK(after.compare(0, before.size(), before) == 0);
  CHECK(after.find("version 2", 1) == std::string::npos);
  CHECK(after.find("Net.usr[0].udpApp[0]") != std::string::npos && after.find("Net.gw.udpApp[0]") != std::string::npos);
  CHECK(after.find("Net.user[0]") == std::string::npos);
  CHECK(fognet_write_sca_users((dir + "/no/such/dir.sca").c_str(), "r", "Net", 3, users.data(), nullptr, 0) == FOGNET_ERR_ARG);
  CHECK(strstr(fognet_io_last_error(), "cannot open") != nullptr);
  CHECK(fognet_write_sca_users(p.c_str(), "r", "Net", 3, nullptr, nullptr, 0) == FOGNET_ERR_ARG);
  CHECK(fognet_write_sca_users(nullptr, "r", "Net", 3, users.data(), nullptr, 0) == FOGNET_ERR_ARG);
  const char* holes[3] = {"a", nullptr, "c"};
  CHECK(fognet_write_sca_users(p.c_str(), "r", "Net", 3, users.data(), holes, 0) == FOGNET_ERR_ARG);
  CHECK(fognet_write_sca_users(p.c_str(), "r", "Net", -1, users.data(), nullptr, 0) == FOGNET_ERR_ARG);
  if (failures) return 1;
  puts("io_users_check: all checks passed");
  return 0;
}
