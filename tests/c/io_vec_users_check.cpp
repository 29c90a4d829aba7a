// io_vec_users_check.cpp — stand-alone driver of fognet_write_vec_users (io.cpp) for the host
// sanitizer build (`make asan`): a new file and one appended after fognet_write_vec, named and
// indexed modules, id_base, vectors without a row, U = 0, and the error paths.
#include <stdio.h>

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

static size_t count(const std::string& s, const std::string& what) {
  size_t n = 0;
  for (size_t p = s.find(what); p != std::string::npos; p = s.find(what, p + 1)) ++n;
  return n;
}

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  const int64_t MS = 1000000000LL;
  // U = 2 after N = 3 nodes: the offset row from the delay vector on (4 queueTime rows before it);
  // delay 3 rows, latency (1, 0), latencyH1 (2, 1), taskTime (0, 2)
  const std::vector<int64_t> offset = {4, 7, 8, 8, 10, 11, 11, 13};
  std::vector<int64_t> time(13), value(13, 0);
  for (int i = 0; i < 13; ++i) time[i] = i * 250 * MS + 1;
  time[7] = 2000 * MS;
  value[4] = MS, value[5] = 2 * MS, value[6] = MS, value[7] = 5000 * MS, value[8] = 6000 * MS, value[9] = 6000 * MS + 1;
  value[10] = 7000 * MS, value[11] = 3000000 * MS, value[12] = -1000;
  const char* names[2] = {"user[3]", "gw"};
  const std::string p = dir + "/users.vec";
  CHECK(fognet_write_vec_users(p.c_str(), "run-1", "Net", 2, 4, offset.data(), time.data(), value.data(), names, 0) ==
        FOGNET_OK);
  const std::string fresh = slurp(p);
  CHECK(fresh.compare(0, 10, "version 2\n") == 0 && count(fresh, "version 2") == 1);
  CHECK(fresh.find("vector 4  Net.broker.udpApp[0]  delay:vector  TV\nattr interpolationmode  none\nattr source  delay\n"
                   "attr title  \"delay, vector\"\n") != std::string::npos);
  CHECK(fresh.find("vector 5  Net.user[3].udpApp[0]  latency:vector  TV\n") != std::string::npos);
  CHECK(fresh.find("vector 10  Net.gw.udpApp[0]  taskTime:vector  TV\n") != std::string::npos);
  CHECK(fresh.find("\n4\t1.000000000001\t0.001\n4\t1.250000000001\t0.002\n4\t1.500000000001\t0.001\n5\t2\t5\n") !=
        std::string::npos);
  CHECK(fresh.find("\n10\t2.750000000001\t3000\n10\t3.000000000001\t-1e-09\n") != std::string::npos);
  CHECK(fresh.find("\n7\t") == std::string::npos && fresh.find("\n8\t") == std::string::npos);  // declared, no rows
  // appended after fognet_write_vec: one header, the same vectors behind it
  const std::string q = dir + "/job.vec";
  const int64_t arrive[2] = {MS, 2 * MS}, dl[3] = {MS, MS, MS}, start[2] = {2 * MS, 3 * MS};
  const int32_t node[2] = {0, 1};
  const uint8_t status[2] = {5, 4};
  CHECK(fognet_write_vec(q.c_str(), "run-1", "Net", 2, 3, arrive, dl, node, status, start, nullptr) == FOGNET_OK);
  const std::string before = slurp(q);
  CHECK(fognet_write_vec_users(q.c_str(), "run-1", "Net", 2, 4, offset.data(), time.data(), value.data(), nullptr, 1) ==
        FOGNET_OK);
  const std::string after = slurp(q);
  CHECK(after.compare(0, before.size(), before) == 0 && count(after, "version 2") == 1);
  CHECK(after.find("vector 6  Net.user[0].udpApp[0]  latencyH1:vector  TV\n", before.size()) != std::string::npos);
  // no row at all, another id_base, and the broker's delay alone
  const std::vector<int64_t> none(8, 0);
  CHECK(fognet_write_vec_users(p.c_str(), "run-1", "Net", 2, 100, none.data(), nullptr, nullptr, nullptr, 0) == FOGNET_OK);
  const std::string empty = slurp(p);
  CHECK(count(empty, "\nvector 10") == 7 && empty.find("\n100\t") == std::string::npos);
  CHECK(fognet_write_vec_users(p.c_str(), "run-1", "Net", 0, 0, none.data(), nullptr, nullptr, nullptr, 0) == FOGNET_OK);
  CHECK(count(slurp(p), "\nvector ") == 1);
  // error paths
  CHECK(fognet_write_vec_users(nullptr, "r", "Net", 2, 4, offset.data(), time.data(), value.data(), nullptr, 0) == FOGNET_ERR_ARG);
  CHECK(fognet_write_vec_users(p.c_str(), "r", "Net", -1, 4, offset.data(), time.data(), value.data(), nullptr, 0) == FOGNET_ERR_ARG);
  CHECK(fognet_write_vec_users(p.c_str(), "r", "Net", 2, -1, offset.data(), time.data(), value.data(), nullptr, 0) == FOGNET_ERR_ARG);
  CHECK(fognet_write_vec_users(p.c_str(), "r", "Net", 2, 4, nullptr, time.data(), value.data(), nullptr, 0) == FOGNET_ERR_ARG);
  CHECK(fognet_write_vec_users(p.c_str(), "r", "Net", 2, 4, offset.data(), nullptr, value.data(), nullptr, 0) == FOGNET_ERR_ARG);
  std::vector<int64_t> bad = offset;
  bad[3] = 2;
  CHECK(fognet_write_vec_users(p.c_str(), "r", "Net", 2, 4, bad.data(), time.data(), value.data(), nullptr, 0) == FOGNET_ERR_ARG);
  const char* hole[2] = {"a", nullptr};
  CHECK(fognet_write_vec_users(p.c_str(), "r", "Net", 2, 4, offset.data(), time.data(), value.data(), hole, 0) == FOGNET_ERR_ARG);
  CHECK(fognet_write_vec_users((dir + "/no/such/dir.vec").c_str(), "r", "Net", 2, 4, offset.data(), time.data(), value.data(),
                               nullptr, 0) == FOGNET_ERR_ARG);
  CHECK(std::string(fognet_io_last_error()).find("cannot open") != std::string::npos);
  if (failures) {
    fprintf(stderr, "io_vec_users_check: %d failure(s)\n", failures);
    return 1;
  }
  printf("io_vec_users_check: ok\n");
  return 0;
}
