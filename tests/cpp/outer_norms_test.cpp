// The kept norms of a launched gemm_outer record (iterative-solver_amd/csrc/outer_norms.h) on their own,
// on the CPU: the header is free of HIP.  Addresses are offsets into one host array, never dereferenced.
#include <cstdio>
#include <vector>

#include "outer_norms.h"

namespace {
int failures = 0;
bool case_ok = true;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      case_ok = false;                                                     \
    }                                                                      \
  } while (0)

template <typename F>
void run(const char* name, F&& f) {
  case_ok = true;
  f();
  std::printf("%s %s\n", case_ok ? "PASS" : "FAIL", name);
  if (!case_ok) ++failures;
}

using ssp::OuterNorms;

constexpr size_t N = 1000;  // elements per vector
double base[40 * N];        // the "device memory": only its addresses are used
double* vec(int i) { return base + size_t(i) * N; }

// m destinations (vectors 0 .. m-1) with the values 10 + j
bool keep(OuterNorms& c, int m, size_t n = N) {
  std::vector<double*> y;
  std::vector<double> v;
  for (int j = 0; j < m; ++j) {
    y.push_back(vec(j));
    v.push_back(10.0 + j);
  }
  if (!c.keep(y.data(), m, n)) return false;
  c.set_values(v.data());
  return true;
}
}  // namespace

int main() {
  run("exact_match_only", [] {
    OuterNorms c;
    CHECK(c.empty() && c.find(vec(0), N) == -1);
    CHECK(keep(c, 3));
    CHECK(!c.empty() && c.size() == 3);
    for (int j = 0; j < 3; ++j) {
      CHECK(c.find(vec(j), N) == j);
      CHECK(c.value(j) == 10.0 + j);
    }
    CHECK(c.find(vec(3), N) == -1);      // the next vector: not a destination
    CHECK(c.find(vec(1) + 2, N) == -1);  // an offset view of a destination
    CHECK(c.find(vec(1) + 2, N - 2) == -1);
    CHECK(c.find(vec(1) - 1, N) == -1);
  });
  run("n_mismatch", [] {
    OuterNorms c;
    CHECK(keep(c, 3));
    CHECK(c.find(vec(1), N - 1) == -1);  // the destination with a shorter n
    CHECK(c.find(vec(1), N + 1) == -1);
    CHECK(c.find(vec(1), 0) == -1);
    CHECK(c.find(vec(1), N) == 1);
  });
  run("forget_all", [] {
    OuterNorms c;
    CHECK(keep(c, 8));
    c.forget();
    CHECK(c.empty() && c.size() == 0);
    for (int j = 0; j < 8; ++j) CHECK(c.find(vec(j), N) == -1);
    c.forget();  // twice is fine
    CHECK(c.empty());
    CHECK(c.find(nullptr, 0) == -1);  // an empty cache matches nothing, not even its own initial state
  });
  run("repeated_query", [] {
    OuterNorms c;
    CHECK(keep(c, 2));
    for (int rep = 0; rep < 3; ++rep) {
      CHECK(c.find(vec(1), N) == 1 && c.value(1) == 11.0);
      CHECK(c.find(vec(0), N) == 0 && c.value(0) == 10.0);
    }
  });
  run("sixteen_destinations", [] {
    OuterNorms c;
    CHECK(keep(c, 16));
    CHECK(c.size() == 16);
    for (int j = 0; j < 16; ++j) CHECK(c.find(vec(j), N) == j && c.value(j) == 10.0 + j);
    CHECK(c.find(vec(16), N) == -1);
  });
  run("not_kept", [] {
    OuterNorms c;
    CHECK(keep(c, 3));
    CHECK(!keep(c, 17));  // more than one launch holds: nothing kept, and the earlier ones are gone
    CHECK(c.empty() && c.find(vec(0), N) == -1);
    CHECK(!keep(c, 0) && c.empty());
    CHECK(!keep(c, 2, 0) && c.empty());
  });
  run("keep_replaces", [] {
    OuterNorms c;
    CHECK(keep(c, 8));
    double* y[2] = {vec(20), vec(21)};
    const double v[2] = {1.5, 2.5};
    CHECK(c.keep(y, 2, N / 2));
    CHECK(c.find(vec(20), N / 2) == 0 && c.value(0) == 0.0);  // values follow the launch
    c.set_values(v);
    CHECK(c.find(vec(21), N / 2) == 1 && c.value(1) == 2.5);
    CHECK(c.find(vec(0), N) == -1 && c.find(vec(20), N) == -1);
  });
  std::printf("%s %d failure(s)\n", failures ? "FAILED" : "OK", failures);
  return failures ? 1 : 0;
}
