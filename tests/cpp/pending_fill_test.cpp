// The pending-zero-fill table of the HIP library (iterative-solver_amd/csrc/pending_fill.h) on its own,
// on the CPU: the header is free of HIP, and every store the table asks for goes through the callable
// the caller passes, which here only records (address, length).  Addresses are offsets into one
// host array, never dereferenced.
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "pending_fill.h"

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

using Flushed = std::vector<std::pair<const double*, size_t>>;
struct Recorder {
  Flushed* out;
  void operator()(double* p, size_t n) { out->emplace_back(p, n); }
};

double base[1 << 16];  // the "device memory": only its addresses are used
double* at(size_t i) { return base + i; }
}  // namespace

int main() {
  using ssp::PendingFills;

  run("exact_match", [] {
    PendingFills t;
    Flushed f;
    CHECK(t.empty() && t.find_exact(at(0), 100) == -1);
    t.insert(at(0), 100, Recorder{&f});
    t.insert(at(100), 50, Recorder{&f});  // adjacent, not overlapping
    CHECK(t.size() == 2 && f.empty());
    CHECK(t.find_exact(at(0), 100) == 0);
    CHECK(t.find_exact(at(100), 50) == 1);
    CHECK(t.find_exact(at(0), 99) == -1);   // same start, shorter
    CHECK(t.find_exact(at(1), 100) == -1);  // same length, shifted
    CHECK(t.find_exact(at(0), 150) == -1);  // spans both
    t.erase(0);
    CHECK(t.size() == 1 && t.find_exact(at(0), 100) == -1 && t.find_exact(at(100), 50) == 0);
  });

  run("overlap_queries", [] {
    PendingFills t;
    Flushed f;
    t.insert(at(100), 100, Recorder{&f});  // [100, 200)
    CHECK(t.find_overlap(at(0), 100) == -1);    // ends where the entry starts
    CHECK(t.find_overlap(at(200), 10) == -1);   // starts where it ends
    CHECK(t.find_overlap(at(0), 101) == 0);     // one element from the left
    CHECK(t.find_overlap(at(199), 10) == 0);    // one element from the right
    CHECK(t.find_overlap(at(150), 1) == 0);     // inside
    CHECK(t.find_overlap(at(0), 1000) == 0);    // covers
    CHECK(t.find_overlap(at(150), 0) == -1);    // an empty range touches nothing
    CHECK(t.find_overlap(at(0), 1000, 1) == -1);
  });

  run("partial_overlap_left_and_right_is_flushed", [] {
    PendingFills t;
    Flushed f;
    t.insert(at(100), 100, Recorder{&f});
    t.insert(at(300), 100, Recorder{&f});
    t.insert(at(500), 100, Recorder{&f});
    // a reader of [50, 150) and one of [350, 450): the first two entries are stored, the third stays
    t.flush_overlap(at(50), 100, Recorder{&f});
    CHECK(f.size() == 1 && f[0].first == at(100) && f[0].second == 100);
    t.flush_overlap(at(350), 100, Recorder{&f});
    CHECK(f.size() == 2 && f[1].first == at(300) && f[1].second == 100);
    CHECK(t.size() == 1 && t.find_exact(at(500), 100) == 0);
    // a new zero fill partly over a pending one, from either side: the old one is stored first
    f.clear();
    t.insert(at(450), 100, Recorder{&f});  // [450, 550) over [500, 600)
    CHECK(f.size() == 1 && f[0].first == at(500));
    CHECK(t.size() == 1 && t.find_exact(at(450), 100) == 0);
    t.insert(at(400), 100, Recorder{&f});  // [400, 500) over [450, 550)
    CHECK(f.size() == 2 && f[1].first == at(450));
    CHECK(t.size() == 1 && t.find_exact(at(400), 100) == 0);
    // a view inside a pending range is a partial overlap too (the entry is not inside the view)
    f.clear();
    t.overwrite(at(410), 10, Recorder{&f});
    CHECK(f.size() == 1 && f[0].first == at(400) && f[0].second == 100 && t.empty());
  });

  run("full_cover_is_dropped", [] {
    PendingFills t;
    Flushed f;
    t.insert(at(100), 50, Recorder{&f});
    t.insert(at(200), 50, Recorder{&f});
    t.insert(at(1000), 50, Recorder{&f});
    // a write-only op over [100, 250): both entries inside it vanish without a store
    t.overwrite(at(100), 150, Recorder{&f});
    CHECK(f.empty() && t.size() == 1 && t.find_exact(at(1000), 50) == 0);
    // exactly the same range: dropped; then a fill of the same range again: one entry, no store
    t.insert(at(1000), 50, Recorder{&f});
    CHECK(f.empty() && t.size() == 1);
    // a larger zero fill swallows the smaller pending one
    t.insert(at(990), 100, Recorder{&f});
    CHECK(f.empty() && t.size() == 1 && t.find_exact(at(990), 100) == 0);
    // covering one entry and cutting another: the first dropped, the second stored
    t.insert(at(2000), 100, Recorder{&f});
    t.overwrite(at(980), 1060, Recorder{&f});  // [980, 2040)
    CHECK(f.size() == 1 && f[0].first == at(2000) && t.empty());
  });

  run("erase_inside_freed_block", [] {
    PendingFills t;
    Flushed f;
    // a 256-B-granular block of 64 doubles at 4096 holding a vector of 40 and, elsewhere, two others
    t.insert(at(4096), 40, Recorder{&f});
    t.insert(at(8192), 40, Recorder{&f});
    t.insert(at(4096 + 48), 8, Recorder{&f});  // a view further into the same block
    t.overwrite_bytes(at(4096), 64 * sizeof(double), Recorder{&f});
    CHECK(f.empty());  // nothing may be written into a block that is being freed
    CHECK(t.size() == 1 && t.find_exact(at(8192), 40) == 0);
    CHECK(t.find_overlap(at(4096), 64) == -1);
    // freeing a block with nothing pending in it changes nothing
    t.overwrite_bytes(at(0), 64 * sizeof(double), Recorder{&f});
    CHECK(f.empty() && t.size() == 1);
  });

  run("overflow_at_65_inserts", [] {
    PendingFills t;
    Flushed f;
    CHECK(PendingFills::kCapacity == 64);
    for (int i = 0; i < 64; ++i) t.insert(at(size_t(i) * 16), 10, Recorder{&f});
    CHECK(t.size() == 64 && f.empty());
    t.insert(at(64 * 16), 10, Recorder{&f});  // the 65th: the 64 before it are stored, oldest first
    CHECK(f.size() == 64 && t.size() == 1 && t.find_exact(at(64 * 16), 10) == 0);
    for (int i = 0; i < 64 && i < int(f.size()); ++i) CHECK(f[size_t(i)].first == at(size_t(i) * 16) && f[size_t(i)].second == 10);
    // a 65th that covers a pending entry frees its slot instead of draining the table
    PendingFills u;
    f.clear();
    for (int i = 0; i < 64; ++i) u.insert(at(size_t(i) * 16), 10, Recorder{&f});
    u.insert(at(0), 12, Recorder{&f});
    CHECK(f.empty() && u.size() == 64 && u.find_exact(at(0), 12) == 63 && u.find_exact(at(16), 10) == 0);
  });

  run("drain_order", [] {
    PendingFills t;
    Flushed f;
    const size_t where[] = {700, 100, 900, 300, 500};
    for (size_t w : where) t.insert(at(w), 7, Recorder{&f});
    t.erase(t.find_exact(at(900), 7));  // the others keep their order
    t.insert(at(200), 7, Recorder{&f});
    t.drain(Recorder{&f});
    const size_t want[] = {700, 100, 300, 500, 200};
    CHECK(f.size() == 5 && t.empty());
    for (size_t i = 0; i < 5 && i < f.size(); ++i) CHECK(f[i].first == at(want[i]) && f[i].second == 7);
    t.drain(Recorder{&f});  // an empty table stores nothing
    CHECK(f.size() == 5);
    t.insert(at(0), 1, Recorder{&f});
    t.clear();
    CHECK(t.empty() && f.size() == 5);
  });

  run("entries_stay_disjoint", [] {
    // the invariant the consuming gemm_outer relies on: distinct exact matches are disjoint ranges
    PendingFills t;
    Flushed f;
    unsigned s = 12345;
    for (int it = 0; it < 2000; ++it) {
      s = s * 1664525u + 1013904223u;
      const size_t p = (s >> 8) % 4000, n = 1 + (s >> 20) % 300;
      switch (it % 4) {
        case 0:
        case 1: t.insert(at(p), n, Recorder{&f}); break;
        case 2: t.flush_overlap(at(p), n, Recorder{&f}); break;
        default: t.overwrite(at(p), n, Recorder{&f}); break;
      }
      for (int i = 0; i < t.size(); ++i) CHECK(t.find_overlap(reinterpret_cast<const void*>(t.at(i).p), t.at(i).n, i + 1) == -1);
      if (it % 4 >= 2) CHECK(t.find_overlap(at(p), n) == -1);
      if (!case_ok) break;
    }
  });

  std::printf("%s %d failure(s)\n", failures ? "FAILED" : "OK", failures);
  return failures ? 1 : 0;
}
