// The pending-gemm_outer record of the HIP library (iterative-solver_amd/csrc/pending_outer.h) on its
// own, on the CPU: the header is free of HIP, and the launch the record asks for goes through the
// callable the caller passes, which here only copies the record.  Addresses are offsets into one host
// array, never dereferenced.
#include <cstdio>
#include <vector>

#include "pending_outer.h"

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

using ssp::PendingOuter;
using Launched = std::vector<PendingOuter::Record>;
struct Recorder {
  Launched* out;
  void operator()(const PendingOuter::Record& r) { out->push_back(r); }
};

constexpr size_t N = 1000;       // elements per vector
double base[200 * N];            // the "device memory": only its addresses are used
double* vec(int i) { return base + size_t(i) * N; }

// k sources (vectors 0 .. k-1), m destinations (vectors 100 .. 100+m-1), alpha(i, j) = 100 i + j
struct Panel {
  std::vector<double> alpha;
  std::vector<const double*> x;
  std::vector<double*> y;
  Panel(int k, int m) {
    for (int i = 0; i < k; ++i) x.push_back(vec(i));
    for (int j = 0; j < m; ++j) y.push_back(vec(100 + j));
    for (int i = 0; i < k; ++i)
      for (int j = 0; j < m; ++j) alpha.push_back(100.0 * i + j);
  }
  bool record(PendingOuter& p, bool set = false, size_t n = N) {
    return p.record(alpha.data(), x.data(), int(x.size()), y.data(), int(y.size()), n, set);
  }
};
}  // namespace

int main() {
  run("record_attach_flush", [] {
    PendingOuter p;
    Launched l;
    p.flush(Recorder{&l});
    CHECK(!p.pending() && l.empty());                  // nothing to launch
    CHECK(!p.attach(2.0, vec(50), vec(100), N));       // nothing to attach to
    Panel a(5, 3);
    CHECK(a.record(p) && p.pending());
    CHECK(p.record().terms() == 0);
    CHECK(p.attach(-2.5, vec(50), vec(101), N));       // destination 1
    CHECK(p.attach(-0.0, vec(51), vec(100), N));       // destination 0: the coefficient is kept as given
    CHECK(p.pending() && l.empty() && p.record().terms() == 2);
    p.flush(Recorder{&l});
    CHECK(!p.pending() && l.size() == 1);
    const PendingOuter::Record& r = l[0];
    CHECK(r.k == 5 && r.m == 3 && r.n == N && !r.set && r.mask == 3u && r.terms() == 2);
    for (int i = 0; i < 5; ++i) CHECK(r.x[i] == vec(i));
    for (int j = 0; j < 3; ++j) CHECK(r.y[j] == vec(100 + j));
    for (int i = 0; i < 5; ++i)
      for (int j = 0; j < 3; ++j) CHECK(r.alpha[i * 3 + j] == 100.0 * i + j);
    CHECK(r.ea[1] == -2.5 && r.ex[1] == vec(50));
    CHECK(r.ea[0] == 0.0 && __builtin_signbit(r.ea[0]) && r.ex[0] == vec(51));
    p.flush(Recorder{&l});
    CHECK(l.size() == 1);                              // launched once
    CHECK(!p.attach(1.0, vec(50), vec(102), N));       // the record is gone
  });

  run("flush_without_terms_and_set_flag", [] {
    PendingOuter p;
    Launched l;
    Panel a(48, 8);
    CHECK(a.record(p, true));
    p.flush(Recorder{&l});
    CHECK(l.size() == 1 && l[0].set && l[0].mask == 0u && l[0].terms() == 0 && l[0].k == 48 && l[0].m == 8);
  });

  run("second_term_on_one_destination", [] {
    PendingOuter p;
    Panel a(4, 2);
    CHECK(a.record(p));
    CHECK(p.attach(1.0, vec(50), vec(100), N));
    CHECK(!p.attach(2.0, vec(51), vec(100), N));       // destination 0 has its term
    CHECK(p.pending() && p.record().terms() == 1 && p.record().ea[0] == 1.0 && p.record().ex[0] == vec(50));
    CHECK(p.attach(2.0, vec(51), vec(101), N));        // destination 1 is still free
  });

  run("x_that_is_a_destination", [] {
    PendingOuter p;
    Panel a(4, 3);
    CHECK(a.record(p));
    CHECK(!p.attach(1.0, vec(101), vec(100), N));      // another destination
    CHECK(!p.attach(1.0, vec(100), vec(100), N));      // the destination itself
    CHECK(!p.attach(1.0, vec(102) - 2, vec(100), N));  // shares two elements with destination 2
    CHECK(!p.attach(1.0, vec(99) + 2, vec(101), N));   // runs two elements into destination 0
    CHECK(p.attach(1.0, vec(99), vec(101), N));        // ends where destination 0 starts
    CHECK(p.attach(1.0, vec(103), vec(100), N));       // starts where destination 2 ends
    CHECK(p.record().terms() == 2);
  });

  run("x_that_is_a_source", [] {
    PendingOuter p;
    Launched l;
    Panel a(4, 2);
    CHECK(a.record(p));
    CHECK(p.attach(3.0, vec(2), vec(101), N));
    p.flush(Recorder{&l});
    CHECK(l.size() == 1 && l[0].mask == 2u && l[0].ex[1] == vec(2) && l[0].x[2] == vec(2));
  });

  run("mismatched_n_or_pointer", [] {
    PendingOuter p;
    Panel a(4, 2);
    CHECK(a.record(p));
    CHECK(!p.attach(1.0, vec(50), vec(100), N - 1));   // shorter
    CHECK(!p.attach(1.0, vec(50), vec(100), N + 1));   // longer
    CHECK(!p.attach(1.0, vec(50), vec(100) + 2, N));   // an offset view of a destination
    CHECK(!p.attach(1.0, vec(50), vec(100) + 2, N - 2));
    CHECK(!p.attach(1.0, vec(50), vec(60), N));        // no destination at all
    CHECK(!p.attach(1.0, vec(50), vec(1), N));         // a source
    CHECK(p.pending() && p.record().terms() == 0);     // the record is unchanged
    CHECK(p.attach(1.0, vec(50), vec(100), N));
  });

  run("fit_limit_on_both_sides", [] {
    {  // k + m == kSrc: the m epilogue sources fit behind the k sources
      PendingOuter p;
      Panel a(PendingOuter::kSrc - 8, 8);
      CHECK(PendingOuter::epilogue_fits(PendingOuter::kSrc - 8, 8));
      CHECK(a.record(p) && p.attach(1.0, vec(80), vec(100), N));
    }
    {  // one more source: recorded, launched without terms
      PendingOuter p;
      Launched l;
      Panel a(PendingOuter::kSrc - 7, 8);
      CHECK(!PendingOuter::epilogue_fits(PendingOuter::kSrc - 7, 8));
      CHECK(a.record(p) && !p.attach(1.0, vec(80), vec(100), N));
      p.flush(Recorder{&l});
      CHECK(l.size() == 1 && l[0].terms() == 0);
    }
    {  // the largest single launch is recorded; more sources or destinations are not
      PendingOuter p;
      Panel a(PendingOuter::kSrc, PendingOuter::kDst);
      CHECK(a.record(p) && !p.attach(1.0, vec(80), vec(100), N));
      PendingOuter q;
      CHECK(!Panel(PendingOuter::kSrc + 1, 1).record(q) && !q.pending());
      CHECK(!Panel(1, PendingOuter::kDst + 1).record(q) && !q.pending());
      CHECK(Panel(PendingOuter::kSrc - PendingOuter::kDst, PendingOuter::kDst).record(q));
      CHECK(q.attach(1.0, vec(80), vec(100 + PendingOuter::kDst - 1), N));
      CHECK(q.record().mask == 1u << (PendingOuter::kDst - 1));
    }
  });

  run("not_recorded", [] {
    PendingOuter p;
    Panel a(4, 2);
    CHECK(!a.record(p, false, 0) && !p.pending());     // n == 0
    CHECK(a.record(p));
    Panel b(3, 1);
    CHECK(!b.record(p));                               // one record at a time: the caller flushes first
    CHECK(p.record().k == 4 && p.record().m == 2);
    PendingOuter q;
    Panel c(4, 2);
    c.y[1] = c.y[0];                                   // a repeated destination
    CHECK(!c.record(q) && !q.pending());
    c.y[1] = c.y[0] + N - 2;                           // destinations that share two elements
    CHECK(!c.record(q) && !q.pending());
    c.y[1] = c.y[0] + N;                               // adjacent
    CHECK(c.record(q));
  });

  run("discard", [] {
    PendingOuter p;
    Launched l;
    Panel a(4, 2);
    CHECK(a.record(p) && p.attach(1.0, vec(50), vec(100), N));
    p.discard();
    CHECK(!p.pending());
    p.flush(Recorder{&l});
    CHECK(l.empty());                                  // never launched
    CHECK(!p.attach(1.0, vec(50), vec(101), N));
    CHECK(a.record(p) && p.record().terms() == 0);     // a new record starts without the old terms
  });

  run("flush_clears_before_launch", [] {
    PendingOuter p;
    Panel a(4, 2), b(3, 1);
    CHECK(a.record(p));
    bool seen = false;
    p.flush([&](const PendingOuter::Record& r) {
      seen = !p.pending() && r.k == 4;                 // a launch that re-enters finds nothing pending
    });
    CHECK(seen && !p.pending());
    CHECK(b.record(p));
  });

  std::printf("%s %d failure(s)\n", failures ? "FAILED" : "OK", failures);
  return failures ? 1 : 0;
}
