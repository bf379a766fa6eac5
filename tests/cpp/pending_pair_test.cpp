// The pair of pending gemm_outer records of the HIP library (iterative-solver_amd/csrc/pending_outer.h,
// OuterPair) on its own, on the CPU: the header is free of HIP, and the launches the records ask for go
// through the callables the caller passes, which here only copy the records.  Addresses are offsets into
// one host array, never dereferenced.
#include <cstdio>
#include <cstring>
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

using ssp::OuterPair;
using ssp::PendingOuter;
using Record = PendingOuter::Record;
using Launched = std::vector<Record>;
struct Recorder {
  Launched* out;
  void operator()(const Record& r) { out->push_back(r); }
};
struct PairLaunch {
  Record a, b;
  unsigned mask = 0;
  double e[OuterPair::kDst] = {};
  int count = 0;
  void operator()(const Record& ra, const Record& rb, unsigned m, const double* ev) {
    a = ra;
    b = rb;
    mask = m;
    for (int j = 0; j < OuterPair::kDst; ++j) e[j] = ev[j];
    ++count;
  }
};

constexpr size_t N = 1000;       // elements per vector
double base[400 * N];            // the "device memory": only its addresses are used
double* vec(int i) { return base + size_t(i) * N; }

// k sources (vectors s0 .. s0+k-1), m destinations (vectors d0 .. d0+m-1), alpha(i, j) = 100 i + j
struct Panel {
  std::vector<double> alpha;
  std::vector<const double*> x;
  std::vector<double*> y;
  Panel(int k, int m, int s0, int d0) {
    for (int i = 0; i < k; ++i) x.push_back(vec(s0 + i));
    for (int j = 0; j < m; ++j) y.push_back(vec(d0 + j));
    for (int i = 0; i < k; ++i)
      for (int j = 0; j < m; ++j) alpha.push_back(100.0 * i + j);
  }
  bool record(PendingOuter& p, bool set = false, size_t n = N) {
    return p.record(alpha.data(), x.data(), int(x.size()), y.data(), int(y.size()), n, set);
  }
  bool may(const OuterPair& q, const PendingOuter& p, bool set = false, size_t n = N) const {
    return q.may_pair(p, alpha.data(), x.data(), int(x.size()), y.data(), int(y.size()), n, set);
  }
  bool pair(OuterPair& q, PendingOuter& p, bool set = false, size_t n = N) {
    return q.pair(p, alpha.data(), x.data(), int(x.size()), y.data(), int(y.size()), n, set);
  }
};
// A: sources 0.., destinations 100..; B: sources 200.., destinations 300..
Panel panel_a(int k = 5, int m = 3) { return Panel(k, m, 0, 100); }
Panel panel_b(int k = 5, int m = 3) { return Panel(k, m, 200, 300); }

bool same_record(const Record& r, const Panel& p, bool set, unsigned mask) {
  const int k = int(p.x.size()), m = int(p.y.size());
  if (r.k != k || r.m != m || r.n != N || r.set != set || r.mask != mask) return false;
  for (int i = 0; i < k; ++i)
    if (r.x[i] != p.x[size_t(i)]) return false;
  for (int j = 0; j < m; ++j)
    if (r.y[j] != p.y[size_t(j)]) return false;
  return std::memcmp(r.alpha, p.alpha.data(), sizeof(double) * size_t(k) * size_t(m)) == 0;
}
}  // namespace

int main() {
  run("pair_and_flush", [] {
    PendingOuter p;
    OuterPair q;
    Panel a = panel_a(), b = panel_b();
    CHECK(!b.may(q, p) && !b.pair(q, p) && !q.paired());   // nothing pending: no A
    CHECK(a.record(p));
    CHECK(b.may(q, p) && !q.paired());                     // may_pair changes nothing
    CHECK(b.pair(q, p) && q.paired() && p.pending());
    CHECK(same_record(q.a(), a, false, 0u) && same_record(p.record(), b, false, 0u));
    CHECK(q.attach(p, -2.5, vec(101), vec(301), N));       // A's destination 1 onto B's destination 1
    CHECK(q.attach(p, -0.0, vec(100), vec(300), N));       // the coefficient is kept as given
    CHECK(q.reg_mask() == 3u && q.reg(1) == -2.5 && q.reg(0) == 0.0 && __builtin_signbit(q.reg(0)));
    CHECK(p.record().terms() == 0);                        // register terms are not B's memory terms
    PairLaunch l;
    q.flush(p, l);
    CHECK(l.count == 1 && !q.paired() && !p.pending());
    CHECK(same_record(l.a, a, false, 0u) && same_record(l.b, b, false, 0u));
    CHECK(l.mask == 3u && l.e[1] == -2.5 && l.e[0] == 0.0 && __builtin_signbit(l.e[0]));
    q.flush(p, l);
    CHECK(l.count == 1);                                   // launched once
    CHECK(a.record(p) && b.pair(q, p) && q.reg_mask() == 0u);  // a new pair starts without the old terms
  });

  run("pairing_conditions", [] {
    const auto fresh = [](PendingOuter& p, bool set = false) {
      p.discard();
      Panel a = panel_a();
      return a.record(p, set);
    };
    PendingOuter p;
    OuterPair q;
    CHECK(fresh(p) && panel_b().may(q, p));                // the base case, for every boundary below
    // call kind
    CHECK(!panel_b().may(q, p, true));
    CHECK(fresh(p, true) && panel_b().may(q, p, true) && !panel_b().may(q, p, false));
    // n, k, m
    CHECK(fresh(p));
    CHECK(!panel_b().may(q, p, false, N - 1) && !panel_b().may(q, p, false, N + 1) && !panel_b().may(q, p, false, 0));
    CHECK(!panel_b(4, 3).may(q, p) && !panel_b(6, 3).may(q, p));
    CHECK(!panel_b(5, 2).may(q, p) && !panel_b(5, 4).may(q, p));
    {  // m <= kDst: 8 pairs, 9 does not
      PendingOuter p8, p9;
      Panel a8 = panel_a(5, OuterPair::kDst), a9 = panel_a(5, OuterPair::kDst + 1);
      CHECK(a8.record(p8) && panel_b(5, OuterPair::kDst).may(q, p8));
      CHECK(a9.record(p9) && !panel_b(5, OuterPair::kDst + 1).may(q, p9));
    }
    // alphas: one bit, and the sign of a zero
    {
      Panel b = panel_b();
      unsigned long long bits;
      std::memcpy(&bits, &b.alpha[7], 8);
      bits ^= 1ull;
      std::memcpy(&b.alpha[7], &bits, 8);
      CHECK(!b.may(q, p));
      Panel c = panel_b();
      c.alpha[0] = -0.0;                                   // alpha(0, 0) is +0.0 in A
      CHECK(!c.may(q, p));
    }
    // a source of B against a destination of A
    {
      Panel b = panel_b();
      b.x[2] = vec(101);
      CHECK(!b.may(q, p));
      b.x[2] = vec(100) - 2;                               // runs two elements into destination 0
      CHECK(!b.may(q, p));
      b.x[2] = vec(99);                                    // ends where destination 0 starts
      CHECK(b.may(q, p));
      b.x[2] = vec(3);                                     // a source of A: both only read it
      CHECK(b.may(q, p));
    }
    // a destination of B against a source or a destination of A
    {
      Panel b = panel_b();
      b.y[1] = vec(2);
      CHECK(!b.may(q, p));
      b.y[1] = vec(4) + N - 2;                             // shares two elements with A's last source
      CHECK(!b.may(q, p));
      b.y[1] = vec(5);                                     // starts where A's last source ends
      CHECK(b.may(q, p));
      b.y[1] = vec(102);
      CHECK(!b.may(q, p));
      b.y[1] = vec(103) - 2;
      CHECK(!b.may(q, p));
      b.y[1] = vec(103);                                   // starts where A's last destination ends
      CHECK(b.may(q, p));
    }
    // B qualifies as a record by itself
    {
      Panel b = panel_b();
      b.y[1] = b.y[0] + 2;                                 // two destinations of B share bytes
      CHECK(!b.may(q, p) && !b.pair(q, p) && !q.paired() && p.pending());
    }
    // a destination of A with a term: not paired, and A is untouched
    CHECK(p.attach(1.0, vec(50), vec(100), N));
    CHECK(!panel_b().may(q, p) && !panel_b().pair(q, p) && !q.paired());
    CHECK(p.pending() && p.record().terms() == 1);
    // a pair is full
    CHECK(fresh(p) && panel_b().pair(q, p));
    CHECK(!Panel(5, 3, 210, 310).may(q, p) && !Panel(5, 3, 210, 310).pair(q, p));
    CHECK(same_record(q.a(), panel_a(), false, 0u) && same_record(p.record(), panel_b(), false, 0u));
  });

  run("register_term_or_not", [] {
    PendingOuter p;
    OuterPair q;
    Panel a = panel_a(), b = panel_b();
    CHECK(!q.attach(p, 1.0, vec(100), vec(300), N));       // no pair
    CHECK(a.record(p));
    CHECK(!q.attach(p, 1.0, vec(100), vec(300), N));       // a single record
    CHECK(b.pair(q, p));
    CHECK(!q.attach(p, 1.0, vec(50), vec(300), N));        // a foreign x
    CHECK(!q.attach(p, 1.0, vec(101), vec(300), N));       // A's destination 1 onto B's destination 0
    CHECK(!q.attach(p, 1.0, vec(200), vec(300), N));       // a source of B
    CHECK(!q.attach(p, 1.0, vec(100), vec(100), N));       // y is a destination of A
    CHECK(!q.attach(p, 1.0, vec(100), vec(300), N - 1));   // another length
    CHECK(!q.attach(p, 1.0, vec(100) + 2, vec(300) + 2, N));  // views
    CHECK(q.reg_mask() == 0u && q.paired());               // nothing changed
    CHECK(q.attach(p, 1.0, vec(100), vec(300), N));
    CHECK(!q.attach(p, 2.0, vec(100), vec(300), N));       // a second term on the same j
    CHECK(q.reg_mask() == 1u && q.reg(0) == 1.0);
    CHECK(q.attach(p, 3.0, vec(102), vec(302), N));
    {  // the term must be able to become B's epilogue term: k + m <= kSrc
      PendingOuter p2;
      OuterPair q2;
      Panel a2(PendingOuter::kSrc - 2, 3, 0, 100), b2(PendingOuter::kSrc - 2, 3, 200, 300);
      CHECK(a2.record(p2) && b2.pair(q2, p2));
      CHECK(!q2.attach(p2, 1.0, vec(100), vec(300), N));
      PendingOuter p3;
      OuterPair q3;
      Panel a3(PendingOuter::kSrc - 3, 3, 0, 100), b3(PendingOuter::kSrc - 3, 3, 200, 300);
      CHECK(a3.record(p3) && b3.pair(q3, p3));
      CHECK(q3.attach(p3, 1.0, vec(100), vec(300), N));
    }
  });

  run("unpair_is_the_single_record_state", [] {
    // the pair, broken ...
    PendingOuter p;
    OuterPair q;
    Launched l;
    Panel a = panel_a(), b = panel_b();
    CHECK(a.record(p) && b.pair(q, p));
    CHECK(q.attach(p, -2.5, vec(101), vec(301), N) && q.attach(p, 4.0, vec(102), vec(302), N));
    bool seen = false;
    q.unpair(p, [&](const Record& r) {
      seen = !q.paired() && p.pending();                   // a launch that re-enters finds B pending alone
      l.push_back(r);
    });
    CHECK(seen && !q.paired() && p.pending() && l.size() == 1 && same_record(l[0], a, false, 0u));
    // ... against the state the calls leave without pairing: A launched, B recorded, the axpys attached
    PendingOuter s;
    Panel b2 = panel_b();
    CHECK(b2.record(s) && s.attach(-2.5, vec(101), vec(301), N) && s.attach(4.0, vec(102), vec(302), N));
    const Record &x = p.record(), &y = s.record();
    CHECK(same_record(x, b, false, 6u) && same_record(y, b, false, 6u));
    for (int j = 1; j < 3; ++j) CHECK(x.ea[j] == y.ea[j] && x.ex[j] == y.ex[j]);
    CHECK(x.terms() == 2);
    // B goes on as a single record: another term, no register term, a flush
    CHECK(p.attach(1.0, vec(50), vec(300), N) && !q.attach(p, 1.0, vec(100), vec(300), N));
    p.flush(Recorder{&l});
    CHECK(l.size() == 2 && l[1].mask == 7u && !p.pending());
    q.unpair(p, Recorder{&l});
    CHECK(l.size() == 2);                                  // nothing to break
  });

  run("unpair_without_terms", [] {
    PendingOuter p;
    OuterPair q;
    Launched l;
    Panel a = panel_a(3, 2), b = panel_b(3, 2);
    CHECK(a.record(p, true) && b.pair(q, p, true));
    q.unpair(p, Recorder{&l});
    CHECK(l.size() == 1 && same_record(l[0], a, true, 0u) && same_record(p.record(), b, true, 0u));
  });

  run("touches", [] {
    PendingOuter p;
    OuterPair q;
    Panel a = panel_a(), b = panel_b();
    CHECK(!q.touches(p, vec(100), N));                     // nothing pending
    CHECK(a.record(p));
    CHECK(q.touches(p, vec(100), N) && q.touches(p, vec(2), N) && !q.touches(p, vec(300), N));
    CHECK(p.attach(1.0, vec(50), vec(100), N));
    CHECK(q.touches(p, vec(50), N));                       // an epilogue source
    CHECK(q.touches(p, vec(49), N + 1) && !q.touches(p, vec(49), N) && q.touches(p, vec(51) - 1, 1));
    CHECK(!q.touches(p, vec(51), 3 * N));
    p.discard();
    CHECK(a.record(p) && b.pair(q, p));
    CHECK(q.touches(p, vec(100), N) && q.touches(p, vec(4), N));      // A's
    CHECK(q.touches(p, vec(302), N) && q.touches(p, vec(200), N));    // B's
    CHECK(!q.touches(p, vec(150), N) && !q.touches(p, vec(5), 95 * N) && q.touches(p, vec(5), 95 * N + 1));
  });

  run("discard", [] {
    PendingOuter p;
    OuterPair q;
    Launched l;
    PairLaunch pl;
    Panel a = panel_a(), b = panel_b();
    CHECK(a.record(p) && b.pair(q, p) && q.attach(p, 1.0, vec(100), vec(300), N));
    q.discard();
    p.discard();
    CHECK(!q.paired() && !p.pending() && q.reg_mask() == 0u);
    q.flush(p, pl);
    q.unpair(p, Recorder{&l});
    CHECK(pl.count == 0 && l.empty());                     // never launched
    CHECK(a.record(p) && b.pair(q, p) && q.reg_mask() == 0u);
  });

  std::printf("%s %d failure(s)\n", failures ? "FAILED" : "OK", failures);
  return failures ? 1 : 0;
}
