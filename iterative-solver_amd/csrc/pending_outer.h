// The pending gemm_outer of a context: a write-only ssp_gemm_outer (ssp_gemm_outer_set, or the
// read-modify-write form that consumed the pending zero fills of all its destinations) of one launch
// is validated and recorded here instead of launched.  An ssp_axpy whose destination is exactly one
// of the record's destinations is attached to it as an epilogue term (a_j, x_j): when the record is
// launched ("flushed"), the kernel adds a_j x_j to the finished sum of destination j before it stores
// it, the fma the separate axpy would have done on the stored and reloaded value.  Every other entry
// point flushes the record first.  DESIGN.md "Deferred gemm_outer".
//
// Host-only and free of HIP: the record knows addresses, lengths and coefficients, and the launch goes
// through the `launch(record)` callable its caller passes (tests/cpp/pending_outer_test.cpp drives it
// on the CPU).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace ssp {

class PendingOuter {
 public:
  static constexpr int kSrc = 64;  // ssp::kOuterSrc: sources of one launch
  static constexpr int kDst = 16;  // ssp::kOuterDst: destinations of one launch

  struct Record {
    double alpha[kSrc * kDst];  // alpha[i * m + j]
    const double* x[kSrc];
    double* y[kDst];
    int k = 0;
    int m = 0;
    size_t n = 0;
    bool set = false;  // the call was ssp_gemm_outer_set (else ssp_gemm_outer over consumed fills)
    // epilogue: y[j] += ea[j] * ex[j] for the destinations whose bit of `mask` is set
    double ea[kDst];
    const double* ex[kDst];
    unsigned mask = 0;

    int terms() const {
      int e = 0;
      for (int j = 0; j < m; ++j) e += (mask >> j) & 1u;
      return e;
    }
  };

  bool pending() const { return pending_; }
  const Record& record() const { return r_; }

  // One launch holds the record's sources and destinations.
  static bool one_launch(int k, int m) { return k >= 1 && m >= 1 && k <= kSrc && m <= kDst; }
  // The launch carries the epilogue sources in its unused source slots [k, k + m).
  static bool epilogue_fits(int k, int m) { return k + m <= kSrc; }

  // Records yy[j] = sum_i alphas[i * m + j] xx[i] over n > 0 elements.  False (nothing recorded) when the
  // shape is not one launch or two destinations share a byte: the caller launches as it always did.
  // Nothing may be pending.
  bool record(const double* alphas, const double* const* xx, int k, double* const* yy, int m, size_t n, bool set) {
    if (pending_ || n == 0 || !one_launch(k, m)) return false;
    for (int j = 0; j < m; ++j)
      for (int i = 0; i < j; ++i)
        if (overlap(yy[i], yy[j], n)) return false;
    for (int i = 0; i < k * m; ++i) r_.alpha[i] = alphas[i];
    for (int i = 0; i < k; ++i) r_.x[i] = xx[i];
    for (int j = 0; j < m; ++j) r_.y[j] = yy[j];
    r_.k = k;
    r_.m = m;
    r_.n = n;
    r_.set = set;
    r_.mask = 0;
    pending_ = true;
    return true;
  }

  // y[0, n) += alpha * x[0, n) with unscaled operands.  True: the term now rides on the record and the
  // caller launches nothing.  False: the record is unchanged, and the caller flushes it and runs the axpy.
  bool attach(double alpha, const double* x, const double* y, size_t n) {
    if (!pending_ || n != r_.n || !epilogue_fits(r_.k, r_.m)) return false;
    int j = 0;
    while (j < r_.m && r_.y[j] != y) ++j;
    if (j == r_.m || ((r_.mask >> j) & 1u)) return false;
    // x is read in the state the launch finds it in: it may be a source, never a destination
    for (int d = 0; d < r_.m; ++d)
      if (overlap(x, r_.y[d], n)) return false;
    r_.ea[j] = alpha;
    r_.ex[j] = x;
    r_.mask |= 1u << j;
    return true;
  }

  // Launches the record, if there is one.
  template <typename F>
  void flush(F&& launch) {
    if (!pending_) return;
    pending_ = false;  // first: `launch` may re-enter the library
    launch(static_cast<const Record&>(r_));
  }

  // Forgets the record without launching it (the context is being destroyed).
  void discard() { pending_ = false; }

  // Moves the record out, unlaunched: it becomes the older record of a pair (OuterPair).  Something must be pending.
  void take(Record* out) {
    *out = r_;
    pending_ = false;
  }

  // [a, a + 8 n) and [b, b + 8 n) share a byte.
  static bool overlap(const void* a, const void* b, size_t n) {
    const uintptr_t p = reinterpret_cast<uintptr_t>(a), q = reinterpret_cast<uintptr_t>(b);
    const size_t bytes = n * sizeof(double);
    return p < q + bytes && q < p + bytes;
  }

 private:
  Record r_;
  bool pending_ = false;
};

// Two pending gemm_outers: the older record A here, the newer record B in the PendingOuter every method
// takes (the context's one pending record, which is B for as long as the pair stands).  The pair is what
// the two solution constructions of a step leave behind -- the same alphas applied to two spaces of
// sources -- and one launch forms both (k_gemm_outer_pair).  An ssp_axpy of A's destination j onto B's
// destination j becomes a register term: the launch adds reg(j) * (the sum of A's destination j, as
// stored) to the sum of B's destination j before it stores that.
//
// Invariant: whatever does not fit the pattern un-pairs first.  unpair() launches A alone, as the single
// record it was, and turns every register term into the ordinary epilogue term of B it would have been
// had A been launched before B was recorded (its source, A's destination, is then in memory).  What is
// left is exactly the single-record state of B, so nothing outside the pattern sees a new state, and A
// always launches before B.
class OuterPair {
 public:
  using Record = PendingOuter::Record;
  static constexpr int kDst = 8;  // destinations of one space in the pair's launch

  bool paired() const { return paired_; }
  const Record& a() const { return a_; }
  unsigned reg_mask() const { return mask_; }
  double reg(int j) const { return e_[j]; }

  // The call yy[j] = sum_i alphas[i * m + j] xx[i] may become B next to the single record A of `single`:
  // it qualifies as a record by itself; same call kind, n, k and m <= kDst; the k m alphas bit for bit
  // equal; no source of B shares a byte with a destination of A; no destination of B shares a byte with
  // a source or a destination of A; A carries no term.
  bool may_pair(const PendingOuter& single, const double* alphas, const double* const* xx, int k, double* const* yy,
                int m, size_t n, bool set) const {
    if (paired_ || !single.pending() || n == 0 || !PendingOuter::one_launch(k, m)) return false;
    const Record& a = single.record();
    if (a.set != set || a.n != n || a.k != k || a.m != m || m > kDst || a.mask != 0) return false;
    if (std::memcmp(a.alpha, alphas, sizeof(double) * size_t(k) * size_t(m)) != 0) return false;
    for (int j = 0; j < m; ++j) {
      for (int i = 0; i < j; ++i)
        if (PendingOuter::overlap(yy[i], yy[j], n)) return false;
      for (int i = 0; i < k; ++i)
        if (PendingOuter::overlap(xx[i], a.y[j], n) || PendingOuter::overlap(yy[j], a.x[i], n)) return false;
      for (int d = 0; d < m; ++d)
        if (PendingOuter::overlap(yy[j], a.y[d], n)) return false;
    }
    return true;
  }

  // Makes the pair: A moves here and the call is recorded in `single` as B.  False: nothing changed.
  bool pair(PendingOuter& single, const double* alphas, const double* const* xx, int k, double* const* yy, int m,
            size_t n, bool set) {
    if (!may_pair(single, alphas, xx, k, yy, m, n, set)) return false;
    single.take(&a_);
    single.record(alphas, xx, k, yy, m, n, set);  // may_pair has checked what record() checks
    mask_ = 0;
    paired_ = true;
    return true;
  }

  // y[0, n) += alpha * x[0, n) with unscaled operands.  True: x is exactly A's destination j, y exactly
  // B's destination j, which had no term, and the term now rides on the pair.  False: nothing changed,
  // and the caller un-pairs.  (The term must be able to become B's epilogue term when the pair breaks.)
  bool attach(const PendingOuter& b, double alpha, const double* x, const double* y, size_t n) {
    if (!paired_ || n != a_.n || !PendingOuter::epilogue_fits(a_.k, a_.m)) return false;
    const Record& rb = b.record();
    int j = 0;
    while (j < a_.m && rb.y[j] != y) ++j;
    if (j == a_.m || a_.y[j] != x || ((mask_ >> j) & 1u) || ((rb.mask >> j) & 1u)) return false;
    e_[j] = alpha;
    mask_ |= 1u << j;
    return true;
  }

  // [p, p + 8 n) shares a byte with a source, a destination or an epilogue source of a pending record.
  bool touches(const PendingOuter& single, const void* p, size_t n) const {
    return (paired_ && touches(a_, p, n)) || (single.pending() && touches(single.record(), p, n));
  }

  // Breaks the pair: launch(A), then the register terms become B's epilogue terms.
  template <typename F>
  void unpair(PendingOuter& b, F&& launch) {
    if (!paired_) return;
    paired_ = false;  // first: `launch` may re-enter the library
    launch(static_cast<const Record&>(a_));
    for (int j = 0; j < a_.m; ++j)
      if ((mask_ >> j) & 1u) b.attach(e_[j], a_.y[j], b.record().y[j], a_.n);
    mask_ = 0;
  }

  // Launches the pair as one: launch(A, B, mask, e), the register terms e[j] for the bits of mask.
  template <typename F>
  void flush(PendingOuter& b, F&& launch) {
    if (!paired_) return;
    paired_ = false;
    Record rb;
    b.take(&rb);
    const unsigned mask = mask_;
    mask_ = 0;
    launch(static_cast<const Record&>(a_), static_cast<const Record&>(rb), mask, static_cast<const double*>(e_));
  }

  // Forgets A without launching it (the context is being destroyed); B is the PendingOuter's to forget.
  void discard() {
    paired_ = false;
    mask_ = 0;
  }

 private:
  static bool touches(const Record& r, const void* p, size_t n) {
    // ranges of different lengths: [p, p + 8 n) against [q, q + 8 r.n)
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const auto hit = [&](const void* q) {
      const uintptr_t b = reinterpret_cast<uintptr_t>(q);
      return a < b + r.n * sizeof(double) && b < a + n * sizeof(double);
    };
    for (int i = 0; i < r.k; ++i)
      if (hit(r.x[i])) return true;
    for (int j = 0; j < r.m; ++j)
      if (hit(r.y[j]) || (((r.mask >> j) & 1u) && hit(r.ex[j]))) return true;
    return false;
  }

  Record a_;
  double e_[kDst] = {};
  unsigned mask_ = 0;
  bool paired_ = false;
};

}  // namespace ssp
