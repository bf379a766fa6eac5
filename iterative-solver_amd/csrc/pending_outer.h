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

 private:
  static bool overlap(const void* a, const void* b, size_t n) {
    const uintptr_t p = reinterpret_cast<uintptr_t>(a), q = reinterpret_cast<uintptr_t>(b);
    const size_t bytes = n * sizeof(double);
    return p < q + bytes && q < p + bytes;
  }

  Record r_;
  bool pending_ = false;
};

}  // namespace ssp
