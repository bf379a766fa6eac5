// The norms a flushed gemm_outer record left behind: when the call that launches the pending record
// (pending_outer.h) is ssp_dot(y, y, n) on exactly one of its destinations, the launch is the NRM
// instance of k_gemm_outer, which sums the squares of every destination as it stores it -- the bits
// k_dot_partial and its fold give on the stored vector.  The m sums are kept here, keyed by the
// destinations' addresses and n, and each later ssp_dot(y_j, y_j, n) on one of them is answered from
// here with no launch.  Every other entry point forgets them all (the prologue that launches a pending
// record: ssp::flush_outer), since any of them may change a destination.  DESIGN.md "Deferred gemm_outer".
//
// Host-only and free of HIP, like PendingOuter: tests/cpp/outer_norms_test.cpp drives it on the CPU.
#pragma once
#include <cstddef>

namespace ssp {

class OuterNorms {
 public:
  static constexpr int kDst = 16;  // ssp::kOuterDst: destinations of one launch

  bool empty() const { return m_ == 0; }
  int size() const { return m_; }

  // The destinations of the launch that is summing their squares; the values follow (set_values), or
  // stay on the device when ranks share the vectors (the caller keeps them, indexed as find() says).
  // False (nothing kept) when m is not 1..kDst or n is 0.
  bool keep(double* const* y, int m, size_t n) {
    forget();
    if (m < 1 || m > kDst || n == 0) return false;
    for (int j = 0; j < m; ++j) {
      y_[j] = y[j];
      v_[j] = 0.0;
    }
    n_ = n;
    m_ = m;
    return true;
  }
  void set_values(const double* v) {
    for (int j = 0; j < m_; ++j) v_[j] = v[j];
  }

  // The index of the kept destination that is exactly (y, n), or -1.  A view of a destination (another
  // address or another length) is not it.
  int find(const double* y, size_t n) const {
    if (n != n_) return -1;
    for (int j = 0; j < m_; ++j)
      if (y_[j] == y) return j;
    return -1;
  }
  double value(int j) const { return v_[j]; }

  void forget() {
    m_ = 0;
    n_ = 0;
  }

 private:
  const double* y_[kDst] = {};
  double v_[kDst] = {};
  size_t n_ = 0;
  int m_ = 0;
};

}  // namespace ssp
