// Pending zero fills of a context: ssp_fill(+0.0) records its range here instead of launching, and the
// range is stored later (a k_fill launch, "flushed"), dropped (a write-only op overwrites it) or
// consumed (ssp_gemm_outer starts its accumulators from zero instead of reading the zeros back).
// DESIGN.md "Deferred zero fills".
//
// Host-only and free of HIP: the table knows addresses and lengths, and every store goes through the
// `flush(p, n)` callable its caller passes (tests/cpp/pending_fill_test.cpp drives it on the CPU).
//
// Invariant: entries are pairwise disjoint, and kept in the order their fills were issued.
#pragma once
#include <cstddef>
#include <cstdint>

namespace ssp {

class PendingFills {
 public:
  static constexpr int kCapacity = 64;  // more than two full destination sets of kOuterDst = 16

  struct Entry {
    uintptr_t p;  // first byte
    size_t n;     // doubles: the range is [p, p + 8 n)
  };

  int size() const { return count_; }
  bool empty() const { return count_ == 0; }
  const Entry& at(int i) const { return e_[i]; }

  // Index of the entry that is exactly (p, n), or -1.
  int find_exact(const void* p, size_t n) const {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    for (int i = 0; i < count_; ++i)
      if (e_[i].p == a && e_[i].n == n) return i;
    return -1;
  }

  // Index of the first entry at or after `from` that shares a byte with [p, p + 8 n), or -1.
  int find_overlap(const void* p, size_t n, int from = 0) const {
    return find_overlap_bytes(reinterpret_cast<uintptr_t>(p), n * sizeof(double), from);
  }

  // Removes entry i; the others keep their order.
  void erase(int i) {
    for (int j = i + 1; j < count_; ++j) e_[j - 1] = e_[j];
    --count_;
  }

  // Stores every entry, oldest first, and empties the table.
  template <typename F>
  void drain(F&& flush) {
    // the table is emptied first: `flush` may re-enter the library
    Entry all[kCapacity];
    const int c = count_;
    for (int i = 0; i < c; ++i) all[i] = e_[i];
    count_ = 0;
    for (int i = 0; i < c; ++i) flush(reinterpret_cast<double*>(all[i].p), all[i].n);
  }

  // Stores (and removes) every entry that shares a byte with [p, p + 8 n): a reader, or a
  // read-modify-write, of that range follows.
  template <typename F>
  void flush_overlap(const void* p, size_t n, F&& flush) {
    for (int i = find_overlap(p, n); i >= 0; i = find_overlap(p, n, i)) {
      const Entry x = e_[i];
      erase(i);
      flush(reinterpret_cast<double*>(x.p), x.n);
    }
  }

  // A write of all of [p, p + bytes) that reads nothing follows (or the range is being freed): entries
  // wholly inside it are dropped, entries it only partly overlaps are stored.
  template <typename F>
  void overwrite_bytes(const void* p, size_t bytes, F&& flush) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    for (int i = find_overlap_bytes(a, bytes, 0); i >= 0; i = find_overlap_bytes(a, bytes, i)) {
      const Entry x = e_[i];
      erase(i);
      const bool inside = x.p >= a && x.p + x.n * sizeof(double) <= a + bytes;
      if (!inside) flush(reinterpret_cast<double*>(x.p), x.n);
    }
  }
  template <typename F>
  void overwrite(const void* p, size_t n, F&& flush) {
    overwrite_bytes(p, n * sizeof(double), static_cast<F&&>(flush));
  }

  // Records a zero fill of [p, p + 8 n), n > 0: entries it covers are dropped, entries it partly
  // overlaps are stored first, and a full table is drained first.
  template <typename F>
  void insert(const void* p, size_t n, F&& flush) {
    overwrite(p, n, flush);
    if (count_ == kCapacity) drain(flush);
    e_[count_].p = reinterpret_cast<uintptr_t>(p);
    e_[count_].n = n;
    ++count_;
  }

  // Forgets every entry without storing it (the context is being destroyed).
  void clear() { count_ = 0; }

 private:
  int find_overlap_bytes(uintptr_t a, size_t bytes, int from) const {
    if (bytes == 0) return -1;
    for (int i = from; i < count_; ++i)
      if (e_[i].p < a + bytes && a < e_[i].p + e_[i].n * sizeof(double)) return i;
    return -1;
  }

  Entry e_[kCapacity];
  int count_ = 0;
};

}  // namespace ssp
