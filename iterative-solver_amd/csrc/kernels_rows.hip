// Row blocks: a caller's row-major block of vectors <-> arena vectors, device to device, one pass.
//
// ssp_rows_import / ssp_rows_export are where the library meets memory it did not allocate (the device
// forms of the reverse-communication API, include/iterative_solver_c.h).  The arena side of a row is
// 16-byte aligned as everywhere else; the caller's side is any double* base and any ld >= n, so a row of
// the caller's block sits at 0 or at 8 mod 16, decided per row (an odd ld alternates).
//   aligned row     the 16-byte path of k_copy / k_copy_win (kernels_stream.hip): the same loops, the
//                   window shape and nontemporal accesses from kWinMin elements;
//   misaligned row  8-byte accesses on both sides, lane i at element base + i: every wave instruction is
//                   one contiguous 512-byte run (a 16-byte access of one side would straddle the other
//                   side's element pairs); the same two shapes, windows of the same bytes per wave.
// One launch moves up to kRowsMax rows (blockIdx.y is the row); pointers and scales ride in the kernel
// argument block.  A row is a bit copy, or with a scale s != 1 the single product x * s of k_copy<true>.
// ssp_rows_export_quantised is the export with the first mq rows rounded through binary32 as they are stored,
// (double)(float)(x * s): k_quantise_f32's value in the export's pass, the same four shapes (k_rows_q).
#include <algorithm>
#include <string>

#include "ssp_internal.h"

namespace {

using ssp::kBlock;
using ssp::kWinMin;
using ssp::kWinU;

constexpr int kRowsMax = 16;

struct RowsArgs {
  const double* src[kRowsMax];
  double* dst[kRowsMax];
  double s[kRowsMax];
  size_t n;
};

using ssp::ld2, ssp::sc1, ssp::sc2, ssp::st2;  // QT: the value k_quantise_f32 stores
__device__ __forceinline__ double ld1nt(const double* p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ void st1nt(double* p, double v) { __builtin_nontemporal_store(v, p); }
// Both sides 16-byte aligned: k_copy's loop (WIN: k_copy_win's).
template <bool SC, bool WIN, bool QT = false>
__device__ __forceinline__ void row_copy16(double* __restrict__ x, const double* __restrict__ y, size_t n, double s) {
  using ssp::ld2nt;
  using ssp::st2nt;
  if (WIN) {
    ssp::for_windows<kWinU>(
        n,
        [&](size_t p0) {
          double2 v[kWinU];
#pragma unroll
          for (int u = 0; u < kWinU; ++u) v[u] = ld2nt(y + 2 * (p0 + 64 * u));
#pragma unroll
          for (int u = 0; u < kWinU; ++u) st2nt(x + 2 * (p0 + 64 * u), sc2<SC, QT>(v[u], s));
        },
        [&](size_t i) { st2(x + 2 * i, sc2<SC, QT>(ld2(y + 2 * i), s)); }, [&](size_t e) { x[e] = sc1<SC, QT>(y[e], s); });
    return;
  }
  const size_t n2 = n >> 1;
  const size_t stride = size_t(gridDim.x) * kBlock;
  size_t i = size_t(blockIdx.x) * kBlock + threadIdx.x;
  for (; i + 3 * stride < n2; i += 4 * stride) {
    double2 a0 = ld2nt(y + 2 * i), a1 = ld2nt(y + 2 * (i + stride)), a2 = ld2nt(y + 2 * (i + 2 * stride)),
            a3 = ld2nt(y + 2 * (i + 3 * stride));
    st2nt(x + 2 * i, sc2<SC, QT>(a0, s));
    st2nt(x + 2 * (i + stride), sc2<SC, QT>(a1, s));
    st2nt(x + 2 * (i + 2 * stride), sc2<SC, QT>(a2, s));
    st2nt(x + 2 * (i + 3 * stride), sc2<SC, QT>(a3, s));
  }
  for (; i < n2; i += stride) st2(x + 2 * i, sc2<SC, QT>(ld2(y + 2 * i), s));
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) x[n - 1] = sc1<SC, QT>(y[n - 1], s);
}

// One side at 8 mod 16: the same two shapes over single elements.  WIN: a wave owns 2 kWinU x 64
// consecutive elements per visit (the kWinU KiB of row_copy16's window), whole windows first, then the
// elements past the last whole window, thread-granular.
template <bool SC, bool WIN, bool QT = false>
__device__ __forceinline__ void row_copy8(double* __restrict__ x, const double* __restrict__ y, size_t n, double s) {
  if (WIN) {
    constexpr int U = 2 * kWinU;
    const int lane = threadIdx.x & 63;
    const size_t gw = size_t(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
    const size_t nw = size_t(gridDim.x) * (kBlock / 64);
    const size_t win = 64 * size_t(U), nwin = n / win;
    for (size_t c = gw; c < nwin; c += nw) {
      const size_t e0 = c * win + lane;
      double v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = ld1nt(y + e0 + 64 * u);
#pragma unroll
      for (int u = 0; u < U; ++u) st1nt(x + e0 + 64 * u, sc1<SC, QT>(v[u], s));
    }
    for (size_t e = nwin * win + size_t(blockIdx.x) * kBlock + threadIdx.x; e < n; e += size_t(gridDim.x) * kBlock)
      x[e] = sc1<SC, QT>(y[e], s);
    return;
  }
  const size_t stride = size_t(gridDim.x) * kBlock;
  size_t i = size_t(blockIdx.x) * kBlock + threadIdx.x;
  for (; i + 3 * stride < n; i += 4 * stride) {
    const double a0 = ld1nt(y + i), a1 = ld1nt(y + i + stride), a2 = ld1nt(y + i + 2 * stride),
                 a3 = ld1nt(y + i + 3 * stride);
    st1nt(x + i, sc1<SC, QT>(a0, s));
    st1nt(x + i + stride, sc1<SC, QT>(a1, s));
    st1nt(x + i + 2 * stride, sc1<SC, QT>(a2, s));
    st1nt(x + i + 3 * stride, sc1<SC, QT>(a3, s));
  }
  for (; i < n; i += stride) x[i] = sc1<SC, QT>(y[i], s);
}

// dst[r] = s[r] * src[r], row r = blockIdx.y; parity and scale are uniform over the row's workgroups.
template <bool WIN>
__global__ __launch_bounds__(kBlock) void k_rows(const RowsArgs a) {
  const int r = blockIdx.y;
  double* const x = a.dst[r];
  const double* const y = a.src[r];
  const double s = a.s[r];
  const bool mis = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15u) != 0;
  if (!mis) {
    if (s == 1.0) row_copy16<false, WIN>(x, y, a.n, s);
    else row_copy16<true, WIN>(x, y, a.n, s);
  } else {
    if (s == 1.0) row_copy8<false, WIN>(x, y, a.n, s);
    else row_copy8<true, WIN>(x, y, a.n, s);
  }
}

// k_rows with rows [0, mq) of the launch rounded through binary32 as they are stored (the export that
// rounds, ssp_rows_export_quantised): the same four shapes, the rounding in place of nothing.
struct RowsQArgs {
  RowsArgs r;
  int mq;
};

template <bool WIN, bool QT>
__device__ __forceinline__ void row_any(double* x, const double* y, size_t n, double s) {
  const bool mis = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15u) != 0;
  if (!mis) {
    if (s == 1.0) row_copy16<false, WIN, QT>(x, y, n, s);
    else row_copy16<true, WIN, QT>(x, y, n, s);
  } else {
    if (s == 1.0) row_copy8<false, WIN, QT>(x, y, n, s);
    else row_copy8<true, WIN, QT>(x, y, n, s);
  }
}

template <bool WIN>
__global__ __launch_bounds__(kBlock) void k_rows_q(const RowsQArgs a) {
  const int r = blockIdx.y;
  if (r < a.mq) row_any<WIN, true>(a.r.dst[r], a.r.src[r], a.r.n, a.r.s[r]);
  else row_any<WIN, false>(a.r.dst[r], a.r.src[r], a.r.n, a.r.s[r]);
}

// Rows [r0, r0 + mm) of one call, already checked: one launch.  The grid of one row is k_copy's for n
// elements; the rows together stay within that rule's workgroups per CU (grid-stride beyond).
// mq >= 0: the first mq rows of the launch are rounded (k_rows_q).
int launch_rows(ssp_ctx* ctx, const char* op, const RowsArgs& a, int mm, int mq = -1) {
  const size_t n = a.n;
  const bool win = n >= kWinMin;
  const unsigned per_cu = win ? 16 : 64;
  unsigned gx = win ? ssp::win_grid(ctx, n, kWinU, per_cu) : ssp::stream_grid(ctx, n / 2 + 1, 4, per_cu);
  const unsigned cap = unsigned(ctx->num_cus) * per_cu;
  if (size_t(gx) * size_t(mm) > cap) gx = std::max(1u, cap / unsigned(mm));
  ssp::LedgerScope ls(ctx, op, 16.0 * mm * n);
  const dim3 g(gx, unsigned(mm));
  if (mq >= 0) {
    const RowsQArgs q{a, mq};
    if (win) SSP_LAUNCH(k_rows_q<true>, g, dim3(kBlock), 0, ctx->stream, q);
    else SSP_LAUNCH(k_rows_q<false>, g, dim3(kBlock), 0, ctx->stream, q);
    SSP_TRY_HIP(hipGetLastError());
    return SSP_OK;
  }
  if (win) SSP_LAUNCH(k_rows<true>, g, dim3(kBlock), 0, ctx->stream, a);
  else SSP_LAUNCH(k_rows<false>, g, dim3(kBlock), 0, ctx->stream, a);
  SSP_TRY_HIP(hipGetLastError());
  return SSP_OK;
}

int bad(const char* what, const char* why) { return ssp::set_error(SSP_ERR_ARG, std::string(what) + ": " + why); }

// The argument checks both directions share: `arena` are the m library vectors, `block` the caller's.
int check_rows(const char* what, const void* block, size_t ld, const double* const* arena, int m, size_t n) {
  if (m < 0) return bad(what, "negative row count");
  if (m == 0 || n == 0) return SSP_OK;
  if (ld < n) return bad(what, "ld smaller than the row length");
  if (!block) return bad(what, "null row block");
  if (reinterpret_cast<uintptr_t>(block) & 7u) return bad(what, "row block not 8-byte aligned");
  if (!arena) return bad(what, "null vector list");
  for (int k = 0; k < m; ++k) {
    if (!arena[k]) return bad(what, "null vector");
    if (!ssp::aligned16(arena[k])) return bad(what, "vector not 16-byte aligned");
  }
  return SSP_OK;
}

}  // namespace

extern "C" {

int ssp_rows_import(ssp_ctx* ctx, const double* src, size_t ld, double* const* dst, int m, size_t n) {
  SSP_CHECK_CTX_KEEP_FILLS(ctx);
  SSP_TRY(check_rows("ssp_rows_import", src, ld, dst, m, n));
  if (m <= 0 || n == 0) return SSP_OK;
  // pending zero fills: the caller's rows are read, so theirs are stored; every destination is written
  // in full and never read, so the ones inside it are dropped
  for (int k = 0; k < m; ++k) {
    SSP_TRY(ssp::flush_fills_over(ctx, src + size_t(k) * ld, n));
    SSP_TRY(ssp::overwrite_fills(ctx, dst[k], n));
  }
  for (int r0 = 0; r0 < m; r0 += kRowsMax) {
    RowsArgs a{};
    const int mm = std::min(kRowsMax, m - r0);
    for (int r = 0; r < mm; ++r) {
      a.src[r] = src + size_t(r0 + r) * ld;
      a.dst[r] = dst[r0 + r];
      a.s[r] = 1.0;
    }
    a.n = n;
    SSP_TRY(launch_rows(ctx, "rows_import", a, mm));
  }
  return SSP_OK;
}

int ssp_rows_export(ssp_ctx* ctx, const double* const* src, const double* xs, int m, double* dst, size_t ld, size_t n) {
  SSP_CHECK_CTX_KEEP_FILLS(ctx);
  SSP_TRY(check_rows("ssp_rows_export", dst, ld, src, m, n));
  if (m <= 0 || n == 0) return SSP_OK;
  // a source with a recorded fill is stored first; fills inside the rows being written are dropped
  for (int k = 0; k < m; ++k) {
    SSP_TRY(ssp::flush_fills_over(ctx, src[k], n));
    SSP_TRY(ssp::overwrite_fills(ctx, dst + size_t(k) * ld, n));
  }
  for (int r0 = 0; r0 < m; r0 += kRowsMax) {
    RowsArgs a{};
    const int mm = std::min(kRowsMax, m - r0);
    for (int r = 0; r < mm; ++r) {
      a.src[r] = src[r0 + r];
      a.dst[r] = dst + size_t(r0 + r) * ld;
      a.s[r] = xs ? xs[r0 + r] : 1.0;
    }
    a.n = n;
    SSP_TRY(launch_rows(ctx, "rows_export", a, mm));
  }
  return SSP_OK;
}

int ssp_rows_export_quantised(ssp_ctx* ctx, const double* const* src, const double* xs, int m, int mq, double* dst,
                              size_t ld, size_t n) {
  SSP_CHECK_CTX_KEEP_FILLS(ctx);
  SSP_TRY(check_rows("ssp_rows_export_quantised", dst, ld, src, m, n));
  if (mq < 0 || mq > std::max(m, 0)) return bad("ssp_rows_export_quantised", "mq outside [0, m]");
  if (m <= 0 || n == 0) return SSP_OK;
  for (int k = 0; k < m; ++k) {
    SSP_TRY(ssp::flush_fills_over(ctx, src[k], n));
    SSP_TRY(ssp::overwrite_fills(ctx, dst + size_t(k) * ld, n));
  }
  for (int r0 = 0; r0 < m; r0 += kRowsMax) {
    RowsArgs a{};
    const int mm = std::min(kRowsMax, m - r0);
    for (int r = 0; r < mm; ++r) {
      a.src[r] = src[r0 + r];
      a.dst[r] = dst + size_t(r0 + r) * ld;
      a.s[r] = xs ? xs[r0 + r] : 1.0;
    }
    a.n = n;
    SSP_TRY(launch_rows(ctx, "rows_export_q", a, mm, std::min(mm, std::max(0, mq - r0))));
  }
  return SSP_OK;
}

}  // extern "C"
