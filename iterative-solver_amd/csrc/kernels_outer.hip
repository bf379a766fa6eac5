// gemm_outer (k sources -> m destinations), its deferred launch and the norms that launch can carry.
//
// Reference: util/gemm.h:257-279 computes it pairwise (handler.axpy per pair), so a 48 -> 8 gemm_outer
// streams 3*8*48 vectors.  Here every vector of the panel is read from HBM exactly once per call:
//   gemm_outer  bytes = 8 N (k + 2 m)
// Also the one home of the deferral protocol over ssp_ctx::outer (DESIGN.md "Deferred gemm_outer"): when a
// call becomes a record (gemm_outer_impl) or the second record of a pair (pair_candidate), who may attach to
// it (outer_take_axpy), who launches it and as which instance (flush_outer, outer_serve_dot), which fill
// leaves it pending (outer_keeps_fill), when the kept norms die and where the rank-local sums live.
#include <algorithm>
#include <string>
#include <vector>

#include "ssp_internal.h"

namespace {

using ssp::kBlock;
using ssp::ld2, ssp::sc1, ssp::sc2;

struct OuterArgs {
  const double* x[ssp::kOuterSrc];
  double* y[ssp::kOuterDst];
  int k;
  int m;
  int set;  // 1: yy[j] = sum (destinations not read: fill(0) + gemm_outer in one pass)
  // EPI: bit j set: y[j] += epi[j] * x[k + j] (the epilogue sources ride in the source slots past the
  // k sources, so k + m <= kOuterSrc).  The new members sit in the padding after `set` and behind
  // `alpha`: every other member keeps its offset, and the instances without EPI their code.
  int epi_mask;
  size_t n;
  const double* alpha_dev;         // k*m > kOuterAlpha: alpha[i*m + j] in device memory
  const double* scale_dev;         // SC: deferred scales, sources [0, k) then destinations [k, k + m)
  double alpha[ssp::kOuterAlpha];  // alpha[i*m + j] in the argument block
  double epi[ssp::kOuterDst];
  // NRM: per-workgroup sums of squares partial[b * m + j], folded by `tail` (nout = m).  At the end of
  // the block, for the same reason.
  double* partial;
  ssp::FoldTail tail;
};
static_assert(sizeof(OuterArgs) <= 4000, "kernel argument block too large");
static_assert(ssp::PendingOuter::kSrc == ssp::kOuterSrc && ssp::PendingOuter::kDst == ssp::kOuterDst,
              "pending_outer.h records one launch");

// yy[j] += sum_i alpha(i,j) xx[i]: for each destination the sources are added in order i = 0..k-1,
// as the reference's pairwise axpy loop does (util/gemm.h:259-264).  Each wave owns windows of
// kOuterWin consecutive double2 positions (64 lanes x 16 B x kOuterWin contiguous bytes per vector)
// and loads 4 sources x kOuterWin positions before the fmas; sources and destinations are streamed
// once, with nontemporal accesses (tools/mb_stream.hip: 5.35 TB/s against 4.8 for one position per
// lane and plain accesses).
constexpr int kOuterWin = 4;
static_assert(kOuterWin == ssp::kDotU, "the norm-carrying instance walks k_dot_partial's windows");

// SET (a.set = 1) is a separate instantiation: the write-only construct_solution form shows under its
// own name in rocprofv3 statistics, so its launches are not averaged with the read-modify-write ones.
// SC: sources and (read-modify-write) destinations with deferred scales, applied as each element is
// loaded (include/subspace_hip.h ssp_gemm_outer_scaled).
// EPI (the flushed record of pending_outer.h with attached ssp_axpy terms): before destination j of
// a.epi_mask is stored, epi[j] * x[k + j] is added to its finished sum by the fma k_axpy_win would have
// done on the stored value.  Unmasked destinations take no term: fma(0, x, acc) would turn a -0.0 sum
// into +0.0 and an infinite x into NaN.
// NRM (the record launched by the ssp_dot(y, y) of one of its destinations, outer_norms.h): next to the
// stores, the sum of squares of every destination as stored, in the bits k_dot_partial<true, false> and
// its fold give on the stored vector.  The launch takes that kernel's grid and its walk: whole windows in
// the window loop (window position u into accumulator u: fma(v.x, v.x, .), fma(v.y, v.y, .)), then the
// positions past the last whole window one per thread of workgroup 0 and the odd last element in its
// thread 0, both into accumulator 0; (s0 + s1) + (s2 + s3), block_sum256's tree, partial[b * m + j],
// ssp::fold_tail.  The stored elements do not depend on the thread that forms them.  The 4 M
// accumulators per lane live in LDS ([j][u][thread]: every lane its own bank pair, 8 M KiB per
// workgroup), not in 8 M more VGPRs, which would halve the M = 8 instance's waves per SIMD.
template <int M>
__device__ __forceinline__ double* outer_norm_acc() {
  __shared__ double acc[M * kOuterWin * kBlock];
  return acc;
}

template <int M, bool DEV, bool SET, bool SC = false, bool EPI = false, bool NRM = false>
__global__ __launch_bounds__(kBlock) void k_gemm_outer(const OuterArgs a) {
  static_assert(!EPI || (SET && !SC), "the epilogue rides on the unscaled write-only form");
  static_assert(!NRM || (SET && !SC && M <= 8), "the norms ride on the unscaled write-only form, 4-position windows");
  using ssp::ld2nt;
  using ssp::st2nt;
  // Device-resident alphas are read through the constant address space (scalar loads, as the
  // argument block's are): they are uniform across the wave and read-only in the kernel.
  using cdouble = const __attribute__((address_space(4))) double;
  const auto alpha = [&](int idx) { return DEV ? ((cdouble*)a.alpha_dev)[idx] : a.alpha[idx]; };
  const auto scale = [&](int idx) { return SC ? ((cdouble*)a.scale_dev)[idx] : 1.0; };
  constexpr int U = M > 8 ? 2 : kOuterWin;  // 16 destinations: 2 windows keep 2 waves per SIMD
  const int lane = threadIdx.x & 63;
  const size_t gw = size_t(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
  const size_t nw = size_t(gridDim.x) * (kBlock / 64);
  const size_t n2 = a.n >> 1, win = 64 * U;
  const double2 z2 = make_double2(0, 0);
  double* nacc = nullptr;  // this thread's accumulators: [j][u] at (j * U + u) * kBlock
  if constexpr (NRM) {
    nacc = outer_norm_acc<M>() + threadIdx.x;
#pragma unroll
    for (int q = 0; q < M * U; ++q) nacc[q * kBlock] = 0;
  }
  // NRM: whole windows only, as ssp::for_windows walks them
  for (size_t c = gw; NRM ? c < n2 / win : c * win < n2; c += nw) {
    const size_t p0 = c * win + lane;
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) ok[u] = NRM || p0 + 64 * u < n2;
    double2 acc[U][M];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < M; ++j) acc[u][j] = (j < a.m && ok[u] && !SET) ? ld2nt(a.y[j] + 2 * (p0 + 64 * u)) : z2;
    if constexpr (SC && !SET) {
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int j = 0; j < M; ++j)
          if (j < a.m) acc[u][j] = sc2<SC>(acc[u][j], scale(a.k + j));  // only a.k + a.m scales exist
    }
    int i = 0;
    for (; i + 4 <= a.k; i += 4) {
      double2 xv[4][U];
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int u = 0; u < U; ++u) xv[b][u] = ok[u] ? ld2nt(a.x[i + b] + 2 * (p0 + 64 * u)) : z2;
      if constexpr (SC) {
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
          for (int u = 0; u < U; ++u) xv[b][u] = sc2<SC>(xv[b][u], scale(i + b));
      }
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int j = 0; j < M; ++j) {
          if (j < a.m) {
            const double al = alpha((i + b) * a.m + j);
#pragma unroll
            for (int u = 0; u < U; ++u) {
              acc[u][j].x = fma(al, xv[b][u].x, acc[u][j].x);
              acc[u][j].y = fma(al, xv[b][u].y, acc[u][j].y);
            }
          }
        }
    }
    for (; i < a.k; ++i) {
      double2 xv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) xv[u] = ok[u] ? ld2nt(a.x[i] + 2 * (p0 + 64 * u)) : z2;
      if constexpr (SC) {
#pragma unroll
        for (int u = 0; u < U; ++u) xv[u] = sc2<SC>(xv[u], scale(i));
      }
#pragma unroll
      for (int j = 0; j < M; ++j) {
        if (j < a.m) {
          const double al = alpha(i * a.m + j);
#pragma unroll
          for (int u = 0; u < U; ++u) {
            acc[u][j].x = fma(al, xv[u].x, acc[u][j].x);
            acc[u][j].y = fma(al, xv[u].y, acc[u][j].y);
          }
        }
      }
    }
    if constexpr (EPI) {
      // B destinations' terms in flight.  The compiler gives ev registers of its own beside xv's (16 B
      // VGPRs at U = 4), so B is what keeps each instance at the waves per SIMD of its write-only form:
      // two at M = 8 (234 VGPRs, two waves, 8 loads per lane in flight), one elsewhere.
      constexpr int B = M == 8 ? 2 : 1;
#pragma unroll
      for (int j0 = 0; j0 < M; j0 += B) {
        double2 ev[B][U];
        bool on[B];
#pragma unroll
        for (int b = 0; b < B; ++b) {
          on[b] = j0 + b < a.m && ((a.epi_mask >> (j0 + b)) & 1);
          if (on[b]) {
#pragma unroll
            for (int u = 0; u < U; ++u) ev[b][u] = ok[u] ? ld2nt(a.x[a.k + j0 + b] + 2 * (p0 + 64 * u)) : z2;
          }
        }
#pragma unroll
        for (int b = 0; b < B; ++b) {
          if (on[b]) {
            const double ea = a.epi[j0 + b];
#pragma unroll
            for (int u = 0; u < U; ++u) {
              acc[u][j0 + b].x = fma(ea, ev[b][u].x, acc[u][j0 + b].x);
              acc[u][j0 + b].y = fma(ea, ev[b][u].y, acc[u][j0 + b].y);
            }
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (ok[u])
#pragma unroll
        for (int j = 0; j < M; ++j)
          if (j < a.m) st2nt(a.y[j] + 2 * (p0 + 64 * u), acc[u][j]);
    if constexpr (NRM) {
#pragma unroll
      for (int j = 0; j < M; ++j)
        if (j < a.m) {
#pragma unroll
          for (int u = 0; u < U; ++u) {
            double s = nacc[(j * U + u) * kBlock];
            s = fma(acc[u][j].x, acc[u][j].x, s);
            s = fma(acc[u][j].y, acc[u][j].y, s);
            nacc[(j * U + u) * kBlock] = s;
          }
          // one destination's accumulators in registers at a time: scheduled freely, all 4 M are loaded
          // up front (100, 126, 175, 242 VGPRs at M = 1, 2, 4, 8 with the epilogue: a wave per SIMD
          // fewer than the instances without norms at M = 1 and M = 4)
          __builtin_amdgcn_sched_barrier(0);
        }
    }
  }
  if constexpr (NRM) {
    if (blockIdx.x == 0) {
      const size_t p = (n2 / win) * win + threadIdx.x;  // fewer than win = kBlock positions are left
      if (p < n2) {
        for (int j = 0; j < a.m; ++j) {
          double2 v = z2;
          for (int i = 0; i < a.k; ++i) {
            const double al = alpha(i * a.m + j);
            const double2 xv = ld2(a.x[i] + 2 * p);
            v.x = fma(al, xv.x, v.x);
            v.y = fma(al, xv.y, v.y);
          }
          if constexpr (EPI) {
            if ((a.epi_mask >> j) & 1) {
              const double2 ev = ld2(a.x[a.k + j] + 2 * p);
              v.x = fma(a.epi[j], ev.x, v.x);
              v.y = fma(a.epi[j], ev.y, v.y);
            }
          }
          *reinterpret_cast<double2*>(a.y[j] + 2 * p) = v;
          double s = nacc[j * U * kBlock];
          s = fma(v.x, v.x, s);
          s = fma(v.y, v.y, s);
          nacc[j * U * kBlock] = s;
        }
      }
      if ((a.n & 1) && threadIdx.x == 0) {
        const size_t e = a.n - 1;
        for (int j = 0; j < a.m; ++j) {
          double v = 0.0;
          for (int i = 0; i < a.k; ++i) v = fma(alpha(i * a.m + j), a.x[i][e], v);
          if constexpr (EPI) {
            if ((a.epi_mask >> j) & 1) v = fma(a.epi[j], a.x[a.k + j][e], v);
          }
          a.y[j][e] = v;
          nacc[j * U * kBlock] = fma(v, v, nacc[j * U * kBlock]);
        }
      }
    }
    __shared__ double red[kBlock / 64][M];
#pragma unroll
    for (int j = 0; j < M; ++j)
      if (j < a.m) {
        const double s0 = nacc[(j * U + 0) * kBlock], s1 = nacc[(j * U + 1) * kBlock];
        const double s2 = nacc[(j * U + 2) * kBlock], s3 = nacc[(j * U + 3) * kBlock];
        double v = (s0 + s1) + (s2 + s3);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) red[threadIdx.x >> 6][j] = v;
      }
    __syncthreads();
    if (int(threadIdx.x) < a.m) {
      double s = 0;  // block_sum256's order
#pragma unroll
      for (int w = 0; w < kBlock / 64; ++w) s += red[w][threadIdx.x];
      ssp::store_partial(a.partial + size_t(blockIdx.x) * a.m + threadIdx.x, s);
    }
    ssp::fold_tail<M>(a.partial, a.tail);
    return;
  }
  if ((a.n & 1) && blockIdx.x == 0 && threadIdx.x < a.m) {
    const size_t e = a.n - 1;
    const int j = threadIdx.x;
    double v = SET ? 0.0 : sc1<SC>(a.y[j][e], scale(a.k + j));
    for (int i = 0; i < a.k; ++i) v = fma(alpha(i * a.m + j), sc1<SC>(a.x[i][e], scale(i)), v);
    if constexpr (EPI) {
      if ((a.epi_mask >> j) & 1) v = fma(a.epi[j], a.x[a.k + j][e], v);
    }
    a.y[j][e] = v;
  }
}

// The launch of a pair of records (pending_outer.h OuterPair): both solution constructions of a step in one
// pass.  The two records share k, m, n and the alphas (device-resident: 2 k pointers, 2 m destinations and the
// alphas do not fit the argument block together; one staged upload of 8 k m bytes per launch, as every launch
// with k m > kOuterAlpha makes).
struct PairArgs {
  const double* xp[ssp::kOuterSrc];  // A's sources
  const double* xa[ssp::kOuterSrc];  // B's sources
  double* yp[ssp::OuterPair::kDst];  // A's destinations
  double* ya[ssp::OuterPair::kDst];  // B's destinations
  double e[ssp::OuterPair::kDst];    // register terms: ya[j] += e[j] * yp[j] for the bits of mask
  const double* alpha_dev;           // alpha[i * m + j]
  size_t n;
  int k;
  int m;
  int mask;
  double* partial;  // as OuterArgs::partial, for the sums of squares of ya
  ssp::FoldTail tail;
};
static_assert(sizeof(PairArgs) <= 4000, "kernel argument block too large");

// yp[j] = sum_i alpha(i,j) xp[i]; ya[j] = sum_i alpha(i,j) xa[i], then for the masked j
// ya[j] = fma(e[j], yp[j], ya[j]) with yp[j] the accumulator just stored -- the double the separate launch
// would have reloaded, so the fma is k_axpy_win's (or EPI's) -- and the sums of squares of the stored ya[j].
// Every destination sees its sources in the order i = 0..k-1 from +0.0, as the SET instance forms it; an
// unmasked destination takes no fma, for the reasons given at k_gemm_outer.  Always the norm-carrying form
// (the pair is launched by the ssp_dot of one of B's destinations and by nothing else), so it takes
// k_dot_partial's grid and walk exactly as the NRM instance of k_gemm_outer does.  Two accumulator sets at
// 4-position windows would need 256 VGPRs: a wave covers its window as two half-windows of two positions
// (u = 0, 1, then u = 2, 3), the P sums then the A sums of each, and each half-window feeds the norm
// accumulators of its own two positions, so accumulator u sees the elements it sees in k_dot_partial, in
// that order.  B: sources in flight per phase.
constexpr int kPairHalf = 2;
template <int M, int B>
__global__ __launch_bounds__(kBlock) void k_gemm_outer_pair(const PairArgs a) {
  static_assert(M <= ssp::OuterPair::kDst && kOuterWin % kPairHalf == 0, "two half-windows of a dot window");
  using ssp::ld2nt;
  using ssp::st2nt;
  using cdouble = const __attribute__((address_space(4))) double;
  const auto alpha = [&](int idx) { return ((cdouble*)a.alpha_dev)[idx]; };
  constexpr int U = kOuterWin, H = kPairHalf;
  const int lane = threadIdx.x & 63;
  const size_t gw = size_t(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
  const size_t nw = size_t(gridDim.x) * (kBlock / 64);
  const size_t n2 = a.n >> 1, win = 64 * U;
  const double2 z2 = make_double2(0, 0);
  double* nacc = outer_norm_acc<M>() + threadIdx.x;  // [j][u] at (j * U + u) * kBlock
#pragma unroll
  for (int q = 0; q < M * U; ++q) nacc[q * kBlock] = 0;
  // acc[v][j] = sum_i alpha(i,j) x[i] at the positions q0 + 64 v
  const auto sums = [&](const double* const(&x)[ssp::kOuterSrc], size_t q0, double2(&acc)[H][M]) {
#pragma unroll
    for (int v = 0; v < H; ++v)
#pragma unroll
      for (int j = 0; j < M; ++j) acc[v][j] = z2;
    int i = 0;
    for (; i + B <= a.k; i += B) {
      double2 xv[B][H];
#pragma unroll
      for (int b = 0; b < B; ++b)
#pragma unroll
        for (int v = 0; v < H; ++v) xv[b][v] = ld2nt(x[i + b] + 2 * (q0 + 64 * v));
#pragma unroll
      for (int b = 0; b < B; ++b)
#pragma unroll
        for (int j = 0; j < M; ++j) {
          if (j < a.m) {
            const double al = alpha((i + b) * a.m + j);
#pragma unroll
            for (int v = 0; v < H; ++v) {
              acc[v][j].x = fma(al, xv[b][v].x, acc[v][j].x);
              acc[v][j].y = fma(al, xv[b][v].y, acc[v][j].y);
            }
          }
        }
    }
    for (; i < a.k; ++i) {
      double2 xv[H];
#pragma unroll
      for (int v = 0; v < H; ++v) xv[v] = ld2nt(x[i] + 2 * (q0 + 64 * v));
#pragma unroll
      for (int j = 0; j < M; ++j) {
        if (j < a.m) {
          const double al = alpha(i * a.m + j);
#pragma unroll
          for (int v = 0; v < H; ++v) {
            acc[v][j].x = fma(al, xv[v].x, acc[v][j].x);
            acc[v][j].y = fma(al, xv[v].y, acc[v][j].y);
          }
        }
      }
    }
  };
  for (size_t c = gw; c < n2 / win; c += nw) {  // whole windows only, as ssp::for_windows walks them
#pragma unroll
    for (int h = 0; h < U / H; ++h) {
      const size_t q0 = c * win + 64 * H * h + lane;  // window position u = H h + v at q0 + 64 v
      double2 ap[H][M], aa[H][M];
      sums(a.xp, q0, ap);
#pragma unroll
      for (int v = 0; v < H; ++v)
#pragma unroll
        for (int j = 0; j < M; ++j)
          if (j < a.m) st2nt(a.yp[j] + 2 * (q0 + 64 * v), ap[v][j]);
      sums(a.xa, q0, aa);
#pragma unroll
      for (int j = 0; j < M; ++j)
        if (j < a.m) {
          if ((a.mask >> j) & 1) {
            const double ea = a.e[j];
#pragma unroll
            for (int v = 0; v < H; ++v) {
              aa[v][j].x = fma(ea, ap[v][j].x, aa[v][j].x);
              aa[v][j].y = fma(ea, ap[v][j].y, aa[v][j].y);
            }
          }
#pragma unroll
          for (int v = 0; v < H; ++v) {
            st2nt(a.ya[j] + 2 * (q0 + 64 * v), aa[v][j]);
            double s = nacc[(j * U + H * h + v) * kBlock];
            s = fma(aa[v][j].x, aa[v][j].x, s);
            s = fma(aa[v][j].y, aa[v][j].y, s);
            nacc[(j * U + H * h + v) * kBlock] = s;
          }
          // one destination's accumulators in registers at a time, as in the NRM instance of k_gemm_outer
          __builtin_amdgcn_sched_barrier(0);
        }
    }
  }
  if (blockIdx.x == 0) {
    const size_t p = (n2 / win) * win + threadIdx.x;  // fewer than win = kBlock positions are left
    if (p < n2) {
      for (int j = 0; j < a.m; ++j) {
        double2 vp = z2, va = z2;
        for (int i = 0; i < a.k; ++i) {
          const double al = alpha(i * a.m + j);
          const double2 xp = ld2(a.xp[i] + 2 * p), xa = ld2(a.xa[i] + 2 * p);
          vp.x = fma(al, xp.x, vp.x);
          vp.y = fma(al, xp.y, vp.y);
          va.x = fma(al, xa.x, va.x);
          va.y = fma(al, xa.y, va.y);
        }
        if ((a.mask >> j) & 1) {
          va.x = fma(a.e[j], vp.x, va.x);
          va.y = fma(a.e[j], vp.y, va.y);
        }
        ssp::st2(a.yp[j] + 2 * p, vp);
        ssp::st2(a.ya[j] + 2 * p, va);
        double s = nacc[j * U * kBlock];
        s = fma(va.x, va.x, s);
        s = fma(va.y, va.y, s);
        nacc[j * U * kBlock] = s;
      }
    }
    if ((a.n & 1) && threadIdx.x == 0) {
      const size_t e = a.n - 1;
      for (int j = 0; j < a.m; ++j) {
        double vp = 0.0, va = 0.0;
        for (int i = 0; i < a.k; ++i) {
          vp = fma(alpha(i * a.m + j), a.xp[i][e], vp);
          va = fma(alpha(i * a.m + j), a.xa[i][e], va);
        }
        if ((a.mask >> j) & 1) va = fma(a.e[j], vp, va);
        a.yp[j][e] = vp;
        a.ya[j][e] = va;
        nacc[j * U * kBlock] = fma(va, va, nacc[j * U * kBlock]);
      }
    }
  }
  __shared__ double red[kBlock / 64][M];
#pragma unroll
  for (int j = 0; j < M; ++j)
    if (j < a.m) {
      const double s0 = nacc[(j * U + 0) * kBlock], s1 = nacc[(j * U + 1) * kBlock];
      const double s2 = nacc[(j * U + 2) * kBlock], s3 = nacc[(j * U + 3) * kBlock];
      double v = (s0 + s1) + (s2 + s3);
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
      if (lane == 0) red[threadIdx.x >> 6][j] = v;
    }
  __syncthreads();
  if (int(threadIdx.x) < a.m) {
    double s = 0;  // block_sum256's order
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) s += red[w][threadIdx.x];
    ssp::store_partial(a.partial + size_t(blockIdx.x) * a.m + threadIdx.x, s);
  }
  ssp::fold_tail<M>(a.partial, a.tail);
}

// The norm-carrying instances (NRM): the unscaled write-only form up to 8 destinations, with or without
// the epilogue.  16 destinations run 2-position windows and would need 128 KiB of LDS: not built.
constexpr int kOuterNormDst = 8;
constexpr int kPairSrc = 4;  // sources in flight per phase of k_gemm_outer_pair
unsigned outer_norm_grid(const ssp_ctx* ctx, size_t n) { return ssp::win_grid(ctx, n, ssp::kDotU, 8); }

// The instantiated width for m destinations: the M of the kernel and of its ledger tag.
int outer_inst(int m) { return m <= 1 ? 1 : m <= 2 ? 2 : m <= 4 ? 4 : m <= 8 ? 8 : 16; }

template <int M, bool DEV, bool SET, bool SC, bool EPI, bool NRM>
void launch_outer_inst(ssp_ctx* ctx, unsigned grid, const OuterArgs& a) {
  SSP_LAUNCH((k_gemm_outer<M, DEV, SET, SC, EPI, NRM>), dim3(grid), dim3(kBlock), 0, ctx->stream, a);
}

// The one dispatch over M.  NRM stops at kOuterNormDst: launch_outer has refused wider launches.
template <bool DEV, bool SET, bool SC, bool EPI = false, bool NRM = false>
void launch_outer_m(ssp_ctx* ctx, unsigned grid, const OuterArgs& a) {
  switch (outer_inst(a.m)) {
    case 1: return launch_outer_inst<1, DEV, SET, SC, EPI, NRM>(ctx, grid, a);
    case 2: return launch_outer_inst<2, DEV, SET, SC, EPI, NRM>(ctx, grid, a);
    case 4: return launch_outer_inst<4, DEV, SET, SC, EPI, NRM>(ctx, grid, a);
    case 8: return launch_outer_inst<8, DEV, SET, SC, EPI, NRM>(ctx, grid, a);
    default:
      if constexpr (!NRM) launch_outer_inst<16, DEV, SET, SC, EPI, NRM>(ctx, grid, a);
  }
}

template <bool SET, bool SC, bool EPI = false, bool NRM = false>
void launch_outer_dev(ssp_ctx* ctx, unsigned grid, const OuterArgs& a) {
  a.alpha_dev ? launch_outer_m<true, SET, SC, EPI, NRM>(ctx, grid, a)
              : launch_outer_m<false, SET, SC, EPI, NRM>(ctx, grid, a);
}

int launch_outer(ssp_ctx* ctx, const OuterArgs& a) {
  // workgroups per CU of the launch: ctx->outer_per_cu (SSP_OUTER_WG_PER_CU at context creation); the
  // norm-carrying launch: k_dot_partial's grid
  const unsigned grid = a.partial ? outer_norm_grid(ctx, a.n)
                                  : ssp::stream_grid(ctx, a.n / 2 + 1, kOuterWin, unsigned(ctx->outer_per_cu));
  if (a.partial) {  // a flushed record launched by the dot of one of its destinations
    if (!a.set || a.scale_dev || a.m > kOuterNormDst || (a.epi_mask && a.k + a.m > ssp::kOuterSrc))
      return ssp::set_error(SSP_ERR_ARG, "gemm_outer: norms on a launch that cannot carry them");
    a.epi_mask ? launch_outer_dev<true, false, true, true>(ctx, grid, a)
               : launch_outer_dev<true, false, false, true>(ctx, grid, a);
  } else if (a.epi_mask) {  // a flushed record with ssp_axpy terms: write-only, unscaled, its epilogue sources in place
    if (!a.set || a.scale_dev || a.k + a.m > ssp::kOuterSrc)
      return ssp::set_error(SSP_ERR_ARG, "gemm_outer: epilogue terms on a launch that cannot carry them");
    launch_outer_dev<true, false, true>(ctx, grid, a);
  } else if (a.scale_dev) {
    a.set ? launch_outer_dev<true, true>(ctx, grid, a) : launch_outer_dev<false, true>(ctx, grid, a);
  } else {
    a.set ? launch_outer_dev<true, false>(ctx, grid, a) : launch_outer_dev<false, false>(ctx, grid, a);
  }
  SSP_TRY_HIP(hipGetLastError());
  return SSP_OK;
}

// The arguments and the ledger tag of the launch that adds source chunk i0 (up to kOuterSrc sources) to
// destination group j0 (up to kOuterDst destinations) of the call yy[j] (+)= sum_i alphas[i * m + j] xx[i]
// (xs, ys: deferred scales, or null; set0: the destinations are not read by their first launch).  The alphas ride
// in the argument block when they fit, else in device memory; all uploads are staged, then copied by one flush.
int outer_args(ssp_ctx* ctx, const double* alphas, const double* const* xx, const double* xs, int k,
               double* const* yy, const double* ys, int m, size_t n, bool set0, int i0, int j0, OuterArgs* out,
               std::string* tag) {
  OuterArgs& a = *out;
  a = OuterArgs{};
  a.k = std::min(ssp::kOuterSrc, k - i0);
  a.m = std::min(ssp::kOuterDst, m - j0);
  a.set = (set0 && i0 == 0) ? 1 : 0;
  a.n = n;
  for (int i = 0; i < a.k; ++i) a.x[i] = xx[i0 + i];
  for (int j = 0; j < a.m; ++j) a.y[j] = yy[j0 + j];
  if (xs || ys) {
    // deferred scales: every source's; the destinations' on their first read only (i0 == 0)
    std::vector<double> scl(size_t(a.k + a.m), 1.0);
    for (int i = 0; i < a.k; ++i) scl[size_t(i)] = xs ? xs[i0 + i] : 1.0;
    for (int j = 0; j < a.m; ++j) scl[size_t(a.k + j)] = (ys && i0 == 0 && !set0) ? ys[j0 + j] : 1.0;
    if (ssp::any_scaled(scl.data(), int(scl.size()))) {
      void* ps;
      SSP_TRY(ssp::upload_small(ctx, scl.data(), scl.size() * sizeof(double), &ps));
      a.scale_dev = static_cast<const double*>(ps);
    }
  }
  const bool dev = a.k * a.m > ssp::kOuterAlpha;
  std::vector<double> block(dev ? size_t(a.k) * a.m : 0);
  double* dst = dev ? block.data() : a.alpha;
  for (int i = 0; i < a.k; ++i)
    for (int j = 0; j < a.m; ++j) dst[i * a.m + j] = alphas[size_t(i0 + i) * m + j0 + j];
  if (dev) {
    void* p;
    SSP_TRY(ssp::upload_small(ctx, block.data(), block.size() * sizeof(double), &p));
    a.alpha_dev = static_cast<const double*>(p);
  }
  SSP_TRY(ssp::flush_uploads(ctx));
  *tag = ssp::shape_tag(dev ? "dev" : "arg", outer_inst(a.m), a.set, a.k, a.m, a.scale_dev != nullptr);
  return SSP_OK;
}

// The launch of a flushed record (pending_outer.h): the write-only kernel its call would have launched,
// or with attached terms its EPI instantiation, under the call's own ledger row; each term adds one
// source stream to the row's bytes.
// norms: as the NRM instance, whose fold delivers the m sums of squares as `tail` says.
int launch_record(ssp_ctx* ctx, const ssp::PendingOuter::Record& r, const ssp::FoldTail* norms = nullptr) {
  const int e = r.terms();
  ssp::LedgerScope ls(ctx, r.set ? "gemm_outer_set" : "gemm_outer", 8.0 * r.n * (r.k + r.m + e));
  OuterArgs a;
  std::string tag;
  SSP_TRY(outer_args(ctx, r.alpha, r.x, nullptr, r.k, r.y, nullptr, r.m, r.n, true, 0, 0, &a, &tag));
  if (e > 0) {  // attach() has checked that the epilogue sources fit behind the k sources
    a.epi_mask = int(r.mask);
    for (int j = 0; j < r.m; ++j) {
      const bool on = (r.mask >> j) & 1u;
      a.x[r.k + j] = on ? r.ex[j] : nullptr;
      a.epi[j] = on ? r.ea[j] : 0.0;
    }
    tag += " epi" + std::to_string(e);
  }
  if (norms) {
    a.partial = ctx->partial;
    a.tail = *norms;
    tag += " nrm";
  }
  ls.detail(tag);
  return launch_outer(ctx, a);
}

// The launch of a pair (pending_outer.h OuterPair), always as its norm-carrying kernel: one event pair under the
// row that carries the calls' own name, two calls, the bytes of both constructions.  The register terms read
// nothing from memory, so they add no bytes.
template <int M>
void launch_pair_inst(ssp_ctx* ctx, unsigned grid, const PairArgs& a) {
  SSP_LAUNCH((k_gemm_outer_pair<M, kPairSrc>), dim3(grid), dim3(kBlock), 0, ctx->stream, a);
}

int launch_pair(ssp_ctx* ctx, const ssp::PendingOuter::Record& ra, const ssp::PendingOuter::Record& rb, unsigned mask,
                const double* e, const ssp::FoldTail& norms) {
  ssp::LedgerScope ls(ctx, rb.set ? "gemm_outer_set" : "gemm_outer", 8.0 * rb.n * (2.0 * rb.k + 2.0 * rb.m));
  ls.calls(2);
  PairArgs a{};
  a.k = rb.k;
  a.m = rb.m;
  a.n = rb.n;
  a.mask = int(mask);
  for (int i = 0; i < rb.k; ++i) {
    a.xp[i] = ra.x[i];
    a.xa[i] = rb.x[i];
  }
  int terms = 0;
  for (int j = 0; j < rb.m; ++j) {
    a.yp[j] = ra.y[j];
    a.ya[j] = rb.y[j];
    const bool on = (mask >> j) & 1u;
    a.e[j] = on ? e[j] : 0.0;
    terms += on;
  }
  void* p;
  SSP_TRY(ssp::upload_small(ctx, rb.alpha, sizeof(double) * size_t(rb.k) * size_t(rb.m), &p));
  a.alpha_dev = static_cast<const double*>(p);
  SSP_TRY(ssp::flush_uploads(ctx));
  a.partial = ctx->partial;
  a.tail = norms;
  ls.detail(ssp::shape_tag("pair", outer_inst(rb.m), 1, rb.k, rb.m, false) + " reg" + std::to_string(terms) + " nrm");
  const unsigned grid = outer_norm_grid(ctx, rb.n);
  switch (outer_inst(rb.m)) {
    case 1: launch_pair_inst<1>(ctx, grid, a); break;
    case 2: launch_pair_inst<2>(ctx, grid, a); break;
    case 4: launch_pair_inst<4>(ctx, grid, a); break;
    case 8: launch_pair_inst<8>(ctx, grid, a); break;
    default: return ssp::set_error(SSP_ERR_ARG, "gemm_outer: a pair wider than its kernel");
  }
  SSP_TRY_HIP(hipGetLastError());
  return SSP_OK;
}

// Breaks a pair (OuterPair::unpair): A is launched alone, as the single record it was, and B is left as the
// single pending record with the register terms as its epilogue terms.
int unpair_outer(ssp_ctx* ctx) {
  ssp::DeferredOuter& d = ctx->outer;
  int status = SSP_OK;
  d.pair.unpair(d.pending, [&](const ssp::PendingOuter::Record& r) { status = launch_record(ctx, r); });
  return status;
}

// The ssp_dot(y, y, n) that finds a pending record with y exactly one of its destinations, n its length and
// the norm-carrying instance built for its width: launches the record as that instance and keeps the m sums
// (one rank: their values, after one wait; ranks: the rank-local sums in norms_dev).  Else nothing happens.
int launch_outer_norms(ssp_ctx* ctx, const double* y, size_t n) {
  ssp::DeferredOuter& d = ctx->outer;
  if (!d.norms_on || !d.pending.pending()) return SSP_OK;
  // a pair: B's destinations (a dot on one of A's, or on anything else, is declined and un-pairs in flush_outer)
  const bool paired = d.pair.paired();
  const ssp::PendingOuter::Record& r = d.pending.record();
  const int m = r.m;
  if (m > kOuterNormDst || n != r.n || std::find(r.y, r.y + m, y) == r.y + m) return SSP_OK;
  d.norms.forget();
  const bool ranks = ssp::comm_attached(ctx);
  ssp::FoldTail tail{};
  int status = ssp::ensure_partial(ctx, size_t(outer_norm_grid(ctx, r.n)) * m);
  if (status == SSP_OK) status = ssp::fold_begin(ctx, m, &tail);
  if (status == SSP_OK && ranks) {
    // rank-local sums: each served dot reduces its own over the ranks, as the dot it replaces does
    if (!d.norms_dev && hipMalloc(reinterpret_cast<void**>(&d.norms_dev), ssp::kOuterDst * sizeof(double)) != hipSuccess)
      status = ssp::set_error(SSP_ERR_NOMEM, "hipMalloc of the norm staging failed");
    tail.out = d.norms_dev;
  }
  if (status != SSP_OK) {  // the record is launched as it always was, and the dot runs by itself
    const int plain = ssp::flush_outer(ctx);
    return plain != SSP_OK ? plain : status;
  }
  d.norms.keep(r.y, m, r.n);
  if (paired)
    d.pair.flush(d.pending, [&](const ssp::PendingOuter::Record& ra, const ssp::PendingOuter::Record& rb, unsigned mask,
                                const double* e) { status = launch_pair(ctx, ra, rb, mask, e, tail); });
  else
    d.pending.flush([&](const ssp::PendingOuter::Record& rec) { status = launch_record(ctx, rec, &tail); });
  if (status == SSP_OK && !ranks) {
    // one wait for all m sums, before anything else can reuse the host result buffer
    double v[ssp::kOuterDst];
    status = ssp::fold_finish(ctx, tail, v);
    if (status == SSP_OK) d.norms.set_values(v);
  }
  if (status != SSP_OK) d.norms.forget();
  return status;
}

}  // namespace

namespace ssp {

int flush_outer(ssp_ctx* ctx) {
  DeferredOuter& d = ctx->outer;
  d.norms.forget();
  if (!d.pending.pending()) return SSP_OK;
  int status = unpair_outer(ctx);  // A first, by itself; B is then the single record
  d.pending.flush([&](const PendingOuter::Record& r) {
    const int s = launch_record(ctx, r);
    if (status == SSP_OK) status = s;
  });
  return status;
}

bool outer_keeps_fill(const ssp_ctx* ctx, const void* p, size_t n) {
  const DeferredOuter& d = ctx->outer;
  return d.pair_on && d.pending.pending() && p && aligned16(p) && !d.pair.touches(d.pending, p, n);
}

int outer_take_axpy(ssp_ctx* ctx, double alpha, const double* x, double xs, double* y, double ys, size_t n,
                    bool* attached) {
  DeferredOuter& d = ctx->outer;
  *attached = false;
  d.norms.forget();  // this prologue may launch no record: y may be a vector whose norm is kept
  if (!d.pending.pending()) return SSP_OK;
  // An unscaled axpy onto exactly one destination of the pending record becomes its epilogue term; x is
  // read by that launch, so its pending zero fills are stored first.  Any other axpy launches the record.
  const bool valid = n > 0 && x && y && aligned16(x) && aligned16(y);
  if (d.pair.paired()) {
    // A's destination j onto B's destination j: a register term of the pair (no pending zero fill overlaps a
    // destination of A).  Any other axpy un-pairs and is then taken as it always was.
    if (valid && xs == 1.0 && ys == 1.0 && d.pair.attach(d.pending, alpha, x, y, n)) {
      *attached = true;
      return SSP_OK;
    }
    SSP_TRY(unpair_outer(ctx));
  }
  if (valid && xs == 1.0 && ys == 1.0 && d.pending.attach(alpha, x, y, n)) {
    *attached = true;
    return flush_fills_over(ctx, x, n);
  }
  return flush_outer(ctx);
}

int outer_serve_dot(ssp_ctx* ctx, const double* x, double xs, const double* y, double ys, size_t n, double* out,
                    bool* served) {
  DeferredOuter& d = ctx->outer;
  *served = false;
  if (!out || x != y || xs != 1.0 || ys != 1.0) return SSP_OK;
  SSP_TRY(launch_outer_norms(ctx, y, n));
  const int j = d.norms.find(y, n);
  if (j < 0) return SSP_OK;
  *served = true;
  if (!comm_attached(ctx)) {
    *out = d.norms.value(j);
    return SSP_OK;
  }
  SSP_TRY(comm_check(ctx));
  SSP_TRY(ensure_result(ctx, 1));
  SSP_TRY_HIP(hipMemcpyAsync(ctx->result_dev, d.norms_dev + j, sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  return reduce_fetch(ctx, out, 1);
}

}  // namespace ssp

namespace {
// The call would be recorded (below), and may stand as record B next to the single pending record A
// (OuterPair::may_pair): every argument check of gemm_outer_impl passes, its operands are unscaled and outside
// exact mode, and the read-modify-write form will consume the pending zero fills of all its destinations.
bool pair_candidate(ssp_ctx* ctx, const double* alphas, const double* const* xx, const double* xs, int k,
                    double* const* yy, const double* ys, int m, size_t n, bool set) {
  ssp::DeferredOuter& d = ctx->outer;
  if (!d.pair_on || !d.defer || !d.pending.pending()) return false;
  if (d.pair.paired()) {  // a third call: A is launched, and the call is weighed against B alone
    if (unpair_outer(ctx) != SSP_OK) return false;
  }
  if (!alphas || !xx || !yy || n == 0 || !ssp::PendingOuter::one_launch(k, m)) return false;
  if (ssp::any_scaled(xs, k) || ssp::exact_mode(ctx, n)) return false;
  for (int i = 0; i < k; ++i)
    if (!xx[i] || !ssp::aligned16(xx[i])) return false;
  for (int j = 0; j < m; ++j) {
    if (!yy[j] || !ssp::aligned16(yy[j])) return false;
    for (int i = 0; i < k; ++i)
      if (yy[j] == xx[i]) return false;
    if (!set && ctx->pending_fills.find_exact(yy[j], n) < 0) return false;
  }
  if (!set && ssp::any_scaled(ys, m)) return false;
  return d.pair.may_pair(d.pending, alphas, xx, k, yy, m, n, set);
}

int gemm_outer_impl(ssp_ctx* ctx, const double* alphas, const double* const* xx, const double* xs, int k,
                    double* const* yy, const double* ys, int m, size_t n, bool set) {
  if (!ctx) return ssp::set_error(SSP_ERR_ARG, "null ssp_ctx");
  SSP_TRY(ssp::use_device(ctx));
  // A call that will stand next to the pending record as the second of a pair (pair_candidate) leaves it
  // pending; every other call launches it first, as SSP_CHECK_CTX_KEEP_FILLS does.
  const bool try_pair = pair_candidate(ctx, alphas, xx, xs, k, yy, ys, m, n, set);
  if (!try_pair) SSP_TRY(ssp::flush_outer(ctx));
  if (m < 0 || k < 0) return ssp::set_error(SSP_ERR_ARG, "ssp_gemm_outer: negative dimension");
  if (set && k == 0) {
    // These zero fills may stay deferred past the return, like a caller's own ssp_fill(0): the next
    // library call stores them.  A caller that hands yy on to code of its own (the host layer's
    // data_wo() destinations reaching a user's action) relies on the rule of include/subspace_hip.h:
    // take ssp_ctx_stream or ssp_synchronize before foreign code touches the memory.
    for (int j = 0; j < m; ++j) SSP_TRY(ssp_fill(ctx, 0.0, yy[j], n));
    return SSP_OK;
  }
  if (m == 0 || n == 0) return SSP_OK;
  if (k == 0) {  // no sources: the destinations' deferred scales still have to be stored
    for (int j = 0; j < m; ++j)
      if (!set && ys && ys[j] != 1.0) SSP_TRY(ssp_scal(ctx, ys[j], yy[j], n));
    return SSP_OK;
  }
  if (!alphas) return ssp::set_error(SSP_ERR_ARG, "ssp_gemm_outer: null alphas");
  SSP_TRY(ssp::check_ptrs(xx, k, n, "ssp_gemm_outer"));
  SSP_TRY(ssp::check_ptrs(yy, m, n, "ssp_gemm_outer"));
  for (int j = 0; j < m; ++j)
    for (int i = 0; i < k; ++i)
      if (yy[j] == xx[i]) return ssp::set_error(SSP_ERR_ARG, "ssp_gemm_outer: a destination aliases a source");
  // Pending zero fills (pending_fill.h).  The sources are read: theirs are stored.  The write-only
  // form overwrites its destinations: the entries inside them are dropped.  The read-modify-write form
  // consumes: when every destination is exactly a pending entry (so they are distinct and disjoint),
  // carries no deferred scale and is outside exact mode, the entries are dropped and the first source
  // chunk of every destination group runs as the SET instantiation, whose accumulators start from the
  // +0.0 that the read-modify-write form would have loaded -- the same bits without writing the zeros
  // and reading them back.  All or nothing: otherwise every entry a destination touches is stored and
  // the call runs as it always did.  Entries no operand touches stay pending.
  bool consume = false;
  if (!ctx->pending_fills.empty()) {
    for (int i = 0; i < k; ++i) SSP_TRY(ssp::flush_fills_over(ctx, xx[i], n));
    if (set) {
      for (int j = 0; j < m; ++j) SSP_TRY(ssp::overwrite_fills(ctx, yy[j], n));
    } else {
      consume = !ssp::any_scaled(ys, m) && !ssp::exact_mode(ctx, n);
      for (int j = 0; consume && j < m; ++j) {
        consume = ctx->pending_fills.find_exact(yy[j], n) >= 0;
        for (int i = 0; consume && i < j; ++i) consume = yy[i] != yy[j];
      }
      for (int j = 0; j < m; ++j) {
        if (consume) ctx->pending_fills.erase(ctx->pending_fills.find_exact(yy[j], n));
        else SSP_TRY(ssp::flush_fills_over(ctx, yy[j], n));
      }
    }
  }
  const bool set0 = set || consume;  // the destinations are not read by their first launch
  // Deferred gemm_outer (pending_outer.h): the unscaled write-only form of one launch is recorded, not
  // launched, so that the ssp_axpy calls that follow on its destinations ride on its stores; whatever
  // else comes next launches it first (ssp::flush_outer, under this call's ledger row).  Everything
  // above has happened as for the launch, so no pending zero fill overlaps an operand of the record.
  if (try_pair) {
    if (set0 && ctx->outer.pair.pair(ctx->outer.pending, alphas, xx, k, yy, m, n, set)) return SSP_OK;
    SSP_TRY(ssp::flush_outer(ctx));  // pair_candidate has checked all of it: not reached
  }
  if (ctx->outer.defer && set0 && !ssp::any_scaled(xs, k) && !ssp::exact_mode(ctx, n) &&
      ctx->outer.pending.record(alphas, xx, k, yy, m, n, set))
    return SSP_OK;
  // Destinations are independent; sources are applied in increasing order, in groups that fit
  // the kernel argument block, so each destination sees the reference's summation order.
  ssp::LedgerScope ls(ctx, set ? "gemm_outer_set" : "gemm_outer", 8.0 * n * (k + (set0 ? 1.0 : 2.0) * m));
  if (ssp::exact_mode(ctx, n)) return ssp::exact_outer(ctx, alphas, xx, xs, k, yy, ys, m, n, set);
  // Up to kOuterSrc sources per launch, so every destination is read and written once per kOuterSrc sources.
  for (int j0 = 0; j0 < m; j0 += ssp::kOuterDst)
    for (int i0 = 0; i0 < k; i0 += ssp::kOuterSrc) {
      OuterArgs a;
      std::string tag;
      SSP_TRY(outer_args(ctx, alphas, xx, xs, k, yy, ys, m, n, set0, i0, j0, &a, &tag));
      if (j0 == 0 && i0 == 0) ls.detail(tag);
      SSP_TRY(launch_outer(ctx, a));
    }
  return SSP_OK;
}
}  // namespace

extern "C" {

int ssp_gemm_outer(ssp_ctx* ctx, const double* alphas, const double* const* xx, int k, double* const* yy, int m,
                   size_t n) {
  return gemm_outer_impl(ctx, alphas, xx, nullptr, k, yy, nullptr, m, n, false);
}

int ssp_gemm_outer_set(ssp_ctx* ctx, const double* alphas, const double* const* xx, int k, double* const* yy, int m,
                       size_t n) {
  return gemm_outer_impl(ctx, alphas, xx, nullptr, k, yy, nullptr, m, n, true);
}

int ssp_gemm_outer_scaled(ssp_ctx* ctx, const double* alphas, const double* const* xx, const double* xs, int k,
                          double* const* yy, const double* ys, int m, size_t n) {
  return gemm_outer_impl(ctx, alphas, xx, xs, k, yy, ys, m, n, false);
}

int ssp_gemm_outer_set_scaled(ssp_ctx* ctx, const double* alphas, const double* const* xx, const double* xs, int k,
                              double* const* yy, int m, size_t n) {
  return gemm_outer_impl(ctx, alphas, xx, xs, k, yy, nullptr, m, n, true);
}

}  // extern "C"
