// Mixed-precision kernels: vectors stored in binary32, arithmetic in FP64 (include/subspace_hip.h
// "mixed precision").  An f32 operand is widened as it is loaded, the f64 result rounded once
// (nearest-even, v_cvt_f32_f64) where the destination is f32; every fma chain is the f64 kernel's.
//
// Layout.  The unit of every kernel here is the QUAD, 4 consecutive elements owned by one lane: an f32
// quad is one 16-byte access (a wave instruction covers 1 KiB contiguous), an f64 quad two 16-byte
// accesses 16 bytes apart (the pair of wave instructions covers 2 KiB contiguous, each whole 128-byte
// line consumed by the two back to back).  Lane l of a window owns quad p0 + l, so an f32 source and
// an f64 destination of the same elements meet in one lane with no cross-lane traffic.
//   gemm_outer  bytes = N (sx k + (1 or 2) sy m)      gemm_inner  bytes = N (sx m + sy k)
// with sx, sy the storage sizes: 48 f32 sources into 8 f64 destinations move 320 N bytes where the f64
// kernel moves 512 N.
//
// Kernels.  k_mx_copy, k_mx_axpy, k_mx_scal, k_mx_dot: one per-element operation each, over map_quads;
// k_mx_rhs_residual_norms<TB, K> (y_j = s_j (ys_j y_j - b_j) with b stored as TB, and <y_j, y_j>, up to 16 pairs per launch);
// k_quantise_f32 (f64 vectors rounded through f32 in place, up to 16 per launch); k_mx_fill; k_mx_outer<TX, TY, M, SET, TWIN> (gemm_outer, launched chunk by chunk from outer_chunks, also the
// dense pass of the ssp_q32_* updates; TWIN: ssp_q32_combine_widen's second store of every result, widened); k_mx_inner<TX, CP, MG, NG> (gemm_inner: the one MFMA tile kernel,
// CP the columns' storage -- float, double, or ByGroup for ssp_q32_gemm_inner_cols); k_q32_store_diff and
// k_q32_anchor_combine (a DIIS history stored as f32 differences behind f64 anchors: for_quads' windows, and
// k_mx_outer's window with one destination that starts from its anchor).  with_pair maps the
// storage pair of a call to the kernel's types.
#include <algorithm>
#include <cstddef>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

#include "mfma_tile.h"
#include "mx_cols_plan.h"
#include "ssp_internal.h"

namespace {

using ssp::kBlock;

typedef float nt_float4 __attribute__((ext_vector_type(4)));
typedef double nt_double2 __attribute__((ext_vector_type(2)));

// One quad as loaded (f32: 4 VGPRs, f64: 8), widened where it is used.
template <typename T>
struct Raw;
template <>
struct Raw<float> {
  nt_float4 a;
  __device__ __forceinline__ double get(int e) const { return double(a[e]); }
};
template <>
struct Raw<double> {
  nt_double2 a, b;
  __device__ __forceinline__ double get(int e) const { return e < 2 ? a[e] : b[e - 2]; }
};

template <typename T>
__device__ __forceinline__ Raw<T> zero_quad() {
  Raw<T> r;
  if constexpr (sizeof(T) == 4) r.a = nt_float4{0.f, 0.f, 0.f, 0.f};
  else {
    r.a = nt_double2{0., 0.};
    r.b = nt_double2{0., 0.};
  }
  return r;
}

// p: the quad's first element (16-byte aligned for f32, 32 for f64).  NT: nontemporal (streamed once).
template <bool NT, typename T>
__device__ __forceinline__ Raw<T> ldq(const T* p) {
  Raw<T> r;
  if constexpr (sizeof(T) == 4) {
    const nt_float4* q = reinterpret_cast<const nt_float4*>(p);
    r.a = NT ? __builtin_nontemporal_load(q) : *q;
  } else {
    const nt_double2* q = reinterpret_cast<const nt_double2*>(p);
    r.a = NT ? __builtin_nontemporal_load(q) : q[0];
    r.b = NT ? __builtin_nontemporal_load(q + 1) : q[1];
  }
  return r;
}

// Stores 4 f64 results, rounded to T.
template <bool NT, typename T>
__device__ __forceinline__ void stq(T* p, const double (&v)[4]) {
  if constexpr (sizeof(T) == 4) {
    const nt_float4 w = {float(v[0]), float(v[1]), float(v[2]), float(v[3])};
    nt_float4* q = reinterpret_cast<nt_float4*>(p);
    if (NT) __builtin_nontemporal_store(w, q);
    else *q = w;
  } else {
    const nt_double2 w0 = {v[0], v[1]}, w1 = {v[2], v[3]};
    nt_double2* q = reinterpret_cast<nt_double2*>(p);
    if (NT) {
      __builtin_nontemporal_store(w0, q);
      __builtin_nontemporal_store(w1, q + 1);
    } else {
      q[0] = w0;
      q[1] = w1;
    }
  }
}

// Window shape over quads (ssp::for_windows over double2 positions): a wave covers U x 64 consecutive
// quads of each vector per visit, then the quads past the last whole window (thread-granular), then
// the n mod 4 last elements (one thread of workgroup 0 each).  fw(p0): the lane's first quad of a
// window (its others are p0 + 64 u); f(p): one quad; fe(e): one element.
template <int U, typename FW, typename F, typename FE>
__device__ __forceinline__ void for_quads(size_t n, FW&& fw, F&& f, FE&& fe) {
  const int lane = threadIdx.x & 63;
  const size_t gw = size_t(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
  const size_t nw = size_t(gridDim.x) * (kBlock / 64);
  const size_t n4 = n >> 2, win = 64 * size_t(U), nwin = n4 / win;
  for (size_t c = gw; c < nwin; c += nw) fw(c * win + lane);
  for (size_t i = nwin * win + size_t(blockIdx.x) * kBlock + threadIdx.x; i < n4; i += size_t(gridDim.x) * kBlock) f(i);
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) fe(4 * n4 + threadIdx.x);
}

// The lane's U quads pos[u] of one vector, as loaded.
template <typename T, int U>
struct Win {
  Raw<T> q[U];
};
template <bool NT, typename T, int U>
__device__ __forceinline__ Win<T, U> ldwin(const T* p, const size_t (&pos)[U]) {
  Win<T, U> w;
#pragma unroll
  for (int u = 0; u < U; ++u) w.q[u] = ldq<NT>(p + 4 * pos[u]);
  return w;
}

unsigned quad_grid(const ssp_ctx* ctx, size_t n, int u, unsigned per_cu) {
  return ssp::stream_grid(ctx, ((n >> 2) / (64 * size_t(u)) + 1) * 64, 1, per_cu);
}

constexpr int kMxU = 4;  // 4 KiB of an f32 vector, 8 KiB of an f64 one, per wave visit

// One operation over the lane's U quads p0 + 64 u of every operand, written once:
// f(e, in0, in1, ...) gets element e of the quad of every input, widened, and returns the f64 value stored
// (rounded) to `out`; with out = nullptr nothing is stored and f only accumulates.  Every load of a visit
// is issued, operand by operand, before the first f, then come the stores.  NT: nontemporal accesses.
template <int U, bool NT, typename O, typename F, typename... TI>
__device__ __forceinline__ void map_quads_at(size_t p0, O out, F& f, const TI*... in) {
  size_t pos[U];  // formed once for every operand: each vector's addresses then share them, as written by hand
#pragma unroll
  for (int u = 0; u < U; ++u) pos[u] = p0 + 64 * u;
  const auto apply = [&](const auto&... v) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      double w[4];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if constexpr (std::is_null_pointer_v<O>) f(e, v.q[u].get(e)...);
        else w[e] = f(e, v.q[u].get(e)...);
      if constexpr (!std::is_null_pointer_v<O>) stq<NT>(out + 4 * pos[u], w);
    }
  };
  apply(ldwin<NT>(in, pos)...);
}

// for_quads<kMxU> with the one per-element operation f: the window form (nontemporal), the single quad
// (plain accesses) and the n mod 4 last elements, which f sees as element 0 of a quad.
template <typename O, typename F, typename... TI>
__device__ __forceinline__ void map_quads(size_t n, O out, F f, const TI*... in) {
  for_quads<kMxU>(
      n, [&](size_t p0) { map_quads_at<kMxU, true>(p0, out, f, in...); },
      [&](size_t p) { map_quads_at<1, false>(p, out, f, in...); },
      [&](size_t i) {
        if constexpr (std::is_null_pointer_v<O>) f(0, double(in[i])...);
        else out[i] = std::remove_pointer_t<O>(f(0, double(in[i])...));
      });
}

// x = (TX)(ys * y)
template <typename TX, typename TY>
__global__ __launch_bounds__(kBlock) void k_mx_copy(TX* __restrict__ x, const TY* __restrict__ y, size_t n, double ys) {
  map_quads(n, x, [=](int, double v) { return v * ys; }, y);
}

// y = (TY)fma(alpha, x, y): the single fma of k_axpy.
template <typename TX, typename TY>
__global__ __launch_bounds__(kBlock) void k_mx_axpy(const TX* __restrict__ x, TY* __restrict__ y, size_t n, double alpha) {
  map_quads(n, y, [=](int, double xv, double yv) { return fma(alpha, xv, yv); }, x, static_cast<const TY*>(y));
}

// x = (float)(alpha * x).  Not k_mx_copy<float, float> in place: both of that kernel's pointers are restrict.
__global__ __launch_bounds__(kBlock) void k_mx_scal(float* __restrict__ x, size_t n, double alpha) {
  map_quads(n, x, [=](int, double v) { return v * alpha; }, static_cast<const float*>(x));
}

// x = (float)alpha: the stride shape of k_fill, one quad per lane and trip.
__global__ __launch_bounds__(kBlock) void k_mx_fill(float* __restrict__ x, size_t n, double alpha) {
  const size_t n4 = n >> 2, stride = size_t(gridDim.x) * kBlock;
  const double w[4] = {alpha, alpha, alpha, alpha};
  for (size_t i = size_t(blockIdx.x) * kBlock + threadIdx.x; i < n4; i += stride) stq<false>(x + 4 * i, w);
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) x[4 * n4 + threadIdx.x] = float(alpha);
}

// <x, y>: the shape of k_dot_partial (4 accumulators per lane, quad e into accumulator e; one partial
// per workgroup, folded in fixed order by the last workgroup to arrive).
template <typename TX, typename TY>
__global__ __launch_bounds__(kBlock) void k_mx_dot(const TX* __restrict__ x, const TY* __restrict__ y, size_t n,
                                                   double* __restrict__ partial, const ssp::FoldTail tail) {
  double acc[4] = {0, 0, 0, 0};
  map_quads(n, nullptr, [&](int e, double xv, double yv) { acc[e] = fma(xv, yv, acc[e]); }, x, y);
  const double s = ssp::block_sum256((acc[0] + acc[1]) + (acc[2] + acc[3]));
  if (threadIdx.x == 0) ssp::store_partial(partial + blockIdx.x, s);
  ssp::fold_tail(partial, tail);
}

// ---- residuals against a right-hand side, and their norms ---------------------------------------------
struct RhsResidualArgs {
  const void* b[ssp::kOuterDst];
  double* y[ssp::kOuterDst];
  double s[ssp::kOuterDst];
  double ys[ssp::kOuterDst];
  int m;
  size_t n;
  double* partial;     // [gridDim.x][m]; null: the residuals only (the exact path forms the norms itself)
  ssp::FoldTail tail;  // the fused fold (with partial)
};

// One element: y * ys (the rounding an eager scal stores), the subtraction rounded once -- what
// fma(-1, b, y) gives, its product being exact -- then the product with s rounded once.  No contraction.
__device__ __forceinline__ double rhs_residual(double yv, double ys, double bv, double s) {
#pragma clang fp contract(off)
  return (yv * ys - bv) * s;
}

// The lane's U quads p0 + 64 u of one pair: the quads of b (as stored) and of y are all in flight before the
// first result is formed; acc takes the lane's squares in element order.
template <int U, bool NT, typename TB>
__device__ __forceinline__ void rhs_residual_at(const TB* b, double* y, double s, double ys, size_t p0, double& acc) {
  Raw<TB> bv[U];
  Raw<double> yv[U];
#pragma unroll
  for (int u = 0; u < U; ++u) bv[u] = ldq<NT>(b + 4 * (p0 + 64 * u));
#pragma unroll
  for (int u = 0; u < U; ++u) yv[u] = ldq<NT>(static_cast<const double*>(y) + 4 * (p0 + 64 * u));
#pragma unroll
  for (int u = 0; u < U; ++u) {
    double w[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      w[e] = rhs_residual(yv[u].get(e), ys, bv[u].get(e), s);
      acc = fma(w[e], w[e], acc);
    }
    stq<NT>(y + 4 * (p0 + 64 * u), w);
  }
}

// y_j = s_j (ys_j y_j - (double)b_j) and the per-workgroup partials of <y_j, y_j>, j < m, in one launch: the
// workgroup takes the pairs one after the other, each over the windows of for_quads (the f32 and f64 elements of
// a position meet in one lane; 4 KiB of an f32 b and 8 KiB of y in flight per wave visit), with one accumulator
// per lane -- the register footprint of one pair whatever m is (all m pairs per window visit, the shape of
// k_axpy_pairs_norm, takes the 255 registers and spills from m = 16 with an f64 quad per operand).  The pair's
// pointers and scales are wave-uniform reads through the constant address space.  The last workgroup to arrive
// folds the partials in fixed order (K: outputs per trip of the fold).
template <typename TB, int K>
__global__ __launch_bounds__(kBlock) void k_mx_rhs_residual_norms(const RhsResidualArgs a) {
  using cchar = const __attribute__((address_space(4))) char;
  using cdouble = const __attribute__((address_space(4))) double;
  typedef const void* cvoidp;
  typedef double* doublep;
  cchar* const karg = (cchar*)__builtin_amdgcn_kernarg_segment_ptr();
  __shared__ double red[kBlock / 64][ssp::kOuterDst];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll 1
  for (int j = 0; j < a.m; ++j) {
    const TB* const b = static_cast<const TB*>(((const __attribute__((address_space(4))) cvoidp*)(karg + offsetof(RhsResidualArgs, b)))[j]);
    double* const y = ((const __attribute__((address_space(4))) doublep*)(karg + offsetof(RhsResidualArgs, y)))[j];
    const double s = ((cdouble*)(karg + offsetof(RhsResidualArgs, s)))[j];
    const double ys = ((cdouble*)(karg + offsetof(RhsResidualArgs, ys)))[j];
    double acc = 0;
    for_quads<kMxU>(
        a.n, [&](size_t p0) { rhs_residual_at<kMxU, true>(b, y, s, ys, p0, acc); },
        [&](size_t p) { rhs_residual_at<1, false>(b, y, s, ys, p, acc); },
        [&](size_t i) {
          const double w = rhs_residual(y[i], ys, double(b[i]), s);
          y[i] = w;
          acc = fma(w, w, acc);
        });
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0) red[wave][j] = acc;
  }
  if (!a.partial) return;
  // per-workgroup sums into partial[block][m] (kernels_panel.hip block_partials), then the fused fold
  __syncthreads();
  if (int(threadIdx.x) < a.m) {
    double t = red[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kBlock / 64; ++w) t += red[w][threadIdx.x];
    ssp::store_partial(a.partial + size_t(blockIdx.x) * a.m + threadIdx.x, t);
  }
  ssp::fold_tail<K>(a.partial, a.tail);
}

// ---- quantise -------------------------------------------------------------------------------------
struct QuantArgs {
  double* x[ssp::kPrecVec];
  double s[ssp::kPrecVec];
  size_t n;
};

// x[v] = (double)(float)(x[v] * s[v]) in place, vector blockIdx.y: the value k_mx_copy<float, double> with
// ys = s[v] would store, widened again, so the later narrowing copy of the result is exact.  The same kernel
// at every length (a rounding has no summation order to keep).
__global__ __launch_bounds__(kBlock) void k_quantise_f32(const QuantArgs a) {
  double* const x = a.x[blockIdx.y];
  const double s = a.s[blockIdx.y];
  map_quads(a.n, x, [=](int, double v) { return double(float(v * s)); }, static_cast<const double*>(x));
}

// ---- gemm_outer -----------------------------------------------------------------------------------
struct MxOuterArgs {
  const void* x[ssp::kOuterSrc];
  void* y[ssp::kOuterDst];
  double* w[ssp::kOuterDst];  // TWIN only: the f64 twins of the f32 destinations
  int k;
  int m;
  size_t n;
  const double* alpha_dev;         // k*m > kOuterAlpha: alpha[i*m + j] in device memory
  const double* scale_dev;         // source scales [0, k) in device memory, or null (all 1)
  const double* yscale_dev;        // destination scales [0, m) in device memory, or null (all 1); not with SET
  double alpha[ssp::kOuterAlpha];  // alpha[i*m + j] in the argument block
};
static_assert(sizeof(MxOuterArgs) <= 4000, "kernel argument block too large");

// yy[j] (+)= sum_i alpha(i,j) (s_i xx[i]), the shape of k_gemm_outer: each wave owns windows of U x 64
// quads, loads a batch of sources x U quads before the fmas (8 f32 or 4 f64 sources: the same 256
// bytes per lane in flight), and adds the sources of every destination in order i = 0..k-1.  The
// accumulators are the widened destinations (U x M x 4 doubles per lane); an f32 destination is rounded
// once, as it is stored.  Alphas and scales are wave-uniform reads through the constant address space.
// A destination's scale (the launch of a call's first source chunk only) is applied as the destination
// is loaded, acc = y * ys[j]: the rounding an eager scal stores, as k_gemm_outer's SC form does.
// TWIN (f32 destinations; ssp_q32_combine_widen, the launch of a call's last source chunk only): each
// accumulator is stored twice, rounded to y[j] and that rounded value widened to w[j] -- the f64 quad's two
// 16-byte stores beside the f32 quad's one, what k_mx_copy<double, float> would store from y[j] read back.
template <typename TX, typename TY, int M, bool SET, bool TWIN = false>
__global__ __launch_bounds__(kBlock) void k_mx_outer(const MxOuterArgs a) {
  static_assert(!TWIN || sizeof(TY) == 4, "a twin belongs to an f32 destination");
  using cdouble = const __attribute__((address_space(4))) double;
  using cchar = const __attribute__((address_space(4))) char;
  cdouble* const alpha = a.alpha_dev ? (cdouble*)a.alpha_dev
                                     : (cdouble*)((cchar*)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(MxOuterArgs, alpha));
  cdouble* const scale_p = (cdouble*)a.scale_dev;
  const auto scale = [&](int i) { return scale_p ? scale_p[i] : 1.0; };
  cdouble* const yscale_p = SET ? nullptr : (cdouble*)a.yscale_dev;
  constexpr int U = M > 8 ? 1 : 2;
  constexpr int B = sizeof(TX) == 4 ? 8 : 4;
  const int lane = threadIdx.x & 63;
  const size_t gw = size_t(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
  const size_t nw = size_t(gridDim.x) * (kBlock / 64);
  const size_t n4 = a.n >> 2, win = 64 * U;
  for (size_t c = gw; c * win < n4; c += nw) {
    const size_t p0 = c * win + lane;
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) ok[u] = p0 + 64 * u < n4;
    double acc[U][M][4];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < M; ++j) {
        const Raw<TY> r = (j < a.m && ok[u] && !SET) ? ldq<true>(static_cast<const TY*>(a.y[j]) + 4 * (p0 + 64 * u))
                                                     : zero_quad<TY>();
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[u][j][e] = r.get(e);
      }
    if (yscale_p) {
#pragma unroll
      for (int j = 0; j < M; ++j)
        if (j < a.m) {
          const double ys = yscale_p[j];
#pragma unroll
          for (int u = 0; u < U; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[u][j][e] *= ys;
        }
    }
    const auto add = [&](int i, const Raw<TX>(&xv)[U]) {
      const double s = scale(i);
      double xw[U][4];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) xw[u][e] = xv[u].get(e) * s;
#pragma unroll
      for (int j = 0; j < M; ++j) {
        if (j < a.m) {
          const double al = alpha[i * a.m + j];
#pragma unroll
          for (int u = 0; u < U; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[u][j][e] = fma(al, xw[u][e], acc[u][j][e]);
        }
      }
    };
    int i = 0;
    for (; i + B <= a.k; i += B) {
      Raw<TX> xv[B][U];
#pragma unroll
      for (int b = 0; b < B; ++b)
#pragma unroll
        for (int u = 0; u < U; ++u)
          xv[b][u] = ok[u] ? ldq<true>(static_cast<const TX*>(a.x[i + b]) + 4 * (p0 + 64 * u)) : zero_quad<TX>();
#pragma unroll
      for (int b = 0; b < B; ++b) add(i + b, xv[b]);
    }
    for (; i < a.k; ++i) {
      Raw<TX> xv[U];
#pragma unroll
      for (int u = 0; u < U; ++u)
        xv[u] = ok[u] ? ldq<true>(static_cast<const TX*>(a.x[i]) + 4 * (p0 + 64 * u)) : zero_quad<TX>();
      add(i, xv);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (ok[u])
#pragma unroll
        for (int j = 0; j < M; ++j)
          if (j < a.m) {
            stq<true>(static_cast<TY*>(a.y[j]) + 4 * (p0 + 64 * u), acc[u][j]);
            if constexpr (TWIN) {
              const double r[4] = {double(float(acc[u][j][0])), double(float(acc[u][j][1])), double(float(acc[u][j][2])),
                                   double(float(acc[u][j][3]))};
              stq<true>(a.w[j] + 4 * (p0 + 64 * u), r);
            }
          }
  }
  // the n mod 4 last elements: thread j of workgroup 0 owns destination j
  if ((a.n & 3) && blockIdx.x == 0 && int(threadIdx.x) < a.m) {
    const int j = threadIdx.x;
    TY* y = static_cast<TY*>(a.y[j]);
    for (size_t e = 4 * n4; e < a.n; ++e) {
      double v = SET ? 0.0 : double(y[e]);
      if (yscale_p) v *= yscale_p[j];
      for (int i = 0; i < a.k; ++i) v = fma(alpha[i * a.m + j], double(static_cast<const TX*>(a.x[i])[e]) * scale(i), v);
      y[e] = TY(v);
      if constexpr (TWIN) a.w[j][e] = double(TY(v));
    }
  }
}

// ---- gemm_inner -----------------------------------------------------------------------------------
struct MxInnerArgs {
  const void* x[ssp::kInnerRows];  // rows: MG groups of 4
  const void* y[ssp::kInnerCols];  // columns: NG groups of 4; ByGroup: the first g64 groups f64, the others f32, and
                                   // a null one is a padding slot (never the first of its group)
  double xs[ssp::kInnerRows];
  double ys[ssp::kInnerCols];
  int m;
  int k;    // ByGroup: slots, a multiple of 4
  int g64;  // ByGroup only
  size_t n;
  double* partial;  // [gridDim.x][m][k]
};
static_assert(sizeof(MxInnerArgs) <= 4000, "kernel argument block too large");

// Storage policies of k_mx_inner: the quads of a chunk's NG column groups (with T = TX, MG row groups) as
// loaded.  load(h, ...): the
// nontemporal load of group h's quad, or zeros for a whole absent group (`present` is wave-uniform, so the
// branch skips the load and no load carries an exec-mask guard); get(h, q): element q of that quad, widened;
// elem(h, g64, p, i): element i of column p of group h, widened, for the remainder loop.
// Every column stored as T:
template <typename T, int NG>
struct TileQuads {
  Raw<T> v[NG];
  __device__ __forceinline__ explicit TileQuads(int) {}
  __device__ __forceinline__ void load(int h, bool present, const void* p, size_t e0) {
    v[h] = present ? ldq<true>(static_cast<const T*>(p) + e0) : zero_quad<T>();
  }
  __device__ __forceinline__ double get(int h, int q) const { return v[h].get(q); }
  __device__ __forceinline__ static double elem(int, int, const void* p, size_t i) { return double(static_cast<const T*>(p)[i]); }
};

// Either, by group (mx_cols_plan.h): group h is f64 when h < g64, a wave-uniform branch, so one launch reads
// its rows once for the columns of both types.  Lanes of a padding slot read their group's first column;
// what they accumulate is stored with the rest (the layout of the partials depends on the slots only) and
// dropped by the host.
// Registers: every group's quad has 16 bytes in lo[h] (an f32 quad, or the first half of an f64 one) and the
// 16 more of hi[h]: any group may be f64 (H64 = NG).  A lean form (H64 = 4: the 16 f64 columns of a subspace
// update, later groups f32 statically, the register footprint of k_mx_inner<double, float>) measured no
// faster on the tile of 16 f64 + 48 f32 columns at N = 1.25e7 and 1e8 (profiles/r8/q32_fused.md), so it is
// not instantiated.
struct ByGroup {};
template <int NG>
struct TileQuads<ByGroup, NG> {
  nt_float4 lo[NG];
  nt_double2 hi[NG];
  const int g64;
  __device__ __forceinline__ explicit TileQuads(int g) : g64(g) {}
  __device__ __forceinline__ void load(int h, bool present, const void* p, size_t e0) {
    lo[h] = nt_float4{0.f, 0.f, 0.f, 0.f};
    hi[h] = nt_double2{0., 0.};
    if (present) {
      if (h < g64) {
        const Raw<double> v = ldq<true>(static_cast<const double*>(p) + e0);
        lo[h] = __builtin_bit_cast(nt_float4, v.a);
        hi[h] = v.b;
      } else {
        lo[h] = ldq<true>(static_cast<const float*>(p) + e0).a;
      }
    }
  }
  __device__ __forceinline__ double get(int h, int q) const {
    double v = double(lo[h][q]);
    if (h < g64) v = q < 2 ? __builtin_bit_cast(nt_double2, lo[h])[q] : hi[h][q - 2];
    return v;
  }
  __device__ __forceinline__ static double elem(int h, int g64, const void* p, size_t i) {
    return h < g64 ? static_cast<const double*>(p)[i] : double(static_cast<const float*>(p)[i]);
  }
};

// The f64 MFMA tile of k_gemm_inner (mfma_tile.h) over chunks of 64 elements, rows stored as TX, columns by
// the policy CP (float, double or ByGroup): the 16 lanes that hold one vector (same l & 3) each load the quad
// p = l >> 2 of the chunk -- 256 contiguous bytes of an f32 vector per load instruction, 512 of an f64 one
// per pair -- and the quad's four elements feed four MFMAs (one per element; the tiles of one element are
// independent, so no MFMA waits for the one before it; each accumulator sees the elements in increasing
// order).  Operands are widened and scaled (v * s, the rounding an eager scal stores) after every load of
// the chunk, rows then columns, is in flight.  Whole absent groups skip their loads by a wave-uniform branch.
template <typename TX, typename CP, int MG, int NG>
__global__ __launch_bounds__(kBlock) void k_mx_inner(const MxInnerArgs a) {
  static_assert(4 * MG <= ssp::kInnerRows && 4 * NG <= ssp::kInnerCols, "tile_lane reads 4 entries per group");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 3, p = lane >> 2;
  ssp::TileLane x[MG], y[NG];
#pragma unroll
  for (int g = 0; g < MG; ++g) x[g] = ssp::tile_lane(a.x, a.xs, a.m, g, r);
#pragma unroll
  for (int h = 0; h < NG; ++h) y[h] = ssp::tile_lane(a.y, a.ys, a.k, h, r);
  double acc[MG][NG];
#pragma unroll
  for (int g = 0; g < MG; ++g)
#pragma unroll
    for (int h = 0; h < NG; ++h) acc[g][h] = 0;
  const auto mac = [&](const double (&xw)[MG], const double (&yw)[NG]) {
#pragma unroll
    for (int g = 0; g < MG; ++g)
#pragma unroll
      for (int h = 0; h < NG; ++h) acc[g][h] = __builtin_amdgcn_mfma_f64_4x4x4f64(xw[g], yw[h], acc[g][h], 0, 0, 0);
  };

  const size_t gw = size_t(__builtin_amdgcn_readfirstlane(int(blockIdx.x * (kBlock / 64) + wave)));
  const size_t nw = size_t(gridDim.x) * (kBlock / 64);
  const size_t nchunks = a.n / 64;
  for (size_t ch = gw; ch < nchunks; ch += nw) {
    const size_t e0 = ch * 64 + 4 * size_t(p);
    TileQuads<TX, MG> xv(0);
    TileQuads<CP, NG> yv(a.g64);
#pragma unroll
    for (int g = 0; g < MG; ++g) xv.load(g, 4 * g < a.m, x[g].p, e0);
#pragma unroll
    for (int h = 0; h < NG; ++h) yv.load(h, 4 * h < a.k, y[h].p, e0);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      double xw[MG], yw[NG];
#pragma unroll
      for (int g = 0; g < MG; ++g) xw[g] = xv.get(g, q) * x[g].s;
#pragma unroll
      for (int h = 0; h < NG; ++h) yw[h] = yv.get(h, q) * y[h].s;
      mac(xw, yw);
    }
  }
  // Remainder [64 nchunks, n): guarded element loads, zeros past n.
  for (size_t s = nchunks * 64 + gw * 64; s < a.n; s += nw * 64) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const size_t i = s + 4 * size_t(p) + q;
      double xw[MG], yw[NG];
#pragma unroll
      for (int g = 0; g < MG; ++g) xw[g] = (x[g].ok && i < a.n) ? double(static_cast<const TX*>(x[g].p)[i]) * x[g].s : 0.0;
#pragma unroll
      for (int h = 0; h < NG; ++h) yw[h] = (y[h].ok && i < a.n) ? TileQuads<CP, NG>::elem(h, a.g64, y[h].p, i) * y[h].s : 0.0;
      mac(xw, yw);
    }
  }
  ssp::tile_store_partials<MG, NG>(acc, a.m, a.k, a.partial);
}

// ---- a DIIS history stored as differences (ssp_q32_store_differences, ssp_q32_anchor_combine) ------
struct StoreDiffArgs {
  const double* v[ssp::kPrecVec];
  double* a[ssp::kPrecVec];
  float* d[ssp::kPrecVec];
  size_t n;
};

// The lane's U quads p0 + 64 u of one vector: the quads of v and of a are all in flight before the first
// difference is formed; d takes (float)(v - a), the subtraction rounded once, and a takes v.
template <int U, bool NT>
__device__ __forceinline__ void store_diff_at(const double* v, double* a, float* d, size_t p0) {
  Raw<double> vv[U], av[U];
#pragma unroll
  for (int u = 0; u < U; ++u) vv[u] = ldq<NT>(v + 4 * (p0 + 64 * u));
#pragma unroll
  for (int u = 0; u < U; ++u) av[u] = ldq<NT>(static_cast<const double*>(a) + 4 * (p0 + 64 * u));
#pragma unroll
  for (int u = 0; u < U; ++u) {
    double x[4], w[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      x[e] = vv[u].get(e);
      w[e] = x[e] - av[u].get(e);
    }
    stq<NT>(d + 4 * (p0 + 64 * u), w);
    stq<NT>(a + 4 * (p0 + 64 * u), x);
  }
}

// d[j] = (float)(v[j] - a[j]), then a[j] = v[j], vector j = blockIdx.y, over the windows of for_quads (the f32
// and f64 elements of a position meet in one lane): 8 + 8 bytes read and 4 + 8 written per element.  The same
// kernel at every length: each element is one subtraction and one narrowing, whatever arithmetic forms it.
__global__ __launch_bounds__(kBlock) void k_q32_store_diff(const StoreDiffArgs a) {
  const double* const v = a.v[blockIdx.y];
  double* const an = a.a[blockIdx.y];
  float* const d = a.d[blockIdx.y];
  for_quads<kMxU>(
      a.n, [&](size_t p0) { store_diff_at<kMxU, true>(v, an, d, p0); },
      [&](size_t p) { store_diff_at<1, false>(v, an, d, p); },
      [&](size_t i) {
        const double x = v[i];
        d[i] = float(x - an[i]);
        an[i] = x;
      });
}

constexpr int kAnchorPanels = 2;  // panels per ssp_q32_anchor_combine launch: the parameters and the residuals
struct AnchorCombineArgs {
  const double* a[kAnchorPanels];  // what a panel starts from: its anchor, or y itself from the second source chunk on
  double* y[kAnchorPanels];
  const float* d[kAnchorPanels][ssp::kOuterSrc];
  double g[ssp::kOuterSrc];  // -gamma_i
  int k;
  size_t n;
};

// y_j = a_j - sum_i gamma_i (double)d_j,i for panel j = blockIdx.y: k_mx_outer's window (2 x 64 quads per wave,
// batches of 8 f32 sources in flight before their fmas) with one destination, whose accumulator starts from the
// anchor instead of the destination: acc = a, then acc = fma(-gamma_i, d_i, acc) for i = 0..k-1 -- the chain of
// k_mx_outer<float, double, 1, false> on a copy of a, element for element.  Coefficients and source pointers
// are wave-uniform reads through the constant address space.
__global__ __launch_bounds__(kBlock) void k_q32_anchor_combine(const AnchorCombineArgs a) {
  using cchar = const __attribute__((address_space(4))) char;
  using cdouble = const __attribute__((address_space(4))) double;
  typedef const float* cfloatp;
  cchar* const karg = (cchar*)__builtin_amdgcn_kernarg_segment_ptr();
  const int j = blockIdx.y;
  cdouble* const g = (cdouble*)(karg + offsetof(AnchorCombineArgs, g));
  const __attribute__((address_space(4))) cfloatp* const d =
      (const __attribute__((address_space(4))) cfloatp*)(karg + offsetof(AnchorCombineArgs, d)) + j * ssp::kOuterSrc;
  const double* const src = a.a[j];
  double* const y = a.y[j];
  constexpr int U = 2, B = 8;
  const int lane = threadIdx.x & 63;
  const size_t gw = size_t(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
  const size_t nw = size_t(gridDim.x) * (kBlock / 64);
  const size_t n4 = a.n >> 2, win = 64 * U;
  for (size_t c = gw; c * win < n4; c += nw) {
    const size_t p0 = c * win + lane;
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) ok[u] = p0 + 64 * u < n4;
    double acc[U][4];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const Raw<double> r = ok[u] ? ldq<true>(src + 4 * (p0 + 64 * u)) : zero_quad<double>();
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[u][e] = r.get(e);
    }
    const auto add = [&](int i, const Raw<float>(&xv)[U]) {
      const double gi = g[i];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[u][e] = fma(gi, xv[u].get(e), acc[u][e]);
    };
    int i = 0;
    for (; i + B <= a.k; i += B) {
      Raw<float> xv[B][U];
#pragma unroll
      for (int b = 0; b < B; ++b)
#pragma unroll
        for (int u = 0; u < U; ++u) xv[b][u] = ok[u] ? ldq<true>(d[i + b] + 4 * (p0 + 64 * u)) : zero_quad<float>();
#pragma unroll
      for (int b = 0; b < B; ++b) add(i + b, xv[b]);
    }
    for (; i < a.k; ++i) {
      Raw<float> xv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) xv[u] = ok[u] ? ldq<true>(d[i] + 4 * (p0 + 64 * u)) : zero_quad<float>();
      add(i, xv);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (ok[u]) stq<true>(y + 4 * (p0 + 64 * u), acc[u]);
  }
  // the n mod 4 last elements: one thread of workgroup 0 each
  if (blockIdx.x == 0 && threadIdx.x < (a.n & 3)) {
    const size_t e = 4 * n4 + threadIdx.x;
    double v = src[e];
    for (int i = 0; i < a.k; ++i) v = fma(g[i], double(d[i][e]), v);
    y[e] = v;
  }
}

// ---- host side ------------------------------------------------------------------------------------
bool bad_dtype(ssp_dtype t) { return t != SSP_F64 && t != SSP_F32; }
double esize(ssp_dtype t) { return t == SSP_F32 ? 4.0 : 8.0; }

// The storage pair of a mixed call as types: launch(X, Y) gets a value of the first operand's storage type
// and one of the second's (tags: only decltype(X), decltype(Y) are used) and launches the kernels of that
// pair.  (f64, f64) never reaches here: every entry point forwards it to its f64 call.
template <typename F>
int with_pair(ssp_dtype tx, ssp_dtype ty, F&& launch) {
  if (tx == SSP_F32 && ty == SSP_F32) launch(float(), float());
  else if (tx == SSP_F32) launch(float(), double());
  else launch(double(), float());
  SSP_TRY_HIP(hipGetLastError());
  return SSP_OK;
}

// The convert launch (no ledger row of its own, no look at exact_max: a convert is the same in both).
int convert(ssp_ctx* ctx, void* x, ssp_dtype tx, const void* y, ssp_dtype ty, double ys, size_t n) {
  if (n == 0) return SSP_OK;
  const dim3 g(quad_grid(ctx, n, kMxU, 16)), b(kBlock);
  return with_pair(tx, ty, [&](auto X, auto Y) {
    using TX = decltype(X);
    using TY = decltype(Y);
    SSP_LAUNCH((k_mx_copy<TX, TY>), g, b, 0, ctx->stream, static_cast<TX*>(x), static_cast<const TY*>(y), n, ys);
  });
}

// Scratch f64 vectors of the exact path (vectors of at most exact_max elements): an f32 operand widened
// once per distinct pointer; blocks go back to the arena when the call returns (stream-ordered reuse).
struct Scratch {
  ssp_ctx* ctx;
  std::map<const void*, double*> widened;
  std::vector<double*> blocks;
  explicit Scratch(ssp_ctx* c) : ctx(c) {}
  Scratch(const Scratch&) = delete;
  Scratch& operator=(const Scratch&) = delete;
  ~Scratch() {
    for (double* b : blocks) (void)ssp_free(ctx, b);
  }
  int fresh(size_t n, double** out) {
    SSP_TRY(ssp_alloc(ctx, n, out));
    blocks.push_back(*out);
    return SSP_OK;
  }
  int widen(const void* p, ssp_dtype t, size_t n, const double** out) {
    if (t == SSP_F64) {
      *out = static_cast<const double*>(p);
      return SSP_OK;
    }
    auto it = widened.find(p);
    if (it == widened.end()) {
      double* w;
      SSP_TRY(fresh(n, &w));
      SSP_TRY(convert(ctx, w, SSP_F64, p, SSP_F32, 1.0, n));
      it = widened.emplace(p, w).first;
    }
    *out = it->second;
    return SSP_OK;
  }
};

// The ladder of k_mx_inner over (MG, NG): the smallest instantiated tile that holds a.m rows and a.k columns.
template <typename TX, typename CP, int MG>
void launch_inner_ng(ssp_ctx* ctx, unsigned grid, const MxInnerArgs& a) {
  const int need = (a.k + 3) / 4;
  const dim3 g(grid), b(kBlock);
  if (need <= 1) SSP_LAUNCH((k_mx_inner<TX, CP, MG, 1>), g, b, 0, ctx->stream, a);
  else if (need <= 2) SSP_LAUNCH((k_mx_inner<TX, CP, MG, 2>), g, b, 0, ctx->stream, a);
  else if (need <= 4) SSP_LAUNCH((k_mx_inner<TX, CP, MG, 4>), g, b, 0, ctx->stream, a);
  else if (need <= 8) SSP_LAUNCH((k_mx_inner<TX, CP, MG, 8>), g, b, 0, ctx->stream, a);
  else if (need <= 12) SSP_LAUNCH((k_mx_inner<TX, CP, MG, 12>), g, b, 0, ctx->stream, a);
  else SSP_LAUNCH((k_mx_inner<TX, CP, MG, 16>), g, b, 0, ctx->stream, a);
}

template <typename TX, typename CP>
void launch_inner_mg(ssp_ctx* ctx, unsigned grid, const MxInnerArgs& a) {
  const int mg = (a.m + 3) / 4;
  if (mg <= 1) launch_inner_ng<TX, CP, 1>(ctx, grid, a);
  else if (mg <= 2) launch_inner_ng<TX, CP, 2>(ctx, grid, a);
  else launch_inner_ng<TX, CP, 4>(ctx, grid, a);
}

int launch_inner(ssp_ctx* ctx, unsigned grid, const MxInnerArgs& a, ssp_dtype tr, ssp_dtype tc) {
  return with_pair(tr, tc, [&](auto X, auto Y) { launch_inner_mg<decltype(X), decltype(Y)>(ctx, grid, a); });
}

// One wave per chunk of 64 elements, at most ctx->inner_per_cu workgroups per CU (k_gemm_inner's grid).
unsigned inner_grid(const ssp_ctx* ctx, size_t n) {
  const size_t blocks = (n / 64 + 1 + 3) / 4;
  const size_t cap = size_t(ctx->num_cus) * size_t(ctx->inner_per_cu);
  return unsigned(std::max<size_t>(1, std::min(blocks, cap)));
}

template <typename TX, typename TY, bool SET, bool TWIN = false>
void launch_outer_m(ssp_ctx* ctx, unsigned grid, const MxOuterArgs& a) {
  const dim3 g(grid), b(kBlock);
  if (a.m <= 1) SSP_LAUNCH((k_mx_outer<TX, TY, 1, SET, TWIN>), g, b, 0, ctx->stream, a);
  else if (a.m <= 2) SSP_LAUNCH((k_mx_outer<TX, TY, 2, SET, TWIN>), g, b, 0, ctx->stream, a);
  else if (a.m <= 4) SSP_LAUNCH((k_mx_outer<TX, TY, 4, SET, TWIN>), g, b, 0, ctx->stream, a);
  else if (a.m <= 8) SSP_LAUNCH((k_mx_outer<TX, TY, 8, SET, TWIN>), g, b, 0, ctx->stream, a);
  else SSP_LAUNCH((k_mx_outer<TX, TY, 16, SET, TWIN>), g, b, 0, ctx->stream, a);
}

// yy[j] = (set ? 0 : ys[j] yy[j]) + sum_i alphas(i, j) (xs[i] xx[i]) on the bandwidth path (k, m, n > 0).
// Destinations are independent, kOuterDst per launch; sources are applied in increasing order, kOuterSrc per
// launch, so each destination sees the reference's summation order (an f32 destination is rounded per launch).
// xs, ys: null for none; the destinations' scales ride along with the first source chunk, and not with set.
// ww (f32 sources and destinations only; null for none): the destinations' f64 twins, written by the launch of
// the last source chunk with the values it stores.
int outer_chunks(ssp_ctx* ctx, const double* alphas, const void* const* xx, ssp_dtype tx, const double* xs, int k,
                 void* const* yy, ssp_dtype ty, const double* ys, int m, size_t n, bool set, double* const* ww = nullptr) {
  // one wave per window of 2 x 64 quads, ctx->outer_per_cu workgroups per CU (SSP_OUTER_WG_PER_CU)
  const unsigned grid = ssp::stream_grid(ctx, n / 4 + 1, 2, unsigned(ctx->outer_per_cu));
  const auto staged = [&](const double* v, size_t count, const double** dev) {
    void* p;
    SSP_TRY(ssp::upload_small(ctx, v, count * sizeof(double), &p));
    *dev = static_cast<const double*>(p);
    return int(SSP_OK);
  };
  for (int j0 = 0; j0 < m; j0 += ssp::kOuterDst) {
    const int mm = std::min(ssp::kOuterDst, m - j0);
    for (int i0 = 0; i0 < k; i0 += ssp::kOuterSrc) {
      MxOuterArgs a{};
      a.m = mm;
      a.k = std::min(ssp::kOuterSrc, k - i0);
      a.n = n;
      for (int i = 0; i < a.k; ++i) a.x[i] = xx[i0 + i];
      for (int j = 0; j < mm; ++j) a.y[j] = yy[j0 + j];
      if (xs) SSP_TRY(staged(xs + i0, size_t(a.k), &a.scale_dev));
      if (ys && !set && i0 == 0) SSP_TRY(staged(ys + j0, size_t(mm), &a.yscale_dev));
      const bool dev = a.k * mm > ssp::kOuterAlpha;
      std::vector<double> block(dev ? size_t(a.k) * mm : 0);
      double* dst = dev ? block.data() : a.alpha;
      for (int i = 0; i < a.k; ++i)
        for (int j = 0; j < mm; ++j) dst[i * mm + j] = alphas[size_t(i0 + i) * m + j0 + j];
      if (dev) SSP_TRY(staged(block.data(), block.size(), &a.alpha_dev));
      SSP_TRY(ssp::flush_uploads(ctx));
      const bool first = set && i0 == 0;  // the launch that writes the destinations without reading them
      if (ww && i0 + ssp::kOuterSrc >= k) {  // the launch that stores the destinations' final values
        for (int j = 0; j < mm; ++j) a.w[j] = ww[j0 + j];
        first ? launch_outer_m<float, float, true, true>(ctx, grid, a) : launch_outer_m<float, float, false, true>(ctx, grid, a);
        SSP_TRY_HIP(hipGetLastError());
        continue;
      }
      SSP_TRY(with_pair(tx, ty, [&](auto X, auto Y) {
        using TX = decltype(X);
        using TY = decltype(Y);
        first ? launch_outer_m<TX, TY, true>(ctx, grid, a) : launch_outer_m<TX, TY, false>(ctx, grid, a);
      }));
    }
  }
  return SSP_OK;
}

}  // namespace

namespace ssp {

// The dense pass of ssp_q32_construct_solution / ssp_q32_block_update outside exact mode:
// yy[j] = (set ? 0 : ys[j] yy[j]) + sum_i alphas(i, j) xx[i] with f32 sources and f64 destinations,
// element for element the fma chain of ssp_gemm_outer_set_scaled / ssp_gemm_outer_scaled on widened
// sources (k_mx_outer; the destination scales ride along with the first source chunk).
int q32_dense_pass(ssp_ctx* ctx, const double* alphas, const float* const* xx, int k, double* const* yy,
                   const double* ys, int m, size_t n, bool set) {
  SSP_TRY(flush_outer(ctx));  // this pass keeps zero fills pending, never a recorded gemm_outer
  if (set && k == 0) {  // zero fills that may stay deferred, as ssp_gemm_outer_set's
    for (int j = 0; j < m; ++j) SSP_TRY(ssp_fill(ctx, 0.0, yy[j], n));
    return SSP_OK;
  }
  if (m == 0 || n == 0) return SSP_OK;
  if (k == 0) {
    for (int j = 0; j < m; ++j)
      if (ys && ys[j] != 1.0) SSP_TRY(ssp_scal(ctx, ys[j], yy[j], n));
    return SSP_OK;
  }
  if (!alphas) return set_error(SSP_ERR_ARG, "ssp_q32: null alphas");
  for (int j = 0; j < m; ++j)
    for (int i = 0; i < k; ++i)
      if (static_cast<const void*>(yy[j]) == static_cast<const void*>(xx[i]))
        return set_error(SSP_ERR_ARG, "ssp_q32: a destination aliases a source");
  // pending zero fills: the sources are read and the read-modify-write destinations too (theirs are
  // stored); a write-only destination's are dropped
  if (!ctx->pending_fills.empty()) {
    for (int i = 0; i < k; ++i) SSP_TRY(flush_fills_over(ctx, xx[i], (n + 1) / 2));
    for (int j = 0; j < m; ++j) SSP_TRY(set ? overwrite_fills(ctx, yy[j], n) : flush_fills_over(ctx, yy[j], n));
  }
  LedgerScope ls(ctx, "gemm_outer_f32", (4.0 * k + (set ? 1.0 : 2.0) * 8.0 * m) * n);
  bool scaled = false;
  for (int j = 0; !set && ys && j < m; ++j) scaled = scaled || ys[j] != 1.0;
  return outer_chunks(ctx, alphas, reinterpret_cast<const void* const*>(xx), SSP_F32, nullptr, k,
                      reinterpret_cast<void* const*>(yy), SSP_F64, scaled ? ys : nullptr, m, n, set);
}

}  // namespace ssp

// The library's dynamic symbol list also holds the weak out-of-line copies of the HIP launch templates that
// the compiler happened not to inline.  k_mx_axpy's three were such; inside with_pair's callable they are
// inlined, so they are instantiated here to leave the list as it was.
#define SSP_KEEP_LAUNCH(TX, TY)                                                                                       \
  template void hipExtLaunchKernelGGL<const TX*, TY*, size_t, double>(void (*)(const TX*, TY*, size_t, double),       \
                                                                      const dim3&, const dim3&, std::uint32_t,        \
                                                                      hipStream_t, hipEvent_t, hipEvent_t,            \
                                                                      std::uint32_t, const TX*, TY*, size_t, double)
SSP_KEEP_LAUNCH(float, float);
SSP_KEEP_LAUNCH(float, double);
SSP_KEEP_LAUNCH(double, float);
#undef SSP_KEEP_LAUNCH

extern "C" {

int ssp_q32_gemm_inner_cols(ssp_ctx* ctx, const double* const* xx, const double* xs, int m, const void* const* yy,
                            const ssp_dtype* ty, const double* ys, int k, size_t n, double* out) {
  SSP_CHECK_CTX(ctx);  // pending zero fills are stored: every operand is read
  if (m < 0 || k < 0) return ssp::set_error(SSP_ERR_ARG, "ssp_q32_gemm_inner_cols: negative dimension");
  if (k > 0 && !ty) return ssp::set_error(SSP_ERR_ARG, "ssp_q32_gemm_inner_cols: null dtype list");
  int n32 = 0;
  for (int j = 0; j < k; ++j) {
    if (bad_dtype(ty[j])) return ssp::set_error(SSP_ERR_ARG, "ssp_q32_gemm_inner_cols: bad dtype");
    n32 += ty[j] == SSP_F32;
  }
  if (m * k > 0 && !out) return ssp::set_error(SSP_ERR_ARG, "ssp_q32_gemm_inner_cols: null out");
  if (m == 0 || k == 0) return SSP_OK;
  SSP_TRY(ssp::check_ptrs(xx, m, n, "ssp_q32_gemm_inner_cols"));
  SSP_TRY(ssp::check_ptrs(yy, k, n, "ssp_q32_gemm_inner_cols"));
  if (n32 == 0)
    return ssp_gemm_inner_scaled(ctx, xx, xs, m, reinterpret_cast<const double* const*>(yy), ys, k, n, out);
  if (n32 == k)  // (its n = 0 is the f64 entry's, in the same m x k layout as its other paths)
    return ssp_mx_gemm_inner(ctx, reinterpret_cast<const void* const*>(xx), SSP_F64, xs, m, yy, SSP_F32, ys, k, n, out);
  std::vector<unsigned char> f32(static_cast<size_t>(k));
  for (int j = 0; j < k; ++j) f32[size_t(j)] = ty[j] == SSP_F32;
  const ssp::ColsPlan plan = ssp::plan_cols(m, f32.data(), k, ssp::kInnerRows, ssp::kInnerCols);
  const int S = plan.slots;
  const size_t total = size_t(m) * S;
  std::vector<double> rs(static_cast<size_t>(m), 1.0), cs(static_cast<size_t>(S), 1.0);
  for (int i = 0; xs && i < m; ++i) rs[size_t(i)] = xs[i];
  for (int j = 0; ys && j < k; ++j) cs[size_t(plan.col_slot[size_t(j)])] = ys[j];
  double bytes = 8.0 * m;
  for (int j = 0; j < k; ++j) bytes += esize(ty[j]);
  std::vector<double> res(total);
  const auto deliver = [&] {
    for (int i = 0; i < m; ++i)
      for (int j = 0; j < k; ++j) out[size_t(i) * k + j] = res[size_t(i) * S + size_t(plan.col_slot[size_t(j)])];
    return SSP_OK;
  };
  if (n == 0) {
    // an empty shard: zeros in the slot layout of every other path, so that the buffer summed over
    // ranks has the layout (m, k, ty[]) give it whatever the local n is (ssp_gemm_inner_scaled's n = 0)
    SSP_TRY(ssp::ensure_result(ctx, total));
    SSP_TRY_HIP(hipMemsetAsync(ctx->result_dev, 0, total * sizeof(double), ctx->stream));
    SSP_TRY(ssp::reduce_fetch(ctx, res.data(), total));
    return deliver();
  }
  const bool exact = ssp::exact_mode(ctx, n);
  Scratch scratch(ctx);
  // exact mode: the reference's sequential dots on widened columns, in the slot layout of the bandwidth
  // path (a padding slot repeats the first row; computed, never read back): what is summed over ranks
  // has the same layout whichever path a rank's shard length takes.
  std::vector<const double*> cols(static_cast<size_t>(exact ? S : 0), xx[0]);
  for (int j = 0; exact && j < k; ++j)
    SSP_TRY(scratch.widen(yy[j], ty[j], n, &cols[size_t(plan.col_slot[size_t(j)])]));
  ssp::FoldTail tail{};
  SSP_TRY(ssp::fold_begin(ctx, int(total), &tail));
  if (exact) {
    ssp::LedgerScope ls(ctx, "gemm_inner_cols", bytes * n);
    SSP_TRY(ssp::exact_inner(ctx, xx, rs.data(), m, cols.data(), cs.data(), S, n, false, tail));
  } else {
    ssp::LedgerScope ls(ctx, "gemm_inner_cols", bytes * n);
    const unsigned grid = inner_grid(ctx, n);
    for (size_t t = 0; t < plan.tiles.size(); ++t) {
      const ssp::ColsTile& tile = plan.tiles[t];
      MxInnerArgs a{};
      a.m = tile.rows;
      a.k = tile.cols;
      a.g64 = tile.g64;
      a.n = n;
      for (int i = 0; i < a.m; ++i) {
        a.x[i] = xx[tile.r0 + i];
        a.xs[i] = rs[size_t(tile.r0 + i)];
      }
      for (int j = 0; j < a.k; ++j) {
        const int col = plan.slot_col[size_t(tile.c0 + j)];
        a.y[j] = col < 0 ? nullptr : yy[col];
        a.ys[j] = cs[size_t(tile.c0 + j)];
      }
      SSP_TRY(ssp::ensure_partial(ctx, size_t(grid) * a.m * a.k));
      a.partial = ctx->partial;
      if (tile.g64 == 0) {  // a tile of f32 columns only: the statically typed kernel on the same arguments
        SSP_TRY(launch_inner(ctx, grid, a, SSP_F64, SSP_F32));
      } else {
        launch_inner_mg<double, ByGroup>(ctx, grid, a);
        SSP_TRY_HIP(hipGetLastError());
      }
      SSP_TRY(ssp::launch_reduce_partials(ctx, ctx->partial, int(grid), a.m, a.k, ctx->result_dev, S, tile.r0, tile.c0,
                                          &tail, t + 1 == plan.tiles.size()));
    }
  }
  SSP_TRY(ssp::fold_finish(ctx, tail, res.data()));
  return deliver();
}

int ssp_q32_combine_widen(ssp_ctx* ctx, const double* alphas, const float* const* xx, int k, float* const* yy,
                          double* const* ww, int m, size_t n) {
  SSP_CHECK_CTX_KEEP_FILLS(ctx);
  if (m < 0 || k < 0) return ssp::set_error(SSP_ERR_ARG, "ssp_q32_combine_widen: negative dimension");
  SSP_TRY(ssp::check_ptrs(xx, k, n, "ssp_q32_combine_widen"));
  SSP_TRY(ssp::check_ptrs(yy, m, n, "ssp_q32_combine_widen"));
  SSP_TRY(ssp::check_ptrs(ww, m, n, "ssp_q32_combine_widen"));
  if (m == 0 || n == 0) return SSP_OK;
  if (k > 0 && !alphas) return ssp::set_error(SSP_ERR_ARG, "ssp_q32_combine_widen: null alphas");
  for (int j = 0; j < m; ++j) {
    for (int i = 0; i < k; ++i)
      if (static_cast<const void*>(yy[j]) == xx[i] || static_cast<const void*>(ww[j]) == xx[i])
        return ssp::set_error(SSP_ERR_ARG, "ssp_q32_combine_widen: a destination aliases a source");
    for (int l = 0; l < m; ++l)
      if (static_cast<const void*>(ww[j]) == yy[l] || (l != j && (yy[l] == yy[j] || ww[l] == ww[j])))
        return ssp::set_error(SSP_ERR_ARG, "ssp_q32_combine_widen: two destinations are the same vector");
  }
  // pending zero fills: the sources are read; the destinations are written in full and read by nothing, so
  // theirs are dropped (one that only shares bytes with an f32 destination's odd end is stored first)
  if (!ctx->pending_fills.empty()) {
    for (int i = 0; i < k; ++i) SSP_TRY(ssp::flush_fills_over(ctx, xx[i], (n + 1) / 2));
    for (int j = 0; j < m; ++j) {
      SSP_TRY(ssp::overwrite_fills(ctx, yy[j], n / 2));
      SSP_TRY(ssp::flush_fills_over(ctx, yy[j], (n + 1) / 2));
      SSP_TRY(ssp::overwrite_fills(ctx, ww[j], n));
    }
  }
  if (k == 0) {  // the sum of no sources
    for (int j = 0; j < m; ++j) {
      SSP_TRY(ssp_fill_f32(ctx, 0.0, yy[j], n));
      SSP_TRY(convert(ctx, ww[j], SSP_F64, yy[j], SSP_F32, 1.0, n));
    }
    return SSP_OK;
  }
  if (ssp::exact_mode(ctx, n)) {  // ssp_mx_gemm_outer's exact path, then the widening copy
    Scratch s(ctx);
    std::vector<const double*> xw(static_cast<size_t>(k));
    std::vector<double*> yw(static_cast<size_t>(m));
    for (int i = 0; i < k; ++i) SSP_TRY(s.widen(xx[i], SSP_F32, n, &xw[size_t(i)]));
    for (int j = 0; j < m; ++j) SSP_TRY(s.fresh(n, &yw[size_t(j)]));
    SSP_TRY(ssp_gemm_outer_set_scaled(ctx, alphas, xw.data(), nullptr, k, yw.data(), m, n));
    for (int j = 0; j < m; ++j) {
      SSP_TRY(convert(ctx, yy[j], SSP_F32, yw[size_t(j)], SSP_F64, 1.0, n));
      SSP_TRY(convert(ctx, ww[j], SSP_F64, yy[j], SSP_F32, 1.0, n));
    }
    return SSP_OK;
  }
  ssp::LedgerScope ls(ctx, "combine_widen_f32", (4.0 * k + 12.0 * m) * n);
  return outer_chunks(ctx, alphas, reinterpret_cast<const void* const*>(xx), SSP_F32, nullptr, k,
                      reinterpret_cast<void* const*>(yy), SSP_F32, nullptr, m, n, true, ww);
}

int ssp_alloc_f32(ssp_ctx* ctx, size_t n, float** out) {
  if (!out) return ssp::set_error(SSP_ERR_ARG, "ssp_alloc_f32: null out");
  double* p = nullptr;
  SSP_TRY(ssp_alloc(ctx, (n + 1) / 2, &p));  // 4 n bytes, rounded as every block of the arena
  *out = reinterpret_cast<float*>(p);
  return SSP_OK;
}

int ssp_free_f32(ssp_ctx* ctx, float* p) { return ssp_free(ctx, reinterpret_cast<double*>(p)); }

int ssp_upload_f32(ssp_ctx* ctx, float* dst, const float* src, size_t n) {
  SSP_CHECK_CTX(ctx);
  if (n == 0) return SSP_OK;
  if (!dst || !src) return ssp::set_error(SSP_ERR_ARG, "ssp_upload_f32: null pointer");
  SSP_TRY_HIP(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  SSP_TRY_HIP(hipStreamSynchronize(ctx->stream));
  return SSP_OK;
}

int ssp_download_f32(ssp_ctx* ctx, float* dst, const float* src, size_t n) {
  SSP_CHECK_CTX(ctx);
  if (n == 0) return SSP_OK;
  if (!dst || !src) return ssp::set_error(SSP_ERR_ARG, "ssp_download_f32: null pointer");
  SSP_TRY_HIP(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  SSP_TRY_HIP(hipStreamSynchronize(ctx->stream));
  return SSP_OK;
}

int ssp_fill_f32(ssp_ctx* ctx, double alpha, float* x, size_t n) {
  SSP_CHECK_CTX(ctx);
  SSP_TRY(ssp::check_vec(x, n, "ssp_fill_f32"));
  if (n == 0) return SSP_OK;
  ssp::LedgerScope ls(ctx, "fill_f32", 4.0 * n);
  SSP_LAUNCH(k_mx_fill, dim3(ssp::stream_grid(ctx, n / 4 + 1, 1, 64)), dim3(kBlock), 0, ctx->stream, x, n, alpha);
  SSP_TRY_HIP(hipGetLastError());
  return SSP_OK;
}

int ssp_scal_f32(ssp_ctx* ctx, double alpha, float* x, size_t n) {
  SSP_CHECK_CTX(ctx);
  SSP_TRY(ssp::check_vec(x, n, "ssp_scal_f32"));
  if (n == 0) return SSP_OK;
  ssp::LedgerScope ls(ctx, "scal_f32", 8.0 * n);
  SSP_LAUNCH(k_mx_scal, dim3(quad_grid(ctx, n, kMxU, 16)), dim3(kBlock), 0, ctx->stream, x, n, alpha);
  SSP_TRY_HIP(hipGetLastError());
  return SSP_OK;
}

int ssp_mx_copy(ssp_ctx* ctx, void* x, ssp_dtype tx, const void* y, ssp_dtype ty, double ys, size_t n) {
  SSP_CHECK_CTX(ctx);
  if (bad_dtype(tx) || bad_dtype(ty)) return ssp::set_error(SSP_ERR_ARG, "ssp_mx_copy: bad dtype");
  SSP_TRY(ssp::check_vec(x, n, "ssp_mx_copy"));
  SSP_TRY(ssp::check_vec(y, n, "ssp_mx_copy"));
  if (tx == SSP_F64 && ty == SSP_F64) {
    double* xd = static_cast<double*>(x);
    const double* yd = static_cast<const double*>(y);
    return ys == 1.0 ? ssp_copy(ctx, xd, yd, n) : ssp_scal_copy(ctx, ys, xd, yd, n);
  }
  if (n == 0) return SSP_OK;
  if (x == y) {
    if (tx != ty) return ssp::set_error(SSP_ERR_ARG, "ssp_mx_copy: a vector converted onto itself");
    return ys == 1.0 ? SSP_OK : ssp_scal_f32(ctx, ys, static_cast<float*>(x), n);
  }
  ssp::LedgerScope ls(ctx, "copy_f32", (esize(tx) + esize(ty)) * n);
  return convert(ctx, x, tx, y, ty, ys, n);
}

int ssp_quantise_f32(ssp_ctx* ctx, double* const* xx, const double* xs, int m, size_t n) {
  SSP_CHECK_CTX(ctx);  // pending zero fills are stored: every vector is read
  if (m < 0) return ssp::set_error(SSP_ERR_ARG, "ssp_quantise_f32: negative dimension");
  if (m == 0 || n == 0) return SSP_OK;
  SSP_TRY(ssp::check_ptrs(xx, m, n, "ssp_quantise_f32"));
  ssp::LedgerScope ls(ctx, "quantise_f32", 16.0 * m * n);
  for (int v0 = 0; v0 < m; v0 += ssp::kPrecVec) {
    QuantArgs a{};
    const int mm = std::min(ssp::kPrecVec, m - v0);
    for (int v = 0; v < mm; ++v) {
      a.x[v] = xx[v0 + v];
      a.s[v] = xs ? xs[v0 + v] : 1.0;
    }
    a.n = n;
    SSP_LAUNCH(k_quantise_f32, dim3(quad_grid(ctx, n, kMxU, 16), unsigned(mm)), dim3(kBlock), 0, ctx->stream, a);
    SSP_TRY_HIP(hipGetLastError());
  }
  return SSP_OK;
}

int ssp_mx_axpy(ssp_ctx* ctx, double alpha, const void* x, ssp_dtype tx, void* y, ssp_dtype ty, size_t n) {
  SSP_CHECK_CTX(ctx);
  if (bad_dtype(tx) || bad_dtype(ty)) return ssp::set_error(SSP_ERR_ARG, "ssp_mx_axpy: bad dtype");
  SSP_TRY(ssp::check_vec(x, n, "ssp_mx_axpy"));
  SSP_TRY(ssp::check_vec(y, n, "ssp_mx_axpy"));
  if (tx == SSP_F64 && ty == SSP_F64) return ssp_axpy(ctx, alpha, static_cast<const double*>(x), static_cast<double*>(y), n);
  if (n == 0) return SSP_OK;
  if (ssp::exact_mode(ctx, n)) {
    Scratch s(ctx);
    const double* xw;
    SSP_TRY(s.widen(x, tx, n, &xw));
    if (ty == SSP_F64) return ssp_axpy(ctx, alpha, xw, static_cast<double*>(y), n);
    double* yw;
    SSP_TRY(s.fresh(n, &yw));
    SSP_TRY(convert(ctx, yw, SSP_F64, y, SSP_F32, 1.0, n));
    SSP_TRY(ssp_axpy(ctx, alpha, xw, yw, n));
    return convert(ctx, y, SSP_F32, yw, SSP_F64, 1.0, n);
  }
  ssp::LedgerScope ls(ctx, "axpy_f32", (esize(tx) + 2 * esize(ty)) * n);
  const dim3 g(quad_grid(ctx, n, kMxU, 16)), b(kBlock);
  return with_pair(tx, ty, [&](auto X, auto Y) {
    using TX = decltype(X);
    using TY = decltype(Y);
    SSP_LAUNCH((k_mx_axpy<TX, TY>), g, b, 0, ctx->stream, static_cast<const TX*>(x), static_cast<TY*>(y), n, alpha);
  });
}

int ssp_mx_dot(ssp_ctx* ctx, const void* x, ssp_dtype tx, const void* y, ssp_dtype ty, size_t n, double* out) {
  SSP_CHECK_CTX(ctx);
  if (bad_dtype(tx) || bad_dtype(ty)) return ssp::set_error(SSP_ERR_ARG, "ssp_mx_dot: bad dtype");
  if (!out) return ssp::set_error(SSP_ERR_ARG, "ssp_mx_dot: null out");
  SSP_TRY(ssp::check_vec(x, n, "ssp_mx_dot"));
  SSP_TRY(ssp::check_vec(y, n, "ssp_mx_dot"));
  if ((tx == SSP_F64 && ty == SSP_F64) || n == 0)  // n = 0: the f64 entry's zero, reduced over ranks
    return ssp_dot(ctx, static_cast<const double*>(x), static_cast<const double*>(y), n, out);
  if (ssp::exact_mode(ctx, n)) {
    Scratch s(ctx);
    const double *xw, *yw;
    SSP_TRY(s.widen(x, tx, n, &xw));
    SSP_TRY(s.widen(y, ty, n, &yw));
    return ssp_dot(ctx, xw, yw, n, out);
  }
  const unsigned grid = quad_grid(ctx, n, kMxU, 8);
  SSP_TRY(ssp::ensure_partial(ctx, grid));
  ssp::FoldTail tail{};
  SSP_TRY(ssp::fold_begin(ctx, 1, &tail));
  {
    ssp::LedgerScope ls(ctx, "dot_f32", (esize(tx) + esize(ty)) * n);
    const dim3 g(grid), b(kBlock);
    SSP_TRY(with_pair(tx, ty, [&](auto X, auto Y) {
      using TX = decltype(X);
      using TY = decltype(Y);
      SSP_LAUNCH((k_mx_dot<TX, TY>), g, b, 0, ctx->stream, static_cast<const TX*>(x), static_cast<const TY*>(y), n,
                 ctx->partial, tail);
    }));
  }
  return ssp::fold_finish(ctx, tail, out);
}

int ssp_mx_rhs_residual_norms(ssp_ctx* ctx, const void* const* bb, ssp_dtype tb, const double* s, double* const* yy,
                              const double* ys, int m, size_t n, double* out) {
  SSP_CHECK_CTX(ctx);  // pending zero fills are stored: every operand is read
  if (bad_dtype(tb)) return ssp::set_error(SSP_ERR_ARG, "ssp_mx_rhs_residual_norms: bad dtype");
  if (m < 0) return ssp::set_error(SSP_ERR_ARG, "ssp_mx_rhs_residual_norms: negative dimension");
  if (m == 0) return SSP_OK;
  if (!s || !out) return ssp::set_error(SSP_ERR_ARG, "ssp_mx_rhs_residual_norms: null scales or out");
  SSP_TRY(ssp::check_ptrs(bb, m, n, "ssp_mx_rhs_residual_norms"));
  SSP_TRY(ssp::check_ptrs(yy, m, n, "ssp_mx_rhs_residual_norms"));
  for (int j = 0; n > 0 && j < m; ++j)
    for (int i = 0; i < m; ++i)
      if (static_cast<const void*>(yy[j]) == bb[i] || (i < j && yy[i] == yy[j]))
        return ssp::set_error(SSP_ERR_ARG, "ssp_mx_rhs_residual_norms: a destination aliases another operand");
  if (m > ssp::kOuterDst) {  // more than one launch: the unfused sequence, same values (at every n: one
                             // reduction per vector on every rank)
    for (int j = 0; j < m; ++j) {
      if (ys && ys[j] != 1.0) SSP_TRY(ssp_scal(ctx, ys[j], yy[j], n));
      SSP_TRY(ssp_mx_axpy(ctx, -1.0, bb[j], tb, yy[j], SSP_F64, n));
      SSP_TRY(ssp_scal(ctx, s[j], yy[j], n));
    }
    for (int j = 0; j < m; ++j) SSP_TRY(ssp_dot(ctx, yy[j], yy[j], n, out + j));
    return SSP_OK;
  }
  if (n == 0) {  // an empty shard: zeros, in the one buffer of length m every other path reduces
    SSP_TRY(ssp::ensure_result(ctx, size_t(m)));
    SSP_TRY_HIP(hipMemsetAsync(ctx->result_dev, 0, size_t(m) * sizeof(double), ctx->stream));
    return ssp::reduce_fetch(ctx, out, size_t(m));
  }
  const bool exact = ssp::exact_mode(ctx, n);
  const unsigned grid = quad_grid(ctx, n, kMxU, unsigned(ctx->fused_per_cu));
  RhsResidualArgs a{};
  a.m = m;
  a.n = n;
  for (int j = 0; j < m; ++j) {
    a.b[j] = bb[j];
    a.y[j] = yy[j];
    a.s[j] = s[j];
    a.ys[j] = ys ? ys[j] : 1.0;
  }
  ssp::FoldTail tail{};
  SSP_TRY(ssp::fold_begin(ctx, m, &tail));
  {
    ssp::LedgerScope ls(ctx, "rhs_residual_norms", (16.0 + esize(tb)) * n * m);
    if (!exact) {
      SSP_TRY(ssp::ensure_partial(ctx, size_t(grid) * m));
      a.partial = ctx->partial;
      a.tail = tail;
    }
    const dim3 g(grid), b(kBlock);
    const auto launch = [&](auto B) {
      using TB = decltype(B);
      if (m <= 1) SSP_LAUNCH((k_mx_rhs_residual_norms<TB, 1>), g, b, 0, ctx->stream, a);
      else if (m <= 4) SSP_LAUNCH((k_mx_rhs_residual_norms<TB, 4>), g, b, 0, ctx->stream, a);
      else SSP_LAUNCH((k_mx_rhs_residual_norms<TB, 8>), g, b, 0, ctx->stream, a);
    };
    if (tb == SSP_F32) launch(float());
    else launch(double());
    SSP_TRY_HIP(hipGetLastError());
    // short vectors: every element above is the unfused sequence's (each operation rounded once, in either
    // arithmetic); the norms are the reference's sequential dots, one reduction for all of them
    if (exact)
      SSP_TRY(ssp::exact_inner(ctx, const_cast<const double* const*>(yy), nullptr, m,
                               const_cast<const double* const*>(yy), nullptr, m, n, true, tail));
  }
  return ssp::fold_finish(ctx, tail, out);
}

int ssp_mx_gemm_inner(ssp_ctx* ctx, const void* const* xx, ssp_dtype tx, const double* xs, int m,
                      const void* const* yy, ssp_dtype ty, const double* ys, int k, size_t n, double* out) {
  SSP_CHECK_CTX(ctx);
  if (bad_dtype(tx) || bad_dtype(ty)) return ssp::set_error(SSP_ERR_ARG, "ssp_mx_gemm_inner: bad dtype");
  if (m < 0 || k < 0) return ssp::set_error(SSP_ERR_ARG, "ssp_mx_gemm_inner: negative dimension");
  if (m * k > 0 && !out) return ssp::set_error(SSP_ERR_ARG, "ssp_mx_gemm_inner: null out");
  if (m == 0 || k == 0) return SSP_OK;
  SSP_TRY(ssp::check_ptrs(xx, m, n, "ssp_mx_gemm_inner"));
  SSP_TRY(ssp::check_ptrs(yy, k, n, "ssp_mx_gemm_inner"));
  if ((tx == SSP_F64 && ty == SSP_F64) || n == 0)  // n = 0: the f64 entry's zeros, reduced over ranks
    return ssp_gemm_inner_scaled(ctx, reinterpret_cast<const double* const*>(xx), xs, m,
                                 reinterpret_cast<const double* const*>(yy), ys, k, n, out);
  if (ssp::exact_mode(ctx, n)) {
    Scratch s(ctx);
    std::vector<const double*> xw(static_cast<size_t>(m)), yw(static_cast<size_t>(k));
    for (int i = 0; i < m; ++i) SSP_TRY(s.widen(xx[i], tx, n, &xw[size_t(i)]));
    for (int j = 0; j < k; ++j) SSP_TRY(s.widen(yy[j], ty, n, &yw[size_t(j)]));
    return ssp_gemm_inner_scaled(ctx, xw.data(), xs, m, yw.data(), ys, k, n, out);
  }
  // The shorter side on the MFMA rows (at most 16 per launch), the longer on the columns (at most 64):
  // the chunking of ssp_gemm_inner, the same result layout for the reduction over ranks.
  const bool swap = m > k;
  const void* const* rows = swap ? yy : xx;
  const void* const* cols = swap ? xx : yy;
  const ssp_dtype tr = swap ? ty : tx, tc = swap ? tx : ty;
  const int R = swap ? k : m, C = swap ? m : k;
  std::vector<double> rs(size_t(R), 1.0), cs(size_t(C), 1.0);
  for (int i = 0; i < m; ++i) (swap ? cs : rs)[size_t(i)] = xs ? xs[i] : 1.0;
  for (int j = 0; j < k; ++j) (swap ? rs : cs)[size_t(j)] = ys ? ys[j] : 1.0;
  const size_t total = size_t(R) * C;
  ssp::FoldTail tail{};
  SSP_TRY(ssp::fold_begin(ctx, int(total), &tail));
  {
    ssp::LedgerScope ls(ctx, "gemm_inner_f32", (esize(tx) * m + esize(ty) * k) * n);
    const unsigned grid = inner_grid(ctx, n);
    for (int r0 = 0; r0 < R; r0 += ssp::kInnerRows) {
      for (int c0 = 0; c0 < C; c0 += ssp::kInnerCols) {
        MxInnerArgs a{};
        a.m = std::min(ssp::kInnerRows, R - r0);
        a.k = std::min(ssp::kInnerCols, C - c0);
        a.n = n;
        for (int i = 0; i < a.m; ++i) {
          a.x[i] = rows[r0 + i];
          a.xs[i] = rs[size_t(r0 + i)];
        }
        for (int j = 0; j < a.k; ++j) {
          a.y[j] = cols[c0 + j];
          a.ys[j] = cs[size_t(c0 + j)];
        }
        SSP_TRY(ssp::ensure_partial(ctx, size_t(grid) * a.m * a.k));
        a.partial = ctx->partial;
        SSP_TRY(launch_inner(ctx, grid, a, tr, tc));
        const bool last = r0 + ssp::kInnerRows >= R && c0 + ssp::kInnerCols >= C;
        SSP_TRY(ssp::launch_reduce_partials(ctx, ctx->partial, int(grid), a.m, a.k, ctx->result_dev, C, r0, c0, &tail, last));
      }
    }
  }
  std::vector<double> t(swap ? total : 0);
  SSP_TRY(ssp::fold_finish(ctx, tail, swap ? t.data() : out));
  if (swap)
    for (int i = 0; i < m; ++i)
      for (int j = 0; j < k; ++j) out[size_t(i) * k + j] = t[size_t(j) * m + i];
  return SSP_OK;
}

int ssp_mx_gemm_outer(ssp_ctx* ctx, const double* alphas, const void* const* xx, ssp_dtype tx, const double* xs, int k,
                      void* const* yy, ssp_dtype ty, int m, size_t n, int set) {
  SSP_CHECK_CTX(ctx);
  if (bad_dtype(tx) || bad_dtype(ty)) return ssp::set_error(SSP_ERR_ARG, "ssp_mx_gemm_outer: bad dtype");
  if (m < 0 || k < 0) return ssp::set_error(SSP_ERR_ARG, "ssp_mx_gemm_outer: negative dimension");
  if (tx == SSP_F64 && ty == SSP_F64) {
    const double* const* xd = reinterpret_cast<const double* const*>(xx);
    double* const* yd = reinterpret_cast<double* const*>(yy);
    return set ? ssp_gemm_outer_set_scaled(ctx, alphas, xd, xs, k, yd, m, n)
               : ssp_gemm_outer_scaled(ctx, alphas, xd, xs, k, yd, nullptr, m, n);
  }
  SSP_TRY(ssp::check_ptrs(xx, k, n, "ssp_mx_gemm_outer"));
  SSP_TRY(ssp::check_ptrs(yy, m, n, "ssp_mx_gemm_outer"));
  if (m == 0 || n == 0) return SSP_OK;
  if (k == 0) {
    for (int j = 0; set && j < m; ++j) {
      if (ty == SSP_F32) SSP_TRY(ssp_fill_f32(ctx, 0.0, static_cast<float*>(yy[j]), n));
      else SSP_TRY(ssp_fill(ctx, 0.0, static_cast<double*>(yy[j]), n));
    }
    return SSP_OK;
  }
  if (!alphas) return ssp::set_error(SSP_ERR_ARG, "ssp_mx_gemm_outer: null alphas");
  for (int j = 0; j < m; ++j)
    for (int i = 0; i < k; ++i)
      if (yy[j] == xx[i]) return ssp::set_error(SSP_ERR_ARG, "ssp_mx_gemm_outer: a destination aliases a source");
  if (ssp::exact_mode(ctx, n)) {
    Scratch s(ctx);
    std::vector<const double*> xw(static_cast<size_t>(k));
    std::vector<double*> yw(static_cast<size_t>(m));
    for (int i = 0; i < k; ++i) SSP_TRY(s.widen(xx[i], tx, n, &xw[size_t(i)]));
    for (int j = 0; j < m; ++j) {
      if (ty == SSP_F64) {
        yw[size_t(j)] = static_cast<double*>(yy[j]);
        continue;
      }
      SSP_TRY(s.fresh(n, &yw[size_t(j)]));
      if (!set) SSP_TRY(convert(ctx, yw[size_t(j)], SSP_F64, yy[j], SSP_F32, 1.0, n));
    }
    SSP_TRY(set ? ssp_gemm_outer_set_scaled(ctx, alphas, xw.data(), xs, k, yw.data(), m, n)
                : ssp_gemm_outer_scaled(ctx, alphas, xw.data(), xs, k, yw.data(), nullptr, m, n));
    for (int j = 0; ty == SSP_F32 && j < m; ++j) SSP_TRY(convert(ctx, yy[j], SSP_F32, yw[size_t(j)], SSP_F64, 1.0, n));
    return SSP_OK;
  }
  ssp::LedgerScope ls(ctx, "gemm_outer_f32", (esize(tx) * k + (set ? 1.0 : 2.0) * esize(ty) * m) * n);
  bool scaled = false;
  for (int i = 0; xs && i < k; ++i) scaled = scaled || xs[i] != 1.0;
  return outer_chunks(ctx, alphas, xx, tx, scaled ? xs : nullptr, k, yy, ty, nullptr, m, n, set != 0);
}

int ssp_q32_store_differences(ssp_ctx* ctx, const double* const* vv, double* const* aa, float* const* dd, int m,
                              size_t n) {
  SSP_CHECK_CTX_KEEP_FILLS(ctx);
  if (m < 0) return ssp::set_error(SSP_ERR_ARG, "ssp_q32_store_differences: negative dimension");
  if (m == 0 || n == 0) return SSP_OK;
  SSP_TRY(ssp::check_ptrs(vv, m, n, "ssp_q32_store_differences"));
  SSP_TRY(ssp::check_ptrs(aa, m, n, "ssp_q32_store_differences"));
  if (dd) SSP_TRY(ssp::check_ptrs(dd, m, n, "ssp_q32_store_differences"));
  for (int j = 0; j < m; ++j)
    for (int l = 0; l < m; ++l) {
      const void* const d = dd ? static_cast<const void*>(dd[l]) : nullptr;
      if (aa[j] == vv[l] || (dd && (d == vv[j] || d == aa[j])))
        return ssp::set_error(SSP_ERR_ARG, "ssp_q32_store_differences: a destination aliases a source");
      if (l != j && (aa[l] == aa[j] || (dd && dd[l] == dd[j])))
        return ssp::set_error(SSP_ERR_ARG, "ssp_q32_store_differences: two destinations are the same vector");
    }
  if (!dd) {  // the first point: the anchors only (ssp_copy drops their pending zero fills and stores the sources')
    for (int j = 0; j < m; ++j) SSP_TRY(ssp_copy(ctx, aa[j], vv[j], n));
    return SSP_OK;
  }
  // pending zero fills: the new points and the anchors are read; the differences are written in full and read by
  // nothing (one that only shares bytes with a difference's odd end is stored first)
  if (!ctx->pending_fills.empty())
    for (int j = 0; j < m; ++j) {
      SSP_TRY(ssp::flush_fills_over(ctx, vv[j], n));
      SSP_TRY(ssp::flush_fills_over(ctx, aa[j], n));
      SSP_TRY(ssp::overwrite_fills(ctx, dd[j], n / 2));
      SSP_TRY(ssp::flush_fills_over(ctx, dd[j], (n + 1) / 2));
    }
  ssp::LedgerScope ls(ctx, "store_differences_f32", 28.0 * m * n);
  for (int v0 = 0; v0 < m; v0 += ssp::kPrecVec) {
    StoreDiffArgs a{};
    const int mm = std::min(ssp::kPrecVec, m - v0);
    for (int v = 0; v < mm; ++v) {
      a.v[v] = vv[v0 + v];
      a.a[v] = aa[v0 + v];
      a.d[v] = dd[v0 + v];
    }
    a.n = n;
    SSP_LAUNCH(k_q32_store_diff, dim3(quad_grid(ctx, n, kMxU, 16), unsigned(mm)), dim3(kBlock), 0, ctx->stream, a);
    SSP_TRY_HIP(hipGetLastError());
  }
  return SSP_OK;
}

int ssp_q32_anchor_combine(ssp_ctx* ctx, const double* gammas, const double* const* aa, const float* const* dd, int k,
                           double* const* yy, int m, size_t n) {
  SSP_CHECK_CTX_KEEP_FILLS(ctx);
  if (m < 0 || k < 0) return ssp::set_error(SSP_ERR_ARG, "ssp_q32_anchor_combine: negative dimension");
  if (m == 0 || n == 0) return SSP_OK;
  SSP_TRY(ssp::check_ptrs(aa, m, n, "ssp_q32_anchor_combine"));
  SSP_TRY(ssp::check_ptrs(yy, m, n, "ssp_q32_anchor_combine"));
  SSP_TRY(ssp::check_ptrs(dd, m * k, n, "ssp_q32_anchor_combine"));
  if (k > 0 && !gammas) return ssp::set_error(SSP_ERR_ARG, "ssp_q32_anchor_combine: null gammas");
  for (int j = 0; j < m; ++j) {
    for (int l = 0; l < m; ++l) {
      if (yy[j] == aa[l]) return ssp::set_error(SSP_ERR_ARG, "ssp_q32_anchor_combine: a destination aliases a source");
      if (l != j && yy[l] == yy[j])
        return ssp::set_error(SSP_ERR_ARG, "ssp_q32_anchor_combine: two destinations are the same vector");
    }
    for (int i = 0; i < m * k; ++i)
      if (static_cast<const void*>(yy[j]) == dd[i])
        return ssp::set_error(SSP_ERR_ARG, "ssp_q32_anchor_combine: a destination aliases a source");
  }
  // pending zero fills: the anchors and the differences are read; the destinations are written in full and read
  // by nothing, so theirs are dropped
  if (!ctx->pending_fills.empty()) {
    for (int j = 0; j < m; ++j) SSP_TRY(ssp::flush_fills_over(ctx, aa[j], n));
    for (int i = 0; i < m * k; ++i) SSP_TRY(ssp::flush_fills_over(ctx, dd[i], (n + 1) / 2));
    for (int j = 0; j < m; ++j) SSP_TRY(ssp::overwrite_fills(ctx, yy[j], n));
  }
  if (k == 0) {  // no differences: the anchors themselves
    for (int j = 0; j < m; ++j) SSP_TRY(ssp_copy(ctx, yy[j], aa[j], n));
    return SSP_OK;
  }
  std::vector<double> neg(static_cast<size_t>(k));
  for (int i = 0; i < k; ++i) neg[size_t(i)] = -gammas[i];
  if (ssp::exact_mode(ctx, n)) {  // short vectors: the unfused sequence itself, ssp_mx_gemm_outer's exact path
    for (int j = 0; j < m; ++j) {
      SSP_TRY(ssp_copy(ctx, yy[j], aa[j], n));
      void* y = yy[j];
      SSP_TRY(ssp_mx_gemm_outer(ctx, neg.data(), reinterpret_cast<const void* const*>(dd + size_t(j) * k), SSP_F32,
                                nullptr, k, &y, SSP_F64, 1, n, 0));
    }
    return SSP_OK;
  }
  ssp::LedgerScope ls(ctx, "anchor_combine_f32", (16.0 + 4.0 * k) * m * n);
  // one wave per window of 2 x 64 quads, ctx->outer_per_cu workgroups per CU: outer_chunks' grid
  const unsigned grid = ssp::stream_grid(ctx, n / 4 + 1, 2, unsigned(ctx->outer_per_cu));
  for (int j0 = 0; j0 < m; j0 += kAnchorPanels) {
    const int mm = std::min(kAnchorPanels, m - j0);
    for (int i0 = 0; i0 < k; i0 += ssp::kOuterSrc) {  // later source chunks go on from what the one before stored
      AnchorCombineArgs a{};
      a.k = std::min(ssp::kOuterSrc, k - i0);
      a.n = n;
      for (int i = 0; i < a.k; ++i) a.g[i] = neg[size_t(i0 + i)];
      for (int j = 0; j < mm; ++j) {
        a.a[j] = i0 == 0 ? aa[j0 + j] : yy[j0 + j];
        a.y[j] = yy[j0 + j];
        for (int i = 0; i < a.k; ++i) a.d[j][i] = dd[size_t(j0 + j) * k + i0 + i];
      }
      SSP_LAUNCH(k_q32_anchor_combine, dim3(grid, unsigned(mm)), dim3(kBlock), 0, ctx->stream, a);
      SSP_TRY_HIP(hipGetLastError());
    }
  }
  return SSP_OK;
}

}  // extern "C"
