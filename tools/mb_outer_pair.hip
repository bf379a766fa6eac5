// Both solution constructions of a step (48 -> 8 twice, N = 1e8, the register terms and the norms) as one pass:
// loop-shape candidates for k_gemm_outer_pair against the library's two launches and the library's own pair
// launch, on the same vectors in one process (development tool, not part of the library).
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude tools/mb_outer_pair.hip -o tools/mb_outer_pair \
//          -Literative-solver_amd/lib -lsubspace_hip -Wl,-rpath,'$ORIGIN/../iterative-solver_amd/lib'
// Run:   tools/mb_outer_pair [n=1e8] [sets=3]
//
// Every candidate walks k_dot_partial's 4-position windows as two half-windows of two positions, keeps the
// 32 norm accumulators per lane in LDS and writes its per-workgroup sums (the fold of the ~2000 partials is
// left out: microseconds).  Candidates:
//   seq B   per half-window the P sums (B sources in flight), the P stores, then the A sums: 56 streams at a time
//   mix G   per group of G sources the P loads and the A loads together (G + G in flight): 112 streams
// Library rows: the chain fill x 8, gemm_outer, fill x 8, gemm_outer, axpy x 8, dot x 8 through the C ABI on a
// context created with SSP_OUTER_PAIR=0 (two launches: write-only, then epilogue + norms) and on a default one
// (the pair's launch); their time is the ledger's "gemm_outer" row, kernel time between two events.
// Placement alone moves gemm_outer by +-4 %, so everything runs on `sets` vector sets, each allocated anew
// behind a pad of another size that stays allocated.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "subspace_hip.h"

#define CK(x)                                                                        \
  do {                                                                               \
    hipError_t e = (x);                                                              \
    if (e != hipSuccess) {                                                           \
      printf("HIP error %s at %s:%d\n", hipGetErrorString(e), __FILE__, __LINE__); \
      exit(1);                                                                       \
    }                                                                                \
  } while (0)
#define SK(x)                                                                   \
  do {                                                                          \
    if ((x) != SSP_OK) {                                                        \
      printf("library error %s at %s:%d\n", ssp_last_error(), __FILE__, __LINE__); \
      exit(1);                                                                  \
    }                                                                           \
  } while (0)

typedef double d2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double2 ld2nt(const double* p) {
  const d2v v = __builtin_nontemporal_load(reinterpret_cast<const d2v*>(p));
  return make_double2(v.x, v.y);
}
__device__ __forceinline__ void st2nt(double* p, double2 v) {
  d2v w = {v.x, v.y};
  __builtin_nontemporal_store(w, reinterpret_cast<d2v*>(p));
}

constexpr int M = 8, K = 48, U = 4, H = 2, kBlock = 256;
struct PArgs {
  const double* xp[K];
  const double* xa[K];
  double* yp[M];
  double* ya[M];
  double e[M];
  const double* alpha;  // device, [i * M + j]
  double* partial;
  size_t n;
};

// Whole windows only: the positions past the last one are one workgroup's work in the library and are left out here.
template <bool MIX, int B>
__global__ __launch_bounds__(kBlock) void k_pair(const PArgs a) {
  using cdouble = const __attribute__((address_space(4))) double;
  const auto alpha = [&](int idx) { return ((cdouble*)a.alpha)[idx]; };
  __shared__ double accs[M * U * kBlock];
  double* nacc = accs + threadIdx.x;
#pragma unroll
  for (int q = 0; q < M * U; ++q) nacc[q * kBlock] = 0;
  const int lane = threadIdx.x & 63;
  const size_t gw = size_t(blockIdx.x) * 4 + (threadIdx.x >> 6), nw = size_t(gridDim.x) * 4;
  const size_t win = 64 * U, nwin = (a.n >> 1) / win;
  const double2 z2 = make_double2(0, 0);
  for (size_t c = gw; c < nwin; c += nw) {
#pragma unroll
    for (int h = 0; h < U / H; ++h) {
      const size_t q0 = c * win + 64 * H * h + lane;
      double2 ap[H][M], aa[H][M];
#pragma unroll
      for (int v = 0; v < H; ++v)
#pragma unroll
        for (int j = 0; j < M; ++j) ap[v][j] = aa[v][j] = z2;
      const auto group = [&](const double* const(&x)[K], int i, double2(&acc)[H][M]) {
        double2 xv[B][H];
#pragma unroll
        for (int b = 0; b < B; ++b)
#pragma unroll
          for (int v = 0; v < H; ++v) xv[b][v] = ld2nt(x[i + b] + 2 * (q0 + 64 * v));
#pragma unroll
        for (int b = 0; b < B; ++b)
#pragma unroll
          for (int j = 0; j < M; ++j) {
            const double al = alpha((i + b) * M + j);
#pragma unroll
            for (int v = 0; v < H; ++v) {
              acc[v][j].x = fma(al, xv[b][v].x, acc[v][j].x);
              acc[v][j].y = fma(al, xv[b][v].y, acc[v][j].y);
            }
          }
      };
      if constexpr (MIX) {
#pragma unroll 1
        for (int i = 0; i < K; i += B) {
          double2 xv[2][B][H];
#pragma unroll
          for (int b = 0; b < B; ++b)
#pragma unroll
            for (int v = 0; v < H; ++v) {
              xv[0][b][v] = ld2nt(a.xp[i + b] + 2 * (q0 + 64 * v));
              xv[1][b][v] = ld2nt(a.xa[i + b] + 2 * (q0 + 64 * v));
            }
#pragma unroll
          for (int b = 0; b < B; ++b)
#pragma unroll
            for (int j = 0; j < M; ++j) {
              const double al = alpha((i + b) * M + j);
#pragma unroll
              for (int v = 0; v < H; ++v) {
                ap[v][j].x = fma(al, xv[0][b][v].x, ap[v][j].x);
                ap[v][j].y = fma(al, xv[0][b][v].y, ap[v][j].y);
                aa[v][j].x = fma(al, xv[1][b][v].x, aa[v][j].x);
                aa[v][j].y = fma(al, xv[1][b][v].y, aa[v][j].y);
              }
            }
        }
#pragma unroll
        for (int v = 0; v < H; ++v)
#pragma unroll
          for (int j = 0; j < M; ++j) st2nt(a.yp[j] + 2 * (q0 + 64 * v), ap[v][j]);
      } else {
#pragma unroll 1
        for (int i = 0; i < K; i += B) group(a.xp, i, ap);
#pragma unroll
        for (int v = 0; v < H; ++v)
#pragma unroll
          for (int j = 0; j < M; ++j) st2nt(a.yp[j] + 2 * (q0 + 64 * v), ap[v][j]);
#pragma unroll 1
        for (int i = 0; i < K; i += B) group(a.xa, i, aa);
      }
#pragma unroll
      for (int j = 0; j < M; ++j) {
        const double ea = a.e[j];
#pragma unroll
        for (int v = 0; v < H; ++v) {
          aa[v][j].x = fma(ea, ap[v][j].x, aa[v][j].x);
          aa[v][j].y = fma(ea, ap[v][j].y, aa[v][j].y);
          st2nt(a.ya[j] + 2 * (q0 + 64 * v), aa[v][j]);
          double s = nacc[(j * U + H * h + v) * kBlock];
          s = fma(aa[v][j].x, aa[v][j].x, s);
          s = fma(aa[v][j].y, aa[v][j].y, s);
          nacc[(j * U + H * h + v) * kBlock] = s;
        }
        __builtin_amdgcn_sched_barrier(0);  // one destination's accumulators in registers at a time
      }
    }
  }
  __shared__ double red[kBlock / 64][M];
#pragma unroll
  for (int j = 0; j < M; ++j) {
    double v = (nacc[(j * U + 0) * kBlock] + nacc[(j * U + 1) * kBlock]) +
               (nacc[(j * U + 2) * kBlock] + nacc[(j * U + 3) * kBlock]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) red[threadIdx.x >> 6][j] = v;
  }
  __syncthreads();
  if (threadIdx.x < M) {
    double s = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) s += red[w][threadIdx.x];
    a.partial[size_t(blockIdx.x) * M + threadIdx.x] = s;
  }
}

__global__ void k_init(double* x, size_t n, unsigned seed) {
  for (size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x)
    x[i] = 1e-3 * double((i * 2654435761u + seed * 40503u) % 2001) - 1.0;
}

float median(std::vector<float> t) {
  std::sort(t.begin(), t.end());
  return t[t.size() / 2];
}

float timeit(const std::function<void()>& f, int reps) {
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  f();
  CK(hipDeviceSynchronize());
  std::vector<float> t;
  for (int r = 0; r < reps; ++r) {
    CK(hipEventRecord(e0));
    f();
    CK(hipEventRecord(e1));
    CK(hipEventSynchronize(e1));
    float ms;
    CK(hipEventElapsedTime(&ms, e0, e1));
    t.push_back(ms);
  }
  CK(hipEventDestroy(e0));
  CK(hipEventDestroy(e1));
  return median(t);
}

// The chain of a step through the C ABI; -> kernel milliseconds of its "gemm_outer" row and the launches in it.
float library_chain(ssp_ctx* ctx, const PArgs& a, const double* alpha_host, double* dots, long long* rows_calls,
                    int* launches) {
  SK(ssp_ledger_reset(ctx));
  for (int j = 0; j < M; ++j) SK(ssp_fill(ctx, 0.0, a.yp[j], a.n));
  SK(ssp_gemm_outer(ctx, alpha_host, a.xp, K, a.yp, M, a.n));
  for (int j = 0; j < M; ++j) SK(ssp_fill(ctx, 0.0, a.ya[j], a.n));
  SK(ssp_gemm_outer(ctx, alpha_host, a.xa, K, a.ya, M, a.n));
  for (int j = 0; j < M; ++j) SK(ssp_axpy(ctx, a.e[j], a.yp[j], a.ya[j], a.n));
  for (int j = 0; j < M; ++j) SK(ssp_dot(ctx, a.ya[j], a.ya[j], a.n, &dots[j]));
  float ms = 0;
  *rows_calls = 0;
  *launches = 0;
  const int cnt = ssp_ledger_count(ctx);
  for (int i = 0; i < cnt; ++i) {
    const char* name;
    long long calls;
    double kms, bytes;
    SK(ssp_ledger_entry(ctx, i, &name, &calls, &kms, &bytes));
    if (!calls) continue;
    if (std::strncmp(name, "gemm_outer", 10) == 0) {
      ms += float(kms);
      *rows_calls += calls;
    } else {
      *launches += int(calls);  // anything else the chain launched (none expected)
    }
  }
  return ms;
}

int main(int argc, char** argv) {
  const size_t n = argc > 1 ? size_t(atof(argv[1])) : 100000000;
  const int sets = argc > 2 ? atoi(argv[2]) : 3;
  const int reps = 5;
  const size_t probe_at = 512 * size_t(1000);  // 256 elements inside a whole window, compared with the library's
  if (n < 2 * probe_at) {
    printf("n must be at least %zu\n", 2 * probe_at);
    return 1;
  }
  setenv("SSP_OUTER_PAIR", "0", 1);
  ssp_ctx *two, *one;
  SK(ssp_ctx_create(0, &two));
  unsetenv("SSP_OUTER_PAIR");
  SK(ssp_ctx_create(0, &one));
  SK(ssp_ledger_enable(two, 1));
  SK(ssp_ledger_enable(one, 1));
  std::vector<double> alpha(K * M);
  for (int i = 0; i < K * M; ++i) alpha[i] = 1e-3 * (i % 17) - 7e-3;
  double* alpha_dev;
  CK(hipMalloc((void**)&alpha_dev, sizeof(double) * K * M));
  CK(hipMemcpy(alpha_dev, alpha.data(), sizeof(double) * K * M, hipMemcpyHostToDevice));
  const int grid = 2048;  // 8 workgroups per CU on 256 CUs: win_grid(n, 4, 8) at this n
  double* partial;
  CK(hipMalloc((void**)&partial, sizeof(double) * grid * M));
  const double bytes_pair = 8.0 * n * (2 * K + 2 * M), bytes_two = 8.0 * n * (2 * K + 3 * M);
  struct Row {
    std::string name;
    double bytes;
    std::vector<float> ms;
  };
  std::vector<Row> rows = {{"library, two launches", bytes_two, {}}, {"library, pair launch", bytes_pair, {}},
                           {"seq 4", bytes_pair, {}},               {"seq 8", bytes_pair, {}},
                           {"mix 2+2", bytes_pair, {}},             {"mix 4+4", bytes_pair, {}}};
  std::vector<void*> pads;
  for (int s = 0; s < sets; ++s) {
    void* pad;
    CK(hipMalloc(&pad, (size_t(37) << 20) * (s + 1) + 4096 * s));  // shifts the set's placement; kept
    pads.push_back(pad);
    std::vector<double*> vec(2 * K + 2 * M);
    for (size_t i = 0; i < vec.size(); ++i) {
      CK(hipMalloc((void**)&vec[i], n * 8));
      hipLaunchKernelGGL(k_init, dim3(2048), dim3(256), 0, 0, vec[i], n, unsigned(i + 131 * s));
    }
    CK(hipDeviceSynchronize());
    PArgs a{};
    a.n = n;
    a.alpha = alpha_dev;
    a.partial = partial;
    for (int i = 0; i < K; ++i) {
      a.xp[i] = vec[i];
      a.xa[i] = vec[K + i];
    }
    for (int j = 0; j < M; ++j) {
      a.yp[j] = vec[2 * K + j];
      a.ya[j] = vec[2 * K + M + j];
      a.e[j] = -0.5 - 0.1 * j;
    }
    // the library forms: one warm-up chain, then reps
    double dots_two[M], dots_one[M], probe_lib[256], probe[256];
    for (int which = 0; which < 2; ++which) {
      ssp_ctx* ctx = which ? one : two;
      double* dots = which ? dots_one : dots_two;
      std::vector<float> t;
      long long calls = 0;
      int others = 0;
      for (int r = 0; r <= reps; ++r) {
        const float ms = library_chain(ctx, a, alpha.data(), dots, &calls, &others);
        if (r) t.push_back(ms);
      }
      if (calls != 2 || others != 0) printf("  unexpected ledger: %lld gemm_outer calls, %d other launches\n", calls, others);
      rows[which].ms.push_back(median(t));
    }
    for (int j = 0; j < M; ++j)
      if (std::memcmp(&dots_two[j], &dots_one[j], 8) != 0) printf("  set %d: library dots differ at j = %d\n", s, j);
    CK(hipMemcpy(probe_lib, a.ya[M - 1] + probe_at, sizeof(probe_lib), hipMemcpyDeviceToHost));
    const auto cand = [&](int row, const std::function<void()>& f) {
      CK(hipMemset(a.ya[M - 1] + probe_at, 0, sizeof(probe)));
      rows[row].ms.push_back(timeit(f, reps));
      CK(hipMemcpy(probe, a.ya[M - 1] + probe_at, sizeof(probe), hipMemcpyDeviceToHost));
      if (std::memcmp(probe, probe_lib, sizeof(probe)) != 0) printf("  set %d: %s differs from the library\n", s, rows[row].name.c_str());
    };
    cand(2, [&] { hipLaunchKernelGGL((k_pair<false, 4>), dim3(grid), dim3(kBlock), 0, 0, a); });
    cand(3, [&] { hipLaunchKernelGGL((k_pair<false, 8>), dim3(grid), dim3(kBlock), 0, 0, a); });
    cand(4, [&] { hipLaunchKernelGGL((k_pair<true, 2>), dim3(grid), dim3(kBlock), 0, 0, a); });
    cand(5, [&] { hipLaunchKernelGGL((k_pair<true, 4>), dim3(grid), dim3(kBlock), 0, 0, a); });
    CK(hipGetLastError());
    SK(ssp_synchronize(two));
    SK(ssp_synchronize(one));
    for (double* v : vec) CK(hipFree(v));
    printf("set %d done\n", s);
    fflush(stdout);
  }
  printf("n = %zu, k = %d, m = %d, grid %d, median of %d per set; ms (GB/s) per vector set\n", n, K, M, grid, reps);
  for (const Row& r : rows) {
    printf("%-24s", r.name.c_str());
    for (float ms : r.ms) printf("  %7.3f (%6.1f)", ms, r.bytes / ms / 1e6);
    printf("\n");
  }
  for (void* p : pads) CK(hipFree(p));
  SK(ssp_ctx_destroy(two));
  SK(ssp_ctx_destroy(one));
  return 0;
}
