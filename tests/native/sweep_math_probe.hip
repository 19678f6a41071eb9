// sweep_math_probe.hip — TEST probe of carmel_amd/csrc/sweep_math.hpp: the product's own exp_le0, log_ge1 and Lse (the header
// is included, not copied), one thread per element on the GPU and a plain loop on the host.  tests/native/Makefile builds
// this file twice: libsweepprobe.so with the flags of kernels.o / tile_sweep.o (the compiler's default contraction) and
// libsweepprobe_nc.so with those of decode_sum.o (-ffp-contract=off).  Not part of the product library.
//
//   int sweep_probe_exp_device(const double* x, double* y, int64_t n);     y[i] = exp_le0(x[i])
//   int sweep_probe_log_device(const double* x, double* y, int64_t n);     y[i] = log_ge1(x[i])
//   int sweep_probe_lse_device(const double* terms, const int64_t* off, int64_t n_rows, double* value, double* m, double* acc);
//       row r = terms[off[r] .. off[r + 1]) added in that order to a fresh Lse; value(), m and acc of each row
//   the same three with _host: the same functions evaluated by the CPU
// Every entry point returns 0 or the failing call's hipError_t (-1: a bad argument).  The device ones allocate, copy and
// synchronise for themselves.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../carmel_amd/csrc/sweep_math.hpp"

using namespace carmel_hip;

namespace {

__global__ void exp_kernel(const double* __restrict__ x, double* __restrict__ y, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = exp_le0(x[i]);
}
__global__ void log_kernel(const double* __restrict__ x, double* __restrict__ y, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = log_ge1(x[i]);
}
__host__ __device__ inline void lse_row(const double* terms, const int64_t* off, int64_t r, double* value, double* m, double* acc) {
  Lse l;
  l.init();
  for (int64_t k = off[r]; k < off[r + 1]; ++k) l.add(terms[k]);
  value[r] = l.value();
  m[r] = l.m;
  acc[r] = l.acc;
}
__global__ void lse_kernel(const double* __restrict__ terms, const int64_t* __restrict__ off, int64_t n_rows,
                           double* __restrict__ value, double* __restrict__ m, double* __restrict__ acc) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n_rows) lse_row(terms, off, r, value, m, acc);
}

// device buffers of one call: whatever was allocated is freed on every way out
struct Bufs {
  void* p[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  int n = 0;
  hipError_t get(void** out, size_t bytes) {
    hipError_t e = hipMalloc(out, bytes ? bytes : 8);
    if (e == hipSuccess) p[n++] = *out;
    return e;
  }
  ~Bufs() {
    for (int i = 0; i < n; ++i) (void)hipFree(p[i]);
  }
};
#define PROBE_CHECK(call)                  \
  do {                                     \
    hipError_t e_ = (call);                \
    if (e_ != hipSuccess) return (int)e_; \
  } while (0)

constexpr int BLOCK = 256;
constexpr int64_t MAX_N = (int64_t)1 << 30;  // (one launch: the grid stays far below 2^31 blocks)

template <class K>
int map_device(K kernel, const double* x, double* y, int64_t n) {
  if (n < 0 || n > MAX_N || (n && (!x || !y))) return -1;
  if (n == 0) return 0;
  Bufs b;
  double *dx, *dy;
  PROBE_CHECK(b.get((void**)&dx, n * sizeof(double)));
  PROBE_CHECK(b.get((void**)&dy, n * sizeof(double)));
  PROBE_CHECK(hipMemcpy(dx, x, n * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(kernel, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, 0, dx, dy, n);
  PROBE_CHECK(hipGetLastError());
  PROBE_CHECK(hipDeviceSynchronize());
  PROBE_CHECK(hipMemcpy(y, dy, n * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

// the rows must tile terms[0 .. off[n_rows]) in order: no kernel is launched over offsets that do not
int check_rows(const int64_t* off, int64_t n_rows) {
  if (n_rows < 0 || n_rows > MAX_N || !off || off[0] != 0) return -1;
  for (int64_t r = 0; r < n_rows; ++r)
    if (off[r + 1] < off[r]) return -1;
  return off[n_rows] > MAX_N ? -1 : 0;
}

}  // namespace

extern "C" {

int sweep_probe_exp_device(const double* x, double* y, int64_t n) { return map_device(exp_kernel, x, y, n); }
int sweep_probe_log_device(const double* x, double* y, int64_t n) { return map_device(log_kernel, x, y, n); }

int sweep_probe_lse_device(const double* terms, const int64_t* off, int64_t n_rows, double* value, double* m, double* acc) {
  if (check_rows(off, n_rows) || !value || !m || !acc) return -1;
  if (n_rows == 0) return 0;
  const int64_t nt = off[n_rows];
  if (nt && !terms) return -1;
  Bufs b;
  double *dt, *dv, *dm, *da;
  int64_t* doff;
  PROBE_CHECK(b.get((void**)&dt, nt * sizeof(double)));
  PROBE_CHECK(b.get((void**)&doff, (n_rows + 1) * sizeof(int64_t)));
  PROBE_CHECK(b.get((void**)&dv, n_rows * sizeof(double)));
  PROBE_CHECK(b.get((void**)&dm, n_rows * sizeof(double)));
  PROBE_CHECK(b.get((void**)&da, n_rows * sizeof(double)));
  if (nt) PROBE_CHECK(hipMemcpy(dt, terms, nt * sizeof(double), hipMemcpyHostToDevice));
  PROBE_CHECK(hipMemcpy(doff, off, (n_rows + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(lse_kernel, dim3((unsigned)((n_rows + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, 0, dt, doff, n_rows, dv, dm, da);
  PROBE_CHECK(hipGetLastError());
  PROBE_CHECK(hipDeviceSynchronize());
  PROBE_CHECK(hipMemcpy(value, dv, n_rows * sizeof(double), hipMemcpyDeviceToHost));
  PROBE_CHECK(hipMemcpy(m, dm, n_rows * sizeof(double), hipMemcpyDeviceToHost));
  PROBE_CHECK(hipMemcpy(acc, da, n_rows * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int sweep_probe_exp_host(const double* x, double* y, int64_t n) {
  if (n < 0 || (n && (!x || !y))) return -1;
  for (int64_t i = 0; i < n; ++i) y[i] = exp_le0(x[i]);
  return 0;
}
int sweep_probe_log_host(const double* x, double* y, int64_t n) {
  if (n < 0 || (n && (!x || !y))) return -1;
  for (int64_t i = 0; i < n; ++i) y[i] = log_ge1(x[i]);
  return 0;
}
int sweep_probe_lse_host(const double* terms, const int64_t* off, int64_t n_rows, double* value, double* m, double* acc) {
  if (check_rows(off, n_rows) || !value || !m || !acc || (off[n_rows] && !terms)) return -1;
  for (int64_t r = 0; r < n_rows; ++r) lse_row(terms, off, r, value, m, acc);
  return 0;
}

}  // extern "C"
