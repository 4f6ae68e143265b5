// standalone micro-benchmark of the field multiply's forms on gfx950: the
// 4x64 CIOS fd_mul_int (the host's form), the radix-2^30 fd_mul_r30 /
// fd_sqr_r30 (the device's form; all three in pasta_device.hpp) and the
// FP64-limb experiment fd_mul_f52 / fd_sqr_f52 (fd52.hpp, not shipped), by
// the method of fd28_bench.hip (2^20 threads x ITER multiplies, three timed
// launches).
//   chain: ITER dependent multiplies per thread (latency-shaped)
//   x4:    4 independent multiplies per step, as in a point addition
//          (throughput-shaped); ITER/4 steps, so the same multiply count
// The last thread's result of every variant is compared with the integer
// chain's, so a wrong multiply cannot post a time.
// Results: profiles/README.md, Round 8.
#include <cstdio>
#include <cstring>
#include <hip/hip_runtime.h>
#include "pasta_device.hpp"
#include "fd52.hpp"
using namespace taiga;

constexpr int ITER = 512;

enum Var { INT_MUL, F52_MUL, F52_SQR, INT_SQR, R30_MUL, R30_SQR };
static const char* kVar[] = {"fd_mul_int", "fd_mul_f52", "fd_sqr_f52", "fd_mul_int(a,a)",
                             "fd_mul_r30", "fd_sqr_r30"};

template <int V>
__device__ __forceinline__ Fq op(const Fq& a, const Fq& b) {
  if constexpr (V == INT_MUL) return fd_mul_int(a, b);
  else if constexpr (V == F52_MUL) return fd_mul_f52(a, b);
  else if constexpr (V == F52_SQR) return fd_sqr_f52(a);
  else if constexpr (V == R30_MUL) return fd_mul_r30(a, b);
  else if constexpr (V == R30_SQR) return fd_sqr_r30(a);
  else return fd_mul_int(a, a);
}

template <int V>
__global__ void __launch_bounds__(256) kb_chain(const Fq* in, Fq* out, u64 n) {
  u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fq a = in[i], b = in[(i + 1) % n];
#pragma unroll 1
  for (int k = 0; k < ITER; k++) a = op<V>(a, b);
  out[i] = a;
}

template <int V>
__global__ void __launch_bounds__(256) kb_x4(const Fq* in, Fq* out, u64 n) {
  u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fq a0 = in[i], a1 = in[(i + 1) % n], a2 = in[(i + 2) % n], a3 = in[(i + 3) % n];
#pragma unroll 1
  for (int k = 0; k < ITER / 4; k++) {
    Fq t0 = op<V>(a0, a1), t1 = op<V>(a1, a2), t2 = op<V>(a2, a3), t3 = op<V>(a3, a0);
    a0 = t0; a1 = t1; a2 = t2; a3 = t3;
  }
  out[i] = fd_add(fd_add(a0, a1), fd_add(a2, a3));
}

template <class K>
static void time3(const char* shape, const char* name, K kern, const Fq* in, Fq* out, u64 n,
                  Fq* last) {
  dim3 grid((unsigned)((n + 255) / 256)), block(256);
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  hipLaunchKernelGGL(kern, grid, block, 0, 0, in, out, n);  // warm-up
  hipDeviceSynchronize();
  float ms[3];
  for (int r = 0; r < 3; r++) {
    hipEventRecord(e0);
    hipLaunchKernelGGL(kern, grid, block, 0, 0, in, out, n);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    hipEventElapsedTime(&ms[r], e0, e1);
  }
  hipMemcpy(last, out + (n - 1), sizeof(Fq), hipMemcpyDeviceToHost);
  float lo = ms[0], hi = ms[0];
  for (int r = 1; r < 3; r++) { lo = ms[r] < lo ? ms[r] : lo; hi = ms[r] > hi ? ms[r] : hi; }
  printf("%-5s %-16s %8.3f %8.3f %8.3f ms  (%.3f ns/mul/thread at the fastest, %.2e mul/s)\n",
         shape, name, ms[0], ms[1], ms[2], lo * 1e6 / ((double)n * ITER),
         (double)n * ITER / (lo * 1e-3));
}

int main() {
  const u64 n = 1 << 20;
  Fq *in, *out;
  if (hipMalloc(&in, n * sizeof(Fq)) != hipSuccess || hipMalloc(&out, n * sizeof(Fq)) != hipSuccess)
    return 1;
  // 0x35.. in the top limb is below the modulus' 0x40..: canonical inputs
  hipMemset(in, 0x35, n * sizeof(Fq));
  Fq h = {{0x0123456789abcdefULL, 0xfedcba9876543210ULL, 0x0f1e2d3c4b5a6978ULL,
           0x1122334455667788ULL}};
  hipMemcpy(in, &h, sizeof h, hipMemcpyHostToDevice);  // in[0]: chain operand of thread n-1
  Fq ref, got;
  int bad = 0;
  time3("chain", kVar[INT_MUL], kb_chain<INT_MUL>, in, out, n, &ref);
  time3("chain", kVar[F52_MUL], kb_chain<F52_MUL>, in, out, n, &got);
  bad += memcmp(&ref, &got, sizeof ref) != 0;
  time3("chain", kVar[R30_MUL], kb_chain<R30_MUL>, in, out, n, &got);
  bad += memcmp(&ref, &got, sizeof ref) != 0;
  time3("chain", kVar[INT_SQR], kb_chain<INT_SQR>, in, out, n, &ref);
  time3("chain", kVar[F52_SQR], kb_chain<F52_SQR>, in, out, n, &got);
  bad += memcmp(&ref, &got, sizeof ref) != 0;
  time3("chain", kVar[R30_SQR], kb_chain<R30_SQR>, in, out, n, &got);
  bad += memcmp(&ref, &got, sizeof ref) != 0;
  time3("x4", kVar[INT_MUL], kb_x4<INT_MUL>, in, out, n, &ref);
  time3("x4", kVar[F52_MUL], kb_x4<F52_MUL>, in, out, n, &got);
  bad += memcmp(&ref, &got, sizeof ref) != 0;
  time3("x4", kVar[R30_MUL], kb_x4<R30_MUL>, in, out, n, &got);
  bad += memcmp(&ref, &got, sizeof ref) != 0;
  time3("x4", kVar[INT_SQR], kb_x4<INT_SQR>, in, out, n, &ref);
  time3("x4", kVar[F52_SQR], kb_x4<F52_SQR>, in, out, n, &got);
  bad += memcmp(&ref, &got, sizeof ref) != 0;
  time3("x4", kVar[R30_SQR], kb_x4<R30_SQR>, in, out, n, &got);
  bad += memcmp(&ref, &got, sizeof ref) != 0;
  printf(bad ? "MISMATCH in %d variants\n" : "all variants agree with the integer form\n", bad);
  return bad || hipDeviceSynchronize() != hipSuccess;
}
