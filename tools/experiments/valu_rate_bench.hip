// standalone micro-benchmark: issue cost of the VALU instructions a field
// multiply is made of, on gfx950. 2^20 threads in blocks of 256 (full
// occupancy); each thread runs 8 independent chains of ITER steps of one
// instruction, so the time per wave-instruction is the pipe's issue rate and
// not its latency. Plain C++ and builtins; check with
//   hipcc -O3 --offload-arch=gfx950 --offload-device-only -S
// that each loop body holds the intended instruction (8 per step; the
// 128-bit add is one v_add_co + three v_addc_co).
// Results: profiles/README.md, Round 8.
#include <cstdio>
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef uint64_t u64;
typedef uint32_t u32;
typedef unsigned __int128 u128;

constexpr int ITER = 512;
constexpr int CH = 8;

enum Op { MAD_U64_U32, MUL_LO_U32, MUL_HI_U32, FMA_F64, ADD_F64, LSHL_ADD_U64, ADD128, NOPS };
static const char* kName[NOPS] = {"v_mad_u64_u32", "v_mul_lo_u32", "v_mul_hi_u32", "v_fma_f64",
                                  "v_add_f64", "v_lshl_add_u64", "add_co+3*addc_co"};
static const int kInstr[NOPS] = {1, 1, 1, 1, 1, 1, 4};  // instructions per chain step

template <int OP>
__global__ void __launch_bounds__(256) k_rate(u64* io, u64 n) {
  u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
  if (i >= n) return;
  u64 seed = io[i];
  u64 y = io[(i + 1) % n] | 1;
  if constexpr (OP == MAD_U64_U32) {
    u64 x[CH];
    for (int c = 0; c < CH; c++) x[c] = seed + c;
    u32 m = (u32)y;
    for (int k = 0; k < ITER; k++)
#pragma unroll
      for (int c = 0; c < CH; c++) x[c] = (u64)(u32)x[c] * m + x[c];
    u64 r = 0;
    for (int c = 0; c < CH; c++) r ^= x[c];
    io[i] = r;
  } else if constexpr (OP == MUL_LO_U32 || OP == MUL_HI_U32) {
    u32 x[CH];
    for (int c = 0; c < CH; c++) x[c] = (u32)seed + c;
    u32 m = (u32)y;
    for (int k = 0; k < ITER; k++)
#pragma unroll
      // mul_lo by the neighbouring chain: a loop-invariant factor is folded into
      // one multiply by its power
      for (int c = 0; c < CH; c++)
        x[c] = OP == MUL_LO_U32 ? x[c] * x[(c + 1) % CH] : __umulhi(x[c], m);
    u32 r = 0;
    for (int c = 0; c < CH; c++) r ^= x[c];
    io[i] = r;
  } else if constexpr (OP == FMA_F64 || OP == ADD_F64) {
    double x[CH];
    for (int c = 0; c < CH; c++) x[c] = (double)(seed & 0xffff) + c;
    double m = (double)(y & 0xff) * 0x1p-8, a = (double)(y & 0xfff);
    for (int k = 0; k < ITER; k++)
#pragma unroll
      for (int c = 0; c < CH; c++) x[c] = OP == FMA_F64 ? __builtin_fma(x[c], m, a) : x[c] + a;
    double r = 0;
    for (int c = 0; c < CH; c++) r += x[c];
    io[i] = (u64)r;
  } else if constexpr (OP == LSHL_ADD_U64) {
    u64 x[CH];
    for (int c = 0; c < CH; c++) x[c] = seed + c;
    for (int k = 0; k < ITER; k++)
#pragma unroll
      for (int c = 0; c < CH; c++) x[c] = (x[c] << 1) + x[(c + 1) % CH];
    u64 r = 0;
    for (int c = 0; c < CH; c++) r ^= x[c];
    io[i] = r;
  } else {
    u128 x[CH];
    for (int c = 0; c < CH; c++) x[c] = ((u128)seed << 64) | (seed + c);
    x[0] |= ((u128)y << 64) | ~y;
    // each chain adds its neighbour: a constant addend would be folded
    // into one closed-form add for the whole loop
    for (int k = 0; k < ITER; k++)
#pragma unroll
      for (int c = 0; c < CH; c++) x[c] += x[(c + 1) % CH];
    u128 r = 0;
    for (int c = 0; c < CH; c++) r ^= x[c];
    io[i] = (u64)r ^ (u64)(r >> 64);
  }
}

template <int OP>
static void run(u64* d, u64 n, double simds, double ghz) {
  dim3 grid((unsigned)(n / 256)), block(256);
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  hipLaunchKernelGGL(k_rate<OP>, grid, block, 0, 0, d, n);  // warm-up
  hipDeviceSynchronize();
  float best = 1e30f, worst = 0;
  for (int r = 0; r < 3; r++) {
    hipEventRecord(e0);
    hipLaunchKernelGGL(k_rate<OP>, grid, block, 0, 0, d, n);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms;
    hipEventElapsedTime(&ms, e0, e1);
    best = ms < best ? ms : best;
    worst = ms > worst ? ms : worst;
  }
  double wave_instr = (double)(n / 64) * CH * ITER * kInstr[OP];
  double ns = best * 1e6 * simds / wave_instr;  // per wave-instruction on one SIMD
  printf("%-18s %8.3f ms (max %8.3f)  %6.2f ns/wave-instr/SIMD  %5.2f cycles at %.2f GHz\n",
         kName[OP], best, worst, ns, ns * ghz, ghz);
}

int main() {
  const u64 n = 1 << 20;
  u64* d;
  if (hipMalloc(&d, n * sizeof(u64)) != hipSuccess) {
    fprintf(stderr, "no device memory\n");
    return 1;
  }
  hipMemset(d, 0x35, n * sizeof(u64));
  int cus = 0, khz = 0;
  hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0);
  hipDeviceGetAttribute(&khz, hipDeviceAttributeClockRate, 0);
  double simds = 4.0 * cus, ghz = khz * 1e-6;
  printf("CUs %d, SIMDs %.0f, peak clock %.2f GHz; %llu threads x %d chains x %d steps\n", cus,
         simds, ghz, (unsigned long long)n, CH, ITER);
  run<MAD_U64_U32>(d, n, simds, ghz);
  run<MUL_LO_U32>(d, n, simds, ghz);
  run<MUL_HI_U32>(d, n, simds, ghz);
  run<FMA_F64>(d, n, simds, ghz);
  run<ADD_F64>(d, n, simds, ghz);
  run<LSHL_ADD_U64>(d, n, simds, ghz);
  run<ADD128>(d, n, simds, ghz);
  return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
