// grand_products.hip — the permutation and lookup grand products of the
// prover on the device: the per-row numerator / denominator terms, a batch
// inversion, and a chained prefix product that writes the z vectors.
// Included by taiga_gpu.cpp (single TU) after openings.hip.
//
// Everything here is exact Fp arithmetic through the TG_HD fd_* primitives,
// Montgomery form throughout; fd_* results are fully reduced, so any
// algebraically equal order of the multiplications gives the same bytes as
// the serial host loops of the oracle prover.
#pragma once
#include <hip/hip_runtime.h>

#include "pasta_device.hpp"

namespace taiga {

// capacities of the term tables; prover_gpu.inc asserts that they equal the
// limits pdesc_parse enforces
constexpr int GP_MAX_COLS = 32;
constexpr int GP_MAX_CHUNKS = 8;
constexpr int GP_MAX_LOOKUPS = 4;

// threads per block of every kernel here
constexpr int GP_B = 256;
// elements per thread of the batch inverse and of the scan. One fd_inv is
// ~320 dependent multiplies and every lane of a wave runs it in lockstep, so
// only the per-thread chain depth GP_E amortises it: a thread spends
// 320 + 3 * GP_E multiplies on GP_E elements. The flat array is 2-9 vectors
// of 2^15 - 6 elements, i.e. 64-288 blocks of 256 threads at GP_E = 4 on a
// 256-CU part: about one wave per SIMD, so the launch costs one inversion's
// latency (~0.45 ms) whatever GP_E is, plus the chain. Measured single-stream
// on the compliance circuit (profiles/README.md, round 5), gp_lookup_z stage
// wall: GP_E = 2 0.60 ms, 4 0.62 ms, 8 0.68 ms. 4 is kept: 2 buys its
// 0.02 ms with twice the inversions, which is SIMD time the other contexts'
// kernels lose when eight proofs share the chip.
#ifndef GP_E
#define GP_E 4
#endif
// elements one block covers
constexpr int GP_T = GP_B * GP_E;

// ---------------- index arithmetic (host-checkable) ----------------

// the batch inverse gives thread t of block b the elements
// b * GP_T + m * GP_B + t, m < GP_E: a block covers GP_T contiguous
// elements and the lanes of a wave read neighbouring ones
TG_HD long gp_inv_index(long block, int t, int m) {
  return block * (long)GP_T + (long)m * GP_B + t;
}
TG_HD long gp_blocks_for(long count) { return (count + GP_T - 1) / GP_T; }

// the scan gives thread t of a block the contiguous run
// [t * GP_E, min((t + 1) * GP_E, len)) of the block's len <= GP_T elements
TG_HD int gp_scan_lo(int t, int len) { return t * GP_E < len ? t * GP_E : len; }
TG_HD int gp_scan_hi(int t, int len) {
  return (t + 1) * GP_E < len ? (t + 1) * GP_E : len;
}

// ---------------- permutation terms ----------------

struct GpPermArgs {
  const Fp* cols[GP_MAX_COLS];   // v_j, Lagrange form
  const Fp* sigma[GP_MAX_COLS];  // sigma_j, Lagrange form
  Fp bdpow[GP_MAX_COLS];         // beta * delta^j
  Fp beta, gamma, omega;
  Fp* num;  // [chunk * u + i]
  Fp* den;
  long u;
  int n_perm, chunk_len;
};

// num[ch][i] = prod_j (v_j[i] + beta delta^j omega^i + gamma),
// den[ch][i] = prod_j (v_j[i] + beta sigma_j[i] + gamma) over chunk ch's
// columns; blockIdx.y is the chunk. A thread takes rows i0, i0 + stride, ..:
// omega^i0 from one power, then a walk by omega^stride.
__global__ void __launch_bounds__(GP_B) k_gp_perm_terms(const GpPermArgs* __restrict__ ap) {
  const GpPermArgs& A = *ap;
  const int ch = blockIdx.y;
  const int lo = ch * A.chunk_len;
  const int hi = lo + A.chunk_len < A.n_perm ? lo + A.chunk_len : A.n_perm;
  const long stride = (long)gridDim.x * GP_B;
  const long i0 = blockIdx.x * (long)GP_B + threadIdx.x;
  if (i0 >= A.u) return;
  const Fp beta = A.beta, gamma = A.gamma;
  Fp w = fd_pow_u64(A.omega, (u64)i0);
  const Fp wstep = fd_pow_u64(A.omega, (u64)stride);
  Fp* num = A.num + (size_t)ch * A.u;
  Fp* den = A.den + (size_t)ch * A.u;
  for (long i = i0; i < A.u; i += stride) {
    Fp pn = fd_one_mont<FpCfg>(), pdv = pn;
    for (int j = lo; j < hi; j++) {
      Fp vg = fd_add(A.cols[j][i], gamma);
      pn = fd_mul(pn, fd_add(fd_mul(A.bdpow[j], w), vg));
      pdv = fd_mul(pdv, fd_add(fd_mul(beta, A.sigma[j][i]), vg));
    }
    num[i] = pn;
    den[i] = pdv;
    w = fd_mul(w, wstep);
  }
}

// ---------------- lookup terms ----------------

struct GpLookupArgs {
  const Fp* a[GP_MAX_LOOKUPS];   // compressed input expression A
  const Fp* s[GP_MAX_LOOKUPS];   // compressed table expression S
  const Fp* ap[GP_MAX_LOOKUPS];  // permuted A'
  const Fp* sp[GP_MAX_LOOKUPS];  // permuted S'
  Fp beta, gamma;
  Fp* num;  // [lookup * u + i]
  Fp* den;
  long u;
};

// num = (A + beta)(S + gamma), den = (A' + beta)(S' + gamma); blockIdx.y is
// the lookup
__global__ void __launch_bounds__(GP_B) k_gp_lookup_terms(const GpLookupArgs* __restrict__ ap) {
  const GpLookupArgs& A = *ap;
  const int l = blockIdx.y;
  const Fp beta = A.beta, gamma = A.gamma;
  Fp* num = A.num + (size_t)l * A.u;
  Fp* den = A.den + (size_t)l * A.u;
  for (long i = blockIdx.x * (long)GP_B + threadIdx.x; i < A.u;
       i += (long)gridDim.x * GP_B) {
    num[i] = fd_mul(fd_add(A.a[l][i], beta), fd_add(A.s[l][i], gamma));
    den[i] = fd_mul(fd_add(A.ap[l][i], beta), fd_add(A.sp[l][i], gamma));
  }
}

// ---------------- batch inverse ----------------

// v[i] <- v[i]^-1 in place over one flat array; a zero stays zero and is
// left out of its thread's running product, so it does not touch its
// neighbours. Per thread: the running products of its GP_E elements (named
// registers: every index below is a compile-time constant), one fd_inv,
// then the backward pass.
__global__ void __launch_bounds__(GP_B) k_gp_batch_inverse(Fp* __restrict__ v, long count) {
  Fp x[GP_E], pre[GP_E];
  Fp run = fd_one_mont<FpCfg>();
#pragma unroll
  for (int m = 0; m < GP_E; m++) {
    long i = gp_inv_index(blockIdx.x, threadIdx.x, m);
    x[m] = i < count ? v[i] : fd_zero<FpCfg>();
    pre[m] = run;
    if (!fd_is_zero(x[m])) run = fd_mul(run, x[m]);
  }
  Fp inv = fd_inv(run);
#pragma unroll
  for (int m = GP_E - 1; m >= 0; m--) {
    if (fd_is_zero(x[m])) continue;
    long i = gp_inv_index(blockIdx.x, threadIdx.x, m);
    v[i] = fd_mul(inv, pre[m]);
    inv = fd_mul(inv, x[m]);
  }
}

// ---------------- chained prefix product ----------------

// One block of the scan: len <= GP_T ratios starting at flat index start,
// never crossing a segment; dst points at the z element of the first one.
struct GpScanBlock {
  long start;
  Fp* dst;
  int len;
  int last;  // the segment ends with this block: it also writes dst[len]
};
// A chain: the blocks [blk_lo, blk_hi) multiply on from init, whatever
// segments they belong to
struct GpScanChain {
  Fp init;
  int blk_lo, blk_hi;
};

// ratio i is a[i] * b[i], or a[i] alone when b is null (the fused
// num * den^-1 of the prover)
__device__ __forceinline__ Fp gp_ratio(const Fp* __restrict__ a, const Fp* __restrict__ b,
                                       long i) {
  return b ? fd_mul(a[i], b[i]) : a[i];
}

// pass 1: bp[block] = product of the block's ratios
__global__ void __launch_bounds__(GP_B) k_gp_scan_reduce(const GpScanBlock* __restrict__ blocks,
                                                         const Fp* __restrict__ a,
                                                         const Fp* __restrict__ b,
                                                         Fp* __restrict__ bp) {
  __shared__ Fp sh[GP_B];
  const GpScanBlock bk = blocks[blockIdx.x];
  const int t = threadIdx.x;
  const int lo = gp_scan_lo(t, bk.len), hi = gp_scan_hi(t, bk.len);
  Fp p = fd_one_mont<FpCfg>();
  for (int i = lo; i < hi; i++) p = fd_mul(p, gp_ratio(a, b, bk.start + i));
  sh[t] = p;
  for (int s = GP_B / 2; s > 0; s >>= 1) {
    __syncthreads();
    if (t < s) {
      p = fd_mul(p, sh[t + s]);
      sh[t] = p;
    }
  }
  if (t == 0) bp[blockIdx.x] = p;
}

// pass 2, one block per chain: off[b] = init * prod of bp over the chain's
// blocks before b. Per thread a contiguous run of block products, an
// exclusive scan of the run products over the block, then the walk.
__global__ void __launch_bounds__(GP_B) k_gp_scan_offsets(const GpScanChain* __restrict__ chains,
                                                          const Fp* __restrict__ bp,
                                                          Fp* __restrict__ off) {
  __shared__ Fp sh[GP_B];
  const GpScanChain cn = chains[blockIdx.x];
  const int t = threadIdx.x;
  const int cnt = cn.blk_hi - cn.blk_lo;
  const int run = (cnt + GP_B - 1) / GP_B;
  const int lo = cn.blk_lo + (t * run < cnt ? t * run : cnt);
  const int hi = cn.blk_lo + ((t + 1) * run < cnt ? (t + 1) * run : cnt);
  Fp p = fd_one_mont<FpCfg>();
  for (int i = lo; i < hi; i++) p = fd_mul(p, bp[i]);
  sh[t] = p;
  for (int o = 1; o < GP_B; o <<= 1) {
    __syncthreads();
    const bool has = t >= o;
    Fp q = fd_zero<FpCfg>();
    if (has) q = sh[t - o];
    __syncthreads();
    if (has) {
      p = fd_mul(p, q);
      sh[t] = p;
    }
  }
  __syncthreads();
  Fp cur = t > 0 ? fd_mul(cn.init, sh[t - 1]) : cn.init;
  for (int i = lo; i < hi; i++) {
    off[i] = cur;
    cur = fd_mul(cur, bp[i]);
  }
}

// pass 3: dst[i] = off[block] * prod of the block's ratios before i; the
// block that ends a segment also writes the value after its last ratio
__global__ void __launch_bounds__(GP_B) k_gp_scan_apply(const GpScanBlock* __restrict__ blocks,
                                                        const Fp* __restrict__ a,
                                                        const Fp* __restrict__ b,
                                                        const Fp* __restrict__ off) {
  __shared__ Fp sh[GP_B];
  const GpScanBlock bk = blocks[blockIdx.x];
  const int t = threadIdx.x;
  const int lo = gp_scan_lo(t, bk.len), hi = gp_scan_hi(t, bk.len);
  Fp r[GP_E];
  Fp p = fd_one_mont<FpCfg>();
#pragma unroll
  for (int m = 0; m < GP_E; m++) {
    r[m] = lo + m < hi ? gp_ratio(a, b, bk.start + lo + m) : fd_one_mont<FpCfg>();
    p = fd_mul(p, r[m]);
  }
  sh[t] = p;
  for (int o = 1; o < GP_B; o <<= 1) {
    __syncthreads();
    const bool has = t >= o;
    Fp q = fd_zero<FpCfg>();
    if (has) q = sh[t - o];
    __syncthreads();
    if (has) {
      p = fd_mul(p, q);
      sh[t] = p;
    }
  }
  __syncthreads();
  const Fp base = off[blockIdx.x];
  Fp cur = t > 0 ? fd_mul(base, sh[t - 1]) : base;
#pragma unroll
  for (int m = 0; m < GP_E; m++) {
    if (lo + m < hi) {
      bk.dst[lo + m] = cur;
      cur = fd_mul(cur, r[m]);
    }
  }
  // the thread that holds the segment's last ratio
  if (bk.last && hi == bk.len && lo < hi) bk.dst[bk.len] = cur;
}

}  // namespace taiga
