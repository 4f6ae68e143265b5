// openings.hip — the opening phase of the prover on the device: batched
// polynomial evaluation, Horner combinations of coefficient vectors, Kate
// division, and the IPA round kernels. Included by taiga_gpu.cpp (single TU)
// after ntt.hip.
//
// Everything here is exact Fp arithmetic through the same TG_HD fd_*
// primitives the host uses; fd_* results are fully reduced, so any
// algebraically equal evaluation order gives the same bytes as the serial
// host loops of the oracle prover (and of the verifier's ppoly_eval).
#pragma once
#include <hip/hip_runtime.h>

#include "pasta_device.hpp"

namespace taiga {

// threads per block of the one-block-per-job kernels (evaluation, division):
// a job's vector is cut into OPN_T contiguous chunks, one per thread
constexpr int OPN_T = 512;

// ---------------- batched evaluation ----------------

struct EvalQuery {
  const Fp* poly;  // coefficient form, Montgomery
  long len;
  Fp x;
};

// out[q] = sum_i poly_q[i] * x_q^i. One block per query: each thread runs
// Horner over its chunk, then the block tree-combines the chunk values —
// level s adds partial[t + s] * x^(chunk * s) into partial[t], so the one
// multiplier every thread needs is squared per level and no thread computes
// a power of its own index.
__global__ void __launch_bounds__(OPN_T) k_poly_eval_batch(const EvalQuery* __restrict__ qs,
                                                           Fp* __restrict__ out) {
  __shared__ Fp part[OPN_T];
  const EvalQuery q = qs[blockIdx.x];
  const int t = threadIdx.x;
  long chunk = (q.len + OPN_T - 1) / OPN_T;
  if (chunk < 1) chunk = 1;
  long lo = t * chunk, hi = lo + chunk < q.len ? lo + chunk : q.len;
  Fp acc = fd_zero<FpCfg>();
  for (long i = hi - 1; i >= lo; i--) acc = fd_add(fd_mul(acc, q.x), q.poly[i]);
  part[t] = acc;
  Fp xs = fd_pow_u64(q.x, (u64)chunk);
  for (int s = 1; s < OPN_T; s <<= 1) {
    __syncthreads();
    if ((t & (2 * s - 1)) == 0) {
      acc = fd_add(acc, fd_mul(part[t + s], xs));
      part[t] = acc;
    }
    xs = fd_sqr(xs);
  }
  if (t == 0) out[blockIdx.x] = acc;
}

// ---------------- Horner combination of vectors ----------------

// out[i] = (..(p0[i] * c + p1[i]) * c + ..) * c + p_{np-1}[i]; out may alias
// any of the inputs (each element is read before it is written).
__global__ void __launch_bounds__(256) k_horner_comb(const Fp* const* polys, int np, Fp c,
                                                     Fp* out, long n) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x) {
    Fp acc = polys[0][i];
    for (int j = 1; j < np; j++) acc = fd_add(fd_mul(acc, c), polys[j][i]);
    out[i] = acc;
  }
}

// ---------------- Kate division ----------------

struct KateJob {
  const Fp* src;  // len coefficients
  Fp* dst;        // may be src: a thread reads and writes only its own chunk
  long len;
  Fp pt;
};

// dst = src / (X - pt), remainder dropped: dst[i] = sum_{j>i} src[j] pt^(j-i-1)
// for i < len - 1, and dst[len-1] = 0 — the serial recurrence
// q[i-1] = a[i] + pt * q[i] in a blocked two-pass form. One block per job: per-thread chunk Horner and pt^chunk, a suffix scan of
// the (value, power) pairs over the block for the carry into each chunk,
// then the recurrence over the chunk from that carry.
__global__ void __launch_bounds__(OPN_T) k_kate_div(const KateJob* __restrict__ jobs) {
  __shared__ Fp shL[OPN_T];
  __shared__ Fp shP[OPN_T];
  const KateJob jb = jobs[blockIdx.x];
  const int t = threadIdx.x;
  long chunk = (jb.len + OPN_T - 1) / OPN_T;
  if (chunk < 1) chunk = 1;
  long lo = t * chunk, hi = lo + chunk < jb.len ? lo + chunk : jb.len;
  Fp L = fd_zero<FpCfg>();
  for (long i = hi - 1; i >= lo; i--) L = fd_add(fd_mul(L, jb.pt), jb.src[i]);
  Fp P = fd_pow_u64(jb.pt, hi > lo ? (u64)(hi - lo) : 0);
  shL[t] = L;
  shP[t] = P;
  // inclusive suffix scan: after it shL[t] is the Horner value of chunks
  // t.. in pt, relative to chunk t's first index
  for (int off = 1; off < OPN_T; off <<= 1) {
    __syncthreads();
    const bool has = t + off < OPN_T;
    Fp l2 = fd_zero<FpCfg>(), p2 = fd_zero<FpCfg>();
    if (has) {
      l2 = shL[t + off];
      p2 = shP[t + off];
    }
    __syncthreads();
    if (has) {
      L = fd_add(L, fd_mul(P, l2));
      P = fd_mul(P, p2);
      shL[t] = L;
      shP[t] = P;
    }
  }
  __syncthreads();
  Fp prev = t + 1 < OPN_T ? shL[t + 1] : fd_zero<FpCfg>();
  for (long i = hi - 1; i >= lo; i--) {
    Fp a = jb.src[i];
    jb.dst[i] = prev;
    prev = fd_add(a, fd_mul(jb.pt, prev));
  }
}

// ---------------- IPA ----------------

constexpr int OPN_POW_CHUNK = 8;

// out[i] = x^i, i < n: one power per thread for its first index, then a walk
__global__ void __launch_bounds__(256) k_fill_powers(Fp* out, long n, Fp x) {
  long i0 = (blockIdx.x * (long)blockDim.x + threadIdx.x) * OPN_POW_CHUNK;
  if (i0 >= n) return;
  Fp cur = fd_pow_u64(x, (u64)i0);
  for (long i = i0; i < n && i < i0 + OPN_POW_CHUNK; i++) {
    out[i] = cur;
    cur = fd_mul(cur, x);
  }
}

__global__ void __launch_bounds__(256) k_fill_const(Fp* out, long n, Fp v) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x)
    out[i] = v;
}

// One IPA round's MSM scalars and inner products. sc holds the two n-long
// scalar vectors sl | sr in CANONICAL form (what the MSM digit kernel
// reads): over the n original bases, with cur = 2 * half,
//   sl[t] = wfold[t] * pp[half + ci], sr[t] = 0           if ci <  half
//   sl[t] = 0, sr[t] = wfold[t] * pp[ci - half]           if ci >= half
// where ci = t & (cur - 1). partials[2b], partials[2b+1] are block b's share
// of <pp[half..], bvec[..half]> and <pp[..half], bvec[half..]> (Montgomery);
// the caller adds the gridDim.x pairs up.
__global__ void __launch_bounds__(256) k_ipa_prepare(const Fp* __restrict__ pp,
                                                     const Fp* __restrict__ bvec,
                                                     const Fp* __restrict__ wfold, long n,
                                                     long half, Fp* __restrict__ sc,
                                                     Fp* __restrict__ partials) {
  __shared__ Fp shl[256];
  __shared__ Fp shr[256];
  const long stride = (long)gridDim.x * blockDim.x;
  const long g0 = blockIdx.x * (long)blockDim.x + threadIdx.x;
  const long cur = half * 2;
  const Fp zero = fd_zero<FpCfg>();
  for (long t = g0; t < n; t += stride) {
    long ci = t & (cur - 1);
    // ci < half pairs with pp[half + ci], ci >= half with pp[ci - half]
    Fp v = fd_from_mont(fd_mul(wfold[t], pp[ci ^ half]));
    long own = ci < half ? t : n + t, other = ci < half ? n + t : t;
    sc[own] = v;
    sc[other] = zero;
  }
  Fp vl = zero, vr = zero;
  for (long i = g0; i < half; i += stride) {
    vl = fd_add(vl, fd_mul(pp[half + i], bvec[i]));
    vr = fd_add(vr, fd_mul(pp[i], bvec[half + i]));
  }
  const int t = threadIdx.x;
  shl[t] = vl;
  shr[t] = vr;
  for (int s = 128; s > 0; s >>= 1) {
    __syncthreads();
    if (t < s) {
      vl = fd_add(vl, shl[t + s]);
      vr = fd_add(vr, shr[t + s]);
      shl[t] = vl;
      shr[t] = vr;
    }
  }
  if (t == 0) {
    partials[2 * blockIdx.x] = vl;
    partials[2 * blockIdx.x + 1] = vr;
  }
}

// the fold that ends a round, from the challenge u and its inverse:
// wfold[t] *= uinv where t & topbit; pp and bvec fold over half
__global__ void __launch_bounds__(256) k_ipa_fold(Fp* pp, Fp* bvec, Fp* wfold, long n,
                                                  long half, long topbit, Fp u, Fp uinv) {
  for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < n;
       t += (long)gridDim.x * blockDim.x) {
    if (t & topbit) wfold[t] = fd_mul(wfold[t], uinv);
    if (t < half) {
      pp[t] = fd_add(pp[t], fd_mul(pp[half + t], u));
      bvec[t] = fd_add(bvec[t], fd_mul(bvec[half + t], uinv));
    }
  }
}

// grid of the n-wide elementwise kernels above; k_ipa_prepare's partials
// array holds 2 * OPN_GRID_MAX elements
constexpr int OPN_GRID_MAX = 128;
static inline int opn_grid(long work) {
  long blocks = (work + 255) / 256;
  if (blocks > OPN_GRID_MAX) blocks = OPN_GRID_MAX;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}

static inline void fill_powers_launch(Fp* out, long n, const Fp& x, hipStream_t stream) {
  long threads = (n + OPN_POW_CHUNK - 1) / OPN_POW_CHUNK;
  hipLaunchKernelGGL(k_fill_powers, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0,
                     stream, out, n, x);
}

}  // namespace taiga
