// msm.hip — Pippenger variable-base MSM over Vesta for gfx950. PRODUCT CODE.
//
// MI355X-native replacement for halo2_proofs' best_multiexp on the
// create_proof hot path (26+ MSM(2^15) per proof; config 2
// of BASELINE.json: 2^20 microbench). Parity: vs the CPU oracle, which is
// pinned to the reference SRS (tests/test_srs_pin.py, test_gpu_parity.py).
//
// Plan (all device-side, HBM-bound integer work, no MFMA):
//   1. k_digits       : 16-bit signed window digits per (point, window),
//                       histogram via atomics
//   2. scan           : exclusive prefix sum over the 16x32768 histogram
//   3. k_scatter      : counting-sort point indices by bucket
//   4. k_bucket_acc   : one thread per bucket, mixed adds (gathers 64 B
//                       affine points — the ceil(255/w)*n*68 B bytes model)
//   5. k_bucket_segsum: per-segment running sums (tot, Y), reduced per
//                       256-segment chunk to T, S and the bit planes of Y
//   6. k_window_sum   : chunk results -> one sum per bucket set
//
// There is one launch chain (msm_run) and two plans for it (MsmPlan). The
// generic plan keeps a bucket set per window, so an MSM comes back as nwin
// window sums and the host shim does the double-and-add combine. The
// fixed-base plan gathers from a table of window-shifted SRS bases into ONE
// bucket set: the MSM comes back as one point and there is nothing to
// combine. msm_finish turns either answer into the MSM's Jacobian point.
//
// Scalars arrive in canonical (standard) form — digit extraction needs no
// Montgomery conversion. Points live device-resident as Montgomery affine
// 64 B AoS (good 64-byte random-gather granularity).

#include "pasta_device.hpp"

namespace taiga {

// window size c and reduce-segment length are runtime parameters chosen by
// MSM size: c=16 for large MSMs (2^20 microbench); c=13 with short segments
// for the prover's n=2^15 commits — at n=2^15 the c=16 bucket space (16 x
// 32768 buckets) dwarfs the point count and k_bucket_reduce's suffix-sum
// walk over it was 44% of proof GPU time (profiles/
// r01_final_proof_kernel_stats.csv); c=13 shrinks the bucket space 6.5x
// (20 x 4096) for +25% bucket-accumulation adds. The result point is
// windowing-independent. (c=12/seg=16 measured slower earlier: the reduce
// kept its long segments and fell to 2.8k threads; segment length must
// shrink with the bucket space.)
constexpr int MSM_C_MAX = 16;
constexpr int MSM_NWIN_MAX = 16;             // ceil(255/16) (alloc worst case
                                             // pairs with MSM_NBUCK_MAX;
                                             // c=13 needs 20x4096 << 16x32768)
constexpr int MSM_NBUCK_MAX = 1 << (MSM_C_MAX - 1);
constexpr int MSM_SEG = 16;                  // seg len of the LARGE-c config
// windows by rule: the signed recoding carries out of the top window unless
// that window's raw value stays below 2^(c-1). Scalars are canonical, so
// < 2^255; with W = floor(255/c) + 1 windows c*W >= 256, the top window holds
// at most 255 - c*(W-1) <= c - 1 bits, and raw + carry <= 2^(c-1) is not
// recoded. ceil(255/c) windows fall one short exactly when c divides 255
// (c = 15, 17): scalars in [2^254, p) then carry out of the top window.
TG_HD constexpr int msm_nwin(int c) { return 255 / c + 1; }
// the widths msm_cfg answers; none divides 255, so for them the rule is
// ceil(255/c) and the table the tests pin is where it was
constexpr bool msm_c_generic(int c) { return (c >= 8 && c <= 13) || c == MSM_C_MAX; }
constexpr bool msm_nwin_is_ceil() {
  for (int c = 8; c <= MSM_C_MAX; c++)
    if (msm_c_generic(c) && msm_nwin(c) != (255 + c - 1) / c) return false;
  return true;
}
static_assert(msm_nwin_is_ceil(), "msm_cfg's window counts moved");
struct MsmCfg {
  int c, nwin, nbuck, nseg, seg;  // the reduction picks its own segment
                                  // length (msm_red_seg); nseg/seg remain
                                  // for the pinned table only
};
inline MsmCfg msm_cfg(long n) {
  if (n >= (1L << 18))
    return MsmCfg{16, msm_nwin(16), 1 << 15, (1 << 15) / MSM_SEG, MSM_SEG};
  // below 2^18 the bucket space must track the MSM size (c ~ log2 n - 2,
  // floored at 8 to keep nwin <= 32 for the d_dig/d_wsums allocs): the prover's
  // n=2^15 commits and IPA rounds take c=13 (the rounds fold scalars over
  // the original bases, so each is a full-n MSM), smaller MSMs smaller
  // windows still. Reduce segments sized so nseg <= 1024 per window.
  int lg = 0;
  while ((1L << (lg + 1)) <= n) lg++;
  int sc = lg - 2 < 8 ? 8 : (lg - 2 > 13 ? 13 : lg - 2);
  int nbuck = 1 << (sc - 1);
  int sseg = nbuck / 1024 > 0 ? nbuck / 1024 : 1;
  return MsmCfg{sc, msm_nwin(sc), nbuck, nbuck / sseg, sseg};
}

struct ScalarRepr {
  u64 l[4];
};  // canonical LE

// window w of the signed recoding of canonical s: sum_w d_w * 2^(c*w) = s
// with |d_w| <= 2^(c-1). Returns the magnitude; sign and the carry into
// window w+1 by reference (carry in: 0 for w = 0).
TG_HD uint32_t msm_digit(const ScalarRepr& s, int w, int c, uint32_t& carry, uint32_t& sign) {
  int bit0 = w * c;
  int limb = bit0 >> 6, sh = bit0 & 63;
  u64 raw = s.l[limb] >> sh;
  if (sh && limb < 3 && sh + c > 64) raw |= s.l[limb + 1] << (64 - sh);
  uint32_t d = ((uint32_t)raw & ((1u << c) - 1)) + carry;
  sign = 0;
  if (d > (1u << (c - 1))) {  // take d - 2^c, carry into the next window
    d = (1u << c) - d;
    sign = 1;
    carry = 1;
  } else {
    carry = 0;
  }
  return d;
}

// digits: packed u32 = mag(17 bits) | sign<<17 ; mag==0 means skip.
// hist[w * MSM_NBUCK + (mag-1)]++; with fixed set (the fixed-base plan of
// msm_run) all windows of a batch element share ONE bucket set and the
// histogram index has no window term: hist[mag-1]++
__global__ void __launch_bounds__(256) k_digits(const ScalarRepr* sc, u64 n, u64 nn, MsmCfg cfg,
                uint32_t* dig, uint32_t* hist, bool fixed) {
  // n = total scalars (= nn * batch); histogram is per batch b = i / nn
  const u64 m = fixed ? (u64)cfg.nbuck : (u64)cfg.nwin * cfg.nbuck;
  const u64 wstride = fixed ? 0 : (u64)cfg.nbuck;
  for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n;
       i += (u64)gridDim.x * blockDim.x) {
    u64 bofs = (i / nn) * m;
    ScalarRepr s = sc[i];
    uint32_t carry = 0;
    for (int w = 0; w < cfg.nwin; w++) {
      uint32_t sign;
      uint32_t d = msm_digit(s, w, cfg.c, carry, sign);
      uint32_t packed = d ? (d | (sign << 17)) : 0;
      dig[i * cfg.nwin + w] = packed;
      if (d) atomicAdd(&hist[bofs + (u64)w * wstride + (d - 1)], 1u);
    }
    // the top window of a <2^255 scalar cannot carry out: cfg.nwin follows
    // msm_nwin, which states the rule for any c
  }
}

// ---- 3-kernel exclusive scan over m = MSM_NWIN*MSM_NBUCK entries ----
__global__ void __launch_bounds__(256) k_scan_block(const uint32_t* in, uint32_t* out, uint32_t* bsum, u64 m) {
  __shared__ uint32_t lds[512];
  u64 base = (u64)blockIdx.x * 512;
  int t = threadIdx.x;  // 256 threads, 2 elements each
  lds[t] = base + t < m ? in[base + t] : 0;
  lds[t + 256] = base + t + 256 < m ? in[base + t + 256] : 0;
  __syncthreads();
  // Blelloch up-sweep / down-sweep on 512 elements
  uint32_t total = 0;
  for (int off = 1; off < 512; off <<= 1) {
    int idx = (t + 1) * off * 2 - 1;
    if (idx < 512) lds[idx] += lds[idx - off];
    __syncthreads();
  }
  if (t == 0) {
    total = lds[511];
    lds[511] = 0;
  }
  __syncthreads();
  for (int off = 256; off >= 1; off >>= 1) {
    int idx = (t + 1) * off * 2 - 1;
    if (idx < 512) {
      uint32_t tmp = lds[idx - off];
      lds[idx - off] = lds[idx];
      lds[idx] += tmp;
    }
    __syncthreads();
  }
  if (base + t < m) out[base + t] = lds[t];
  if (base + t + 256 < m) out[base + t + 256] = lds[t + 256];
  if (t == 0) bsum[blockIdx.x] = total;
}

// single-block scan of block sums (nb <= 4096 here: 16*32768/512 = 1024)
__global__ void __launch_bounds__(256) k_scan_sums(uint32_t* bsum, u64 nb) {
  __shared__ uint32_t lds[4096];
  for (u64 i = threadIdx.x; i < nb; i += blockDim.x) lds[i] = bsum[i];
  __syncthreads();
  if (threadIdx.x == 0) {  // serial: nb tiny, once per MSM
    uint32_t acc = 0;
    for (u64 i = 0; i < nb; i++) {
      uint32_t v = lds[i];
      lds[i] = acc;
      acc += v;
    }
  }
  __syncthreads();
  for (u64 i = threadIdx.x; i < nb; i += blockDim.x) bsum[i] = lds[i];
}

__global__ void __launch_bounds__(256) k_scan_add(uint32_t* out, const uint32_t* bsum, u64 m) {
  u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) out[i] += bsum[i / 512];
}

static inline int msm_grid(u64 work, int block = 256) {
  u64 blocks = (work + block - 1) / block;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}

// exclusive scan over m entries (two-level when m/512 exceeds one block's
// LDS); bsum workspace holds level-1 (+ level-2) block sums.
inline void msm_scan(const uint32_t* in, uint32_t* out, uint32_t* bsum, u64 m,
                     hipStream_t stream) {
  u64 nb1 = (m + 511) / 512;
  hipLaunchKernelGGL(k_scan_block, dim3((unsigned)nb1), dim3(256), 0, stream, in, out,
                     bsum, m);
  if (nb1 <= 4096) {
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(256), 0, stream, bsum, nb1);
  } else {
    u64 nb2 = (nb1 + 511) / 512;
    uint32_t* bsum2 = bsum + nb1;
    hipLaunchKernelGGL(k_scan_block, dim3((unsigned)nb2), dim3(256), 0, stream, bsum,
                       bsum, bsum2, nb1);
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(256), 0, stream, bsum2, nb2);
    hipLaunchKernelGGL(k_scan_add, dim3((unsigned)((nb1 + 255) / 256)), dim3(256), 0,
                       stream, bsum, bsum2, nb1);
  }
  hipLaunchKernelGGL(k_scan_add, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream,
                     out, bsum, m);
}

// scatter: sorted[off[bucket]++] = i | sign<<31. With fb_stride = N != 0
// (fixed-base chain) the one bucket set takes every window's digits and the
// entry is the table index w * N + i, the point [2^(c*w)] G_i.
__global__ void __launch_bounds__(256) k_scatter(const uint32_t* dig, u64 n, u64 nn, MsmCfg cfg,
                 uint32_t* off, uint32_t* sorted, uint32_t fb_stride) {
  const u64 m = fb_stride ? (u64)cfg.nbuck : (u64)cfg.nwin * cfg.nbuck;
  const u64 wstride = fb_stride ? 0 : (u64)cfg.nbuck;
  for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n;
       i += (u64)gridDim.x * blockDim.x) {
    u64 bofs = (i / nn) * m;
    uint32_t il = (uint32_t)(i % nn);  // batch-local point index
    for (int w = 0; w < cfg.nwin; w++) {
      uint32_t packed = dig[i * cfg.nwin + w];
      uint32_t mag = packed & 0x1FFFFu;
      if (!mag) continue;
      uint32_t sign = (packed >> 17) & 1u;
      uint32_t pos = atomicAdd(&off[bofs + (u64)w * wstride + (mag - 1)], 1u);
      sorted[pos] = ((uint32_t)w * fb_stride + il) | (sign << 31);
    }
  }
}

// bucket accumulation, phase 1: thread per bucket for small buckets; big
// buckets (heavily duplicated scalars, e.g. the prover's grand-product tail
// rows) are deferred to a wave-per-bucket phase-2 kernel — a single lane
// serially adding tens of thousands of points is a 100x tail otherwise.
constexpr uint32_t MSM_BIG_BUCKET = 64;

// ---- bucket length sort (round 2) ----
// Bucket sizes are Poisson(n/nbuck) (mean ~8 for the prover's c=13 commits),
// so a 64-lane wave processing 64 random buckets runs at the speed of its
// LONGEST bucket (E[max of 64 Poisson(8)] ~ 19): ~2.3x of the lane-time is
// divergence waste. A 66-bin counting sort of bucket ids by length (len
// 0..64, 65 = big) makes every wave's buckets uniform-length — the same
// additions in the same per-bucket order, so proofs stay bit-identical.
constexpr int MSM_LEN_BINS = 66;

// LDS-aggregated: a block counts into LDS and merges 66 counters once —
// per-item global atomics on 66 addresses measured 1.3 ms/launch (26x the
// whole sort's useful work) from contention.
__global__ void __launch_bounds__(256) k_len_hist(const uint32_t* start, const uint32_t* end,
                                                  u64 m, uint32_t* lhist) {
  __shared__ uint32_t lh[MSM_LEN_BINS];
  for (int i = threadIdx.x; i < MSM_LEN_BINS; i += blockDim.x) lh[i] = 0;
  __syncthreads();
  for (u64 b = blockIdx.x * (u64)blockDim.x + threadIdx.x; b < m;
       b += (u64)gridDim.x * blockDim.x) {
    uint32_t len = end[b] - start[b];
    atomicAdd(&lh[len > MSM_BIG_BUCKET ? MSM_LEN_BINS - 1 : len], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < MSM_LEN_BINS; i += blockDim.x)
    if (lh[i]) atomicAdd(&lhist[i], lh[i]);
}

__global__ void k_len_scan(uint32_t* lhist) {  // exclusive scan, 66 entries
  if (threadIdx.x == 0) {
    uint32_t acc = 0;
    for (int i = 0; i < MSM_LEN_BINS; i++) {
      uint32_t v = lhist[i];
      lhist[i] = acc;
      acc += v;
    }
  }
}

// Tiled two-phase placement: a block ranks a 2048-bucket tile in LDS, then
// reserves per-bin ranges with ONE global atomic per live bin. Order within
// a bin is racy across tiles — irrelevant: every bucket is processed once
// and results are stored by bucket id, so proof bytes are unaffected.
__global__ void __launch_bounds__(256) k_len_scatter(const uint32_t* start, const uint32_t* end,
                                                     u64 m, uint32_t* loff, uint32_t* order) {
  __shared__ uint32_t cnt[MSM_LEN_BINS];
  __shared__ uint32_t base[MSM_LEN_BINS];
  const u64 tile_sz = (u64)blockDim.x * 8;
  for (u64 t0 = (u64)blockIdx.x * tile_sz; t0 < m; t0 += (u64)gridDim.x * tile_sz) {
    for (int i = threadIdx.x; i < MSM_LEN_BINS; i += blockDim.x) cnt[i] = 0;
    __syncthreads();
    uint32_t bin[8], rank[8];
    for (int j = 0; j < 8; j++) {
      u64 b = t0 + (u64)j * blockDim.x + threadIdx.x;
      if (b < m) {
        uint32_t len = end[b] - start[b];
        bin[j] = len > MSM_BIG_BUCKET ? MSM_LEN_BINS - 1 : len;
        rank[j] = atomicAdd(&cnt[bin[j]], 1u);
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < MSM_LEN_BINS; i += blockDim.x)
      base[i] = cnt[i] ? atomicAdd(&loff[i], cnt[i]) : 0u;
    __syncthreads();
    for (int j = 0; j < 8; j++) {
      u64 b = t0 + (u64)j * blockDim.x + threadIdx.x;
      if (b < m) order[base[bin[j]] + rank[j]] = (uint32_t)b;
    }
    __syncthreads();
  }
}

template <bool SAFE>
__global__ void __launch_bounds__(256, 1) k_bucket_acc(const uint32_t* start, const uint32_t* end,
                             const uint32_t* sorted, const VestaAff* pts,
                             VestaJac* buckets, u64 nbuckets_total, uint32_t* big_list,
                             uint32_t* big_count, const uint32_t* order) {
  for (u64 t = blockIdx.x * (u64)blockDim.x + threadIdx.x; t < nbuckets_total;
       t += (u64)gridDim.x * blockDim.x) {
    // length-sorted order (null = identity): waves see uniform bucket sizes
    u64 b = order ? order[t] : t;
    uint32_t s = start[b], e = end[b];
    if (e - s > MSM_BIG_BUCKET) {
      uint32_t slot = atomicAdd(big_count, 1u);
      big_list[slot] = (uint32_t)b;
      continue;
    }
    if (!SAFE) {
      if (s == e) {
        buckets[b] = jac_identity<FqCfg>();
        continue;
      }
      uint32_t ent0 = sorted[s];
      VestaAff p0 = pts[ent0 & 0x7FFFFFFFu];
      if (ent0 >> 31) p0 = aff_neg_fast(p0);
      VestaJac acc;
      acc.x = p0.x;
      acc.y = p0.y;
      acc.z = fd_one_mont<FqCfg>();
      for (uint32_t idx = s + 1; idx < e; idx++) {
        uint32_t ent = sorted[idx];
        VestaAff p = pts[ent & 0x7FFFFFFFu];
        if (ent >> 31) p = aff_neg_fast(p);
        jac_add_aff_fast(acc, p);
      }
      buckets[b] = acc;
    } else {
      VestaJac acc = jac_identity<FqCfg>();
      for (uint32_t idx = s; idx < e; idx++) {
        uint32_t ent = sorted[idx];
        VestaAff p = pts[ent & 0x7FFFFFFFu];
        if (ent >> 31) p = aff_neg(p);
        jac_add_aff_inplace(acc, p);
      }
      buckets[b] = acc;
    }
  }
}

// phase 2: one 256-lane block per big bucket; lane-strided partials + LDS
// tree. 256 lanes (vs round-1's 64): the real circuits' bit/byte-valued
// advice columns (blake2s decompositions) concentrate ~n/2 points into
// single buckets — the wide block cuts the serial run per lane 4x
// (k_bucket_acc_big was 15.8% of proof GPU time).
constexpr int MSM_BIG_LANES = 256;
template <bool SAFE>
__global__ void __launch_bounds__(MSM_BIG_LANES, 1) k_bucket_acc_big(const uint32_t* start,
                                 const uint32_t* end, const uint32_t* sorted,
                                 const VestaAff* pts, VestaJac* buckets,
                                 const uint32_t* big_list, const uint32_t* big_count) {
  __shared__ VestaJac lds[MSM_BIG_LANES];
  uint32_t nbig = *big_count;
  for (uint32_t gi = blockIdx.x; gi < nbig; gi += gridDim.x) {
    u64 b = big_list[gi];
    uint32_t s = start[b], e = end[b];
    int t = threadIdx.x;
    VestaJac acc = jac_identity<FqCfg>();
    if (!SAFE) {
      uint32_t first = s + (uint32_t)t;
      if (first < e) {
        uint32_t ent0 = sorted[first];
        VestaAff p0 = pts[ent0 & 0x7FFFFFFFu];
        if (ent0 >> 31) p0 = aff_neg_fast(p0);
        acc.x = p0.x;
        acc.y = p0.y;
        acc.z = fd_one_mont<FqCfg>();
        for (uint32_t idx = first + MSM_BIG_LANES; idx < e; idx += MSM_BIG_LANES) {
          uint32_t ent = sorted[idx];
          VestaAff p = pts[ent & 0x7FFFFFFFu];
          if (ent >> 31) p = aff_neg_fast(p);
          jac_add_aff_fast(acc, p);
        }
      }
    } else {
      for (uint32_t idx = s + t; idx < e; idx += MSM_BIG_LANES) {
        uint32_t ent = sorted[idx];
        VestaAff p = pts[ent & 0x7FFFFFFFu];
        if (ent >> 31) p = aff_neg(p);
        jac_add_aff_inplace(acc, p);
      }
    }
    lds[t] = acc;
    __syncthreads();
    for (int off = MSM_BIG_LANES / 2; off >= 1; off >>= 1) {
      if (t < off) lds[t] = jac_add(lds[t], lds[t + off]);
      __syncthreads();
    }
    if (t == 0) buckets[b] = lds[0];
    __syncthreads();
  }
}

// ---- bucket reduction: window sum W = sum_d (d+1)*B_d, additions only ----
// With d = s*j + q (segments of s buckets, M = nbuck/s of them per window):
//   W = sum_j tot_j + s*F(Y),  tot_j = sum_q (q+1)*B_{sj+q},  Y_j = sum_q B_{sj+q},
//   F(Y) = sum_j j*Y_j.
// Level 1 (k_bucket_segsum): a block takes a chunk of Wd = min(M, 256)
// consecutive segments, one lane per segment (tot_j, Y_j by running sums),
// and reduces the chunk in LDS to T = sum tot, S = sum Y and the bit planes
// P_b = sum_{t: bit b of t set} Y_t of the lane index t. The planes fall out
// of ONE folding tree (msm_wtree_active): folding the upper half of the live
// range onto the lower half leaves the upper half intact, and its plain sum is
// the plane of that bit. Level 2 (k_window_sum, one block per bucket set) adds
// the K = M/Wd chunks up: with j = Wd*k + t,
//   F = sum_b 2^b * sum_k P_{k,b} + Wd * sum_a 2^a * sum_{k: bit a set} S_k.
// So every weight is applied by doublings once per window, never per segment.
// All of it uses the complete jac_add/jac_dbl: empty buckets, repeated bases
// and the zero halves of the IPA vectors make identity, P+P and P+(-P)
// operands routine here.

// level-1 segment length, chosen per bucket-space size for depth against
// parallelism (independent of MsmCfg::seg, which only the tests' table pins)
TG_HD constexpr int msm_red_seg(int nbuck) {
  return nbuck <= 1024 ? 2 : (nbuck <= 4096 ? 4 : 16);
}

// level 1, one segment B[0..s): tot = sum (q+1)*B[q], y = sum B[q]
TG_HD void msm_seg_sums(const VestaJac* B, int s, VestaJac& tot, VestaJac& y) {
  VestaJac run = B[s - 1];
  VestaJac t = run;
  for (int d = s - 2; d >= 0; d--) {
    run = jac_add(run, B[d]);
    t = jac_add(t, run);
  }
  tot = t;
  y = run;
}

constexpr int MSM_WS_WIDTH = 256;  // segments per chunk = lanes of a level-1 block
// level-2 lanes per term = chunks per bucket set at most, the two widths of
// k_window_sum: 8 serves the generic plan (c=16: 2048 segments), 32 the fixed-base
constexpr int MSM_WS_KMAX = 8;
constexpr int MSM_WS_KWIDE = 32;
constexpr int MSM_CHUNK_OUT = 10;  // points a chunk hands on: T, S, P_0..P_7
constexpr int MSM_WS_TERMS = 16;   // level-2 sum: T, <= 8 planes, <= 5 chunk-index planes

TG_HD constexpr int msm_ws_width(int M) { return M < MSM_WS_WIDTH ? M : MSM_WS_WIDTH; }
TG_HD constexpr int msm_lg2(int v) {
  int l = 0;
  while ((1 << l) < v) l++;
  return l;
}

// level 1, lane tid of chunk q = w*K + k (window w of the batch, chunk k):
// segment k*Wd + tid of that window into T[tid], C[tid]
TG_HD void msm_chunk_load(const VestaJac* buckets, int nbuck, int s, u64 q, int tid, VestaJac* C,
                          VestaJac* T) {
  const int M = nbuck / s, Wd = msm_ws_width(M), K = M / Wd;
  if (tid >= Wd) return;
  u64 w = q / K, k = q % K;
  msm_seg_sums(buckets + w * (u64)nbuck + (k * Wd + tid) * (u64)s, s, T[tid], C[tid]);
}

// folding tree with bit planes: at step off, slot i takes slot i+off iff its
// bits at and above off are zero (the fold of [0, 2*off)) or a single bit
// above off (the plain sum of an upper half [2^b, 2^(b+1)) left by an earlier
// fold). After the off=1 step slot 2^b holds P_b and slot 0 the total.
// A slot that is read in a step has bit off set, so it is not written in it.
TG_HD bool msm_wtree_active(int i, int off) {
  int hi = i & ~(off - 1);
  return (hi & (hi - 1)) == 0 && (hi & off) == 0;
}

// level 1, one tree step for lane tid of the 256: the plane tree on C, and
// the plain tree on T in lanes the plane tree never uses at this step (the
// upper half at off=128, else lanes 192..255, whose two top bits are set),
// so that no wave runs both
TG_HD void msm_chunk_step(VestaJac* C, VestaJac* T, int Wd, int off, int tid) {
  if (tid < Wd && msm_wtree_active(tid, off)) C[tid] = jac_add(C[tid], C[tid + off]);
  const int base = MSM_WS_WIDTH - (off > 64 ? off : 64);
  if (tid >= base && tid - base < off) T[tid - base] = jac_add(T[tid - base], T[tid - base + off]);
}

// level 1, lane tid < 2 + log2(Wd) stores one of the chunk's results
TG_HD void msm_chunk_store(const VestaJac* C, const VestaJac* T, int Wd, u64 q, int tid,
                           VestaJac* partials) {
  if (tid >= 2 + msm_lg2(Wd)) return;
  partials[q * MSM_CHUNK_OUT + tid] = tid == 0 ? T[0] : (tid == 1 ? C[0] : C[1 << (tid - 2)]);
}

// level 2, lane = KMAX*e + k: chunk k's summand of term e of
//   W = sum_k T_k + s * (sum_b 2^b * sum_k P_{k,b} + Wd * sum_a 2^a * sum_{k: bit a} S_k)
// (e = 0: T; e = 1..lgw: plane e-1; e = lgw+1+a: chunk-index plane a)
// KMAX = lanes per term; the narrow width unless named
template <int KMAX = MSM_WS_KMAX>
TG_HD VestaJac msm_wsum_input(const VestaJac* chunks, int Wd, int K, int lane) {
  const int e = lane / KMAX, k = lane & (KMAX - 1);
  const int lgw = msm_lg2(Wd), lgk = msm_lg2(K);
  const VestaJac* c = chunks + k * MSM_CHUNK_OUT;
  if (k >= K) return jac_identity<FqCfg>();
  if (e == 0) return c[0];
  if (e <= lgw) return c[1 + e];
  int a = e - lgw - 1;
  if (a < lgk && ((k >> a) & 1)) return c[1];
  return jac_identity<FqCfg>();
}

// level 2: term e, summed over the chunks, times its power of two (lgs = log2 s)
TG_HD VestaJac msm_wsum_scale(VestaJac v, int Wd, int K, int lgs, int e) {
  // plane e-1 weighs 2^(e-1); chunk-index plane a = e-lgw-1 weighs Wd * 2^a
  const int nterms = 1 + msm_lg2(Wd) + msm_lg2(K);
  const int ndbl = (e >= 1 && e < nterms) ? e - 1 + lgs : 0;
  for (int i = 0; i < ndbl; i++) v = jac_dbl(v);
  return v;
}

// level 1: one block per chunk; chunk q's MSM_CHUNK_OUT results go to
// partials[q * MSM_CHUNK_OUT ..]. 48 KB of LDS: three blocks per CU.
__global__ void __launch_bounds__(MSM_WS_WIDTH, 1) k_bucket_segsum(const VestaJac* buckets,
                                                                   VestaJac* partials, int nbuck,
                                                                   int s) {
  __shared__ VestaJac lds[2 * MSM_WS_WIDTH];
  VestaJac* C = lds;
  VestaJac* T = lds + MSM_WS_WIDTH;
  const int tid = threadIdx.x;
  const int Wd = msm_ws_width(nbuck / s);
  msm_chunk_load(buckets, nbuck, s, blockIdx.x, tid, C, T);
  __syncthreads();
  for (int off = Wd / 2; off >= 1; off >>= 1) {
    msm_chunk_step(C, T, Wd, off, tid);
    __syncthreads();
  }
  msm_chunk_store(C, T, Wd, blockIdx.x, tid, partials);
}

// level 2: block w turns bucket set w's K <= KMAX chunk results into one
// Jacobian sum, KMAX lanes per term (a window sum under the generic plan,
// which the host shim combines with the same TG_HD primitives; the MSM itself
// under the fixed-base plan)
template <int KMAX>
__global__ void __launch_bounds__(MSM_WS_TERMS* KMAX) k_window_sum(const VestaJac* partials,
                                                                   VestaJac* wsums, int Wd, int K,
                                                                   int lgs) {
  __shared__ VestaJac X[MSM_WS_TERMS * KMAX];
  const int tid = threadIdx.x, k = tid & (KMAX - 1), e = tid / KMAX;
  X[tid] = msm_wsum_input<KMAX>(partials + (u64)blockIdx.x * K * MSM_CHUNK_OUT, Wd, K, tid);
  __syncthreads();
  for (int off = K / 2; off >= 1; off >>= 1) {
    if (k < off) X[tid] = jac_add(X[tid], X[tid + off]);
    __syncthreads();
  }
  VestaJac v = jac_identity<FqCfg>();
  if (k == 0) v = msm_wsum_scale(X[tid], Wd, K, lgs, e);
  __syncthreads();
  if (k == 0) X[e] = v;
  __syncthreads();
  for (int off = MSM_WS_TERMS / 2; off >= 1; off >>= 1) {
    if (tid < off) X[tid] = jac_add(X[tid], X[tid + off]);
    __syncthreads();
  }
  if (tid == 0) wsums[blockIdx.x] = X[0];
}

// synthetic bench bases: out[i] = [k_i] G with k_i a splitmix64-derived
// 256-bit scalar — RANDOM multiples, like the SRS points the production
// MSMs gather. Small sequential multiples ([seed+i+1]G, the first cut) are
// NOT usable with the fast accumulation path: bucket partial sums are
// [sum of +-k]G with |sum| < 2^27, which collides with the next point
// [+-k_j]G at small-INTEGER rates — the doubling/annihilation cases the
// fast kernel omits (caught by the 2^20 MSM linearity property test,
// round 2; the prover was never exposed: SRS bases are random points).
// Deterministic and byte-identical to the oracle's orc_gen_bases.
__device__ __forceinline__ u64 tg_sm64(u64 x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
__global__ void __launch_bounds__(256) k_gen_bases(VestaAff* out, u64 n, u64 seed) {
  // generator (-1, 2) in Mont form
  for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n;
       i += (u64)gridDim.x * blockDim.x) {
    Fq one = fd_one_mont<FqCfg>();
    VestaAff G;
    G.x = fd_neg(one);
    Fq two = fd_add(one, one);
    G.y = two;
    u64 k[4];
    for (int j = 0; j < 4; j++)
      k[j] = tg_sm64(seed * 0xD1B54A32D192ED03ull + i * 4 + (u64)j);
    VestaJac acc = jac_identity<FqCfg>();
    VestaJac base = jac_from_aff(G);
    for (int b = 0; b < 256; b++) {
      if ((k[b >> 6] >> (b & 63)) & 1) acc = jac_add(acc, base);
      base = jac_dbl(base);
    }
    out[i] = jac_to_aff(acc);
  }
}

// ---- workspace + launcher ----
// (sets = MsmPlan::sets(), bucket sets per MSM: nwin, or 1 with a table)
struct MsmWork {
  uint32_t* d_dig = nullptr;     // n * NWIN
  uint32_t* d_hist = nullptr;    // sets * NBUCK per MSM (start offsets after scan)
  uint32_t* d_off = nullptr;     // running copy for scatter
  uint32_t* d_end = nullptr;     // end offsets (= start + count)
  uint32_t* d_bsum = nullptr;    // scan block sums
  uint32_t* d_sorted = nullptr;  // n * NWIN entries (base or table indices)
  VestaJac* d_buckets = nullptr;   // sets * NBUCK per MSM
  VestaJac* d_partials = nullptr;  // sets * K chunks of MSM_CHUNK_OUT per MSM
  VestaJac* d_wsums = nullptr;  // sets sums per MSM (msm_finish, on the host)
  uint32_t* d_big = nullptr;    // big-bucket work list + count (phase 2)
  uint32_t* d_order = nullptr;  // bucket ids counting-sorted by length
  uint32_t* d_lhist = nullptr;  // MSM_LEN_BINS length histogram / offsets
  u64 cap_n = 0;
  u64 cap_b = 1;
};

inline hipError_t msm_work_alloc(MsmWork& w, u64 n_total, u64 batch = 1) {
  if (w.cap_n >= n_total && w.cap_b >= batch) return hipSuccess;
  if (n_total < w.cap_n) n_total = w.cap_n;
  if (batch < w.cap_b) batch = w.cap_b;
  u64 m = (u64)MSM_NWIN_MAX * MSM_NBUCK_MAX * batch;
  hipError_t e;
#define TGW_FREE(p) \
  if (p) { hipFree(p); p = nullptr; }
  TGW_FREE(w.d_dig) TGW_FREE(w.d_hist) TGW_FREE(w.d_off) TGW_FREE(w.d_end)
  TGW_FREE(w.d_bsum) TGW_FREE(w.d_sorted) TGW_FREE(w.d_buckets) TGW_FREE(w.d_partials)
  TGW_FREE(w.d_wsums) TGW_FREE(w.d_big) TGW_FREE(w.d_order) TGW_FREE(w.d_lhist)
#undef TGW_FREE
  if ((e = hipMalloc(&w.d_dig, n_total * 32 * 4)) != hipSuccess) return e;  /* nwin<=32 (c=8) */
  if ((e = hipMalloc(&w.d_hist, m * 4)) != hipSuccess) return e;
  if ((e = hipMalloc(&w.d_off, m * 4)) != hipSuccess) return e;
  if ((e = hipMalloc(&w.d_end, m * 4)) != hipSuccess) return e;
  u64 nb1 = (m + 511) / 512;
  if ((e = hipMalloc(&w.d_bsum, (nb1 + (nb1 + 511) / 512 + 1) * 4)) != hipSuccess) return e;
  if ((e = hipMalloc(&w.d_sorted, n_total * 32 * 4)) != hipSuccess) return e;
  if ((e = hipMalloc(&w.d_buckets, m * sizeof(VestaJac))) != hipSuccess) return e;
  // MSM_CHUNK_OUT points per level-1 chunk, sets * batch * K chunks. Worst
  // case c=16: nwin * K = 16 * 8 = 128 per batch, exactly this; the other
  // rows have 32, 29, 26 (K=1), 48, 44 (K=2) and 80 (c=13, K=4), the
  // fixed-base plan 1 * 32 (msm_plans_fit holds every plan to it).
  if ((e = hipMalloc(&w.d_partials, (u64)MSM_NWIN_MAX * MSM_WS_KMAX * batch * MSM_CHUNK_OUT *
                                        sizeof(VestaJac))) != hipSuccess)
    return e;
  if ((e = hipMalloc(&w.d_wsums, MSM_NWIN_MAX * 2 * batch * sizeof(VestaJac))) !=
      hipSuccess)
    return e;
  if ((e = hipMalloc(&w.d_big, (m + 1) * 4)) != hipSuccess) return e;
  if ((e = hipMalloc(&w.d_order, m * 4)) != hipSuccess) return e;
  if ((e = hipMalloc(&w.d_lhist, MSM_LEN_BINS * 4)) != hipSuccess) return e;
  w.cap_n = n_total;
  w.cap_b = batch;
  return hipSuccess;
}

// counting-sort bucket ids by length into w.d_order (see MSM_LEN_BINS note);
// call between k_scatter (start/end final) and k_bucket_acc. Returns the
// order array to hand to k_bucket_acc. Measured on MI355X: 1.44x on
// k_bucket_acc at the prover's c=13 (Poisson(8) buckets, wave runs at
// max-of-64 ~ 19 without it) and 1.15x at c=16/n=2^20 — but ONLY with the
// LDS-aggregated histogram/scatter below; the first cut's per-item global
// atomics on 66 bins serialized the whole chip across all proving streams.
inline const uint32_t* msm_len_sort(MsmWork& w, u64 m, hipStream_t stream) {
  hipMemsetAsync(w.d_lhist, 0, MSM_LEN_BINS * 4, stream);
  hipLaunchKernelGGL(k_len_hist, dim3(msm_grid(m)), dim3(256), 0, stream, w.d_hist,
                     w.d_end, m, w.d_lhist);
  hipLaunchKernelGGL(k_len_scan, dim3(1), dim3(64), 0, stream, w.d_lhist);
  hipLaunchKernelGGL(k_len_scatter, dim3(msm_grid(m, 256 * 8)), dim3(256), 0, stream,
                     w.d_hist, w.d_end, m, w.d_lhist, w.d_order);
  return w.d_order;
}

// bucket accumulation, both phases. SAFE handles identity/duplicate bases
// (caller-uploaded sets); the branch-free variant needs distinct
// non-identity bases (SRS sets, gen_bases output).
template <bool SAFE>
inline void msm_acc_launch(MsmWork& w, u64 m, const VestaAff* bases, const uint32_t* ord,
                           hipStream_t stream) {
  hipLaunchKernelGGL(k_bucket_acc<SAFE>, dim3(msm_grid(m)), dim3(256), 0, stream,
                     w.d_hist, w.d_end, w.d_sorted, bases, w.d_buckets, m, w.d_big,
                     w.d_big + m, ord);
  hipLaunchKernelGGL(k_bucket_acc_big<SAFE>, dim3(1024), dim3(MSM_BIG_LANES), 0, stream,
                     w.d_hist, w.d_end, w.d_sorted, bases, w.d_buckets, w.d_big,
                     w.d_big + m);
}

// prof indices of msm_run: the six stages in P_MSM_* order, then the two
// accumulation kernels alone (inside MSM_P_ACC, which also covers the
// length sort), then the whole chain up to the window sums.
enum {
  MSM_P_DIGITS = 0, MSM_P_SCAN, MSM_P_SCATTER, MSM_P_ACC, MSM_P_REDUCE, MSM_P_WSUM,
  MSM_P_ACC_KERNELS, MSM_P_CHAIN,
};

// the unprofiled ProfFn
inline int msm_noprof(int) { return 0; }

// ---- fixed-base tables: window weights folded into precomputed bases ----
// The SRS sets never change after tg_load_srs, so the weights 2^(c*w) that
// the generic plan applies per MSM (nwin bucket reductions, then the host's
// Horner combine) are applied to the bases once, at load:
//   T[w][j] = [2^(c*w)] G_j,   sum_j k_j G_j = sum_j sum_w d_{j,w} T[w][j],
// ONE bucket set per MSM, one reduction, one point back. Reduction cost no
// longer grows with the window count, so the window is wider than msm_cfg's
// c=13 at n=2^15 (profiles/README.md, round 6, has the measurements).
constexpr int MSM_FB_C = 16;
constexpr int MSM_FB_NWIN = msm_nwin(MSM_FB_C);
constexpr int MSM_FB_NBUCK = 1 << (MSM_FB_C - 1);
// tables are built for SRS sizes up to 2^MSM_FB_KMAX (64 B * nwin * 2^k per
// set: 2 x 32 MiB at k=15); a larger SRS stays on the generic plan
constexpr int MSM_FB_KMAX = 17;
static_assert(MSM_FB_C <= MSM_C_MAX && MSM_FB_NWIN <= 32, "workspace sizing (msm_work_alloc)");
static_assert((u64)MSM_FB_NWIN << MSM_FB_KMAX < (1ull << 31), "sorted entry: index | sign<<31");

// table build, window w from window w-1: c doublings per point (Jacobian out)
__global__ void __launch_bounds__(256) k_fb_dbl(const VestaAff* prev, VestaJac* out, u64 n, int c) {
  for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n;
       i += (u64)gridDim.x * blockDim.x) {
    VestaJac p = jac_from_aff(prev[i]);
    for (int b = 0; b < c; b++) p = jac_dbl(p);
    out[i] = p;
  }
}

// Jacobian -> Montgomery affine with a batched inversion: a thread walks
// MSM_FB_INV_RUN consecutive points, inverts the product of their z once and
// unwinds it. No point of the table is the identity (the group has prime
// order and the SRS points are checked non-identity), so every z is nonzero.
constexpr int MSM_FB_INV_RUN = 32;
__global__ void __launch_bounds__(64) k_fb_to_aff(const VestaJac* in, VestaAff* out, u64 n) {
  for (u64 t = blockIdx.x * (u64)blockDim.x + threadIdx.x; t * MSM_FB_INV_RUN < n;
       t += (u64)gridDim.x * blockDim.x) {
    const u64 i0 = t * MSM_FB_INV_RUN;
    const int cnt = n - i0 < (u64)MSM_FB_INV_RUN ? (int)(n - i0) : MSM_FB_INV_RUN;
    Fq pre[MSM_FB_INV_RUN];  // pre[i] = z_0 * ... * z_i
    Fq acc = in[i0].z;
    pre[0] = acc;
    for (int i = 1; i < cnt; i++) {
      acc = fd_mul(acc, in[i0 + i].z);
      pre[i] = acc;
    }
    Fq inv = fd_inv(acc);  // 1 / (z_0 ... z_{cnt-1})
    for (int i = cnt - 1; i >= 0; i--) {
      VestaJac p = in[i0 + i];
      Fq zi = i ? fd_mul(inv, pre[i - 1]) : inv;  // 1 / z_i
      inv = fd_mul(inv, p.z);
      Fq zi2 = fd_sqr(zi);
      VestaAff a;
      a.x = fd_mul(p.x, zi2);
      a.y = fd_mul(p.y, fd_mul(zi2, zi));
      out[i0 + i] = a;
    }
  }
}

// build tab[w * n + j] = [2^(MSM_FB_C * w)] bases[j], w < MSM_FB_NWIN; tmp
// holds n Jacobian points
inline void msm_fb_build(const VestaAff* bases, VestaAff* tab, VestaJac* tmp, u64 n,
                         hipStream_t stream) {
  hipMemcpyAsync(tab, bases, n * sizeof(VestaAff), hipMemcpyDeviceToDevice, stream);
  const u64 runs = (n + MSM_FB_INV_RUN - 1) / MSM_FB_INV_RUN;
  for (int w = 1; w < MSM_FB_NWIN; w++) {
    hipLaunchKernelGGL(k_fb_dbl, dim3(msm_grid(n)), dim3(256), 0, stream,
                       tab + (u64)(w - 1) * n, tmp, n, MSM_FB_C);
    hipLaunchKernelGGL(k_fb_to_aff, dim3(msm_grid(runs, 64)), dim3(64), 0, stream, tmp,
                       tab + (u64)w * n, n);
  }
}

// the fixed-base plan's reduction, one bucket set per MSM. With a single set
// there is parallelism to spare, so segments are short (s = 4 against the
// generic 16 at this bucket count) and the set has 32 chunks, which level 2
// folds with 32 lanes per term. Serial chain in point operations, c=16: 6
// (segment) + 8 (chunk tree) + 5 (chunk fold) + 14 (doublings) + 4 (terms) =
// 37, against 59 with the generic c=16 row (s = 16, K = 8).
constexpr int MSM_FB_SEG = 4;

// ---- the launch plan: everything the two uses of msm_run disagree about ----
struct MsmPlan {
  MsmCfg cfg;
  const VestaAff* pts;  // what the accumulation gathers from: the bases, or their table
  uint32_t stride;      // table stride N (its SRS set's size); 0: plain bases, generic plan
  bool safe;            // accumulation that handles identities and equal x
  int rseg, rWd, rK;    // reduction: buckets per segment, segments per chunk, chunks per set
  // bucket sets per MSM = Jacobian points msm_run returns per MSM
  int sets() const { return stride ? 1 : cfg.nwin; }
};

inline MsmPlan msm_plan(const MsmCfg& cfg, const VestaAff* pts, uint32_t stride, bool safe,
                        int rseg) {
  const int rWd = msm_ws_width(cfg.nbuck / rseg);
  return MsmPlan{cfg, pts, stride, safe, rseg, rWd, cfg.nbuck / rseg / rWd};
}

// nn points per MSM over plain device bases; safe for sets that may hold
// identities or repeated points (caller uploads)
inline MsmPlan msm_plan_generic(long nn, const VestaAff* bases, bool safe) {
  const MsmCfg cfg = msm_cfg(nn);
  return msm_plan(cfg, bases, 0, safe, msm_red_seg(cfg.nbuck));
}

// over the first nn <= tab_n bases of an SRS set, through its table
// (msm_fb_build of tab_n points). The table's points must be pairwise
// x-distinct (tg_load_srs checks it), for the branch-free accumulation.
inline MsmPlan msm_plan_fixed(const VestaAff* tab, u64 tab_n) {
  return msm_plan(MsmCfg{MSM_FB_C, MSM_FB_NWIN, MSM_FB_NBUCK, MSM_FB_NBUCK / MSM_SEG, MSM_SEG},
                  tab, (uint32_t)tab_n, false, MSM_FB_SEG);
}

// a reduction shape that the kernels and the workspace hold: whole chunks, a
// power-of-two K within the level-2 lanes per term, sets * K chunks within
// d_partials, and T + planes + chunk-index planes within MSM_WS_TERMS
constexpr bool msm_red_fits(int sets, int nbuck, int s) {
  const int M = nbuck / s, Wd = msm_ws_width(M), K = M / Wd;
  return K * Wd * s == nbuck && (K & (K - 1)) == 0 && K <= MSM_WS_KWIDE &&
         sets * K <= MSM_NWIN_MAX * MSM_WS_KMAX && 1 + msm_lg2(Wd) + msm_lg2(K) <= MSM_WS_TERMS;
}
constexpr bool msm_plans_fit() {
  for (int c = 8; c <= MSM_C_MAX; c++)
    if (msm_c_generic(c) &&
        !msm_red_fits(msm_nwin(c), 1 << (c - 1), msm_red_seg(1 << (c - 1))))
      return false;
  return msm_red_fits(1, MSM_FB_NBUCK, MSM_FB_SEG);
}
static_assert(msm_plans_fit(), "a plan's reduction outgrows level 2 or the d_partials allocation");

template <int KMAX>
inline void msm_wsum_launch(MsmWork& w, const MsmPlan& plan, u64 B, hipStream_t stream) {
  hipLaunchKernelGGL(k_window_sum<KMAX>, dim3(plan.sets() * B), dim3(MSM_WS_TERMS * KMAX), 0,
                     stream, w.d_partials, w.d_wsums, plan.rWd, plan.rK, msm_lg2(plan.rseg));
}

// B same-size MSMs (nn points each, n = nn * B canonical device scalars) by
// one plan: enqueues the whole kernel chain on stream and the copy of the
// plan.sets() * B Jacobian sums to host out (valid after the caller
// synchronizes the stream; msm_finish turns each MSM's sets() points into
// the MSM). w must be msm_work_alloc'ed for (n, B).
// ProfFn: callable int->RAII scope, as in ntt_run (msm_noprof for none).
template <class ProfFn>
inline void msm_run(MsmWork& w, const ScalarRepr* d_scalars, u64 n, u64 nn, u64 B,
                    const MsmPlan& plan, hipStream_t stream, VestaJac* out, ProfFn&& prof) {
  const MsmCfg& cfg = plan.cfg;
  const u64 m = (u64)plan.sets() * cfg.nbuck * B;
  {
    [[maybe_unused]] auto chain = prof(MSM_P_CHAIN);
    {
      [[maybe_unused]] auto p = prof(MSM_P_DIGITS);
      hipMemsetAsync(w.d_hist, 0, m * 4, stream);
      hipLaunchKernelGGL(k_digits, dim3(msm_grid(n)), dim3(256), 0, stream, d_scalars, n,
                         nn, cfg, w.d_dig, w.d_hist, plan.stride != 0);
    }
    {
      [[maybe_unused]] auto p = prof(MSM_P_SCAN);
      msm_scan(w.d_hist, w.d_off, w.d_bsum, m, stream);
      hipMemcpyAsync(w.d_hist, w.d_off, m * 4, hipMemcpyDeviceToDevice, stream);
    }
    {
      [[maybe_unused]] auto p = prof(MSM_P_SCATTER);
      hipLaunchKernelGGL(k_scatter, dim3(msm_grid(n)), dim3(256), 0, stream, w.d_dig, n,
                         nn, cfg, w.d_off, w.d_sorted, plan.stride);
      hipMemcpyAsync(w.d_end, w.d_off, m * 4, hipMemcpyDeviceToDevice, stream);
    }
    {
      [[maybe_unused]] auto p = prof(MSM_P_ACC);
      hipMemsetAsync(w.d_big + m, 0, 4, stream);
      const uint32_t* ord = msm_len_sort(w, m, stream);
      [[maybe_unused]] auto pk = prof(MSM_P_ACC_KERNELS);
      if (plan.safe)
        msm_acc_launch<true>(w, m, plan.pts, ord, stream);
      else
        msm_acc_launch<false>(w, m, plan.pts, ord, stream);
    }
    {
      [[maybe_unused]] auto p = prof(MSM_P_REDUCE);
      hipLaunchKernelGGL(k_bucket_segsum, dim3(plan.sets() * B * plan.rK), dim3(MSM_WS_WIDTH),
                         0, stream, w.d_buckets, w.d_partials, cfg.nbuck, plan.rseg);
    }
    {
      [[maybe_unused]] auto p = prof(MSM_P_WSUM);
      if (plan.rK <= MSM_WS_KMAX)
        msm_wsum_launch<MSM_WS_KMAX>(w, plan, B, stream);
      else
        msm_wsum_launch<MSM_WS_KWIDE>(w, plan, B, stream);
    }
  }
  hipMemcpyAsync(out, w.d_wsums, sizeof(VestaJac) * plan.sets() * B, hipMemcpyDeviceToHost,
                 stream);
}

// host-side final combine: acc = sum_w 2^(c*w) * wsum[w]  (Horner, ~240
// doublings of O(1) work — the same TG_HD primitives as the kernels)
inline VestaJac msm_host_combine_jac(const VestaJac* wsums, const MsmCfg& cfg) {
  VestaJac acc = jac_identity<FqCfg>();
  for (int w = cfg.nwin - 1; w >= 0; w--) {
    if (w != cfg.nwin - 1)
      for (int b = 0; b < cfg.c; b++) acc = jac_dbl(acc);
    acc = jac_add(acc, wsums[w]);
  }
  return acc;
}

inline VestaAff msm_host_combine(const VestaJac* wsums, const MsmCfg& cfg) {
  return jac_to_aff(msm_host_combine_jac(wsums, cfg));
}

// one MSM from the plan.sets() points msm_run returned for it: the Horner
// combine of the generic plan's window sums; the fixed-base plan's one point
// is the MSM as it came
inline VestaJac msm_finish(const MsmPlan& plan, const VestaJac* sums) {
  return plan.sets() > 1 ? msm_host_combine_jac(sums, plan.cfg) : sums[0];
}

}  // namespace taiga
