// lookup_argument.hip — permute_expression_pair of the lookup argument on
// the device: A' is the ascending sort of the compressed input expression A
// over the usable rows, S' holds A'[i] wherever A' takes a new value and the
// table values left over, in sorted order, in the other rows.
// Included by taiga_gpu.cpp (single TU) after grand_products.hip. The
// compress kernel k_lk_compress needs the expression interpreter and lives
// beside it in prover_gpu.inc; the launchers are there too.
//
// The order is that of the canonical integer, limb 3 down to limb 0, so the
// sort converts out of Montgomery form on load, everything in between holds
// canonical limbs, and k_lk_write converts back on the last write. Rows past
// u are padded with the all-ones key, which is above every canonical value.
// The sort is a bitonic network: exact, deterministic, keys only.
#pragma once
#include <hip/hip_runtime.h>

#include "pasta_device.hpp"

namespace taiga {

// capacity of the argument tables; prover_gpu.inc asserts that it equals the
// limit pdesc_parse enforces. Two arrays are sorted per lookup (A and S).
constexpr int LK_MAX_LOOKUPS = 4;
constexpr int LK_MAX_ARRAYS = 2 * LK_MAX_LOOKUPS;

// threads per block of every kernel here
constexpr int LK_B = 256;
// keys one block sorts in LDS. 2048 keys of 32 bytes are 64 KiB, which leaves
// two workgroups per CU within the 160 KiB of a gfx950 CU. The proof-level
// arrays are 2^15 long: 16 tiles, and 15 launches per sort (one tile sort,
// then per merge level its global strides and one LDS finish).
// tests/test_device_lookup_permute.py mirrors this constant.
#ifndef LK_TILE
#define LK_TILE 2048
#endif
static_assert((LK_TILE & (LK_TILE - 1)) == 0 && LK_TILE >= 2, "LK_TILE is a power of two");
static_assert(LK_TILE * 32 <= 65536, "a tile must fit the 64 KiB static LDS limit");

// ---------------- index arithmetic (host-checkable) ----------------

// the network runs over np = 2^m >= u keys
TG_HD long lk_padded(long u) {
  long np = 1;
  while (np < u) np <<= 1;
  return np;
}
// keys per block of the LDS kernels, and their grid
TG_HD long lk_tile_len(long np) { return np < LK_TILE ? np : LK_TILE; }
TG_HD long lk_tiles(long np) { return np / lk_tile_len(np); }
// key e < lk_tile_len of tile b
TG_HD long lk_tile_index(long b, long np, long e) { return b * lk_tile_len(np) + e; }
// A compare-exchange stage of stride j (a power of two) over len keys has
// len / 2 pairs; pair p is (lo, lo + j) where lo is p with a zero bit
// inserted at bit log2(j). Consecutive p give consecutive lo inside a run of
// j keys, so the lanes of a wave read neighbouring keys at every stride.
TG_HD long lk_pair_lo(long p, long j) { return ((p & ~(j - 1)) << 1) | (p & (j - 1)); }
TG_HD long lk_pair_hi(long lo, long j) { return lo | j; }
// merge level k (the sorted runs grow to k keys): the pair sorts ascending
// when bit k of its global index is clear. The last level has k = np.
TG_HD bool lk_pair_up(long lo, long k) { return (lo & k) == 0; }
// grid of the global stage (one pair per thread) and of the row kernels
TG_HD long lk_stage_blocks(long np) { return (np / 2 + LK_B - 1) / LK_B; }
TG_HD long lk_row_blocks(long u) { return (u + LK_B - 1) / LK_B; }
// launches of one sort: the tile sort, then for every level above a tile
// its strides >= the tile length and one LDS finish
TG_HD int lk_sort_launches(long np) {
  int c = 1;
  for (long k = 2 * lk_tile_len(np); k <= np; k <<= 1) {
    for (long j = k / 2; j >= lk_tile_len(np); j >>= 1) c++;
    c++;
  }
  return c;
}
// the flag arrays of lookup l in the flat scan: first[] then taken[], u each
TG_HD long lk_first_at(int l, long u, long i) { return (2L * l) * u + i; }
TG_HD long lk_taken_at(int l, long u, long p) { return (2L * l + 1) * u + p; }
// rank among the slots whose flag is clear: idx minus the flags set before
// it, which is the exclusive scan at idx minus the scan at the array's start
TG_HD long lk_clear_rank(long idx, uint32_t scan_at, uint32_t scan_base) {
  return idx - (long)(scan_at - scan_base);
}

// ---------------- keys ----------------

// canonical integer order, limb 3 down to limb 0
TG_HD bool lk_key_lt(const Fp& a, const Fp& b) {
  for (int i = 3; i > 0; i--)
    if (a.l[i] != b.l[i]) return a.l[i] < b.l[i];
  return a.l[0] < b.l[0];
}
TG_HD Fp lk_pad_key() { return Fp{{~0ULL, ~0ULL, ~0ULL, ~0ULL}}; }
// first p in [0, u) with t[p] >= v, or u
TG_HD long lk_lower_bound(const Fp* t, long u, const Fp& v) {
  long lo = 0, hi = u;
  while (lo < hi) {
    long mid = lo + (hi - lo) / 2;
    if (lk_key_lt(t[mid], v)) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// ---------------- sort ----------------

struct LkSortArgs {
  const Fp* src[LK_MAX_ARRAYS];  // Montgomery form, rows < u read
  Fp* dst[LK_MAX_ARRAYS];        // np canonical keys, sorted ascending
  long u, np;
};

// The tile in LDS, one plane per limb: a lane reads limb w of key e at
// sh[w][e], so neighbouring lanes read neighbouring 8-byte words (conflict
// free for strides >= 64, two-way at stride 1).
__device__ __forceinline__ void lk_tile_store(u64 (*sh)[LK_TILE], int e, const Fp& v) {
#pragma unroll
  for (int w = 0; w < 4; w++) sh[w][e] = v.l[w];
}
__device__ __forceinline__ Fp lk_tile_load(u64 (*sh)[LK_TILE], int e) {
  Fp v;
#pragma unroll
  for (int w = 0; w < 4; w++) v.l[w] = sh[w][e];
  return v;
}

// one compare-exchange stage over the tl keys of the tile that starts at
// global index base
__device__ __forceinline__ void lk_tile_stage(u64 (*sh)[LK_TILE], long base, int tl, long k,
                                              int j) {
  for (int p = threadIdx.x; p < tl / 2; p += LK_B) {
    const int lo = (int)lk_pair_lo(p, j), hi = (int)lk_pair_hi(lo, j);
    const Fp a = lk_tile_load(sh, lo), b = lk_tile_load(sh, hi);
    const bool swap = lk_pair_up(base + lo, k) ? lk_key_lt(b, a) : lk_key_lt(a, b);
    if (swap) {
      lk_tile_store(sh, lo, b);
      lk_tile_store(sh, hi, a);
    }
  }
  __syncthreads();
}

// every level up to the tile length: dst tile <- sorted src tile, ascending
// or descending as the next level wants it. blockIdx.y is the array.
__global__ void __launch_bounds__(LK_B) k_lk_sort_tile(LkSortArgs A) {
  __shared__ u64 sh[4][LK_TILE];
  const Fp* __restrict__ src = A.src[blockIdx.y];
  Fp* __restrict__ dst = A.dst[blockIdx.y];
  const int tl = (int)lk_tile_len(A.np);
  const long base = lk_tile_index(blockIdx.x, A.np, 0);
  for (int e = threadIdx.x; e < tl; e += LK_B) {
    const long g = base + e;
    lk_tile_store(sh, e, g < A.u ? fd_from_mont(src[g]) : lk_pad_key());
  }
  __syncthreads();
  for (int k = 2; k <= tl; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) lk_tile_stage(sh, base, tl, k, j);
  for (int e = threadIdx.x; e < tl; e += LK_B) dst[base + e] = lk_tile_load(sh, e);
}

// one stage of level k at a stride j >= the tile length: a pair per thread
__global__ void __launch_bounds__(LK_B) k_lk_sort_global(LkSortArgs A, long k, long j) {
  Fp* __restrict__ dst = A.dst[blockIdx.y];
  const long p = blockIdx.x * (long)LK_B + threadIdx.x;
  if (p >= A.np / 2) return;
  const long lo = lk_pair_lo(p, j), hi = lk_pair_hi(lo, j);
  const Fp a = dst[lo], b = dst[hi];
  const bool swap = lk_pair_up(lo, k) ? lk_key_lt(b, a) : lk_key_lt(a, b);
  if (swap) {
    dst[lo] = b;
    dst[hi] = a;
  }
}

// the strides below the tile length of level k, in LDS
__global__ void __launch_bounds__(LK_B) k_lk_sort_merge(LkSortArgs A, long k) {
  __shared__ u64 sh[4][LK_TILE];
  Fp* __restrict__ dst = A.dst[blockIdx.y];
  const int tl = (int)lk_tile_len(A.np);
  const long base = lk_tile_index(blockIdx.x, A.np, 0);
  for (int e = threadIdx.x; e < tl; e += LK_B) lk_tile_store(sh, e, dst[base + e]);
  __syncthreads();
  for (int j = tl >> 1; j > 0; j >>= 1) lk_tile_stage(sh, base, tl, k, j);
  for (int e = threadIdx.x; e < tl; e += LK_B) dst[base + e] = lk_tile_load(sh, e);
}

// ---------------- S' ----------------

// bits of the error word
constexpr uint32_t LK_ERR_MISSING = 1;  // an input value is not in the table
constexpr uint32_t LK_ERR_RANK = 2;     // a leftover position out of range

struct LkPermArgs {
  Fp* ap[LK_MAX_LOOKUPS];       // sorted A: canonical in, Montgomery out
  const Fp* t[LK_MAX_LOOKUPS];  // sorted table, canonical
  Fp* sp[LK_MAX_LOOKUPS];       // S', Montgomery
  uint32_t* err;
  uint32_t* flags;  // lk_first_at / lk_taken_at; taken[] zero on entry
  uint32_t* scan;   // exclusive scan of flags over the flat array
  uint32_t* lpos;   // [l * u + r]: position in t of the r-th leftover
  long u;
};

// first[i] = A' takes a new value at i; such a slot takes the first table
// entry equal to it. Distinct values have distinct lower bounds, so no two
// slots take the same entry. blockIdx.y is the lookup.
__global__ void __launch_bounds__(LK_B) k_lk_first(LkPermArgs A) {
  const int l = blockIdx.y;
  const long i = blockIdx.x * (long)LK_B + threadIdx.x;
  if (i >= A.u) return;
  const Fp* __restrict__ ap = A.ap[l];
  const Fp* __restrict__ t = A.t[l];
  const Fp a = ap[i];
  const bool first = i == 0 || !fd_eq(a, ap[i - 1]);
  A.flags[lk_first_at(l, A.u, i)] = first;
  if (!first) return;
  const long p = lk_lower_bound(t, A.u, a);
  if (p == A.u || !fd_eq(t[p], a))
    atomicOr(A.err, LK_ERR_MISSING);
  else
    A.flags[lk_taken_at(l, A.u, p)] = 1;
}

// the table entries nobody took, in order: lpos[rank] = position
__global__ void __launch_bounds__(LK_B) k_lk_leftover(LkPermArgs A) {
  const int l = blockIdx.y;
  const long p = blockIdx.x * (long)LK_B + threadIdx.x;
  if (p >= A.u) return;
  const long at = lk_taken_at(l, A.u, p);
  if (A.flags[at]) return;
  const long r = lk_clear_rank(p, A.scan[at], A.scan[lk_taken_at(l, A.u, 0)]);
  A.lpos[(long)l * A.u + r] = (uint32_t)p;
}

// S'[i] = A'[i] at a first slot, the r-th leftover at the r-th repeat slot;
// both rows go back to Montgomery form. With the error word set the counts
// of repeats and leftovers need not agree, and nothing is written.
__global__ void __launch_bounds__(LK_B) k_lk_write(LkPermArgs A) {
  const int l = blockIdx.y;
  const long i = blockIdx.x * (long)LK_B + threadIdx.x;
  if (i >= A.u || *A.err) return;
  const Fp a = A.ap[l][i];
  Fp s = a;
  const long at = lk_first_at(l, A.u, i);
  if (!A.flags[at]) {
    const long r = lk_clear_rank(i, A.scan[at], A.scan[lk_first_at(l, A.u, 0)]);
    const uint32_t q = A.lpos[(long)l * A.u + r];
    if (q >= A.u) {
      atomicOr(A.err, LK_ERR_RANK);
      return;
    }
    s = A.t[l][q];
  }
  A.ap[l][i] = fd_to_mont(a);
  A.sp[l][i] = fd_to_mont(s);
}

}  // namespace taiga
