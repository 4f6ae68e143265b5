// lk_index_probe — the index arithmetic of lookup_argument.hip on the host.
// The sort and S' kernels address memory only through the TG_HD functions at
// the top of that file; this program runs the whole algorithm the way the
// launchers and kernels do (grids, blocks, threads, stages), over heap arrays
// of EXACTLY the sizes the launchers use, so that an index outside them is an
// AddressSanitizer report. Every compare-exchange stage must touch every key
// exactly once, and A' and S' must equal the serial loop restated below.
// Built by tests/test_lk_index_host.py with -fsanitize=address,undefined.
//
// usage: lk_index_probe U...   a first line with the constants, then one
// line per u:
//   "<u> np=<keys sorted> launches=<sort launches> stages=<stages walked>
//    pairs=<pairs visited once> ok"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lookup_argument.hip"

using namespace taiga;

static uint64_t g_rng = 0x9E3779B97F4A7C15ULL;
static uint64_t next_u64() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return g_rng;
}

// a heap array of exactly count elements (at least one byte is allocated)
template <class T>
struct Heap {
  T* p;
  size_t count;
  explicit Heap(size_t n) : p((T*)calloc(n ? n : 1, n ? sizeof(T) : 1)), count(n) {}
  ~Heap() { free(p); }
  T& operator[](size_t i) { return p[i]; }
};

static long g_stages, g_pairs;

// one stage over len keys at keys[0..len), global index of keys[0] is base:
// the pairs as the threads of one block (tile kernels) take them
static int tile_stage(Fp* keys, unsigned char* seen, long base, int tl, long k, int j) {
  memset(seen, 0, (size_t)tl);
  for (int t = 0; t < LK_B; t++)
    for (int p = t; p < tl / 2; p += LK_B) {
      long lo = lk_pair_lo(p, j), hi = lk_pair_hi(lo, j);
      if (lo < 0 || hi >= tl || hi != lo + j) return 10;
      seen[lo]++;
      seen[hi]++;
      bool swap = lk_pair_up(base + lo, k) ? lk_key_lt(keys[hi], keys[lo])
                                           : lk_key_lt(keys[lo], keys[hi]);
      if (swap) std::swap(keys[lo], keys[hi]);
    }
  for (int e = 0; e < tl; e++)
    if (seen[e] != 1) return 11;
  return 0;
}

// dst <- sorted src[0..u) padded to np, as dev_lk_sort launches it
static int walk_sort(const Fp* src, long u, Fp* dst, long np, int* launches) {
  const int tl = (int)lk_tile_len(np);
  Heap<Fp> sh((size_t)tl);  // the tile in LDS
  Heap<unsigned char> seen((size_t)tl), gseen((size_t)np);
  *launches = 0;
  // k_lk_sort_tile
  for (long b = 0; b < lk_tiles(np); b++) {
    const long base = lk_tile_index(b, np, 0);
    for (int t = 0; t < LK_B; t++)
      for (int e = t; e < tl; e += LK_B) {
        long g = lk_tile_index(b, np, e);
        sh[e] = g < u ? fd_from_mont(src[g]) : lk_pad_key();
      }
    for (int k = 2; k <= tl; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        if (int rc = tile_stage(sh.p, seen.p, base, tl, k, j)) return rc;
        if (b == 0) g_stages++;
        g_pairs += tl / 2;
      }
    for (int t = 0; t < LK_B; t++)
      for (int e = t; e < tl; e += LK_B) dst[lk_tile_index(b, np, e)] = sh[e];
  }
  ++*launches;
  for (long k = 2 * tl; k <= np; k <<= 1) {
    // k_lk_sort_global, one launch per stride
    for (long j = k / 2; j >= tl; j >>= 1) {
      memset(gseen.p, 0, (size_t)np);
      for (long b = 0; b < lk_stage_blocks(np); b++)
        for (int t = 0; t < LK_B; t++) {
          long p = b * (long)LK_B + t;
          if (p >= np / 2) continue;
          long lo = lk_pair_lo(p, j), hi = lk_pair_hi(lo, j);
          if (hi != lo + j) return 12;
          gseen[lo]++;
          gseen[hi]++;
          bool swap = lk_pair_up(lo, k) ? lk_key_lt(dst[hi], dst[lo])
                                        : lk_key_lt(dst[lo], dst[hi]);
          if (swap) std::swap(dst[lo], dst[hi]);
        }
      for (long e = 0; e < np; e++)
        if (gseen[e] != 1) return 13;
      g_stages++;
      g_pairs += np / 2;
      ++*launches;
    }
    // k_lk_sort_merge
    for (long b = 0; b < lk_tiles(np); b++) {
      const long base = lk_tile_index(b, np, 0);
      for (int e = 0; e < tl; e++) sh[e] = dst[lk_tile_index(b, np, e)];
      for (int j = tl >> 1; j > 0; j >>= 1) {
        if (int rc = tile_stage(sh.p, seen.p, base, tl, k, j)) return rc;
        if (b == 0) g_stages++;
        g_pairs += tl / 2;
      }
      for (int e = 0; e < tl; e++) dst[lk_tile_index(b, np, e)] = sh[e];
    }
    ++*launches;
  }
  return 0;
}

// permute_expression_pair as the provers' serial loop states it, on
// canonical values
static bool serial_pair(std::vector<Fp> a, std::vector<Fp> t, std::vector<Fp>& ap,
                        std::vector<Fp>& sp) {
  const long u = (long)a.size();
  std::sort(a.begin(), a.end(), lk_key_lt);
  std::sort(t.begin(), t.end(), lk_key_lt);
  sp.assign(u, Fp{});
  std::vector<Fp> leftover;
  std::vector<long> repeats;
  long j = 0;
  for (long i = 0; i < u; i++) {
    if (i == 0 || !fd_eq(a[i], a[i - 1])) {
      while (j < u && lk_key_lt(t[j], a[i])) leftover.push_back(t[j++]);
      if (j >= u || !fd_eq(t[j], a[i])) return false;
      sp[i] = t[j++];
    } else {
      repeats.push_back(i);
    }
  }
  while (j < u) leftover.push_back(t[j++]);
  if (leftover.size() != repeats.size()) return false;
  for (size_t r = 0; r < repeats.size(); r++) sp[repeats[r]] = leftover[r];
  ap = a;
  return true;
}

static int run(long u) {
  // a table of u values with repeats, keys that differ in limb 3 and in
  // limb 0; the inputs are drawn from a part of it
  std::vector<Fp> s_can(u), a_can(u);
  for (long i = 0; i < u; i++)
    s_can[i] = Fp{{next_u64() % 61, 0, next_u64() % 3 ? 0 : 1ULL << 40, next_u64() % 5}};
  const long hot = u / 3 + 1;
  for (long i = 0; i < u; i++) a_can[i] = s_can[next_u64() % hot];
  std::vector<Fp> ap_ref, sp_ref;
  if (!serial_pair(a_can, s_can, ap_ref, sp_ref)) return 20;

  const long np = lk_padded(u);
  if (np < u || (np & (np - 1)) || (np > 1 && np / 2 >= u)) return 21;
  if (lk_tiles(np) * lk_tile_len(np) != np) return 22;
  Heap<Fp> src_a((size_t)u), src_s((size_t)u), ap((size_t)np), t((size_t)np), sp((size_t)u);
  for (long i = 0; i < u; i++) {
    src_a[i] = fd_to_mont(a_can[i]);
    src_s[i] = fd_to_mont(s_can[i]);
  }
  g_stages = g_pairs = 0;
  int la = 0, lt = 0;
  if (int rc = walk_sort(src_a.p, u, ap.p, np, &la)) return rc;
  const long stages = g_stages, pairs = g_pairs;
  if (int rc = walk_sort(src_s.p, u, t.p, np, &lt)) return rc;
  if (la != lt || la != lk_sort_launches(np)) return 23;

  // dev_lk_permute with one lookup: flags | scan | lpos, m = 2u flat flags
  const int l = 0;
  const size_t m = 2 * (size_t)u;
  Heap<uint32_t> flags(m), scan(m), lpos((size_t)u);
  uint32_t err = 0;
  // k_lk_first
  for (long b = 0; b < lk_row_blocks(u); b++)
    for (int th = 0; th < LK_B; th++) {
      long i = b * (long)LK_B + th;
      if (i >= u) continue;
      bool first = i == 0 || !fd_eq(ap[i], ap[i - 1]);
      flags[lk_first_at(l, u, i)] = first;
      if (!first) continue;
      long p = lk_lower_bound(t.p, u, ap[i]);
      if (p == u || !fd_eq(t[p], ap[i])) err |= LK_ERR_MISSING;
      else flags[lk_taken_at(l, u, p)] = 1;
    }
  if (err) return 24;
  // the exclusive scan over the flat flags (msm_scan on the device)
  uint32_t acc = 0;
  for (size_t i = 0; i < m; i++) {
    scan[i] = acc;
    acc += flags[i];
  }
  // k_lk_leftover
  for (long b = 0; b < lk_row_blocks(u); b++)
    for (int th = 0; th < LK_B; th++) {
      long p = b * (long)LK_B + th;
      if (p >= u) continue;
      long at = lk_taken_at(l, u, p);
      if (flags[at]) continue;
      long r = lk_clear_rank(p, scan[at], scan[lk_taken_at(l, u, 0)]);
      lpos[(size_t)l * u + r] = (uint32_t)p;
    }
  // k_lk_write
  for (long b = 0; b < lk_row_blocks(u); b++)
    for (int th = 0; th < LK_B; th++) {
      long i = b * (long)LK_B + th;
      if (i >= u) continue;
      Fp a = ap[i], sv = a;
      long at = lk_first_at(l, u, i);
      if (!flags[at]) {
        long r = lk_clear_rank(i, scan[at], scan[lk_first_at(l, u, 0)]);
        uint32_t q = lpos[(size_t)l * u + r];
        if (q >= u) return 25;
        sv = t[q];
      }
      ap[i] = fd_to_mont(a);
      sp[i] = fd_to_mont(sv);
    }
  for (long i = 0; i < u; i++) {
    if (!fd_eq(fd_from_mont(ap[i]), ap_ref[i])) return 26;
    if (!fd_eq(fd_from_mont(sp[i]), sp_ref[i])) return 27;
  }
  printf("%ld np=%ld launches=%d stages=%ld pairs=%ld ok\n", u, np, la, stages, pairs);
  return 0;
}

int main(int argc, char** argv) {
  printf("LK_B=%d LK_TILE=%d\n", LK_B, (int)LK_TILE);
  for (int a = 1; a < argc; a++) {
    long u = atol(argv[a]);
    if (u < 1) return 2;
    if (int rc = run(u)) {
      fprintf(stderr, "u=%ld: check %d failed\n", u, rc);
      return rc;
    }
  }
  return 0;
}
