// msm_reduce_probe.cpp — host-side run of the MSM bucket reduction of msm.hip:
// the level-1 segment sums and the level-2 bit-plane window sum are TG_HD
// functions, so this program runs them with loops in place of lanes, over
// bucket arrays that reach their edge cases, for every row of msm_cfg().
// TEST CODE: built and driven by tests/test_msm_reduce_host.py; it has its own
// main and takes no input, so it also runs stand-alone (e.g. under host
// sanitizers). Calls no HIP runtime function: runs without a GPU.
//
// Each window sum is compared, as an affine point, with the naive
// sum_d (d+1)*B_d (double-and-add per bucket, then summed). Output, one line
// per window:   <c> <case> <OK|FAIL> <x> <y>      (affine, standard form)
// Exit status 1 if any line is FAIL.
//
// Buckets are known multiples of the generator, so the driver can also check
// x, y against one scalar multiplication. The construction it mirrors:
//   r[i]  = sm64(0xC0FFEE + i), i < 16        pts[i] = [r[i]]G
//   walk(seed): K_d = K_{d-1} + r[sm64(seed * 65536 + d) & 15], K_{-1} = 0
//   dbl(i) = [2 r[i]]G
// Cases (N buckets, s = msm_red_seg(N)):
//   random      B_d = [K_d]G, walk(c)
//   allid       all identity
//   single.<d>  only B_d = dbl(d & 15)
//   allequal    every B_d = dbl(3)
//   negpairs0   B_2i = [K_i]G, B_2i+1 = -B_2i, walk(c + 100)
//   negpairs1   B_0 = dbl(5), B_2i+1 = [K_i]G, B_2i+2 = -B_2i+1 (i < N/2-1),
//               B_N-1 = dbl(7), walk(c + 101): the pairs straddle segments
//   b2a.w0/.w1  two windows in the batch layout: identity, then walk(c + 200)
//   b2b.w0/.w1  walk(c + 201), then identity

#include <cinttypes>
#include <cstdio>
#include <set>
#include <string>
#include <vector>

#include "msm_probe_common.hpp"

static std::string hex(const Fq& a) {
  char buf[65];
  snprintf(buf, sizeof buf, "%016" PRIx64 "%016" PRIx64 "%016" PRIx64 "%016" PRIx64, a.l[3],
           a.l[2], a.l[1], a.l[0]);
  return buf;
}

static std::vector<VestaJac> walk(u64 seed, int n) {
  std::vector<VestaJac> out(n);
  VestaJac cur = jac_identity<FqCfg>();
  for (int d = 0; d < n; d++) {
    cur = jac_add(cur, pts[sm64(seed * 65536 + (u64)d) & 15]);
    out[d] = cur;
  }
  return out;
}

// the reference: sum_d (d+1)*B_d
static VestaJac naive(const VestaJac* B, int N) {
  VestaJac acc = jac_identity<FqCfg>();
  for (int d = 0; d < N; d++)
    if (!jac_is_identity(B[d])) acc = jac_add(acc, mul_small(B[d], (u64)d + 1));
  return acc;
}

static int failures = 0;

static void check(int c, const std::string& name, const std::vector<VestaJac>& buckets, int nwin,
                  int N) {
  std::vector<VestaJac> got = reduce<MSM_WS_KMAX>(buckets, nwin, N, msm_red_seg(N));
  for (int w = 0; w < nwin; w++) {
    VestaAff a = jac_to_aff(got[w]);
    VestaAff b = jac_to_aff(naive(buckets.data() + (size_t)w * N, N));
    bool ok = fd_eq(a.x, b.x) && fd_eq(a.y, b.y);
    if (!ok) failures++;
    std::string nm = nwin > 1 ? name + ".w" + std::to_string(w) : name;
    printf("%d %s %s %s %s\n", c, nm.c_str(), ok ? "OK" : "FAIL", hex(fd_from_mont(a.x)).c_str(),
           hex(fd_from_mont(a.y)).c_str());
  }
}

int main() {
  make_table();
  const long sizes[] = {1 << 10, 1 << 11, 1 << 12, 1 << 13, 1 << 14, 1 << 15, 1 << 18};
  for (long n : sizes) {
    MsmCfg cfg = msm_cfg(n);
    const int c = cfg.c, N = cfg.nbuck;
    const int s = msm_red_seg(N), M = N / s, Wd = msm_ws_width(M);
    const VestaJac id = jac_identity<FqCfg>();
    printf("# c=%d nbuck=%d s=%d M=%d width=%d\n", c, N, s, M, Wd);

    check(c, "random", walk((u64)c, N), 1, N);
    check(c, "allid", std::vector<VestaJac>(N, id), 1, N);

    // single buckets: segment edges, every power of two (the plane and
    // tree-region boundaries, in segments and in buckets), the chunk
    // boundaries, and both ends
    std::set<int> ds = {0, 1, s - 1, s, s + 1, N - 2, N - 1};
    for (int p = 1; p < N; p <<= 1)
      for (int d : {p - 1, p, p + 1}) ds.insert(d);
    for (int k = 1; k < M / Wd; k++)
      for (int d : {s * Wd * k - 1, s * Wd * k, s * Wd * k + 1}) ds.insert(d);
    for (int d : ds) {
      if (d < 0 || d >= N) continue;
      std::vector<VestaJac> b(N, id);
      b[d] = jac_dbl(pts[d & 15]);
      check(c, "single." + std::to_string(d), b, 1, N);
    }

    check(c, "allequal", std::vector<VestaJac>(N, jac_dbl(pts[3])), 1, N);

    {
      std::vector<VestaJac> x = walk((u64)c + 100, N / 2), b(N);
      for (int i = 0; i < N / 2; i++) {
        b[2 * i] = x[i];
        b[2 * i + 1] = jac_neg(x[i]);
      }
      check(c, "negpairs0", b, 1, N);
    }
    {
      std::vector<VestaJac> x = walk((u64)c + 101, N / 2 - 1), b(N);
      b[0] = jac_dbl(pts[5]);
      for (int i = 0; i < N / 2 - 1; i++) {
        b[2 * i + 1] = x[i];
        b[2 * i + 2] = jac_neg(x[i]);
      }
      b[N - 1] = jac_dbl(pts[7]);
      check(c, "negpairs1", b, 1, N);
    }
    {
      std::vector<VestaJac> b(2 * (size_t)N, id), x = walk((u64)c + 200, N);
      for (int d = 0; d < N; d++) b[N + d] = x[d];
      check(c, "b2a", b, 2, N);
    }
    {
      std::vector<VestaJac> b(2 * (size_t)N, id), x = walk((u64)c + 201, N);
      for (int d = 0; d < N; d++) b[d] = x[d];
      check(c, "b2b", b, 2, N);
    }
  }
  return failures ? 1 : 0;
}
