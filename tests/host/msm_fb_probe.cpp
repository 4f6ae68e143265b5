// msm_fb_probe.cpp — host-side runs of two parts of the fixed-base MSM chain
// of msm.hip. TEST CODE: built and driven by tests/test_msm_recode_host.py.
//
// msm_fb_probe <hex scalar>...   the signed-digit recoding (msm_digit, the
//   function k_digits calls per window) at the chain's window width. First
//   line "# c nwin", then per 64-digit hex scalar its nwin signed digits,
//   lowest window first, and the carry left after the top window.
// msm_fb_probe reduce            the one-bucket-set reduction (k_bucket_segsum
//   at MSM_FB_SEG, then k_window_sum<32> with up to 32 chunks), loops in place
//   of lanes and blocks (msm_probe_common.hpp), against sum_d (d+1)*B_d
//   computed another way. One line "<name> OK|FAIL" per case and batch element.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "msm_probe_common.hpp"

static VestaJac naive(const VestaJac* B, int N) {
  // sum_d (d+1)*B_d by the suffix-sum walk
  VestaJac run = jac_identity<FqCfg>(), acc = jac_identity<FqCfg>();
  for (int d = N - 1; d >= 0; d--) {
    run = jac_add(run, B[d]);
    acc = jac_add(acc, run);
  }
  return acc;
}

static int failures = 0;

// single >= 0: only that bucket is occupied, and the expected sum is one
// small multiplication
static void check(const std::string& name, const std::vector<VestaJac>& buckets, int B,
                  int single = -1) {
  std::vector<VestaJac> got = reduce<MSM_WS_KWIDE>(buckets, B, MSM_FB_NBUCK, MSM_FB_SEG);
  for (int b = 0; b < B; b++) {
    VestaAff x = jac_to_aff(got[b]);
    VestaAff y = jac_to_aff(single >= 0
                                ? mul_small(buckets[single], (u64)single + 1)
                                : naive(buckets.data() + (size_t)b * MSM_FB_NBUCK, MSM_FB_NBUCK));
    bool ok = fd_eq(x.x, y.x) && fd_eq(x.y, y.y);
    if (!ok) failures++;
    printf("%s.b%d %s\n", name.c_str(), b, ok ? "OK" : "FAIL");
  }
}

static int run_reduce() {
  make_table();
  const int N = MSM_FB_NBUCK;
  const VestaJac id = jac_identity<FqCfg>();
  {  // dense, two batch elements
    std::vector<VestaJac> b(2 * (size_t)N);
    VestaJac cur = id;
    for (size_t d = 0; d < b.size(); d++) {
      cur = jac_add(cur, pts[sm64(77 * 65536 + d) & 15]);
      b[d] = cur;
    }
    check("random", b, 2);
  }
  check("allid", std::vector<VestaJac>(N, id), 1);
  check("allequal", std::vector<VestaJac>(N, pts[3]), 1);
  // one bucket alone: both ends, and either side of every second power of two, and of the
  // chunk length
  // (where a segment, a chunk lane's bit plane or a chunk index bit turns over)
  std::vector<int> at = {0, N - 1, MSM_FB_SEG * MSM_WS_WIDTH - 1, MSM_FB_SEG * MSM_WS_WIDTH, N / 2 - 1, N / 2};
  for (int p = 1; p < N; p <<= 2) {
    at.push_back(p - 1 > 0 ? p - 1 : 1);
    at.push_back(p);
  }
  for (int d : at) {
    std::vector<VestaJac> b(N, id);
    b[d] = pts[d & 15];
    check("single." + std::to_string(d), b, 1, d);
  }
  return failures ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "reduce")) return run_reduce();
  const MsmCfg cfg = msm_plan_fixed(nullptr, 1).cfg;
  printf("# %d %d\n", cfg.c, cfg.nwin);
  for (int a = 1; a < argc; a++) {
    if (strlen(argv[a]) != 64) return 2;
    ScalarRepr s;
    for (int i = 0; i < 4; i++) {
      char limb[17];
      memcpy(limb, argv[a] + 16 * (3 - i), 16);
      limb[16] = 0;
      s.l[i] = strtoull(limb, nullptr, 16);
    }
    uint32_t carry = 0;
    for (int w = 0; w < cfg.nwin; w++) {
      uint32_t sign;
      uint32_t d = msm_digit(s, w, cfg.c, carry, sign);
      printf("%s%u ", sign ? "-" : "", d);
    }
    printf("%u\n", carry);
  }
  return 0;
}
