// fdmul_probe.cpp — host-side probe of the field multiply's other forms:
// the radix-2^30 multiply and squaring the device uses (fd_mul_r30,
// fd_sqr_r30 of pasta_device.hpp) and the FP64-limb experiment (fd_mul_f52,
// fd_sqr_f52, f52_prod of tools/experiments/fd52.hpp), next to the CIOS form
// (fd_mul_int) they must equal.
// TEST CODE: built and driven by tests/test_fd_mul_variants_host.py.
//
// Reads one operation per line from stdin, prints one line per operation.
// Calls no HIP runtime function, so it runs on a machine without a GPU.
// Field elements travel as 64 hex digits (big-endian integer), raw limbs as
// the kernels see them:
//   mulf <p|q> a b -> fd_mul_f52(a, b)     muli <p|q> a b -> fd_mul_int(a, b)
//   sqrf <p|q> a   -> fd_sqr_f52(a)
//   mulr <p|q> a b -> fd_mul_r30(a, b)     sqrr <p|q> a   -> fd_sqr_r30(a)
//   split x y (hex, each < 2^52) -> "H L" (decimal, L signed) with
//     x*y == H*2^52 + L, taken from the bit patterns f52_prod returns

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "pasta_device.hpp"
#include "fd52.hpp"

using namespace taiga;

static bool parse_hex(const char* s, u64 l[4]) {
  if (strlen(s) != 64) return false;
  for (int i = 0; i < 4; i++) {
    u64 v = 0;
    for (int j = 0; j < 16; j++) {
      char ch = s[(3 - i) * 16 + j];
      int d;
      if (ch >= '0' && ch <= '9') d = ch - '0';
      else if (ch >= 'a' && ch <= 'f') d = ch - 'a' + 10;
      else return false;
      v = (v << 4) | (u64)d;
    }
    l[i] = v;
  }
  return true;
}

template <class C>
static void put(const Fd<C>& a) {
  printf("%016" PRIx64 "%016" PRIx64 "%016" PRIx64 "%016" PRIx64 "\n", a.l[3], a.l[2], a.l[1],
         a.l[0]);
}

template <class C>
static bool field_op(const char* op, const char* sa, const char* sb) {
  Fd<C> a, b;
  if (!parse_hex(sa, a.l)) return false;
  if (!strcmp(op, "sqrf") || !strcmp(op, "sqrr")) {
    put(op[3] == 'f' ? fd_sqr_f52(a) : fd_sqr_r30(a));
    return true;
  }
  if (!sb || !parse_hex(sb, b.l)) return false;
  if (!strcmp(op, "mulf")) put(fd_mul_f52(a, b));
  else if (!strcmp(op, "mulr")) put(fd_mul_r30(a, b));
  else if (!strcmp(op, "muli")) put(fd_mul_int(a, b));
  else return false;
  return true;
}

int main() {
  static char line[512];
  while (fgets(line, sizeof line, stdin)) {
    char* t[4] = {nullptr, nullptr, nullptr, nullptr};
    int nt = 0;
    for (char* w = strtok(line, " \n"); w && nt < 4; w = strtok(nullptr, " \n")) t[nt++] = w;
    if (nt == 0) continue;
    bool ok = false;
    if (!strcmp(t[0], "split") && nt == 3) {
      u64 x = strtoull(t[1], nullptr, 16), y = strtoull(t[2], nullptr, 16);
      if (x <= F52_MASK && y <= F52_MASK) {
        u64 hb, lb;
        f52_prod((double)x, (double)y, hb, lb);
        printf("%" PRIu64 " %" PRId64 "\n", hb - F52_K104, (int64_t)(lb - F52_K15));
        ok = true;
      }
    } else if (nt >= 3 && (!strcmp(t[1], "p") || !strcmp(t[1], "q"))) {
      ok = t[1][0] == 'p' ? field_op<FpCfg>(t[0], t[2], t[3]) : field_op<FqCfg>(t[0], t[2], t[3]);
    }
    if (!ok) {
      printf("ERR %s\n", t[0]);
      return 2;
    }
  }
  return 0;
}
