// arith_probe.cpp — host-side probe of the product's __host__ __device__
// arithmetic (pasta_device.hpp), the host parts of msm.hip (msm_cfg,
// msm_host_combine) and the fd28 experiment (tools/experiments/fd28.hpp).
// TEST CODE: built and driven by tests/test_host_arith.py and test_fd28.py.
//
// Reads one operation per line from stdin, prints one line of hex results.
// Calls no HIP runtime function, so it runs on a machine without a GPU.
//
// Field elements travel as 64 hex digits (big-endian integer). Field lines
// are "<op> <p|q> <args...>":
//   raw ops work on the limbs as given (what the kernels see):
//     add a b | sub a b | neg a | mul a b | sqr a | tomont a | frommont a |
//     isodd a | rt a | canon a   (canon prints 1 iff a < modulus)
//   standard-form ops convert to Montgomery form, run, and convert back:
//     inv a | pow a e(decimal u64) | sqrt a   (sqrt prints "<flag> [root]")
// Curve lines (Vesta; every coordinate in standard form, converted here):
//   jdbl X Y Z | jadd X1 Y1 Z1 X2 Y2 Z2 | jadda X Y Z x y | jaddi X Y Z x y |
//   jaddf X Y Z x y | jneg X Y Z        -> "X Y Z"
//   aneg x y | anegf x y | j2a X Y Z   -> "x y"
//   comb c nwin (X Y Z)*nwin           -> "x y"
//   cfg n -> "c nwin nbuck nseg seg" ; consts -> the MSM_* constants
// fd28 experiment (Fp): mul28 a b -> a*b*2^-280 mod p, or "NONCANONICAL" when
//   an operand is not below p

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "pasta_device.hpp"
#include "msm.hip"
#include "fd28.hpp"

using namespace taiga;

static bool parse_hex(const std::string& s, u64 l[4]) {
  if (s.size() != 64) return false;
  for (int i = 0; i < 4; i++) {
    u64 v = 0;
    for (int j = 0; j < 16; j++) {
      char ch = s[(3 - i) * 16 + j];
      int d;
      if (ch >= '0' && ch <= '9') d = ch - '0';
      else if (ch >= 'a' && ch <= 'f') d = ch - 'a' + 10;
      else if (ch >= 'A' && ch <= 'F') d = ch - 'A' + 10;
      else return false;
      v = (v << 4) | (u64)d;
    }
    l[i] = v;
  }
  return true;
}

template <class C>
static std::string hex(const Fd<C>& a) {
  char buf[65];
  snprintf(buf, sizeof buf, "%016" PRIx64 "%016" PRIx64 "%016" PRIx64 "%016" PRIx64,
           a.l[3], a.l[2], a.l[1], a.l[0]);
  return buf;
}

template <class C>
static bool get(const std::vector<std::string>& t, size_t i, Fd<C>& out) {
  return i < t.size() && parse_hex(t[i], out.l);
}

template <class C>
static bool field_op(const std::vector<std::string>& t, std::string& out) {
  const std::string& op = t[0];
  Fd<C> a, b;
  if (!get(t, 2, a)) return false;
  if (op == "add" || op == "sub" || op == "mul") {
    if (!get(t, 3, b)) return false;
    out = hex(op == "add" ? fd_add(a, b) : op == "sub" ? fd_sub(a, b) : fd_mul(a, b));
  } else if (op == "neg") {
    out = hex(fd_neg(a));
  } else if (op == "sqr") {
    out = hex(fd_sqr(a));
  } else if (op == "tomont") {
    out = hex(fd_to_mont(a));
  } else if (op == "frommont") {
    out = hex(fd_from_mont(a));
  } else if (op == "rt") {
    out = hex(fd_from_mont(fd_to_mont(a)));
  } else if (op == "isodd") {
    out = fd_is_odd_std(a) ? "1" : "0";
  } else if (op == "canon") {
    out = fd_is_canonical(a) ? "1" : "0";
  } else if (op == "inv") {
    out = hex(fd_from_mont(fd_inv(fd_to_mont(a))));
  } else if (op == "pow") {
    if (t.size() < 4) return false;
    u64 e = strtoull(t[3].c_str(), nullptr, 10);
    out = hex(fd_from_mont(fd_pow_u64(fd_to_mont(a), e)));
  } else if (op == "sqrt") {
    Fd<C> r;
    if (fd_sqrt(r, fd_to_mont(a)))
      out = "1 " + hex(fd_from_mont(r));
    else
      out = "0";
  } else {
    return false;
  }
  return true;
}

static bool get_jac(const std::vector<std::string>& t, size_t i, VestaJac& p) {
  Fq x, y, z;
  if (!get(t, i, x) || !get(t, i + 1, y) || !get(t, i + 2, z)) return false;
  p.x = fd_to_mont(x);
  p.y = fd_to_mont(y);
  p.z = fd_to_mont(z);
  return true;
}

static bool get_aff(const std::vector<std::string>& t, size_t i, VestaAff& p) {
  Fq x, y;
  if (!get(t, i, x) || !get(t, i + 1, y)) return false;
  p.x = fd_to_mont(x);
  p.y = fd_to_mont(y);
  return true;
}

static std::string put_jac(const VestaJac& p) {
  return hex(fd_from_mont(p.x)) + " " + hex(fd_from_mont(p.y)) + " " + hex(fd_from_mont(p.z));
}

static std::string put_aff(const VestaAff& p) {
  return hex(fd_from_mont(p.x)) + " " + hex(fd_from_mont(p.y));
}

static bool curve_op(const std::vector<std::string>& t, std::string& out) {
  const std::string& op = t[0];
  VestaJac p, q;
  VestaAff a;
  if (op == "jdbl") {
    if (!get_jac(t, 1, p)) return false;
    out = put_jac(jac_dbl(p));
  } else if (op == "jadd") {
    if (!get_jac(t, 1, p) || !get_jac(t, 4, q)) return false;
    out = put_jac(jac_add(p, q));
  } else if (op == "jadda" || op == "jaddi" || op == "jaddf") {
    if (!get_jac(t, 1, p) || !get_aff(t, 4, a)) return false;
    if (op == "jadda") p = jac_add_aff(p, a);
    else if (op == "jaddi") jac_add_aff_inplace(p, a);
    else jac_add_aff_fast(p, a);
    out = put_jac(p);
  } else if (op == "jneg") {
    if (!get_jac(t, 1, p)) return false;
    out = put_jac(jac_neg(p));
  } else if (op == "aneg" || op == "anegf") {
    if (!get_aff(t, 1, a)) return false;
    out = put_aff(op == "aneg" ? aff_neg(a) : aff_neg_fast(a));
  } else if (op == "j2a") {
    if (!get_jac(t, 1, p)) return false;
    out = put_aff(jac_to_aff(p));
  } else if (op == "comb") {
    if (t.size() < 3) return false;
    MsmCfg cfg{atoi(t[1].c_str()), atoi(t[2].c_str()), 0, 0, 0};
    if (cfg.c < 1 || cfg.nwin < 1 || cfg.nwin > 32) return false;
    VestaJac ws[32];
    for (int w = 0; w < cfg.nwin; w++)
      if (!get_jac(t, 3 + 3 * (size_t)w, ws[w])) return false;
    out = put_aff(msm_host_combine(ws, cfg));
  } else {
    return false;
  }
  return true;
}

int main() {
  std::string line;
  char buf[4096];
  std::string acc;
  while (fgets(buf, sizeof buf, stdin)) {
    acc += buf;
    if (acc.empty() || acc.back() != '\n') continue;
    line.swap(acc);
    acc.clear();
    std::istringstream is(line);
    std::vector<std::string> t;
    for (std::string w; is >> w;) t.push_back(w);
    if (t.empty()) continue;
    std::string out;
    bool ok;
    if (t[0] == "cfg" && t.size() == 2) {
      MsmCfg c = msm_cfg(atol(t[1].c_str()));
      out = std::to_string(c.c) + " " + std::to_string(c.nwin) + " " + std::to_string(c.nbuck) +
            " " + std::to_string(c.nseg) + " " + std::to_string(c.seg);
      ok = true;
    } else if (t[0] == "consts") {
      out = std::to_string(MSM_C_MAX) + " " + std::to_string(MSM_NWIN_MAX) + " " +
            std::to_string(MSM_NBUCK_MAX) + " " + std::to_string(MSM_SEG) + " " +
            std::to_string(MSM_BIG_BUCKET) + " " + std::to_string(MSM_BIG_LANES);
      ok = true;
    } else if (t[0] == "mul28") {
      Fp a, b;
      ok = get(t, 1, a) && get(t, 2, b);
      if (ok && fd_is_canonical(a) && fd_is_canonical(b))
        out = hex(fd28_norm(fd28_mul(fd28_from<FpCfg>(a), fd28_from<FpCfg>(b))));
      else
        out = "NONCANONICAL";
    } else if (t.size() >= 3 && (t[1] == "p" || t[1] == "q")) {
      ok = t[1] == "p" ? field_op<FpCfg>(t, out) : field_op<FqCfg>(t, out);
    } else {
      ok = curve_op(t, out);
    }
    if (!ok) {
      printf("ERR %s\n", t[0].c_str());
      return 2;
    }
    puts(out.c_str());
  }
  return 0;
}
