// fd52.hpp — EXPERIMENT (round 8, negative result): Montgomery multiply
// whose limb products run on the FP64 FMA pipe (Emmart's 52-bit split).
//
// Measured on gfx950 it is no faster than the integer CIOS form
// (fdmul_bench.hip; numbers in profiles/README.md, Round 8, and DESIGN.md
// section 9 item 2): v_mad_u64_u32 issues at the same rate as v_fma_f64
// there, so moving the products buys nothing and the split costs four FP64
// operations per limb product. The product library does not use it. It is
// kept, exact and tested (tests/test_fd_mul_variants_host.py), so that the
// measurement can be repeated.
#pragma once

#include "../../taiga_amd/csrc/pasta_device.hpp"

namespace taiga {

// Operands are cut into five 52-bit limbs held as doubles. For
// integers 0 <= x, y < 2^52 (round-to-nearest, the default mode):
//   hi = fma(x, y, 2^104)        = 2^104 + H*2^52, H = round(x*y / 2^52)
//   lo = fma(x, y, 2^104 - hi)   = x*y - H*2^52, exact, |lo| <= 2^51
// so bits(hi) - bits(2^104) == H and bits(lo + 1.5*2^52) - bits(1.5*2^52)
// == lo as integers: the bit patterns are summed in 64-bit columns and the
// constants taken off as integers. No carry chain until the end.
//
// Five 52-bit Montgomery steps divide by 2^260. Both operands are cut as
// limbs of 4a and 4b (4a < 2^258), so the result is 16ab / 2^260 = ab / R
// with R = 2^256 unchanged, and T / 2^260 < 16ab / 2^260 + p < 2p for
// a, b < p: one conditional subtraction, as in the integer form. The
// modulus is 2^254 + t, t < 2^126: limbs 0..2 of p are products, limb 3 is
// zero and limb 4 is the single bit 2^46, a shift.
constexpr u64 F52_MASK = (1ULL << 52) - 1;
constexpr u64 F52_K52 = 0x4330000000000000ULL;   // bits(2^52)
constexpr u64 F52_K104 = 0x4670000000000000ULL;  // bits(2^104)
constexpr u64 F52_K15 = 0x4338000000000000ULL;   // bits(1.5 * 2^52)

template <class C>
struct F52Cfg {
  static constexpr double P0 = (double)(C::MOD[0] & F52_MASK);
  static constexpr double P1 = (double)(((C::MOD[0] >> 52) | (C::MOD[1] << 12)) & F52_MASK);
  static constexpr double P2 = (double)(((C::MOD[1] >> 40) | (C::MOD[2] << 24)) & F52_MASK);
  static_assert((((C::MOD[2] >> 28) | (C::MOD[3] << 36)) & F52_MASK) == 0, "limb 3 of p");
  static_assert((C::MOD[3] >> 16) == (1ULL << 46), "limb 4 of p");
  static constexpr double NINV = (double)(C::INV & F52_MASK);  // -p^-1 mod 2^52
};

TG_HD double f52_from_bits(u64 v) { return __builtin_bit_cast(double, v); }
TG_HD u64 f52_bits(double v) { return __builtin_bit_cast(u64, v); }

// integer v < 2^52 -> double
TG_HD double f52_limb(u64 v) { return f52_from_bits(v | F52_K52) - 0x1p52; }

// x*y = H*2^52 + L; returns hb = F52_K104 + H and lb = F52_K15 + L
TG_HD void f52_prod(double x, double y, u64& hb, u64& lb) {
  double hi = __builtin_fma(x, y, 0x1p104);
  double lo = __builtin_fma(x, y, 0x1p104 - hi);
  hb = f52_bits(hi);
  lb = f52_bits(lo + 0x1.8p52);
}

// the five 52-bit limbs of 4a
template <class C>
TG_HD void f52_split4(const Fd<C>& a, double x[5]) {
  x[0] = f52_limb((a.l[0] << 2) & F52_MASK);
  x[1] = f52_limb(((a.l[0] >> 50) | (a.l[1] << 14)) & F52_MASK);
  x[2] = f52_limb(((a.l[1] >> 38) | (a.l[2] << 26)) & F52_MASK);
  x[3] = f52_limb(((a.l[2] >> 26) | (a.l[3] << 38)) & F52_MASK);
  x[4] = f52_limb(a.l[3] >> 14);
}

// Montgomery-reduce ten signed 52-bit columns (two's complement in u64,
// |col| < 2^57) by 2^260 and return the canonical value.
template <class C>
TG_HD Fd<C> f52_reduce(u64 col[10]) {
  using K = F52Cfg<C>;
#pragma unroll
  for (int i = 0; i < 5; i++) {
    // m = col[i] * (-p^-1) mod 2^52, its low half taken by the same split
    double cd = f52_limb(col[i] & F52_MASK);
    double h = __builtin_fma(cd, K::NINV, 0x1p104);
    double l = __builtin_fma(cd, K::NINV, 0x1p104 - h);
    // (L + 2^51) mod 2^52 with bit 51 flipped back is L mod 2^52
    u64 mi = (f52_bits(l + 0x1.8p52) ^ (1ULL << 51)) & F52_MASK;
    double md = f52_limb(mi);
    u64 hb, lb;
    f52_prod(md, K::P0, hb, lb);
    col[i] += lb - F52_K15;
    col[i + 1] += hb - F52_K104;
    f52_prod(md, K::P1, hb, lb);
    col[i + 1] += lb - F52_K15;
    col[i + 2] += hb - F52_K104;
    f52_prod(md, K::P2, hb, lb);
    col[i + 2] += lb - F52_K15;
    col[i + 3] += hb - F52_K104;
    col[i + 4] += (mi & 63) << 46;  // m * 2^46, cut at the column edge
    col[i + 5] += mi >> 6;
    // col[i] is now a multiple of 2^52: only its carry lives on
    col[i + 1] += (u64)((int64_t)col[i] >> 52);
  }
  u64 r[5];
  u64 carry = 0;
#pragma unroll
  for (int k = 0; k < 5; k++) {
    u64 v = col[5 + k] + carry;
    r[k] = k < 4 ? (v & F52_MASK) : v;
    carry = (u64)((int64_t)v >> 52);
  }
  Fd<C> out{{r[0] | (r[1] << 52), (r[1] >> 12) | (r[2] << 40), (r[2] >> 24) | (r[3] << 28),
             (r[3] >> 36) | (r[4] << 16)}};
  fd_reduce_once(out);
  return out;
}

template <class C>
TG_HD Fd<C> fd_mul_f52(const Fd<C>& a, const Fd<C>& b) {
  double x[5], y[5];
  f52_split4(a, x);
  f52_split4(b, y);
  u64 col[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 5; i++) {
#pragma unroll
    for (int j = 0; j < 5; j++) {
      u64 hb, lb;
      f52_prod(x[i], y[j], hb, lb);
      col[i + j] += lb - F52_K15;
      col[i + j + 1] += hb - F52_K104;
    }
  }
  return f52_reduce<C>(col);
}

// 15 limb products instead of 25: the off-diagonal ones are summed apart
// and doubled as integers (doubling a limb would leave the 2^52 range).
template <class C>
TG_HD Fd<C> fd_sqr_f52(const Fd<C>& a) {
  double x[5];
  f52_split4(a, x);
  u64 col[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  u64 off[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 5; i++) {
    u64 hb, lb;
    f52_prod(x[i], x[i], hb, lb);
    col[2 * i] += lb - F52_K15;
    col[2 * i + 1] += hb - F52_K104;
#pragma unroll
    for (int j = i + 1; j < 5; j++) {
      f52_prod(x[i], x[j], hb, lb);
      off[i + j] += lb - F52_K15;
      off[i + j + 1] += hb - F52_K104;
    }
  }
#pragma unroll
  for (int k = 0; k < 10; k++) col[k] += off[k] << 1;
  return f52_reduce<C>(col);
}

}  // namespace taiga
