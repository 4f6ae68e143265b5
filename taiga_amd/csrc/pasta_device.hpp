// pasta_device.hpp — CDNA4 (gfx950) device library: Pasta fields and curves.
//
// PRODUCT CODE (taiga_amd / libtaiga_gpu.so). From-scratch MI355X-native
// implementation of the arithmetic behind halo2's create_proof hot path
// (reference boundary: taiga_halo2/src/proof.rs:25-42; the MSM/NTT engine
// lives in the un-vendored heliaxdev/halo2+pasta_curves deps — SURVEY.md
// §8a/§8c). Parity is established against the CPU oracle (oracle/), which
// is itself pinned to the reference's bundled SRS bytes.
//
// Representation: 4x64-limb Montgomery (R = 2^256), on the host and in
// memory. 255-bit modular integer work: VALU v_mad_u64_u32 — no MFMA
// anywhere on this path (it is not a dense contraction). On the device a
// multiply cuts its operands into nine 30-bit limbs and sums the limb
// products in 64-bit columns that cannot overflow (fd_mul_r30): one
// v_mad_u64_u32 per product and no carry flags, where the 4x64 CIOS form
// (fd_mul_int, the host's) spends most of its issue slots on VCC carry
// chains, their hazard padding and register moves. Values enter and leave a
// multiply in the 4x64 form. All limb loops are fully unrolled so limb
// indices are compile-time constants (no scratch spills from runtime
// indexing).

#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// All field/curve primitives are host+device: the GPU kernels use them on
// gfx950, and the thin C-ABI host shim reuses the same code for O(1)-sized
// work (final window combines, transcript scalars) — no second
// implementation to drift.
#define TG_HD __host__ __device__ __forceinline__

#include "pasta_field.hpp"  // the fields; the curves follow here

namespace taiga {

// ---- curve: y^2 = x^3 + 5 over the cfg field ----
// Affine in Montgomery form; (0,0) encodes the identity (x=0 is off-curve
// for b=5 since 5 is a non-residue in both Pasta fields).
template <class C>
struct Aff {
  Fd<C> x, y;
};

// Jacobian; identity is z == 0
template <class C>
struct Jac {
  Fd<C> x, y, z;
};

template <class C>
TG_HD bool aff_is_identity(const Aff<C>& p) {
  return fd_is_zero(p.x) && fd_is_zero(p.y);
}

template <class C>
TG_HD Jac<C> jac_identity() {
  Jac<C> r;
  r.x = fd_zero<C>(); r.y = fd_zero<C>(); r.z = fd_zero<C>();
  return r;
}

template <class C>
TG_HD bool jac_is_identity(const Jac<C>& p) {
  return fd_is_zero(p.z);
}

template <class C>
TG_HD Jac<C> jac_from_aff(const Aff<C>& a) {
  Jac<C> r;
  if (aff_is_identity(a)) return jac_identity<C>();
  r.x = a.x; r.y = a.y; r.z = fd_one_mont<C>();
  return r;
}

// dbl-2009-l (a = 0)
template <class C>
TG_HD Jac<C> jac_dbl(const Jac<C>& p) {
  if (jac_is_identity(p) || fd_is_zero(p.y)) return jac_identity<C>();
  Fd<C> A = fd_sqr(p.x);
  Fd<C> B = fd_sqr(p.y);
  Fd<C> Cc = fd_sqr(B);
  Fd<C> t = fd_sqr(fd_add(p.x, B));
  t = fd_sub(fd_sub(t, A), Cc);
  Fd<C> D = fd_add(t, t);
  Fd<C> E = fd_add(fd_add(A, A), A);
  Fd<C> F = fd_sqr(E);
  Jac<C> r;
  r.x = fd_sub(fd_sub(F, D), D);
  Fd<C> zz = fd_sqr(p.z);
  Fd<C> yz = fd_sub(fd_sub(fd_sqr(fd_add(p.y, p.z)), B), zz);
  r.z = yz;
  Fd<C> c8 = fd_add(Cc, Cc);
  c8 = fd_add(c8, c8);
  c8 = fd_add(c8, c8);
  r.y = fd_sub(fd_mul(fd_sub(D, r.x), E), c8);
  return r;
}

// add-2007-bl full add
template <class C>
TG_HD Jac<C> jac_add(const Jac<C>& p, const Jac<C>& q) {
  if (jac_is_identity(p)) return q;
  if (jac_is_identity(q)) return p;
  Fd<C> z1z1 = fd_sqr(p.z);
  Fd<C> z2z2 = fd_sqr(q.z);
  Fd<C> u1 = fd_mul(p.x, z2z2);
  Fd<C> u2 = fd_mul(q.x, z1z1);
  Fd<C> s1 = fd_mul(fd_mul(p.y, q.z), z2z2);
  Fd<C> s2 = fd_mul(fd_mul(q.y, p.z), z1z1);
  if (fd_eq(u1, u2)) {
    if (fd_eq(s1, s2)) return jac_dbl(p);
    return jac_identity<C>();
  }
  Fd<C> h = fd_sub(u2, u1);
  Fd<C> i = fd_sqr(fd_add(h, h));
  Fd<C> j = fd_mul(h, i);
  Fd<C> rr = fd_sub(s2, s1);
  rr = fd_add(rr, rr);
  Fd<C> v = fd_mul(u1, i);
  Jac<C> r;
  r.x = fd_sub(fd_sub(fd_sub(fd_sqr(rr), j), v), v);
  Fd<C> s1j = fd_mul(s1, j);
  s1j = fd_add(s1j, s1j);
  r.y = fd_sub(fd_mul(fd_sub(v, r.x), rr), s1j);
  Fd<C> t = fd_sub(fd_sub(fd_sqr(fd_add(p.z, q.z)), z1z1), z2z2);
  r.z = fd_mul(t, h);
  return r;
}

// mixed add (q affine, madd-2007-bl)
template <class C>
TG_HD Jac<C> jac_add_aff(const Jac<C>& p, const Aff<C>& q) {
  if (aff_is_identity(q)) return p;
  if (jac_is_identity(p)) return jac_from_aff(q);
  Fd<C> z1z1 = fd_sqr(p.z);
  Fd<C> u2 = fd_mul(q.x, z1z1);
  Fd<C> s2 = fd_mul(fd_mul(q.y, p.z), z1z1);
  if (fd_eq(p.x, u2)) {
    if (fd_eq(p.y, s2)) return jac_dbl(p);
    return jac_identity<C>();
  }
  Fd<C> h = fd_sub(u2, p.x);
  Fd<C> hh = fd_sqr(h);
  Fd<C> i = fd_add(hh, hh);
  i = fd_add(i, i);
  Fd<C> j = fd_mul(h, i);
  Fd<C> rr = fd_sub(s2, p.y);
  rr = fd_add(rr, rr);
  Fd<C> v = fd_mul(p.x, i);
  Jac<C> r;
  r.x = fd_sub(fd_sub(fd_sub(fd_sqr(rr), j), v), v);
  Fd<C> yj = fd_mul(p.y, j);
  yj = fd_add(yj, yj);
  r.y = fd_sub(fd_mul(fd_sub(v, r.x), rr), yj);
  Fd<C> t = fd_sub(fd_sub(fd_sqr(fd_add(p.z, h)), z1z1), hh);
  r.z = t;
  return r;
}


// single-exit, in-place mixed add: acc += q. Same math as jac_add_aff but
// structured to keep every temporary in registers (the multi-return version
// left a 72 B/lane scratch allocation = ~2 GB of spill traffic per 2^20-MSM
// bucket pass).
template <class C>
TG_HD void jac_add_aff_inplace(Jac<C>& acc, const Aff<C>& q) {
  bool q_id = aff_is_identity(q);
  bool p_id = jac_is_identity(acc);
  // general path temporaries
  Fd<C> z1z1 = fd_sqr(acc.z);
  Fd<C> u2 = fd_mul(q.x, z1z1);
  Fd<C> s2 = fd_mul(fd_mul(q.y, acc.z), z1z1);
  bool x_eq = fd_eq(acc.x, u2);
  bool y_eq = fd_eq(acc.y, s2);
  if (!q_id && !p_id && !x_eq) {
    Fd<C> h = fd_sub(u2, acc.x);
    Fd<C> hh = fd_sqr(h);
    Fd<C> i = fd_add(hh, hh);
    i = fd_add(i, i);
    Fd<C> j = fd_mul(h, i);
    Fd<C> rr = fd_sub(s2, acc.y);
    rr = fd_add(rr, rr);
    Fd<C> v = fd_mul(acc.x, i);
    Fd<C> x3 = fd_sub(fd_sub(fd_sub(fd_sqr(rr), j), v), v);
    Fd<C> yj = fd_mul(acc.y, j);
    yj = fd_add(yj, yj);
    Fd<C> y3 = fd_sub(fd_mul(fd_sub(v, x3), rr), yj);
    Fd<C> z3 = fd_sub(fd_sub(fd_sqr(fd_add(acc.z, h)), z1z1), hh);
    acc.x = x3;
    acc.y = y3;
    acc.z = z3;
  } else if (!q_id && !p_id && x_eq && y_eq) {
    acc = jac_dbl(acc);
  } else if (!q_id && !p_id) {
    acc = jac_identity<C>();
  } else if (!q_id) {
    acc = jac_from_aff(q);
  }  // else: q identity, acc unchanged
}


// branch-free mixed add for bucket accumulation over DISTINCT, non-identity
// bases (the SRS / prover path): no identity or equal-x handling, so no
// divergent struct merges (the safe variant's exceptional branches cost a
// 72 B/lane scratch spill ~= 2 GB of HBM traffic per 2^20-MSM bucket pass).
// Precondition: acc != identity, q != identity, acc.x/Z^2 != q.x. A mid-sum
// accidental collision has probability ~2^-127 and any wrong result is
// caught by proof verification.
template <class C>
TG_HD void jac_add_aff_fast(Jac<C>& acc, const Aff<C>& q) {
  Fd<C> z1z1 = fd_sqr(acc.z);
  Fd<C> u2 = fd_mul(q.x, z1z1);
  Fd<C> s2 = fd_mul(fd_mul(q.y, acc.z), z1z1);
  Fd<C> h = fd_sub(u2, acc.x);
  Fd<C> hh = fd_sqr(h);
  Fd<C> i = fd_add(hh, hh);
  i = fd_add(i, i);
  Fd<C> j = fd_mul(h, i);
  Fd<C> rr = fd_sub(s2, acc.y);
  rr = fd_add(rr, rr);
  Fd<C> v = fd_mul(acc.x, i);
  Fd<C> x3 = fd_sub(fd_sub(fd_sub(fd_sqr(rr), j), v), v);
  Fd<C> yj = fd_mul(acc.y, j);
  yj = fd_add(yj, yj);
  acc.y = fd_sub(fd_mul(fd_sub(v, x3), rr), yj);
  acc.z = fd_sub(fd_sub(fd_sqr(fd_add(acc.z, h)), z1z1), hh);
  acc.x = x3;
}

// unguarded negation for non-identity affine points (y != 0)
template <class C>
TG_HD Aff<C> aff_neg_fast(const Aff<C>& p) {
  Aff<C> r;
  r.x = p.x;
  u64 borrow = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    u128 dd = (u128)C::MOD[i] - p.y.l[i] - borrow;
    r.y.l[i] = (u64)dd;
    borrow = (u64)(dd >> 64) ? 1u : 0u;
  }
  return r;
}

template <class C>
TG_HD Jac<C> jac_neg(const Jac<C>& p) {
  Jac<C> r = p;
  if (!jac_is_identity(p)) r.y = fd_neg(p.y);
  return r;
}

template <class C>
TG_HD Aff<C> aff_neg(const Aff<C>& p) {
  Aff<C> r = p;
  if (!aff_is_identity(p)) r.y = fd_neg(p.y);
  return r;
}

// Jacobian -> affine (one inversion; for single points / small batches)
template <class C>
TG_HD Aff<C> jac_to_aff(const Jac<C>& p) {
  Aff<C> r;
  if (jac_is_identity(p)) {
    r.x = fd_zero<C>(); r.y = fd_zero<C>();
    return r;
  }
  Fd<C> zi = fd_inv(p.z);
  Fd<C> zi2 = fd_sqr(zi);
  r.x = fd_mul(p.x, zi2);
  r.y = fd_mul(p.y, fd_mul(zi2, zi));
  return r;
}

using Fp = Fd<FpCfg>;
using Fq = Fd<FqCfg>;
using VestaAff = Aff<FqCfg>;  // commitment curve (scalars in Fp)
using VestaJac = Jac<FqCfg>;

}  // namespace taiga
