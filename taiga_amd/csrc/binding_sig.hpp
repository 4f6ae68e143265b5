// binding_sig.hpp — RedDSA binding signatures over Pallas + the
// transaction binding digest (host-side crypto of the wire layer,
// SURVEY §8f-4; taiga_halo2/src/binding_signature.rs +
// transaction.rs:116-158). PRODUCT CODE.
//
// Restates the PUBLIC RedDSA algorithm (Zcash protocol §5.4.7, the
// reddsa crate) instantiated like the reference's TaigaBinding
// (binding_signature.rs:23-31):
//   - H* = BLAKE2b-512 with personalization "Taiga_RedPallasH", output
//     wide-reduced into the Pallas scalar field (Fq)
//   - signature = R_bytes(32, compressed point) ‖ S_bytes(32, LE scalar)
//   - verify: S·B == R + c·vk with c = H*(R_bytes ‖ vk_bytes ‖ msg)
//   - sign nonce r = H*(T ‖ vk_bytes ‖ msg), T = 80 bytes of caller
//     randomness (here: a ChaCha20 DRBG stream from a 32-byte seed, the
//     same deterministic-randomness convention as the prover)
// Basepoint: the reference's sinsemilla-derived
// RESOURCE_COMMIT_DOMAIN.R() (constant.rs:160), pinned in
// pallas_basepoint() below.
//
// The binding vk aggregates a bundle's delta commitments
// (transaction.rs:99-114): vk = Σ cv_i, sk = Σ r_i, which closes for
// balanced bundles because cv_i = r_i·B once value terms cancel.
#pragma once

#include "host_crypto.hpp"
#include "pasta_device.hpp"

namespace taiga {

using PallasAff = Aff<FpCfg>;  // Pallas: y^2 = x^3 + 5 over Fp, order q
using PallasJac = Jac<FpCfg>;

static const char BS_PERSONAL[17] = "Taiga_RedPallasH";

inline PallasJac pallas_basepoint() {
  // RESOURCE_COMMIT_DOMAIN.R() (constant.rs:160) — the sinsemilla
  // CommitDomain("Taiga-NoteCommit") R point, derived in-repo via the
  // restated pasta group-hash chain and PINNED byte-for-byte against the
  // reference's R_U/R_Z window tables (tests/test_fixed_base_tables.py).
  // Compressed: ac338f5595ca028817a2634b14f0ea18e56e618e36b699aea753ff6adaff8b90
  // Standard-form limbs; converted to Montgomery here.
  static const Fp RX = {{0x8802ca95558f33acULL, 0x18eaf0144b63a217ULL,
                         0xae99b6368e616ee5ULL, 0x108bffda6aff53a7ULL}};
  static const Fp RY = {{0x8c0b30657333c5e1ULL, 0xb8b4f7c83326a380ULL,
                         0x3ebb783b59d92092ULL, 0x1319b788fe5fec16ULL}};
  PallasAff g;
  g.x = fd_to_mont(RX);
  g.y = fd_to_mont(RY);
  return jac_from_aff(g);
}

// [s]P for a Pallas point with an Fq scalar (Mont in, 255-bit double-add;
// host-side, not performance-critical)
inline PallasJac pallas_mul(const PallasJac& p, const Fq& s_mont) {
  Fq s = fd_from_mont(s_mont);
  PallasJac acc = jac_identity<FpCfg>();
  for (int i = 254; i >= 0; i--) {
    acc = jac_dbl(acc);
    if ((s.l[i >> 6] >> (i & 63)) & 1) acc = jac_add(acc, p);
  }
  return acc;
}

// compressed encoding: x.to_repr with y-oddness in bit 255; identity = 0^32
inline void pallas_compress(uint8_t out[32], const PallasJac& p) {
  PallasAff a = jac_to_aff(p);
  if (aff_is_identity(a)) {
    memset(out, 0, 32);
    return;
  }
  Fp x = fd_from_mont(a.x);
  memcpy(out, x.l, 32);
  if (fd_is_odd_std(a.y)) out[31] |= 0x80;
}

inline bool pallas_decompress(PallasJac& out, const uint8_t in[32]) {
  uint8_t b[32];
  memcpy(b, in, 32);
  unsigned sign = b[31] >> 7;
  b[31] &= 0x7F;
  Fp x;
  memcpy(x.l, b, 32);
  bool zero = true;
  for (int i = 0; i < 4; i++)
    if (x.l[i]) zero = false;
  if (zero) {
    if (sign) return false;
    out = jac_identity<FpCfg>();
    return true;
  }
  if (!fd_is_canonical(x)) return false;
  Fp xm = fd_to_mont(x);
  Fp five{{5, 0, 0, 0}};
  Fp rhs = fd_add(fd_mul(fd_sqr(xm), xm), fd_to_mont(five));
  Fp y;
  if (!fd_sqrt(y, rhs)) return false;
  if (fd_is_odd_std(y) != (bool)sign) y = fd_neg(y);
  PallasAff a;
  a.x = xm;
  a.y = y;
  out = jac_from_aff(a);
  return true;
}

// H*(input) -> Fq (BLAKE2b-512, personal "Taiga_RedPallasH", wide reduce)
inline Fq bs_hstar(const uint8_t* a, size_t alen, const uint8_t* b, size_t blen,
                   const uint8_t* c, size_t clen) {
  Blake2b h(64, (const uint8_t*)BS_PERSONAL);
  if (alen) h.update(a, alen);
  if (blen) h.update(b, blen);
  if (clen) h.update(c, clen);
  uint8_t dig[64];
  h.final(dig);
  return from_uniform_512<FqCfg>(dig);
}

inline bool bs_scalar_from_bytes(Fq& out, const uint8_t in[32]) {
  Fq v;
  memcpy(v.l, in, 32);
  if (!fd_is_canonical(v)) return false;
  out = fd_to_mont(v);
  return true;
}

// sk (canonical scalar bytes) -> compressed vk
inline int bs_derive_vk(uint8_t vk_out[32], const uint8_t sk[32]) {
  Fq s;
  if (!bs_scalar_from_bytes(s, sk)) return -1;
  pallas_compress(vk_out, pallas_mul(pallas_basepoint(), s));
  return 0;
}

inline int bs_sign(uint8_t sig_out[64], const uint8_t sk[32], const uint8_t* msg,
                   size_t msg_len, const uint8_t rng_seed[32]) {
  Fq s;
  if (!bs_scalar_from_bytes(s, sk)) return -1;
  uint8_t vk_bytes[32];
  pallas_compress(vk_bytes, pallas_mul(pallas_basepoint(), s));
  uint8_t T[80];
  Drbg rng(rng_seed);
  rng.bytes(T, 80);
  Fq r = bs_hstar(T, 80, vk_bytes, 32, msg, msg_len);
  PallasJac R = pallas_mul(pallas_basepoint(), r);
  pallas_compress(sig_out, R);
  Fq c = bs_hstar(sig_out, 32, vk_bytes, 32, msg, msg_len);
  Fq S = fd_add(r, fd_mul(c, s));
  Fq S_std = fd_from_mont(S);
  memcpy(sig_out + 32, S_std.l, 32);
  return 0;
}

inline int bs_verify(const uint8_t vk_bytes[32], const uint8_t* msg, size_t msg_len,
                     const uint8_t sig[64]) {
  PallasJac vk, R;
  if (!pallas_decompress(vk, vk_bytes)) return -1;
  if (!pallas_decompress(R, sig)) return -1;
  Fq S;
  if (!bs_scalar_from_bytes(S, sig + 32)) return -1;
  Fq c = bs_hstar(sig, 32, vk_bytes, 32, msg, msg_len);
  // S*B == R + c*vk
  PallasJac lhs = pallas_mul(pallas_basepoint(), S);
  PallasJac rhs = jac_add(R, pallas_mul(vk, c));
  PallasAff la = jac_to_aff(lhs), ra = jac_to_aff(rhs);
  if (aff_is_identity(la) != aff_is_identity(ra)) return -1;
  if (!fd_eq(la.x, ra.x) || !fd_eq(la.y, ra.y)) return -1;
  return 0;
}

// binding vk = Σ delta commitments (compressed points) — transaction.rs:99
inline int bs_vk_from_deltas(uint8_t vk_out[32], const uint8_t* deltas, size_t n) {
  PallasJac acc = jac_identity<FpCfg>();
  for (size_t i = 0; i < n; i++) {
    PallasJac p;
    if (!pallas_decompress(p, deltas + 32 * i)) return -1;
    acc = jac_add(acc, p);
  }
  pallas_compress(vk_out, acc);
  return 0;
}

// Transaction::digest (transaction.rs:116-158): BLAKE2b-256, personal
// "TxBindingSigHash", over nullifiers ‖ output_cms ‖ delta_commitments ‖
// anchors (each a 32-byte encoding; the transparent bundle contributes
// the same four streams after the shielded one — pass them concatenated).
inline void bs_tx_digest(uint8_t out[32], const uint8_t* nfs, size_t n_nf,
                         const uint8_t* cms, size_t n_cm, const uint8_t* deltas,
                         size_t n_delta, const uint8_t* anchors, size_t n_anchor) {
  Blake2b h(32, (const uint8_t*)"TxBindingSigHash");
  if (n_nf) h.update(nfs, 32 * n_nf);
  if (n_cm) h.update(cms, 32 * n_cm);
  if (n_delta) h.update(deltas, 32 * n_delta);
  if (n_anchor) h.update(anchors, 32 * n_anchor);
  h.final(out);
}

}  // namespace taiga
