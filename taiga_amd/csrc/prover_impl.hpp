// prover_impl.hpp — the MI355X-native create_proof pipeline. PRODUCT CODE.
// Included at the end of taiga_gpu.cpp (single TU with the kernels + Ctx).
//
// This is the replacement for halo2_proofs::plonk::create_proof behind
// Proof::create (reference taiga_halo2/src/proof.rs:25-42):
// every MSM (column/lookup/z/h/multiopen/IPA commitments) and every NTT
// (lagrange<->coeff, extended-coset transforms) runs on the gfx950 kernels
// (msm.hip / ntt.hip) over device-resident Montgomery data; the host does
// Blake2b Fiat–Shamir, sorting, grand products, gate folding and O(1)
// bookkeeping (north_star split; pointwise stages move device-side next).
//
// Byte-parity: proofs are bit-identical to the CPU oracle
// (oracle/prover.c) on the same SRS/desc/seeds — tests/test_prover_parity.py.

#pragma once

#include "host_crypto.hpp"

#include <algorithm>
#include <cstdlib>

namespace taiga {

// ---------------- circuit description (TGD1 blob) ----------------
enum { XCONST, XFIXED, XADVICE, XINSTANCE, XADD, XSUB, XMUL, XNEG, XSCALE };

struct ExprOp {
  uint32_t tag, a;
  int32_t b;
};
struct PExpr {
  std::vector<ExprOp> ops;
};
struct PQuery {
  uint32_t col;
  int32_t rot;
};
struct PLookup {
  std::vector<PExpr> in, tab;
};

struct PDesc {
  int k, ext_k, n_fixed, n_advice, n_instance, bf;
  int n_gates, n_perm, chunk_len, n_lookups, n_consts;
  int n_advice_q, n_fixed_q, n_instance_q, n_instance_rows;
  long n, ext_n, usable;
  std::vector<Fp> consts;
  std::vector<PQuery> advice_q, fixed_q, instance_q;
  std::vector<std::pair<uint32_t, uint32_t>> perm_cols;
  std::vector<PExpr> gates;
  std::vector<PLookup> lookups;
  std::vector<std::pair<uint32_t, uint32_t>> sigma_map;  // n_perm * n
  std::vector<std::vector<Fp>> fixed_lag;                // Mont
  std::vector<uint8_t> blob;
};

inline bool pdesc_parse(PDesc& d, const uint8_t* blob, size_t len) {
  const uint8_t* p = blob;
  const uint8_t* end = blob + len;
  auto ru32 = [&]() { uint32_t v; memcpy(&v, p, 4); p += 4; return v; };
  auto ri32 = [&]() { int32_t v; memcpy(&v, p, 4); p += 4; return v; };
  if (len < 64 || memcmp(p, "TGD1", 4) != 0) return false;
  p += 4;
  d.k = (int)ru32(); d.ext_k = (int)ru32(); d.n_fixed = (int)ru32();
  d.n_advice = (int)ru32(); d.n_instance = (int)ru32(); d.bf = (int)ru32();
  d.n_gates = (int)ru32(); d.n_perm = (int)ru32(); d.chunk_len = (int)ru32();
  d.n_lookups = (int)ru32(); d.n_consts = (int)ru32();
  d.n_advice_q = (int)ru32(); d.n_fixed_q = (int)ru32();
  d.n_instance_q = (int)ru32(); d.n_instance_rows = (int)ru32();
  d.n = 1L << d.k;
  d.ext_n = 1L << d.ext_k;
  d.usable = d.n - (d.bf + 1);
  // capacity guards, matched to the static device-side arrays
  // (HFoldArgs in prover_gpu.inc) and host stacks; sized for the exact
  // compliance/RL circuits (95+ gates, 17-21 fixed columns, ext 2^19)
  if (d.n_gates > 256 || d.n_fixed > 64 || d.n_advice > 16 || d.n_perm > 32 ||
      d.n_lookups > 4 || d.n_advice_q > 64 || d.n_fixed_q > 64 ||
      d.n_instance_q > 2 || d.n_instance > 1 || (d.ext_n / d.n) > 32)
    return false;
  auto rd_fp = [&]() {
    Fp v;
    memcpy(v.l, p, 32);
    p += 32;
    return fd_to_mont(v);
  };
  d.consts.resize(d.n_consts);
  for (auto& c : d.consts) c = rd_fp();
  auto rd_queries = [&](std::vector<PQuery>& qs, int nq) {
    qs.resize(nq);
    for (auto& q : qs) {
      q.col = ru32();
      q.rot = ri32();
    }
  };
  rd_queries(d.advice_q, d.n_advice_q);
  rd_queries(d.fixed_q, d.n_fixed_q);
  rd_queries(d.instance_q, d.n_instance_q);
  d.perm_cols.resize(d.n_perm);
  for (auto& pc : d.perm_cols) {
    pc.first = ru32();
    pc.second = ru32();
  }
  auto rd_expr = [&](PExpr& e) {
    uint32_t no = ru32();
    e.ops.resize(no);
    for (auto& op : e.ops) {
      op.tag = ru32();
      op.a = ru32();
      op.b = ri32();
    }
  };
  d.gates.resize(d.n_gates);
  for (auto& g : d.gates) rd_expr(g);
  d.lookups.resize(d.n_lookups);
  for (auto& l : d.lookups) {
    uint32_t ni = ru32(), nt = ru32();
    l.in.resize(ni);
    l.tab.resize(nt);
    for (auto& e : l.in) rd_expr(e);
    for (auto& e : l.tab) rd_expr(e);
  }
  d.sigma_map.resize((size_t)d.n_perm * d.n);
  for (auto& s : d.sigma_map) {
    s.first = ru32();
    s.second = ru32();
  }
  d.fixed_lag.resize(d.n_fixed);
  for (int c = 0; c < d.n_fixed; c++) {
    d.fixed_lag[c].resize(d.n);
    for (long i = 0; i < d.n; i++) d.fixed_lag[c][i] = rd_fp();
  }
  if (p != end) return false;
  d.blob.assign(blob, blob + len);
  return true;
}

// ---------------- expression evaluation (host) ----------------
struct PEvalCtx {
  const PDesc* d;
  const std::vector<Fp>* fixed;     // [n_fixed]
  const std::vector<Fp>* advice;    // [n_advice]
  const std::vector<Fp>* instance;  // [n_instance]
  long size;
  long rot_scale;
};

inline Fp pexpr_eval(const PExpr& e, const PEvalCtx& c, long row) {
  Fp stack[16];
  int sp = 0;
  for (const auto& op : e.ops) {
    switch (op.tag) {
      case XCONST: stack[sp++] = c.d->consts[op.a]; break;
      case XFIXED:
      case XADVICE:
      case XINSTANCE: {
        long r = (row + (long)op.b * c.rot_scale) & (c.size - 1);
        const std::vector<Fp>* col = op.tag == XFIXED ? &c.fixed[op.a]
                                     : op.tag == XADVICE ? &c.advice[op.a]
                                                         : &c.instance[op.a];
        stack[sp++] = (*col)[r];
        break;
      }
      case XADD: stack[sp - 2] = fd_add(stack[sp - 2], stack[sp - 1]); sp--; break;
      case XSUB: stack[sp - 2] = fd_sub(stack[sp - 2], stack[sp - 1]); sp--; break;
      case XMUL: stack[sp - 2] = fd_mul(stack[sp - 2], stack[sp - 1]); sp--; break;
      case XNEG: stack[sp - 1] = fd_neg(stack[sp - 1]); break;
      case XSCALE: stack[sp - 1] = fd_mul(stack[sp - 1], c.d->consts[op.a]); break;
    }
  }
  return stack[0];
}

// ---------------- small host field helpers ----------------
inline Fp fp_pow_small(const Fp& base, long e) {
  Fp acc = fd_one_mont<FpCfg>();
  Fp b = base;
  while (e) {
    if (e & 1) acc = fd_mul(acc, b);
    b = fd_sqr(b);
    e >>= 1;
  }
  return acc;
}

// chunked-Horner evaluation (identical result to plain Horner)
inline Fp ppoly_eval(const Fp* coeff, long n, const Fp& x) {
  const int T = 8;
  long chunk = (n + T - 1) / T;
  Fp partial[T];
#ifdef _OPENMP
#pragma omp parallel for schedule(static)
#endif
  for (int t = 0; t < T; t++) {
    long lo = t * chunk, hi = std::min(lo + chunk, n);
    Fp acc = fd_zero<FpCfg>();
    for (long i = hi - 1; i >= lo; i--) acc = fd_add(fd_mul(acc, x), coeff[i]);
    partial[t] = acc;
  }
  Fp xc = fp_pow_small(x, chunk);
  Fp out = fd_zero<FpCfg>(), xp = fd_one_mont<FpCfg>();
  for (int t = 0; t < T; t++) {
    out = fd_add(out, fd_mul(partial[t], xp));
    xp = fd_mul(xp, xc);
  }
  return out;
}

inline void pbatch_inv(Fp* v, long n) {
  // blocked Montgomery trick: one field inversion per block, blocks parallel
  const int T = 16;
  long chunk = (n + T - 1) / T;
#ifdef _OPENMP
#pragma omp parallel for schedule(static)
#endif
  for (int t = 0; t < T; t++) {
    long lo = t * chunk, hi = std::min(lo + chunk, n);
    if (lo >= hi) continue;
    std::vector<Fp> pre(hi - lo);
    Fp run = fd_one_mont<FpCfg>();
    for (long i = lo; i < hi; i++) {
      pre[i - lo] = run;
      if (!fd_is_zero(v[i])) run = fd_mul(run, v[i]);
    }
    Fp inv = fd_inv(run);
    for (long i = hi - 1; i >= lo; i--) {
      if (fd_is_zero(v[i])) continue;
      Fp tt = fd_mul(inv, pre[i - lo]);
      inv = fd_mul(inv, v[i]);
      v[i] = tt;
    }
  }
}

// z[0] = init; z[i+1] = z[i] * r[i] for i < u  (parallel blocked scan)
inline void pprefix_prod(Fp* z, const Fp* r, long u, const Fp& init) {
  const int T = 16;
  long chunk = (u + T - 1) / T;
  Fp bp[T];
#ifdef _OPENMP
#pragma omp parallel for schedule(static)
#endif
  for (int t = 0; t < T; t++) {
    long lo = t * chunk, hi = std::min(lo + chunk, u);
    Fp p = fd_one_mont<FpCfg>();
    for (long i = lo; i < hi; i++) p = fd_mul(p, r[i]);
    bp[t] = p;
  }
  Fp off[T];
  Fp acc = init;
  for (int t = 0; t < T; t++) {
    off[t] = acc;
    acc = fd_mul(acc, bp[t]);
  }
#ifdef _OPENMP
#pragma omp parallel for schedule(static)
#endif
  for (int t = 0; t < T; t++) {
    long lo = t * chunk, hi = std::min(lo + chunk, u);
    Fp p = off[t];
    for (long i = lo; i < hi; i++) {
      z[i] = p;
      p = fd_mul(p, r[i]);
    }
  }
  z[u] = acc;
}

// fixed-point window table: [j] holds tab[w][d] = [d * 2^(8w)] P for
// d in 1..255, w in 0..31 — turns a 255-bit scalar mult of a FIXED point
// (W, U) into <=32 mixed adds.
struct FixedMulTab {
  std::vector<VestaJac> tab;  // 32 windows * 255 digits (jacobian: no
                              // per-entry inversion at init)
  void init(const VestaAff& P) {
    tab.resize(32 * 255);
    VestaJac base = jac_from_aff(P);
    for (int w = 0; w < 32; w++) {
      VestaJac acc = base;
      for (int dd = 1; dd <= 255; dd++) {
        tab[w * 255 + (dd - 1)] = acc;
        acc = jac_add(acc, base);
      }
      base = acc;  // = 256 * base = [2^(8(w+1))] P
    }
  }
  VestaJac mul(const Fd<FpCfg>& s_mont) const {
    Fd<FpCfg> s = fd_from_mont(s_mont);
    VestaJac acc = jac_identity<FqCfg>();
    for (int w = 0; w < 32; w++) {
      unsigned dd = (unsigned)((s.l[w / 8] >> (8 * (w % 8))) & 0xFF);
      if (dd) acc = jac_add(acc, tab[w * 255 + (dd - 1)]);
    }
    return acc;
  }
};

// host jacobian helpers (host side of MSM combine)
inline VestaJac jac_mul_host(const VestaJac& p, const Fp& s_mont) {
  Fp s = fd_from_mont(s_mont);
  VestaJac acc = jac_identity<FqCfg>();
  VestaJac base = p;
  for (int limb = 0; limb < 4; limb++) {
    u64 bits = s.l[limb];
    for (int b = 0; b < 64; b++) {
      if (bits & 1) acc = jac_add(acc, base);
      base = jac_dbl(base);
      bits >>= 1;
    }
  }
  return acc;
}

}  // namespace taiga
