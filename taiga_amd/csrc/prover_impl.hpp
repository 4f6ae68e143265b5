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

// Capacities of the engine: the one place they are written down. The device
// argument block (HFoldArgs in prover_gpu.inc), the host work arrays of the
// prover and the verifier, and the guards of pdesc_parse are all sized from
// these, and oracle/prover.c carries the same figures. Sized for the exact
// compliance/RL circuits (95+ gates, 17-21 fixed columns, ext 2^19).
constexpr int TG_MAX_K = 24;           // 2^k rows
constexpr int TG_MAX_EXT_RATIO = 32;   // ext_n / n (quotient pieces)
constexpr int TG_MAX_FIXED = 64;
constexpr int TG_MAX_ADVICE = 16;
constexpr int TG_MAX_INSTANCE = 1;     // instance columns
constexpr int TG_MAX_GATES = 256;
constexpr int TG_MAX_PERM = 32;        // permutation columns
constexpr int TG_MAX_CHUNKS = 8;       // permutation product polynomials
constexpr int TG_MAX_LOOKUPS = 4;
constexpr int TG_MAX_LK_EXPRS = 4;     // input (and table) expressions per lookup
constexpr int TG_MAX_QUERIES = 64;     // per kind, and of all kinds together
constexpr int TG_MAX_INSTANCE_Q = 2;
constexpr int TG_MAX_STACK = 8;        // postfix stack peak (DSTK registers)
constexpr int TG_MAX_COL_POINTS = 4;   // distinct rotations queried on one column
constexpr int TG_MAX_POINT_SETS = 16;  // distinct multiopen point sets

// Parses and VALIDATES a TGD1 blob. Returns false — never reads past
// blob+len, never throws — for anything the engine's fixed-size arrays or
// index arithmetic could not hold: a count over its TG_MAX_* limit, an
// index out of range, an unknown op tag, postfix that underflows, ends at
// a depth other than 1 or peaks above TG_MAX_STACK, a query that an
// expression or a permutation column uses but the query lists lack, a
// truncated blob, trailing bytes. `d` is unspecified after a false return.
inline bool pdesc_parse(PDesc& d, const uint8_t* blob, size_t len) {
  const uint8_t* p = blob;
  const uint8_t* end = blob + len;
  auto left = [&]() { return (size_t)(end - p); };
  auto ru32 = [&]() { uint32_t v; memcpy(&v, p, 4); p += 4; return v; };
  auto ri32 = [&]() { int32_t v; memcpy(&v, p, 4); p += 4; return v; };
  if (len < 64 || memcmp(p, "TGD1", 4) != 0) return false;
  p += 4;
  uint32_t hdr[15];
  for (uint32_t& h : hdr) h = ru32();
  // every header word as unsigned, before any becomes an int or a shift
  const uint32_t hmax[15] = {TG_MAX_K, TG_MAX_K + 5, TG_MAX_FIXED, TG_MAX_ADVICE,
                             TG_MAX_INSTANCE, 1u << TG_MAX_K, TG_MAX_GATES,
                             TG_MAX_PERM, 1u << 20, TG_MAX_LOOKUPS,
                             1u << 20, TG_MAX_QUERIES, TG_MAX_QUERIES,
                             TG_MAX_INSTANCE_Q, 1u << TG_MAX_K};
  for (int i = 0; i < 15; i++)
    if (hdr[i] > hmax[i]) return false;
  d.k = (int)hdr[0]; d.ext_k = (int)hdr[1]; d.n_fixed = (int)hdr[2];
  d.n_advice = (int)hdr[3]; d.n_instance = (int)hdr[4]; d.bf = (int)hdr[5];
  d.n_gates = (int)hdr[6]; d.n_perm = (int)hdr[7]; d.chunk_len = (int)hdr[8];
  d.n_lookups = (int)hdr[9]; d.n_consts = (int)hdr[10];
  d.n_advice_q = (int)hdr[11]; d.n_fixed_q = (int)hdr[12];
  d.n_instance_q = (int)hdr[13]; d.n_instance_rows = (int)hdr[14];
  if (d.k < 1 || d.ext_k < d.k) return false;
  d.n = 1L << d.k;
  d.ext_n = 1L << d.ext_k;
  if (d.ext_n / d.n > TG_MAX_EXT_RATIO) return false;
  if ((long)d.bf + 1 >= d.n) return false;
  d.usable = d.n - (d.bf + 1);
  if (d.n_instance_rows > d.usable) return false;
  if (d.n_instance != 1) return false;  // the prover commits exactly one
  if (d.n_advice_q + d.n_fixed_q + d.n_instance_q > TG_MAX_QUERIES) return false;
  // permutation product polynomials: 1..TG_MAX_CHUNKS of them
  if (d.n_perm < 1 || d.chunk_len < 1) return false;
  if ((d.n_perm + d.chunk_len - 1) / d.chunk_len > TG_MAX_CHUNKS) return false;
  auto rd_fp = [&]() {
    Fp v;
    memcpy(v.l, p, 32);
    p += 32;
    return fd_to_mont(v);
  };
  if (left() / 32 < (size_t)d.n_consts) return false;
  d.consts.resize(d.n_consts);
  for (auto& c : d.consts) c = rd_fp();
  auto rd_queries = [&](std::vector<PQuery>& qs, int nq, int ncols) {
    if (left() / 8 < (size_t)nq) return false;
    qs.resize(nq);
    for (auto& q : qs) {
      q.col = ru32();
      q.rot = ri32();
      // rotations are walked step by step when a point is rotated
      if (q.col >= (uint32_t)ncols || q.rot <= -d.n || q.rot >= d.n) return false;
    }
    // one column opens at no more than TG_MAX_COL_POINTS points, each once
    for (size_t i = 0; i < qs.size(); i++) {
      int same = 0;
      for (size_t j = 0; j < qs.size(); j++) {
        if (qs[j].col != qs[i].col) continue;
        if (j < i && qs[j].rot == qs[i].rot) return false;
        same++;
      }
      if (same > TG_MAX_COL_POINTS) return false;
    }
    return true;
  };
  if (!rd_queries(d.advice_q, d.n_advice_q, d.n_advice)) return false;
  if (!rd_queries(d.fixed_q, d.n_fixed_q, d.n_fixed)) return false;
  if (!rd_queries(d.instance_q, d.n_instance_q, d.n_instance)) return false;
  auto listed = [](const std::vector<PQuery>& qs, uint32_t col, int32_t rot) {
    for (const auto& q : qs)
      if (q.col == col && q.rot == rot) return true;
    return false;
  };
  if (left() / 8 < (size_t)d.n_perm) return false;
  d.perm_cols.resize(d.n_perm);
  for (auto& pc : d.perm_cols) {
    pc.first = ru32();   // 0 advice, 1 fixed, 2 instance
    pc.second = ru32();
    if (pc.first > 2) return false;
    const std::vector<PQuery>& qs =
        pc.first == 0 ? d.advice_q : pc.first == 1 ? d.fixed_q : d.instance_q;
    int ncols = pc.first == 0 ? d.n_advice : pc.first == 1 ? d.n_fixed : d.n_instance;
    // the verifier reads a permutation column's value from its query at
    // rotation 0
    if (pc.second >= (uint32_t)ncols || !listed(qs, pc.second, 0)) return false;
  }
  auto rd_expr = [&](PExpr& e) {
    if (left() < 4) return false;
    uint32_t no = ru32();
    if (left() / 12 < no) return false;
    e.ops.resize(no);
    int depth = 0;
    for (auto& op : e.ops) {
      op.tag = ru32();
      op.a = ru32();
      op.b = ri32();
      switch (op.tag) {
        case XCONST:
          if (op.a >= (uint32_t)d.n_consts) return false;
          depth++;
          break;
        case XFIXED:
          if (!listed(d.fixed_q, op.a, op.b)) return false;
          depth++;
          break;
        case XADVICE:
          if (!listed(d.advice_q, op.a, op.b)) return false;
          depth++;
          break;
        case XINSTANCE:
          if (!listed(d.instance_q, op.a, op.b)) return false;
          depth++;
          break;
        case XADD:
        case XSUB:
        case XMUL:
          if (depth < 2) return false;
          depth--;
          break;
        case XSCALE:
          if (op.a >= (uint32_t)d.n_consts) return false;
          [[fallthrough]];
        case XNEG:
          if (depth < 1) return false;
          break;
        default:
          return false;
      }
      if (depth > TG_MAX_STACK) return false;
    }
    return depth == 1;
  };
  d.gates.resize(d.n_gates);
  for (auto& g : d.gates)
    if (!rd_expr(g)) return false;
  d.lookups.resize(d.n_lookups);
  for (auto& l : d.lookups) {
    if (left() < 8) return false;
    uint32_t ni = ru32(), nt = ru32();
    if (ni < 1 || ni > (uint32_t)TG_MAX_LK_EXPRS || nt < 1 ||
        nt > (uint32_t)TG_MAX_LK_EXPRS)
      return false;
    l.in.resize(ni);
    l.tab.resize(nt);
    for (auto& e : l.in)
      if (!rd_expr(e)) return false;
    for (auto& e : l.tab)
      if (!rd_expr(e)) return false;
  }
  // distinct multiopen point sets, as rotation sequences in query order:
  // one per column, {x} for sigma/h/random, the permutation products
  // ({x, wx, w^last x}, the last one without w^last x) and the lookup
  // polynomials ({x, wx}, {x, w^-1 x}, {x})
  {
    std::vector<std::vector<int32_t>> sets;
    auto add_set = [&](const std::vector<int32_t>& s) {
      if (!s.empty() && std::find(sets.begin(), sets.end(), s) == sets.end())
        sets.push_back(s);
    };
    auto col_sets = [&](const std::vector<PQuery>& qs, int ncols) {
      for (int c = 0; c < ncols; c++) {
        std::vector<int32_t> s;
        for (const auto& q : qs)
          if (q.col == (uint32_t)c) s.push_back(q.rot);
        add_set(s);
      }
    };
    col_sets(d.instance_q, d.n_instance);
    col_sets(d.advice_q, d.n_advice);
    col_sets(d.fixed_q, d.n_fixed);
    add_set({0});
    add_set({0, 1});
    if ((d.n_perm + d.chunk_len - 1) / d.chunk_len > 1) add_set({0, 1, -(d.bf + 1)});
    if (d.n_lookups) add_set({0, -1});
    if ((int)sets.size() > TG_MAX_POINT_SETS) return false;
  }
  if (left() / 8 / (size_t)d.n < (size_t)d.n_perm) return false;
  d.sigma_map.resize((size_t)d.n_perm * d.n);
  for (auto& s : d.sigma_map) {
    s.first = ru32();
    s.second = ru32();
    if (s.first >= (uint32_t)d.n_perm || s.second >= (uint64_t)d.n) return false;
  }
  if (left() / 32 / (size_t)d.n < (size_t)d.n_fixed) return false;
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
  Fp stack[TG_MAX_STACK];
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
