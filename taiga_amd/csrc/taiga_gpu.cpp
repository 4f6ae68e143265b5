// taiga_gpu.cpp — C-ABI host shim of libtaiga_gpu.so. PRODUCT CODE.
//
// Thin extern "C" layer over the gfx950 kernels (msm.hip, ntt.hip); see
// include/taiga_gpu.h for the boundary contract and the reference
// interfaces each entry point replaces. No CPU fallback: every entry point
// fails with TG_ERR_HIP when no HIP device works.

#include "../../include/taiga_gpu.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

#include "msm.hip"
#include "ntt.hip"
#include "openings.hip"
#include "grand_products.hip"
#include "lookup_argument.hip"
#include "poseidon.hip"
#include "binding_sig.hpp"
#include "tx_wire.hpp"
#include "witness.hpp"
#include "prover_impl.hpp"
#include "hf_rtc.hpp"
#include "resident_guard.hpp"

namespace taiga {

// ---------- small device kernels for API ingestion ----------

// canonical bytes -> Mont, with canonicality check (err bitmask != 0 on bad)
template <class C>
__global__ void __launch_bounds__(256) k_to_mont_check(Fd<C>* out, const Fd<C>* in, u64 n, unsigned* err) {
  for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n;
       i += (u64)gridDim.x * blockDim.x) {
    Fd<C> v = in[i];
    if (!fd_is_canonical(v)) atomicOr(err, 1u);
    out[i] = fd_to_mont(v);
  }
}

// canonicality check alone, for values that stay in canonical form (the MSM
// scalars): read-only over in[0, n)
template <class C>
__global__ void __launch_bounds__(256) k_canonical_check(const Fd<C>* in, u64 n, unsigned* err) {
  for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n;
       i += (u64)gridDim.x * blockDim.x)
    if (!fd_is_canonical(in[i])) atomicOr(err, 1u);
}

template <class C>
__global__ void __launch_bounds__(256) k_from_mont(Fd<C>* out, const Fd<C>* in, u64 n) {
  for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n;
       i += (u64)gridDim.x * blockDim.x)
    out[i] = fd_from_mont(in[i]);
}

// canonical affine x||y pairs -> Mont affine (identity = all-zero pair)
__global__ void __launch_bounds__(256) k_aff_to_mont_check(VestaAff* out, const VestaAff* in, u64 n,
                                    unsigned* err) {
  for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n;
       i += (u64)gridDim.x * blockDim.x) {
    VestaAff p = in[i];
    if (fd_is_zero(p.x) && fd_is_zero(p.y)) {
      out[i] = p;  // identity stays (0,0)
      continue;
    }
    bool bad = !fd_is_canonical(p.x) || !fd_is_canonical(p.y);
    VestaAff m;
    m.x = fd_to_mont(p.x);
    m.y = fd_to_mont(p.y);
    // on-curve check: y^2 == x^3 + 5
    Fq five{{5, 0, 0, 0}};
    Fq rhs = fd_add(fd_mul(fd_sqr(m.x), m.x), fd_to_mont(five));
    if (!fd_eq(fd_sqr(m.y), rhs)) bad = true;
    if (bad) atomicOr(err, 1u);
    out[i] = m;
  }
}

// decompress 32-byte compressed points -> Mont affine
__global__ void __launch_bounds__(256) k_decompress(VestaAff* out, const uint8_t* in, u64 n, unsigned* err) {
  for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n;
       i += (u64)gridDim.x * blockDim.x) {
    const uint8_t* b = in + 32 * i;
    u64 l[4];
    memcpy(l, b, 32);
    unsigned sign = (unsigned)(l[3] >> 63);
    l[3] &= 0x7FFFFFFFFFFFFFFFULL;
    if ((l[0] | l[1] | l[2] | l[3]) == 0) {
      if (sign) { atomicOr(err, 1u); }
      out[i].x = fd_zero<FqCfg>();
      out[i].y = fd_zero<FqCfg>();
      continue;
    }
    Fq x{{l[0], l[1], l[2], l[3]}};
    bool bad = !fd_is_canonical(x);
    Fq xm = fd_to_mont(x);
    Fq five{{5, 0, 0, 0}};
    Fq rhs = fd_add(fd_mul(fd_sqr(xm), xm), fd_to_mont(five));
    Fq y;
    if (!bad && !fd_sqrt(y, rhs)) bad = true;
    if (bad) {
      atomicOr(err, 1u);
      out[i].x = fd_zero<FqCfg>();
      out[i].y = fd_zero<FqCfg>();
      continue;
    }
    if (fd_is_odd_std(y) != (bool)sign) y = fd_neg(y);
    out[i].x = xm;
    out[i].y = y;
  }
}

// ---------- profiling ----------

struct ProfCounter {
  std::vector<hipEvent_t> starts, stops;
  double done_ms = 0;
  long done_n = 0;
};

static const char* const PROF_NAMES[] = {
    "msm_digits", "msm_scan",  "msm_scatter", "msm_bucket_acc", "msm_reduce",
    "msm_wsum",   "ntt_stage", "ntt_fused",   "ntt_bitrev",     "ntt_scale",
    "msm_total",  "ntt_total", "gp_terms",    "gp_inverse",     "gp_scan",
    "lk_compress", "lk_sort",  "lk_permute"};
constexpr int PROF_N = sizeof(PROF_NAMES) / sizeof(PROF_NAMES[0]);

struct PPk;

struct Ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;

  // SRS
  int k = -1;
  VestaAff* d_g = nullptr;
  VestaAff* d_gl = nullptr;
  // fixed-base tables of d_g and d_gl (msm_fb_build): MSM_FB_NWIN arrays of
  // 2^k points each, [2^(MSM_FB_C*w)] G_j. Null when k > MSM_FB_KMAX (those
  // sets stay on the generic plan, msm_plan_for).
  VestaAff* d_g_tab = nullptr;
  VestaAff* d_gl_tab = nullptr;
  VestaAff h_w, h_u;  // Mont form, host copies

  // custom bases / staged inputs. cap_* is what a buffer can hold; n_bases,
  // n_scalars and poly_k say what valid caller input it holds now (0 / -1:
  // none). They are cleared before a buffer is freed or overwritten and set
  // again only when the new content is complete and accepted.
  VestaAff* d_bases = nullptr;
  u64 cap_bases = 0;
  u64 n_bases = 0;
  bool bases_distinct = false;  // gen_bases output: distinct, non-identity
  // shared with the prover (gpu_msm_reserve), which overwrites it
  ScalarRepr* d_scalars = nullptr;
  u64 cap_scalars = 0;
  u64 n_scalars = 0;
  Fp* d_poly = nullptr;
  Fp* d_poly_tmp = nullptr;
  u64 cap_poly = 0;  // elements in each of d_poly, d_poly_tmp
  int poly_k = -1;

  MsmWork msm;
  NttPlan ntt;
  struct PPk* ppk = nullptr;            // active proving key (prover_gpu.inc)
  std::vector<struct PPk*> ppk_slots;   // PK cache: one entry
                                        // per tg_keygen call; slot id = index

  bool prof = false;
  bool pos_ready = false;  // poseidon constants uploaded to __constant__
  ProfCounter prof_c[PROF_N];
};

// the launch plan of nn-point MSMs over a device base array of this context:
// the fixed-base plan when it is an SRS set whose table is built, else the
// generic one. SRS bases and gen_bases output are distinct non-identity
// points and take the branch-free accumulation; uploaded bases may hold
// identities and duplicates and take the safe one.
static MsmPlan msm_plan_for(const Ctx* c, const VestaAff* bases, long nn) {
  const VestaAff* tab = bases == c->d_g ? c->d_g_tab : (bases == c->d_gl ? c->d_gl_tab : nullptr);
  if (tab) return msm_plan_fixed(tab, 1ULL << c->k);
  return msm_plan_generic(nn, bases, bases == c->d_bases && !c->bases_distinct);
}

static thread_local std::string g_err;

static int set_err(Ctx* c, const char* where, hipError_t e) {
  std::string msg = std::string(where) + ": " + hipGetErrorString(e);
  if (c)
    c->err = msg;
  else
    g_err = msg;
  return TG_ERR_HIP;
}

// bind the calling thread to this ctx's device: HIP device selection is
// per-thread, and callers may invoke entries from worker threads (one
// process per GPU with thread pools — the 8-GPU bench path)
static int tg_enter(Ctx* c) {
  hipError_t e = hipSetDevice(c->device);
  if (e != hipSuccess) return set_err(c, "hipSetDevice", e);
  return 0;
}

// idx < 0: a scope that records nothing (a launcher stage the caller does
// not profile)
struct ProfScope {
  Ctx* c;
  int idx;
  bool on;
  ProfScope(Ctx* c_, int idx_) : c(c_), idx(idx_), on(c_->prof && idx_ >= 0) {
    if (on) {
      hipEvent_t ev;
      hipEventCreate(&ev);
      hipEventRecord(ev, c->stream);
      c->prof_c[idx].starts.push_back(ev);
    }
  }
  ~ProfScope() {
    if (on) {
      hipEvent_t ev;
      hipEventCreate(&ev);
      hipEventRecord(ev, c->stream);
      c->prof_c[idx].stops.push_back(ev);
    }
  }
};

enum {
  P_MSM_DIGITS = 0, P_MSM_SCAN, P_MSM_SCATTER, P_MSM_ACC, P_MSM_REDUCE,
  P_MSM_WSUM, P_NTT_STAGE, P_NTT_FUSED, P_NTT_BITREV, P_NTT_SCALE,
  P_MSM_TOTAL, P_NTT_TOTAL, P_GP_TERMS, P_GP_INVERSE, P_GP_SCAN,
  P_LK_COMPRESS, P_LK_SORT, P_LK_PERMUTE,
};
static_assert(P_LK_PERMUTE + 1 == PROF_N, "PROF_NAMES and the P_* indices disagree");

}  // namespace taiga

#include "prover_gpu.inc"

using namespace taiga;

// ---------- host helpers shared by the entry points ----------

// temporary device memory, freed on every way out of the scope
template <class T>
struct DevTmp {
  T* p = nullptr;
  DevTmp() = default;
  DevTmp(const DevTmp&) = delete;
  DevTmp& operator=(const DevTmp&) = delete;
  ~DevTmp() {
    if (p) hipFree(p);
  }
  hipError_t alloc(size_t count) { return hipMalloc(&p, count * sizeof(T)); }
};

// make a resident input buffer hold at least n elements (the entry points
// leave no work pending on the stream, so the old buffer can go at once). The
// caller has already cleared the count of valid elements; after a failed
// allocation buf is null and cap is 0.
template <class T>
static hipError_t dev_reserve(T*& buf, u64& cap, u64 n) {
  if (buf && cap >= n) return hipSuccess;
  if (buf) hipFree(buf);
  buf = nullptr;
  cap = 0;
  hipError_t e = hipMalloc(&buf, n * sizeof(T));
  if (e != hipSuccess) {
    buf = nullptr;
    return e;
  }
  cap = n;
  return hipSuccess;
}

// the 4-byte device flag the ingestion kernels OR their verdict into
static hipError_t err_flag_new(DevTmp<unsigned>& f, hipStream_t stream) {
  hipError_t e = f.alloc(1);
  return e != hipSuccess ? e : hipMemsetAsync(f.p, 0, 4, stream);
}

// enqueue its read-back (valid after the stream is synchronized)
static void err_flag_read(const DevTmp<unsigned>& f, unsigned* host, hipStream_t stream) {
  hipMemcpyAsync(host, f.p, 4, hipMemcpyDeviceToHost, stream);
}

static int emit_proof(const std::vector<uint8_t>& proof, uint8_t* out, size_t cap,
                      size_t* out_len) {
  if (proof.size() > cap) return TG_ERR_BADARG;
  memcpy(out, proof.data(), proof.size());
  *out_len = proof.size();
  return TG_OK;
}

// batch-verification weights: rho_0 = 1, rho_i = DRBG(Blake2b(parts...))
// field draws. The caller chooses what the batch hash covers, in order.
static std::vector<Fp> batch_rho(
    size_t m, std::initializer_list<std::pair<const void*, size_t>> parts) {
  std::vector<Fp> rho(m);
  rho[0] = fd_one_mont<FpCfg>();
  if (m > 1) {
    Blake2b h(32, (const uint8_t*)"TaigaGPU-BatchVf");
    for (const auto& part : parts) h.update((const uint8_t*)part.first, part.second);
    uint8_t seed[32];
    h.final(seed);
    Drbg rng(seed);
    for (size_t i = 1; i < m; i++) rho[i] = rng.field<FpCfg>();
  }
  return rho;
}

/* expand the 192-byte borsh CompliancePublicInputs block into the real
 * 9 instance rows [nf, anchor, cm, delta_x, delta_y, rlcm halves]
 * (compliance.rs to_instance order; closes the round-1 placeholder
 * mapping flagged in ADVICE.md item 3) */
static bool compliance_rows_expand(const uint8_t* inst192, uint8_t rows[288]) {
  memcpy(rows, inst192 + 32, 32);       // nf
  memcpy(rows + 32, inst192, 32);       // anchor
  memcpy(rows + 64, inst192 + 64, 32);  // cm
  bool all0 = true;
  for (int b = 0; b < 32; b++)
    if (inst192[96 + b]) all0 = false;
  if (all0) {
    memset(rows + 96, 0, 64);
  } else {
    PallasJac d;
    if (!pallas_decompress(d, inst192 + 96)) return false;
    PallasAff a = jac_to_aff(d);
    Fp x = fd_from_mont(a.x), y = fd_from_mont(a.y);
    memcpy(rows + 96, x.l, 32);
    memcpy(rows + 128, y.l, 32);
  }
  for (int half = 0; half < 2; half++) {
    memset(rows + 160 + 64 * half, 0, 64);
    memcpy(rows + 160 + 64 * half, inst192 + 128 + 32 * half, 16);
    memcpy(rows + 192 + 64 * half + 0, inst192 + 128 + 32 * half + 16, 16);
  }
  return true;
}

// a key's verifying-key bytes as embedded in the wire formats: compressed
// fixed commitments, then compressed sigma commitments
static std::vector<uint8_t> pk_vk_bytes(const PPk* k) {
  std::vector<uint8_t> out;
  uint8_t b[32];
  for (const auto* commits : {&k->fixed_commits, &k->sigma_commits})
    for (const VestaAff& p : *commits) {
      Transcript::compress(b, p);
      out.insert(out.end(), b, b + 32);
    }
  return out;
}

// common tail of tg_compliance_prove / tg_rl_prove: run the attached
// witness program on the parsed inputs, read the circuit-computed instance
// rows into inst_rows (caller pre-fills the rows the circuit does not
// compute), prove, emit the proof and the canonical instance rows
static int witness_prove(Ctx* c, const std::vector<Fp>& inputs, std::vector<Fp>& inst_rows,
                         const uint8_t rng_seed[32], uint8_t* proof_out, size_t cap,
                         size_t* out_len, uint8_t* instance_out) {
  PDesc& d = c->ppk->d;
  std::vector<std::vector<Fp>> advice_lag;
  if (!c->ppk->tgw.run_mont(inputs, d.n_advice, advice_lag)) return TG_ERR_BADARG;
  c->ppk->tgw.read_instance_mont(advice_lag, inst_rows);
  std::vector<Fp> inst_lag(d.n, fd_zero<FpCfg>());
  std::copy(inst_rows.begin(), inst_rows.end(), inst_lag.begin());
  std::vector<uint8_t> proof;
  int rc = pprove_core(c, *c->ppk, inst_lag, advice_lag, rng_seed, proof);
  if (rc != 0) return rc;
  if ((rc = emit_proof(proof, proof_out, cap, out_len)) != TG_OK) return rc;
  if (instance_out)
    for (size_t r = 0; r < inst_rows.size(); r++) {
      Fp v = fd_from_mont(inst_rows[r]);
      memcpy(instance_out + 32 * r, v.l, 32);
    }
  return TG_OK;
}

extern "C" {

int tg_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char* tg_error_string(const tg_ctx* ctx) {
  const Ctx* c = (const Ctx*)ctx;
  return c ? c->err.c_str() : g_err.c_str();
}

int tg_init(int device, tg_ctx** out) {
  if (!out) return TG_ERR_BADARG;
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return set_err(nullptr, "hipSetDevice", e);
  Ctx* c = new Ctx();
  c->device = device;
  if ((e = hipStreamCreate(&c->stream)) != hipSuccess) {
    delete c;
    return set_err(nullptr, "hipStreamCreate", e);
  }
  *out = (tg_ctx*)c;
  return TG_OK;
}

void tg_destroy(tg_ctx* ctx) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return;
  hipStreamSynchronize(c->stream);
  for (PPk* pk : c->ppk_slots) {
    pdev_free(pk->pd);
    for (Fp* p : pk->d_fixed_coeff) hipFree(p);
    for (Fp* p : pk->d_sigma_coeff) hipFree(p);
    delete pk;
  }
  c->ppk_slots.clear();
  c->ppk = nullptr;
#define TGF(p) \
  if (p) hipFree(p)
  TGF(c->d_g); TGF(c->d_gl); TGF(c->d_g_tab); TGF(c->d_gl_tab);
  TGF(c->d_bases); TGF(c->d_scalars);
  TGF(c->d_poly); TGF(c->d_poly_tmp);
  TGF(c->msm.d_dig); TGF(c->msm.d_hist); TGF(c->msm.d_off); TGF(c->msm.d_end);
  TGF(c->msm.d_bsum); TGF(c->msm.d_sorted); TGF(c->msm.d_buckets);
  TGF(c->msm.d_partials); TGF(c->msm.d_wsums);
  TGF(c->ntt.d_tw_fwd); TGF(c->ntt.d_tw_inv);
#undef TGF
  hipStreamDestroy(c->stream);
  delete c;
}

int tg_synchronize(tg_ctx* ctx) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  hipError_t e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return set_err(c, "sync", e);
  return TG_OK;
}

void tg_prof_enable(tg_ctx* ctx, int on) { ((Ctx*)ctx)->prof = on != 0; }

void tg_prof_reset(tg_ctx* ctx) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return;
  for (auto& pc : c->prof_c) {
    for (auto ev : pc.starts) hipEventDestroy(ev);
    for (auto ev : pc.stops) hipEventDestroy(ev);
    pc.starts.clear();
    pc.stops.clear();
    pc.done_ms = 0;
    pc.done_n = 0;
  }
}

int tg_prof_get(tg_ctx* ctx, const char* name, double* total_ms, long* count) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  hipStreamSynchronize(c->stream);
  for (int i = 0; i < PROF_N; i++) {
    if (strcmp(PROF_NAMES[i], name) != 0) continue;
    ProfCounter& pc = c->prof_c[i];
    for (size_t j = 0; j < pc.stops.size(); j++) {
      float ms = 0;
      hipEventElapsedTime(&ms, pc.starts[j], pc.stops[j]);
      pc.done_ms += ms;
      pc.done_n++;
      hipEventDestroy(pc.starts[j]);
      hipEventDestroy(pc.stops[j]);
    }
    pc.starts.clear();
    pc.stops.clear();
    *total_ms = pc.done_ms;
    *count = pc.done_n;
    return TG_OK;
  }
  return TG_ERR_BADARG;
}

// ---------- SRS ----------

// true when a set of compressed points holds the identity (all-zero x) or two
// points with the same x (a repeat, or a point and its negation). MSMs over
// the SRS sets run the branch-free accumulation (jac_add_aff_fast), whose
// precondition is exactly that neither occurs. One sort of the sign-masked
// encodings, once per load.
static bool srs_set_degenerate(const uint8_t* set, u64 cnt, bool check_dups) {
  std::vector<std::array<uint8_t, 32>> enc(cnt);
  const std::array<uint8_t, 32> zero{};
  for (u64 i = 0; i < cnt; i++) {
    memcpy(enc[i].data(), set + 32 * i, 32);
    enc[i][31] &= 0x7F;
    if (enc[i] == zero) return true;
  }
  if (!check_dups) return false;
  std::sort(enc.begin(), enc.end());
  return std::adjacent_find(enc.begin(), enc.end()) != enc.end();
}

// true when two of the cnt Montgomery-affine points share an x coordinate
// (one sort, once per load; Montgomery form is a bijection, so equal x is
// equal limbs)
static bool aff_x_repeats(const VestaAff* pts, u64 cnt) {
  std::vector<std::array<u64, 4>> xs(cnt);
  for (u64 i = 0; i < cnt; i++) memcpy(xs[i].data(), pts[i].x.l, 32);
  std::sort(xs.begin(), xs.end());
  return std::adjacent_find(xs.begin(), xs.end()) != xs.end();
}

static void srs_free(Ctx* c) {
  VestaAff** sets[4] = {&c->d_g, &c->d_gl, &c->d_g_tab, &c->d_gl_tab};
  for (VestaAff** p : sets)
    if (*p) { hipFree(*p); *p = nullptr; }
}

// the fixed-base tables of the two sets just decompressed. The branch-free
// accumulation needs what srs_set_degenerate checks for a set to hold over a
// whole table, since any two of its nwin * 2^k points can meet in a bucket
// (G_1 = [2^c] G_0 passes the per-set check and would put T[1][0] = T[0][1]
// into one bucket): a table with a repeated x is refused.
static int srs_build_tables(Ctx* c, u64 n) {
  hipError_t e;
  const u64 tn = (u64)MSM_FB_NWIN * n;
  if ((e = hipMalloc(&c->d_g_tab, tn * sizeof(VestaAff))) != hipSuccess)
    return set_err(c, "srs alloc g table", e);
  if ((e = hipMalloc(&c->d_gl_tab, tn * sizeof(VestaAff))) != hipSuccess)
    return set_err(c, "srs alloc gl table", e);
  DevTmp<VestaJac> d_tmp;
  if ((e = d_tmp.alloc(n)) != hipSuccess) return set_err(c, "srs alloc table tmp", e);
  msm_fb_build(c->d_g, c->d_g_tab, d_tmp.p, n, c->stream);
  msm_fb_build(c->d_gl, c->d_gl_tab, d_tmp.p, n, c->stream);
  std::vector<VestaAff> h_tab(tn);
  for (const VestaAff* tab : {c->d_g_tab, c->d_gl_tab}) {
    hipMemcpyAsync(h_tab.data(), tab, tn * sizeof(VestaAff), hipMemcpyDeviceToHost, c->stream);
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess)
      return set_err(c, "srs table build", e);
    if (aff_x_repeats(h_tab.data(), tn)) return TG_ERR_ENCODING;
  }
  return TG_OK;
}

int tg_load_srs(tg_ctx* ctx, const uint8_t* bytes, size_t len) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  if (len < 4) return TG_ERR_BADARG;
  uint32_t k;
  memcpy(&k, bytes, 4);
  if (k > 28) return TG_ERR_BADARG;
  u64 n = 1ULL << k;
  if (len != 4 + 2 * n * 32 + 64) return TG_ERR_BADARG;
  // from here on the old SRS is replaced: a rejected load leaves none
  c->k = -1;
  if (srs_set_degenerate(bytes + 4, n, true) ||
      srs_set_degenerate(bytes + 4 + 32 * n, n, true) ||
      srs_set_degenerate(bytes + 4 + 64 * n, 2, false))
    return TG_ERR_ENCODING;
  hipError_t e;
  srs_free(c);
  if ((e = hipMalloc(&c->d_g, n * sizeof(VestaAff))) != hipSuccess)
    return set_err(c, "srs alloc g", e);
  if ((e = hipMalloc(&c->d_gl, n * sizeof(VestaAff))) != hipSuccess)
    return set_err(c, "srs alloc gl", e);
  DevTmp<uint8_t> d_comp;
  DevTmp<VestaAff> d_wu;  // w and u, decompressed on device, copied to host
  DevTmp<unsigned> d_err;
  if ((e = d_comp.alloc(2 * n * 32 + 64)) != hipSuccess)
    return set_err(c, "srs alloc comp", e);
  if ((e = d_wu.alloc(2)) != hipSuccess) return set_err(c, "srs alloc wu", e);
  if ((e = err_flag_new(d_err, c->stream)) != hipSuccess)
    return set_err(c, "srs alloc err", e);
  hipMemcpyAsync(d_comp.p, bytes + 4, 2 * n * 32 + 64, hipMemcpyHostToDevice, c->stream);
  hipLaunchKernelGGL(k_decompress, dim3(msm_grid(n)), dim3(256), 0, c->stream, c->d_g,
                     d_comp.p, n, d_err.p);
  hipLaunchKernelGGL(k_decompress, dim3(msm_grid(n)), dim3(256), 0, c->stream, c->d_gl,
                     d_comp.p + n * 32, n, d_err.p);
  hipLaunchKernelGGL(k_decompress, dim3(1), dim3(64), 0, c->stream, d_wu.p,
                     d_comp.p + 2 * n * 32, 2, d_err.p);
  unsigned h_err = 0;
  err_flag_read(d_err, &h_err, c->stream);
  VestaAff h_wu[2];
  hipMemcpyAsync(h_wu, d_wu.p, 2 * sizeof(VestaAff), hipMemcpyDeviceToHost, c->stream);
  e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return set_err(c, "srs decompress", e);
  if (h_err) return TG_ERR_ENCODING;
  if (k <= (uint32_t)MSM_FB_KMAX) {
    int rc = srs_build_tables(c, n);
    if (rc != TG_OK) {
      srs_free(c);  // a rejected load leaves no table (and no SRS) behind
      return rc;
    }
  }
  c->h_w = h_wu[0];
  c->h_u = h_wu[1];
  c->k = (int)k;
  return TG_OK;
}

int tg_srs_k(const tg_ctx* ctx) {
  const Ctx* c = (const Ctx*)ctx;
  return c->k >= 0 ? c->k : TG_ERR_NOSRS;
}

// ---------- MSM ----------

int tg_bases_upload(tg_ctx* ctx, const uint8_t* points_xy, size_t n) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  if (!n) return TG_ERR_BADARG;
  // from here on the old base set is replaced: a rejected upload leaves none
  c->n_bases = 0;
  c->bases_distinct = false;
  hipError_t e;
  if ((e = dev_reserve(c->d_bases, c->cap_bases, n)) != hipSuccess)
    return set_err(c, "bases alloc", e);
  DevTmp<VestaAff> d_raw;
  DevTmp<unsigned> d_err;
  if ((e = d_raw.alloc(n)) != hipSuccess) return set_err(c, "bases raw alloc", e);
  if ((e = err_flag_new(d_err, c->stream)) != hipSuccess)
    return set_err(c, "bases err alloc", e);
  hipMemcpyAsync(d_raw.p, points_xy, n * 64, hipMemcpyHostToDevice, c->stream);
  hipLaunchKernelGGL(k_aff_to_mont_check, dim3(msm_grid(n)), dim3(256), 0, c->stream,
                     c->d_bases, d_raw.p, n, d_err.p);
  unsigned h_err = 0;
  err_flag_read(d_err, &h_err, c->stream);
  e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return set_err(c, "bases upload", e);
  if (h_err) return TG_ERR_ENCODING;
  c->n_bases = n;
  return TG_OK;
}

int tg_gen_bases(tg_ctx* ctx, size_t n, uint64_t seed) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  if (!n) return TG_ERR_BADARG;
  c->n_bases = 0;  // as in tg_bases_upload
  c->bases_distinct = false;
  hipError_t e;
  if ((e = dev_reserve(c->d_bases, c->cap_bases, n)) != hipSuccess)
    return set_err(c, "bases alloc", e);
  hipLaunchKernelGGL(k_gen_bases, dim3(msm_grid(n)), dim3(256), 0, c->stream, c->d_bases,
                     n, seed);
  e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return set_err(c, "gen bases", e);
  c->n_bases = n;
  c->bases_distinct = true;
  return TG_OK;
}

int tg_bases_download(tg_ctx* ctx, size_t n, uint8_t* out_xy) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  if (!n || !c->d_bases || c->n_bases < n) return TG_ERR_BADARG;
  hipError_t e;
  DevTmp<Fq> tmp;
  if ((e = tmp.alloc(2 * n)) != hipSuccess) return set_err(c, "bases dl alloc", e);
  hipLaunchKernelGGL(k_from_mont<FqCfg>, dim3(ntt_grid(2 * n)), dim3(256), 0, c->stream,
                     tmp.p, (const Fq*)c->d_bases, (u64)(2 * n));
  hipMemcpyAsync(out_xy, tmp.p, n * 64, hipMemcpyDeviceToHost, c->stream);
  e = hipStreamSynchronize(c->stream);
  return e == hipSuccess ? TG_OK : set_err(c, "bases dl", e);
}

int tg_scalars_upload(tg_ctx* ctx, const uint8_t* scalars, size_t n) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  if (!n) return TG_ERR_BADARG;
  // from here on the old scalars are replaced: a rejected upload leaves none
  c->n_scalars = 0;
  hipError_t e;
  if ((e = dev_reserve(c->d_scalars, c->cap_scalars, n)) != hipSuccess)
    return set_err(c, "scalars alloc", e);
  DevTmp<unsigned> d_err;
  if ((e = err_flag_new(d_err, c->stream)) != hipSuccess)
    return set_err(c, "scalars err alloc", e);
  hipMemcpyAsync(c->d_scalars, scalars, n * 32, hipMemcpyHostToDevice, c->stream);
  // k_digits recodes 255 bits: a scalar >= p is refused here, once, so that
  // tg_msm_resident need not look at the values again
  hipLaunchKernelGGL(k_canonical_check<FpCfg>, dim3(msm_grid(n)), dim3(256), 0, c->stream,
                     (const Fp*)c->d_scalars, (u64)n, d_err.p);
  unsigned h_err = 0;
  err_flag_read(d_err, &h_err, c->stream);
  e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return set_err(c, "scalars upload", e);
  if (h_err) return TG_ERR_ENCODING;
  c->n_scalars = n;
  return TG_OK;
}

// argument and base-set checks of an MSM of n points over base_set, before
// any allocation or launch; on TG_OK *plan is the launch plan for that set
static int msm_guard(const Ctx* c, size_t n, int base_set, MsmPlan* plan) {
  if (base_set < 0 || base_set > 2 || !n) return TG_ERR_BADARG;
  if (base_set == 0) {
    if (!c->d_bases || c->n_bases < n) return TG_ERR_STATE;
  } else {
    if (c->k < 0) return TG_ERR_NOSRS;
    if (n > (1ULL << c->k)) return TG_ERR_BADARG;
  }
  const VestaAff* sets[3] = {c->d_bases, c->d_g, c->d_gl};
  *plan = msm_plan_for(c, sets[base_set], (long)n);
  return TG_OK;
}

// the MSM of the first n resident scalars (the caller has checked them) by plan
static int msm_common(Ctx* c, size_t n, const MsmPlan& plan, uint8_t out_xy[64]) {
  hipError_t e;
  if ((e = msm_work_alloc(c->msm, n)) != hipSuccess) return set_err(c, "msm ws", e);
  VestaJac sums[32]; /* sets() <= nwin <= 32 (c >= 8) */
  // all six stages + total; the accumulation scope covers the length sort
  static const int MSM_PROF_MAP[8] = {P_MSM_DIGITS, P_MSM_SCAN,   P_MSM_SCATTER,
                                      P_MSM_ACC,    P_MSM_REDUCE, P_MSM_WSUM,
                                      -1,           P_MSM_TOTAL};
  auto prof = [&](int idx) { return ProfScope(c, MSM_PROF_MAP[idx]); };
  msm_run(c->msm, c->d_scalars, n, n, 1, plan, c->stream, sums, prof);
  hipError_t es = hipStreamSynchronize(c->stream);
  if (es != hipSuccess) return set_err(c, "msm run", es);
  VestaAff r = jac_to_aff(msm_finish(plan, sums));
  if (aff_is_identity(r)) {
    memset(out_xy, 0, 64);
  } else {
    Fq x = fd_from_mont(r.x), y = fd_from_mont(r.y);
    memcpy(out_xy, x.l, 32);
    memcpy(out_xy + 32, y.l, 32);
  }
  return TG_OK;
}

int tg_msm_resident(tg_ctx* ctx, size_t n, int base_set, uint8_t out_xy[64]) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  MsmPlan plan;
  int rc = msm_guard(c, n, base_set, &plan);
  if (rc != TG_OK) return rc;
  if (!c->d_scalars || c->n_scalars < n) return TG_ERR_STATE;
  return msm_common(c, n, plan, out_xy);
}

int tg_msm_pallas(tg_ctx* ctx, const uint8_t* scalars, size_t n, int base_set,
                  uint8_t out_xy[64]) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  MsmPlan plan;
  int rc = msm_guard(c, n, base_set, &plan);
  if (rc != TG_OK) return rc;
  if ((rc = tg_scalars_upload(ctx, scalars, n)) != TG_OK) return rc;
  return msm_common(c, n, plan, out_xy);
}

// ---------- NTT ----------

int tg_poly_upload(tg_ctx* ctx, const uint8_t* poly, uint32_t k) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  u64 n;
  int rc = ntt_size_guard(k, c->poly_k, false, &n);
  if (rc != TG_OK) return rc;
  // from here on the old polynomial is replaced: a rejected upload leaves none
  c->poly_k = -1;
  hipError_t e;
  if (c->cap_poly != n) {  // both buffers are exactly 2^k long
    if (c->d_poly) { hipFree(c->d_poly); c->d_poly = nullptr; }
    if (c->d_poly_tmp) { hipFree(c->d_poly_tmp); c->d_poly_tmp = nullptr; }
    c->cap_poly = 0;
    if ((e = hipMalloc(&c->d_poly, n * sizeof(Fp))) != hipSuccess) {
      c->d_poly = nullptr;
      return set_err(c, "poly alloc", e);
    }
    if ((e = hipMalloc(&c->d_poly_tmp, n * sizeof(Fp))) != hipSuccess) {
      c->d_poly_tmp = nullptr;
      return set_err(c, "poly tmp alloc", e);
    }
    c->cap_poly = n;
  }
  DevTmp<unsigned> d_err;
  if ((e = err_flag_new(d_err, c->stream)) != hipSuccess)
    return set_err(c, "poly err alloc", e);
  // upload canonical into tmp, convert to Mont into d_poly
  hipMemcpyAsync(c->d_poly_tmp, poly, n * 32, hipMemcpyHostToDevice, c->stream);
  hipLaunchKernelGGL(k_to_mont_check<FpCfg>, dim3(ntt_grid(n)), dim3(256), 0, c->stream,
                     c->d_poly, c->d_poly_tmp, n, d_err.p);
  unsigned h_err = 0;
  err_flag_read(d_err, &h_err, c->stream);
  e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return set_err(c, "poly upload", e);
  if (h_err) return TG_ERR_ENCODING;
  c->poly_k = (int)k;
  return TG_OK;
}

int tg_ntt_resident(tg_ctx* ctx, int dir, uint32_t k, int coset) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  u64 n;
  int rc = ntt_size_guard(k, c->poly_k, true, &n);
  // bad arguments are reported before missing state
  if (rc == TG_ERR_BADARG) return rc;
  if (coset) return TG_ERR_BADARG;  // arrives with the prover pipeline
  if (rc != TG_OK) return rc;
  hipError_t e;
  if ((e = ntt_plan_init(c->ntt, (int)k, c->stream)) != hipSuccess)
    return set_err(c, "ntt plan", e);
  Fp ninv;
  if (dir) {
    // n^{-1} in Mont form, computed host-side with the shared primitives
    Fp nstd{{n, 0, 0, 0}};
    ninv = fd_inv(fd_to_mont(nstd));
  }
  {
    ProfScope total(c, P_NTT_TOTAL);
    static const int NTT_PROF_MAP[4] = {P_NTT_BITREV, P_NTT_FUSED, P_NTT_STAGE,
                                        P_NTT_SCALE};
    auto prof = [&](int idx) { return ProfScope(c, NTT_PROF_MAP[idx]); };
    if ((e = ntt_run(c->d_poly, c->d_poly_tmp, c->ntt, (int)k, dir != 0, c->stream,
                     dir ? &ninv : nullptr, prof)) != hipSuccess)
      return set_err(c, "ntt run", e);
  }
  e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return set_err(c, "ntt sync", e);
  return TG_OK;
}

int tg_poly_download(tg_ctx* ctx, uint8_t* poly, uint32_t k) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  u64 n;
  int rc = ntt_size_guard(k, c->poly_k, true, &n);
  if (rc != TG_OK) return rc;
  // from_mont into tmp, then D2H
  hipLaunchKernelGGL(k_from_mont<FpCfg>, dim3(ntt_grid(n)), dim3(256), 0, c->stream,
                     c->d_poly_tmp, c->d_poly, n);
  hipMemcpyAsync(poly, c->d_poly_tmp, n * 32, hipMemcpyDeviceToHost, c->stream);
  hipError_t e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return set_err(c, "poly download", e);
  return TG_OK;
}

int tg_ntt_fp(tg_ctx* ctx, int dir, uint32_t k, int coset, uint8_t* poly) {
  int rc = tg_poly_upload(ctx, poly, k);
  if (rc != TG_OK) return rc;
  rc = tg_ntt_resident(ctx, dir, k, coset);
  if (rc != TG_OK) return rc;
  return tg_poly_download(ctx, poly, k);
}

/* ---- prover ABI (implementation in prover_gpu.inc) ---- */

/* builds a proving key and caches it; returns the non-negative slot id
 * (also leaves it active for the slotless entry points). PKs are cached for
 * the ctx lifetime — the reference's generic-macro path re-keygens per
 * proof (resource_logic_circuit.rs:578-580); the cache is §8f-1's fix. */
int tg_keygen(tg_ctx* ctx, const uint8_t* desc, size_t desc_len) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  if (c->k < 0) return TG_ERR_NOSRS;
  PPk* pk = new PPk();
  int rc = ppk_keygen(c, *pk, desc, desc_len);
  if (rc != 0) {
    delete pk;
    return rc;
  }
  c->ppk_slots.push_back(pk);
  c->ppk = pk;
  return (int)c->ppk_slots.size() - 1;
}

/* select a previously built proving key by slot id */
int tg_select_key(tg_ctx* ctx, int slot) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  if (slot < 0 || (size_t)slot >= c->ppk_slots.size()) return TG_ERR_BADARG;
  c->ppk = c->ppk_slots[slot];
  return TG_OK;
}

int tg_key_gate_path(tg_ctx* ctx) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  if (!c->ppk || !c->ppk->ready) return TG_ERR_STATE;
  return c->ppk->rtc && c->ppk->rtc->ready ? 1 : 0;
}

int tg_create_proof(tg_ctx* ctx, const uint8_t inst_seed[32], const uint8_t wit_seed[32],
                    const uint8_t rng_seed[32], uint8_t* proof_out, size_t cap,
                    size_t* out_len) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  if (!c->ppk || !c->ppk->ready) return TG_ERR_STATE;
  std::vector<uint8_t> proof;
  int rc = pprove(c, *c->ppk, inst_seed, wit_seed, rng_seed, proof);
  if (rc != 0) return rc;
  return emit_proof(proof, proof_out, cap, out_len);
}

int tg_witness_hash(tg_ctx* ctx, const uint8_t inst_seed[32], const uint8_t wit_seed[32],
                    uint8_t out[32]) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  if (!c->ppk || !c->ppk->ready) return TG_ERR_STATE;
  PDesc& d = c->ppk->d;
  std::vector<Fp> inst;
  cs1_instance(d, inst_seed, inst);
  std::vector<std::vector<Fp>> adv;
  cs1_witness(d, wit_seed, inst, adv);
  Blake2b h(32);
  std::vector<uint8_t> buf(32 * (size_t)d.n);
  for (int col = 0; col < d.n_advice; col++) {
#ifdef _OPENMP
#pragma omp parallel for schedule(static)
#endif
    for (long i = 0; i < d.n; i++) {
      Fp v = fd_from_mont(adv[col][i]);
      memcpy(buf.data() + 32 * i, v.l, 32);
    }
    h.update(buf.data(), buf.size());
  }
  h.final(out);
  return TG_OK;
}

int tg_verify_proof(tg_ctx* ctx, const uint8_t inst_seed[32], const uint8_t* proof,
                    size_t proof_len) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  if (!c->ppk || !c->ppk->ready) return TG_ERR_STATE;
  return pverify(c, *c->ppk, inst_seed, proof, proof_len);
}

/* raw-instance verification: instance = n_instance_rows x 32B canonical
 * reprs (the drop-in shape of plonk::verify_proof's instance slices —
 * proof.rs:45-54). */
int tg_verify_proof_raw(tg_ctx* ctx, const uint8_t* instance, const uint8_t* proof,
                        size_t proof_len) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  if (!c->ppk || !c->ppk->ready) return TG_ERR_STATE;
  if (!instance) return TG_ERR_BADARG;
  return pverify_raw(c, *c->ppk, instance, proof, proof_len);
}

/* batch verification (the halo2 BatchVerifier / Guard
 * accumulation pattern behind proof.rs:45-54): each proof contributes a
 * final-check guard; guards are combined with random weights so that all
 * m IPA final checks collapse into ONE g-sized GPU MSM plus a few hundred
 * variable points. Weights are derived by hashing the whole batch (a
 * prover cannot predict them). All proofs must be for the active key.
 * Returns TG_OK iff every proof is valid; -1 if the combined check fails;
 * -1xx on the first structurally malformed proof. */
int tg_verify_batch(tg_ctx* ctx, size_t m, const uint8_t* inst_seeds,
                    const uint8_t* proofs, const size_t* proof_lens) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  if (!c->ppk || !c->ppk->ready) return TG_ERR_STATE;
  if (m == 0 || m > 4096 || !inst_seeds || !proofs || !proof_lens) return TG_ERR_BADARG;
  std::vector<PVGuard> gds(m);
  size_t off = 0;
  for (size_t i = 0; i < m; i++) {
    std::vector<Fp> inst_lag;
    cs1_instance(c->ppk->d, inst_seeds + 32 * i, inst_lag);
    int rc = pverify_guard(c, *c->ppk, inst_lag, proofs + off,
                           proof_lens[i], gds[i]);
    if (rc != 0) return rc;
    off += proof_lens[i];
  }
  /* weights over Blake2b(m ‖ seeds ‖ proofs) */
  uint64_t mle = (uint64_t)m;
  std::vector<Fp> rho = batch_rho(m, {{&mle, 8}, {inst_seeds, 32 * m}, {proofs, off}});
  return pverify_eval(c, *c->ppk, gds.data(), (int)m, rho.data());
}

/* raw-instance batch verification: the ptx-bundle shape (§8f-3 + §8f-4
 * composed): instances = concatenated n_instance_rows x 32B blocks, one
 * per proof, for the ACTIVE key. Same combined-check semantics as
 * tg_verify_batch. */
int tg_verify_batch_raw(tg_ctx* ctx, size_t m, const uint8_t* instances,
                        const uint8_t* proofs, const size_t* proof_lens) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  if (!c->ppk || !c->ppk->ready) return TG_ERR_STATE;
  if (m == 0 || m > 4096 || !instances || !proofs || !proof_lens) return TG_ERR_BADARG;
  size_t inst_stride = 32 * (size_t)c->ppk->d.n_instance_rows;
  std::vector<PVGuard> gds(m);
  size_t off = 0;
  for (size_t i = 0; i < m; i++) {
    std::vector<Fp> inst_lag;
    int rc = pinst_from_raw(c->ppk->d, instances + inst_stride * i, inst_lag);
    if (rc != 0) return rc;
    rc = pverify_guard(c, *c->ppk, inst_lag, proofs + off, proof_lens[i], gds[i]);
    if (rc != 0) return rc;
    off += proof_lens[i];
  }
  uint64_t mle = (uint64_t)m;
  std::vector<Fp> rho =
      batch_rho(m, {{&mle, 8}, {instances, inst_stride * m}, {proofs, off}});
  return pverify_eval(c, *c->ppk, gds.data(), (int)m, rho.data());
}

/* ---- binding signatures + transaction digest (host-side wire layer,
 * SURVEY §8f-4; binding_signature.rs / transaction.rs:116-158) ----
 * RedDSA over Pallas, H* = BLAKE2b-512("Taiga_RedPallasH"), ctx-free.
 * See binding_sig.hpp for the basepoint pin status. */
int tg_binding_vk(const uint8_t sk[32], uint8_t vk_out[32]) {
  return bs_derive_vk(vk_out, sk) ? TG_ERR_ENCODING : TG_OK;
}

int tg_delta_commit(const uint8_t r[32], uint8_t cv_out[32]) {
  Fq s;
  if (!bs_scalar_from_bytes(s, r)) return TG_ERR_ENCODING;
  pallas_compress(cv_out, pallas_mul(pallas_basepoint(), s));
  return TG_OK;
}

int tg_binding_sign(const uint8_t sk[32], const uint8_t* msg, size_t msg_len,
                    const uint8_t rng_seed[32], uint8_t sig_out[64]) {
  if (!msg && msg_len) return TG_ERR_BADARG;
  return bs_sign(sig_out, sk, msg, msg_len, rng_seed) ? TG_ERR_ENCODING : TG_OK;
}

int tg_binding_verify(const uint8_t vk[32], const uint8_t* msg, size_t msg_len,
                      const uint8_t sig[64]) {
  if (!msg && msg_len) return TG_ERR_BADARG;
  return bs_verify(vk, msg, msg_len, sig) ? -1 : TG_OK;
}

int tg_binding_vk_from_deltas(const uint8_t* deltas, size_t n, uint8_t vk_out[32]) {
  if (n && !deltas) return TG_ERR_BADARG;
  return bs_vk_from_deltas(vk_out, deltas, n) ? TG_ERR_ENCODING : TG_OK;
}

int tg_tx_digest(const uint8_t* nfs, size_t n_nf, const uint8_t* cms, size_t n_cm,
                 const uint8_t* deltas, size_t n_delta, const uint8_t* anchors,
                 size_t n_anchor, uint8_t out[32]) {
  bs_tx_digest(out, nfs, n_nf, cms, n_cm, deltas, n_delta, anchors, n_anchor);
  return TG_OK;
}

/* ---- transaction wire format (borsh layouts cited in
 * tx_wire.hpp) ---- */

/* ctx-free wire check: parse a borsh Transaction, recompute
 * Transaction::digest from the compliance instances, aggregate delta
 * commitments into the binding vk and verify the binding signature.
 * vk_len = byte length of one embedded resource-logic VerifyingKey
 * (32*(n_fixed+n_perm) for TGD1 circuits). Returns TG_OK; -1 on a bad
 * binding signature; -2xx on structural decode errors. */
int tg_tx_wire_check(const uint8_t* tx, size_t len, uint32_t vk_len,
                     uint32_t* n_sptx, uint32_t* n_proofs) {
  if (!tx) return TG_ERR_BADARG; /* short inputs fail structurally in the parser */
  return tx_check(tx, len, vk_len, n_sptx, n_proofs, nullptr);
}

/* full transaction verification against the ACTIVE key: wire check +
 * binding signature + ONE combined batch verification of every compliance
 * proof in the bundle. Round-1 instance mapping: the first
 * n_instance_rows fields of each 192-byte compliance instance block
 * (requires n_instance_rows <= 6). The REAL compliance circuit expands
 * the 6 borsh fields into 9 instance rows — [nf, anchor, cm, delta.x,
 * delta.y, rl_in x2 halves, rl_out x2 halves], constant.rs:54-62 — which
 * replaces this mapping in round 2. */
int tg_tx_verify(tg_ctx* ctx, const uint8_t* tx, size_t len) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  if (!c->ppk || !c->ppk->ready) return TG_ERR_STATE;
  PDesc& d = c->ppk->d;
  if (d.n_instance_rows > 6) return TG_ERR_BADARG;
  uint32_t vk_len = 32u * (uint32_t)(d.n_fixed + d.n_perm);
  TxDigestStreams st;
  int rc = tx_check(tx, len, vk_len, nullptr, nullptr, &st);
  if (rc) return rc;
  size_t m = st.proof_ptr.size();
  if (m == 0) return TG_OK;
  std::vector<PVGuard> gds(m);
  for (size_t i = 0; i < m; i++) {
    std::vector<Fp> inst_lag;
    rc = pinst_from_raw(d, st.inst_ptr[i], inst_lag);
    if (rc) return rc;
    rc = pverify_guard(c, *c->ppk, inst_lag, st.proof_ptr[i], st.proof_len[i], gds[i]);
    if (rc) return rc;
  }
  std::vector<Fp> rho = batch_rho(m, {{tx, len}});  // the tx alone, no count prefix
  return pverify_eval(c, *c->ppk, gds.data(), (int)m, rho.data());
}

/* one combined batch check of scattered proofs on the ACTIVE key (insts =
 * their raw instance blocks, concatenated); an empty group passes.
 * TG_ERR_BADARG passes through, any other failure is -1. */
static int verify_group(tg_ctx* ctx, const uint8_t* insts,
                        const std::vector<const uint8_t*>& proof_ptr,
                        const std::vector<size_t>& proof_len) {
  if (proof_ptr.empty()) return TG_OK;
  std::vector<uint8_t> proofs;
  for (size_t i = 0; i < proof_ptr.size(); i++)
    proofs.insert(proofs.end(), proof_ptr[i], proof_ptr[i] + proof_len[i]);
  int rc = tg_verify_batch_raw(ctx, proof_ptr.size(), insts, proofs.data(),
                               proof_len.data());
  return rc == TG_OK || rc == TG_ERR_BADARG ? rc : -1;
}

/* common tail of tg_tx_verify_full / tg_ptx_verify: batch-verify the RL
 * group (22-row instances) on slot_rl, then the compliance group (cinst =
 * expanded 9-row instances) on slot_compliance */
static int verify_rl_then_compliance(tg_ctx* ctx, int slot_rl, int slot_compliance,
                                     const std::vector<const uint8_t*>& rl_inst,
                                     const std::vector<const uint8_t*>& rl_proof,
                                     const std::vector<size_t>& rl_len,
                                     const std::vector<uint8_t>& cinst,
                                     const std::vector<const uint8_t*>& c_proof,
                                     const std::vector<size_t>& c_len) {
  int rc = tg_select_key(ctx, slot_rl);
  if (rc) return rc;
  std::vector<uint8_t> insts;
  for (const uint8_t* ip : rl_inst) insts.insert(insts.end(), ip, ip + 22 * 32);
  if ((rc = verify_group(ctx, insts.data(), rl_proof, rl_len))) return rc;
  if ((rc = tg_select_key(ctx, slot_compliance))) return rc;
  return verify_group(ctx, cinst.data(), c_proof, c_len);
}

/* FULL transaction verification (round 2; supersedes tg_tx_verify's
 * compliance-only check — ADVICE.md item 2): borsh Transaction parse +
 * Transaction::digest + binding signature (tx_check), then batch-verify
 * EVERY compliance proof (slot_compliance; 192-B instances expanded to
 * the real 9 rows) and EVERY resource-logic proof (slot_rl; vk bytes
 * must match the slot), plus the per-sptx execute() consistency checks.
 * TG_OK only when the whole transaction is valid. */
int tg_tx_verify_full(tg_ctx* ctx, int slot_compliance, int slot_rl,
                      const uint8_t* tx, size_t len) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  int rc = tg_select_key(ctx, slot_rl);
  if (rc) return rc;
  PPk* rlk = c->ppk;
  uint32_t vk_len = 32u * (uint32_t)(rlk->fixed_commits.size() +
                                     rlk->sigma_commits.size());
  TxDigestStreams st;
  rc = tx_check(tx, len, vk_len, nullptr, nullptr, &st);
  if (rc) return rc;
  // vk match + consistency checks per sptx
  const std::vector<uint8_t> vk_ref = pk_vk_bytes(rlk);
  for (const uint8_t* vkb : st.rl_vk_ptr)
    if (memcmp(vkb, vk_ref.data(), vk_len) != 0) return -207;
  st.sptx_comp_begin.push_back(st.n_compliance);
  st.sptx_rl_begin.push_back(st.n_rl);
  std::vector<uint8_t> cinst;
  for (uint32_t i = 0; i < st.n_compliance; i++) {
    uint8_t rows[288];
    if (!compliance_rows_expand(st.inst_ptr[i], rows)) return -204;
    cinst.insert(cinst.end(), rows, rows + 288);
  }
  for (uint32_t s2 = 0; s2 < st.n_sptx; s2++) {
    uint32_t c0 = st.sptx_comp_begin[s2], c1 = st.sptx_comp_begin[s2 + 1];
    uint32_t r0 = st.sptx_rl_begin[s2], r1 = st.sptx_rl_begin[s2 + 1];
    if (r1 == r0) continue;
    const uint8_t* root0 = st.rl_inst_ptr[r0];
    uint32_t in_seen = 0, out_seen = 0;
    for (uint32_t r = r0; r < r1; r++) {
      if (memcmp(st.rl_inst_ptr[r], root0, 32) != 0) return -301;
      const uint8_t* self_id = st.rl_inst_ptr[r] + 32;
      if (st.rl_is_input[r]) {
        uint32_t ci = c0 + in_seen++;
        if (ci >= c1 || memcmp(self_id, cinst.data() + 288ul * ci, 32) != 0)
          return -303;
      } else {
        uint32_t ci = c0 + out_seen++;
        if (ci >= c1 || memcmp(self_id, cinst.data() + 288ul * ci + 64, 32) != 0)
          return -304;
      }
    }
  }
  return verify_rl_then_compliance(ctx, slot_rl, slot_compliance, st.rl_inst_ptr,
                                   st.rl_proof_ptr, st.rl_proof_len, cinst, st.proof_ptr,
                                   st.proof_len);
}

/* batched Poseidon P128Pow5T3 ConstantLength<L> hashing (GPU witness
 * synthesis; replaces host-side halo2_gadgets poseidon
 * hashing — utils.rs:40-48): msgs = n x L x 32B canonical reprs,
 * out = n x 32B canonical digests. One hash per GPU thread. */
int tg_poseidon_hash(tg_ctx* ctx, const uint8_t* msgs, size_t n, int L,
                     uint8_t* out) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  if (!msgs || !out || n == 0 || L < 1 || L > 64) return TG_ERR_BADARG;
  hipError_t e;
  if (!c->pos_ready) {
    if ((e = pos_upload_consts()) != hipSuccess)
      return set_err(c, "poseidon consts", e);
    c->pos_ready = true;
  }
  DevTmp<Fp> d_in, d_out;
  DevTmp<unsigned> d_err;
  if (d_in.alloc(n * (size_t)L) != hipSuccess || d_out.alloc(n) != hipSuccess ||
      err_flag_new(d_err, c->stream) != hipSuccess)
    return TG_ERR_NOMEM;
  hipMemcpyAsync(d_in.p, msgs, n * (size_t)L * 32, hipMemcpyHostToDevice, c->stream);
  u64 grid = (n + 255) / 256;
  if (grid > 16384) grid = 16384;
  hipLaunchKernelGGL(k_poseidon_hash, dim3(grid), dim3(256), 0, c->stream,
                     d_out.p, d_in.p, (u64)n, L, d_err.p);
  unsigned h_err = 0;
  err_flag_read(d_err, &h_err, c->stream);
  std::vector<uint8_t> h_out(n * 32);
  hipMemcpyAsync(h_out.data(), d_out.p, n * 32, hipMemcpyDeviceToHost, c->stream);
  e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return set_err(c, "poseidon", e);
  if (h_err) return TG_ERR_ENCODING;
  memcpy(out, h_out.data(), n * 32);
  return TG_OK;
}

/* raw-witness proving (SURVEY §8b witness-blob shape): instance =
 * n_instance_rows x 32B canonical reprs; advice = n_advice x 2^k x 32B
 * canonical, column-major (rows beyond usable = n-(bf+1) are replaced by
 * blinding). */
/* attach a TGW1 witness-synthesis program (tools/circuit/emit.py) to the
 * ACTIVE key slot; required by tg_compliance_prove / tg_rl_prove */
int tg_witness_program_load(tg_ctx* ctx, const uint8_t* tgw, size_t len) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  if (!c->ppk || !c->ppk->ready) return TG_ERR_STATE;
  if (!c->ppk->tgw.parse(tgw, len)) return TG_ERR_BADARG;
  if ((int)c->ppk->tgw.k != c->ppk->d.k) return TG_ERR_BADARG;
  return TG_OK;
}

/* drop-in ComplianceInfo prove (replaces ComplianceInfo::build +
 * Proof::create — compliance.rs:190-233 + proof.rs:25-42): parses the
 * borsh ComplianceInfo, synthesizes the exact compliance circuit witness
 * via the attached program, reads the circuit-computed public inputs back
 * (nf, cm, delta, RL commitments; anchor from the blob), proves on the
 * GPU. instance_out = 9 x 32B rows (CompliancePublicInputs::to_instance
 * order). */
int tg_compliance_prove(tg_ctx* ctx, const uint8_t* info_borsh, size_t len,
                        const uint8_t rng_seed[32], uint8_t* proof_out,
                        size_t cap, size_t* out_len, uint8_t instance_out[288]) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  if (!c->ppk || !c->ppk->ready || !c->ppk->tgw.ready) return TG_ERR_STATE;
  PDesc& d = c->ppk->d;
  if (d.n_instance_rows != 9 || c->ppk->tgw.n_inputs != 124) return TG_ERR_STATE;
  std::vector<Fp> inputs;
  if (!compliance_inputs(info_borsh, len, inputs)) return TG_ERR_ENCODING;
  std::vector<Fp> inst_rows(9, fd_zero<FpCfg>());
  inst_rows[1] = inputs[1];  // anchor from the blob
  return witness_prove(c, inputs, inst_rows, rng_seed, proof_out, cap, out_len,
                       instance_out);
}

/* drop-in TrivialRL prove (resource_logic_examples.rs get_verifying_info):
 * witness = borsh ResourceExistenceWitness; pad_rseed drives the random
 * instance padding (rows 6..21). instance_out = 22 x 32B. */
int tg_rl_prove(tg_ctx* ctx, const uint8_t* witness_borsh, size_t len,
                const uint8_t pad_rseed[32], const uint8_t rng_seed[32],
                uint8_t* proof_out, size_t cap, size_t* out_len,
                uint8_t instance_out[704]) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  if (!c->ppk || !c->ppk->ready || !c->ppk->tgw.ready) return TG_ERR_STATE;
  PDesc& d = c->ppk->d;
  if (d.n_instance_rows != 22 || c->ppk->tgw.n_inputs != 41) return TG_ERR_STATE;
  std::vector<Fp> inputs;
  uint8_t pad[16 * 32];
  if (!rl_inputs(witness_borsh, len, pad_rseed, inputs, pad))
    return TG_ERR_ENCODING;
  std::vector<Fp> inst_rows(22, fd_zero<FpCfg>());
  for (int r = 0; r < 16; r++) {
    Fp v;
    memcpy(v.l, pad + 32 * r, 32);
    inst_rows[6 + r] = fd_to_mont(v);
  }
  return witness_prove(c, inputs, inst_rows, rng_seed, proof_out, cap, out_len,
                       instance_out);
}

/* synthesized-advice export for parity tests: runs the attached program on
 * a borsh witness (kind 0 = compliance, 1 = RL) and writes the advice
 * column bytes (n_advice x 2^k x 32). */
int tg_witness_synthesize(tg_ctx* ctx, int kind, const uint8_t* borsh, size_t len,
                          const uint8_t pad_rseed[32], uint8_t* advice_out,
                          uint8_t* instance_out) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  if (!c->ppk || !c->ppk->ready || !c->ppk->tgw.ready) return TG_ERR_STATE;
  PDesc& d = c->ppk->d;
  std::vector<Fp> inputs;
  size_t ninst = (size_t)d.n_instance_rows * 32;
  std::vector<uint8_t> inst(ninst, 0);
  if (kind == 0) {
    if (!compliance_inputs(borsh, len, inputs)) return TG_ERR_ENCODING;
    Fp a = fd_from_mont(inputs[1]);
    memcpy(inst.data() + 32, a.l, 32);
  } else {
    if (ninst < 22 * 32) return TG_ERR_STATE;
    if (!rl_inputs(borsh, len, pad_rseed, inputs, inst.data() + 6 * 32))
      return TG_ERR_ENCODING;
  }
  memset(advice_out, 0, 32ul * d.n_advice * d.n);
  if (!c->ppk->tgw.run(inputs, d.n_advice, advice_out)) return TG_ERR_BADARG;
  c->ppk->tgw.read_instance(d.n_advice, advice_out, inst.data());
  if (instance_out) memcpy(instance_out, inst.data(), ninst);
  return TG_OK;
}

/* ---- ShieldedPartialTransaction::build / verify (shielded_ptx.rs:98-137,
 * BASELINE configs[3]) ----
 * Builds one borsh ShieldedPartialTransaction: n_compliance compliance
 * proofs (borsh ComplianceInfo units, 1528 B each; key slot
 * slot_compliance) + per input/output resource one TrivialRL proof (borsh
 * ResourceExistenceWitness units, 334 B each; slot_rl), binding_sig_r =
 * sum of the units' rcv (Some), empty hints. Per-proof randomness is
 * drawn from ONE ChaCha20 stream over rng_seed in build order:
 * compliance proof seeds first, then per RL (pad_rseed, proof seed) —
 * the determinized stand-in for the reference's single &mut rng
 * (shielded_ptx.rs:105-125; DESIGN.md randomness ledger). */
int tg_ptx_build(tg_ctx* ctx, int slot_compliance, int slot_rl,
                 uint32_t n_compliance, const uint8_t* compliance_units,
                 uint32_t n_in, uint32_t n_out, const uint8_t* rl_units,
                 const uint8_t rng_seed[32], uint8_t* ptx_out, size_t cap,
                 size_t* out_len) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  if (n_compliance > 64 || n_in + n_out > 128) return TG_ERR_BADARG;
  Drbg stream(rng_seed);
  std::vector<uint8_t> out;
  auto put_u32 = [&](uint32_t v) {
    out.push_back((uint8_t)v);
    out.push_back((uint8_t)(v >> 8));
    out.push_back((uint8_t)(v >> 16));
    out.push_back((uint8_t)(v >> 24));
  };
  // compliances
  put_u32(n_compliance);
  Fq rcv_sum = fd_zero<FqCfg>();
  int rc = tg_select_key(ctx, slot_compliance);
  if (rc) return rc;
  for (uint32_t i = 0; i < n_compliance; i++) {
    const uint8_t* unit = compliance_units + 1528ul * i;
    uint8_t seed[32];
    stream.bytes(seed, 32);
    uint8_t proof[1 << 14];
    size_t plen = 0;
    uint8_t inst[288];
    rc = tg_compliance_prove(ctx, unit, 1528, seed, proof, sizeof(proof), &plen,
                             inst);
    if (rc) return rc;
    // rcv from the unit's rseed (last 32 bytes)
    rcv_sum = fd_add(rcv_sum, prf_expand<FqCfg>(unit + 1528 - 32, 3));
    put_u32((uint32_t)plen);
    out.insert(out.end(), proof, proof + plen);
    // CompliancePublicInputs borsh (compliance.rs:82-93):
    // anchor ‖ nf ‖ cm ‖ delta(compressed) ‖ rlcm_in ‖ rlcm_out
    out.insert(out.end(), inst + 32, inst + 64);   // anchor (row 1)
    out.insert(out.end(), inst, inst + 32);        // nf (row 0)
    out.insert(out.end(), inst + 64, inst + 96);   // cm (row 2)
    {  // delta rows 3,4 -> compressed pallas point
      Fp x, y;
      memcpy(x.l, inst + 96, 32);
      memcpy(y.l, inst + 128, 32);
      uint8_t comp[32];
      if (fd_is_zero(x) && fd_is_zero(y)) {
        memset(comp, 0, 32);
      } else {
        memcpy(comp, x.l, 32);
        comp[31] |= (uint8_t)((y.l[0] & 1) << 7);
      }
      out.insert(out.end(), comp, comp + 32);
    }
    for (int half = 0; half < 2; half++) {  // rlcm halves -> 32B commitment
      uint8_t cmb[32];
      memcpy(cmb, inst + (160 + 64 * half), 16);
      memcpy(cmb + 16, inst + (192 + 64 * half), 16);
      out.insert(out.end(), cmb, cmb + 32);
    }
  }
  // RL sets (inputs then outputs)
  rc = tg_select_key(ctx, slot_rl);
  if (rc) return rc;
  const std::vector<uint8_t> vk_bytes = pk_vk_bytes(c->ppk);
  for (int grp = 0; grp < 2; grp++) {
    uint32_t cnt = grp == 0 ? n_in : n_out;
    uint32_t base = grp == 0 ? 0 : n_in;
    put_u32(cnt);
    for (uint32_t i = 0; i < cnt; i++) {
      const uint8_t* unit = rl_units + 334ul * (base + i);
      uint8_t pad[32], seed[32];
      stream.bytes(pad, 32);
      stream.bytes(seed, 32);
      uint8_t proof[1 << 14];
      size_t plen = 0;
      uint8_t inst[704];
      rc = tg_rl_prove(ctx, unit, 334, pad, seed, proof, sizeof(proof), &plen,
                       inst);
      if (rc) return rc;
      out.insert(out.end(), vk_bytes.begin(), vk_bytes.end());
      put_u32((uint32_t)plen);
      out.insert(out.end(), proof, proof + plen);
      out.insert(out.end(), inst, inst + 704);
      put_u32(0);  // app_dynamic_resource_logic_verifying_info: empty vec
    }
  }
  out.push_back(1);  // Some(binding_sig_r)
  {
    Fq s = fd_from_mont(rcv_sum);
    uint8_t b[32];
    memcpy(b, s.l, 32);
    out.insert(out.end(), b, b + 32);
  }
  put_u32(0);  // hints: empty
  return emit_proof(out, ptx_out, cap, out_len);
}

/* verify one borsh ShieldedPartialTransaction end-to-end
 * (ShieldedPartialTransaction::execute, shielded_ptx.rs:232-240):
 * batch-verify ALL compliance proofs (slot_compliance) and ALL RL proofs
 * (slot_rl, vk bytes must match the slot's key), then the consistency
 * checks: every RL root equals the others (resource merkle root), input
 * RL self-ids == compliance nfs, output RL self-ids == compliance cms.
 * Returns TG_OK, -1 proof failure, -3xx consistency, -2xx structure. */
int tg_ptx_verify(tg_ctx* ctx, int slot_compliance, int slot_rl,
                  const uint8_t* ptx, size_t len) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  int rc = tg_select_key(ctx, slot_rl);
  if (rc) return rc;
  PPk* rlk = c->ppk;
  uint32_t vk_len = 32u * (uint32_t)(rlk->fixed_commits.size() +
                                     rlk->sigma_commits.size());
  const std::vector<uint8_t> vk_ref = pk_vk_bytes(rlk);
  TxCursor cur{ptx, len};
  uint32_t n_cvi;
  if (!cur.u32(n_cvi) || n_cvi > 64) return -201;
  std::vector<const uint8_t*> cproof;
  std::vector<size_t> cplen;
  std::vector<uint8_t> cinst;  // 9 rows x 32 per proof
  std::vector<uint8_t> nfs, cms;
  for (uint32_t i = 0; i < n_cvi; i++) {
    uint32_t plen;
    const uint8_t* p;
    if (!cur.u32(plen) || plen > (1u << 20) || !cur.take(p, plen)) return -202;
    cproof.push_back(p);
    cplen.push_back(plen);
    const uint8_t* inst;
    if (!cur.take(inst, 192)) return -203;
    uint8_t rows[288];
    if (!compliance_rows_expand(inst, rows)) return -204;
    cinst.insert(cinst.end(), rows, rows + 288);
    nfs.insert(nfs.end(), rows, rows + 32);
    cms.insert(cms.end(), rows + 64, rows + 96);
  }
  uint32_t n_in = 0, n_out = 0;
  std::vector<const uint8_t*> rproof;
  std::vector<size_t> rplen;
  std::vector<const uint8_t*> rinst;
  std::vector<uint8_t> self_ids, roots;
  for (int grp = 0; grp < 2; grp++) {
    uint32_t cnt;
    if (!cur.u32(cnt) || cnt > 128) return -205;
    (grp == 0 ? n_in : n_out) = cnt;
    for (uint32_t i = 0; i < cnt; i++) {
      const uint8_t* vkb;
      if (!cur.take(vkb, vk_len)) return -206;
      if (memcmp(vkb, vk_ref.data(), vk_len) != 0)
        return -207;  // unknown RL vk (only the TrivialRL key is loaded)
      uint32_t plen;
      const uint8_t* p;
      if (!cur.u32(plen) || plen > (1u << 20) || !cur.take(p, plen)) return -208;
      const uint8_t* inst;
      if (!cur.take(inst, 22 * 32)) return -209;
      rproof.push_back(p);
      rplen.push_back(plen);
      rinst.push_back(inst);
      roots.insert(roots.end(), inst, inst + 32);
      self_ids.insert(self_ids.end(), inst + 32, inst + 64);
      uint32_t ndyn;
      if (!cur.u32(ndyn) || ndyn != 0) return -210;  // dynamic RLs: not built
    }
  }
  const uint8_t* b;
  if (!cur.take(b, 1)) return -211;
  if (*b == 1 && !cur.take(b, 32)) return -212;
  uint32_t n_hints;
  if (!cur.u32(n_hints) || !cur.take(b, n_hints)) return -213;
  if (cur.left != 0) return -214;
  // consistency (shielded_ptx.rs:156-230): roots all equal; input self-ids
  // match nfs in order; output self-ids match cms
  for (uint32_t i = 1; i < n_in + n_out; i++)
    if (memcmp(roots.data(), roots.data() + 32ul * i, 32) != 0) return -301;
  if (n_in != n_cvi || n_out != n_cvi) return -302;
  for (uint32_t i = 0; i < n_in; i++)
    if (memcmp(self_ids.data() + 32ul * i, nfs.data() + 32ul * i, 32) != 0)
      return -303;
  for (uint32_t i = 0; i < n_out; i++)
    if (memcmp(self_ids.data() + 32ul * (n_in + i), cms.data() + 32ul * i, 32) != 0)
      return -304;
  // no proofs at all is not a bundle this entry accepts
  if (n_cvi == 0) return TG_ERR_BADARG;
  return verify_rl_then_compliance(ctx, slot_rl, slot_compliance, rinst, rproof, rplen,
                                   cinst, cproof, cplen);
}

int tg_create_proof_raw(tg_ctx* ctx, const uint8_t* instance, const uint8_t* advice,
                        const uint8_t rng_seed[32], uint8_t* proof_out, size_t cap,
                        size_t* out_len) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  if (!c->ppk || !c->ppk->ready) return TG_ERR_STATE;
  std::vector<uint8_t> proof;
  int rc = pprove_raw(c, *c->ppk, instance, advice, rng_seed, proof);
  if (rc != 0) return rc;
  return emit_proof(proof, proof_out, cap, out_len);
}

}  /* extern "C" */

// ---------- diagnostics: the opening-phase kernels on caller data ----------

// canonical LE caller bytes -> Montgomery host vector; false if any is >= p
static bool diag_to_mont(const uint8_t* src, size_t count, std::vector<Fp>& out) {
  out.resize(count);
  for (size_t i = 0; i < count; i++) {
    Fp v;
    memcpy(v.l, src + 32 * i, 32);
    if (!fd_is_canonical(v)) return false;
    out[i] = fd_to_mont(v);
  }
  return true;
}

static void diag_from_mont(const std::vector<Fp>& in, uint8_t* dst) {
  for (size_t i = 0; i < in.size(); i++) {
    Fp v = fd_from_mont(in[i]);
    memcpy(dst + 32 * i, v.l, 32);
  }
}

// a device copy of a Montgomery host vector (at least one element long)
static hipError_t diag_upload(Ctx* c, DevTmp<Fp>& d, const std::vector<Fp>& h) {
  hipError_t e = d.alloc(std::max<size_t>(1, h.size()));
  if (e != hipSuccess) return e;
  return hipMemcpyAsync(d.p, h.data(), h.size() * sizeof(Fp), hipMemcpyHostToDevice,
                        c->stream);
}

// the diagnostics' own staging, released on every way out
struct DiagDev {
  ProverDev pd;
  ~DiagDev() { pdev_free(pd); }
};

extern "C" {

int tg_fp_poly_eval_batch(tg_ctx* ctx, const uint8_t* coeffs, size_t n_coeffs,
                          const uint64_t* offs, const uint64_t* lens,
                          const uint8_t* points, size_t nq, uint8_t* out) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  if (!nq) return TG_ERR_BADARG;
  std::vector<Fp> h, pts;
  if (!diag_to_mont(coeffs, n_coeffs, h) || !diag_to_mont(points, nq, pts))
    return TG_ERR_ENCODING;
  DevTmp<Fp> d;
  hipError_t e = diag_upload(c, d, h);
  if (e != hipSuccess) return set_err(c, "eval upload", e);
  std::vector<EvalQuery> qs(nq);
  for (size_t q = 0; q < nq; q++) {
    if (offs[q] > n_coeffs || lens[q] > n_coeffs - offs[q]) return TG_ERR_BADARG;
    qs[q] = EvalQuery{d.p + offs[q], (long)lens[q], pts[q]};
  }
  DiagDev dd;
  std::vector<Fp> evs(nq);
  int rc = dev_poly_eval_batch(c, dd.pd, qs, evs.data());
  if (rc) return rc;
  if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return set_err(c, "eval", e);
  diag_from_mont(evs, out);
  return TG_OK;
}

int tg_fp_kate_div(tg_ctx* ctx, uint8_t* coeffs, size_t len, const uint8_t* points,
                   size_t npts) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  if (!len || !npts || npts > len) return TG_ERR_BADARG;
  std::vector<Fp> h, pts;
  if (!diag_to_mont(coeffs, len, h) || !diag_to_mont(points, npts, pts))
    return TG_ERR_ENCODING;
  DevTmp<Fp> d_src, d_dst;
  hipError_t e = diag_upload(c, d_src, h);
  if (e == hipSuccess) e = d_dst.alloc(len);
  if (e != hipSuccess) return set_err(c, "kate upload", e);
  DiagDev dd;
  // as in multiopen: the first division leaves its source alone, the
  // following ones run in place on a vector one shorter each time
  for (size_t j = 0; j < npts; j++) {
    std::vector<KateJob> job{
        KateJob{j == 0 ? d_src.p : d_dst.p, d_dst.p, (long)(len - j), pts[j]}};
    int rc = dev_kate_div(c, dd.pd, job);
    if (rc) return rc;
  }
  hipMemcpyAsync(h.data(), d_dst.p, len * sizeof(Fp), hipMemcpyDeviceToHost, c->stream);
  if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return set_err(c, "kate", e);
  diag_from_mont(h, coeffs);
  return TG_OK;
}

int tg_fp_horner_comb(tg_ctx* ctx, const uint8_t* polys, size_t np, size_t n,
                      const uint8_t challenge[32], uint8_t* out) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  if (!np || !n) return TG_ERR_BADARG;
  std::vector<Fp> h, ch;
  if (!diag_to_mont(polys, np * n, h) || !diag_to_mont(challenge, 1, ch))
    return TG_ERR_ENCODING;
  DevTmp<Fp> d, d_out;
  hipError_t e = diag_upload(c, d, h);
  if (e == hipSuccess) e = d_out.alloc(n);
  if (e != hipSuccess) return set_err(c, "comb upload", e);
  std::vector<const Fp*> ptrs(np);
  for (size_t j = 0; j < np; j++) ptrs[j] = d.p + j * n;
  DiagDev dd;
  int rc = dev_horner_comb(c, dd.pd, ptrs, ch[0], d_out.p, (long)n);
  if (rc) return rc;
  std::vector<Fp> res(n);
  hipMemcpyAsync(res.data(), d_out.p, n * sizeof(Fp), hipMemcpyDeviceToHost, c->stream);
  if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return set_err(c, "comb", e);
  diag_from_mont(res, out);
  return TG_OK;
}

int tg_ipa_open_probe(tg_ctx* ctx, uint32_t k, const uint8_t* poly, const uint8_t x3[32],
                      const uint8_t* challenges, const uint8_t* round_blinds,
                      const uint8_t blind[32], uint8_t* lr_out, uint8_t a_out[32],
                      uint8_t blind_out[32]) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  if (c->k < 0) return TG_ERR_NOSRS;
  if (k < 1 || (int)k > c->k) return TG_ERR_BADARG;
  size_t n = (size_t)1 << k;
  std::vector<Fp> pp, pt, us, rb, b0;
  if (!diag_to_mont(poly, n, pp) || !diag_to_mont(x3, 1, pt) ||
      !diag_to_mont(challenges, k, us) || !diag_to_mont(round_blinds, 2 * (size_t)k, rb) ||
      !diag_to_mont(blind, 1, b0))
    return TG_ERR_ENCODING;
  for (const Fp& u : us)
    if (fd_is_zero(u)) return TG_ERR_BADARG;
  DevTmp<Fp> d_pp, d_bvec, d_wfold;
  hipError_t e = diag_upload(c, d_pp, pp);
  if (e == hipSuccess) e = d_bvec.alloc(n);
  if (e == hipSuccess) e = d_wfold.alloc(n);
  if (e != hipSuccess) return set_err(c, "ipa probe upload", e);
  fill_powers_launch(d_bvec.p, (long)n, pt[0], c->stream);
  hipLaunchKernelGGL(k_fill_const, dim3(opn_grid((long)n)), dim3(256), 0, c->stream,
                     d_wfold.p, (long)n, fd_one_mont<FpCfg>());
  FixedMulTab utab, wtab;
  utab.init(c->h_u);
  wtab.init(c->h_w);
  DiagDev dd;
  Fp blind_acc = b0[0], a_final;
  int round = 0;
  auto put_point = [](uint8_t* dst, const VestaAff& p) {
    if (aff_is_identity(p)) {
      memset(dst, 0, 64);
      return;
    }
    Fq x = fd_from_mont(p.x), y = fd_from_mont(p.y);
    memcpy(dst, x.l, 32);
    memcpy(dst + 32, y.l, 32);
  };
  int rc = ipa_rounds_dev(
      c, dd.pd, (int)k, d_pp.p, d_bvec.p, d_wfold.p, utab, wtab, blind_acc, a_final,
      [&](Fp& l_rand, Fp& r_rand) {
        l_rand = rb[2 * round];
        r_rand = rb[2 * round + 1];
      },
      [&](const VestaAff& La, const VestaAff& Ra, Fp& uch) {
        put_point(lr_out + 128 * (size_t)round, La);
        put_point(lr_out + 128 * (size_t)round + 64, Ra);
        uch = us[round++];
        return 0;
      },
      [](int) {});
  if (rc) return rc;
  diag_from_mont({a_final}, a_out);
  diag_from_mont({blind_acc}, blind_out);
  return TG_OK;
}

// ---------- diagnostics: the grand-product kernels on caller data ----------

// most elements one of these calls takes (512 MiB of field elements)
static const size_t GP_DIAG_MAX = (size_t)1 << 24;

// download count Montgomery elements from d and write them out canonical
static int diag_download(Ctx* c, const Fp* d, size_t count, uint8_t* out,
                         const char* where) {
  std::vector<Fp> res(count);
  hipMemcpyAsync(res.data(), d, count * sizeof(Fp), hipMemcpyDeviceToHost, c->stream);
  hipError_t e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return set_err(c, where, e);
  diag_from_mont(res, out);
  return TG_OK;
}

int tg_fp_batch_inverse(tg_ctx* ctx, uint8_t* vals, size_t n) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  if (!n || n > GP_DIAG_MAX) return TG_ERR_BADARG;
  std::vector<Fp> h;
  if (!diag_to_mont(vals, n, h)) return TG_ERR_ENCODING;
  DevTmp<Fp> d;
  hipError_t e = diag_upload(c, d, h);
  if (e != hipSuccess) return set_err(c, "inverse upload", e);
  int rc = dev_gp_batch_inverse(c, d.p, (long)n);
  if (rc) return rc;
  return diag_download(c, d.p, n, vals, "inverse");
}

int tg_fp_prefix_product(tg_ctx* ctx, const uint8_t* ratios, const uint64_t* seg_lens,
                         size_t nseg, const uint8_t init[32], uint8_t* z_out) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  if (!nseg || nseg > GP_DIAG_MAX) return TG_ERR_BADARG;
  size_t total = 0;
  for (size_t s = 0; s < nseg; s++) {
    if (!seg_lens[s] || seg_lens[s] > GP_DIAG_MAX - total) return TG_ERR_BADARG;
    total += seg_lens[s];
  }
  std::vector<Fp> h, i0;
  if (!diag_to_mont(ratios, total, h) || !diag_to_mont(init, 1, i0))
    return TG_ERR_ENCODING;
  DevTmp<Fp> d, d_z;
  hipError_t e = diag_upload(c, d, h);
  if (e == hipSuccess) e = d_z.alloc(total + nseg);
  if (e != hipSuccess) return set_err(c, "prefix upload", e);
  std::vector<GpSeg> segs(nseg);
  size_t zo = 0;
  for (size_t s = 0; s < nseg; s++) {
    segs[s] = GpSeg{(long)seg_lens[s], d_z.p + zo, s > 0, i0[0]};
    zo += seg_lens[s] + 1;
  }
  DiagDev dd;
  int rc = dev_gp_scan(c, dd.pd, d.p, nullptr, segs);
  if (rc) return rc;
  return diag_download(c, d_z.p, total + nseg, z_out, "prefix");
}

int tg_perm_product_probe(tg_ctx* ctx, uint32_t k, uint64_t u, uint32_t ncols,
                          uint32_t chunk_len, const uint8_t* values, const uint8_t* sigmas,
                          const uint8_t beta[32], const uint8_t gamma[32], uint8_t* z_out) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  if (k < 4 || k > 15 || !ncols || ncols > (uint32_t)TG_MAX_PERM || !chunk_len)
    return TG_ERR_BADARG;
  size_t n = (size_t)1 << k;
  if (u < 1 || u >= n) return TG_ERR_BADARG;
  uint32_t nchunks = (ncols + chunk_len - 1) / chunk_len;
  if (nchunks > (uint32_t)TG_MAX_CHUNKS) return TG_ERR_BADARG;
  std::vector<Fp> hv, hs, bg, gm;
  if (!diag_to_mont(values, ncols * n, hv) || !diag_to_mont(sigmas, ncols * n, hs) ||
      !diag_to_mont(beta, 1, bg) || !diag_to_mont(gamma, 1, gm))
    return TG_ERR_ENCODING;
  DevTmp<Fp> d_v, d_s, d_num, d_den, d_z;
  hipError_t e = diag_upload(c, d_v, hv);
  if (e == hipSuccess) e = diag_upload(c, d_s, hs);
  if (e == hipSuccess) e = d_num.alloc(nchunks * u);
  if (e == hipSuccess) e = d_den.alloc(nchunks * u);
  if (e == hipSuccess) e = d_z.alloc(nchunks * (u + 1));
  if (e != hipSuccess) return set_err(c, "perm probe upload", e);
  // omega and delta as keygen derives them
  Fp omega = host_domain_omega((int)k, false);
  Fp delta{{5, 0, 0, 0}};
  delta = fd_to_mont(delta);
  for (int i = 0; i < 32; i++) delta = fd_sqr(delta);
  std::vector<const Fp*> cols(ncols), sig(ncols);
  for (uint32_t j = 0; j < ncols; j++) {
    cols[j] = d_v.p + j * n;
    sig[j] = d_s.p + j * n;
  }
  DiagDev dd;
  int rc = dev_gp_perm_terms(c, dd.pd, cols, sig, (int)chunk_len, (long)u, bg[0], gm[0],
                             omega, delta, d_num.p, d_den.p);
  if (!rc) rc = dev_gp_batch_inverse(c, d_den.p, (long)(nchunks * u));
  if (rc) return rc;
  std::vector<GpSeg> segs(nchunks);
  for (uint32_t ch = 0; ch < nchunks; ch++)
    segs[ch] = GpSeg{(long)u, d_z.p + ch * (u + 1), ch > 0, fd_one_mont<FpCfg>()};
  if ((rc = dev_gp_scan(c, dd.pd, d_num.p, d_den.p, segs))) return rc;
  return diag_download(c, d_z.p, nchunks * (u + 1), z_out, "perm probe");
}

int tg_lookup_product_probe(tg_ctx* ctx, uint32_t k, uint64_t u, const uint8_t* a,
                            const uint8_t* s, const uint8_t* ap, const uint8_t* sp,
                            const uint8_t beta[32], const uint8_t gamma[32],
                            uint8_t* z_out) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  if (k < 4 || k > 15) return TG_ERR_BADARG;
  size_t n = (size_t)1 << k;
  if (u < 1 || u >= n) return TG_ERR_BADARG;
  std::vector<Fp> h[4], bg, gm;
  const uint8_t* src[4] = {a, s, ap, sp};
  for (int v = 0; v < 4; v++)
    if (!diag_to_mont(src[v], n, h[v])) return TG_ERR_ENCODING;
  if (!diag_to_mont(beta, 1, bg) || !diag_to_mont(gamma, 1, gm)) return TG_ERR_ENCODING;
  DevTmp<Fp> d_in[4], d_num, d_den, d_z;
  hipError_t e = hipSuccess;
  for (int v = 0; v < 4 && e == hipSuccess; v++) e = diag_upload(c, d_in[v], h[v]);
  if (e == hipSuccess) e = d_num.alloc(u);
  if (e == hipSuccess) e = d_den.alloc(u);
  if (e == hipSuccess) e = d_z.alloc(u + 1);
  if (e != hipSuccess) return set_err(c, "lookup probe upload", e);
  const Fp *pa = d_in[0].p, *ps = d_in[1].p, *pap = d_in[2].p, *psp = d_in[3].p;
  DiagDev dd;
  int rc = dev_gp_lookup_terms(c, dd.pd, 1, &pa, &ps, &pap, &psp, (long)u, bg[0], gm[0],
                               d_num.p, d_den.p);
  if (!rc) rc = dev_gp_batch_inverse(c, d_den.p, (long)u);
  if (rc) return rc;
  std::vector<GpSeg> segs{GpSeg{(long)u, d_z.p, false, fd_one_mont<FpCfg>()}};
  if ((rc = dev_gp_scan(c, dd.pd, d_num.p, d_den.p, segs))) return rc;
  return diag_download(c, d_z.p, u + 1, z_out, "lookup probe");
}

int tg_lookup_permute_probe(tg_ctx* ctx, uint64_t u, const uint8_t* a, const uint8_t* s,
                            uint8_t* ap_out, uint8_t* sp_out) {
  Ctx* c = (Ctx*)ctx;
  if (!c || tg_enter(c)) return TG_ERR_BADARG;
  if (!u || u > (uint64_t)LK_MAX_U) return TG_ERR_BADARG;
  std::vector<Fp> ha, hs;
  if (!diag_to_mont(a, u, ha) || !diag_to_mont(s, u, hs)) return TG_ERR_ENCODING;
  // the prover sorts in slots of n = 2^k rows; here the network's own size
  const size_t np = (size_t)lk_padded((long)u);
  DevTmp<Fp> d_a, d_s, d_ap, d_t, d_sp;
  hipError_t e = diag_upload(c, d_a, ha);
  if (e == hipSuccess) e = diag_upload(c, d_s, hs);
  if (e == hipSuccess) e = d_ap.alloc(np);
  if (e == hipSuccess) e = d_t.alloc(np);
  if (e == hipSuccess) e = d_sp.alloc(u);
  if (e != hipSuccess) return set_err(c, "permute probe upload", e);
  const Fp* src[2] = {d_a.p, d_s.p};
  Fp* dst[2] = {d_ap.p, d_t.p};
  Fp *pap = d_ap.p, *psp = d_sp.p;
  const Fp* pt = d_t.p;
  DiagDev dd;
  int rc = dev_lk_sort(c, 2, src, dst, (long)u, (long)np);
  if (!rc) rc = dev_lk_permute(c, dd.pd, 1, &pap, &pt, &psp, (long)u);
  if (rc) return rc;
  dev_lk_fetch_err(c, dd.pd);
  e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return set_err(c, "permute probe", e);
  if (dd.pd.lk_err_h) return TG_ERR_BADARG;  // an element of a is missing from s
  rc = diag_download(c, d_ap.p, u, ap_out, "permute probe");
  if (rc) return rc;
  return diag_download(c, d_sp.p, u, sp_out, "permute probe");
}

}  /* extern "C" */
