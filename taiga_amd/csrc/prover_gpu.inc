// prover_gpu.inc — product prover: GPU-offloaded pipeline over a Ctx.
// Included by taiga_gpu.cpp AFTER the Ctx definition (single TU).
// See prover_impl.hpp header for the boundary/parity statement.

namespace taiga {

// ---------------- device helpers over Ctx ----------------

struct ProverDev {
  Fp* ws0 = nullptr;  // ext_n-sized scratch
  Fp* ws1 = nullptr;
  void* d_hargs = nullptr;  // device-resident HFoldArgs (too big for kernel args)
  Fp* sc_stage = nullptr;  // batched-MSM scalar staging
  long sc_cap = 0;
  std::vector<Fp*> ext_pool;  // per-proof device ext buffers (h-fold inputs)
  // opening phase (openings.hip): n-element slots holding the coefficient
  // form of every per-proof polynomial the openings read, sized from the
  // descriptor at keygen; the multiopen / IPA work vectors, sized when the
  // number of point sets is first known; and the staging of the small
  // per-launch tables and results
  Fp* coef = nullptr;
  int coef_slots = 0;
  Fp* open_ws = nullptr;
  int open_slots = 0;
  void* d_stage = nullptr;
  size_t stage_cap = 0;
  Fp* d_small = nullptr;
  size_t small_cap = 0;
  // grand products (grand_products.hip): n-element slots holding Lagrange
  // forms, sized from the descriptor at keygen. The sigma columns and the
  // fixed columns of the permutation are uploaded once per key; per proof
  // the advice and instance columns, the lookup vectors and the z vectors
  // live here, where the commits, the grand-product kernels and the
  // transforms all read them; the last slots hold the flat num / den arrays.
  Fp* lag = nullptr;
  int lag_slots = 0;
  // host copies of the small tables those launchers upload: they must
  // outlive the stream's next synchronisation
  GpPermArgs gp_perm_h;
  GpLookupArgs gp_lk_h;
  std::vector<uint8_t> gp_scan_h;
  // lookup argument (lookup_argument.hip): the 32-bit work arrays of the S'
  // construction (error word, flags, their scan, leftover positions, block
  // sums), the host copy of the error word, and the device argument block of
  // k_lk_compress (built once per key)
  uint32_t* lk_ws = nullptr;
  size_t lk_ws_cap = 0;
  uint32_t lk_err_h = 0;
  void* d_lkargs = nullptr;
  NttPlan plan_n, plan_ext;
  long ext_n = 0, n = 0;
};

// grow-only device buffer; the stream is drained before the old one goes
template <class T>
static T* pdev_grow(Ctx* c, T*& p, size_t& cap, size_t need) {
  if (cap >= need) return p;
  if (p) {
    hipStreamSynchronize(c->stream);
    hipFree(p);
    p = nullptr;
    cap = 0;
  }
  if (hipMalloc(&p, need * sizeof(T)) != hipSuccess) return nullptr;
  cap = need;
  return p;
}

static void* pdev_stage(Ctx* c, ProverDev& pd, size_t bytes) {
  uint8_t* p = (uint8_t*)pd.d_stage;
  p = pdev_grow(c, p, pd.stage_cap, std::max<size_t>(bytes, 16384));
  pd.d_stage = p;
  return p;
}

static Fp* pdev_small(Ctx* c, ProverDev& pd, size_t count) {
  return pdev_grow(c, pd.d_small, pd.small_cap,
                   std::max<size_t>(count, 2 * OPN_GRID_MAX));
}

// n-element slot arrays: (re)allocated only when more slots are needed
static Fp* pdev_slots(Ctx* c, Fp*& p, int& have, int want, long n) {
  size_t cap = (size_t)have * n;
  Fp* r = pdev_grow(c, p, cap, (size_t)want * n);
  have = (int)(cap / n);
  return r;
}

static hipError_t pdev_init(Ctx* c, ProverDev& pd, int k, int ext_k) {
  long n = 1L << k, ext_n = 1L << ext_k;
  if (pd.ext_n >= ext_n && pd.n >= n) return hipSuccess;
  hipError_t e;
  if (pd.ws0) hipFree(pd.ws0);
  if (pd.ws1) hipFree(pd.ws1);
  if ((e = hipMalloc(&pd.ws0, ext_n * sizeof(Fp))) != hipSuccess) return e;
  if ((e = hipMalloc(&pd.ws1, ext_n * sizeof(Fp))) != hipSuccess) return e;
  if ((e = ntt_plan_init(pd.plan_n, k, c->stream)) != hipSuccess) return e;
  if ((e = ntt_plan_init(pd.plan_ext, ext_k, c->stream)) != hipSuccess) return e;
  pd.ext_n = ext_n;
  pd.n = n;
  return hipSuccess;
}

static Fp* pdev_ext_buf(ProverDev& pd, size_t idx) {
  while (pd.ext_pool.size() <= idx) {
    Fp* p = nullptr;
    if (hipMalloc(&p, pd.ext_n * sizeof(Fp)) != hipSuccess) return nullptr;
    pd.ext_pool.push_back(p);
  }
  return pd.ext_pool[idx];
}

static void pdev_free(ProverDev& pd) {
  for (Fp* p : pd.ext_pool) hipFree(p);
  pd.ext_pool.clear();
  if (pd.coef) hipFree(pd.coef);
  if (pd.lag) hipFree(pd.lag);
  if (pd.open_ws) hipFree(pd.open_ws);
  if (pd.d_stage) hipFree(pd.d_stage);
  if (pd.d_small) hipFree(pd.d_small);
  if (pd.d_hargs) hipFree(pd.d_hargs);
  if (pd.lk_ws) hipFree(pd.lk_ws);
  if (pd.d_lkargs) hipFree(pd.d_lkargs);
  if (pd.sc_stage) hipFree(pd.sc_stage);
  if (pd.ws0) hipFree(pd.ws0);
  if (pd.ws1) hipFree(pd.ws1);
  if (pd.plan_n.d_tw_fwd) hipFree(pd.plan_n.d_tw_fwd);
  if (pd.plan_n.d_tw_inv) hipFree(pd.plan_n.d_tw_inv);
  if (pd.plan_ext.d_tw_fwd) hipFree(pd.plan_ext.d_tw_fwd);
  if (pd.plan_ext.d_tw_inv) hipFree(pd.plan_ext.d_tw_inv);
  pd = ProverDev();
}

// lagrange(Mont host) -> coeff(Mont host), via GPU iNTT
static int gpu_lag_to_coeff(Ctx* c, ProverDev& pd, Fp* data, int k, const Fp& ninv) {
  long n = 1L << k;
  hipMemcpyAsync(pd.ws0, data, n * sizeof(Fp), hipMemcpyHostToDevice, c->stream);
  if (ntt_run(pd.ws0, pd.ws1, pd.plan_n, k, true, c->stream, &ninv, ntt_noprof) !=
      hipSuccess)
    return TG_ERR_HIP;
  hipMemcpyAsync(data, pd.ws0, n * sizeof(Fp), hipMemcpyDeviceToHost, c->stream);
  return hipStreamSynchronize(c->stream) == hipSuccess ? 0 : TG_ERR_HIP;
}

// coeff(n) -> extended-coset evals(ext_n), via zeta-distribute + GPU NTT
static int gpu_coeff_to_ext(Ctx* c, ProverDev& pd, const Fp* coeff, Fp* ext_out, int k,
                            int ext_k, const Fp& zeta) {
  long n = 1L << k, ext_n = 1L << ext_k;
  hipMemcpyAsync(pd.ws0, coeff, n * sizeof(Fp), hipMemcpyHostToDevice, c->stream);
  hipMemsetAsync(pd.ws0 + n, 0, (ext_n - n) * sizeof(Fp), c->stream);
  coset_scale_launch(pd.ws0, (u64)ext_n, zeta, c->stream);
  if (ntt_run(pd.ws0, pd.ws1, pd.plan_ext, ext_k, false, c->stream, nullptr,
              ntt_noprof) != hipSuccess)
    return TG_ERR_HIP;
  hipMemcpyAsync(ext_out, pd.ws0, ext_n * sizeof(Fp), hipMemcpyDeviceToHost, c->stream);
  return hipStreamSynchronize(c->stream) == hipSuccess ? 0 : TG_ERR_HIP;
}

// fused: lagrange(host, Mont) -> coeff, left on device in the coefficient
// pool slot d_coeff_dst (the openings read it there; it never returns to
// the host) + extended-coset evals left on device in d_ext_dst
static int gpu_lag_to_coeff_ext_dev(Ctx* c, ProverDev& pd, const Fp* lag,
                                    Fp* d_coeff_dst, Fp* d_ext_dst, int k, int ext_k,
                                    const Fp& ninv, const Fp& zeta,
                                    hipMemcpyKind from = hipMemcpyHostToDevice) {
  long n = 1L << k, ext_n = 1L << ext_k;
  hipMemcpyAsync(pd.ws0, lag, n * sizeof(Fp), from, c->stream);
  if (ntt_run(pd.ws0, pd.ws1, pd.plan_n, k, true, c->stream, &ninv, ntt_noprof) !=
      hipSuccess)
    return TG_ERR_HIP;
  hipMemcpyAsync(d_coeff_dst, pd.ws0, n * sizeof(Fp), hipMemcpyDeviceToDevice, c->stream);
  hipMemcpyAsync(d_ext_dst, pd.ws0, n * sizeof(Fp), hipMemcpyDeviceToDevice, c->stream);
  hipMemsetAsync(d_ext_dst + n, 0, (ext_n - n) * sizeof(Fp), c->stream);
  coset_scale_launch(d_ext_dst, (u64)ext_n, zeta, c->stream);
  if (ntt_run(d_ext_dst, pd.ws1, pd.plan_ext, ext_k, false, c->stream, nullptr,
              ntt_noprof) != hipSuccess)
    return TG_ERR_HIP;
  return 0;  // a host lag must outlive the stream's next synchronisation
}

// the same from a Lagrange vector already on the device (a slot of the
// Lagrange pool), which is left as it is
static int gpu_dlag_to_coeff_ext_dev(Ctx* c, ProverDev& pd, const Fp* d_lag,
                                     Fp* d_coeff_dst, Fp* d_ext_dst, int k, int ext_k,
                                     const Fp& ninv, const Fp& zeta) {
  return gpu_lag_to_coeff_ext_dev(c, pd, d_lag, d_coeff_dst, d_ext_dst, k, ext_k, ninv,
                                  zeta, hipMemcpyDeviceToDevice);
}

// workspace and the canonical-scalar array for B MSMs of nn points each.
// The array is the buffer tg_scalars_upload fills: the prover is about to
// overwrite it, so from here on it holds no caller scalars (tg_msm_resident
// answers TG_ERR_STATE until the next tg_scalars_upload).
static int gpu_msm_reserve(Ctx* c, long nn, int B) {
  long ntot = nn * B;
  c->n_scalars = 0;
  if (msm_work_alloc(c->msm, (u64)ntot, (u64)B) != hipSuccess) return TG_ERR_NOMEM;
  if (!c->d_scalars || c->cap_scalars < (u64)ntot) {
    if (c->d_scalars) {
      hipStreamSynchronize(c->stream);
      hipFree(c->d_scalars);
      c->d_scalars = nullptr;
    }
    c->cap_scalars = 0;
    if (hipMalloc(&c->d_scalars, ntot * sizeof(ScalarRepr)) != hipSuccess) {
      c->d_scalars = nullptr;
      return TG_ERR_NOMEM;
    }
    c->cap_scalars = (u64)ntot;
  }
  return 0;
}

// Batched GPU MSM: B same-size MSMs (nn points each) over ONE device base
// array, one kernel chain, from the B concatenated CANONICAL scalar vectors
// already in c->d_scalars (gpu_msm_reserve'd). Each result gets its
// blind*W added via the fixed-point table.
static int gpu_msm_commit_canon(Ctx* c, long nn, int B, const VestaAff* d_bases,
                                const Fp* blinds, VestaAff* outs,
                                const FixedMulTab* wtab) {
  long ntot = nn * B;
  ProfScope total(c, P_MSM_TOTAL);
  // the SRS sets go through their fixed-base tables: one point per MSM comes
  // back and there is nothing to combine
  const MsmPlan plan = msm_plan_for(c, d_bases, nn);
  const size_t per = (size_t)plan.sets();
  std::vector<VestaJac> sums(per * B);
  // only the two accumulation kernels are bracketed here (bench.py reads
  // msm_bucket_acc with profiling on; more event records would sit inside
  // its timed region)
  auto prof = [&](int idx) {
    return ProfScope(c, idx == MSM_P_ACC_KERNELS ? (int)P_MSM_ACC : -1);
  };
  msm_run(c->msm, c->d_scalars, (u64)ntot, (u64)nn, (u64)B, plan, c->stream, sums.data(), prof);
  if (hipStreamSynchronize(c->stream) != hipSuccess) return TG_ERR_HIP;
#ifdef _OPENMP
#pragma omp parallel for schedule(static)
#endif
  for (int b = 0; b < B; b++) {
    VestaJac acc = msm_finish(plan, sums.data() + per * b);
    if (!fd_is_zero(blinds[b])) acc = jac_add(acc, wtab->mul(blinds[b]));
    outs[b] = jac_to_aff(acc);
  }
  return 0;
}

// the same from B concatenated Montgomery vectors already on the device
static int gpu_msm_commit_batch_dev(Ctx* c, const Fp* d_mont_scalars, long nn, int B,
                                    const VestaAff* d_bases, const Fp* blinds,
                                    VestaAff* outs, const FixedMulTab* wtab) {
  long ntot = nn * B;
  int rc = gpu_msm_reserve(c, nn, B);
  if (rc) return rc;
  hipLaunchKernelGGL(k_from_mont<FpCfg>, dim3(ntt_grid(ntot)), dim3(256), 0, c->stream,
                     (Fp*)c->d_scalars, d_mont_scalars, (u64)ntot);
  return gpu_msm_commit_canon(c, nn, B, d_bases, blinds, outs, wtab);
}

// ... and from host Montgomery vectors: upload, then the device form
static int gpu_msm_commit_batch(Ctx* c, ProverDev& pd, const Fp* mont_scalars, long nn,
                                int B, const VestaAff* d_bases, const Fp* blinds,
                                VestaAff* outs, const FixedMulTab* wtab) {
  long ntot = nn * B;
  size_t cap = (size_t)pd.sc_cap;
  if (!pdev_grow(c, pd.sc_stage, cap, (size_t)ntot)) return TG_ERR_NOMEM;
  pd.sc_cap = (long)cap;
  hipMemcpyAsync(pd.sc_stage, mont_scalars, ntot * sizeof(Fp), hipMemcpyHostToDevice,
                 c->stream);
  return gpu_msm_commit_batch_dev(c, pd.sc_stage, nn, B, d_bases, blinds, outs, wtab);
}

// ---------------- opening-phase launchers (kernels: openings.hip) ---------
// Each enqueues on the context's stream and returns; results the host needs
// are valid after the caller's next stream synchronisation. The small
// tables go through pd.d_stage: a later table's upload is stream-ordered
// behind the kernel that reads the earlier one.

// evs_host[q] = poly_q(x_q) for every query, one launch
static int dev_poly_eval_batch(Ctx* c, ProverDev& pd, const std::vector<EvalQuery>& qs,
                               Fp* evs_host) {
  if (qs.empty()) return 0;
  size_t nq = qs.size();
  EvalQuery* dq = (EvalQuery*)pdev_stage(c, pd, nq * sizeof(EvalQuery));
  Fp* dout = pdev_small(c, pd, nq);
  if (!dq || !dout) return TG_ERR_NOMEM;
  hipMemcpyAsync(dq, qs.data(), nq * sizeof(EvalQuery), hipMemcpyHostToDevice, c->stream);
  hipLaunchKernelGGL(k_poly_eval_batch, dim3((unsigned)nq), dim3(OPN_T), 0, c->stream,
                     (const EvalQuery*)dq, dout);
  hipMemcpyAsync(evs_host, dout, nq * sizeof(Fp), hipMemcpyDeviceToHost, c->stream);
  return 0;
}

// d_out[i] = Horner over polys[..][i] in ch (first poly highest power)
static int dev_horner_comb(Ctx* c, ProverDev& pd, const std::vector<const Fp*>& polys,
                           const Fp& ch, Fp* d_out, long n) {
  if (polys.empty()) return TG_ERR_BADARG;
  const Fp** dp = (const Fp**)pdev_stage(c, pd, polys.size() * sizeof(Fp*));
  if (!dp) return TG_ERR_NOMEM;
  hipMemcpyAsync(dp, polys.data(), polys.size() * sizeof(Fp*), hipMemcpyHostToDevice,
                 c->stream);
  hipLaunchKernelGGL(k_horner_comb, dim3(ntt_grid(n)), dim3(256), 0, c->stream,
                     (const Fp* const*)dp, (int)polys.size(), ch, d_out, n);
  return 0;
}

// independent divisions by (X - pt), one block each
static int dev_kate_div(Ctx* c, ProverDev& pd, const std::vector<KateJob>& jobs) {
  if (jobs.empty()) return 0;
  KateJob* dj = (KateJob*)pdev_stage(c, pd, jobs.size() * sizeof(KateJob));
  if (!dj) return TG_ERR_NOMEM;
  hipMemcpyAsync(dj, jobs.data(), jobs.size() * sizeof(KateJob), hipMemcpyHostToDevice,
                 c->stream);
  hipLaunchKernelGGL(k_kate_div, dim3((unsigned)jobs.size()), dim3(OPN_T), 0, c->stream,
                     (const KateJob*)dj);
  return 0;
}

// ---------------- grand-product launchers (kernels: grand_products.hip) ----
// Same conventions as the opening-phase launchers above. The host copies of
// the tables live in pd, so they outlive the stream's next synchronisation.

static_assert(GP_MAX_COLS == TG_MAX_PERM && GP_MAX_CHUNKS == TG_MAX_CHUNKS &&
                  GP_MAX_LOOKUPS == TG_MAX_LOOKUPS,
              "grand_products.hip tables and the pdesc_parse limits disagree");

// rows a thread of the term kernels walks
constexpr int GP_TERM_ROWS = 4;
static inline unsigned gp_term_grid(long u) {
  long per = (long)GP_B * GP_TERM_ROWS;
  return (unsigned)std::max<long>(1, (u + per - 1) / per);
}

// d_num / d_den [ch * u + i], i < u, for every chunk of chunk_len columns
static int dev_gp_perm_terms(Ctx* c, ProverDev& pd, const std::vector<const Fp*>& cols,
                             const std::vector<const Fp*>& sigmas, int chunk_len, long u,
                             const Fp& beta, const Fp& gamma, const Fp& omega,
                             const Fp& delta, Fp* d_num, Fp* d_den) {
  int n_perm = (int)cols.size();
  if (n_perm < 1 || n_perm > GP_MAX_COLS || sigmas.size() != cols.size() ||
      chunk_len < 1 || u < 1)
    return TG_ERR_BADARG;
  int nchunks = (n_perm + chunk_len - 1) / chunk_len;
  if (nchunks > GP_MAX_CHUNKS) return TG_ERR_BADARG;
  GpPermArgs& A = pd.gp_perm_h;
  A = GpPermArgs{};
  Fp bd = beta;
  for (int j = 0; j < n_perm; j++) {
    A.cols[j] = cols[j];
    A.sigma[j] = sigmas[j];
    A.bdpow[j] = bd;
    bd = fd_mul(bd, delta);
  }
  A.beta = beta;
  A.gamma = gamma;
  A.omega = omega;
  A.num = d_num;
  A.den = d_den;
  A.u = u;
  A.n_perm = n_perm;
  A.chunk_len = chunk_len;
  GpPermArgs* dA = (GpPermArgs*)pdev_stage(c, pd, sizeof(GpPermArgs));
  if (!dA) return TG_ERR_NOMEM;
  hipMemcpyAsync(dA, &A, sizeof(GpPermArgs), hipMemcpyHostToDevice, c->stream);
  ProfScope ps(c, P_GP_TERMS);
  hipLaunchKernelGGL(k_gp_perm_terms, dim3(gp_term_grid(u), (unsigned)nchunks), dim3(GP_B),
                     0, c->stream, (const GpPermArgs*)dA);
  return 0;
}

// d_num / d_den [l * u + i], i < u, for every lookup
static int dev_gp_lookup_terms(Ctx* c, ProverDev& pd, int nlk, const Fp* const* a,
                               const Fp* const* s, const Fp* const* ap,
                               const Fp* const* sp, long u, const Fp& beta,
                               const Fp& gamma, Fp* d_num, Fp* d_den) {
  if (nlk < 1 || nlk > GP_MAX_LOOKUPS || u < 1) return TG_ERR_BADARG;
  GpLookupArgs& A = pd.gp_lk_h;
  A = GpLookupArgs{};
  for (int l = 0; l < nlk; l++) {
    A.a[l] = a[l];
    A.s[l] = s[l];
    A.ap[l] = ap[l];
    A.sp[l] = sp[l];
  }
  A.beta = beta;
  A.gamma = gamma;
  A.num = d_num;
  A.den = d_den;
  A.u = u;
  GpLookupArgs* dA = (GpLookupArgs*)pdev_stage(c, pd, sizeof(GpLookupArgs));
  if (!dA) return TG_ERR_NOMEM;
  hipMemcpyAsync(dA, &A, sizeof(GpLookupArgs), hipMemcpyHostToDevice, c->stream);
  ProfScope ps(c, P_GP_TERMS);
  hipLaunchKernelGGL(k_gp_lookup_terms, dim3(gp_term_grid(u), (unsigned)nlk), dim3(GP_B), 0,
                     c->stream, (const GpLookupArgs*)dA);
  return 0;
}

// d_v[i] <- d_v[i]^-1, i < count, zeros staying zero: one launch
static int dev_gp_batch_inverse(Ctx* c, Fp* d_v, long count) {
  if (count < 1 || gp_blocks_for(count) > 0x7fffffffL) return TG_ERR_BADARG;
  ProfScope ps(c, P_GP_INVERSE);
  hipLaunchKernelGGL(k_gp_batch_inverse, dim3((unsigned)gp_blocks_for(count)), dim3(GP_B), 0,
                     c->stream, d_v, count);
  return 0;
}

// one segment of the chained prefix product: len ratios, len + 1 values
// written to d_dst. A chained segment starts from the value the previous
// segment ended with, any other from init.
struct GpSeg {
  long len;
  Fp* d_dst;
  bool chained;
  Fp init;
};

// z_s[0] = start value, z_s[i+1] = z_s[i] * ratio_s[i] for every segment;
// the ratios are d_a[i] * d_b[i] (d_b may be null) over the concatenation
// of the segments. Three launches whatever the number of segments; the
// chaining values stay on the device.
static int dev_gp_scan(Ctx* c, ProverDev& pd, const Fp* d_a, const Fp* d_b,
                       const std::vector<GpSeg>& segs) {
  if (segs.empty()) return TG_ERR_BADARG;
  std::vector<GpScanBlock> blocks;
  std::vector<GpScanChain> chains;
  long flat = 0;
  for (size_t s = 0; s < segs.size(); s++) {
    const GpSeg& sg = segs[s];
    if (sg.len < 1) return TG_ERR_BADARG;
    if (s == 0 || !sg.chained)
      chains.push_back(GpScanChain{sg.init, (int)blocks.size(), (int)blocks.size()});
    for (long o = 0; o < sg.len; o += GP_T) {
      int len = (int)std::min<long>(GP_T, sg.len - o);
      blocks.push_back(GpScanBlock{flat + o, sg.d_dst + o, len, o + len == sg.len ? 1 : 0});
    }
    if (blocks.size() > 0x3fffffff) return TG_ERR_BADARG;
    chains.back().blk_hi = (int)blocks.size();
    flat += sg.len;
  }
  size_t nb = blocks.size(), bbytes = nb * sizeof(GpScanBlock);
  size_t cbytes = chains.size() * sizeof(GpScanChain);
  pd.gp_scan_h.resize(bbytes + cbytes);
  memcpy(pd.gp_scan_h.data(), blocks.data(), bbytes);
  memcpy(pd.gp_scan_h.data() + bbytes, chains.data(), cbytes);
  uint8_t* dt = (uint8_t*)pdev_stage(c, pd, bbytes + cbytes);
  Fp* d_bp = pdev_small(c, pd, 2 * nb);
  if (!dt || !d_bp) return TG_ERR_NOMEM;
  Fp* d_off = d_bp + nb;
  hipMemcpyAsync(dt, pd.gp_scan_h.data(), bbytes + cbytes, hipMemcpyHostToDevice,
                 c->stream);
  const GpScanBlock* dblk = (const GpScanBlock*)dt;
  const GpScanChain* dch = (const GpScanChain*)(dt + bbytes);
  ProfScope ps(c, P_GP_SCAN);
  hipLaunchKernelGGL(k_gp_scan_reduce, dim3((unsigned)nb), dim3(GP_B), 0, c->stream, dblk,
                     d_a, d_b, d_bp);
  hipLaunchKernelGGL(k_gp_scan_offsets, dim3((unsigned)chains.size()), dim3(GP_B), 0,
                     c->stream, dch, (const Fp*)d_bp, d_off);
  hipLaunchKernelGGL(k_gp_scan_apply, dim3((unsigned)nb), dim3(GP_B), 0, c->stream, dblk,
                     d_a, d_b, (const Fp*)d_off);
  return 0;
}

// ---------------- lookup-argument launchers (kernels: lookup_argument.hip) --
// Same conventions again. Everything is enqueued on the context's stream.

static_assert(LK_MAX_LOOKUPS == TG_MAX_LOOKUPS,
              "lookup_argument.hip tables and the pdesc_parse limits disagree");
// largest array the sort and the 32-bit ranks are sized for
constexpr long LK_MAX_U = 1L << 24;
static_assert(TG_MAX_K <= 24, "LK_MAX_U must cover every key's row count");

// d_dst[a] <- the ascending canonical sort of d_src[a][0..u) (Montgomery
// form) padded to np keys with the all-ones key; np is a power of two >= u
// and d_dst[a] is np long; no source is a destination. All arrays go through
// the same lk_sort_launches(np) launches.
static int dev_lk_sort(Ctx* c, int narr, const Fp* const* d_src, Fp* const* d_dst, long u,
                       long np) {
  if (narr < 1 || narr > LK_MAX_ARRAYS || u < 1 || np < u || np > LK_MAX_U ||
      (np & (np - 1)) != 0)
    return TG_ERR_BADARG;
  LkSortArgs A{};
  for (int a = 0; a < narr; a++) {
    A.src[a] = d_src[a];
    A.dst[a] = d_dst[a];
  }
  A.u = u;
  A.np = np;
  const long tl = lk_tile_len(np);
  const dim3 tiles((unsigned)lk_tiles(np), (unsigned)narr);
  ProfScope ps(c, P_LK_SORT);
  hipLaunchKernelGGL(k_lk_sort_tile, tiles, dim3(LK_B), 0, c->stream, A);
  for (long k = 2 * tl; k <= np; k <<= 1) {
    for (long j = k / 2; j >= tl; j >>= 1)
      hipLaunchKernelGGL(k_lk_sort_global, dim3((unsigned)lk_stage_blocks(np), (unsigned)narr),
                         dim3(LK_B), 0, c->stream, A, k, j);
    hipLaunchKernelGGL(k_lk_sort_merge, tiles, dim3(LK_B), 0, c->stream, A, k);
  }
  return 0;
}

// For every lookup: d_ap[l] holds the sorted canonical A' and d_t[l] the
// sorted canonical table (dev_lk_sort output), u rows each. Writes S' to
// d_sp[l] and turns d_ap[l] into Montgomery form, rows < u. An input value
// that the table lacks sets the device error word; dev_lk_fetch_err brings
// it to pd.lk_err_h, valid after the caller's next stream synchronisation.
static int dev_lk_permute(Ctx* c, ProverDev& pd, int nlk, Fp* const* d_ap,
                          const Fp* const* d_t, Fp* const* d_sp, long u) {
  if (nlk < 1 || nlk > LK_MAX_LOOKUPS || u < 1 || u > LK_MAX_U) return TG_ERR_BADARG;
  const size_t m = (size_t)2 * nlk * u;  // flat flags: first[], taken[] per lookup
  const size_t nb1 = (m + 511) / 512, nb2 = (nb1 + 511) / 512;
  // error word (padded to 4 words) | flags | scan | lpos | block sums
  const size_t need = 4 + 2 * m + (size_t)nlk * u + nb1 + nb2;
  uint32_t* ws = pdev_grow(c, pd.lk_ws, pd.lk_ws_cap, need);
  if (!ws) return TG_ERR_NOMEM;
  LkPermArgs A{};
  for (int l = 0; l < nlk; l++) {
    A.ap[l] = d_ap[l];
    A.t[l] = d_t[l];
    A.sp[l] = d_sp[l];
  }
  A.err = ws;
  A.flags = ws + 4;
  A.scan = A.flags + m;
  A.lpos = A.scan + m;
  uint32_t* bsum = A.lpos + (size_t)nlk * u;
  A.u = u;
  const dim3 grid((unsigned)lk_row_blocks(u), (unsigned)nlk);
  ProfScope ps(c, P_LK_PERMUTE);
  // clears the error word for this proof and the taken[] flags
  hipMemsetAsync(ws, 0, (4 + m) * sizeof(uint32_t), c->stream);
  hipLaunchKernelGGL(k_lk_first, grid, dim3(LK_B), 0, c->stream, A);
  msm_scan(A.flags, A.scan, bsum, (u64)m, c->stream);
  hipLaunchKernelGGL(k_lk_leftover, grid, dim3(LK_B), 0, c->stream, A);
  hipLaunchKernelGGL(k_lk_write, grid, dim3(LK_B), 0, c->stream, A);
  return 0;
}

static void dev_lk_fetch_err(Ctx* c, ProverDev& pd) {
  hipMemcpyAsync(&pd.lk_err_h, pd.lk_ws, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
}

// The IPA rounds over the first 2^k bases of d_g, on device vectors d_pp
// (the polynomial), d_bvec (powers of the opening point) and d_wfold (ones
// on entry), all 2^k long and folded in place. L_j / R_j are MSMs over the
// ORIGINAL bases with folded scalar vectors (wfold tracks the g-fold
// coefficients) instead of folding the point vector itself — the group
// elements are identical. Per round the host only draws the two blinds
// (draw), adds the U / W terms, and hands L, R to emit, which returns the
// round challenge. Returns pp[0] in a_out; blind_acc is updated in place.
// lap(0) / lap(1) close a host / MSM span for the caller's stage timing.
template <class DrawFn, class EmitFn, class LapFn>
static int ipa_rounds_dev(Ctx* c, ProverDev& pd, int k, Fp* d_pp, Fp* d_bvec, Fp* d_wfold,
                          const FixedMulTab& utab, const FixedMulTab& wtab, Fp& blind_acc,
                          Fp& a_out, DrawFn&& draw, EmitFn&& emit, LapFn&& lap) {
  long n = 1L << k;
  int rc = gpu_msm_reserve(c, n, 2);
  if (rc) return rc;
  Fp* d_part = pdev_small(c, pd, 2 * OPN_GRID_MAX);
  if (!d_part) return TG_ERR_NOMEM;
  int grid = opn_grid(n);
  std::vector<Fp> part(2 * (size_t)grid);
  long half = n >> 1;
  for (int round = 0; round < k; round++, half >>= 1) {
    Fp l_rand, r_rand;
    draw(l_rand, r_rand);
    hipLaunchKernelGGL(k_ipa_prepare, dim3(grid), dim3(256), 0, c->stream,
                       (const Fp*)d_pp, (const Fp*)d_bvec, (const Fp*)d_wfold, n, half,
                       (Fp*)c->d_scalars, d_part);
    hipMemcpyAsync(part.data(), d_part, part.size() * sizeof(Fp), hipMemcpyDeviceToHost,
                   c->stream);
    lap(0);
    VestaAff LR[2];
    Fp zeros[2] = {fd_zero<FpCfg>(), fd_zero<FpCfg>()};
    if ((rc = gpu_msm_commit_canon(c, n, 2, c->d_g, zeros, LR, &wtab))) return rc;
    lap(1);
    Fp value_l = fd_zero<FpCfg>(), value_r = fd_zero<FpCfg>();
    for (int b = 0; b < grid; b++) {
      value_l = fd_add(value_l, part[2 * b]);
      value_r = fd_add(value_r, part[2 * b + 1]);
    }
    VestaJac Lj = jac_from_aff(LR[0]), Rj = jac_from_aff(LR[1]);
    Lj = jac_add(Lj, utab.mul(value_l));
    Lj = jac_add(Lj, wtab.mul(l_rand));
    Rj = jac_add(Rj, utab.mul(value_r));
    Rj = jac_add(Rj, wtab.mul(r_rand));
    Fp uch;
    if ((rc = emit(jac_to_aff(Lj), jac_to_aff(Rj), uch))) return rc;
    Fp uch_inv = fd_inv(uch);
    long topbit = (long)1 << (k - 1 - round);
    hipLaunchKernelGGL(k_ipa_fold, dim3(grid), dim3(256), 0, c->stream, d_pp, d_bvec,
                       d_wfold, n, half, topbit, uch, uch_inv);
    blind_acc = fd_add(blind_acc, fd_mul(uch, l_rand));
    blind_acc = fd_add(blind_acc, fd_mul(uch_inv, r_rand));
    lap(0);
  }
  hipMemcpyAsync(&a_out, d_pp, sizeof(Fp), hipMemcpyDeviceToHost, c->stream);
  return hipStreamSynchronize(c->stream) == hipSuccess ? 0 : TG_ERR_HIP;
}

// single-MSM wrapper (keygen-time calls before the W table exists pass
// wtab = nullptr and fall back to the generic host scalar mult)
static int gpu_msm_commit(Ctx* c, ProverDev& pd, const Fp* mont_scalars, long nn,
                          const VestaAff* d_bases, const Fp& blind, const VestaAff& Wp,
                          VestaAff& out, const FixedMulTab* wtab = nullptr) {
  if (wtab) return gpu_msm_commit_batch(c, pd, mont_scalars, nn, 1, d_bases, &blind,
                                        &out, wtab);
  Fp zero = fd_zero<FpCfg>();
  int rc = gpu_msm_commit_batch(c, pd, mont_scalars, nn, 1, d_bases, &zero, &out,
                                nullptr);
  if (rc) return rc;
  if (!fd_is_zero(blind)) {
    VestaJac acc = jac_from_aff(out);
    acc = jac_add(acc, jac_mul_host(jac_from_aff(Wp), blind));
    out = jac_to_aff(acc);
  }
  return 0;
}


// ---------------- device h-fold (quotient evaluation on the ext coset) ----
// The TGD1 postfix expressions have stack depth <= TG_MAX_STACK (pdesc_parse
// checks it); the device interpreter keeps the stack in that many named
// registers s0..s7 (runtime-indexed arrays would go to scratch — guide rule).

struct DevExpr {
  int off, len;
};

// device-side extra op tag: query-cache reference (rewritten at keygen
// from XFIXED/XADVICE/XINSTANCE — the h-fold kernel preloads every
// distinct (column, rotation) value once per row instead of re-gathering
// it per expression op; bit-exact, pure evaluation optimization)
constexpr uint32_t XQUERY = 9;
struct DevQuery {
  int kind;  // 0 fixed, 1 advice, 2 instance
  int col;
  int rot;
};
constexpr int HF_MAX_Q = TG_MAX_QUERIES;
static_assert(TG_MAX_STACK == 8, "DSTK_* keep the stack in registers s0..s7");

struct HFoldArgs {
  long ext_n, rs;
  int n_gates, n_perm, chunk_len, nlk, nchunks, last_rot, n_consts;
  Fp beta, gamma, y, theta;
  const Fp *x_ext, *l0, *llast, *lactive, *t_inv;
  const ExprOp* ops;
  const Fp* consts;
  // every array below is sized by the limit pdesc_parse enforces
  DevExpr gates[TG_MAX_GATES];
  int lk_nin[TG_MAX_LOOKUPS], lk_ntab[TG_MAX_LOOKUPS];
  DevExpr lk_in[TG_MAX_LOOKUPS][TG_MAX_LK_EXPRS], lk_tab[TG_MAX_LOOKUPS][TG_MAX_LK_EXPRS];
  const Fp* fixed_cols[TG_MAX_FIXED];
  const Fp* advice_cols[TG_MAX_ADVICE];
  const Fp* inst_cols[TG_MAX_INSTANCE];
  const Fp* sigma[TG_MAX_PERM];
  int perm_kind[TG_MAX_PERM], perm_idx[TG_MAX_PERM];
  Fp dpow[TG_MAX_PERM];
  const Fp* zp[TG_MAX_CHUNKS];
  const Fp* lkz[TG_MAX_LOOKUPS];
  const Fp* lkap[TG_MAX_LOOKUPS];
  const Fp* lksp[TG_MAX_LOOKUPS];
  Fp* out;
  const DevQuery* queries;  // combined [fixed_q..., advice_q..., instance_q...]
  int n_queries;
  const Fp* acc_init;  // pre-folded gate accumulator (RTC path), or null
};
#define HF_CAP(field, cap)                                                    \
  static_assert(sizeof(HFoldArgs::field) / sizeof(((HFoldArgs*)0)->field[0]) == \
                    (size_t)(cap),                                              \
                "HFoldArgs::" #field " and its pdesc_parse guard disagree")
HF_CAP(gates, TG_MAX_GATES);
HF_CAP(fixed_cols, TG_MAX_FIXED);
HF_CAP(advice_cols, TG_MAX_ADVICE);
HF_CAP(inst_cols, TG_MAX_INSTANCE);
HF_CAP(sigma, TG_MAX_PERM);
HF_CAP(dpow, TG_MAX_PERM);
HF_CAP(zp, TG_MAX_CHUNKS);
HF_CAP(lkz, TG_MAX_LOOKUPS);
HF_CAP(lk_in, TG_MAX_LOOKUPS);
HF_CAP(lk_in[0], TG_MAX_LK_EXPRS);
HF_CAP(lk_tab[0], TG_MAX_LK_EXPRS);
#undef HF_CAP

#define DSTK_PUSH(v)                                   \
  do {                                                 \
    Fp _v = (v);                                       \
    switch (sp) {                                      \
      case 0: s0 = _v; break;                          \
      case 1: s1 = _v; break;                          \
      case 2: s2 = _v; break;                          \
      case 3: s3 = _v; break;                          \
      case 4: s4 = _v; break;                          \
      case 5: s5 = _v; break;                          \
      case 6: s6 = _v; break;                          \
      default: s7 = _v; break;                         \
    }                                                  \
    sp++;                                              \
  } while (0)

#define DSTK_BIN(OPFN)                                 \
  do {                                                 \
    switch (sp) {                                      \
      case 2: s0 = OPFN(s0, s1); break;                \
      case 3: s1 = OPFN(s1, s2); break;                \
      case 4: s2 = OPFN(s2, s3); break;                \
      case 5: s3 = OPFN(s3, s4); break;                \
      case 6: s4 = OPFN(s4, s5); break;                \
      case 7: s5 = OPFN(s5, s6); break;                \
      default: s6 = OPFN(s6, s7); break;               \
    }                                                  \
    sp--;                                              \
  } while (0)

#define DSTK_UN(OPFN)                                  \
  do {                                                 \
    switch (sp) {                                      \
      case 1: s0 = OPFN(s0); break;                    \
      case 2: s1 = OPFN(s1); break;                    \
      case 3: s2 = OPFN(s2); break;                    \
      case 4: s3 = OPFN(s3); break;                    \
      case 5: s4 = OPFN(s4); break;                    \
      case 6: s5 = OPFN(s5); break;                    \
      case 7: s6 = OPFN(s6); break;                    \
      default: s7 = OPFN(s7); break;                   \
    }                                                  \
  } while (0)

#define DSTK_SCALE(C)                                  \
  do {                                                 \
    switch (sp) {                                      \
      case 1: s0 = fd_mul(s0, (C)); break;             \
      case 2: s1 = fd_mul(s1, (C)); break;             \
      case 3: s2 = fd_mul(s2, (C)); break;             \
      case 4: s3 = fd_mul(s3, (C)); break;             \
      case 5: s4 = fd_mul(s4, (C)); break;             \
      case 6: s5 = fd_mul(s5, (C)); break;             \
      case 7: s6 = fd_mul(s6, (C)); break;             \
      default: s7 = fd_mul(s7, (C)); break;            \
    }                                                  \
  } while (0)

__device__ __forceinline__ Fp dev_expr_eval(const HFoldArgs& A, const DevExpr& e,
                                            long row, const Fp* qv) {
  Fp s0, s1, s2, s3, s4, s5, s6, s7;
  int sp = 0;
  for (int oi = 0; oi < e.len; oi++) {
    ExprOp op = A.ops[e.off + oi];
    switch (op.tag) {
      case XCONST: DSTK_PUSH(A.consts[op.a]); break;
      case XQUERY: DSTK_PUSH(qv[op.a]); break;
      case XFIXED:
      case XADVICE:
      case XINSTANCE: {
        long r = (row + (long)op.b * A.rs) & (A.ext_n - 1);
        const Fp* col = op.tag == XFIXED ? A.fixed_cols[op.a]
                        : op.tag == XADVICE ? A.advice_cols[op.a] : A.inst_cols[op.a];
        DSTK_PUSH(col[r]);
        break;
      }
      case XADD: DSTK_BIN(fd_add); break;
      case XSUB: DSTK_BIN(fd_sub); break;
      case XMUL: DSTK_BIN(fd_mul); break;
      case XNEG:
        DSTK_UN(fd_neg);
        break;
      case XSCALE:
        DSTK_SCALE(A.consts[op.a]);
        break;
    }
  }
  return s0;
}

__global__ void __launch_bounds__(256, 1) k_h_fold(const HFoldArgs* __restrict__ Ap) {
  const HFoldArgs& A = *Ap;
  Fp one = fd_one_mont<FpCfg>();
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < A.ext_n;
       i += (long)gridDim.x * blockDim.x) {
    // preload every queried (column, rotation) value once for this row
    Fp qv[HF_MAX_Q];
    for (int q = 0; q < A.n_queries; q++) {
      DevQuery dq = A.queries[q];
      long r = (i + (long)dq.rot * A.rs) & (A.ext_n - 1);
      const Fp* col = dq.kind == 0 ? A.fixed_cols[dq.col]
                      : dq.kind == 1 ? A.advice_cols[dq.col] : A.inst_cols[dq.col];
      qv[q] = col[r];
    }
    Fp acc = A.acc_init ? A.acc_init[i] : fd_zero<FpCfg>();
    auto yf = [&](const Fp& v) { acc = fd_add(fd_mul(acc, A.y), v); };
    // gates (skipped when the RTC kernel pre-folded them into acc_init)
    for (int g = 0; g < A.n_gates; g++) yf(dev_expr_eval(A, A.gates[g], i, qv));
    long nexti = (i + A.rs) & (A.ext_n - 1);
    long lasti = (i + (long)A.last_rot * A.rs) & (A.ext_n - 1);
    // permutation
    yf(fd_mul(fd_sub(one, A.zp[0][i]), A.l0[i]));
    {
      Fp zl = A.zp[A.nchunks - 1][i];
      yf(fd_mul(fd_sub(fd_sqr(zl), zl), A.llast[i]));
    }
    for (int ch = 1; ch < A.nchunks; ch++)
      yf(fd_mul(fd_sub(A.zp[ch][i], A.zp[ch - 1][lasti]), A.l0[i]));
    for (int ch = 0; ch < A.nchunks; ch++) {
      int lo = ch * A.chunk_len;
      int hi = lo + A.chunk_len;
      if (hi > A.n_perm) hi = A.n_perm;
      Fp left = A.zp[ch][nexti];
      Fp right = A.zp[ch][i];
      for (int jj = lo; jj < hi; jj++) {
        const Fp* col = A.perm_kind[jj] == 0 ? A.advice_cols[A.perm_idx[jj]]
                        : A.perm_kind[jj] == 1 ? A.fixed_cols[A.perm_idx[jj]]
                                               : A.inst_cols[A.perm_idx[jj]];
        Fp v = col[i];
        left = fd_mul(left, fd_add(fd_add(fd_mul(A.beta, A.sigma[jj][i]), v), A.gamma));
        right = fd_mul(
            right, fd_add(fd_add(fd_mul(fd_mul(A.dpow[jj], A.x_ext[i]), A.beta), v),
                          A.gamma));
      }
      yf(fd_mul(fd_sub(left, right), A.lactive[i]));
    }
    // lookups
    long previ = (i - A.rs) & (A.ext_n - 1);
    for (int l = 0; l < A.nlk; l++) {
      Fp z = A.lkz[l][i], zn = A.lkz[l][nexti];
      Fp ap = A.lkap[l][i], apv = A.lkap[l][previ], spv = A.lksp[l][i];
      Fp acomp = fd_zero<FpCfg>();
      for (int e = 0; e < A.lk_nin[l]; e++)
        acomp = fd_add(fd_mul(acomp, A.theta), dev_expr_eval(A, A.lk_in[l][e], i, qv));
      Fp scomp = fd_zero<FpCfg>();
      for (int e = 0; e < A.lk_ntab[l]; e++)
        scomp = fd_add(fd_mul(scomp, A.theta), dev_expr_eval(A, A.lk_tab[l][e], i, qv));
      yf(fd_mul(fd_sub(one, z), A.l0[i]));
      yf(fd_mul(fd_sub(fd_sqr(z), z), A.llast[i]));
      Fp left = fd_mul(fd_mul(zn, fd_add(ap, A.beta)), fd_add(spv, A.gamma));
      Fp right = fd_mul(fd_mul(z, fd_add(acomp, A.beta)), fd_add(scomp, A.gamma));
      yf(fd_mul(fd_sub(left, right), A.lactive[i]));
      yf(fd_mul(fd_sub(ap, spv), A.l0[i]));
      yf(fd_mul(fd_mul(fd_sub(ap, spv), fd_sub(ap, apv)), A.lactive[i]));
    }
    A.out[i] = fd_mul(acc, A.t_inv[i]);
  }
}

// ---------------- lookup compress (Lagrange rows) ----------------
// The compressed input and table expressions of every lookup over the usable
// rows, through the same flattened programs and register stack as the h-fold.
// The argument block is an HFoldArgs whose columns are the Lagrange pool
// slots: rotation stride rs = 1 and mask ext_n - 1 = n - 1, and only the
// first n_queries = h_nq_lk queries (the ones lookups use) are preloaded.
// theta changes per proof and is a kernel argument; the block is per key.

struct LkCompressOut {
  Fp* a[TG_MAX_LOOKUPS];
  Fp* s[TG_MAX_LOOKUPS];
};

// a[l][i], s[l][i] = Horner in theta over lookup l's input / table
// expressions at row i < u; rows >= u are never read and stay as they are
__global__ void __launch_bounds__(256) k_lk_compress(const HFoldArgs* __restrict__ Ap, Fp theta,
                                                     long u, LkCompressOut out) {
  const HFoldArgs& A = *Ap;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < u;
       i += (long)gridDim.x * blockDim.x) {
    Fp qv[HF_MAX_Q];
    for (int q = 0; q < A.n_queries; q++) {
      DevQuery dq = A.queries[q];
      long r = (i + (long)dq.rot * A.rs) & (A.ext_n - 1);
      const Fp* col = dq.kind == 0 ? A.fixed_cols[dq.col]
                      : dq.kind == 1 ? A.advice_cols[dq.col] : A.inst_cols[dq.col];
      qv[q] = col[r];
    }
    for (int l = 0; l < A.nlk; l++) {
      Fp acomp = fd_zero<FpCfg>();
      for (int e = 0; e < A.lk_nin[l]; e++)
        acomp = fd_add(fd_mul(acomp, theta), dev_expr_eval(A, A.lk_in[l][e], i, qv));
      Fp scomp = fd_zero<FpCfg>();
      for (int e = 0; e < A.lk_ntab[l]; e++)
        scomp = fd_add(fd_mul(scomp, theta), dev_expr_eval(A, A.lk_tab[l][e], i, qv));
      out.a[l][i] = acomp;
      out.s[l][i] = scomp;
    }
  }
}


// ---------------- product proving key ----------------

struct PPk {
  PDesc d;
  Fp omega, omega_inv, zeta, zeta_inv, delta, n_inv, ext_n_inv;
  std::vector<std::vector<Fp>> fixed_ext;
  std::vector<std::vector<Fp>> sigma_lag, sigma_ext;
  std::vector<Fp> l0_ext, llast_ext, lactive_ext, t_inv_ext, x_ext;
  Fp vk_repr;
  std::vector<VestaAff> sigma_commits, fixed_commits;
  FixedMulTab wtab, utab;  // fast [s]W / [s]U (blinds, IPA inner-product terms)
  // device-resident h-fold inputs (uploaded once at keygen)
  std::vector<Fp*> d_fixed_ext, d_sigma_ext;
  // coefficient form of the fixed and sigma polynomials (n each), read by
  // the opening phase on the device
  std::vector<Fp*> d_fixed_coeff, d_sigma_coeff;
  Fp *d_l0 = nullptr, *d_llast = nullptr, *d_lactive = nullptr, *d_tinv = nullptr,
     *d_xext = nullptr;
  ExprOp* d_ops = nullptr;
  Fp* d_consts = nullptr;
  std::vector<DevQuery> h_queries;
  int h_nq_lk = 0;  // prefix of h_queries referenced by lookup exprs
  DevQuery* d_queries = nullptr;
  HfRtcKernel* rtc = nullptr;  // runtime-specialized gate evaluation (hf_rtc.hpp)
  Fp** d_colptrs = nullptr;    // column pointer table for the RTC kernel
  std::vector<DevExpr> gate_de;                  // per gate
  std::vector<std::vector<DevExpr>> lk_in_de, lk_tab_de;
  ProverDev pd;
  TgwProgram tgw;  // attached witness-synthesis program (witness.hpp)
  bool ready = false;
};

// Slot numbers of the Lagrange pool (pd.lag), from the descriptor alone:
//   sigma columns | fixed columns of the permutation and of the
//                   lookup expressions, one slot each         (once per key)
//   advice | instance | z (chunks, then lookups)              (per proof)
//   per lookup A', S', A, S | flat num | flat den
//   per lookup the sorted table (scratch of the A' / S' construction)
// n_perm + (fixed columns used) + n_advice + 1 + 3 * nz + 5 * n_lookups
// slots in all. The advice slots, the z slots and each A', S' pair are
// contiguous: a batched commit reads them as one concatenation.
struct LagLayout {
  int sigma = 0, fixed = 0, adv = 0, inst = 0, z = 0, lk = 0, num = 0, den = 0, lkt = 0,
      total = 0;
  int nz = 0;
  // per fixed column, -1 if neither permuted nor queried by a lookup
  std::vector<int> fixed_slot;
  explicit LagLayout(const PDesc& d) {
    int nchunks = (d.n_perm + d.chunk_len - 1) / d.chunk_len;
    nz = nchunks + d.n_lookups;
    fixed = sigma + d.n_perm;
    fixed_slot.assign(d.n_fixed, -1);
    int nfp = 0;
    for (int j = 0; j < d.n_perm; j++) {
      auto [kind, idx] = d.perm_cols[j];
      if (kind == 1 && fixed_slot[idx] < 0) fixed_slot[idx] = fixed + nfp++;
    }
    auto lookup_fixed = [&](const PExpr& e) {
      for (const auto& op : e.ops)
        if (op.tag == XFIXED && fixed_slot[op.a] < 0) fixed_slot[op.a] = fixed + nfp++;
    };
    for (const auto& lk_ : d.lookups) {
      for (const auto& e : lk_.in) lookup_fixed(e);
      for (const auto& e : lk_.tab) lookup_fixed(e);
    }
    adv = fixed + nfp;
    inst = adv + d.n_advice;
    z = inst + 1;
    lk = z + nz;
    num = lk + 4 * d.n_lookups;
    den = num + nz;
    lkt = den + nz;
    total = lkt + d.n_lookups;
  }
};

static Fp host_domain_omega(int k, bool inverse) {
  Fp root;
#pragma unroll
  for (int i = 0; i < 4; i++) root.l[i] = inverse ? FpCfg::ROOT_INV[i] : FpCfg::ROOT[i];
  Fp w = fd_to_mont(root);
  for (int i = k; i < 32; i++) w = fd_sqr(w);
  return w;
}

static int ppk_keygen(Ctx* c, PPk& pk, const uint8_t* desc, size_t desc_len) {
  if (!pdesc_parse(pk.d, desc, desc_len)) return TG_ERR_BADARG;
  PDesc& d = pk.d;
  if (c->k != d.k) return TG_ERR_NOSRS;
  long n = d.n, ext_n = d.ext_n;
  hipError_t e = pdev_init(c, pk.pd, d.k, d.ext_k);
  if (e != hipSuccess) return TG_ERR_NOMEM;
  pk.omega = host_domain_omega(d.k, false);
  pk.omega_inv = host_domain_omega(d.k, true);
  Fp ext_omega = host_domain_omega(d.ext_k, false);
  // zeta = 5^((p-1)/3)
  {
    Fp five{{5, 0, 0, 0}};
    five = fd_to_mont(five);
    u64 mod1[4], ee[4];
    u64 borrow = 0;
    for (int i = 0; i < 4; i++) {
      u128 dd = (u128)FpCfg::MOD[i] - (i == 0 ? 1 : 0) - borrow;
      mod1[i] = (u64)dd;
      borrow = (u64)(dd >> 64) ? 1 : 0;
    }
    u128 rem = 0;
    for (int i = 3; i >= 0; i--) {
      u128 cur = (rem << 64) | mod1[i];
      ee[i] = (u64)(cur / 3);
      rem = cur % 3;
    }
    pk.zeta = fd_pow(five, ee);
    pk.zeta_inv = fd_inv(pk.zeta);
    pk.delta = five;
    for (int i = 0; i < 32; i++) pk.delta = fd_sqr(pk.delta);
  }
  {
    Fp nl{{(u64)n, 0, 0, 0}};
    pk.n_inv = fd_inv(fd_to_mont(nl));
    Fp el{{(u64)ext_n, 0, 0, 0}};
    pk.ext_n_inv = fd_inv(fd_to_mont(el));
  }
  // x_ext
  pk.x_ext.resize(ext_n);
  pk.x_ext[0] = pk.zeta;
  for (long i = 1; i < ext_n; i++) pk.x_ext[i] = fd_mul(pk.x_ext[i - 1], ext_omega);
  // t_inv_ext
  pk.t_inv_ext.resize(ext_n);
  {
    long period = ext_n / n;
    Fp zeta_n = fd_one_mont<FpCfg>();
    for (long i = 0; i < n % 3; i++) zeta_n = fd_mul(zeta_n, pk.zeta);
    Fp mu = ext_omega;
    for (int i = 0; i < d.k; i++) mu = fd_sqr(mu);
    Fp one = fd_one_mont<FpCfg>();
    Fp cur = zeta_n;
    for (long i = 0; i < period; i++) {
      Fp t = fd_inv(fd_sub(cur, one));
      for (long j = i; j < ext_n; j += period) pk.t_inv_ext[j] = t;
      cur = fd_mul(cur, mu);
    }
  }
  // coefficient form -> the key's device copy (gpu_lag_to_coeff leaves it
  // in ws0 as well as on the host)
  auto keep_coeff = [&](Fp*& dst) -> int {
    if (hipMalloc(&dst, n * sizeof(Fp)) != hipSuccess) return TG_ERR_NOMEM;
    hipMemcpyAsync(dst, pk.pd.ws0, n * sizeof(Fp), hipMemcpyDeviceToDevice, c->stream);
    return 0;
  };
  // fixed transforms (GPU)
  pk.fixed_ext.resize(d.n_fixed);
  pk.d_fixed_coeff.assign(d.n_fixed, nullptr);
  for (int col = 0; col < d.n_fixed; col++) {
    std::vector<Fp> coeff = d.fixed_lag[col];
    if (gpu_lag_to_coeff(c, pk.pd, coeff.data(), d.k, pk.n_inv)) return TG_ERR_HIP;
    if (keep_coeff(pk.d_fixed_coeff[col])) return TG_ERR_NOMEM;
    pk.fixed_ext[col].resize(ext_n);
    if (gpu_coeff_to_ext(c, pk.pd, coeff.data(), pk.fixed_ext[col].data(), d.k, d.ext_k,
                         pk.zeta))
      return TG_ERR_HIP;
  }
  // sigma polys
  pk.sigma_lag.resize(d.n_perm);
  pk.d_sigma_coeff.assign(d.n_perm, nullptr);
  pk.sigma_ext.resize(d.n_perm);
  {
    std::vector<Fp> dpow(d.n_perm), wpow(n);
    dpow[0] = fd_one_mont<FpCfg>();
    for (int j = 1; j < d.n_perm; j++) dpow[j] = fd_mul(dpow[j - 1], pk.delta);
    wpow[0] = fd_one_mont<FpCfg>();
    for (long i = 1; i < n; i++) wpow[i] = fd_mul(wpow[i - 1], pk.omega);
    for (int j = 0; j < d.n_perm; j++) {
      pk.sigma_lag[j].resize(n);
#ifdef _OPENMP
#pragma omp parallel for schedule(static)
#endif
      for (long i = 0; i < n; i++) {
        auto [cj, ri] = d.sigma_map[(size_t)j * n + i];
        pk.sigma_lag[j][i] = fd_mul(dpow[cj], wpow[ri]);
      }
      std::vector<Fp> coeff = pk.sigma_lag[j];
      if (gpu_lag_to_coeff(c, pk.pd, coeff.data(), d.k, pk.n_inv)) return TG_ERR_HIP;
      if (keep_coeff(pk.d_sigma_coeff[j])) return TG_ERR_NOMEM;
      pk.sigma_ext[j].resize(ext_n);
      if (gpu_coeff_to_ext(c, pk.pd, coeff.data(), pk.sigma_ext[j].data(), d.k, d.ext_k,
                           pk.zeta))
        return TG_ERR_HIP;
    }
  }
  // l0 / llast / lactive
  {
    std::vector<Fp> scratch(n, fd_zero<FpCfg>());
    auto basis_ext = [&](long row, std::vector<Fp>& out) -> int {
      std::fill(scratch.begin(), scratch.end(), fd_zero<FpCfg>());
      scratch[row] = fd_one_mont<FpCfg>();
      if (gpu_lag_to_coeff(c, pk.pd, scratch.data(), d.k, pk.n_inv)) return -1;
      out.resize(ext_n);
      return gpu_coeff_to_ext(c, pk.pd, scratch.data(), out.data(), d.k, d.ext_k, pk.zeta);
    };
    if (basis_ext(0, pk.l0_ext)) return TG_ERR_HIP;
    if (basis_ext(d.usable, pk.llast_ext)) return TG_ERR_HIP;
    std::fill(scratch.begin(), scratch.end(), fd_zero<FpCfg>());
    Fp one = fd_one_mont<FpCfg>();
    for (long i = d.usable + 1; i < n; i++) scratch[i] = one;
    if (gpu_lag_to_coeff(c, pk.pd, scratch.data(), d.k, pk.n_inv)) return TG_ERR_HIP;
    pk.lactive_ext.resize(ext_n);
    if (gpu_coeff_to_ext(c, pk.pd, scratch.data(), pk.lactive_ext.data(), d.k, d.ext_k,
                         pk.zeta))
      return TG_ERR_HIP;
#ifdef _OPENMP
#pragma omp parallel for schedule(static)
#endif
    for (long i = 0; i < ext_n; i++)
      pk.lactive_ext[i] = fd_sub(one, fd_add(pk.llast_ext[i], pk.lactive_ext[i]));
  }
  // fixed-point tables for W and U (fast blind*W / value*U host mults)
  pk.wtab.init(c->h_w);
  pk.utab.init(c->h_u);
  // sigma + fixed commitments (lagrange bases, blind = 1), batched
  {
    Fp one = fd_one_mont<FpCfg>();
    pk.sigma_commits.resize(d.n_perm);
    pk.fixed_commits.resize(d.n_fixed);
    int B = d.n_perm + d.n_fixed;
    std::vector<Fp> cat((size_t)n * B), blinds(B, one);
    std::vector<VestaAff> cms(B);
    for (int j = 0; j < d.n_perm; j++)
      memcpy(cat.data() + (size_t)j * n, pk.sigma_lag[j].data(), (size_t)n * sizeof(Fp));
    for (int col = 0; col < d.n_fixed; col++)
      memcpy(cat.data() + (size_t)(d.n_perm + col) * n, d.fixed_lag[col].data(),
             (size_t)n * sizeof(Fp));
    if (gpu_msm_commit_batch(c, pk.pd, cat.data(), n, B, c->d_gl, blinds.data(),
                             cms.data(), &pk.wtab))
      return TG_ERR_HIP;
    for (int j = 0; j < d.n_perm; j++) pk.sigma_commits[j] = cms[j];
    for (int col = 0; col < d.n_fixed; col++) pk.fixed_commits[col] = cms[d.n_perm + col];
  }
  // vk repr
  {
    Blake2b h(64, (const uint8_t*)"Halo2-Verify-Key");
    u64 l = (u64)desc_len;
    uint8_t lb[8];
    memcpy(lb, &l, 8);
    h.update(lb, 8);
    h.update(desc, desc_len);
    uint8_t dig[64];
    h.final(dig);
    pk.vk_repr = from_uniform_512<FpCfg>(dig);
  }
  // ---- device-resident h-fold inputs ----
  {
    auto up_ext = [&](const std::vector<Fp>& v, Fp*& dst) -> int {
      if (hipMalloc(&dst, v.size() * sizeof(Fp)) != hipSuccess) return -1;
      hipMemcpyAsync(dst, v.data(), v.size() * sizeof(Fp), hipMemcpyHostToDevice,
                     c->stream);
      return 0;
    };
    pk.d_fixed_ext.resize(d.n_fixed);
    for (int col = 0; col < d.n_fixed; col++)
      if (up_ext(pk.fixed_ext[col], pk.d_fixed_ext[col])) return TG_ERR_NOMEM;
    pk.d_sigma_ext.resize(d.n_perm);
    for (int j = 0; j < d.n_perm; j++)
      if (up_ext(pk.sigma_ext[j], pk.d_sigma_ext[j])) return TG_ERR_NOMEM;
    if (up_ext(pk.l0_ext, pk.d_l0)) return TG_ERR_NOMEM;
    if (up_ext(pk.llast_ext, pk.d_llast)) return TG_ERR_NOMEM;
    if (up_ext(pk.lactive_ext, pk.d_lactive)) return TG_ERR_NOMEM;
    if (up_ext(pk.t_inv_ext, pk.d_tinv)) return TG_ERR_NOMEM;
    if (up_ext(pk.x_ext, pk.d_xext)) return TG_ERR_NOMEM;
    // flatten + upload expressions (stack depth re-checked against DSTK)
    std::vector<ExprOp> flat;
    // query table: [fixed_q..., advice_q..., instance_q...] — the h-fold
    // kernel preloads these per row; gate/lookup ops are rewritten to
    // XQUERY references (bit-exact rewrite)
    std::vector<DevQuery> qtab;
    for (const auto& q : d.fixed_q) qtab.push_back({0, (int)q.col, q.rot});
    for (const auto& q : d.advice_q) qtab.push_back({1, (int)q.col, q.rot});
    for (const auto& q : d.instance_q) qtab.push_back({2, (int)q.col, q.rot});
    if ((int)qtab.size() > HF_MAX_Q) return TG_ERR_BADARG;
    // order lookup-referenced queries first: when the RTC module pre-folds
    // the gates, k_h_fold only needs the lookup expressions' queries, so
    // its per-row qv preload stops at h_nq_lk (the full-table preload was
    // 822 MB/launch of dead scratch-write traffic — profiles/r02 PMC).
    {
      std::vector<char> used(qtab.size(), 0);
      auto mark = [&](const PExpr& e) {
        for (const auto& op : e.ops)
          if (op.tag == XFIXED || op.tag == XADVICE || op.tag == XINSTANCE) {
            int k = op.tag == XFIXED ? 0 : op.tag == XADVICE ? 1 : 2;
            for (size_t i = 0; i < qtab.size(); i++)
              if (qtab[i].kind == k && qtab[i].col == (int)op.a &&
                  qtab[i].rot == (int32_t)op.b)
                used[i] = 1;
          }
      };
      for (int l = 0; l < d.n_lookups; l++) {
        for (const auto& e : d.lookups[l].in) mark(e);
        for (const auto& e : d.lookups[l].tab) mark(e);
      }
      std::vector<DevQuery> reord;
      for (size_t i = 0; i < qtab.size(); i++)
        if (used[i]) reord.push_back(qtab[i]);
      pk.h_nq_lk = (int)reord.size();
      for (size_t i = 0; i < qtab.size(); i++)
        if (!used[i]) reord.push_back(qtab[i]);
      qtab = reord;
    }
    auto qidx = [&](int kind, uint32_t col, int32_t rot) -> int {
      for (size_t i = 0; i < qtab.size(); i++)
        if (qtab[i].kind == kind && qtab[i].col == (int)col && qtab[i].rot == rot)
          return (int)i;
      return -1;
    };
    auto add_expr = [&](const PExpr& e) -> DevExpr {
      int depth = 0, maxd = 0;
      for (const auto& op : e.ops) {
        if (op.tag <= XINSTANCE) depth++;
        else if (op.tag == XADD || op.tag == XSUB || op.tag == XMUL) depth--;
        if (depth > maxd) maxd = depth;
      }
      if (maxd > TG_MAX_STACK) return DevExpr{-1, -1};  // DSTK register stack depth
      DevExpr de{(int)flat.size(), (int)e.ops.size()};
      for (ExprOp op : e.ops) {
        if (op.tag == XFIXED || op.tag == XADVICE || op.tag == XINSTANCE) {
          int qi = qidx(op.tag == XFIXED ? 0 : op.tag == XADVICE ? 1 : 2,
                        op.a, op.b);
          if (qi < 0) return DevExpr{-1, -1};  // every query must be listed
          op.tag = XQUERY;
          op.a = (uint32_t)qi;
          op.b = 0;
        }
        flat.push_back(op);
      }
      return de;
    };
    pk.h_queries = qtab;
    pk.gate_de.clear();
    for (const auto& g : d.gates) {
      DevExpr de = add_expr(g);
      if (de.off < 0) return TG_ERR_BADARG;
      pk.gate_de.push_back(de);
    }
    pk.lk_in_de.assign(d.n_lookups, {});
    pk.lk_tab_de.assign(d.n_lookups, {});
    for (int l = 0; l < d.n_lookups; l++) {
      for (const auto& e : d.lookups[l].in) {
        DevExpr de = add_expr(e);
        if (de.off < 0) return TG_ERR_BADARG;
        pk.lk_in_de[l].push_back(de);
      }
      for (const auto& e : d.lookups[l].tab) {
        DevExpr de = add_expr(e);
        if (de.off < 0) return TG_ERR_BADARG;
        pk.lk_tab_de[l].push_back(de);
      }
    }
    if (hipMalloc(&pk.d_ops, std::max<size_t>(1, flat.size()) * sizeof(ExprOp)) !=
        hipSuccess)
      return TG_ERR_NOMEM;
    hipMemcpyAsync(pk.d_ops, flat.data(), flat.size() * sizeof(ExprOp),
                   hipMemcpyHostToDevice, c->stream);
    if (hipMalloc(&pk.d_queries,
                  std::max<size_t>(1, pk.h_queries.size()) * sizeof(DevQuery)) !=
        hipSuccess)
      return TG_ERR_NOMEM;
    hipMemcpyAsync(pk.d_queries, pk.h_queries.data(),
                   pk.h_queries.size() * sizeof(DevQuery), hipMemcpyHostToDevice,
                   c->stream);
    pk.rtc = hf_rtc_get(d);
    if (pk.rtc) {
      if (hipMalloc(&pk.d_colptrs,
                    sizeof(Fp*) * (d.n_fixed + d.n_advice + d.n_instance)) !=
          hipSuccess)
        return TG_ERR_NOMEM;
    }
    if (hipMalloc(&pk.d_consts, std::max<size_t>(1, d.consts.size()) * sizeof(Fp)) !=
        hipSuccess)
      return TG_ERR_NOMEM;
    hipMemcpyAsync(pk.d_consts, d.consts.data(), d.consts.size() * sizeof(Fp),
                   hipMemcpyHostToDevice, c->stream);
    if (hipStreamSynchronize(c->stream) != hipSuccess) return TG_ERR_HIP;
  }
  // the per-proof coefficient pool, sized from the descriptor: instance,
  // advice, permutation z chunks, lookup z / A' / S', then the random
  // polynomial, the collapsed h and the IPA's s polynomial
  {
    int nchunks = (d.n_perm + d.chunk_len - 1) / d.chunk_len;
    int slots = 1 + d.n_advice + nchunks + 3 * d.n_lookups + 3;
    if (!pdev_slots(c, pk.pd.coef, pk.pd.coef_slots, slots, n)) return TG_ERR_NOMEM;
  }
  // the Lagrange pool, sized the same way; its per-key part is uploaded here
  {
    LagLayout L(d);
    if (!pdev_slots(c, pk.pd.lag, pk.pd.lag_slots, L.total, n)) return TG_ERR_NOMEM;
    auto up = [&](int slot, const std::vector<Fp>& v) {
      hipMemcpyAsync(pk.pd.lag + (size_t)slot * n, v.data(), n * sizeof(Fp),
                     hipMemcpyHostToDevice, c->stream);
    };
    for (int j = 0; j < d.n_perm; j++) up(L.sigma + j, pk.sigma_lag[j]);
    for (int col = 0; col < d.n_fixed; col++)
      if (L.fixed_slot[col] >= 0) up(L.fixed_slot[col], d.fixed_lag[col]);
    // the argument block of k_lk_compress: the lookup programs over the
    // pool's Lagrange columns (a fixed column no lookup queries stays null)
    if (d.n_lookups > 0) {
      ProverDev& pd = pk.pd;
      HFoldArgs A{};  // uploaded before the synchronisation below
      A.ext_n = n;
      A.rs = 1;
      A.nlk = d.n_lookups;
      A.n_consts = d.n_consts;
      A.ops = pk.d_ops;
      A.consts = pk.d_consts;
      A.queries = pk.d_queries;
      A.n_queries = pk.h_nq_lk;
      for (int l = 0; l < d.n_lookups; l++) {
        A.lk_nin[l] = (int)pk.lk_in_de[l].size();
        A.lk_ntab[l] = (int)pk.lk_tab_de[l].size();
        for (size_t e = 0; e < pk.lk_in_de[l].size(); e++) A.lk_in[l][e] = pk.lk_in_de[l][e];
        for (size_t e = 0; e < pk.lk_tab_de[l].size(); e++)
          A.lk_tab[l][e] = pk.lk_tab_de[l][e];
      }
      for (int col = 0; col < d.n_fixed; col++)
        if (L.fixed_slot[col] >= 0) A.fixed_cols[col] = pd.lag + (size_t)L.fixed_slot[col] * n;
      for (int col = 0; col < d.n_advice; col++)
        A.advice_cols[col] = pd.lag + (size_t)(L.adv + col) * n;
      A.inst_cols[0] = pd.lag + (size_t)L.inst * n;
      if (!pd.d_lkargs && hipMalloc(&pd.d_lkargs, sizeof(HFoldArgs)) != hipSuccess)
        return TG_ERR_NOMEM;
      if (hipMemcpy(pd.d_lkargs, &A, sizeof(HFoldArgs), hipMemcpyHostToDevice) != hipSuccess)
        return TG_ERR_HIP;
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess) return TG_ERR_HIP;
  }
  pk.ready = true;
  return 0;
}

}  // namespace taiga

namespace taiga {

// ---------------- CS1 witness (spec: tools/gen_cs1.py; must match oracle) --
constexpr long CS1_REGION = 8192;

static void cs1_instance(const PDesc& d, const uint8_t seed[32], std::vector<Fp>& inst) {
  Drbg rg(seed);
  inst.assign(d.n, fd_zero<FpCfg>());
  for (int r = 0; r < d.n_instance_rows; r++) inst[r] = rg.field<FpCfg>();
}

static void cs1_witness(const PDesc& d, const uint8_t seed[32],
                        const std::vector<Fp>& inst, std::vector<std::vector<Fp>>& adv) {
  long n = d.n, u = d.usable;
  adv.assign(10, std::vector<Fp>(n));
#ifdef _OPENMP
#pragma omp parallel for schedule(static) collapse(2)
#endif
  for (int col = 0; col < 10; col++) {
    for (long i = 0; i < n; i++) {
      if (i >= u) {
        adv[col][i] = fd_zero<FpCfg>();
      } else if (col == 4 && i >= 2 * CS1_REGION && i < 3 * CS1_REGION) {
        Drbg dd(seed);
        dd.counter = (uint32_t)((u64)col * n + i);
        dd.pos = 64;
        uint8_t buf[64];
        dd.bytes(buf, 64);
        u64 v;
        memcpy(&v, buf, 8);
        Fp sv{{v & 1023, 0, 0, 0}};
        adv[col][i] = fd_to_mont(sv);
      } else {
        adv[col][i] = drbg_cell_field<FpCfg>(seed, (u64)col * n + i);
      }
    }
  }
  for (int r = 0; r < d.n_instance_rows; r++) adv[0][r] = inst[r];
  {
    Fp s42{{42, 0, 0, 0}};
    adv[7][0] = fd_to_mont(s42);
  }
#ifdef _OPENMP
#pragma omp parallel for schedule(static)
#endif
  for (long i = 0; i < CS1_REGION; i++) {
    adv[2][i] = fd_mul(adv[0][i], adv[1][i]);
    adv[3][i] = fd_add(adv[0][i], adv[1][i]);
    if (i < 4096) adv[5][i] = adv[4][i + 1];
  }
#ifdef _OPENMP
#pragma omp parallel for schedule(static)
#endif
  for (long i = CS1_REGION; i < 2 * CS1_REGION; i++) {
    Fp p = fd_mul(adv[0][i], adv[1][i]);
    p = fd_mul(p, adv[4][i]);
    p = fd_mul(p, adv[5][i]);
    p = fd_mul(p, adv[6][i]);
    p = fd_mul(p, adv[7][i]);
    p = fd_mul(p, adv[8][i]);
    p = fd_mul(p, adv[9][i]);
    adv[2][i + 1] = p;
  }
#ifdef _OPENMP
#pragma omp parallel for schedule(static)
#endif
  for (long i = 2 * CS1_REGION - 1; i < 3 * CS1_REGION - 1; i++)
    adv[3][i] = fd_zero<FpCfg>();
}

// ---------------- shared h-fold row (mirror of oracle h_fold_row) --------
struct PHRow {
  const PDesc* d;
  Fp beta, gamma, y, x, l0, llast, lactive;
  const Fp* gate_vals;
  const Fp* perm_colvals;
  const Fp* sigma_vals;
  const Fp (*zp)[2];
  const Fp* zp_last;
  const Fp (*lk)[7];
  const Fp* dpow;
};

static Fp ph_fold_row(const PHRow& r) {
  const PDesc* d = r.d;
  int nchunks = (d->n_perm + d->chunk_len - 1) / d->chunk_len;
  Fp one = fd_one_mont<FpCfg>();
  Fp acc = fd_zero<FpCfg>();
  auto yf = [&](const Fp& v) { acc = fd_add(fd_mul(acc, r.y), v); };
  for (int g = 0; g < d->n_gates; g++) yf(r.gate_vals[g]);
  yf(fd_mul(fd_sub(one, r.zp[0][0]), r.l0));
  yf(fd_mul(fd_sub(fd_sqr(r.zp[nchunks - 1][0]), r.zp[nchunks - 1][0]), r.llast));
  for (int i = 1; i < nchunks; i++)
    yf(fd_mul(fd_sub(r.zp[i][0], r.zp_last[i - 1]), r.l0));
  for (int i = 0; i < nchunks; i++) {
    int lo = i * d->chunk_len;
    int hi = std::min(lo + d->chunk_len, d->n_perm);
    Fp left = r.zp[i][1], right = r.zp[i][0];
    for (int j = lo; j < hi; j++) {
      Fp t = fd_add(fd_add(fd_mul(r.beta, r.sigma_vals[j]), r.perm_colvals[j]), r.gamma);
      left = fd_mul(left, t);
      Fp u2 = fd_add(fd_add(fd_mul(fd_mul(r.dpow[j], r.x), r.beta), r.perm_colvals[j]),
                     r.gamma);
      right = fd_mul(right, u2);
    }
    yf(fd_mul(fd_sub(left, right), r.lactive));
  }
  for (int l = 0; l < d->n_lookups; l++) {
    const Fp* L = r.lk[l];
    yf(fd_mul(fd_sub(one, L[0]), r.l0));
    yf(fd_mul(fd_sub(fd_sqr(L[0]), L[0]), r.llast));
    Fp left = fd_mul(fd_mul(L[1], fd_add(L[2], r.beta)), fd_add(L[4], r.gamma));
    Fp right = fd_mul(fd_mul(L[0], fd_add(L[5], r.beta)), fd_add(L[6], r.gamma));
    yf(fd_mul(fd_sub(left, right), r.lactive));
    yf(fd_mul(fd_sub(L[2], L[4]), r.l0));
    yf(fd_mul(fd_mul(fd_sub(L[2], L[4]), fd_sub(L[2], L[3])), r.lactive));
  }
  return acc;
}

// ---------------- the product prove ----------------

struct PMQuery {
  int poly_id;
  Fp point, eval;
};

struct StageTimer {
  bool on;
  hipStream_t stream;
  double last;
  StageTimer(hipStream_t s) : stream(s) {
    on = getenv("TG_PROF_STAGES") != nullptr;
    if (on) {
      hipStreamSynchronize(stream);
      last = now();
    }
  }
  static double now() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + 1e-9 * ts.tv_nsec;
  }
  void mark(const char* name) {
    if (!on) return;
    hipStreamSynchronize(stream);
    double t = now();
    fprintf(stderr, "# stage %-22s %8.2f ms\n", name, (t - last) * 1e3);
    last = sub_last = t;
  }
  // a mark inside a stage: the time since the previous mark of either kind;
  // the enclosing stage's own mark still reports the whole stage
  double sub_last = 0;
  void sub(const char* name) {
    if (!on) return;
    hipStreamSynchronize(stream);
    double t = now();
    fprintf(stderr, "# substage %-19s %8.2f ms\n", name,
            (t - (sub_last > last ? sub_last : last)) * 1e3);
    sub_last = t;
  }
};

// core prover over a MATERIALIZED witness (instance lagrange vector +
// advice lagrange columns, Mont form; advice rows >= usable are overwritten
// with blinding). The seeded CS1 path and the raw-witness ABI both land
// here, so proof bytes depend only on (SRS, desc, witness, rng stream).
static int pprove_core(Ctx* c, PPk& pk, std::vector<Fp>& inst_lag,
                       std::vector<std::vector<Fp>>& advice_lag,
                       const uint8_t rng_seed[32], std::vector<uint8_t>& proof_out) {
  StageTimer st_(c->stream);
  PDesc& d = pk.d;
  long n = d.n, ext_n = d.ext_n, u = d.usable;
  int nchunks = (d.n_perm + d.chunk_len - 1) / d.chunk_len;
  int nlk = d.n_lookups;
  ProverDev& pd = pk.pd;
  Drbg rng(rng_seed);
  Transcript ts;
  Fp one = fd_one_mont<FpCfg>();

  ts.common_scalar(pk.vk_repr);

  // Lagrange pool slots (sized and half filled at keygen): every column is
  // uploaded once, and the commits, the grand products and the transforms
  // read it there
  const LagLayout LG(d);
  if (pd.lag_slots < LG.total) return TG_ERR_STATE;
  auto lslot = [&](int idx) { return pd.lag + (size_t)idx * n; };
  auto lag_up = [&](int idx, const std::vector<Fp>& v) {
    hipMemcpyAsync(lslot(idx), v.data(), n * sizeof(Fp), hipMemcpyHostToDevice, c->stream);
  };

  // 1. instance
  VestaAff inst_cm;
  lag_up(LG.inst, inst_lag);
  if (gpu_msm_commit_batch_dev(c, lslot(LG.inst), n, 1, c->d_gl, &one, &inst_cm, &pk.wtab))
    return TG_ERR_HIP;
  ts.common_point(inst_cm);
  st_.mark("instance_commit");
  // device ext-buffer layout: advice | inst | permz | lkz | lkAp | lkSp | h
  const int EB_ADV = 0, EB_INST = EB_ADV + d.n_advice, EB_PZ = EB_INST + d.n_instance;
  const int EB_LZ = EB_PZ + nchunks, EB_AP = EB_LZ + nlk, EB_SP = EB_AP + nlk;
  const int EB_H = EB_SP + nlk;
  // coefficient pool slots (sized at keygen): the coefficient form stays on
  // the device, where the opening phase reads it
  const int CS_INST = 0, CS_ADV = 1, CS_PZ = CS_ADV + d.n_advice, CS_LZ = CS_PZ + nchunks;
  const int CS_AP = CS_LZ + nlk, CS_SP = CS_AP + nlk, CS_RAND = CS_SP + nlk;
  const int CS_H = CS_RAND + 1, CS_S = CS_H + 1;
  if (pd.coef_slots < CS_S + 1) return TG_ERR_STATE;
  auto cslot = [&](int idx) { return pd.coef + (size_t)idx * n; };
  Fp* d_inst_ext = pdev_ext_buf(pd, EB_INST);
  if (!d_inst_ext) return TG_ERR_NOMEM;
  if (gpu_dlag_to_coeff_ext_dev(c, pd, lslot(LG.inst), cslot(CS_INST), d_inst_ext, d.k,
                                d.ext_k, pk.n_inv, pk.zeta))
    return TG_ERR_HIP;

  // 2. advice
  for (int col = 0; col < d.n_advice; col++)
    for (long i = u; i < n; i++) advice_lag[col][i] = rng.field<FpCfg>();
  std::vector<Fp> advice_blind(d.n_advice);
  for (int col = 0; col < d.n_advice; col++) advice_blind[col] = rng.field<FpCfg>();
  {
    for (int col = 0; col < d.n_advice; col++) lag_up(LG.adv + col, advice_lag[col]);
    std::vector<VestaAff> cms(d.n_advice);
    if (gpu_msm_commit_batch_dev(c, lslot(LG.adv), n, d.n_advice, c->d_gl,
                                 advice_blind.data(), cms.data(), &pk.wtab))
      return TG_ERR_HIP;
    for (int col = 0; col < d.n_advice; col++)
      if (ts.write_point(cms[col])) return TG_ERR_BADARG;
  }
  for (int col = 0; col < d.n_advice; col++) {
    Fp* dbuf = pdev_ext_buf(pd, EB_ADV + col);
    if (!dbuf) return TG_ERR_NOMEM;
    if (gpu_dlag_to_coeff_ext_dev(c, pd, lslot(LG.adv + col), cslot(CS_ADV + col), dbuf,
                                  d.k, d.ext_k, pk.n_inv, pk.zeta))
      return TG_ERR_HIP;
  }

  st_.mark("advice_commit+ext");
  Fp theta = ts.squeeze();

  // 3. lookups, on the device (lookup_argument.hip): compress A and S over
  // the usable rows, sort A into A' and S into the table scratch, build S'.
  // Rows u..n-1 of A' and S' are blinding drawn here in the order the host
  // loops drew them: per lookup the A' rows, the S' rows, the A' blind, the
  // S' blind. The draws do not depend on the values, so nothing waits for
  // the kernels; the uploads are ordered after them on the stream, where
  // they overwrite the sort's padding.
  std::vector<Fp> lkAp_blind(nlk), lkSp_blind(nlk);
  if (nlk > 0) {
    if (!pd.d_lkargs) return TG_ERR_STATE;
    LkCompressOut co{};
    const Fp* srt_src[LK_MAX_ARRAYS];
    Fp *srt_dst[LK_MAX_ARRAYS], *pap[TG_MAX_LOOKUPS], *psp[TG_MAX_LOOKUPS];
    const Fp* pt[TG_MAX_LOOKUPS];
    for (int l = 0; l < nlk; l++) {
      pap[l] = lslot(LG.lk + 4 * l);
      psp[l] = lslot(LG.lk + 4 * l + 1);
      co.a[l] = lslot(LG.lk + 4 * l + 2);
      co.s[l] = lslot(LG.lk + 4 * l + 3);
      pt[l] = lslot(LG.lkt + l);
      srt_src[2 * l] = co.a[l];
      srt_dst[2 * l] = pap[l];
      srt_src[2 * l + 1] = co.s[l];
      srt_dst[2 * l + 1] = lslot(LG.lkt + l);
    }
    {
      ProfScope ps(c, P_LK_COMPRESS);
      hipLaunchKernelGGL(k_lk_compress, dim3(ntt_grid(u)), dim3(256), 0, c->stream,
                         (const HFoldArgs*)pd.d_lkargs, theta, u, co);
    }
    st_.sub("lk_compress");
    int rc = dev_lk_sort(c, 2 * nlk, srt_src, srt_dst, u, n);
    if (!rc) rc = dev_lk_permute(c, pd, nlk, pap, pt, psp, u);
    if (rc) return rc;
    const long nblind = n - u;
    std::vector<Fp> lk_tail((size_t)2 * nlk * nblind);  // outlives the next sync
    for (int l = 0; l < nlk; l++) {
      Fp* ta = lk_tail.data() + (size_t)2 * l * nblind;
      Fp* tsp = ta + nblind;
      for (long i = 0; i < nblind; i++) ta[i] = rng.field<FpCfg>();
      for (long i = 0; i < nblind; i++) tsp[i] = rng.field<FpCfg>();
      lkAp_blind[l] = rng.field<FpCfg>();
      lkSp_blind[l] = rng.field<FpCfg>();
      hipMemcpyAsync(pap[l] + u, ta, nblind * sizeof(Fp), hipMemcpyHostToDevice, c->stream);
      hipMemcpyAsync(psp[l] + u, tsp, nblind * sizeof(Fp), hipMemcpyHostToDevice, c->stream);
    }
    // the error word travels back with the first commit's synchronisation
    dev_lk_fetch_err(c, pd);
    st_.sub("lk_sort_permute");
    for (int l = 0; l < nlk; l++) {
      Fp blds[2] = {lkAp_blind[l], lkSp_blind[l]};
      VestaAff cms[2];
      if (gpu_msm_commit_batch_dev(c, pap[l], n, 2, c->d_gl, blds, cms, &pk.wtab))
        return TG_ERR_HIP;
      // an input value that the table lacks
      if (pd.lk_err_h) return TG_ERR_BADARG;
      if (ts.write_point(cms[0])) return TG_ERR_BADARG;
      if (ts.write_point(cms[1])) return TG_ERR_BADARG;
    }
    st_.sub("lk_commit");
  }

  st_.mark("lookup_permute");
  Fp beta = ts.squeeze();
  Fp gamma = ts.squeeze();
  // (finer marks inside the grand-product stage)

  // 4. permutation grand products (chunks CHAIN via last_z)
  // on the device (grand_products.hip). z vector b < nchunks is chunk b's,
  // the others are the lookups'; its rows 0..u come from the scan, rows
  // u+1..n-1 are blinding drawn here, in the order the host loops drew them:
  // per vector the rows, then the blind. The draws do not depend on the
  // values, so nothing waits for the kernels.
  const int nz = nchunks + nlk;
  const long ntail = n - u - 1;
  std::vector<Fp> z_tail((size_t)nz * ntail), z_blind(nz);  // outlive the next sync
  auto draw_tail = [&](int b) {
    Fp* t = z_tail.data() + (size_t)b * ntail;
    for (long i = 0; i < ntail; i++) t[i] = rng.field<FpCfg>();
    z_blind[b] = rng.field<FpCfg>();
    if (ntail > 0)
      hipMemcpyAsync(lslot(LG.z + b) + u + 1, t, ntail * sizeof(Fp), hipMemcpyHostToDevice,
                     c->stream);
  };
  {
    std::vector<const Fp*> cols(d.n_perm), sigmas(d.n_perm);
    for (int jj = 0; jj < d.n_perm; jj++) {
      auto [kind, idx] = d.perm_cols[jj];
      cols[jj] = lslot(kind == 0 ? LG.adv + (int)idx
                       : kind == 1 ? LG.fixed_slot[idx] : LG.inst);
      sigmas[jj] = lslot(LG.sigma + jj);
    }
    int rc = dev_gp_perm_terms(c, pd, cols, sigmas, d.chunk_len, u, beta, gamma, pk.omega,
                               pk.delta, lslot(LG.num), lslot(LG.den));
    if (rc) return rc;
    for (int ch = 0; ch < nchunks; ch++) draw_tail(ch);
  }
  st_.mark("gp_perm_z");
  /* perm z commits batched with lookup z below */

  // 5. lookup grand products; then ONE inversion over every chunk's and
  // every lookup's denominators, and one scan: the chunks are one chain
  // from 1 (each starts where the one before ended), every lookup its own
  {
    if (nlk > 0) {
      const Fp *pa[TG_MAX_LOOKUPS], *psv[TG_MAX_LOOKUPS], *pap[TG_MAX_LOOKUPS],
          *psp[TG_MAX_LOOKUPS];
      for (int l = 0; l < nlk; l++) {
        pap[l] = lslot(LG.lk + 4 * l);
        psp[l] = lslot(LG.lk + 4 * l + 1);
        pa[l] = lslot(LG.lk + 4 * l + 2);
        psv[l] = lslot(LG.lk + 4 * l + 3);
      }
      int rc = dev_gp_lookup_terms(c, pd, nlk, pa, psv, pap, psp, u, beta, gamma,
                                   lslot(LG.num) + (size_t)nchunks * u,
                                   lslot(LG.den) + (size_t)nchunks * u);
      if (rc) return rc;
    }
    int rc = dev_gp_batch_inverse(c, lslot(LG.den), (long)nz * u);
    if (rc) return rc;
    std::vector<GpSeg> segs(nz);
    for (int b = 0; b < nz; b++)
      segs[b] = GpSeg{u, lslot(LG.z + b), b > 0 && b < nchunks, one};
    if ((rc = dev_gp_scan(c, pd, lslot(LG.num), lslot(LG.den), segs))) return rc;
    for (int l = 0; l < nlk; l++) draw_tail(nchunks + l);
  }
  st_.mark("gp_lookup_z");
  {
    int B = nz;
    const std::vector<Fp>& blinds = z_blind;
    std::vector<VestaAff> cms(B);
    if (gpu_msm_commit_batch_dev(c, lslot(LG.z), n, B, c->d_gl, blinds.data(), cms.data(),
                                 &pk.wtab))
      return TG_ERR_HIP;
    for (int b = 0; b < B; b++)
      if (ts.write_point(cms[b])) return TG_ERR_BADARG;
  }

  // 6. vanishing random poly
  st_.mark("gp_z_commits");
  std::vector<Fp> random_poly(n);
  drbg_fields_par(rng, random_poly.data(), n);
  Fp random_blind = rng.field<FpCfg>();
  {
    // uploaded once into its pool slot: the commit and the openings read it there
    VestaAff cm;
    hipMemcpyAsync(cslot(CS_RAND), random_poly.data(), n * sizeof(Fp),
                   hipMemcpyHostToDevice, c->stream);
    if (gpu_msm_commit_batch_dev(c, cslot(CS_RAND), n, 1, c->d_g, &random_blind, &cm,
                                 &pk.wtab))
      return TG_ERR_HIP;
    if (ts.write_point(cm)) return TG_ERR_BADARG;
  }

  st_.mark("grand_products+rand");
  Fp ych = ts.squeeze();

  // 7. h on extended coset (transforms via GPU; fold on host OpenMP)
  for (int ch = 0; ch < nchunks; ch++) {
    Fp* dbuf = pdev_ext_buf(pd, EB_PZ + ch);
    if (!dbuf) return TG_ERR_NOMEM;
    if (gpu_dlag_to_coeff_ext_dev(c, pd, lslot(LG.z + ch), cslot(CS_PZ + ch), dbuf, d.k,
                                  d.ext_k, pk.n_inv, pk.zeta))
      return TG_ERR_HIP;
  }
  for (int l = 0; l < nlk; l++) {
    Fp *dz = pdev_ext_buf(pd, EB_LZ + l), *dap = pdev_ext_buf(pd, EB_AP + l),
       *dsp = pdev_ext_buf(pd, EB_SP + l);
    if (!dz || !dap || !dsp) return TG_ERR_NOMEM;
    if (gpu_dlag_to_coeff_ext_dev(c, pd, lslot(LG.z + nchunks + l), cslot(CS_LZ + l), dz,
                                  d.k, d.ext_k, pk.n_inv, pk.zeta))
      return TG_ERR_HIP;
    if (gpu_dlag_to_coeff_ext_dev(c, pd, lslot(LG.lk + 4 * l), cslot(CS_AP + l), dap, d.k,
                                  d.ext_k, pk.n_inv, pk.zeta))
      return TG_ERR_HIP;
    if (gpu_dlag_to_coeff_ext_dev(c, pd, lslot(LG.lk + 4 * l + 1), cslot(CS_SP + l), dsp,
                                  d.k, d.ext_k, pk.n_inv, pk.zeta))
      return TG_ERR_HIP;
  }
  st_.mark("z_transforms");
  {
    HFoldArgs A{};
    A.ext_n = ext_n;
    A.rs = ext_n / n;
    A.n_gates = d.n_gates;
    A.n_perm = d.n_perm;
    A.chunk_len = d.chunk_len;
    A.nlk = nlk;
    A.nchunks = nchunks;
    A.last_rot = -(d.bf + 1);
    A.n_consts = d.n_consts;
    A.beta = beta;
    A.gamma = gamma;
    A.y = ych;
    A.theta = theta;
    A.x_ext = pk.d_xext;
    A.l0 = pk.d_l0;
    A.llast = pk.d_llast;
    A.lactive = pk.d_lactive;
    A.t_inv = pk.d_tinv;
    A.ops = pk.d_ops;
    A.consts = pk.d_consts;
    A.queries = pk.d_queries;
    A.n_queries = (int)pk.h_queries.size();
    for (int g = 0; g < d.n_gates; g++) A.gates[g] = pk.gate_de[g];
    for (int l = 0; l < nlk; l++) {
      A.lk_nin[l] = (int)pk.lk_in_de[l].size();
      A.lk_ntab[l] = (int)pk.lk_tab_de[l].size();
      for (size_t e = 0; e < pk.lk_in_de[l].size(); e++) A.lk_in[l][e] = pk.lk_in_de[l][e];
      for (size_t e = 0; e < pk.lk_tab_de[l].size(); e++)
        A.lk_tab[l][e] = pk.lk_tab_de[l][e];
      A.lkz[l] = pdev_ext_buf(pd, EB_LZ + l);
      A.lkap[l] = pdev_ext_buf(pd, EB_AP + l);
      A.lksp[l] = pdev_ext_buf(pd, EB_SP + l);
    }
    for (int col = 0; col < d.n_fixed; col++) A.fixed_cols[col] = pk.d_fixed_ext[col];
    for (int col = 0; col < d.n_advice; col++)
      A.advice_cols[col] = pdev_ext_buf(pd, EB_ADV + col);
    A.inst_cols[0] = d_inst_ext;
    Fp dp = fd_one_mont<FpCfg>();
    for (int jj = 0; jj < d.n_perm; jj++) {
      A.sigma[jj] = pk.d_sigma_ext[jj];
      A.perm_kind[jj] = (int)d.perm_cols[jj].first;
      A.perm_idx[jj] = (int)d.perm_cols[jj].second;
      A.dpow[jj] = dp;
      dp = fd_mul(dp, pk.delta);
    }
    for (int ch = 0; ch < nchunks; ch++) A.zp[ch] = pdev_ext_buf(pd, EB_PZ + ch);
    A.out = pdev_ext_buf(pd, EB_H);
    if (!A.out) return TG_ERR_NOMEM;
    A.acc_init = nullptr;
    if (pk.rtc && pk.rtc->ready) {
      // runtime-specialized gate fold (hf_rtc.hpp): bit-identical to the
      // interpreter loop it replaces
      std::vector<Fp*> colptrs;
      for (int col = 0; col < d.n_fixed; col++) colptrs.push_back(pk.d_fixed_ext[col]);
      for (int col = 0; col < d.n_advice; col++)
        colptrs.push_back(pdev_ext_buf(pd, EB_ADV + col));
      colptrs.push_back(d_inst_ext);
      if (hipMemcpyAsync(pk.d_colptrs, colptrs.data(), sizeof(Fp*) * colptrs.size(),
                         hipMemcpyHostToDevice, c->stream) != hipSuccess)
        return TG_ERR_HIP;
      Fp* gacc = pdev_ext_buf(pd, EB_H + 1);
      if (!gacc) return TG_ERR_NOMEM;
      Fp yv = A.y;
      long extn = ext_n, rsv = A.rs;
      Fp** dcols = pk.d_colptrs;
      void* params[] = {&gacc, &dcols, &yv, &extn, &rsv};
      if (hipModuleLaunchKernel(pk.rtc->fn, (unsigned)ntt_grid(ext_n), 1, 1, 256, 1,
                                1, 0, c->stream, params, nullptr) != hipSuccess)
        return TG_ERR_HIP;
      A.acc_init = gacc;
      A.n_gates = 0;
      A.n_queries = pk.h_nq_lk;  // gates gone: preload only lookup queries
      st_.mark("h_rtc_gates");
    }
    if (!pd.d_hargs && hipMalloc(&pd.d_hargs, sizeof(HFoldArgs)) != hipSuccess)
      return TG_ERR_NOMEM;
    if (hipMemcpyAsync(pd.d_hargs, &A, sizeof(HFoldArgs), hipMemcpyHostToDevice,
                       c->stream) != hipSuccess)
      return TG_ERR_HIP;
    hipLaunchKernelGGL(k_h_fold, dim3(ntt_grid(ext_n)), dim3(256), 0, c->stream,
                       (const HFoldArgs*)pd.d_hargs);
    st_.mark("h_fold_rest");
  }
  // iNTT + zeta-undistribute directly on the device h buffer; the pieces
  // of h's coefficient form stay there (commit scalars, then the collapse)
  Fp* dH = pdev_ext_buf(pd, EB_H);
  if (ntt_run(dH, pd.ws1, pd.plan_ext, d.ext_k, true, c->stream, &pk.ext_n_inv,
              ntt_noprof) != hipSuccess)
    return TG_ERR_HIP;
  coset_scale_launch(dH, (u64)ext_n, pk.zeta_inv, c->stream);
  int npieces = (int)(ext_n / n);
  std::vector<Fp> h_blind(npieces);
  for (int pce = 0; pce < npieces; pce++) h_blind[pce] = rng.field<FpCfg>();
  {
    std::vector<VestaAff> cms(npieces);
    if (gpu_msm_commit_batch_dev(c, dH, n, npieces, c->d_g, h_blind.data(), cms.data(),
                                 &pk.wtab))
      return TG_ERR_HIP;
    for (int pce = 0; pce < npieces; pce++)
      if (ts.write_point(cms[pce])) return TG_ERR_BADARG;
  }

  st_.mark("h_commit");
  Fp x = ts.squeeze();
  Fp xn = x;
  for (int i = 0; i < d.k; i++) xn = fd_sqr(xn);

  // 8. evals, on the device. Every point is known once x is squeezed and no
  // challenge is drawn between the evaluation writes, so all of step 8 is
  // one batched launch, one download and one synchronisation; the scalars
  // then go to the transcript in the order the queries were listed.
  auto rot_pt = [&](const Fp& xx, int rot) {
    Fp w = fd_one_mont<FpCfg>();
    const Fp& base = rot < 0 ? pk.omega_inv : pk.omega;
    for (int i = 0; i < (rot < 0 ? -rot : rot); i++) w = fd_mul(w, base);
    return fd_mul(xx, w);
  };
  // h collapsed: Horner over the pieces in x^n, highest piece first
  Fp h_collapsed_blind = h_blind[npieces - 1];
  for (int pce = npieces - 2; pce >= 0; pce--)
    h_collapsed_blind = fd_add(fd_mul(h_collapsed_blind, xn), h_blind[pce]);
  {
    std::vector<const Fp*> pieces;
    for (int pce = npieces - 1; pce >= 0; pce--) pieces.push_back(dH + (size_t)pce * n);
    if (dev_horner_comb(c, pd, pieces, xn, cslot(CS_H), n)) return TG_ERR_HIP;
  }
  std::vector<Fp> adv_eval(d.n_advice_q), fix_eval(d.n_fixed_q), sig_eval(d.n_perm);
  Fp rand_eval, h_eval;
  Fp pz_eval[TG_MAX_CHUNKS][2], pz_last_eval[TG_MAX_CHUNKS], lk_eval[TG_MAX_LOOKUPS][5];
  std::vector<Fp> inst_eval(d.n_instance_q);
  Fp x_next = rot_pt(x, 1), x_prev = rot_pt(x, -1), x_last = rot_pt(x, -(d.bf + 1));
  {
    std::vector<EvalQuery> evq;
    std::vector<Fp*> dest;  // where each query's value goes
    auto ask = [&](const Fp* poly, const Fp& pt, Fp& into) {
      evq.push_back(EvalQuery{poly, n, pt});
      dest.push_back(&into);
    };
    for (int q = 0; q < d.n_advice_q; q++)
      ask(cslot(CS_ADV + d.advice_q[q].col), rot_pt(x, d.advice_q[q].rot), adv_eval[q]);
    for (int q = 0; q < d.n_fixed_q; q++)
      ask(pk.d_fixed_coeff[d.fixed_q[q].col], rot_pt(x, d.fixed_q[q].rot), fix_eval[q]);
    ask(cslot(CS_RAND), x, rand_eval);
    for (int j = 0; j < d.n_perm; j++) ask(pk.d_sigma_coeff[j], x, sig_eval[j]);
    for (int ch = 0; ch < nchunks; ch++) {
      ask(cslot(CS_PZ + ch), x, pz_eval[ch][0]);
      ask(cslot(CS_PZ + ch), x_next, pz_eval[ch][1]);
    }
    for (int ch = 0; ch < nchunks - 1; ch++) ask(cslot(CS_PZ + ch), x_last, pz_last_eval[ch]);
    for (int l = 0; l < nlk; l++) {
      ask(cslot(CS_LZ + l), x, lk_eval[l][0]);
      ask(cslot(CS_LZ + l), x_next, lk_eval[l][1]);
      ask(cslot(CS_AP + l), x, lk_eval[l][2]);
      ask(cslot(CS_AP + l), x_prev, lk_eval[l][3]);
      ask(cslot(CS_SP + l), x, lk_eval[l][4]);
    }
    size_t n_written = evq.size();  // the rest is not written to the transcript
    ask(cslot(CS_H), x, h_eval);
    for (int q = 0; q < d.n_instance_q; q++)
      ask(cslot(CS_INST), rot_pt(x, d.instance_q[q].rot), inst_eval[q]);
    std::vector<Fp> evs(evq.size());
    if (dev_poly_eval_batch(c, pd, evq, evs.data())) return TG_ERR_HIP;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return TG_ERR_HIP;
    for (size_t i = 0; i < evs.size(); i++) {
      *dest[i] = evs[i];
      if (i < n_written) ts.write_scalar(evs[i]);
    }
  }

  st_.mark("evals");
  // 9. multiopen query list (order mirrors the oracle exactly); the
  // polynomials are device coefficient vectors
  struct PolyRef {
    const Fp* coeff;
    Fp blind;
  };
  std::vector<PolyRef> polys;
  std::vector<PMQuery> queries;
  auto add_poly = [&](const Fp* coeff, const Fp& blind) {
    polys.push_back({coeff, blind});
    return (int)polys.size() - 1;
  };
  auto add_q = [&](int pid, const Fp& pt, const Fp& ev) {
    queries.push_back({pid, pt, ev});
  };
  int pid_inst = add_poly(cslot(CS_INST), one);
  std::vector<int> pid_adv(d.n_advice);
  for (int col = 0; col < d.n_advice; col++)
    pid_adv[col] = add_poly(cslot(CS_ADV + col), advice_blind[col]);
  std::vector<int> pid_pz(nchunks);
  for (int ch = 0; ch < nchunks; ch++)
    pid_pz[ch] = add_poly(cslot(CS_PZ + ch), z_blind[ch]);
  std::vector<int> pid_lz(nlk), pid_lap(nlk), pid_lsp(nlk);
  for (int l = 0; l < nlk; l++) {
    pid_lz[l] = add_poly(cslot(CS_LZ + l), z_blind[nchunks + l]);
    pid_lap[l] = add_poly(cslot(CS_AP + l), lkAp_blind[l]);
    pid_lsp[l] = add_poly(cslot(CS_SP + l), lkSp_blind[l]);
  }
  std::vector<int> pid_fix(d.n_fixed);
  for (int col = 0; col < d.n_fixed; col++)
    pid_fix[col] = add_poly(pk.d_fixed_coeff[col], one);
  std::vector<int> pid_sig(d.n_perm);
  for (int j = 0; j < d.n_perm; j++) pid_sig[j] = add_poly(pk.d_sigma_coeff[j], one);
  int pid_h = add_poly(cslot(CS_H), h_collapsed_blind);
  int pid_rand = add_poly(cslot(CS_RAND), random_blind);

  for (int q = 0; q < d.n_instance_q; q++)
    add_q(pid_inst, rot_pt(x, d.instance_q[q].rot), inst_eval[q]);
  for (int q = 0; q < d.n_advice_q; q++)
    add_q(pid_adv[d.advice_q[q].col], rot_pt(x, d.advice_q[q].rot), adv_eval[q]);
  for (int ch = 0; ch < nchunks; ch++) {
    add_q(pid_pz[ch], x, pz_eval[ch][0]);
    add_q(pid_pz[ch], x_next, pz_eval[ch][1]);
  }
  for (int ch = 0; ch < nchunks - 1; ch++) add_q(pid_pz[ch], x_last, pz_last_eval[ch]);
  for (int l = 0; l < nlk; l++) {
    add_q(pid_lz[l], x, lk_eval[l][0]);
    add_q(pid_lap[l], x, lk_eval[l][2]);
    add_q(pid_lsp[l], x, lk_eval[l][4]);
    add_q(pid_lap[l], x_prev, lk_eval[l][3]);
    add_q(pid_lz[l], x_next, lk_eval[l][1]);
  }
  for (int q = 0; q < d.n_fixed_q; q++)
    add_q(pid_fix[d.fixed_q[q].col], rot_pt(x, d.fixed_q[q].rot), fix_eval[q]);
  for (int j = 0; j < d.n_perm; j++) add_q(pid_sig[j], x, sig_eval[j]);
  add_q(pid_h, x, h_eval);
  add_q(pid_rand, x, rand_eval);

  // ---- multiopen ----
  Fp x1 = ts.squeeze();
  Fp x2 = ts.squeeze();
  int NP = (int)polys.size();
  std::vector<int> order;
  std::vector<int> poly_set(NP, -1);
  std::vector<std::vector<Fp>> ppts(NP), pevs(NP);
  for (const auto& q : queries) {
    if (ppts[q.poly_id].empty()) order.push_back(q.poly_id);
    ppts[q.poly_id].push_back(q.point);
    pevs[q.poly_id].push_back(q.eval);
  }
  std::vector<std::vector<Fp>> set_pts;
  for (int pid : order) {
    int found = -1;
    for (size_t s = 0; s < set_pts.size(); s++) {
      if (set_pts[s].size() != ppts[pid].size()) continue;
      bool eq = true;
      for (size_t j = 0; j < set_pts[s].size(); j++)
        if (!fd_eq(set_pts[s][j], ppts[pid][j])) { eq = false; break; }
      if (eq) { found = (int)s; break; }
    }
    if (found < 0) {
      found = (int)set_pts.size();
      set_pts.push_back(ppts[pid]);
    }
    poly_set[pid] = found;
  }
  int n_sets = (int)set_pts.size();
  // device work vectors: q_poly[s], each set's quotient, bvec, wfold
  if (!pdev_slots(c, pd.open_ws, pd.open_slots, 2 * n_sets + 2, n)) return TG_ERR_NOMEM;
  auto wslot = [&](int idx) { return pd.open_ws + (size_t)idx * n; };
  auto q_poly = [&](int s) { return wslot(s); };
  auto quot = [&](int s) { return wslot(n_sets + s); };
  Fp *d_bvec = wslot(2 * n_sets), *d_wfold = wslot(2 * n_sets + 1);
  // q_poly[s] = Horner in x1 over the set's polynomials, in query order;
  // the blinds and evaluations combine on the host (scalars)
  std::vector<std::vector<const Fp*>> set_polys(n_sets);
  std::vector<Fp> q_blind(n_sets, fd_zero<FpCfg>());
  std::vector<std::vector<Fp>> q_ev(n_sets);
  for (int s = 0; s < n_sets; s++) q_ev[s].assign(set_pts[s].size(), fd_zero<FpCfg>());
  for (int pid : order) {
    int s = poly_set[pid];
    set_polys[s].push_back(polys[pid].coeff);
    q_blind[s] = fd_add(fd_mul(q_blind[s], x1), polys[pid].blind);
    for (size_t j = 0; j < q_ev[s].size(); j++)
      q_ev[s][j] = fd_add(fd_mul(q_ev[s][j], x1), pevs[pid][j]);
  }
  for (int s = 0; s < n_sets; s++)
    if (dev_horner_comb(c, pd, set_polys[s], x1, q_poly(s), n)) return TG_ERR_HIP;
  // quotient of each set by its points, one after the other (the length
  // drops by one per point); the sets divide side by side
  {
    size_t max_pts = 0;
    for (int s = 0; s < n_sets; s++) max_pts = std::max(max_pts, set_pts[s].size());
    for (size_t j = 0; j < max_pts; j++) {
      std::vector<KateJob> jobs;
      for (int s = 0; s < n_sets; s++)
        if (set_pts[s].size() > j)
          jobs.push_back(KateJob{j == 0 ? q_poly(s) : quot(s), quot(s), n - (long)j,
                                 set_pts[s][j]});
      if (dev_kate_div(c, pd, jobs)) return TG_ERR_HIP;
    }
  }
  // f = Horner in x2 over the quotients (in place over the first)
  Fp* d_f = quot(0);
  {
    std::vector<const Fp*> qs;
    for (int s = 0; s < n_sets; s++) qs.push_back(quot(s));
    if (dev_horner_comb(c, pd, qs, x2, d_f, n)) return TG_ERR_HIP;
  }
  Fp f_blind = rng.field<FpCfg>();
  {
    VestaAff cm;
    if (gpu_msm_commit_batch_dev(c, d_f, n, 1, c->d_g, &f_blind, &cm, &pk.wtab))
      return TG_ERR_HIP;
    if (ts.write_point(cm)) return TG_ERR_BADARG;
  }
  st_.mark("multiopen_f");
  Fp x3 = ts.squeeze();
  // the IPA's s polynomial is drawn here (the next draws of the rng stream;
  // the transcript is not involved), so that its evaluation at x3 shares
  // the launch with the q_poly evaluations
  std::vector<Fp> s_poly(n);
  drbg_fields_par(rng, s_poly.data(), n);
  hipMemcpyAsync(cslot(CS_S), s_poly.data(), n * sizeof(Fp), hipMemcpyHostToDevice,
                 c->stream);
  std::vector<Fp> q_at_x3(n_sets + 1);
  {
    std::vector<EvalQuery> evq;
    for (int s = 0; s < n_sets; s++) evq.push_back(EvalQuery{q_poly(s), n, x3});
    evq.push_back(EvalQuery{cslot(CS_S), n, x3});
    if (dev_poly_eval_batch(c, pd, evq, q_at_x3.data())) return TG_ERR_HIP;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return TG_ERR_HIP;
  }
  for (int s = 0; s < n_sets; s++) ts.write_scalar(q_at_x3[s]);
  Fp x4 = ts.squeeze();
  // final = Horner in x4 over f, q_poly[0], q_poly[1], ... (in place over f)
  Fp final_blind = f_blind;
  {
    std::vector<const Fp*> qs{d_f};
    for (int s = 0; s < n_sets; s++) {
      qs.push_back(q_poly(s));
      final_blind = fd_add(fd_mul(final_blind, x4), q_blind[s]);
    }
    if (dev_horner_comb(c, pd, qs, x4, d_f, n)) return TG_ERR_HIP;
  }

  st_.mark("multiopen_final");
  // ---- IPA ----
  // s(x3) = 0: the constant term takes the evaluation off
  s_poly[0] = fd_sub(s_poly[0], q_at_x3[n_sets]);
  hipMemcpyAsync(cslot(CS_S), s_poly.data(), sizeof(Fp), hipMemcpyHostToDevice, c->stream);
  Fp s_blind = rng.field<FpCfg>();
  {
    VestaAff cm;
    if (gpu_msm_commit_batch_dev(c, cslot(CS_S), n, 1, c->d_g, &s_blind, &cm, &pk.wtab))
      return TG_ERR_HIP;
    if (ts.write_point(cm)) return TG_ERR_BADARG;
  }
  Fp xi = ts.squeeze();
  // pp = final + xi * s (in place over final); bvec = powers of x3
  Fp* d_pp = d_f;
  {
    std::vector<const Fp*> qs{cslot(CS_S), d_f};
    if (dev_horner_comb(c, pd, qs, xi, d_pp, n)) return TG_ERR_HIP;
  }
  Fp blind_acc = fd_add(final_blind, fd_mul(s_blind, xi));
  fill_powers_launch(d_bvec, n, x3, c->stream);
  hipLaunchKernelGGL(k_fill_const, dim3(opn_grid(n)), dim3(256), 0, c->stream, d_wfold, n,
                     one);
  st_.mark("ipa_setup");
  double tm_msm = 0, tm_host = 0;
  auto lap = [&](int which) {
    if (st_.on) {
      hipStreamSynchronize(c->stream);
      double t = StageTimer::now();
      (which ? tm_msm : tm_host) += t - st_.last;
      st_.last = t;
    }
  };
  Fp a_final;
  {
    int rc = ipa_rounds_dev(
        c, pd, d.k, d_pp, d_bvec, d_wfold, pk.utab, pk.wtab, blind_acc, a_final,
        [&](Fp& l_rand, Fp& r_rand) {
          l_rand = rng.field<FpCfg>();
          r_rand = rng.field<FpCfg>();
        },
        [&](const VestaAff& La, const VestaAff& Ra, Fp& uch) {
          if (ts.write_point(La)) return (int)TG_ERR_BADARG;
          if (ts.write_point(Ra)) return (int)TG_ERR_BADARG;
          uch = ts.squeeze();
          return 0;
        },
        lap);
    if (rc) return rc;
  }
  if (st_.on)
    fprintf(stderr, "# ipa-split host=%.1f msm=%.1f ms\n", tm_host * 1e3, tm_msm * 1e3);
  st_.mark("ipa");
  ts.write_scalar(a_final);
  ts.write_scalar(blind_acc);
  proof_out = std::move(ts.proof);
  return 0;
}

// seeded CS1 path (round-1 bench/tests convention)
static int pprove(Ctx* c, PPk& pk, const uint8_t inst_seed[32], const uint8_t wit_seed[32],
                  const uint8_t rng_seed[32], std::vector<uint8_t>& proof_out) {
  std::vector<Fp> inst_lag;
  cs1_instance(pk.d, inst_seed, inst_lag);
  std::vector<std::vector<Fp>> advice_lag;
  cs1_witness(pk.d, wit_seed, inst_lag, advice_lag);
  return pprove_core(c, pk, inst_lag, advice_lag, rng_seed, proof_out);
}

// raw-witness path (SURVEY §8b tg_create_proof(witness_blob, ...) shape):
// instance = n_instance_rows x 32B canonical; advice = n_advice x n x 32B
// canonical, column-major (rows >= usable ignored).
static int pprove_raw(Ctx* c, PPk& pk, const uint8_t* instance, const uint8_t* advice,
                      const uint8_t rng_seed[32], std::vector<uint8_t>& proof_out) {
  PDesc& d = pk.d;
  long n = d.n;
  std::vector<Fp> inst_lag(n, fd_zero<FpCfg>());
  for (int r = 0; r < d.n_instance_rows; r++) {
    Fp v;
    memcpy(v.l, instance + 32 * r, 32);
    if (!fd_is_canonical(v)) return TG_ERR_ENCODING;
    inst_lag[r] = fd_to_mont(v);
  }
  std::vector<std::vector<Fp>> advice_lag(d.n_advice, std::vector<Fp>(n));
  int bad = 0;
#ifdef _OPENMP
#pragma omp parallel for schedule(static) collapse(2) reduction(| : bad)
#endif
  for (int col = 0; col < d.n_advice; col++) {
    for (long i = 0; i < n; i++) {
      Fp v;
      memcpy(v.l, advice + ((size_t)col * n + i) * 32, 32);
      if (!fd_is_canonical(v)) bad |= 1;
      advice_lag[col][i] = fd_to_mont(v);
    }
  }
  if (bad) return TG_ERR_ENCODING;
  return pprove_core(c, pk, inst_lag, advice_lag, rng_seed, proof_out);
}

}  // namespace taiga

namespace taiga {

// ---------------- product verifier (mirrors oracle orc_verify) ----------

static Fp plagrange_at(const Fp& x, long i, const Fp& xn, const PPk& pk, long n) {
  Fp wi = fd_one_mont<FpCfg>();
  {
    Fp base = pk.omega;
    long e = i;
    while (e) {
      if (e & 1) wi = fd_mul(wi, base);
      base = fd_sqr(base);
      e >>= 1;
    }
  }
  Fp one = fd_one_mont<FpCfg>();
  Fp num = fd_mul(fd_mul(fd_sub(xn, one), wi), pk.n_inv);
  return fd_mul(num, fd_inv(fd_sub(x, wi)));
}

struct PScalarCtx {
  const PDesc* d;
  const Fp* adv_eval;
  const Fp* fix_eval;
  const Fp* inst_eval;
};

static int pfind_q(const std::vector<PQuery>& qs, uint32_t col, int32_t rot) {
  for (size_t i = 0; i < qs.size(); i++)
    if (qs[i].col == col && qs[i].rot == rot) return (int)i;
  return -1;
}

static bool pexpr_eval_scalar(Fp& out, const PExpr& e, const PScalarCtx& c) {
  Fp stack[TG_MAX_STACK];
  int sp = 0;
  for (const auto& op : e.ops) {
    switch (op.tag) {
      case XCONST: stack[sp++] = c.d->consts[op.a]; break;
      case XFIXED: {
        int q = pfind_q(c.d->fixed_q, op.a, op.b);
        if (q < 0) return false;
        stack[sp++] = c.fix_eval[q];
        break;
      }
      case XADVICE: {
        int q = pfind_q(c.d->advice_q, op.a, op.b);
        if (q < 0) return false;
        stack[sp++] = c.adv_eval[q];
        break;
      }
      case XINSTANCE: {
        int q = pfind_q(c.d->instance_q, op.a, op.b);
        if (q < 0) return false;
        stack[sp++] = c.inst_eval[q];
        break;
      }
      case XADD: stack[sp - 2] = fd_add(stack[sp - 2], stack[sp - 1]); sp--; break;
      case XSUB: stack[sp - 2] = fd_sub(stack[sp - 2], stack[sp - 1]); sp--; break;
      case XMUL: stack[sp - 2] = fd_mul(stack[sp - 2], stack[sp - 1]); sp--; break;
      case XNEG: stack[sp - 1] = fd_neg(stack[sp - 1]); break;
      case XSCALE: stack[sp - 1] = fd_mul(stack[sp - 1], c.d->consts[op.a]); break;
    }
  }
  out = stack[0];
  return true;
}

// [s]*acc + q on host affine points
static VestaAff pmuladd(const VestaAff& acc, const Fp& s, const VestaAff& q) {
  VestaJac r = jac_mul_host(jac_from_aff(acc), s);
  r = jac_add(r, jac_from_aff(q));
  return jac_to_aff(r);
}

// IPA verification "guard" (the accumulated-check pattern of halo2's
// BatchVerifier / Guard, proof.rs:45-54 via SURVEY §8f-3): everything a
// proof's final check needs, as one linear combination of group elements
// that must equal the identity. Guards from many proofs combine with
// random weights into a single check sharing one g-sized MSM.
struct PVGuard {
  std::vector<VestaAff> pts;  // per-proof variable points (commitments,
  std::vector<Fp> scs;        //   S, L/R) with their Mont-form scalars
  Fp u_coeff, w_coeff;        // coefficients of the shared U and W points
  Fp c_fin;                   // scalar on G_final = MSM(s-vector, g)
  std::vector<Fp> uch_inv;    // k inverse IPA challenges (define s-vector)
};

// transcript + scalar phase of verification: parses the proof, recomputes
// the expected quotient eval, and emits the final-check guard. No group
// MSM work happens here (the q_cm / P folds are kept symbolic as scalar
// coefficients on the transcript commitments).
static int pverify_guard(Ctx* c, PPk& pk, const std::vector<Fp>& inst_lag,
                         const uint8_t* proof, size_t proof_len, PVGuard& gd) {
  PDesc& d = pk.d;
  long n = d.n;
  int nchunks = (d.n_perm + d.chunk_len - 1) / d.chunk_len;
  int nlk = d.n_lookups;
  int npieces = (int)(d.ext_n / n);
  ProverDev& pd = pk.pd;
  Transcript ts;
  ts.init_read(proof, proof_len);
  Fp one = fd_one_mont<FpCfg>();

  ts.common_scalar(pk.vk_repr);
  VestaAff inst_cm;
  if (gpu_msm_commit(c, pd, inst_lag.data(), n, c->d_gl, one, c->h_w, inst_cm, &pk.wtab))
    return TG_ERR_HIP;
  ts.common_point(inst_cm);

  std::vector<VestaAff> adv_cm(d.n_advice);
  for (int col = 0; col < d.n_advice; col++)
    if (!ts.read_point(adv_cm[col])) return -101;
  Fp theta = ts.squeeze();
  std::vector<VestaAff> lap_cm(nlk), lsp_cm(nlk);
  for (int l = 0; l < nlk; l++) {
    if (!ts.read_point(lap_cm[l])) return -102;
    if (!ts.read_point(lsp_cm[l])) return -103;
  }
  Fp beta = ts.squeeze();
  Fp gamma = ts.squeeze();
  std::vector<VestaAff> pz_cm(nchunks);
  for (int ch = 0; ch < nchunks; ch++)
    if (!ts.read_point(pz_cm[ch])) return -104;
  std::vector<VestaAff> lz_cm(nlk);
  for (int l = 0; l < nlk; l++)
    if (!ts.read_point(lz_cm[l])) return -105;
  VestaAff rand_cm;
  if (!ts.read_point(rand_cm)) return -106;
  Fp ych = ts.squeeze();
  std::vector<VestaAff> h_cm(npieces);
  for (int pce = 0; pce < npieces; pce++)
    if (!ts.read_point(h_cm[pce])) return -107;
  Fp x = ts.squeeze();
  Fp xn = x;
  for (int i = 0; i < d.k; i++) xn = fd_sqr(xn);

  std::vector<Fp> adv_eval(d.n_advice_q), fix_eval(d.n_fixed_q), sig_eval(d.n_perm);
  Fp rand_eval;
  Fp pz_eval[TG_MAX_CHUNKS][2], pz_last_eval[TG_MAX_CHUNKS], lk_eval[TG_MAX_LOOKUPS][5];
  for (int q = 0; q < d.n_advice_q; q++)
    if (!ts.read_scalar(adv_eval[q])) return -110;
  for (int q = 0; q < d.n_fixed_q; q++)
    if (!ts.read_scalar(fix_eval[q])) return -111;
  if (!ts.read_scalar(rand_eval)) return -112;
  for (int j = 0; j < d.n_perm; j++)
    if (!ts.read_scalar(sig_eval[j])) return -113;
  for (int ch = 0; ch < nchunks; ch++) {
    if (!ts.read_scalar(pz_eval[ch][0])) return -114;
    if (!ts.read_scalar(pz_eval[ch][1])) return -115;
  }
  for (int ch = 0; ch < nchunks - 1; ch++)
    if (!ts.read_scalar(pz_last_eval[ch])) return -116;
  for (int l = 0; l < nlk; l++)
    for (int j = 0; j < 5; j++)
      if (!ts.read_scalar(lk_eval[l][j])) return -117;

  // instance evals (verifier-computed; GPU iNTT + host Horner)
  std::vector<Fp> inst_coeff = inst_lag;
  if (gpu_lag_to_coeff(c, pd, inst_coeff.data(), d.k, pk.n_inv)) return TG_ERR_HIP;
  auto rot_pt = [&](const Fp& xx, int rot) {
    Fp w = fd_one_mont<FpCfg>();
    const Fp& base = rot < 0 ? pk.omega_inv : pk.omega;
    for (int i = 0; i < (rot < 0 ? -rot : rot); i++) w = fd_mul(w, base);
    return fd_mul(xx, w);
  };
  std::vector<Fp> inst_eval(d.n_instance_q);
  for (int q = 0; q < d.n_instance_q; q++)
    inst_eval[q] = ppoly_eval(inst_coeff.data(), n, rot_pt(x, d.instance_q[q].rot));

  // expected h eval via the shared fold
  Fp expected_h;
  {
    PScalarCtx sc{&d, adv_eval.data(), fix_eval.data(), inst_eval.data()};
    Fp gate_vals[TG_MAX_GATES];
    for (int g = 0; g < d.n_gates; g++)
      if (!pexpr_eval_scalar(gate_vals[g], d.gates[g], sc)) return -120;
    Fp perm_colvals[TG_MAX_PERM], sigma_vals[TG_MAX_PERM];
    for (int jj = 0; jj < d.n_perm; jj++) {
      auto [kind, idx] = d.perm_cols[jj];
      int q;
      if (kind == 0) {
        q = pfind_q(d.advice_q, idx, 0);
        if (q < 0) return -121;
        perm_colvals[jj] = adv_eval[q];
      } else if (kind == 1) {
        q = pfind_q(d.fixed_q, idx, 0);
        if (q < 0) return -122;
        perm_colvals[jj] = fix_eval[q];
      } else {
        q = pfind_q(d.instance_q, idx, 0);
        if (q < 0) return -123;
        perm_colvals[jj] = inst_eval[q];
      }
      sigma_vals[jj] = sig_eval[jj];
    }
    Fp lk[TG_MAX_LOOKUPS][7];
    for (int l = 0; l < nlk; l++) {
      lk[l][0] = lk_eval[l][0];
      lk[l][1] = lk_eval[l][1];
      lk[l][2] = lk_eval[l][2];
      lk[l][3] = lk_eval[l][3];
      lk[l][4] = lk_eval[l][4];
      Fp acc = fd_zero<FpCfg>();
      for (const auto& e : d.lookups[l].in) {
        Fp v;
        if (!pexpr_eval_scalar(v, e, sc)) return -124;
        acc = fd_add(fd_mul(acc, theta), v);
      }
      lk[l][5] = acc;
      acc = fd_zero<FpCfg>();
      for (const auto& e : d.lookups[l].tab) {
        Fp v;
        if (!pexpr_eval_scalar(v, e, sc)) return -125;
        acc = fd_add(fd_mul(acc, theta), v);
      }
      lk[l][6] = acc;
    }
    Fp l0 = plagrange_at(x, 0, xn, pk, n);
    Fp llast = plagrange_at(x, d.usable, xn, pk, n);
    Fp lblind = fd_zero<FpCfg>();
    for (long i = d.usable + 1; i < n; i++)
      lblind = fd_add(lblind, plagrange_at(x, i, xn, pk, n));
    Fp lactive = fd_sub(one, fd_add(llast, lblind));
    Fp zp[TG_MAX_CHUNKS][2], zp_last[TG_MAX_CHUNKS];
    for (int ch = 0; ch < nchunks; ch++) {
      zp[ch][0] = pz_eval[ch][0];
      zp[ch][1] = pz_eval[ch][1];
      zp_last[ch] = ch < nchunks - 1 ? pz_last_eval[ch] : fd_zero<FpCfg>();
    }
    std::vector<Fp> dpow(d.n_perm);
    dpow[0] = fd_one_mont<FpCfg>();
    for (int jj = 1; jj < d.n_perm; jj++) dpow[jj] = fd_mul(dpow[jj - 1], pk.delta);
    PHRow hr{&d, beta, gamma, ych, x, l0, llast, lactive, gate_vals, perm_colvals,
             sigma_vals, (const Fp(*)[2])zp, zp_last, (const Fp(*)[7])lk, dpow.data()};
    Fp acc = ph_fold_row(hr);
    expected_h = fd_mul(acc, fd_inv(fd_sub(xn, one)));
  }

  // multiopen verification (commitments; same query order as pprove)
  Fp x_next = rot_pt(x, 1), x_prev = rot_pt(x, -1), x_last = rot_pt(x, -(d.bf + 1));
  std::vector<VestaAff> pcm;
  std::vector<PMQuery> queries;
  auto addc = [&](const VestaAff& cm) {
    pcm.push_back(cm);
    return (int)pcm.size() - 1;
  };
  auto add_q = [&](int pid, const Fp& pt, const Fp& ev) {
    queries.push_back({pid, pt, ev});
  };
  int pid_inst = addc(inst_cm);
  std::vector<int> pid_adv(d.n_advice);
  for (int col = 0; col < d.n_advice; col++) pid_adv[col] = addc(adv_cm[col]);
  std::vector<int> pid_pz(nchunks);
  for (int ch = 0; ch < nchunks; ch++) pid_pz[ch] = addc(pz_cm[ch]);
  std::vector<int> pid_lz(nlk), pid_lap(nlk), pid_lsp(nlk);
  for (int l = 0; l < nlk; l++) {
    pid_lz[l] = addc(lz_cm[l]);
    pid_lap[l] = addc(lap_cm[l]);
    pid_lsp[l] = addc(lsp_cm[l]);
  }
  std::vector<int> pid_fix(d.n_fixed);
  for (int col = 0; col < d.n_fixed; col++) pid_fix[col] = addc(pk.fixed_commits[col]);
  std::vector<int> pid_sig(d.n_perm);
  for (int j = 0; j < d.n_perm; j++) pid_sig[j] = addc(pk.sigma_commits[j]);
  VestaAff h_col_cm = h_cm[npieces - 1];
  for (int pce = npieces - 2; pce >= 0; pce--) h_col_cm = pmuladd(h_col_cm, xn, h_cm[pce]);
  int pid_h = addc(h_col_cm);
  int pid_rand = addc(rand_cm);

  for (int q = 0; q < d.n_instance_q; q++)
    add_q(pid_inst, rot_pt(x, d.instance_q[q].rot), inst_eval[q]);
  for (int q = 0; q < d.n_advice_q; q++)
    add_q(pid_adv[d.advice_q[q].col], rot_pt(x, d.advice_q[q].rot), adv_eval[q]);
  for (int ch = 0; ch < nchunks; ch++) {
    add_q(pid_pz[ch], x, pz_eval[ch][0]);
    add_q(pid_pz[ch], x_next, pz_eval[ch][1]);
  }
  for (int ch = 0; ch < nchunks - 1; ch++) add_q(pid_pz[ch], x_last, pz_last_eval[ch]);
  for (int l = 0; l < nlk; l++) {
    add_q(pid_lz[l], x, lk_eval[l][0]);
    add_q(pid_lap[l], x, lk_eval[l][2]);
    add_q(pid_lsp[l], x, lk_eval[l][4]);
    add_q(pid_lap[l], x_prev, lk_eval[l][3]);
    add_q(pid_lz[l], x_next, lk_eval[l][1]);
  }
  for (int q = 0; q < d.n_fixed_q; q++)
    add_q(pid_fix[d.fixed_q[q].col], rot_pt(x, d.fixed_q[q].rot), fix_eval[q]);
  for (int j = 0; j < d.n_perm; j++) add_q(pid_sig[j], x, sig_eval[j]);
  add_q(pid_h, x, expected_h);
  add_q(pid_rand, x, rand_eval);

  Fp x1 = ts.squeeze();
  Fp x2 = ts.squeeze();
  int NP = (int)pcm.size();
  std::vector<int> order;
  std::vector<int> poly_set(NP, -1);
  std::vector<std::vector<Fp>> ppts(NP), pevs(NP);
  for (const auto& q : queries) {
    if (ppts[q.poly_id].empty()) order.push_back(q.poly_id);
    ppts[q.poly_id].push_back(q.point);
    pevs[q.poly_id].push_back(q.eval);
  }
  std::vector<std::vector<Fp>> set_pts;
  for (int pid : order) {
    int found = -1;
    for (size_t s = 0; s < set_pts.size(); s++) {
      if (set_pts[s].size() != ppts[pid].size()) continue;
      bool eq = true;
      for (size_t j = 0; j < set_pts[s].size(); j++)
        if (!fd_eq(set_pts[s][j], ppts[pid][j])) { eq = false; break; }
      if (eq) { found = (int)s; break; }
    }
    if (found < 0) {
      found = (int)set_pts.size();
      set_pts.push_back(ppts[pid]);
    }
    poly_set[pid] = found;
  }
  int n_sets = (int)set_pts.size();
  std::vector<std::vector<int>> set_pids(n_sets);
  std::vector<std::vector<Fp>> q_ev(n_sets);
  for (int s = 0; s < n_sets; s++) q_ev[s].assign(set_pts[s].size(), fd_zero<FpCfg>());
  for (int pid : order) {
    int s = poly_set[pid];
    set_pids[s].push_back(pid);
    for (size_t j = 0; j < q_ev[s].size(); j++)
      q_ev[s][j] = fd_add(fd_mul(q_ev[s][j], x1), pevs[pid][j]);
  }
  VestaAff f_cm;
  if (!ts.read_point(f_cm)) return -130;
  Fp x3 = ts.squeeze();
  std::vector<Fp> q_at_x3(n_sets);
  for (int s = 0; s < n_sets; s++)
    if (!ts.read_scalar(q_at_x3[s])) return -131;
  Fp x4 = ts.squeeze();
  Fp f_val = fd_zero<FpCfg>();
  for (int s = 0; s < n_sets; s++) {
    Fp r = fd_zero<FpCfg>();
    for (size_t j = 0; j < set_pts[s].size(); j++) {
      Fp term = q_ev[s][j];
      Fp den = one;
      for (size_t m2 = 0; m2 < set_pts[s].size(); m2++) {
        if (m2 == j) continue;
        term = fd_mul(term, fd_sub(x3, set_pts[s][m2]));
        den = fd_mul(den, fd_sub(set_pts[s][j], set_pts[s][m2]));
      }
      r = fd_add(r, fd_mul(term, fd_inv(den)));
    }
    Fp num = fd_sub(q_at_x3[s], r);
    Fp den = one;
    for (const Fp& pt : set_pts[s]) den = fd_mul(den, fd_sub(x3, pt));
    num = fd_mul(num, fd_inv(den));
    f_val = s == 0 ? num : fd_add(fd_mul(f_val, x2), num);
  }
  // symbolic fold of P = ((f_cm·x4 + q_cm[0])·x4 + q_cm[1])·x4 + …:
  // coefficient x4^{n_sets-1-s} on each q_cm[s], x4^{n_sets} on f_cm, and
  // q_cm[s] = Σ_i pcm[m_i]·x1^{t-1-i} over that set's members in order.
  std::vector<Fp> set_coef(n_sets);
  Fp x4p = one;
  for (int s = n_sets - 1; s >= 0; s--) {
    set_coef[s] = x4p;
    x4p = fd_mul(x4p, x4);
  }
  Fp f_coef = x4p;  // x4^{n_sets}
  std::vector<Fp> pid_coef(NP);
  for (int s = 0; s < n_sets; s++) {
    int t = (int)set_pids[s].size();
    Fp x1p = one;
    for (int i = t - 1; i >= 0; i--) {
      pid_coef[set_pids[s][i]] = fd_mul(x1p, set_coef[s]);
      x1p = fd_mul(x1p, x1);
    }
  }
  Fp v = f_val;
  for (int s = 0; s < n_sets; s++) v = fd_add(fd_mul(v, x4), q_at_x3[s]);
  // IPA rounds
  VestaAff S;
  if (!ts.read_point(S)) return -132;
  Fp xi = ts.squeeze();
  gd.pts.clear();
  gd.scs.clear();
  gd.pts.reserve(NP + 2 + 2 * d.k);
  gd.scs.reserve(NP + 2 + 2 * d.k);
  gd.pts.push_back(f_cm);
  gd.scs.push_back(f_coef);
  for (int pid = 0; pid < NP; pid++) {
    gd.pts.push_back(pcm[pid]);
    gd.scs.push_back(pid_coef[pid]);
  }
  gd.pts.push_back(S);
  gd.scs.push_back(xi);
  std::vector<Fp> uch(d.k), uch_inv(d.k);
  for (int round = 0; round < d.k; round++) {
    VestaAff L, R;
    if (!ts.read_point(L)) return -133;
    if (!ts.read_point(R)) return -134;
    uch[round] = ts.squeeze();
    uch_inv[round] = fd_inv(uch[round]);
    gd.pts.push_back(L);
    gd.scs.push_back(uch[round]);
    gd.pts.push_back(R);
    gd.scs.push_back(uch_inv[round]);
  }
  Fp c_fin, f_syn;
  if (!ts.read_scalar(c_fin)) return -135;
  if (!ts.read_scalar(f_syn)) return -136;
  if (ts.rpos != ts.rlen) return -137;
  Fp b_fin = one;
  {
    std::vector<Fp> xp(d.k);
    xp[d.k - 1] = x3;
    for (int j = d.k - 2; j >= 0; j--) xp[j] = fd_sqr(xp[j + 1]);
    for (int j = 0; j < d.k; j++)
      b_fin = fd_mul(b_fin, fd_add(fd_mul(uch_inv[j], xp[j]), one));
  }
  // the check is lhs − rhs == identity:
  //   lhs = P + ξ·S + v·U + Σ(u_j·L_j + u_j⁻¹·R_j)
  //   rhs = c·G_final + c·b·U + f_syn·W
  Fp zero = fd_zero<FpCfg>();
  gd.u_coeff = fd_sub(v, fd_mul(c_fin, b_fin));
  gd.w_coeff = fd_sub(zero, f_syn);
  gd.c_fin = c_fin;  // folded NEGATED into the combined s-vector
  gd.uch_inv = uch_inv;
  return 0;
}

// host Pippenger (c=8, OpenMP over the 32 windows) for the guards' variable
// points — a few hundred points; the n-sized g MSM stays on the GPU. Safe
// for duplicate/identity points (generic jacobian adds).
static VestaJac pv_var_msm(const std::vector<VestaAff>& pts, const std::vector<Fp>& scs_mont) {
  long nn = (long)pts.size();
  std::vector<Fp> sc(nn);
  for (long i = 0; i < nn; i++) sc[i] = fd_from_mont(scs_mont[i]);
  const int NW = 32;  // 32 windows x 8 bits cover the 255-bit scalars
  std::vector<VestaJac> wsum(NW);
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic)
#endif
  for (int w = 0; w < NW; w++) {
    VestaJac buckets[255];
    for (int b = 0; b < 255; b++) buckets[b] = jac_identity<FqCfg>();
    int limb = w / 8, off = (w % 8) * 8;
    for (long i = 0; i < nn; i++) {
      int dig = (int)((sc[i].l[limb] >> off) & 0xFF);
      if (dig && !aff_is_identity(pts[i]))
        buckets[dig - 1] = jac_add(buckets[dig - 1], jac_from_aff(pts[i]));
    }
    VestaJac run = jac_identity<FqCfg>(), tot = jac_identity<FqCfg>();
    for (int b = 254; b >= 0; b--) {
      run = jac_add(run, buckets[b]);
      tot = jac_add(tot, run);
    }
    wsum[w] = tot;
  }
  VestaJac acc = jac_identity<FqCfg>();
  for (int w = NW - 1; w >= 0; w--) {
    for (int dd = 0; dd < 8; dd++) acc = jac_dbl(acc);
    acc = jac_add(acc, wsum[w]);
  }
  return acc;
}

// combined evaluation of m guards with random weights rho (rho[0] may be 1):
// Σ_i rho_i·guard_i must be the identity. One GPU MSM over the resident g
// bases covers every proof's G_final (s-vectors are weight-summed on host).
static int pverify_eval(Ctx* c, PPk& pk, const PVGuard* gds, int m, const Fp* rho) {
  PDesc& d = pk.d;
  long n = d.n;
  Fp zero = fd_zero<FpCfg>();
  std::vector<Fp> svec(n, zero);
  for (int i = 0; i < m; i++) {
    Fp w = fd_sub(zero, fd_mul(rho[i], gds[i].c_fin));  // −rho·c (rhs side)
    const Fp* ui = gds[i].uch_inv.data();
#ifdef _OPENMP
#pragma omp parallel for schedule(static)
#endif
    for (long j = 0; j < n; j++) {
      Fp s = w;
      for (int b = 0; b < d.k; b++)
        if ((j >> (d.k - 1 - b)) & 1) s = fd_mul(s, ui[b]);
      svec[j] = fd_add(svec[j], s);
    }
  }
  VestaAff gcomb;
  if (gpu_msm_commit(c, pk.pd, svec.data(), n, c->d_g, zero, c->h_w, gcomb, &pk.wtab))
    return TG_ERR_HIP;
  std::vector<VestaAff> pts;
  std::vector<Fp> scs;
  Fp ucoef = zero, wcoef = zero;
  for (int i = 0; i < m; i++) {
    for (size_t j = 0; j < gds[i].pts.size(); j++) {
      pts.push_back(gds[i].pts[j]);
      scs.push_back(fd_mul(rho[i], gds[i].scs[j]));
    }
    ucoef = fd_add(ucoef, fd_mul(rho[i], gds[i].u_coeff));
    wcoef = fd_add(wcoef, fd_mul(rho[i], gds[i].w_coeff));
  }
  VestaJac acc = pv_var_msm(pts, scs);
  acc = jac_add(acc, jac_from_aff(gcomb));
  if (!fd_is_zero(ucoef)) acc = jac_add(acc, pk.utab.mul(ucoef));
  if (!fd_is_zero(wcoef)) acc = jac_add(acc, pk.wtab.mul(wcoef));
  return jac_is_identity(acc) ? 0 : -1;
}

// canonical instance rows -> full Lagrange instance column (Mont)
static int pinst_from_raw(const PDesc& d, const uint8_t* instance,
                          std::vector<Fp>& inst_lag) {
  inst_lag.assign(d.n, fd_zero<FpCfg>());
  for (int r = 0; r < d.n_instance_rows; r++) {
    Fp v;
    memcpy(v.l, instance + 32 * r, 32);
    if (!fd_is_canonical(v)) return TG_ERR_ENCODING;
    inst_lag[r] = fd_to_mont(v);
  }
  return 0;
}

static int pverify(Ctx* c, PPk& pk, const uint8_t inst_seed[32], const uint8_t* proof,
                   size_t proof_len) {
  PVGuard gd;
  std::vector<Fp> inst_lag;
  cs1_instance(pk.d, inst_seed, inst_lag);
  int rc = pverify_guard(c, pk, inst_lag, proof, proof_len, gd);
  if (rc) return rc;
  Fp one = fd_one_mont<FpCfg>();
  return pverify_eval(c, pk, &gd, 1, &one);
}

// raw-instance verification (the real drop-in shape: instances are data,
// not seeds — mirrors plonk::verify_proof's instance slices, proof.rs:45-54)
static int pverify_raw(Ctx* c, PPk& pk, const uint8_t* instance, const uint8_t* proof,
                       size_t proof_len) {
  PVGuard gd;
  std::vector<Fp> inst_lag;
  int rc = pinst_from_raw(pk.d, instance, inst_lag);
  if (rc) return rc;
  rc = pverify_guard(c, pk, inst_lag, proof, proof_len, gd);
  if (rc) return rc;
  Fp one = fd_one_mont<FpCfg>();
  return pverify_eval(c, pk, &gd, 1, &one);
}

}  // namespace taiga

