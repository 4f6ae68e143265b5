// msm_probe_common.hpp — what msm_reduce_probe.cpp and msm_fb_probe.cpp share:
// known multiples of the generator to fill buckets with, and the host mirror
// of the MSM bucket reduction of msm.hip. TEST CODE. Calls no HIP runtime
// function.
#pragma once

#include <cstdlib>
#include <vector>

#include "pasta_device.hpp"
#include "msm.hip"

using namespace taiga;

static u64 sm64(u64 x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

static VestaJac mul_small(const VestaJac& p, u64 k) {
  VestaJac acc = jac_identity<FqCfg>(), base = p;
  while (k) {
    if (k & 1) acc = jac_add(acc, base);
    base = jac_dbl(base);
    k >>= 1;
  }
  return acc;
}

// pts[i] = [sm64(0xC0FFEE + i)]G
static VestaJac pts[16];

static void make_table() {
  Fq one = fd_one_mont<FqCfg>();
  VestaAff G;
  G.x = fd_neg(one);  // generator (-1, 2)
  G.y = fd_add(one, one);
  for (int i = 0; i < 16; i++) pts[i] = mul_small(jac_from_aff(G), sm64(0xC0FFEEull + i));
}

// k_bucket_segsum and k_window_sum<KMAX> with loops in place of lanes and
// blocks: sets bucket sets of N buckets each, segments of s, one sum per set
template <int KMAX>
static std::vector<VestaJac> reduce(const std::vector<VestaJac>& buckets, int sets, int N, int s) {
  const int M = N / s, Wd = msm_ws_width(M), K = M / Wd;
  const int lgs = msm_lg2(s), lanes = MSM_WS_TERMS * KMAX;
  if (K > KMAX) abort();  // msm_run would have picked the wider kernel
  // memory a kernel does not write starts out as garbage (a non-identity
  // point): a slot read before it is written shows up in the result
  std::vector<VestaJac> partials((size_t)sets * K * MSM_CHUNK_OUT, pts[9]), sums(sets);
  for (u64 q = 0; q < (u64)sets * K; q++) {  // k_bucket_segsum, block q
    std::vector<VestaJac> lds(2 * MSM_WS_WIDTH, pts[9]);
    VestaJac* C = lds.data();
    VestaJac* T = C + MSM_WS_WIDTH;
    for (int tid = 0; tid < MSM_WS_WIDTH; tid++) msm_chunk_load(buckets.data(), N, s, q, tid, C, T);
    for (int off = Wd / 2; off >= 1; off >>= 1)
      for (int tid = 0; tid < MSM_WS_WIDTH; tid++) msm_chunk_step(C, T, Wd, off, tid);
    for (int tid = 0; tid < MSM_WS_WIDTH; tid++) msm_chunk_store(C, T, Wd, q, tid, partials.data());
  }
  for (int w = 0; w < sets; w++) {  // k_window_sum<KMAX>, block w
    std::vector<VestaJac> X(lanes, pts[9]), v(MSM_WS_TERMS);
    for (int tid = 0; tid < lanes; tid++)
      X[tid] = msm_wsum_input<KMAX>(partials.data() + (size_t)w * K * MSM_CHUNK_OUT, Wd, K, tid);
    for (int off = K / 2; off >= 1; off >>= 1)
      for (int tid = 0; tid < lanes; tid++)
        if ((tid & (KMAX - 1)) < off) X[tid] = jac_add(X[tid], X[tid + off]);
    for (int e = 0; e < MSM_WS_TERMS; e++) v[e] = msm_wsum_scale(X[e * KMAX], Wd, K, lgs, e);
    for (int e = 0; e < MSM_WS_TERMS; e++) X[e] = v[e];
    for (int off = MSM_WS_TERMS / 2; off >= 1; off >>= 1)
      for (int tid = 0; tid < off; tid++) X[tid] = jac_add(X[tid], X[tid + off]);
    sums[w] = X[0];
  }
  return sums;
}
