// desc_probe.cpp — host-side probe of the TGD1 parser (pdesc_parse in
// prover_impl.hpp) and of the gate-kernel source generator and its cache key
// (hf_rtc.hpp). TEST CODE: built with the host sanitizers and driven by
// tests/test_desc_parse.py. Calls no HIP runtime function, so it runs on a
// machine without a GPU.
//
// argv[1] names a file of records; one output line per record ('R' apart).
//   'P' u32 len, blob
//       parse            -> "accept <the 15 header words> src=<n>" | "reject"
//       (src = length of the generated hf_gates source, 0 = none)
//   'S' u32 len, blob, u32 gate, u32 nops, nops * (u32 tag, u32 a, i32 b)
//       parse (must accept), REPLACE that gate's postfix behind the parser's
//       back, generate   -> "src <n> <1 if the text is a whole kernel>"
//   'K' u32 len, blob
//       cache paths      -> "key <default> <one prelude character changed>
//                            <default again>"
//   'C'                  -> "caps <the TG_MAX_* constants>"
//   'R'                  -> the text of hf_rtc_prelude(), as it is (many lines)
// Every blob is copied into a heap block of exactly len bytes, so a read
// past the end is a sanitizer report, not luck.

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pasta_device.hpp"
#include "host_crypto.hpp"
#include "prover_impl.hpp"
#include "hf_rtc.hpp"

using namespace taiga;

struct Reader {
  const std::vector<uint8_t>& v;
  size_t pos = 0;
  bool take(void* dst, size_t n) {
    if (v.size() - pos < n) return false;
    memcpy(dst, v.data() + pos, n);
    pos += n;
    return true;
  }
};

static bool whole_kernel(const std::string& s) {
  long depth = 0;
  for (char c : s) {
    if (c == '{') depth++;
    if (c == '}' && --depth < 0) return false;
  }
  return depth == 0 && s.find("void __launch_bounds__(256) hf_gates(") != std::string::npos &&
         s.size() > 2 && s.compare(s.size() - 2, 2, "}\n") == 0;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> all;
  uint8_t buf[1 << 16];
  for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) all.insert(all.end(), buf, buf + n);
  fclose(f);
  Reader r{all};
  uint8_t mode;
  while (r.take(&mode, 1)) {
    if (mode == 'C') {
      printf("caps %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", TG_MAX_K,
             TG_MAX_EXT_RATIO, TG_MAX_FIXED, TG_MAX_ADVICE, TG_MAX_INSTANCE, TG_MAX_GATES,
             TG_MAX_PERM, TG_MAX_CHUNKS, TG_MAX_LOOKUPS, TG_MAX_LK_EXPRS, TG_MAX_QUERIES,
             TG_MAX_INSTANCE_Q, TG_MAX_STACK, TG_MAX_COL_POINTS, TG_MAX_POINT_SETS);
      continue;
    }
    if (mode == 'R') {
      std::string pre = hf_rtc_prelude();
      fwrite(pre.data(), 1, pre.size(), stdout);
      continue;
    }
    uint32_t len;
    if (!r.take(&len, 4) || all.size() - r.pos < len) return 3;
    uint8_t* blob = (uint8_t*)malloc(len ? len : 1);
    r.take(blob, len);
    PDesc* d = new PDesc();
    bool ok = pdesc_parse(*d, blob, len);
    if (mode == 'P') {
      if (!ok) {
        printf("reject\n");
      } else {
        printf("accept %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d src=%zu\n", d->k, d->ext_k,
               d->n_fixed, d->n_advice, d->n_instance, d->bf, d->n_gates, d->n_perm,
               d->chunk_len, d->n_lookups, d->n_consts, d->n_advice_q, d->n_fixed_q,
               d->n_instance_q, d->n_instance_rows, hf_rtc_source(*d).size());
      }
    } else if (mode == 'S') {
      uint32_t gate, nops;
      if (!ok || !r.take(&gate, 4) || !r.take(&nops, 4) || gate >= d->gates.size()) return 4;
      std::vector<ExprOp> ops(nops);
      for (auto& op : ops)
        if (!r.take(&op.tag, 4) || !r.take(&op.a, 4) || !r.take(&op.b, 4)) return 4;
      d->gates[gate].ops = ops;
      std::string src = hf_rtc_source(*d);
      printf("src %zu %d\n", src.size(), src.empty() ? 0 : (int)whole_kernel(src));
    } else if (mode == 'K') {
      if (!ok) return 5;
      std::string pre = hf_rtc_prelude();
      std::string src = hf_rtc_source(*d);
      std::string pre2 = pre;
      pre2[pre2.size() / 2] ^= 1;  // one character of the prelude
      std::string src2 = hf_rtc_source(*d, pre2);
      printf("key %s %s %s\n", hf_cache_path(hf_cache_key(*d, src)).c_str(),
             hf_cache_path(hf_cache_key(*d, src2)).c_str(),
             hf_cache_path(hf_cache_key(*d, hf_rtc_source(*d, pre))).c_str());
    } else {
      return 6;
    }
    delete d;
    free(blob);
  }
  return 0;
}
