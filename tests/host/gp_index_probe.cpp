// gp_index_probe — the index arithmetic of grand_products.hip on the host.
// The kernels address memory only through the TG_HD functions gp_inv_index,
// gp_blocks_for, gp_scan_lo and gp_scan_hi; this program walks them the way
// the kernels do, over heap arrays of EXACTLY the sizes the launchers
// allocate, so that an index outside them is an AddressSanitizer report.
// Built by tests/test_gp_index_host.py with -fsanitize=address,undefined.
//
// usage: gp_index_probe COUNT...   one line per count:
//   "<count> inv=<elements touched once> scan=<elements touched once>"
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "grand_products.hip"

using namespace taiga;

int main(int argc, char** argv) {
  printf("GP_B=%d GP_E=%d GP_T=%d\n", GP_B, GP_E, GP_T);
  for (int a = 1; a < argc; a++) {
    long count = atol(argv[a]);
    if (count < 1) return 2;
    // k_gp_batch_inverse: grid gp_blocks_for(count), every thread its GP_E
    // elements, those at or past count skipped
    unsigned char* seen = (unsigned char*)calloc((size_t)count, 1);
    long inv_once = 0;
    for (long b = 0; b < gp_blocks_for(count); b++)
      for (int t = 0; t < GP_B; t++)
        for (int m = 0; m < GP_E; m++) {
          long i = gp_inv_index(b, t, m);
          if (i < count) seen[i]++;
        }
    for (long i = 0; i < count; i++) inv_once += seen[i] == 1;
    free(seen);
    // k_gp_scan_reduce / _apply: the launcher cuts count ratios into blocks
    // of at most GP_T; thread t takes [gp_scan_lo, gp_scan_hi) of its block
    // and the block that ends the segment also writes element len
    unsigned char* z = (unsigned char*)calloc((size_t)count + 1, 1);
    long scan_once = 0;
    for (long o = 0; o < count; o += GP_T) {
      int len = (int)(count - o < GP_T ? count - o : GP_T);
      bool last = o + len == count;
      int prev_hi = 0;
      for (int t = 0; t < GP_B; t++) {
        int lo = gp_scan_lo(t, len), hi = gp_scan_hi(t, len);
        if (lo != prev_hi || hi < lo || hi - lo > GP_E) return 3;
        prev_hi = hi;
        for (int i = lo; i < hi; i++) z[o + i]++;
        if (last && hi == len && lo < hi) z[o + len]++;
      }
      if (prev_hi != len) return 4;
    }
    for (long i = 0; i <= count; i++) scan_once += z[i] == 1;
    free(z);
    printf("%ld inv=%ld scan=%ld\n", count, inv_once, scan_once);
  }
  return 0;
}
