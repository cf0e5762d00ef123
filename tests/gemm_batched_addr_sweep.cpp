// TEST INFRASTRUCTURE of tests/test_gemm_batched_addr.py: the loops of capital_amd/csrc/gemm_batched.hip (gm_macro, gm_wave, gm_group)
// replayed on the CPU, lane by lane, with the address functions the kernels themselves call (capital_amd/csrc/gemm_batched_addr.h).
// Reads one wavefront / workgroup per line from stdin:
//   group NP n a_kcontig b_kcontig lda ldb ldc G  m_0 k_0 ... m_(G-1) k_(G-1)
// group = 1: one block per workgroup (G = 1, NP = 64), macro tiles of 64 x 32 dealt over the waves; group = 0: a wavefront of G = 64 / NP
// blocks, passes of NP columns.  Block j of the line has m_j rows and contraction length k_j (0 0: a dead group at the tail of a grid).
// Checks: every addressed offset of op(A), op(B) and C decodes to an element inside the operand's m x k, k x n or m x n extent; every
// element of every C rectangle is addressed exactly once.  Prints the number of lines, loads and stores; exits 1 on the first finding.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gemm_batched_addr.h"

static long long loads = 0, stores = 0, line_no = 0;

static void fail(const char* what, long long off, int lane, int s, long long q) {
  std::printf("line %lld: %s: offset %lld lane %d slab %d k step %lld\n", line_no, what, off, lane, s, q);
  std::exit(1);
}

// the element (i, qq) a lane is to supply, worked out here on its own, against the offset the library's function gave: inside the extent
// (i < lim, qq < k <= the stored extent) and at the column-major place of the operand as stored
static void check_load(bool kcontig, long long ld, long long off, int i, long long qq, int lim, long long k, const char* what, int lane, int s, long long q) {
  const long long want = kcontig ? qq + (long long)i * ld : i + qq * ld;
  if (i < 0 || i >= lim || qq < 0 || qq >= k || off != want || (kcontig ? k : (long long)lim) > ld) fail(what, off, lane, s, q);
  loads++;
}

struct Blk { int m; long long k; std::vector<int> seen; };

static void macro(int NP, int NJ, int I0, int J0, int n, bool akc, bool bkc, long long lda, long long ldb, long long ldc, std::vector<Blk>& blk, int mmax,
                  long long kmax) {
  const long long a_si = gm_stride_i(akc, lda), a_sq = gm_stride_q(akc, lda), b_si = gm_stride_i(bkc, ldb), b_sq = gm_stride_q(bkc, ldb);
  for (int lane = 0; lane < 64; lane++) {
    const int lr = lane & 15;
    for (long long q = 0; q < kmax; q += 4) {            // the groups of GM_U steps and the tail visit the same q
      for (int s = 0; s < 4; s++) {
        if (!gm_slab_on(NP, I0, s, mmax)) continue;
        const Blk& b = blk[gm_sub(NP, s * 16 + lr)];
        const GmAt at = gm_load_at(a_si, a_sq, b.m, b.k, NP, I0, s, lane, q);
        if (at.on) check_load(akc, lda, at.off, I0 + (s * 16 + lr) % NP, q + lane / 16, b.m, b.k, "op(A)", lane, s, q);
      }
      for (int s = 0; s < NJ; s++) {
        if (!gm_slab_on(NP, J0, s, n)) continue;
        const Blk& b = blk[gm_sub(NP, s * 16 + lr)];
        const int bn = b.m > 0 ? n : 0;                  // a dead group has n = 0 as well
        const GmAt at = gm_load_at(b_si, b_sq, bn, b.k, NP, J0, s, lane, q);
        if (at.on) check_load(bkc, ldb, at.off, J0 + (s * 16 + lr) % NP, q + lane / 16, bn, b.k, "op(B)", lane, s, q);
      }
    }
    for (int si = 0; si < 4; si++)
      for (int sj = 0; sj < NJ; sj++) {
        if (!gm_tile(NP, si, sj) || !gm_slab_on(NP, I0, si, mmax) || !gm_slab_on(NP, J0, sj, n)) continue;
        Blk& b = blk[gm_sub(NP, si * 16 + lr)];
        const int bn = b.m > 0 ? n : 0;
        for (int r = 0; r < 4; r++) {
          const GmAt at = gm_store_at(b.m, bn, ldc, NP, I0, J0, si, sj, lane, r);
          if (!at.on) continue;
          if (at.off < 0) fail("C", at.off, lane, si, sj);
          const long long row = at.off % ldc, col = at.off / ldc;
          if (row >= b.m || col >= bn) fail("C", at.off, lane, si, sj);
          b.seen[(size_t)(row + col * b.m)]++;
          stores++;
        }
      }
  }
}

int main() {
  int group, NP, n, akc, bkc, G;
  long long lda, ldb, ldc;
  while (std::scanf("%d %d %d %d %d %lld %lld %lld %d", &group, &NP, &n, &akc, &bkc, &lda, &ldb, &ldc, &G) == 9) {
    line_no++;
    std::vector<Blk> blk((size_t)G);
    int mmax = 0;
    long long kmax = 0;
    for (Blk& b : blk) {
      if (std::scanf("%d %lld", &b.m, &b.k) != 2) { std::printf("line %lld: short\n", line_no); return 1; }
      b.seen.assign((size_t)b.m * (size_t)n, 0);
      mmax = std::max(mmax, b.m);
      kmax = std::max(kmax, b.k);
    }
    if (n > GM_MAX || mmax > GM_MAX || (group ? G != 1 || NP != 64 : G != 64 / NP || mmax > NP)) { std::printf("line %lld: not a launch the library makes\n", line_no); return 1; }
    if (group) {
      const int nt = gm_group_tiles(mmax, n);
      for (int wave = 0; wave < 4; wave++)
        for (int t = wave; t < nt; t += 4) macro(64, GM_GROUP_NJ, gm_group_I0(t, mmax), gm_group_J0(t, mmax), n, akc, bkc, lda, ldb, ldc, blk, mmax, kmax);
    } else {
      for (int pass = 0; pass < gm_wave_passes(NP, n); pass++) macro(NP, 4, 0, pass * NP, n, akc, bkc, lda, ldb, ldc, blk, mmax, kmax);
    }
    for (size_t j = 0; j < blk.size(); j++)
      for (size_t e = 0; e < blk[j].seen.size(); e++)
        if (blk[j].seen[e] != 1) {
          std::printf("line %lld: block %zu: element %zu of C is addressed %d times\n", line_no, j, e, blk[j].seen[e]);
          return 1;
        }
  }
  std::printf("ok %lld %lld %lld\n", line_no, loads, stores);
  return 0;
}
