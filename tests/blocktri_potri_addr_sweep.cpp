// TEST INFRASTRUCTURE of tests/test_blocktri_potri_addr.py: the loops of bt_inverse (capital_amd/csrc/blocktri_kernels.h) as
// blocktri_potri_batched.hip launches them - the chain of a lane group from bt_chain_fixed, a walk of T steps at position T - 1 - step -
// replayed on the CPU, workgroup by workgroup and lane by lane, with the address functions the kernel itself calls
// (capital_amd/csrc/blocktri_addr.h).  Reads one launch per line from stdin:
//   n T batch fill ldd step_d stride_d lde step_e stride_e eblocks dfirst
// eblocks is the number of coupling blocks per chain the E operand really holds (T - 1 for every launch the library makes) and dfirst the
// first position the D operand really holds (0 for every launch the library makes): a line that says fewer blocks or a later first
// position is a planted fault - the kernel would address a coupling block, or a predecessor, the chain does not have.
// The requests for U and E are replayed where the kernel of the row's NP makes them (early where its registers allow it, see the loop).
// Checks: every access that is `on` decodes to an element inside its block's extent, of the chain the lane (or the wave row) belongs to and
// of the position the loop is at; nothing at position -1 or T (the functions are asked there as the kernel asks them: the answer must be
// `off`), no E at all with T = 1; the lane groups beyond `batch` address nothing; every element of every upper triangle of D and of every E
// block is read exactly once; the written set is exactly the D triangles - the whole D blocks with fill - plus the E blocks, each element
// once; every LDS offset lies inside its area; both exchange areas are cleared word by word exactly once; and every word (row, k) with
// row, k < n of an MFMA operand - G, the mirrored Sigma, C - is written exactly once between the clearing of its area's contents and the
// phase that reads it.  Prints "ok <lines> <global accesses> <LDS accesses>"; exits 1 on the first finding.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "blocktri_addr.h"

static long long line_no = 0, globals = 0, ldss = 0;

static void fail(const char* what, const char* why, long long off, long long wg, int lane, long long pos) {
  std::printf("line %lld: %s: %s: offset %lld workgroup %lld lane %d position %lld\n", line_no, what, why, off, wg, lane, pos);
  std::exit(1);
}

struct Operand {                         // positions first .. blocks - 1 of n x n blocks per chain
  const char* name;
  long long ld, step, stride, blocks, first, batch;
  int n;
  std::vector<int> rd, wr;
  void init() {
    if (blocks <= 0) return;
    if (ld < n) fail(name, "leading dimension below n", ld, -1, -1, -1);
    if (blocks > 1 && step < ld * n) fail(name, "step below one block", step, -1, -1, -1);
    if (batch > 1 && stride < (blocks > 1 ? step * blocks : ld * n)) fail(name, "stride below one chain", stride, -1, -1, -1);
    rd.assign((size_t)(batch * blocks * n * n), 0);
    wr.assign((size_t)(batch * blocks * n * n), 0);
  }
  // the element an offset names; it must be (chain, pos, row, col)
  size_t at(long long off, long long chain, long long pos, int row, int col, bool upper, long long wg, int lane) {
    globals++;
    if (off < 0) fail(name, "negative offset", off, wg, lane, pos);
    if (blocks <= 0) fail(name, "the operand holds no block", off, wg, lane, pos);
    if (chain < 0 || chain >= batch) fail(name, "a dead lane group addresses memory", off, wg, lane, pos);
    if (pos < first || pos >= blocks) fail(name, "position outside the chain", off, wg, lane, pos);
    const long long rem = off - chain * stride - pos * step;
    if (rem < 0 || rem >= ld * n) fail(name, "outside the block", off, wg, lane, pos);
    const int r = (int)(rem % ld), c = (int)(rem / ld);
    if (r >= n || c >= n) fail(name, "a pad row or column", off, wg, lane, pos);
    if (upper && r > c) fail(name, "the strictly lower triangle", off, wg, lane, pos);
    if (r != row || c != col) fail(name, "not the element the loop is at", off, wg, lane, pos);
    return (size_t)(((chain * blocks + pos) * n + c) * n + r);
  }
  void expect(const std::vector<int>& v, bool upper, const char* why) {
    for (long long b = 0; b < batch * blocks; b++)
      for (int c = 0; c < n; c++)
        for (int r = 0; r < n; r++)
          if (v[(size_t)((b * n + c) * n + r)] != ((upper && r > c) ? 0 : 1)) fail(name, why, (b * n + c) * n + r, -1, -1, b % blocks);
  }
};

static void lds(long long off, long long size, const char* what, long long wg, int lane, long long pos) {
  ldss++;
  if (off < 0 || off >= size) fail(what, "outside the LDS area", off, wg, lane, pos);
}

int main() {
  long long n_, T, batch, fill_, ldd, step_d, stride_d, lde, step_e, stride_e, eblocks, dfirst;
  while (std::scanf("%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", &n_, &T, &batch, &fill_, &ldd, &step_d, &stride_d, &lde, &step_e,
                    &stride_e, &eblocks, &dfirst) == 12) {
    line_no++;
    if (n_ < 1 || n_ > BT_MAX || T < 1 || batch < 1 || fill_ < 0 || fill_ > 1) { std::printf("line %lld: not a launch the library makes\n", line_no); return 1; }
    const int n = (int)n_, NP = bt_padded(n), G = 64 / NP, fill = (int)fill_;
    const long long nwg = (batch + G - 1) / G;
    const BtGeo gd = {ldd, step_d, stride_d, T, batch, n, NP}, ge = {lde, step_e, stride_e, T, batch, n, NP};
    const BtGeo all = {ldd, step_d, stride_d, T, nwg * G, n, NP};      // the same launch with every lane group alive
    Operand D = {"D", ldd, step_d, stride_d, T, dfirst, batch, n, {}, {}}, E = {"E", lde, step_e, stride_e, eblocks, 0, batch, n, {}, {}};
    D.init();
    E.init();
    const long long img = (long long)G * bt_img_size(NP), xs = bt_x_size(NP);
    // the chain of a lane (its own group's) and of its wave row in slab s, as BtFixed answers
    auto own_of = [&](long long wg, int lane) { return bt_chain_fixed(gd, ge, 0, wg, bt_group(NP, lane)); };
    auto row_of = [&](const BtGeo& g, long long wg, int lane, int s) { return bt_chain_fixed(g, g, 0, wg, bt_row_group(NP, lane, s)); };

    for (long long wg = 0; wg < nwg; wg++) {
      std::vector<int> gw((size_t)xs, 0), sw((size_t)xs, 0), cleared((size_t)(2 * xs), 0);
      for (int j = 0; j < bt_x_clear_passes(NP); j++)
        for (int lane = 0; lane < 64; lane++) {
          const BtAt at = bt_x_clear(NP, lane, j);
          if (at.on) { lds(at.off, 2 * xs, "exchange", wg, lane, -1); cleared[(size_t)at.off]++; }
        }
      for (int v : cleared)
        if (v != 1) fail("exchange", "a word is not cleared once", v, wg, -1, -1);
      for (int lane = 0; lane < 64; lane++)
        for (int cc = 0; cc < n; cc++) {
          const BtAt at = bt_tri_at(gd, own_of(wg, lane), lane, bt_pos(own_of(wg, lane), 0, true), cc);
          if (at.on) {
            D.rd[D.at(at.off, bt_chain(NP, wg, lane), T - 1, lane % NP, cc, true, wg, lane)]++;
            lds(bt_img_base(NP, lane) + bt_img_at(NP, lane % NP, cc), img, "image", wg, lane, T - 1);
          }
        }
      // an MFMA phase: every operand word the lanes read lies in the area and, for a row and a k below n, was written exactly once
      auto product = [&](const std::vector<int>& a, const std::vector<int>& b, const char* an, const char* bn, bool upper, long long pos) {
        for (int lane = 0; lane < 64; lane++)
          for (int q = 0; q < n; q += 4)
            for (int sl = 0; sl < 4; sl++) {
              if (!bt_slab_on(NP, sl, n)) continue;
              bool used = false;
              for (int so = 0; so < 4; so++) used = used || (bt_tile(NP, sl, so, upper) && bt_slab_on(NP, so, n)) || (bt_tile(NP, so, sl, upper) && bt_slab_on(NP, so, n));
              if (!used) fail("exchange", "a slab that is on meets no tile", sl, wg, lane, pos);
              const BtAt at = bt_x_slab(n, lane, sl, q);
              if (!at.on) continue;
              lds(at.off, xs, "exchange", wg, lane, pos);
              lds(at.off, xs, "exchange", wg, lane, pos);
              const int w = sl * 16 + lane % 16, k = q + lane / 16;
              if (at.off != bt_x_own(k, w)) fail("exchange", "not word w of line k", at.off, wg, lane, pos);
              if (w % NP < n && a[(size_t)at.off] != 1) fail(an, "an operand word is read before it is written once", at.off, wg, lane, pos);
              if (w % NP < n && b[(size_t)at.off] != 1) fail(bn, "an operand word is read before it is written once", at.off, wg, lane, pos);
            }
      };

      auto ecol = [&](long long wg_, int lane, long long p, bool may) {
        for (int i = 0; i < n; i++) {
          const BtAt at = bt_ecol_at(ge, own_of(wg_, lane), lane, p, i);
          if (at.on && !may) fail("E", "a coupling block at position -1", at.off, wg_, lane, p);
          if (at.on) E.rd[E.at(at.off, bt_chain(NP, wg_, lane), p, i, lane % NP, false, wg_, lane)]++;
        }
      };
      auto tri = [&](long long wg_, int lane, long long p, bool may) {
        for (int cc = 0; cc < n; cc++) {
          const BtAt at = bt_tri_at(gd, own_of(wg_, lane), lane, p, cc);
          if (at.on && !may) fail("D", "a predecessor at position 0", at.off, wg_, lane, p);
          if (at.on) D.rd[D.at(at.off, bt_chain(NP, wg_, lane), p, lane % NP, cc, true, wg_, lane)]++;
        }
      };

      for (long long step = 0; step < T; step++) {
        const long long pos = T - 1 - step;          // of every chain that is alive
        const bool first = step == 0, prev = bt_has_next(T, step);       // the kernel's wave-uniform test: the walk goes on
        if (pos < 0 || pos >= T || prev != (pos > 0)) fail("D", "the walk leaves the chain", pos, wg, -1, pos);
        for (int lane = 0; lane < 64; lane++) {
          const BtChain own = own_of(wg, lane);
          if (own.T != (bt_chain(NP, wg, lane) < batch ? T : 0) || own.id != bt_chain(NP, wg, lane)) fail("chain", "not the lane group's chain", own.id, wg, lane, pos);
          if (own.T > 0 && bt_pos(own, step, true) != pos) fail("D", "the walk is not at the step's position", bt_pos(own, step, true), wg, lane, pos);
        }
        // the requests, as the kernel makes them: row r of U_(pos-1) in front of position pos at NP <= 32 (position 0 included: the answer
        // must be off), behind it otherwise; column c of E_(pos-1) behind the substitution of every position but the first at NP < 64
        // (the first one of a chain in front of the walk), column c of E_pos in front of it at NP = 64
        for (int lane = 0; lane < 64; lane++) {
          if (NP <= 32 || prev) tri(wg, lane, pos - 1, prev);
          if (NP < 64 && first) ecol(wg, lane, pos - 1, prev);
          if (!first) ecol(wg, lane, NP < 64 ? pos - 1 : pos, NP < 64 ? prev : true);
        }
        if (!first) {                              // G: the lane's column along its own line of X1
          std::fill(gw.begin(), gw.end(), 0);
          for (int lane = 0; lane < 64; lane++)
            for (int i = 0; i < n; i++)
              if (lane % NP < n) { const int off = bt_xt_own(NP, i, lane); lds(off, xs, "exchange", wg, lane, pos); gw[(size_t)off]++; }
        }
        for (int lane = 0; lane < 64; lane++)      // the image <-> registers: the substitution, the inverse, the product
          for (int i = 0; i < NP; i++)
            lds(bt_img_base(NP, lane) + (i <= lane % NP ? bt_img_at(NP, i, lane % NP) : bt_img_at(NP, lane % NP, i)), img, "image", wg, lane, pos);
        if (!first) {
          product(gw, sw, "G", "Sigma", false, pos);
          std::fill(sw.begin(), sw.end(), 0);
          for (int lane = 0; lane < 64; lane++)    // C -> E_pos and X2
            for (int si = 0; si < 4; si++)
              for (int sj = 0; sj < 4; sj++)
                for (int r = 0; r < 4; r++) {
                  if (!bt_tile(NP, si, sj, false) || !bt_slab_on(NP, si, n) || !bt_slab_on(NP, sj, n)) continue;
                  const int wi = si * 16 + (lane & 15), wj = sj * 16 + (lane >> 4) + 4 * r;
                  const BtChain chr = row_of(ge, wg, lane, si);
                  const BtAt at = bt_etile_at(ge, chr, lane, bt_pos(chr, step, true), si, sj, r);
                  if (at.on) E.wr[E.at(at.off, bt_chain(NP, wg, wi), pos, wi % NP, wj % NP, false, wg, lane)]++;
                  const BtAt xt = bt_xt_tile(n, NP, lane, si, sj, r);
                  if (xt.on != bt_etile_at(all, row_of(all, wg, lane, si), lane, pos, si, sj, r).on) fail("exchange", "the tile store of C and its copy in LDS disagree", xt.off, wg, lane, pos);
                  if (xt.on) {
                    lds(xt.off, xs, "exchange", wg, lane, pos);
                    if (xt.off != bt_x_own(wj % NP, wi)) fail("exchange", "not word wi of line col", xt.off, wg, lane, pos);
                    sw[(size_t)xt.off]++;
                  }
                }
          product(sw, gw, "C", "G", true, pos);
        } else {                                   // position T - 1: the kernel asks for no coupling block; the accessor would say no
          for (int lane = 0; lane < 64; lane++)
            if (bt_etile_at(ge, row_of(ge, wg, lane, 0), lane, pos, 0, 0, 0).on || bt_ecol_at(ge, own_of(wg, lane), lane, pos, 0).on) fail("E", "a coupling block at position T - 1", 0, wg, lane, pos);
        }
        std::vector<int> seen((size_t)img, 0);
        std::fill(sw.begin(), sw.end(), 0);
        for (int lane = 0; lane < 64; lane++)      // P from the image, the mirrored Sigma into X2
          for (int si = 0; si < 4; si++)
            for (int sj = 0; sj < 4; sj++)
              for (int r = 0; r < 4; r++) {
                if (!bt_tile(NP, si, sj, true) || !bt_slab_on(NP, si, n) || !bt_slab_on(NP, sj, n)) continue;
                const BtAt it = bt_img_tile(n, NP, lane, si, sj, r);
                if (it.on) { lds(it.off, img, "image", wg, lane, pos); seen[(size_t)it.off]++; }
                const BtAt up = bt_sig_tile(n, NP, lane, si, sj, r, false), lo = bt_sig_tile(n, NP, lane, si, sj, r, true);
                if (up.on != it.on || (lo.on && !up.on)) fail("exchange", "the mirrored store and the read of P disagree", up.off, wg, lane, pos);
                if (up.on) { lds(up.off, xs, "exchange", wg, lane, pos); sw[(size_t)up.off]++; }
                if (lo.on) { lds(lo.off, xs, "exchange", wg, lane, pos); sw[(size_t)lo.off]++; }
              }
        for (int grp = 0; grp < G; grp++)
          for (int c = 0; c < n; c++)
            for (int r = 0; r < n; r++) {
              if (r <= c && seen[(size_t)(grp * bt_img_size(NP) + bt_img_at(NP, r, c))] != 1) fail("image", "an element of P is not read once", r + c * n, wg, grp, pos);
              if (sw[(size_t)bt_x_own(r, grp * NP + c)] != 1) fail("Sigma", "a word of the mirrored block is not written once", r + c * n, wg, grp, pos);
            }
        for (int lane = 0; lane < 64; lane++)      // Sigma -> D_pos
          for (int cc = 0; cc < n; cc++) {
            const BtAt at = bt_full_at(gd, own_of(wg, lane), lane, pos, cc, fill);
            if (!at.on) continue;
            D.wr[D.at(at.off, bt_chain(NP, wg, lane), pos, lane % NP, cc, fill == 0, wg, lane)]++;
            lds(bt_x_own(cc, lane), xs, "exchange", wg, lane, pos);
            if (sw[(size_t)bt_x_own(cc, lane)] != 1) fail("Sigma", "the store of D reads a word that was not written", bt_x_own(cc, lane), wg, lane, pos);
          }
        if (!prev) break;
        for (int lane = 0; lane < 64; lane++)      // U_(pos-1) -> the image
          for (int cc = lane % NP; cc < n; cc++) lds(bt_img_base(NP, lane) + bt_img_at(NP, lane % NP, cc), img, "image", wg, lane, pos);
      }
    }
    D.expect(D.rd, true, "the upper triangle is not read exactly once");
    D.expect(D.wr, fill == 0, "the written set of D is not the triangles (fill = 0) or the blocks (fill = 1), each element once");
    if (eblocks > 0) {
      E.expect(E.rd, false, "the element is not read exactly once");
      E.expect(E.wr, false, "the element is not written exactly once");
    }
  }
  std::printf("ok %lld %lld %lld\n", line_no, globals, ldss);
  return 0;
}
