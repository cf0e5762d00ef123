// TEST INFRASTRUCTURE of tests/test_blocktri_addr.py: the loops of capital_amd/csrc/blocktri_kernels.h (bt_factor, bt_solve with
// half = 0, 1, 2, bt_couple) as blocktri_batched.hip launches them - the chain of a lane group from bt_chain_fixed, a walk of T steps -
// replayed on the CPU, workgroup by workgroup and lane by lane, with the address functions the kernels themselves call
// (capital_amd/csrc/blocktri_addr.h).  Reads one launch per line from stdin:
//   n T batch nrhs ldd step_d stride_d lde step_e stride_e ldb stride_b eblocks
// eblocks is the number of coupling blocks per chain the E operand really holds - T - 1 for every launch the library makes; a line that
// says less is a planted fault (the kernel would address a coupling block the chain does not have).
// Checks: every access that is `on` decodes to an element inside its block's extent, of the lane's own chain and of the position the loop
// is at; position T - 1 addresses no E block and no successor and T = 1 no E at all (the functions are asked there as the kernel asks them:
// the answer must be `off`); the lane groups beyond `batch` address nothing; the factor reads and writes every element of every upper
// triangle of D and of every E block exactly once and nothing else; a sweep of the solve writes every element of every right-hand-side
// segment exactly once and reads D and E only; the LDS offsets stay inside their areas and the tile stores hit every element they should
// exactly once.  Prints "ok <lines> <global accesses> <LDS accesses>"; exits 1 on the first finding.
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

struct Operand {                         // `blocks` n x n blocks per chain
  const char* name;
  long long ld, step, stride, blocks, batch;
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
  // the element an offset names; it must be (chain, pos) and, where row >= 0, (row, col)
  size_t at(long long off, long long chain, long long pos, int row, int col, bool upper, long long wg, int lane) {
    globals++;
    if (off < 0) fail(name, "negative offset", off, wg, lane, pos);
    if (blocks <= 0) fail(name, "the operand holds no block", off, wg, lane, pos);
    if (chain < 0 || chain >= batch) fail(name, "a dead lane group addresses memory", off, wg, lane, pos);
    if (pos < 0 || pos >= blocks) fail(name, "position outside the chain", off, wg, lane, pos);
    const long long rem = off - chain * stride - pos * step;
    if (rem < 0 || rem >= ld * n) fail(name, "outside the block", off, wg, lane, pos);
    const int r = (int)(rem % ld), c = (int)(rem / ld);
    if (r >= n || c >= n) fail(name, "a pad row or column", off, wg, lane, pos);
    if (upper && r > c) fail(name, "the strictly lower triangle", off, wg, lane, pos);
    if (row >= 0 && (r != row || c != col)) fail(name, "not the element the loop is at", off, wg, lane, pos);
    return (size_t)(((chain * blocks + pos) * n + c) * n + r);
  }
  void expect(const std::vector<int>& v, int count, bool upper, const char* why) {
    for (long long b = 0; b < batch * blocks; b++)
      for (int c = 0; c < n; c++)
        for (int r = 0; r < n; r++) {
          const int want = (upper && r > c) ? 0 : count;
          if (v[(size_t)((b * n + c) * n + r)] != want) fail(name, why, (b * n + c) * n + r, -1, -1, b % blocks);
        }
  }
};

struct Rhs {
  long long ldb, stride_b, nrhs, rows, batch;
  std::vector<int> rd, wr;
  void init() {
    if (ldb < rows) fail("B", "leading dimension below T n", ldb, -1, -1, -1);
    if (batch > 1 && stride_b < ldb * nrhs) fail("B", "stride below one chain", stride_b, -1, -1, -1);
    rd.assign((size_t)(batch * nrhs * rows), 0);
    wr.assign((size_t)(batch * nrhs * rows), 0);
  }
  size_t at(long long off, long long chain, long long col, long long row, long long wg, int lane) {
    globals++;
    if (off < 0) fail("B", "negative offset", off, wg, lane, row);
    if (chain < 0 || chain >= batch) fail("B", "a dead lane group addresses memory", off, wg, lane, row);
    if (col < 0 || col >= nrhs) fail("B", "a column beyond nrhs", off, wg, lane, row);
    if (off != chain * stride_b + col * ldb + row || row < 0 || row >= rows) fail("B", "not the element the loop is at", off, wg, lane, row);
    return (size_t)((chain * nrhs + col) * rows + row);
  }
};

static void lds(long long off, long long size, const char* what, long long wg, int lane, long long pos) {
  ldss++;
  if (off < 0 || off >= size) fail(what, "outside the LDS area", off, wg, lane, pos);
}

int main() {
  long long n_, T, batch, nrhs, ldd, step_d, stride_d, lde, step_e, stride_e, ldb, stride_b, eblocks;
  while (std::scanf("%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", &n_, &T, &batch, &nrhs, &ldd, &step_d, &stride_d, &lde, &step_e,
                    &stride_e, &ldb, &stride_b, &eblocks) == 13) {
    line_no++;
    if (n_ < 1 || n_ > BT_MAX || T < 1 || batch < 1 || nrhs < 1) { std::printf("line %lld: not a launch the library makes\n", line_no); return 1; }
    const int n = (int)n_, NP = bt_padded(n), G = 64 / NP;
    const long long nwg = (batch + G - 1) / G;
    BtGeo gd = {ldd, step_d, stride_d, T, batch, n, NP}, ge = {lde, step_e, stride_e, T, batch, n, NP};
    Operand D = {"D", ldd, step_d, stride_d, T, batch, n, {}, {}}, E = {"E", lde, step_e, stride_e, eblocks, batch, n, {}, {}};
    D.init();
    E.init();
    const long long img = (long long)G * bt_img_size(NP), xs = bt_x_size(NP);
    // the chain of a lane (its own group's) and of its wave row in slab s, as BtFixed answers
    auto own_of = [&](long long wg, int lane) { return bt_chain_fixed(gd, ge, stride_b, wg, bt_group(NP, lane)); };
    auto row_of = [&](long long wg, int lane, int s) { return bt_chain_fixed(gd, ge, stride_b, wg, bt_row_group(NP, lane, s)); };

    // ---------------------------------------------------------------------------------------------- the factor
    std::vector<int> scalars((size_t)batch, 0);
    for (long long wg = 0; wg < nwg; wg++) {
      for (int lane = 0; lane < 64; lane++)
        for (int cc = 0; cc < n; cc++) {
          const BtAt at = bt_tri_at(gd, own_of(wg, lane), lane, 0, cc);
          if (at.on) { D.rd[D.at(at.off, bt_chain(NP, wg, lane), 0, lane % NP, cc, true, wg, lane)]++; lds(bt_img_base(NP, lane) + bt_img_at(NP, lane % NP, cc), img, "image", wg, lane, 0); }
        }
      for (long long pos = 0; pos < T; pos++) {
        const bool has = bt_has_next(T, pos);
        std::vector<int> imgw((size_t)img, 0);
        for (int lane = 0; lane < 64; lane++) {
          const long long chain = bt_chain(NP, wg, lane);
          const BtChain own = own_of(wg, lane);
          if (own.T != (chain < batch ? T : 0) || own.id != chain) fail("chain", "not the lane group's chain", own.id, wg, lane, pos);
          for (int i = 0; i < n; i++) {            // the request for E_pos: asked at every position, the last one included
            const BtAt at = bt_ecol_at(ge, own, lane, pos, i);
            if (at.on && !has) fail("E", "a coupling block at position T - 1", at.off, wg, lane, pos);
            if (at.on) E.rd[E.at(at.off, chain, pos, i, lane % NP, false, wg, lane)]++;
          }
          for (int si = 0; si < 4; si++)           // the request for D_(pos+1)
            for (int sj = 0; sj < 4; sj++)
              for (int r = 0; r < 4; r++) {
                if (!bt_tile(NP, si, sj, true) || !bt_slab_on(NP, si, n) || !bt_slab_on(NP, sj, n)) continue;
                const BtAt at = bt_next_at(gd, row_of(wg, lane, si), lane, pos, si, sj, r);
                if (at.on && !has) fail("D", "a successor at position T - 1", at.off, wg, lane, pos);
                if (at.on) D.rd[D.at(at.off, bt_chain(NP, wg, si * 16 + (lane & 15)), pos + 1, -1, -1, true, wg, lane)]++;
                const BtAt it = bt_img_tile(n, NP, lane, si, sj, r);
                const BtGeo all = {ldd, step_d, stride_d, pos + 2, bt_chain(NP, wg, 63) + 1, n, NP};      // every group alive, with a successor
                if (it.on != bt_next_at(all, bt_chain_fixed(all, all, 0, wg, bt_row_group(NP, lane, si)), lane, pos, si, sj, r).on)
                  fail("image", "the tile store and the tile load disagree", it.off, wg, lane, pos);
                if (it.on && has) { lds(it.off, img, "image", wg, lane, pos); imgw[(size_t)it.off]++; }
              }
          for (int i = 0; i < NP; i++)             // the image <-> registers, the rows of U, the logarithms
            lds(bt_img_base(NP, lane) + (i <= lane % NP ? bt_img_at(NP, i, lane % NP) : bt_img_at(NP, lane % NP, i)), img, "image", wg, lane, pos);
          lds(bt_log_at(NP, lane, lane % NP), 64, "logarithms", wg, lane, pos);
          for (int cc = 0; cc < n; cc++) {         // U_pos -> D_pos
            const BtAt at = bt_tri_at(gd, own, lane, pos, cc);
            if (at.on) D.wr[D.at(at.off, chain, pos, lane % NP, cc, true, wg, lane)]++;
          }
          if (!has) continue;
          for (int i = 0; i < n; i++) {            // W_pos -> E_pos and the exchange area
            const BtAt at = bt_ecol_at(ge, own, lane, pos, i);
            if (at.on) E.wr[E.at(at.off, chain, pos, i, lane % NP, false, wg, lane)]++;
            lds(bt_x_own(i, lane), xs, "exchange", wg, lane, pos);
          }
          for (int q = 0; q < n; q += 4)
            for (int sl = 0; sl < 4; sl++) {
              if (!bt_slab_on(NP, sl, n)) continue;
              const BtAt at = bt_x_slab(n, lane, sl, q);
              if (at.on) { lds(at.off, xs, "exchange", wg, lane, pos); if (at.off != bt_x_own(q + lane / 16, sl * 16 + lane % 16)) fail("exchange", "not the column's row", at.off, wg, lane, pos); }
            }
        }
        if (has)                                   // S_(pos+1) fills the upper triangle of every group's image exactly
          for (int grp = 0; grp < G; grp++)
            for (int c = 0; c < n; c++)
              for (int r = 0; r <= c; r++)
                if (imgw[(size_t)(grp * bt_img_size(NP) + bt_img_at(NP, r, c))] != 1) fail("image", "an element of the successor is not written once", r + c * n, wg, grp, pos);
      }
      for (int lane = 0; lane < 64; lane++) {
        const BtAt at = bt_scalar_at(NP, own_of(wg, lane), lane);
        if (at.on) {
          if (at.off < 0 || at.off >= batch || at.off != bt_chain(NP, wg, lane)) fail("info", "not the chain's entry", at.off, wg, lane, -1);
          scalars[(size_t)at.off]++;
          globals++;
        }
      }
    }
    D.expect(D.rd, 1, true, "the factor does not read the element exactly once");
    D.expect(D.wr, 1, true, "the factor does not write the element exactly once");
    if (eblocks > 0) {
      E.expect(E.rd, 1, false, "the factor does not read the element exactly once");
      E.expect(E.wr, 1, false, "the factor does not write the element exactly once");
    }
    for (int v : scalars)
      if (v != 1) fail("info", "a chain's entry is not written once", v, -1, -1, -1);

    // ---------------------------------------------------------------------------------------------- the solve, half = 0, 1, 2
    for (int half = 0; half < 3; half++) {
      Rhs B = {ldb, stride_b, nrhs, T * n, batch, {}, {}};
      B.init();
      std::fill(D.rd.begin(), D.rd.end(), 0);
      if (eblocks > 0) std::fill(E.rd.begin(), E.rd.end(), 0);
      const long long passes = bt_rhs_passes(NP, nrhs);
      // a step of a sweep: ascending at position `step`, descending at T - 1 - step of the addressed chain (bt_pos); the walk has T steps
      auto seg = [&](std::vector<int>& v, long long wg, long long pass, long long step, bool desc, bool target) {
        for (int lane = 0; lane < 64; lane++) {
          const BtChain own = own_of(wg, lane);
          const long long pos = target ? bt_couple_tpos(own, step, desc) : bt_pos(own, step, desc);
          for (int i = 0; i < n; i++) {
            const BtAt at = bt_rhs_at(gd, own, ldb, nrhs, lane, pass, pos, i);
            if (at.on) v[B.at(at.off, bt_chain(NP, wg, lane), pass * NP + lane % NP, pos * n + i, wg, lane)]++;
          }
        }
      };
      auto tri = [&](long long wg, long long step, bool desc) {
        for (int lane = 0; lane < 64; lane++) {
          const BtChain own = own_of(wg, lane);
          const long long pos = bt_pos(own, step, desc);
          if (own.T > 0 && pos != (desc ? T - 1 - step : step)) fail("D", "the walk is not at the step's position", pos, wg, lane, step);
          for (int cc = 0; cc < n; cc++) {
            const BtAt at = bt_tri_at(gd, own, lane, pos, cc);
            if (at.on) D.rd[D.at(at.off, bt_chain(NP, wg, lane), pos, lane % NP, cc, true, wg, lane)]++;
          }
        }
      };
      auto couple = [&](long long wg, long long pass, long long step, bool desc) {
        const long long epos = desc ? T - 2 - step : step, tpos = desc ? T - 2 - step : step + 1;      // of every chain that is alive
        const bool trans = !desc;
        seg(B.rd, wg, pass, step, desc, true);
        std::vector<int> xw((size_t)xs, 0);
        bool onc[4];
        for (int sl = 0; sl < 4; sl++) onc[sl] = pass * NP + (sl * 16) % NP < nrhs;
        for (int lane = 0; lane < 64; lane++) {
          const BtChain own = own_of(wg, lane);
          if (own.T > 0 && bt_couple_tpos(own, step, desc) != tpos) fail("B", "not the target segment of the step", tpos, wg, lane, step);
          if (bt_rhs_at(gd, own, ldb, nrhs, lane, pass, bt_couple_tpos(own, step, desc), 0).on && !onc[lane / 16]) fail("exchange", "a live column in a skipped slab", lane, wg, lane, tpos);
          for (int i = 0; i < n; i++) lds(bt_x_own(i, lane), xs, "exchange", wg, lane, tpos);
          for (int q = 0; q < n; q += 4)
            for (int sl = 0; sl < 4; sl++) {
              if (bt_slab_on(NP, sl, n)) {
                const BtChain chr = row_of(wg, lane, sl);
                if (chr.T > 0 && bt_couple_epos(chr, step, desc) != epos) fail("E", "not the coupling block of the step", epos, wg, lane, step);
                const BtAt at = bt_eslab_at(ge, chr, lane, bt_couple_epos(chr, step, desc), sl, q, trans);
                const int row = (sl * 16 + lane % 16) % NP, k = q + lane / 16;
                if (at.on) E.rd[E.at(at.off, bt_chain(NP, wg, sl * 16 + lane % 16), epos, trans ? k : row, trans ? row : k, false, wg, lane)]++;
              }
              if (onc[sl]) {
                const BtAt at = bt_x_slab(n, lane, sl, q);
                if (at.on) lds(at.off, xs, "exchange", wg, lane, tpos);
              }
            }
          for (int si = 0; si < 4; si++)
            for (int sj = 0; sj < 4; sj++)
              for (int r = 0; r < 4; r++) {
                if (!bt_tile(NP, si, sj, false) || !bt_slab_on(NP, si, n) || !onc[sj]) continue;
                const BtAt at = bt_x_tile(n, NP, lane, si, sj, r);
                if (at.on) { lds(at.off, xs, "exchange", wg, lane, tpos); xw[(size_t)at.off]++; }
              }
        }
        for (int w = 0; w < 64; w++)               // every row of every column of a slab that is on receives its product exactly once
          for (int i = 0; i < n; i++)
            if (xw[(size_t)bt_x_own(i, w)] != (onc[w / 16] ? 1 : 0)) fail("exchange", "a product is not written once", bt_x_own(i, w), wg, w, tpos);
      };
      for (long long wg = 0; wg < nwg; wg++) {
        for (int lane = 0; lane < 64; lane++) {
          const BtAt at = bt_info_at(own_of(wg, lane));
          if (at.on && (at.off >= batch || at.off != bt_chain(NP, wg, lane))) fail("info", "not the chain's entry", at.off, wg, lane, -1);
        }
        for (long long pass = 0; pass < passes; pass++)
          for (int desc = 0; desc < 2; desc++) {
            if ((desc == 0 && half == 2) || (desc == 1 && half == 1)) continue;
            seg(B.rd, wg, pass, 0, desc != 0, false);
            for (long long step = 0; step < T; step++) {
              tri(wg, step, desc != 0);
              seg(B.wr, wg, pass, step, desc != 0, false);
              if (!bt_has_next(T, step)) break;
              couple(wg, pass, step, desc != 0);
            }
          }
      }
      const int sweeps = half == 0 ? 2 : 1;
      for (size_t e = 0; e < B.wr.size(); e++)
        if (B.wr[e] != sweeps || B.rd[e] != sweeps) fail("B", "an element of a segment is not read and written once per sweep", (long long)e, -1, -1, -1);
      D.expect(D.rd, sweeps * (int)passes, true, "a sweep does not read the factor's element once per pass");
      if (eblocks > 0) E.expect(E.rd, sweeps * (int)passes, false, "a sweep does not read the coupling element once per pass");
    }
  }
  std::printf("ok %lld %lld %lld\n", line_no, globals, ldss);
  return 0;
}
