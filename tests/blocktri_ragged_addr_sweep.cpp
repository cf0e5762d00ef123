// TEST INFRASTRUCTURE of tests/test_blocktri_ragged_addr.py: the loops of capital_amd/csrc/blocktri_kernels.h (bt_factor, bt_solve with
// half = 0, 1, 2, bt_inverse with fill = 0, 1) as blocktri_vbatched.hip launches them - the chain of a lane group from bt_chain_plan -
// replayed on the CPU, workgroup by workgroup and lane by lane over the plan's sorted list, with the address functions the kernels
// themselves call (capital_amd/csrc/blocktri_addr.h) and asked exactly as the kernels ask them, the prefetches included.  Reads one launch per line from stdin:
//   n nrhs ldd step_d lde step_e ldb eslots batch  then per chain: T first R
// T and first are what the PLAN says; R is the number of positions the chain's operands really hold and eslots the number of slots the E
// operand really holds - R = T and eslots = the plan's ESLOTS for every launch the library makes; a line that says less is a planted fault.
// Checks: every access that is `on` lies inside the addressed chain's OWN slots of D, its own R - 1 coupling slots of E (the last E slot
// of a chain is never addressed) and its own rows of the stacked B, at the element the loop is at; a chain that has ended, a chain of
// T = 0 and a dead lane group address nothing; the written set is exactly the triangles (full blocks under fill), the E blocks and the
// right-hand-side segments, each element once per step, and info / logdet entries of the chains with T > 0 only; every exchange-area
// word below n that a product reads was written for that position, and no word at or beyond n is ever written in the areas that rely
// on their initial +0.0.  Prints "ok <lines> <global accesses> <LDS accesses>"; exits 1 on the first finding.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "blocktri_addr.h"

static long long line_no = 0, globals = 0, ldss = 0;

static void fail(const char* what, const char* why, long long off, long long wg, int lane, long long pos) {
  std::printf("line %lld: %s: %s: offset %lld workgroup %lld lane %d position %lld\n", line_no, what, why, off, wg, lane, pos);
  std::exit(1);
}

struct Chain { long long T, first, R, row; };

struct Operand {                         // a sequence of n x n slots; chain c owns `own(c)` of them from first[c]
  const char* name;
  long long ld, step, slots;             // slots: what the operand really holds
  int n, less;                           // less = 1 for E: a chain owns R - 1 slots
  const std::vector<Chain>* ch;
  std::vector<int> rd, wr;
  void init(bool used) {
    if (!used) return;
    if (ld < n) fail(name, "leading dimension below n", ld, -1, -1, -1);
    if (slots > 1 && step < ld * n) fail(name, "step below one block", step, -1, -1, -1);
    rd.assign((size_t)(slots * n * n), 0);
    wr.assign((size_t)(slots * n * n), 0);
  }
  size_t at(long long off, long long chain, long long pos, int row, int col, bool upper, long long wg, int lane) {
    globals++;
    if (off < 0) fail(name, "negative offset", off, wg, lane, pos);
    if (chain < 0 || chain >= (long long)ch->size()) fail(name, "a dead lane group addresses memory", off, wg, lane, pos);
    const Chain& c = (*ch)[(size_t)chain];
    if (pos < 0 || pos >= c.R - less) fail(name, "position outside the chain's own slots", off, wg, lane, pos);
    const long long slot = c.first + pos;
    if (slot >= slots) fail(name, "a slot beyond the operand", off, wg, lane, pos);
    const long long rem = off - slot * step;
    if (rem < 0 || rem >= ld * n) fail(name, "outside the block", off, wg, lane, pos);
    const int r = (int)(rem % ld), cc = (int)(rem / ld);
    if (r >= n || cc >= n) fail(name, "a pad row or column", off, wg, lane, pos);
    if (upper && r > cc) fail(name, "the strictly lower triangle", off, wg, lane, pos);
    if (row >= 0 && (r != row || cc != col)) fail(name, "not the element the loop is at", off, wg, lane, pos);
    return (size_t)((slot * n + cc) * n + r);
  }
  // every element of every owned slot `count` times (the upper triangle only where upper), every other slot untouched
  void expect(const std::vector<int>& v, int count, bool upper, const char* why) {
    if (v.empty()) return;
    std::vector<char> owned((size_t)slots, 0);
    for (const Chain& c : *ch)
      for (long long i = 0; i < c.R - less; i++)
        if (c.first + i < slots) owned[(size_t)(c.first + i)] = 1;
    for (long long s = 0; s < slots; s++)
      for (int c = 0; c < n; c++)
        for (int r = 0; r < n; r++) {
          const int want = (!owned[(size_t)s] || (upper && r > c)) ? 0 : count;
          if (v[(size_t)((s * n + c) * n + r)] != want) fail(name, why, (s * n + c) * n + r, -1, -1, s);
        }
  }
  void clear() { std::fill(rd.begin(), rd.end(), 0); std::fill(wr.begin(), wr.end(), 0); }
};

struct Rhs {
  long long ldb, nrhs, rows;             // rows = n ROWS
  int n;
  const std::vector<Chain>* ch;
  std::vector<int> rd, wr;
  void init() {
    if (ldb < rows) fail("B", "leading dimension below n ROWS", ldb, -1, -1, -1);
    rd.assign((size_t)(nrhs * rows), 0);
    wr.assign((size_t)(nrhs * rows), 0);
  }
  size_t at(long long off, long long chain, long long col, long long pos, int r, long long wg, int lane) {
    globals++;
    if (off < 0) fail("B", "negative offset", off, wg, lane, pos);
    if (chain < 0 || chain >= (long long)ch->size()) fail("B", "a dead lane group addresses memory", off, wg, lane, pos);
    const Chain& c = (*ch)[(size_t)chain];
    if (pos < 0 || pos >= c.R) fail("B", "a segment outside the chain's own rows", off, wg, lane, pos);
    if (col < 0 || col >= nrhs) fail("B", "a column beyond nrhs", off, wg, lane, pos);
    const long long row = (c.row + pos) * n + r;
    if (off != col * ldb + row || row >= rows) fail("B", "not the element the loop is at", off, wg, lane, pos);
    return (size_t)(col * rows + row);
  }
};

static void lds(long long off, long long size, const char* what, long long wg, int lane, long long pos) {
  ldss++;
  if (off < 0 || off >= size) fail(what, "outside the LDS area", off, wg, lane, pos);
}

// an exchange area with a stamp per word: which phase wrote it last
struct Area {
  std::vector<long long> stamp;
  long long size;
  const char* name;
  void init(long long s, const char* nm) { size = s; name = nm; stamp.assign((size_t)s, -1); }
  void write(long long off, long long phase, long long wg, int lane, long long pos) { lds(off, size, name, wg, lane, pos); stamp[(size_t)off] = phase; }
  void read(long long off, long long phase, long long wg, int lane, long long pos) {
    lds(off, size, name, wg, lane, pos);
    if (stamp[(size_t)off] != phase) fail(name, "a product reads a word that was not written for this position", off, wg, lane, pos);
  }
};

int main() {
  long long n_, nrhs, ldd, step_d, lde, step_e, ldb, eslots, batch;
  while (std::scanf("%lld %lld %lld %lld %lld %lld %lld %lld %lld", &n_, &nrhs, &ldd, &step_d, &lde, &step_e, &ldb, &eslots, &batch) == 9) {
    line_no++;
    if (n_ < 1 || n_ > BT_MAX || batch < 1 || nrhs < 1) { std::printf("line %lld: not a launch the library makes\n", line_no); return 1; }
    std::vector<Chain> ch((size_t)batch);
    long long rows = 0, dslots = 0, tmax = 0;
    bool multi = false;
    for (auto& c : ch) {
      if (std::scanf("%lld %lld %lld", &c.T, &c.first, &c.R) != 3 || c.T < 0 || c.first < 0 || c.R < 0 || c.R > c.T) { std::printf("line %lld: bad chain\n", line_no); return 1; }
      c.row = rows;
      rows += c.T;
      if (c.R > 0) dslots = std::max(dslots, c.first + c.R);
      tmax = std::max(tmax, c.T);
      multi = multi || c.T > 1;
    }
    const int n = (int)n_, NP = bt_padded(n), G = 64 / NP;
    std::vector<long long> order((size_t)batch);
    std::iota(order.begin(), order.end(), 0LL);
    std::stable_sort(order.begin(), order.end(), [&](long long a, long long b) { return ch[(size_t)a].T > ch[(size_t)b].T; });
    const long long nwg = (batch + G - 1) / G;
    BtGeo gd = {ldd, step_d, 0, 0, 0, n, NP}, ge = {lde, step_e, 0, 0, 0, n, NP};
    Operand D = {"D", ldd, step_d, dslots, n, 0, &ch, {}, {}}, E = {"E", lde, step_e, eslots, n, 1, &ch, {}, {}};
    D.init(true);
    E.init(multi);
    const long long img = (long long)G * bt_img_size(NP), xs = bt_x_size(NP);
    long long phase = 0;

    // the wavefront's table, as BtPlan fills it: a group beyond the list has T = 0 (its id is never used)
    auto table = [&](long long wg, BtChain* tab, long long& Tw) {
      Tw = 0;
      for (int grp = 0; grp < G; grp++) {
        const long long at = bt_chain(NP, wg, grp * NP);
        tab[grp] = bt_chain_plan(gd, ge, 0, 0, 0, -1);
        if (at < batch) {
          const long long id = order[(size_t)at];
          tab[grp] = bt_chain_plan(gd, ge, ch[(size_t)id].first, ch[(size_t)id].T, ch[(size_t)id].row, id);
        }
        Tw = std::max(Tw, (long long)tab[grp].T);
      }
    };

    // ---------------------------------------------------------------------------------------------- the factor
    std::vector<int> scalars((size_t)batch, 0);
    for (long long wg = 0; wg < nwg; wg++) {
      BtChain tab[8];
      long long Tw;
      table(wg, tab, Tw);
      for (int lane = 0; lane < 64; lane++)
        for (int cc = 0; cc < n; cc++) {
          const BtChain& own = tab[bt_group(NP, lane)];
          const BtAt at = bt_tri_at(gd, own, lane, 0, cc);
          if (at.on) { D.rd[D.at(at.off, own.id, 0, lane % NP, cc, true, wg, lane)]++; lds(bt_img_base(NP, lane) + bt_img_at(NP, lane % NP, cc), img, "image", wg, lane, 0); }
        }
      Area X;
      X.init(xs, "exchange");
      for (long long pos = 0; pos < Tw; pos++) {
        phase++;
        for (int lane = 0; lane < 64; lane++) {
          const BtChain& own = tab[bt_group(NP, lane)];
          for (int i = 0; i < n; i++) {            // the request for E_pos: asked at every step
            const BtAt at = bt_ecol_at(ge, own, lane, pos, i);
            if (at.on) E.rd[E.at(at.off, own.id, pos, i, lane % NP, false, wg, lane)]++;
          }
          for (int si = 0; si < 4; si++) {         // the request for D_(pos+1), asked about the chain of the wave row
            const BtChain& chr = tab[bt_row_group(NP, lane, si)];
            for (int sj = 0; sj < 4; sj++)
              for (int r = 0; r < 4; r++) {
                if (!bt_tile(NP, si, sj, true) || !bt_slab_on(NP, si, n) || !bt_slab_on(NP, sj, n)) continue;
                const BtAt at = bt_next_at(gd, chr, lane, pos, si, sj, r);
                const int wi = si * 16 + (lane & 15), wj = sj * 16 + (lane >> 4) + 4 * r;
                if (at.on) D.rd[D.at(at.off, chr.id, pos + 1, wi % NP, wj % NP, true, wg, lane)]++;
                const BtAt it = bt_img_tile(n, NP, lane, si, sj, r);
                if (at.on && !it.on) fail("image", "a loaded successor element has no place in the image", it.off, wg, lane, pos);
                if (it.on) lds(it.off, img, "image", wg, lane, pos);
              }
          }
          for (int cc = 0; cc < n; cc++) {         // U_pos -> D_pos
            const BtAt at = bt_tri_at(gd, own, lane, pos, cc);
            if (at.on) D.wr[D.at(at.off, own.id, pos, lane % NP, cc, true, wg, lane)]++;
          }
          lds(bt_log_at(NP, lane, lane % NP), 64, "logarithms", wg, lane, pos);
        }
        if (!bt_has_next(Tw, pos)) break;
        for (int lane = 0; lane < 64; lane++) {
          const BtChain& own = tab[bt_group(NP, lane)];
          for (int i = 0; i < n; i++) {            // W_pos -> E_pos and, for every lane, the exchange area (+0.0 where the lane has none)
            const BtAt at = bt_ecol_at(ge, own, lane, pos, i);
            if (at.on) E.wr[E.at(at.off, own.id, pos, i, lane % NP, false, wg, lane)]++;
            X.write(bt_x_own(i, lane), phase, wg, lane, pos);
          }
        }
        for (int lane = 0; lane < 64; lane++)
          for (int q = 0; q < n; q += 4)
            for (int sl = 0; sl < 4; sl++) {
              if (!bt_slab_on(NP, sl, n)) continue;
              const BtAt at = bt_x_slab(n, lane, sl, q);
              if (at.on) X.read(at.off, phase, wg, lane, pos);
            }
      }
      for (int lane = 0; lane < 64; lane++) {
        const BtChain& own = tab[bt_group(NP, lane)];
        const BtAt at = bt_scalar_at(NP, own, lane);
        if (at.on) {
          if (at.off < 0 || at.off >= batch || ch[(size_t)at.off].T == 0) fail("info", "not the entry of a chain with a position", at.off, wg, lane, -1);
          scalars[(size_t)at.off]++;
          globals++;
        }
      }
    }
    D.expect(D.rd, 1, true, "the factor does not read the element exactly once");
    D.expect(D.wr, 1, true, "the factor does not write the element exactly once");
    E.expect(E.rd, 1, false, "the factor does not read the element exactly once");
    E.expect(E.wr, 1, false, "the factor does not write the element exactly once");
    for (long long c = 0; c < batch; c++)
      if (scalars[(size_t)c] != (ch[(size_t)c].T > 0 ? 1 : 0)) fail("info", "a chain's entry is not written once, or that of an empty chain is written", c, -1, -1, -1);

    // ---------------------------------------------------------------------------------------------- the solve, half = 0, 1, 2
    for (int half = 0; half < 3; half++) {
      Rhs B = {ldb, nrhs, rows * n, n, &ch, {}, {}};
      B.init();
      D.clear();
      E.clear();
      const long long passes = bt_rhs_passes(NP, nrhs);
      for (long long wg = 0; wg < nwg; wg++) {
        BtChain tab[8];
        long long Tw;
        table(wg, tab, Tw);
        for (int lane = 0; lane < 64; lane++) {
          const BtAt at = bt_info_at(tab[bt_group(NP, lane)]);
          if (at.on && (at.off < 0 || at.off >= batch || ch[(size_t)at.off].T == 0)) fail("info", "not the entry of a chain with a position", at.off, wg, lane, -1);
        }
        Area X;
        X.init(xs, "exchange");
        auto seg = [&](std::vector<int>& v, long long pass, long long step, bool desc, bool target) {
          for (int lane = 0; lane < 64; lane++) {
            const BtChain& own = tab[bt_group(NP, lane)];
            const long long pos = target ? bt_couple_tpos(own, step, desc) : bt_pos(own, step, desc);
            for (int i = 0; i < n; i++) {
              const BtAt at = bt_rhs_at(gd, own, ldb, nrhs, lane, pass, pos, i);
              if (at.on) v[B.at(at.off, own.id, pass * NP + lane % NP, pos, i, wg, lane)]++;
            }
          }
        };
        auto tri = [&](long long step, bool desc) {
          for (int lane = 0; lane < 64; lane++) {
            const BtChain& own = tab[bt_group(NP, lane)];
            const long long pos = bt_pos(own, step, desc);
            for (int cc = 0; cc < n; cc++) {
              const BtAt at = bt_tri_at(gd, own, lane, pos, cc);
              if (at.on) D.rd[D.at(at.off, own.id, pos, lane % NP, cc, true, wg, lane)]++;
            }
          }
        };
        auto couple = [&](long long pass, long long step, bool desc) {
          seg(B.rd, pass, step, desc, true);
          phase++;
          bool onc[4];
          for (int sl = 0; sl < 4; sl++) onc[sl] = pass * NP + (sl * 16) % NP < nrhs;
          for (int lane = 0; lane < 64; lane++)
            for (int i = 0; i < n; i++) X.write(bt_x_own(i, lane), phase, wg, lane, step);
          std::vector<int> xw((size_t)xs, 0);
          for (int lane = 0; lane < 64; lane++) {
            const BtChain& own = tab[bt_group(NP, lane)];
            if (bt_rhs_at(gd, own, ldb, nrhs, lane, pass, bt_couple_tpos(own, step, desc), 0).on && !onc[lane / 16]) fail("exchange", "a live column in a skipped slab", lane, wg, lane, step);
            for (int q = 0; q < n; q += 4)
              for (int sl = 0; sl < 4; sl++) {
                if (bt_slab_on(NP, sl, n)) {
                  const BtChain& chr = tab[bt_row_group(NP, lane, sl)];
                  const long long epos = bt_couple_epos(chr, step, desc);
                  const BtAt at = bt_eslab_at(ge, chr, lane, epos, sl, q, !desc);
                  const int row = (sl * 16 + lane % 16) % NP, k = q + lane / 16;
                  if (at.on) E.rd[E.at(at.off, chr.id, epos, !desc ? k : row, !desc ? row : k, false, wg, lane)]++;
                }
                if (onc[sl]) {
                  const BtAt at = bt_x_slab(n, lane, sl, q);
                  if (at.on) X.read(at.off, phase, wg, lane, step);
                }
              }
            for (int si = 0; si < 4; si++)
              for (int sj = 0; sj < 4; sj++)
                for (int r = 0; r < 4; r++) {
                  if (!bt_tile(NP, si, sj, false) || !bt_slab_on(NP, si, n) || !onc[sj]) continue;
                  const BtAt at = bt_x_tile(n, NP, lane, si, sj, r);
                  if (at.on) { lds(at.off, xs, "exchange", wg, lane, step); xw[(size_t)at.off]++; }
                }
          }
          for (int w = 0; w < 64; w++)
            for (int i = 0; i < n; i++)
              if (xw[(size_t)bt_x_own(i, w)] != (onc[w / 16] ? 1 : 0)) fail("exchange", "a product is not written once", bt_x_own(i, w), wg, w, step);
        };
        for (long long pass = 0; pass < passes; pass++)
          for (int desc = 0; desc < 2; desc++) {
            if ((desc == 0 && half == 2) || (desc == 1 && half == 1)) continue;
            seg(B.rd, pass, 0, desc != 0, false);
            for (long long step = 0; step < Tw; step++) {
              tri(step, desc != 0);
              seg(B.wr, pass, step, desc != 0, false);
              if (!bt_has_next(Tw, step)) break;
              couple(pass, step, desc != 0);
            }
          }
      }
      const int sweeps = half == 0 ? 2 : 1;
      for (size_t e = 0; e < B.wr.size(); e++)
        if (B.wr[e] != sweeps || B.rd[e] != sweeps) fail("B", "an element of a segment is not read and written once per sweep", (long long)e, -1, -1, -1);
      D.expect(D.rd, sweeps * (int)passes, true, "a sweep does not read the factor's element once per pass");
      E.expect(E.rd, sweeps * (int)passes, false, "a sweep does not read the coupling element once per pass");
      D.expect(D.wr, 0, true, "the solve writes D");
      E.expect(E.wr, 0, false, "the solve writes E");
    }

    // ---------------------------------------------------------------------------------------------- the selected inverse, fill = 0, 1
    const bool EARLY = NP < 64, EARLY_U = NP <= 32;
    for (int fill = 0; fill < 2; fill++) {
      D.clear();
      E.clear();
      for (long long wg = 0; wg < nwg; wg++) {
        BtChain tab[8];
        long long Tw;
        table(wg, tab, Tw);
        Area XG, XS;                               // X1 (G_i) and X2 (Sigma, C): both start as +0.0 and rely on it at and beyond n
        XG.init(xs, "exchange X1");
        XS.init(xs, "exchange X2");
        for (int lane = 0; lane < 64; lane++)
          for (int j = 0; j < bt_x_clear_passes(NP); j++) {
            const BtAt at = bt_x_clear(NP, lane, j);
            if (at.on) lds(at.off, 2 * xs, "exchange", wg, lane, -1);
          }
        auto below_n = [&](long long off, const char* what, long long w_, int lane, long long step) {
          if (off / BT_LDX >= n || (off % BT_LDX) >= 64 || (off % BT_LDX) % NP >= n) fail(what, "a word at or beyond n is written", off, w_, lane, step);
        };
        auto tri_read = [&](int lane, long long pos) {
          const BtChain& own = tab[bt_group(NP, lane)];
          for (int cc = 0; cc < n; cc++) {
            const BtAt at = bt_tri_at(gd, own, lane, pos, cc);
            if (at.on) D.rd[D.at(at.off, own.id, pos, lane % NP, cc, true, wg, lane)]++;
          }
        };
        auto ecol_read = [&](int lane, long long pos) {
          const BtChain& own = tab[bt_group(NP, lane)];
          for (int i = 0; i < n; i++) {
            const BtAt at = bt_ecol_at(ge, own, lane, pos, i);
            if (at.on) E.rd[E.at(at.off, own.id, pos, i, lane % NP, false, wg, lane)]++;
          }
        };
        auto product = [&](Area& a, long long pa, Area& b, long long pb, long long step) {
          for (int lane = 0; lane < 64; lane++)
            for (int q = 0; q < n; q += 4)
              for (int sl = 0; sl < 4; sl++) {
                if (!bt_slab_on(NP, sl, n)) continue;
                const BtAt at = bt_x_slab(n, lane, sl, q);
                if (!at.on) continue;
                if ((at.off % BT_LDX) % NP < n) { a.read(at.off, pa, wg, lane, step); b.read(at.off, pb, wg, lane, step); }
                else if (a.stamp[(size_t)at.off] != -1 || b.stamp[(size_t)at.off] != -1) fail("exchange", "a word at or beyond n no longer holds its +0.0", at.off, wg, lane, step);
              }
        };
        for (int lane = 0; lane < 64; lane++) {
          const BtChain& own = tab[bt_group(NP, lane)];
          tri_read(lane, bt_pos(own, 0, true));
          if (EARLY) ecol_read(lane, bt_pos(own, 0, true) - 1);
        }
        long long sig_phase = -2;
        for (long long step = 0; step < Tw; step++) {
          const bool first = step == 0;
          const long long pg = ++phase;
          for (int lane = 0; lane < 64; lane++) {
            const BtChain& own = tab[bt_group(NP, lane)];
            const long long pos = bt_pos(own, step, true);
            if (EARLY_U) tri_read(lane, pos - 1);
            if (!first) {
              if (!EARLY) ecol_read(lane, pos);
              for (int i = 0; i < n; i++)
                if (lane % NP < n) { below_n(bt_xt_own(NP, i, lane), "exchange X1", wg, lane, step); XG.write(bt_xt_own(NP, i, lane), pg, wg, lane, step); }
              if (EARLY) ecol_read(lane, pos - 1);
            }
          }
          if (!first) {
            product(XG, pg, XS, sig_phase, step);
            const long long pc = ++phase;
            for (int lane = 0; lane < 64; lane++)
              for (int si = 0; si < 4; si++) {
                const BtChain& chr = tab[bt_row_group(NP, lane, si)];
                const long long rpos = bt_pos(chr, step, true);
                for (int sj = 0; sj < 4; sj++)
                  for (int r = 0; r < 4; r++) {
                    if (!bt_tile(NP, si, sj, false) || !bt_slab_on(NP, si, n) || !bt_slab_on(NP, sj, n)) continue;
                    const int wi = si * 16 + (lane & 15), wj = sj * 16 + (lane >> 4) + 4 * r;
                    const BtAt at = bt_etile_at(ge, chr, lane, rpos, si, sj, r);
                    if (at.on) E.wr[E.at(at.off, chr.id, rpos, wi % NP, wj % NP, false, wg, lane)]++;
                    const BtAt xt = bt_xt_tile(n, NP, lane, si, sj, r);
                    if (xt.on) { below_n(xt.off, "exchange X2", wg, lane, step); XS.write(xt.off, pc, wg, lane, step); }
                  }
              }
            product(XS, pc, XG, pg, step);
          }
          sig_phase = ++phase;
          for (int lane = 0; lane < 64; lane++)
            for (int si = 0; si < 4; si++)
              for (int sj = 0; sj < 4; sj++)
                for (int r = 0; r < 4; r++) {
                  if (!bt_tile(NP, si, sj, true) || !bt_slab_on(NP, si, n) || !bt_slab_on(NP, sj, n)) continue;
                  const BtAt it = bt_img_tile(n, NP, lane, si, sj, r);
                  if (it.on) lds(it.off, img, "image", wg, lane, step);
                  for (int mirror = 0; mirror < 2; mirror++) {
                    const BtAt st = bt_sig_tile(n, NP, lane, si, sj, r, mirror != 0);
                    if (st.on) { below_n(st.off, "exchange X2", wg, lane, step); XS.write(st.off, sig_phase, wg, lane, step); }
                  }
                }
          for (int lane = 0; lane < 64; lane++) {
            const BtChain& own = tab[bt_group(NP, lane)];
            const long long pos = bt_pos(own, step, true);
            for (int cc = 0; cc < n; cc++) {
              const BtAt at = bt_full_at(gd, own, lane, pos, cc, fill);
              if (at.on) { D.wr[D.at(at.off, own.id, pos, lane % NP, cc, fill == 0, wg, lane)]++; XS.read(bt_x_own(cc, lane), sig_phase, wg, lane, step); }
            }
          }
          if (!bt_has_next(Tw, step)) break;
          if (!EARLY_U)
            for (int lane = 0; lane < 64; lane++) tri_read(lane, bt_pos(tab[bt_group(NP, lane)], step, true) - 1);
        }
      }
      D.expect(D.rd, 1, true, "the inverse does not read the factor's element exactly once");
      D.expect(D.wr, 1, fill == 0, "the inverse does not write the element exactly once");
      E.expect(E.rd, 1, false, "the inverse does not read the coupling element exactly once");
      E.expect(E.wr, 1, false, "the inverse does not write the coupling element exactly once");
    }
  }
  std::printf("ok %lld %lld %lld\n", line_no, globals, ldss);
  return 0;
}
