// The address arithmetic of the block-tridiagonal kernels (blocktri_kernels.h): which element of D, E, B, info / logdet and of the LDS
// areas a lane touches at a chain position, and whether it touches it at all - as functions the kernels call AND a plain C++ program can
// call (tests/test_blocktri_addr.py, test_blocktri_potri_addr.py and test_blocktri_ragged_addr.py replay the kernels' loops on the CPU,
// lane by lane: every addressed offset inside its block, no E block and no successor at position T - 1, no predecessor at position 0, no
// E at all with T = 1, nothing from a dead lane group or an ended chain, the written set exactly the triangles, the E blocks and the
// right-hand-side segments).  The kernels form no address any other way.  Nothing here knows a pointer: a global offset is in elements
// from the operand's base pointer (D, E, B, info, logdet), an LDS offset in doubles from the start of the area.
//
// THE SHAPES.  A wavefront carries G = 64 / NP chains in lane groups of NP lanes (NP = 8 / 16 / 32 / 64, the smallest >= n): lane l is
// lane l % NP of group l / NP.  Three ways of looking at a block occur:
//   triangle   potrf_batched.hip's: lane r of a group walks row r of the upper triangle, a loop runs over the columns (a column is contiguous);
//   column     trsm_batched.hip's: lane k of a group owns column k (of E: a column of W; of B: right-hand side pass NP + k), rows in registers;
//   tile       syrk_batched.hip's / gemm_batched.hip's: the 64 wave rows (and columns) w = 16 s + l % 16 are row w % NP of group w / NP, lane l
//              supplies k position q + l / 16 of slab s and holds in accumulator register r of tile (si, sj) wave row 16 si + l % 16, wave
//              column 16 sj + l / 16 + 4 r; a tile exists where both slabs belong to the same group.
//
// THE ADDRESSED CHAIN.  Every global accessor takes a BtChain: where the chain's blocks start in D, E and B, how many positions it has and
// which entry of info / logdet is its own.  Two constructors make one - bt_chain_fixed by arithmetic from the launch (chain wg G + group,
// `stride` apart), bt_chain_plan from a record of a ragged plan (slots of ONE sequence per operand, stacked right-hand sides) - and nothing
// below them knows which.  A lane group without a chain (beyond `batch`, beyond the plan's list) and a chain without a position have
// T = 0: that turns every predicate off.  The chain asked about is the lane's own where the lane walks a row or a column of its group, the
// chain of the WAVE ROW (bt_row_group) where it holds a tile element or supplies a slab - a lane then asks about another group's chain.
// POSITIONS: the wavefront walks steps 0 .. (the largest T of its groups) - 1.  Ascending (factor, forward sweep) step s is position s of
// every chain.  Descending (backward sweep, selected inverse) step s is position T - 1 - s of the ADDRESSED chain: every chain starts at
// step 0 with its own last position and is active while s < T in both directions - there is no joining in the middle of a walk.  What a
// chain does not have (position -1, position T, the coupling block at T - 1) is asked of the same functions and answered `off`.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BT_HD __host__ __device__ __forceinline__
#else
#define BT_HD inline
#endif

constexpr int BT_MAX = 64;             // largest block
constexpr int BT_LDX = 68;             // doubles per line of the exchange area (64 wave columns + 4: the four k positions of a slab start 4 banks apart)

struct BtAt {                          // one access: the offset and whether the lane makes it
  int64_t off;
  bool on;
};

struct BtGeo {                         // one operand of one launch: blocks of n x n, leading dimension ld, `step` apart along a chain
  int64_t ld, step, stride;            // fixed size: chains `stride` apart,
  int64_t T, batch;                    // T positions each (the operand holds T blocks for D, T - 1 for E), `batch` chains; a plan uses none of the three
  int n, NP;
};

struct BtChain {                       // the addressed chain
  int64_t d, e, b;                     // its first block in D and in E, its first row of the first right-hand side in B: element offsets
  int64_t T;                           // positions; 0: nothing is addressed
  int64_t id;                          // the entry of info and logdet
};

BT_HD constexpr int bt_padded(const int n) { return n <= 8 ? 8 : n <= 16 ? 16 : n <= 32 ? 32 : 64; }
BT_HD constexpr int bt_group(const int NP, const int w) { return w / NP; }          // lane or wave row / column -> its lane group
BT_HD constexpr int bt_idx(const int NP, const int w) { return w % NP; }            //                           -> its index there
BT_HD constexpr int bt_row_group(const int NP, const int lane, const int s) { return bt_group(NP, s * 16 + (lane & 15)); }   // the group of the lane's wave row in slab s
BT_HD constexpr int64_t bt_chain(const int NP, const int64_t wg, const int w) { return wg * (64 / NP) + bt_group(NP, w); }   // the place in the batch / the plan's list

// FIXED SIZE: group `group` of workgroup wg carries chain wg G + group of `batch` chains of gd.T positions
BT_HD BtChain bt_chain_fixed(const BtGeo& gd, const BtGeo& ge, const int64_t stride_b, const int64_t wg, const int group) {
  const int64_t c = wg * (64 / gd.NP) + group;
  BtChain ch;
  ch.d = c * gd.stride; ch.e = c * ge.stride; ch.b = c * stride_b;
  ch.T = c < gd.batch ? gd.T : 0;
  ch.id = c;
  return ch;
}
// A PLAN: D and E are ONE sequence of n x n slots each, `step` apart; the chain owns slots first .. first + T - 1 of D, slot first + i of E
// holds the coupling between its positions i and i + 1 (the chain's last slot of E is never addressed) and block rows row .. row + T - 1
// of the stacked right-hand sides
BT_HD BtChain bt_chain_plan(const BtGeo& gd, const BtGeo& ge, const int64_t first, const int64_t T, const int64_t row, const int64_t id) {
  BtChain ch;
  ch.d = first * gd.step; ch.e = first * ge.step; ch.b = row * gd.n;
  ch.T = T;
  ch.id = id;
  return ch;
}

BT_HD constexpr bool bt_has_next(const int64_t T, const int64_t pos) { return pos + 1 < T; }   // wave-uniform form: the walk of T steps goes on behind pos
BT_HD constexpr int64_t bt_pos(const BtChain& ch, const int64_t step, const bool desc) { return desc ? ch.T - 1 - step : step; }
BT_HD constexpr bool bt_active(const BtChain& ch, const int64_t pos) { return pos >= 0 && pos < ch.T; }
BT_HD constexpr bool bt_has_next(const BtChain& ch, const int64_t pos) { return pos >= 0 && bt_has_next(ch.T, pos); }   // pos has a coupling block and a successor
// the coupling block and the target segment of the solve's product at a step: ascending E_pos into segment pos + 1, descending E_(pos-1) into pos - 1
BT_HD constexpr int64_t bt_couple_epos(const BtChain& ch, const int64_t step, const bool desc) { return desc ? bt_pos(ch, step, true) - 1 : step; }
BT_HD constexpr int64_t bt_couple_tpos(const BtChain& ch, const int64_t step, const bool desc) { return desc ? bt_pos(ch, step, true) - 1 : step + 1; }

// does tile (si, sj) exist: both slabs carry the same chain(s); upper: only the tiles of the upper triangle (the factor's successor update)
BT_HD constexpr bool bt_tile(const int NP, const int si, const int sj, const bool upper) {
  return (si * 16) / NP == (sj * 16) / NP && (!upper || si <= sj);
}
// wave-uniform: does slab s hold a row below n
BT_HD constexpr bool bt_slab_on(const int NP, const int s, const int n) { return (s * 16) % NP < n; }

// ------------------------------------------------------------------------------------------------ D (g is the geometry of D)
// TRIANGLE of diagonal block `pos` of the lane's own chain: lane -> row, column c (the loads of U or S, the store of every factor)
BT_HD BtAt bt_tri_at(const BtGeo& g, const BtChain& ch, const int lane, const int64_t pos, const int c) {
  const int r = bt_idx(g.NP, lane);
  BtAt a;
  a.on = bt_active(ch, pos) && r <= c && c < g.n;
  a.off = ch.d + pos * g.step + r + (int64_t)c * g.ld;
  return a;
}
// the store of diagonal block `pos` from the mirrored area: lane -> row, column c; fill = 0: the upper triangle (bt_tri_at's set), else the FULL block
BT_HD BtAt bt_full_at(const BtGeo& g, const BtChain& ch, const int lane, const int64_t pos, const int c, const int fill) {
  const int r = bt_idx(g.NP, lane);
  BtAt a;
  a.on = bt_active(ch, pos) && r < g.n && c >= 0 && c < g.n && (fill != 0 || r <= c);
  a.off = ch.d + pos * g.step + r + (int64_t)c * g.ld;
  return a;
}
// TILE of the SUCCESSOR block pos + 1 (the factor reads D_(pos+1) where the rank-n product lands): register r of tile (si, sj); ch is the
// chain of wave row si 16 + lane % 16
BT_HD BtAt bt_next_at(const BtGeo& g, const BtChain& ch, const int lane, const int64_t pos, const int si, const int sj, const int r) {
  const int wi = si * 16 + (lane & 15), wj = sj * 16 + (lane >> 4) + 4 * r;
  const int row = bt_idx(g.NP, wi), col = bt_idx(g.NP, wj);
  BtAt a;
  a.on = bt_group(g.NP, wi) == bt_group(g.NP, wj) && row <= col && col < g.n && bt_has_next(ch, pos);
  a.off = ch.d + (pos + 1) * g.step + row + (int64_t)col * g.ld;
  return a;
}

// ------------------------------------------------------------------------------------------------ E (g is the geometry of E; the chain holds T - 1 blocks)
// COLUMN of coupling block `pos` of the lane's own chain (the factor: W replaces B column by column): lane -> column, row q
BT_HD BtAt bt_ecol_at(const BtGeo& g, const BtChain& ch, const int lane, const int64_t pos, const int q) {
  const int c = bt_idx(g.NP, lane);
  BtAt a;
  a.on = bt_has_next(ch, pos) && c < g.n && q >= 0 && q < g.n;
  a.off = ch.e + pos * g.step + q + (int64_t)c * g.ld;
  return a;
}
// SLAB of coupling block `pos` as an MFMA operand of the solve: slab s, k step q (a multiple of four); ch is the chain of wave row
// s 16 + lane % 16.  trans: the lane supplies W^T(row, k) = W[k, row] (forward sweep), else W(row, k) (backward sweep)
BT_HD BtAt bt_eslab_at(const BtGeo& g, const BtChain& ch, const int lane, const int64_t pos, const int s, const int q, const bool trans) {
  const int w = s * 16 + (lane & 15), row = bt_idx(g.NP, w), k = q + (lane >> 4);
  BtAt a;
  a.on = bt_has_next(ch, pos) && row < g.n && k < g.n;
  a.off = ch.e + pos * g.step + (trans ? k + (int64_t)row * g.ld : row + (int64_t)k * g.ld);
  return a;
}
// TILE of coupling block `pos` (the inverse's store of C_pos from the accumulators): register r of tile (si, sj); ch is the chain of wave
// row si 16 + lane % 16
BT_HD BtAt bt_etile_at(const BtGeo& g, const BtChain& ch, const int lane, const int64_t pos, const int si, const int sj, const int r) {
  const int wi = si * 16 + (lane & 15), wj = sj * 16 + (lane >> 4) + 4 * r;
  const int row = bt_idx(g.NP, wi), col = bt_idx(g.NP, wj);
  BtAt a;
  a.on = bt_group(g.NP, wi) == bt_group(g.NP, wj) && row < g.n && col < g.n && bt_has_next(ch, pos);
  a.off = ch.e + pos * g.step + row + (int64_t)col * g.ld;
  return a;
}

// ------------------------------------------------------------------------------------------------ B, info, logdet
// COLUMN of segment `pos` of the right-hand sides of the lane's own chain: lane -> right-hand side pass NP + lane % NP, row r of the segment
BT_HD BtAt bt_rhs_at(const BtGeo& g, const BtChain& ch, const int64_t ldb, const int64_t nrhs, const int lane, const int64_t pass, const int64_t pos,
                     const int r) {
  const int64_t col = pass * g.NP + bt_idx(g.NP, lane);
  BtAt a;
  a.on = bt_active(ch, pos) && col < nrhs && r >= 0 && r < g.n;
  a.off = ch.b + col * ldb + pos * g.n + r;
  return a;
}
BT_HD constexpr int64_t bt_rhs_passes(const int NP, const int64_t nrhs) { return (nrhs + NP - 1) / NP; }

// the chain's entry of info and logdet: lane 0 of a group whose chain has a position (the entries of empty chains are not written)
BT_HD BtAt bt_scalar_at(const int NP, const BtChain& ch, const int lane) {
  BtAt a;
  a.on = ch.T > 0 && bt_idx(NP, lane) == 0;
  a.off = ch.id;
  return a;
}
// every lane of such a group reads its chain's info in the solve and the inverse
BT_HD BtAt bt_info_at(const BtChain& ch) {
  BtAt a;
  a.on = ch.T > 0;
  a.off = ch.id;
  return a;
}

// ------------------------------------------------------------------------------------------------ LDS
// the factor image of a group (batched_small.h's PbImg<NP>::at, restated for the sweep; the kernels assert that the two agree)
BT_HD constexpr int bt_img_ld(const int NP) { return NP + 2; }
BT_HD constexpr int bt_img_size(const int NP) { return (NP / 2) * bt_img_ld(NP); }
BT_HD constexpr int bt_img_at(const int NP, const int r, const int c) {
  return r < NP / 2 ? r * bt_img_ld(NP) + (c - r) : (NP - 1 - r) * bt_img_ld(NP) + c + 1;
}
BT_HD constexpr int bt_img_base(const int NP, const int lane) { return bt_group(NP, lane) * bt_img_size(NP); }

// the 64 logarithms of the wavefront's diagonals: entry j of the lane's group
BT_HD constexpr int bt_log_at(const int NP, const int lane, const int j) { return bt_group(NP, lane) * NP + j; }

// the exchange area of the wavefront: NP lines of BT_LDX doubles; line q holds row q of the 64 columns the lanes own
BT_HD constexpr int bt_x_size(const int NP) { return NP * BT_LDX; }
BT_HD constexpr int bt_x_own(const int q, const int lane) { return q * BT_LDX + lane; }          // the lane's own column, row q
// as an MFMA operand: slab s, k step q: the lane supplies (k = q + lane / 16, wave column 16 s + lane % 16); off below k < n
BT_HD BtAt bt_x_slab(const int n, const int lane, const int s, const int q) {
  const int k = q + (lane >> 4);
  BtAt a;
  a.on = k < n;
  a.off = k * BT_LDX + s * 16 + (lane & 15);
  return a;
}
// the solve's product, register r of tile (si, sj), goes to row `row` of the column of the lane that owns wave column wj
BT_HD BtAt bt_x_tile(const int n, const int NP, const int lane, const int si, const int sj, const int r) {
  const int wi = si * 16 + (lane & 15), wj = sj * 16 + (lane >> 4) + 4 * r;
  BtAt a;
  a.on = bt_group(NP, wi) == bt_group(NP, wj) && bt_idx(NP, wi) < n;
  a.off = bt_idx(NP, wi) * BT_LDX + wj;
  return a;
}
// the factor's successor, register r of tile (si, sj): element (row, col) of the image of the group of wave row wi; on exactly where
// bt_next_at is, for a chain with a successor
BT_HD BtAt bt_img_tile(const int n, const int NP, const int lane, const int si, const int sj, const int r) {
  const int wi = si * 16 + (lane & 15), wj = sj * 16 + (lane >> 4) + 4 * r;
  const int row = bt_idx(NP, wi), col = bt_idx(NP, wj);
  BtAt a;
  a.on = bt_group(NP, wi) == bt_group(NP, wj) && row <= col && col < n;
  a.off = bt_img_base(NP, wi) + bt_img_at(NP, row, col);
  return a;
}

// An exchange area read by bt_x_slab holds element (x, k) of the block of wave index w = group NP + x at line k, word w.  Three stores of
// the selected inverse fill one:
// the lane that owns COLUMN k = lane % NP of its group's block (G_i after the substitution) writes its rows x along its own line;
BT_HD constexpr int bt_xt_own(const int NP, const int x, const int lane) { return bt_idx(NP, lane) * BT_LDX + bt_group(NP, lane) * NP + x; }
// register r of tile (si, sj) holds element (row, col) of the block of wave row wi (C_i for the second product): line col, word wi;
BT_HD BtAt bt_xt_tile(const int n, const int NP, const int lane, const int si, const int sj, const int r) {
  const int wi = si * 16 + (lane & 15), wj = sj * 16 + (lane >> 4) + 4 * r;
  BtAt a;
  a.on = bt_group(NP, wi) == bt_group(NP, wj) && bt_idx(NP, wi) < n && bt_idx(NP, wj) < n;
  a.off = bt_idx(NP, wj) * BT_LDX + wi;
  return a;
}
// THE MIRRORED AREA: register r of an upper tile holds element (row, col), row <= col, of the symmetric block: it goes to line row, word wj
// and (mirror, row < col only) to line col, word wi - every word (x, k), x, k < n, of every group exactly once.  Lane l then finds column
// cc of row l % NP of its group's block at bt_x_own(cc, l).
BT_HD BtAt bt_sig_tile(const int n, const int NP, const int lane, const int si, const int sj, const int r, const bool mirror) {
  const int wi = si * 16 + (lane & 15), wj = sj * 16 + (lane >> 4) + 4 * r;
  const int row = bt_idx(NP, wi), col = bt_idx(NP, wj);
  BtAt a;
  a.on = bt_group(NP, wi) == bt_group(NP, wj) && col < n && (mirror ? row < col : row <= col);
  a.off = mirror ? col * BT_LDX + wi : row * BT_LDX + wj;
  return a;
}
// both exchange areas (contiguous) start as +0.0: pass j of the lanes over 2 bt_x_size(NP) doubles
BT_HD constexpr int bt_x_clear_passes(const int NP) { return (2 * bt_x_size(NP) + 63) / 64; }
BT_HD BtAt bt_x_clear(const int NP, const int lane, const int j) {
  BtAt a;
  a.off = (int64_t)j * 64 + lane;
  a.on = a.off < 2 * bt_x_size(NP);
  return a;
}

// THE TABLE of the G <= 8 chains of a wavefront on a plan, in LDS: BT_TAB int64 per group (d, e, b, T, id); lane 0 of every group writes
// its entry.  A fixed-size launch has none: a chain there is arithmetic.
constexpr int BT_TAB = 5;
BT_HD constexpr int bt_tab_at(const int group, const int field) { return group * BT_TAB + field; }
BT_HD constexpr int bt_tab_size() { return 8 * BT_TAB; }
