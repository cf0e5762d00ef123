// The address arithmetic of blocktri_batched.hip: which element of D, E, B, info / logdet and of the two LDS areas a lane touches at a
// chain position, and whether it touches it at all - as functions the kernels call AND a plain C++ program can call
// (tests/test_blocktri_addr.py replays the kernels' loops on the CPU, lane by lane, over the rows of tests/blocktri_cases.py: every
// addressed offset inside its block, no E block and no successor at position T - 1, no E at all with T = 1, nothing from a dead lane
// group, the written set exactly the triangles, the E blocks and the right-hand-side segments).  The kernels form no address any other way.
// Nothing here knows a pointer: a global offset is in elements from the operand's base pointer (D, E, B, info, logdet), an LDS offset in
// doubles from the start of the area.
//
// THE SHAPES.  A wavefront carries G = 64 / NP chains in lane groups of NP lanes (NP = 8 / 16 / 32 / 64, the smallest >= n): lane l belongs
// to chain wg G + l / NP and is lane l % NP of its group.  Three ways of looking at a block occur:
//   triangle   potrf_batched.hip's: lane r of a group walks row r of the upper triangle, a loop runs over the columns (a column is contiguous);
//   column     trsm_batched.hip's: lane k of a group owns column k (of E: a column of W; of B: right-hand side pass NP + k), rows in registers;
//   tile       syrk_batched.hip's / gemm_batched.hip's: the 64 wave rows (and columns) w = 16 s + l % 16 are row w % NP of chain w / NP, lane l
//              supplies k position q + l / 16 of slab s and holds in accumulator register r of tile (si, sj) wave row 16 si + l % 16, wave
//              column 16 sj + l / 16 + 4 r; a tile exists where both slabs belong to the same chain.
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

struct BtGeo {                         // one operand of one launch: blocks of n x n, leading dimension ld, `step` apart along a chain, chains `stride` apart
  int64_t ld, step, stride;
  int64_t T, batch;                    // positions of a chain (the operand holds T blocks for D, T - 1 for E), chains
  int n, NP;
};

BT_HD constexpr int bt_padded(const int n) { return n <= 8 ? 8 : n <= 16 ? 16 : n <= 32 ? 32 : 64; }
BT_HD constexpr int bt_group(const int NP, const int w) { return w / NP; }          // lane or wave row / column -> its lane group
BT_HD constexpr int bt_idx(const int NP, const int w) { return w % NP; }            //                           -> its index there
BT_HD constexpr int64_t bt_chain(const int NP, const int64_t wg, const int w) { return wg * (64 / NP) + bt_group(NP, w); }
BT_HD constexpr bool bt_live(const BtGeo& g, const int64_t wg, const int w) { return bt_chain(g.NP, wg, w) < g.batch; }
BT_HD constexpr bool bt_has_next(const int64_t T, const int64_t pos) { return pos + 1 < T; }   // position pos has a coupling block and a successor
BT_HD constexpr int64_t bt_block(const BtGeo& g, const int64_t chain, const int64_t pos) { return chain * g.stride + pos * g.step; }

// does tile (si, sj) exist: both slabs carry the same chain(s); upper: only the tiles of the upper triangle (the factor's successor update)
BT_HD constexpr bool bt_tile(const int NP, const int si, const int sj, const bool upper) {
  return (si * 16) / NP == (sj * 16) / NP && (!upper || si <= sj);
}
// wave-uniform: does slab s hold a row below n
BT_HD constexpr bool bt_slab_on(const int NP, const int s, const int n) { return (s * 16) % NP < n; }

// ------------------------------------------------------------------------------------------------ D
// TRIANGLE of diagonal block `pos`: lane -> row, column c (the first load of a chain, the store of every factor, the solve's load of U)
BT_HD BtAt bt_tri_at(const BtGeo& g, const int64_t wg, const int lane, const int64_t pos, const int c) {
  const int r = bt_idx(g.NP, lane);
  BtAt a;
  a.on = bt_live(g, wg, lane) && pos >= 0 && pos < g.T && r <= c && c < g.n;
  a.off = bt_block(g, bt_chain(g.NP, wg, lane), pos) + r + (int64_t)c * g.ld;
  return a;
}

// TILE of the SUCCESSOR block pos + 1 (the factor reads D_(pos+1) where the rank-n product lands): register r of tile (si, sj)
BT_HD BtAt bt_next_at(const BtGeo& g, const int64_t wg, const int lane, const int64_t pos, const int si, const int sj, const int r) {
  const int lr = lane & 15, kg = lane >> 4;
  const int wi = si * 16 + lr, wj = sj * 16 + kg + 4 * r;
  const int row = bt_idx(g.NP, wi), col = bt_idx(g.NP, wj);
  BtAt a;
  a.on = bt_group(g.NP, wi) == bt_group(g.NP, wj) && row <= col && col < g.n && bt_live(g, wg, wi) && pos >= 0 && bt_has_next(g.T, pos);
  a.off = bt_block(g, bt_chain(g.NP, wg, wi), pos + 1) + row + (int64_t)col * g.ld;
  return a;
}

// ------------------------------------------------------------------------------------------------ E (g.T is the chain's T: E holds T - 1 blocks)
// COLUMN of coupling block `pos` (the factor: W replaces B column by column): lane -> column, row q
BT_HD BtAt bt_ecol_at(const BtGeo& g, const int64_t wg, const int lane, const int64_t pos, const int q) {
  const int c = bt_idx(g.NP, lane);
  BtAt a;
  a.on = bt_live(g, wg, lane) && pos >= 0 && bt_has_next(g.T, pos) && c < g.n && q >= 0 && q < g.n;
  a.off = bt_block(g, bt_chain(g.NP, wg, lane), pos) + q + (int64_t)c * g.ld;
  return a;
}

// SLAB of coupling block `pos` as an MFMA operand of the solve: slab s, k step q (a multiple of four).  trans: the lane supplies
// W^T(row, k) = W[k, row] (forward sweep), else W(row, k) (backward sweep)
BT_HD BtAt bt_eslab_at(const BtGeo& g, const int64_t wg, const int lane, const int64_t pos, const int s, const int q, const bool trans) {
  const int lr = lane & 15, kg = lane >> 4;
  const int w = s * 16 + lr, row = bt_idx(g.NP, w), k = q + kg;
  BtAt a;
  a.on = bt_live(g, wg, w) && pos >= 0 && bt_has_next(g.T, pos) && row < g.n && k < g.n;
  a.off = bt_block(g, bt_chain(g.NP, wg, w), pos) + (trans ? k + (int64_t)row * g.ld : row + (int64_t)k * g.ld);
  return a;
}

// ------------------------------------------------------------------------------------------------ B, info, logdet
// COLUMN of segment `pos` of the right-hand sides: lane -> right-hand side pass NP + lane % NP, row r of the segment (row pos n + r of the system)
BT_HD BtAt bt_rhs_at(const BtGeo& g, const int64_t ldb, const int64_t stride_b, const int64_t nrhs, const int64_t wg, const int lane, const int64_t pass,
                     const int64_t pos, const int r) {
  const int64_t col = pass * g.NP + bt_idx(g.NP, lane);
  BtAt a;
  a.on = bt_live(g, wg, lane) && col < nrhs && pos >= 0 && pos < g.T && r >= 0 && r < g.n;
  a.off = bt_chain(g.NP, wg, lane) * stride_b + col * ldb + pos * g.n + r;
  return a;
}
BT_HD constexpr int64_t bt_rhs_passes(const int NP, const int64_t nrhs) { return (nrhs + NP - 1) / NP; }

// the chain's entry of info and logdet: lane 0 of a live group
BT_HD BtAt bt_scalar_at(const BtGeo& g, const int64_t wg, const int lane) {
  BtAt a;
  a.on = bt_live(g, wg, lane) && bt_idx(g.NP, lane) == 0;
  a.off = bt_chain(g.NP, wg, lane);
  return a;
}
// every lane of a live group reads its chain's info in the solve
BT_HD BtAt bt_info_at(const BtGeo& g, const int64_t wg, const int lane) {
  BtAt a;
  a.on = bt_live(g, wg, lane);
  a.off = bt_chain(g.NP, wg, lane);
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
// bt_next_at is, for a live group with a successor
BT_HD BtAt bt_img_tile(const int n, const int NP, const int lane, const int si, const int sj, const int r) {
  const int wi = si * 16 + (lane & 15), wj = sj * 16 + (lane >> 4) + 4 * r;
  const int row = bt_idx(NP, wi), col = bt_idx(NP, wj);
  BtAt a;
  a.on = bt_group(NP, wi) == bt_group(NP, wj) && row <= col && col < n;
  a.off = bt_img_base(NP, wi) + bt_img_at(NP, row, col);
  return a;
}

// ------------------------------------------------------------------------------------------------ the selected inverse (blocktri_potri_batched.hip)
// THE DESCENDING WALK: step 0 is position T - 1, the last step position 0, which has no predecessor.  What position pos - 1 needs is asked
// of bt_tri_at and bt_ecol_at at pos - 1: both are off at position -1.
BT_HD constexpr int64_t bt_walk_pos(const int64_t T, const int64_t step) { return T - 1 - step; }
BT_HD constexpr bool bt_has_prev(const int64_t pos) { return pos > 0; }

// the store of diagonal block `pos` from the mirrored area: lane -> row, column c; fill = 0: the upper triangle (bt_tri_at's set), else the FULL block
BT_HD BtAt bt_full_at(const BtGeo& g, const int64_t wg, const int lane, const int64_t pos, const int c, const int fill) {
  const int r = bt_idx(g.NP, lane);
  BtAt a;
  a.on = bt_live(g, wg, lane) && pos >= 0 && pos < g.T && r < g.n && c >= 0 && c < g.n && (fill != 0 || r <= c);
  a.off = bt_block(g, bt_chain(g.NP, wg, lane), pos) + r + (int64_t)c * g.ld;
  return a;
}

// TILE of coupling block `pos` (the store of C_pos from the accumulators): register r of tile (si, sj)
BT_HD BtAt bt_etile_at(const BtGeo& g, const int64_t wg, const int lane, const int64_t pos, const int si, const int sj, const int r) {
  const int wi = si * 16 + (lane & 15), wj = sj * 16 + (lane >> 4) + 4 * r;
  const int row = bt_idx(g.NP, wi), col = bt_idx(g.NP, wj);
  BtAt a;
  a.on = bt_group(g.NP, wi) == bt_group(g.NP, wj) && row < g.n && col < g.n && bt_live(g, wg, wi) && pos >= 0 && bt_has_next(g.T, pos);
  a.off = bt_block(g, bt_chain(g.NP, wg, wi), pos) + row + (int64_t)col * g.ld;
  return a;
}

// An exchange area read by bt_x_slab holds element (x, k) of the block of wave index w = group NP + x at line k, word w.  Three stores fill one:
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

// ------------------------------------------------------------------------------------------------ ragged chains (blocktri_vbatched.hip)
// CHAINS OF DIFFERENT LENGTHS on a plan: D and E are ONE sequence of n x n slots, `step` apart (BtGeo::stride, T and batch are not used);
// chain c owns slots first .. first + T - 1 of D, and slot first + i of E holds the coupling between its positions i and i + 1 - the last
// slot of a chain is never addressed.  The right-hand sides are stacked: the chain owns block rows row .. row + T - 1 of B.  A wavefront
// carries the G chains at wg G .. wg G + G - 1 of the plan's sorted list; a lane group beyond the list, or one whose chain has T = 0, is
// DEAD: T = 0 turns every predicate off.
// The accessors take the ADDRESSED chain as values: the lane's own chain where the lane walks a row or a column of its group, the chain of
// the WAVE ROW (btv_row_group) where it holds a tile element or supplies a slab - a lane then asks about another group's chain.
// POSITIONS: the wavefront walks steps 0 .. (its largest T) - 1.  Ascending (factor, forward sweep) step s is position s of every chain.
// Descending (backward sweep, selected inverse) step s is position T - 1 - s of the ADDRESSED chain (bt_walk_pos with that chain's T):
// every chain starts at step 0 with its own last position, exactly as the fixed-size kernels start, and a chain is active while s < T in
// both directions - there is no joining in the middle of a walk.  What a chain does not have (position -1, position T, the coupling block
// at T - 1) is asked of the same functions and answered `off`.
struct BtChain {
  int64_t first, T, row;               // first slot, positions, first block row of the stacked right-hand sides
  int64_t id;                          // index in batch order: the entry of info and logdet
};

BT_HD constexpr int btv_row_group(const int NP, const int lane, const int s) { return bt_group(NP, s * 16 + (lane & 15)); }   // the group of the lane's wave row in slab s
BT_HD constexpr int64_t btv_pos(const BtChain& ch, const int64_t step, const bool desc) { return desc ? bt_walk_pos(ch.T, step) : step; }
BT_HD constexpr bool btv_active(const BtChain& ch, const int64_t pos) { return pos >= 0 && pos < ch.T; }
BT_HD constexpr bool btv_has_next(const BtChain& ch, const int64_t pos) { return pos >= 0 && bt_has_next(ch.T, pos); }
BT_HD constexpr bool btv_has_prev(const BtChain& ch, const int64_t pos) { return bt_has_prev(pos) && pos < ch.T; }
BT_HD constexpr int64_t btv_block(const BtGeo& g, const BtChain& ch, const int64_t pos) { return (ch.first + pos) * g.step; }
// the coupling block and the target segment of the solve's product at a step: ascending E_pos into segment pos + 1, descending E_(pos-1) into pos - 1
BT_HD constexpr int64_t btv_couple_epos(const BtChain& ch, const int64_t step, const bool desc) { return desc ? btv_pos(ch, step, true) - 1 : step; }
BT_HD constexpr int64_t btv_couple_tpos(const BtChain& ch, const int64_t step, const bool desc) { return desc ? btv_pos(ch, step, true) - 1 : step + 1; }

// bt_tri_at on the lane's own chain
BT_HD BtAt btv_tri_at(const BtGeo& g, const BtChain& ch, const int lane, const int64_t pos, const int c) {
  const int r = bt_idx(g.NP, lane);
  BtAt a;
  a.on = btv_active(ch, pos) && r <= c && c < g.n;
  a.off = btv_block(g, ch, pos) + r + (int64_t)c * g.ld;
  return a;
}
// bt_next_at; ch is the chain of wave row si 16 + lane % 16
BT_HD BtAt btv_next_at(const BtGeo& g, const BtChain& ch, const int lane, const int64_t pos, const int si, const int sj, const int r) {
  const int wi = si * 16 + (lane & 15), wj = sj * 16 + (lane >> 4) + 4 * r;
  const int row = bt_idx(g.NP, wi), col = bt_idx(g.NP, wj);
  BtAt a;
  a.on = bt_group(g.NP, wi) == bt_group(g.NP, wj) && row <= col && col < g.n && btv_has_next(ch, pos);
  a.off = btv_block(g, ch, pos + 1) + row + (int64_t)col * g.ld;
  return a;
}
// bt_ecol_at on the lane's own chain
BT_HD BtAt btv_ecol_at(const BtGeo& g, const BtChain& ch, const int lane, const int64_t pos, const int q) {
  const int c = bt_idx(g.NP, lane);
  BtAt a;
  a.on = btv_has_next(ch, pos) && c < g.n && q >= 0 && q < g.n;
  a.off = btv_block(g, ch, pos) + q + (int64_t)c * g.ld;
  return a;
}
// bt_eslab_at; ch is the chain of wave row s 16 + lane % 16
BT_HD BtAt btv_eslab_at(const BtGeo& g, const BtChain& ch, const int lane, const int64_t pos, const int s, const int q, const bool trans) {
  const int w = s * 16 + (lane & 15), row = bt_idx(g.NP, w), k = q + (lane >> 4);
  BtAt a;
  a.on = btv_has_next(ch, pos) && row < g.n && k < g.n;
  a.off = btv_block(g, ch, pos) + (trans ? k + (int64_t)row * g.ld : row + (int64_t)k * g.ld);
  return a;
}
// bt_rhs_at on the lane's own chain: row (ch.row + pos) n + r of the stacked system
BT_HD BtAt btv_rhs_at(const BtGeo& g, const BtChain& ch, const int64_t ldb, const int64_t nrhs, const int lane, const int64_t pass, const int64_t pos,
                      const int r) {
  const int64_t col = pass * g.NP + bt_idx(g.NP, lane);
  BtAt a;
  a.on = btv_active(ch, pos) && col < nrhs && r >= 0 && r < g.n;
  a.off = col * ldb + (ch.row + pos) * g.n + r;
  return a;
}
// the chain's entry of info and logdet: lane 0 of a group whose chain has a position (the entries of empty chains are not written)
BT_HD BtAt btv_scalar_at(const int NP, const BtChain& ch, const int lane) {
  BtAt a;
  a.on = ch.T > 0 && bt_idx(NP, lane) == 0;
  a.off = ch.id;
  return a;
}
BT_HD BtAt btv_info_at(const BtChain& ch) {
  BtAt a;
  a.on = ch.T > 0;
  a.off = ch.id;
  return a;
}
// bt_full_at on the lane's own chain
BT_HD BtAt btv_full_at(const BtGeo& g, const BtChain& ch, const int lane, const int64_t pos, const int c, const int fill) {
  const int r = bt_idx(g.NP, lane);
  BtAt a;
  a.on = btv_active(ch, pos) && r < g.n && c >= 0 && c < g.n && (fill != 0 || r <= c);
  a.off = btv_block(g, ch, pos) + r + (int64_t)c * g.ld;
  return a;
}
// bt_etile_at; ch is the chain of wave row si 16 + lane % 16
BT_HD BtAt btv_etile_at(const BtGeo& g, const BtChain& ch, const int lane, const int64_t pos, const int si, const int sj, const int r) {
  const int wi = si * 16 + (lane & 15), wj = sj * 16 + (lane >> 4) + 4 * r;
  const int row = bt_idx(g.NP, wi), col = bt_idx(g.NP, wj);
  BtAt a;
  a.on = bt_group(g.NP, wi) == bt_group(g.NP, wj) && row < g.n && col < g.n && btv_has_next(ch, pos);
  a.off = btv_block(g, ch, pos) + row + (int64_t)col * g.ld;
  return a;
}
// THE TABLE of the wavefront's G <= 8 chains in LDS: BTV_TAB int64 per group (first, T, row, id); lane 0 of every group writes its entry
constexpr int BTV_TAB = 4;
BT_HD constexpr int btv_tab_at(const int group, const int field) { return group * BTV_TAB + field; }
BT_HD constexpr int btv_tab_size() { return 8 * BTV_TAB; }
