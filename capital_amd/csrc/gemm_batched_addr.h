// The address arithmetic of gemm_batched.hip: which element of op(A), op(B) and C a lane touches, and whether it touches it at all - as
// functions the kernels call AND a plain C++ program can call (tests/test_gemm_batched_addr.py sweeps them on the CPU, lane by lane, over
// the shapes of tests/gemm_batched_cases.py: every addressed offset inside its operand, the addressed set of C exactly the rectangle).
// Nothing here knows a pointer: an offset is in elements from the first element of the block's operand.
//
// THE TILES (gemm_batched.hip has the full account).  A wavefront works on a MACRO TILE: four row slabs of 16 rows of op(A) against NJ
// column slabs of 16 columns of op(B).  Lane l supplies, per k step of four, element (16 s + l % 16, q + l / 16) of slab s - for op(A) the
// row, for op(B) the column - and holds in accumulator register r of tile (si, sj) the element of wave row 16 si + l % 16 and wave column
// 16 sj + l / 16 + 4 r.  With NP < 64 rows to a block the 64 wave rows (and columns) are 64 / NP blocks of NP: wave row w is row
// base + w % NP of block w / NP of the wavefront, and a tile exists where its row slab and its column slab belong to the same block.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GM_HD __host__ __device__ __forceinline__
#else
#define GM_HD inline
#endif

constexpr int GM_MAX = 256;            // largest m and n
constexpr int GM_ROWS = 64;            // rows of a macro tile (four slabs)
constexpr int GM_GROUP_NJ = 2;         // column slabs of a macro tile of the workgroup path: 64 rows x 32 columns

struct GmAt {                          // one access: the offset in elements and whether the lane makes it
  int64_t off;
  bool on;
};

// the block of the wavefront that wave row / column w belongs to, and its index in that block
GM_HD constexpr int gm_sub(const int NP, const int w) { return w / NP; }
GM_HD constexpr int gm_idx(const int NP, const int base, const int w) { return base + w % NP; }

// does tile (si, sj) exist: both slabs carry the same block(s)
GM_HD constexpr bool gm_tile(const int NP, const int si, const int sj) { return (si * 16) / NP == (sj * 16) / NP; }

// wave-uniform: does slab s hold a row (column) below lim, the largest m (n) of the wavefront
GM_HD constexpr bool gm_slab_on(const int NP, const int base, const int s, const int lim) { return base + (s * 16) % NP < lim; }

// strides of an operand along its rows (A: the rows of op(A); B: the columns of op(B)) and along k.  kcontig: k is the contiguous
// direction - A with CAP_TRANS (stored k x m), B with CAP_NOTRANS (stored k x n).
GM_HD constexpr int64_t gm_stride_i(const bool kcontig, const int64_t ld) { return kcontig ? ld : 1; }
GM_HD constexpr int64_t gm_stride_q(const bool kcontig, const int64_t ld) { return kcontig ? 1 : ld; }

// THE LOADER: what lane `lane` reads for slab s of the macro tile whose slabs start at `base`, at k step q (a multiple of four); lim = m
// (op(A)) or n (op(B)) of the lane's block, k its contraction length
GM_HD GmAt gm_load_at(const int64_t si, const int64_t sq, const int lim, const int64_t k, const int NP, const int base, const int s, const int lane,
                      const int64_t q) {
  const int lr = lane & 15, kg = lane >> 4;
  const int i = gm_idx(NP, base, s * 16 + lr);
  GmAt a;
  a.on = i < lim && q + kg < k;
  a.off = i * si + (q + kg) * sq;
  return a;
}

// THE STORE (and, with beta != 0, the read in front of it): register r of tile (si, sj) of the macro tile at (I0, J0)
GM_HD GmAt gm_store_at(const int m, const int n, const int64_t ldc, const int NP, const int I0, const int J0, const int si, const int sj, const int lane,
                       const int r) {
  const int lr = lane & 15, kg = lane >> 4;
  const int wi = si * 16 + lr, wj = sj * 16 + kg + 4 * r;
  const int row = gm_idx(NP, I0, wi), col = gm_idx(NP, J0, wj);
  GmAt a;
  a.on = gm_sub(NP, wi) == gm_sub(NP, wj) && row < m && col < n;
  a.off = row + (int64_t)col * ldc;
  return a;
}

// THE WAVE PATH (a wavefront per 64 / NP blocks): column passes of NP columns, J0 = pass * NP; the rows fit one pass (m <= NP)
GM_HD constexpr int gm_wave_passes(const int NP, const int n) { return (n + NP - 1) / NP; }

// THE WORKGROUP PATH (a workgroup of four waves per block): macro tiles of 64 rows x 32 columns, down the rows first; tile t goes to wave
// t % 4
GM_HD constexpr int gm_group_tiles(const int m, const int n) { return ((m + GM_ROWS - 1) / GM_ROWS) * ((n + 16 * GM_GROUP_NJ - 1) / (16 * GM_GROUP_NJ)); }
GM_HD constexpr int gm_group_I0(const int t, const int m) { return (t % ((m + GM_ROWS - 1) / GM_ROWS)) * GM_ROWS; }
GM_HD constexpr int gm_group_J0(const int t, const int m) { return (t / ((m + GM_ROWS - 1) / GM_ROWS)) * 16 * GM_GROUP_NJ; }
