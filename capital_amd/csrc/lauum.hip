// fp64 triangular product C(upper) = W W^T, W upper triangular (LAPACK dlauum, out of place) on v_mfma_f64_16x16x4_f64 for gfx950,
// and the small kernels of the SPD inverse / log-determinant built on it (mirror of the upper triangle, NaN fill, sum of log r_ii).
//
// A^-1 = R^-1 R^-T is this product with W = R^-1.  Not in the reference: cholinv stops at R, R^-1 (cholinv.hpp:30-46).
//
// dlauum_nt_kernel: C[i][j] = sum_{k >= j} W[i][k] W[j][k] for i <= j - the NT form, both operands row blocks of W and therefore
// M-contiguous in column-major storage, the K range cut to the staircase (n^3 / 3 flops instead of the n^3 of an upper-tile SYRK with dense K).
//   * one 128 x 128 C tile per workgroup, 4 waves of 64 x 64, K tile 16: the register pattern and the rotated double-buffered LDS-DMA
//     pipeline of gemm.hip's tn_dma_tile, with BOTH operands staged as the [k][128] half-swapped image of its M-contiguous A operand;
//   * only tiles ti <= tj exist; tile (ti, tj) walks k from 128 tj to n;
//   * the first 128 k of that walk (the diagonal K block) hold elements with k < row in operand B (and in A on a diagonal tile): the
//     strictly lower triangle of W, which the contract says is garbage.  Those 8 K tiles are staged through registers with a select
//     (never a multiply: the garbage may be NaN) and their all-zero 16 x 16 blocks are skipped with wave-uniform branches; every later
//     K tile is dense and runs the unbranched pipeline;
//   * plain stores, diagonal tiles masked to row <= col: nothing below the diagonal of C is written.
// Tile order (CAP_LAUUM_ORDER, DESIGN.md "SPD inverse"): block b runs on XCD b % 8; XCD x owns the tile COLUMNS tj = x, x + 8, ... and walks
// them in ascending order, rows ascending inside a column.  Work per tile falls with tj, so every XCD starts with its longest tiles;
// the tiles resident on an XCD at one time belong to one or two columns, walk the same K range in step and share operand B's row panel
// (and, one column later, operand A's panels) in that XCD's L2.
#include <algorithm>
#include <type_traits>

#include "common.h"

namespace {

constexpr int LT = 128, LK = 16, LTHREADS = 256;
constexpr int L_TILE = LT * LK;          // doubles per operand tile (16 KiB)
constexpr int L_DIAG_KT = LT / LK;       // K tiles of the diagonal K block

#ifndef CAP_LAUUM_ORDER
#define CAP_LAUUM_ORDER 1                // 1: tile columns per XCD (see above); 0: the plain column-major triangle walk (measurement only)
#endif

struct LauumArgs {
  const double* W; double* C;
  int64_t ldw, ldc;
  int T;                                 // tiles per side (n / 128)
};

// block -> tile; false: the block has no tile (the XCDs' lists differ in length)
__device__ __forceinline__ bool lauum_block_to_tile(int T, int b, int& ti, int& tj) {
  int s = CAP_LAUUM_ORDER == 1 ? (b >> 3) : b;
  for (int c = CAP_LAUUM_ORDER == 1 ? (b & 7) : 0; c < T; c += (CAP_LAUUM_ORDER == 1 ? 8 : 1)) {
    if (s <= c) { ti = s; tj = c; return true; }
    s -= c + 1;
  }
  return false;
}
int64_t lauum_grid(int64_t T) {
  if (CAP_LAUUM_ORDER != 1) return T * (T + 1) / 2;
  int64_t most = 0;
  for (int64_t x = 0; x < 8; x++) {
    int64_t cnt = 0;
    for (int64_t c = x; c < T; c += 8) cnt += c + 1;
    most = std::max(most, cnt);
  }
  return most * 8;
}

__global__ void __launch_bounds__(LTHREADS, 2) dlauum_nt_kernel(const LauumArgs g) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  int ti, tj;
  if (!lauum_block_to_tile(g.T, (int)blockIdx.x, ti, tj)) return;
  const int64_t i0 = (int64_t)ti * LT, j0 = (int64_t)tj * LT;
  const int t = threadIdx.x, lane = t & 63;
  const int wid_s = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wi = (wid_s & 1) * 64, wj = (wid_s >> 1) * 64;
  const int lr = lane & 15, kg = lane >> 4;
  const bool diag = ti == tj;
  const int nk = (int)(((int64_t)g.T * LT - j0) / LK);      // >= 8

  // LDS carve: [A0][B0][A1][B1], 16 KiB each
  auto sA = [&](int buf) -> double* { return smem + buf * 2 * L_TILE; };
  auto sB = [&](int buf) -> double* { return smem + buf * 2 * L_TILE + L_TILE; };

  d4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};

  // fragments of an 8-deep half tile (h8 = 0 / 8): x / y take k = h8 + 2 kg and h8 + 2 kg + 1 on both operands (the same permutation, so
  // the sum over k is unchanged); rows with (k >> 1) odd are stored with their 128-byte segments swapped in pairs: ds_read_b64 stays conflict free
  const int flip = (kg & 1) << 4;
  auto read_frags = [&](const double* tA, const double* tB, int h8, d2 (&fa)[4], d2 (&fb)[4]) {
    const double* ra = tA + (h8 + 2 * kg) * LT;
    const double* rb = tB + (h8 + 2 * kg) * LT;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int m = (wi + 16 * i + lr) ^ flip;
      fa[i] = (d2){ra[m], ra[LT + m]};
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int m = (wj + 16 * j + lr) ^ flip;
      fb[j] = (d2){rb[m], rb[LT + m]};
    }
  };
  d2 fa0[4], fb0[4], fa1[4], fb1[4];

  // ---- the diagonal K block, k in [j0, j0 + 128): register-staged, masked to k >= row, dead blocks skipped ------------------------------
  {
    // thread t stages the pairs (k = c >> 6, rows 2 (c & 63), + 1), c = t + 256 s: 16-byte loads along the contiguous rows
    auto load_masked = [&](int64_t o0, int64_t k0, d2 (&r)[4]) {
#pragma unroll
      for (int s = 0; s < 4; s++) {
        const int c = t + LTHREADS * s;
        const int64_t k = k0 + (c >> 6), row = o0 + (c & 63) * 2;
        const d2 v = *reinterpret_cast<const d2*>(g.W + k * g.ldw + row);
        r[s] = (d2){k >= row ? v.x : 0.0, k >= row + 1 ? v.y : 0.0};
      }
    };
    auto store_mc = [&](double* lds, const d2 (&r)[4]) {
#pragma unroll
      for (int s = 0; s < 4; s++) {
        const int c = t + LTHREADS * s;
        const int k = c >> 6, o2 = (c & 63) * 2;
        *reinterpret_cast<d2*>(lds + k * LT + (o2 ^ (((k >> 1) & 1) << 4))) = r[s];
      }
    };
    // kr: first k of the half tile relative to j0.  Block column j (rows wj + 16 j ... of operand B) is all zero while kr + 7 < wj + 16 j;
    // on a diagonal tile the same holds for operand A's block rows, and blocks entirely below the diagonal of C are never stored.
    auto mma_skip = [&](const d2 (&fa)[4], const d2 (&fb)[4], int kr) {
      const int dj = kr + 7 - wj, di = kr + 7 - wi;
      const int jhi = dj < 0 ? -1 : (dj >> 4);
      const int ihi = !diag ? 3 : di < 0 ? -1 : (di >> 4);
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const bool on = j <= jhi && i <= ihi && !(diag && wi + 16 * i > wj + 16 * j);
          if (on) {
            acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fb[j].x, fa[i].x, acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fb[j].y, fa[i].y, acc[i][j], 0, 0, 0);
          }
        }
    };
    // (no prefetch: the staging registers would not fit beside the accumulators and two fragment sets, and the second workgroup of
    //  the CU covers the load latency of these 8 K tiles)
    for (int kt = 0; kt < L_DIAG_KT; kt++) {
      {
        d2 ra[4], rb[4];
        load_masked(i0, j0 + (int64_t)kt * LK, ra);
        load_masked(j0, j0 + (int64_t)kt * LK, rb);
        store_mc(sA(0), ra);
        store_mc(sB(0), rb);
      }
      __syncthreads();
      read_frags(sA(0), sB(0), 0, fa0, fb0);
      mma_skip(fa0, fb0, kt * LK);
      read_frags(sA(0), sB(0), 8, fa0, fb0);
      mma_skip(fa0, fb0, kt * LK + 8);
      __syncthreads();
    }
  }

  // ---- the dense K tiles, k in [j0 + 128, n): LDS-DMA, rotated software pipeline (gemm.hip tn_dma_tile) ------------------------------------
  //   prologue : DMA t0 | sync | read F0(t0,h0) | DMA t1 | read F1(t0,h1) | MMA(F0)
  //   loop kt  : sync | DMA A t(kt+2) | read F0(t(kt+1),h0) | MMA(F1) | DMA B t(kt+2) | read F1(t(kt+1),h1) | MMA(F0)
  //   tail     : MMA(F1)
  // The barrier at the top of iteration kt proves: all reads of tile kt are done (its buffer may be refilled) and tile kt + 1 has landed
  // (every wave drains its own DMA share with vmcnt(0) before it).
  const int nd = nk - L_DIAG_KT;
  if (nd > 0) {
    // one wave-instruction moves one k row (1 KiB): wave w moves rows 4 w ... 4 w + 3 of the K tile.  The row's address is wave-uniform,
    // the per-lane part is one of two loop-invariant 32-bit offsets (the half swap of rows with (k >> 1) odd is applied on the SOURCE side).
    const double* rowA = g.W + i0 + (j0 + LT + wid_s * 4) * g.ldw;
    const double* rowB = g.W + j0 + (j0 + LT + wid_s * 4) * g.ldw;
    const uint32_t voff0 = (uint32_t)lane << 4, voff1 = (uint32_t)(lane ^ 8) << 4;
    const int64_t kstep = (int64_t)LK * g.ldw;            // one K tile further (doubles): the row pointers advance by scalar adds
    auto dma = [&](const double* rows, double* dst) {    // rows: the wave's first row of the K tile (wave-uniform)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const char* src = reinterpret_cast<const char*>(rows + q * g.ldw) + ((q & 2) ? voff1 : voff0);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(dst + (wid_s * 4 + q) * LT), 16, 0, 0);
      }
    };
    auto mma32 = [&](const d2 (&fa)[4], const d2 (&fb)[4]) {
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fb[j].x, fa[i].x, acc[i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fb[j].y, fa[i].y, acc[i][j], 0, 0, 0);
    };
    // 32 MFMAs, 4 LDS-DMA pieces and 16 LDS reads per phase: one piece per 8 MFMAs, two reads per 4
    auto interleave = [&]() {
#pragma unroll
      for (int q = 0; q < 8; q++) {
        __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
        if (q & 1) __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
      }
    };
    dma(rowA, sA(0));
    dma(rowB, sB(0));
    __builtin_amdgcn_s_waitcnt(0x0070);                  // vmcnt(0) lgkmcnt(0): my share of tile 0 has landed
    __syncthreads();
    read_frags(sA(0), sB(0), 0, fa0, fb0);
    {
      const int64_t k1 = nd > 1 ? kstep : 0;
      rowA += k1; rowB += k1;                             // tile min(1, nd - 1)
      dma(rowA, sA(1));
      dma(rowB, sB(1));
    }
    read_frags(sA(0), sB(0), 8, fa1, fb1);
    __builtin_amdgcn_sched_barrier(0);
    mma32(fa0, fb0);
    __builtin_amdgcn_sched_barrier(0);
    for (int kt = 0; kt + 1 < nd; kt++) {
      const int nxt = (kt + 1) & 1;
      __builtin_amdgcn_s_waitcnt(0x0070);                // F1 is complete and my share of tile kt + 1 has landed
      __syncthreads();
      const int64_t adv = (kt + 2 < nd) ? kstep : 0;     // tile min(kt + 2, nd - 1): the last refill is redundant but branch-free
      rowA += adv; rowB += adv;
      dma(rowA, sA(nxt ^ 1));
      read_frags(sA(nxt), sB(nxt), 0, fa0, fb0);
      mma32(fa1, fb1);
      interleave();
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_waitcnt(0xc07f);                // lgkmcnt(0): F0 has landed (last read issued >= 4 MFMAs ago)
      dma(rowB, sB(nxt ^ 1));
      read_frags(sA(nxt), sB(nxt), 8, fa1, fb1);
      mma32(fa0, fb0);
      interleave();
      __builtin_amdgcn_sched_barrier(0);
    }
    mma32(fa1, fb1);
  }

  // epilogue: lane holds C[i0 + wi + 16 i + lr][j0 + wj + 16 j + kg + 4 r]; the branch is block-uniform
  auto epilogue = [&](auto masked) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int64_t row = i0 + wi + 16 * i + lr;
#pragma unroll
      for (int j = 0; j < 4; j++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int64_t col = j0 + wj + 16 * j + kg + 4 * r;
          if (!masked.value || row <= col) g.C[row + col * g.ldc] = acc[i][j][r];
        }
    }
  };
  if (diag) epilogue(std::true_type{}); else epilogue(std::false_type{});
}

// X[col][row] = X[row][col] for row < col: 32 x 32 blocks through LDS, 256-byte segments both on the read and on the write
__global__ void __launch_bounds__(256) mirror_upper_kernel(double* X, int64_t ld, int64_t n) {
  __shared__ double tile[32][33];
  const int64_t bi = blockIdx.x, bj = blockIdx.y;
  if (bi > bj) return;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
  for (int s = 0; s < 4; s++) {
    const int c = ty + 8 * s;
    const int64_t row = bi * 32 + tx, col = bj * 32 + c;
    if (row < n && col < n && row < col) tile[c][tx] = X[row + col * ld];
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < 4; s++) {
    const int c = ty + 8 * s;
    const int64_t row = bj * 32 + tx, col = bi * 32 + c;       // element (row, col) of the lower triangle = (col, row) of the upper one
    if (row < n && col < n && col < row) X[row + col * ld] = tile[tx][c];
  }
}

// NaN over the window (tri = 1: its upper triangle) when the factor failed
__global__ void tri_nan_kernel(double* X, int64_t ld, int64_t n, int tri, const int* info) {
  if (*info == 0) return;
  for (int64_t col = blockIdx.y; col < n; col += gridDim.y)
    for (int64_t row = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; row < n; row += (int64_t)gridDim.x * blockDim.x)
      if (!tri || row <= col) X[row + col * ld] = __builtin_nan("");
}

// 2 sum log r_ii: thread t adds the elements t, t + 256, ... in ascending order, the 256 partial sums are folded as a binary tree in LDS -
// a fixed order, so two calls give the same bits
__global__ void __launch_bounds__(256) logdet_kernel(const double* R, int64_t ldr, int64_t n, const int* info, double* out) {
  __shared__ double part[256];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int64_t i = t; i < n; i += 256) s += log(R[i * (ldr + 1)]);
  part[t] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) part[t] += part[t + w];
    __syncthreads();
  }
  if (t == 0) *out = (info && *info != 0) ? __builtin_nan("") : 2.0 * part[0];
}

}  // namespace

// upper triangle of C = W W^T for any n, leading dimensions and alignment; W and C must not overlap.  The kernel takes the aligned leading
// n0 = 128 floor(n / 128) square; with W = [W11 W12; 0 W22] the ragged border of r = n - n0 < 128 rows is composed around it:
//   C11 += W12 W12^T (K = r),  C12 = W12 W22^T,  C22 = W22 W22^T   with W22 copied into a zero-lower r x r scratch
// An odd ldw or a W that is not 16-byte aligned (the DMA moves 16-byte pieces) goes through a zero-lower copy of all of W and the register-staged
// NT product with dense K: correct, three times the flops, no LDS-DMA.
int cap_lauum_launch(int64_t n, const double* W, int64_t ldw, double* C, int64_t ldc, hipStream_t stream) {
  if (n < 0) return CAP_ERR_ARG;
  if (n == 0) return CAP_OK;
  if (!W || !C || ldw < n || ldc < n) return CAP_ERR_ARG;
  if ((ldw & 1) || (((uintptr_t)W) & 15)) {
    // (the product below never splits K - an upper product with fewer than 128 tiles has K = n < 4096 - so it does not ask for this scratch itself)
    const int64_t lds_ = cap_round_up(n, 2);
    double* Wc = cap_scratch(lds_ * n, stream);
    if (!Wc) return CAP_ERR_ALLOC;
    CAP_TRY(cap_copy_window(W, 0, ldw, 0, 0, Wc, 0, lds_, 0, 0, n, n, 1, 1, (void*)stream));
    return cap_gemm_launch(CAP_NOTRANS, CAP_TRANS, n, n, n, 1.0, Wc, lds_, Wc, lds_, 0.0, C, ldc, 1, stream, CAP_TAG_NO_ATOMIC);
  }
  const int64_t n0 = (n / LT) * LT, r = n - n0;
  if (n0 > 0) {
    const int64_t grid = lauum_grid(n0 / LT);
    if (grid > 0x7fffffff) return CAP_ERR_UNSUPPORTED;
    LauumArgs g{W, C, ldw, ldc, (int)(n0 / LT)};
    cap_acc_r(W, ldw, n0, n0, 1);
    cap_acc_w(C, ldc, n0, n0, 1);
    hipLaunchKernelGGL(dlauum_nt_kernel, dim3((unsigned)grid), dim3(LTHREADS), 4 * L_TILE * sizeof(double), stream, g);
    CAP_HIP(hipGetLastError());
  }
  if (r == 0) return CAP_OK;
  const int64_t ldr_ = cap_round_up(r, 2);
  double* W22 = cap_scratch(ldr_ * r, stream);
  if (!W22) return CAP_ERR_ALLOC;
  const double* W12 = W + n0 * ldw;
  CAP_TRY(cap_copy_window(W, 0, ldw, n0, n0, W22, 0, ldr_, 0, 0, r, r, 1, 1, (void*)stream));
  if (n0 > 0) {
    CAP_TRY(cap_gemm_launch(CAP_NOTRANS, CAP_TRANS, n0, n0, r, 1.0, W12, ldw, W12, ldw, 1.0, C, ldc, 1, stream, CAP_TAG_NO_ATOMIC));
    CAP_TRY(cap_gemm_launch(CAP_NOTRANS, CAP_TRANS, n0, r, r, 1.0, W12, ldw, W22, ldr_, 0.0, C + n0 * ldc, ldc, 0, stream, CAP_TAG_NO_ATOMIC));
  }
  return cap_gemm_launch(CAP_NOTRANS, CAP_TRANS, r, r, r, 1.0, W22, ldr_, W22, ldr_, 0.0, C + n0 + n0 * ldc, ldc, 1, stream, CAP_TAG_NO_ATOMIC);
}

int cap_mirror_upper(double* X, int64_t ld, int64_t n, hipStream_t stream) {
  if (n <= 1) return CAP_OK;
  const int64_t nb = cap_ceil_div(n, 32);
  if (nb > 65535) return CAP_ERR_UNSUPPORTED;
  cap_acc_r(X, ld, n, n, 1);
  cap_acc_w(X, ld, n, n, 2);          // (the diagonal is in both notes and is not written: the same launch, no conflict)
  hipLaunchKernelGGL(mirror_upper_kernel, dim3((unsigned)nb, (unsigned)nb), dim3(256), 0, stream, X, ld, n);
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}

int cap_tri_nan_fill(double* X, int64_t ld, int64_t n, int tri, const int* info, hipStream_t stream) {
  if (!info || n <= 0) return CAP_OK;
  if (cap_acc_on()) { cap_acc_w(X, ld, n, n, tri ? 1 : 0); cap_acc_r(info, 1, 1, 1, 0, 4); }
  hipLaunchKernelGGL(tri_nan_kernel, dim3((unsigned)std::min<int64_t>(cap_ceil_div(n, 256), 64), (unsigned)std::min<int64_t>(n, 65535)), dim3(256), 0, stream, X, ld, n, tri, info);
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}

int cap_logdet_launch(const double* R, int64_t ldr, int64_t n, const int* info, double* out, hipStream_t stream) {
  if (cap_acc_on()) {
    cap_acc_r(R, ldr + 1, 1, n);      // the diagonal: n windows of one element, ldr + 1 apart
    if (info) cap_acc_r(info, 1, 1, 1, 0, 4);
    cap_acc_w(out, 1, 1, 1);
  }
  hipLaunchKernelGGL(logdet_kernel, dim3(1), dim3(256), 0, stream, R, ldr, n, info, out);
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}

extern "C" int cap_dlauum(int uplo, int64_t n, const double* W, int64_t ldw, double* C, int64_t ldc, void* stream) {
  if (n < 0 || (n > 0 && (!W || !C || ldw < n || ldc < n))) return CAP_ERR_ARG;
  if (n > 0) {                         // the windows' address ranges must be disjoint
    const uintptr_t w0 = (uintptr_t)W, w1 = w0 + sizeof(double) * (uintptr_t)((n - 1) * ldw + n);
    const uintptr_t c0 = (uintptr_t)C, c1 = c0 + sizeof(double) * (uintptr_t)((n - 1) * ldc + n);
    if (w0 < c1 && c0 < w1) return CAP_ERR_ARG;
  }
  if (uplo != CAP_UPPER) return CAP_ERR_UNSUPPORTED;
  if (n == 0) return CAP_OK;
  return cap_lauum_launch(n, W, ldw, C, ldc, cap_stream(stream));
}
