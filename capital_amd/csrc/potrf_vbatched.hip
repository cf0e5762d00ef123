// Variable-size batched Cholesky factor, solve and SPD inverse (cap_vbatch_plan_*, cap_dpotrf_vbatched, cap_dpotrs_vbatched,
// cap_dpotri_vbatched): a batch of column-major blocks of DIFFERENT sizes 0 <= n_i <= 256, block i at A + offset[i] with leading dimension
// ld[i], the right-hand sides stacked: block i owns rows row_off[i] .. row_off[i] + n_i of B, row_off the prefix sum of n in batch order.
//
// THE PLAN sorts the batch once, on the host, into the seven size classes of the fixed-size kernels - a wavefront per 64 / NP blocks for
// NP = 8, 16, 32, 64 (the smallest one >= n_i), a workgroup per block for NBLK = ceil(n_i / 64) = 2, 3, 4 - and keeps, on the device, one record
// per block (offset, leading dimension, row offset, n) and per class the list of its block indices, stably sorted by n_i: the blocks that share
// a wave have neighbouring sizes.  A call is ONE launch per non-empty class on the caller's stream (seven at most) and nothing else: no
// scratch, no allocation, no memset, no atomics, no helper stream, no host synchronisation; nothing between workgroups.
//
// THE ARITHMETIC is that of the fixed-size entries, from the shared headers batched_small.h / batched_blocked.h / batched_inverse.h: every block gets, bit
// for bit, what the fixed-size entry writes for it with n = n_i and batch = 1 - info and logdet included - whichever blocks share its wave, its
// class list or the batch.
//   n_i > 64: the workgroup looks its block up (blockIdx.x -> class list -> record) and runs the fixed-size kernel's body on it; n is uniform
//     over the workgroup as it always was.
//   n_i <= 64: the lane groups of one wave now have different sizes.  Whatever stands in front of a __syncthreads or a lane shuffle - the
//     factor's steps, the product's rows, the loops of the coalesced load and store - branches on nmax, the largest n of the wave (uniform);
//     a group with n < nmax computes on padding there.  Padding is zeros in registers (columns c >= n of a group) and never-read words of the
//     group's own LDS image; it cannot reach a real element: step J of the factor changes a_ic for i > J only, so the steps J >= n change rows
//     at or beyond n alone, and the steps J < n read d = a_JJ from lane J < n and row J of the image at columns < n - real data.  Everything
//     with an effect outside the registers is a lane predicate on the group's own n: the loads (c <= cc < n: never outside the block's own
//     upper triangle), the stores, the first-bad-pivot decision (steps J < n only), the logarithms and their sum.  Where no lane talks to
//     another one - the two substitutions and the inverse's sweep - the group's own n is simply the `n` of the fixed-size step: the branch
//     becomes a lane mask and every lane executes exactly the fixed-size sequence for its own block.  The product's row sums take the
//     group's own n for their chunks (a padded chunk would add +0 products, which is not the identity on a sum that underflowed to -0).
//     A wave's dead groups (the tail of a class) have n = 0: every predicate is false for them.
// SHARED (vbatch_plan.h): the plan's layout, the walk over its classes (vb_for_each_class), a lane group's lookup of its block (vb_group,
// vb_load_upper) and the dispatch of a runtime class to a kernel instance (vb_with_int) - what trsm_batched.hip, cholupdate_batched.hip and
// syrk_batched.hip run on too.
#include <algorithm>
#include <new>
#include <vector>

#include "batched_small.h"
#include "batched_blocked.h"
#include "batched_inverse.h"
#include "capital_amd.h"
#include "vbatch_plan.h"   // the plan, its walk and the lane group's block lookup (vb_group, vb_load_upper)

namespace {

constexpr int VB_MAX = 256;

struct VbArgs {                        // one class of one call
  const VbRec* rec;
  const int64_t* list; int64_t count;  // the block indices of the class, sorted by n
  double* A;
  int* info; double* logdet;           // batch order
  double* B; int64_t ldb, nrhs;
  int fill;
};

// pb_factor_step with the wave's nmax in the uniform branches and the group's n in the pivot decision
template <int NP>
__device__ __forceinline__ void vb_factor_step(double (&a)[NP], double* s, int c, int nmax, int n, const int J, int& info, bool& bad) {
  using Img = PbImg<NP>;
  if (J >= nmax) return;
  const double d = __shfl(a[J], J, NP);
  const bool fail = !(d > 0.0) && J < n;   // a NaN fails too; the pivots of the padding do not count
  if (fail && !bad) info = J + 1;
  bad = bad || fail;
  const double sq = __dsqrt_rn(d);
  double r = c == J ? sq : a[J] / sq;
  r = bad ? (double)NAN : r;
  if (c >= J) s[Img::at(J, c)] = r;
  __syncthreads();
#pragma unroll
  for (int i0 = ((J + 1) / PB_CH) * PB_CH; i0 < NP; i0 += PB_CH) {
    if (i0 < nmax) {
#pragma unroll
      for (int i = (i0 > J + 1 ? i0 : J + 1); i < i0 + PB_CH; i++) a[i] = fma(-s[Img::at(J, i)], r, a[i]);
    }
  }
}
template <int NP, int... J>
__device__ __forceinline__ void vb_factor_steps(double (&a)[NP], double* s, int c, int nmax, int n, int& info, bool& bad, std::integer_sequence<int, J...>) {
  (vb_factor_step<NP>(a, s, c, nmax, n, J, info, bad), ...);
}

// the two substitutions: the fixed-size steps with the group's own n (no lane talks to another one), skipped as a wave beyond nmax
template <int NP, int... J>
__device__ __forceinline__ void vb_solve_steps(double (&x)[NP], const double* s, int nmax, int n, std::integer_sequence<int, J...>) {
  ((J < nmax ? pb_forward_step<NP>(x, s, n, J) : (void)0), ...);
  ((NP - 1 - J < nmax ? pb_backward_step<NP>(x, s, n, NP - 1 - J) : (void)0), ...);
}

// pi_product_row with the wave's nmax in front of the barrier and the group's n in the chunks of the sum
template <int NP>
__device__ __forceinline__ void vb_product_row(const double (&w)[NP], double* s, int j, int nmax, int n, const int I) {
  using Img = PiImg<NP>;
  if (I >= nmax) return;
  double acc = 0.0;
#pragma unroll
  for (int k0 = (I / PI_CH) * PI_CH; k0 < NP; k0 += PI_CH) {
    if (k0 < n) {
#pragma unroll
      for (int k = (k0 > I ? k0 : I); k < k0 + PI_CH; k++) acc = fma(s[Img::at(I, k)], w[k], acc);
    }
  }
  __syncthreads();                       // (one wave: orders the reads of row I in front of its stores)
  if (j >= I) s[Img::at(I, j)] = acc;
}
template <int NP, int... I>
__device__ __forceinline__ void vb_product_rows(const double (&w)[NP], double* s, int j, int nmax, int n, std::integer_sequence<int, I...>) {
  (vb_product_row<NP>(w, s, j, nmax, n, I), ...);
}

// ------------------------------------------------------------------------------------------------ n <= 64: a wavefront per 64 / NP blocks
template <int NP>
__global__ __launch_bounds__(64) void potrf_vbatched_kernel(VbArgs g) {
  constexpr int G = 64 / NP;
  using Img = PbImg<NP>;
  __shared__ double s_img[G * Img::SIZE];
  __shared__ double s_log[64];
  const int lane = threadIdx.x, grp = lane / NP, c = lane % NP;
  const VbGroup v = vb_group<NP>(g.rec, g.list, g.count);
  const int n = v.n, nmax = v.nmax;
  double* A = g.A + v.off;
  double* s = s_img + grp * Img::SIZE;

  vb_load_upper<Img>(A, v.ld, n, nmax, c, s);
  __syncthreads();
  double a[NP];
#pragma unroll
  for (int i = 0; i < NP; i++) {
    const double t = s[Img::at(i, c)];
    a[i] = (i <= c && c < n) ? t : 0.0;
  }
  __syncthreads();                       // the image is in registers: from here on it takes the rows of R

  int info = 0;
  bool bad = false;
  if constexpr (NP < 64) {
#pragma unroll
    for (int j = 0; j < NP; j++) vb_factor_step<NP>(a, s, c, nmax, n, j, info, bad);
  } else {
    vb_factor_steps<NP>(a, s, c, nmax, n, info, bad, std::make_integer_sequence<int, NP>{});
  }
  __syncthreads();

#pragma unroll 8
  for (int cc = 0; cc < nmax; cc++)
    if (c <= cc && cc < n) A[c + (int64_t)cc * v.ld] = s[Img::at(c, cc)];
  if (g.info && n > 0 && c == 0) g.info[v.blk] = info;
  if (g.logdet) {                        // 2 sum_j log r_jj in ascending j, as potrf_batched_kernel
    s_log[lane] = c < n ? log(s[Img::at(c, c)]) : 0.0;
    __syncthreads();
    if (n > 0 && c == 0) {
      double t = 0.0;
      for (int j = 0; j < n; j++) t += s_log[grp * NP + j];
      g.logdet[v.blk] = bad ? (double)NAN : 2.0 * t;
    }
  }
}

template <int NP>
__global__ __launch_bounds__(64) void potrs_vbatched_kernel(VbArgs g) {
  constexpr int G = 64 / NP;
  using Img = PbImg<NP>;
  __shared__ double s_img[G * Img::SIZE];
  const int lane = threadIdx.x, grp = lane / NP, k = lane % NP;
  const VbGroup v = vb_group<NP>(g.rec, g.list, g.count);
  const int n = v.n, nmax = v.nmax;
  const double* s = s_img + grp * Img::SIZE;

  vb_load_upper<Img>(g.A + v.off, v.ld, n, nmax, k, s_img + grp * Img::SIZE);
  const bool bad = g.info && n > 0 && g.info[v.blk] != 0;
  __syncthreads();

  for (int64_t k0 = 0; k0 < g.nrhs; k0 += NP) {
    const bool on = n > 0 && k0 + k < g.nrhs;
    double* b = g.B + (on ? v.row + (k0 + k) * g.ldb : 0);
    double x[NP];
#pragma unroll
    for (int i = 0; i < NP; i++) {
      x[i] = 0.0;
      if (i < nmax) { if (on && i < n) x[i] = b[i]; }
    }
    if constexpr (NP < 64) {
#pragma unroll
      for (int j = 0; j < NP; j++)
        if (j < nmax) pb_forward_step<NP>(x, s, n, j);
#pragma unroll
      for (int j = NP - 1; j >= 0; j--)
        if (j < nmax) pb_backward_step<NP>(x, s, n, j);
    } else {
      vb_solve_steps<NP>(x, s, nmax, n, std::make_integer_sequence<int, NP>{});
    }
#pragma unroll
    for (int i = 0; i < NP; i++) {
      if (i < nmax) { if (on && i < n) b[i] = bad ? (double)NAN : x[i]; }
    }
  }
}

template <int NP>
__global__ __launch_bounds__(64) void potri_vbatched_kernel(VbArgs g) {
  constexpr int G = 64 / NP;
  using Img = PiImg<NP>;
  __shared__ double s_img[G * Img::SIZE];
  const int lane = threadIdx.x, grp = lane / NP, c = lane % NP;
  const VbGroup v = vb_group<NP>(g.rec, g.list, g.count);
  const int n = v.n, nmax = v.nmax;
  const int64_t ld = v.ld;
  double* A = g.A + v.off;
  double* s = s_img + grp * Img::SIZE;
  const bool bad = g.info && n > 0 && g.info[v.blk] != 0;

#pragma unroll 8
  for (int cc = 0; cc < nmax; cc++)
    if (c <= cc && cc < n) s[Img::at(c, cc)] = A[c + (int64_t)cc * ld];
  __syncthreads();

  {
    double x[NP];
    pi_invert<NP>(x, s, c, n);           // the group's own n: a lane mask, the fixed-size sequence per block
    __syncthreads();                     // every lane is through with R: the image takes W
    pi_put_column<NP>(x, s, c, n);
  }
  __syncthreads();

  double w[NP];
#pragma unroll
  for (int k = 0; k < NP; k++) {
    const double t = s[Img::at(c < k ? c : k, k)];
    w[k] = k >= c ? t : 0.0;
  }
  __syncthreads();
  if constexpr (NP < 64) {
#pragma unroll
    for (int i = 0; i < NP; i++) vb_product_row<NP>(w, s, c, nmax, n, i);
  } else {
    vb_product_rows<NP>(w, s, c, nmax, n, std::make_integer_sequence<int, NP>{});
  }
  __syncthreads();

  const bool fill = g.fill;
#pragma unroll 8
  for (int cc = 0; cc < nmax; cc++) {
    if (c <= cc && cc < n) {
      const double t = bad ? (double)NAN : s[Img::at(c, cc)];
      A[c + (int64_t)cc * ld] = t;
      if (fill && c < cc) A[cc + (int64_t)c * ld] = t;
    }
  }
}

// ------------------------------------------------------------------------------------------------ 64 < n <= 256: a workgroup per block
template <int NBLK>
__global__ __launch_bounds__(64 * bb_factor_waves(NBLK)) void potrf_vbatched_blocked_kernel(VbArgs g) {
  const int64_t blk = g.list[blockIdx.x];
  const VbRec r = g.rec[blk];
  bb_factor_block<NBLK>(g.A + r.off, r.ld, (int)r.n, g.info, g.logdet, blk);
}

__global__ __launch_bounds__(BB_THREADS) void potrs_vbatched_blocked_kernel(VbArgs g) {
  const int64_t blk = g.list[blockIdx.x];
  const VbRec r = g.rec[blk];
  bb_solve_block(g.A + r.off, r.ld, g.B + r.row, g.ldb, g.nrhs, (int)r.n, g.info, blk);
}

template <int NBLK>
__global__ __launch_bounds__(64 * pi_waves(NBLK)) void potri_vbatched_blocked_kernel(VbArgs g) {
  const int64_t blk = g.list[blockIdx.x];
  const VbRec r = g.rec[blk];
  pi_blocked_block<NBLK>(g.A + r.off, r.ld, (int)r.n, g.info, blk, 1, g.fill);
}

enum { VB_FACTOR, VB_SOLVE, VB_INVERSE };

void vb_launch(int op, int cls, dim3 grid, hipStream_t s, const VbArgs& g) {
  const int np = 8 << cls, nblk = cls - 2;       // the template argument of the class: NP up to class 3, NBLK above
  if (op == VB_FACTOR) {
    if (cls < 4) vb_with_int<8, 16, 32, 64>(np, [&](auto NP) { hipLaunchKernelGGL(potrf_vbatched_kernel<NP()>, grid, dim3(64), 0, s, g); });
    else vb_with_int<2, 3, 4>(nblk, [&](auto NB) { hipLaunchKernelGGL(potrf_vbatched_blocked_kernel<NB()>, grid, dim3(64 * bb_factor_waves(NB())), 0, s, g); });
  } else if (op == VB_SOLVE) {
    if (cls < 4) vb_with_int<8, 16, 32, 64>(np, [&](auto NP) { hipLaunchKernelGGL(potrs_vbatched_kernel<NP()>, grid, dim3(64), 0, s, g); });
    else hipLaunchKernelGGL(potrs_vbatched_blocked_kernel, grid, dim3(BB_THREADS), 0, s, g);
  } else {
    if (cls < 4) vb_with_int<8, 16, 32, 64>(np, [&](auto NP) { hipLaunchKernelGGL(potri_vbatched_kernel<NP()>, grid, dim3(64), 0, s, g); });
    else vb_with_int<2, 3, 4>(nblk, [&](auto NB) { hipLaunchKernelGGL(potri_vbatched_blocked_kernel<NB()>, grid, dim3(64 * pi_waves(NB())), 0, s, g); });
  }
}

// the launches of one call: one per non-empty class, in class order
int vb_run(int op, const cap_vbatch_plan* p, VbArgs g, hipStream_t s) {
  if (p->nonempty == 0) return CAP_OK;
  if (p->device < 0) return CAP_ERR_HIP;
  g.rec = p->d_rec;
  return vb_for_each_class(p, [&](int cls, const int64_t* list, int64_t count, const std::vector<int64_t>& blocks, dim3 grid) {
    g.list = list;
    g.count = count;
    if (cap_acc_on()) {
      for (int64_t b : blocks) {
        const VbRec& r = p->rec[b];
        if (op == VB_FACTOR) {
          cap_acc_rw(g.A + r.off, r.ld, r.n, r.n, 1);
          if (g.info) cap_acc_w(g.info + b, 0, 1, 1, 0, 4);
          if (g.logdet) cap_acc_w(g.logdet + b, 0, 1, 1);
        } else if (op == VB_SOLVE) {
          cap_acc_r(g.A + r.off, r.ld, r.n, r.n, 1);
          cap_acc_rw(g.B + r.row, g.ldb, r.n, g.nrhs);
          if (g.info) cap_acc_r(g.info + b, 0, 1, 1, 0, 4);
        } else {
          cap_acc_rw(g.A + r.off, r.ld, r.n, r.n, g.fill ? 0 : 1);
          if (g.info) cap_acc_r(g.info + b, 0, 1, 1, 0, 4);
        }
      }
    }
    vb_launch(op, cls, grid, s, g);
  });
}

}  // namespace

extern "C" {

int cap_vbatch_plan_create(int64_t batch, const int64_t* n, const int64_t* ld, const int64_t* offset, cap_vbatch_plan** out) {
  if (!out) return CAP_ERR_ARG;
  *out = nullptr;
  if (batch < 0 || (batch > 0 && !n)) return CAP_ERR_ARG;
  cap_vbatch_plan* p = new (std::nothrow) cap_vbatch_plan;
  if (!p) return CAP_ERR_ALLOC;
  p->batch = batch;
  p->rec.resize((size_t)batch);
  int64_t packed = 0, row = 0;
  bool too_large = false;
  std::vector<std::pair<int64_t, int64_t>> win;      // (first element, one past the last) of every non-empty block
  for (int64_t i = 0; i < batch; i++) {
    VbRec& r = p->rec[(size_t)i];
    r.n = n[i];
    r.ld = ld ? ld[i] : (n[i] > 1 ? n[i] : 1);
    r.off = offset ? offset[i] : packed;
    r.row = row;
    if (r.n < 0 || r.ld < r.n || r.off < 0) { delete p; return CAP_ERR_ARG; }
    packed = vb_clip((__int128)packed + (__int128)r.ld * r.n);
    row = vb_clip((__int128)row + r.n);
    if (r.n == 0) continue;
    too_large = too_large || r.n > VB_MAX;
    const int64_t end = vb_clip((__int128)r.off + (__int128)(r.n - 1) * r.ld + r.n);      // (sizes that are refused below may be huge)
    win.emplace_back(r.off, end);
    p->total = std::max(p->total, end);
    p->nmax = std::max(p->nmax, r.n);
  }
  p->rows = row;
  std::sort(win.begin(), win.end());
  for (size_t k = 1; k < win.size(); k++)
    if (win[k].first < win[k - 1].second) { delete p; return CAP_ERR_ARG; }       // two blocks' windows meet
  if (too_large) { delete p; return CAP_ERR_UNSUPPORTED; }
  for (int64_t i = 0; i < batch; i++)
    if (p->rec[(size_t)i].n > 0) p->list[vb_class(p->rec[(size_t)i].n)].push_back(i);
  int64_t at = 0;
  for (int cls = 0; cls < VB_CLASSES; cls++) {
    std::vector<int64_t>& l = p->list[cls];
    std::stable_sort(l.begin(), l.end(), [&](int64_t a, int64_t b) { return p->rec[(size_t)a].n < p->rec[(size_t)b].n; });
    if (vb_grid((int64_t)l.size(), vb_per_group(cls)) < 0) { delete p; return CAP_ERR_UNSUPPORTED; }   // one 1-D grid per class
    p->list_at[cls] = at;
    at += (int64_t)l.size();
    p->nonempty += l.empty() ? 0 : 1;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); *out = p; return CAP_OK; }
  if (hipGetDevice(&p->device) != hipSuccess) { (void)hipGetLastError(); delete p; return CAP_ERR_HIP; }
  if (at > 0) {
    std::vector<int64_t> all;
    all.reserve((size_t)at);
    for (int cls = 0; cls < VB_CLASSES; cls++) all.insert(all.end(), p->list[cls].begin(), p->list[cls].end());
    if (hipMalloc((void**)&p->d_rec, sizeof(VbRec) * (size_t)batch) != hipSuccess ||
        hipMalloc((void**)&p->d_list, sizeof(int64_t) * (size_t)at) != hipSuccess ||
        hipMemcpy(p->d_rec, p->rec.data(), sizeof(VbRec) * (size_t)batch, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(p->d_list, all.data(), sizeof(int64_t) * (size_t)at, hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipGetLastError();
      cap_vbatch_plan_destroy(p);
      return CAP_ERR_ALLOC;
    }
  }
  *out = p;
  return CAP_OK;
}

int cap_vbatch_plan_destroy(cap_vbatch_plan* p) {
  if (!p) return CAP_OK;
  if (p->d_rec) (void)hipFree(p->d_rec);
  if (p->d_list) (void)hipFree(p->d_list);
  delete p;
  return CAP_OK;
}

int64_t cap_vbatch_plan_info(const cap_vbatch_plan* p, int what) {
  if (!p) return -1;
  switch (what) {
    case CAP_VBATCH_BATCH: return p->batch;
    case CAP_VBATCH_TOTAL: return p->total;
    case CAP_VBATCH_ROWS: return p->rows;
    case CAP_VBATCH_NMAX: return p->nmax;
    case CAP_VBATCH_LAUNCHES: return p->nonempty;
    default:
      if (what >= CAP_VBATCH_COUNT && what < CAP_VBATCH_COUNT + VB_CLASSES) return (int64_t)p->list[what - CAP_VBATCH_COUNT].size();
      return -1;
  }
}

int cap_vbatch_plan_table(const cap_vbatch_plan* p, int cls, int64_t* blocks, int64_t cap) {
  if (!p || cls < 0 || cls >= VB_CLASSES || cap < 0 || (cap > 0 && !blocks)) return CAP_ERR_ARG;
  const std::vector<int64_t>& l = p->list[cls];
  const int64_t m = std::min(cap, (int64_t)l.size());
  for (int64_t k = 0; k < m; k++) blocks[k] = l[(size_t)k];
  return CAP_OK;
}

int cap_dpotrf_vbatched(const cap_vbatch_plan* p, int uplo, double* A, int* info, double* logdet, void* stream) {
  if (!p) return CAP_ERR_ARG;
  if (p->nonempty > 0 && !A) return CAP_ERR_ARG;
  if (uplo != CAP_UPPER) return CAP_ERR_UNSUPPORTED;    // as cap_dpotrf_batched
  VbArgs g = {};
  g.A = A; g.info = info; g.logdet = logdet;
  return vb_run(VB_FACTOR, p, g, cap_stream(stream));
}

int cap_dpotrs_vbatched(const cap_vbatch_plan* p, int uplo, int64_t nrhs, const double* R, double* B, int64_t ldb, const int* info,
                        void* stream) {
  if (!p || nrhs < 0) return CAP_ERR_ARG;
  if (p->nonempty > 0 && nrhs > 0 && (!R || !B)) return CAP_ERR_ARG;
  if (ldb < p->rows) return CAP_ERR_ARG;
  if (uplo != CAP_UPPER) return CAP_ERR_UNSUPPORTED;
  if (nrhs == 0) return CAP_OK;
  VbArgs g = {};
  g.A = const_cast<double*>(R); g.B = B; g.ldb = ldb; g.nrhs = nrhs; g.info = const_cast<int*>(info);
  return vb_run(VB_SOLVE, p, g, cap_stream(stream));
}

int cap_dpotri_vbatched(const cap_vbatch_plan* p, int uplo, double* R, const int* info, int fill, void* stream) {
  if (!p) return CAP_ERR_ARG;
  if (p->nonempty > 0 && !R) return CAP_ERR_ARG;
  if (fill != 0 && fill != 1) return CAP_ERR_ARG;
  if (uplo != CAP_UPPER) return CAP_ERR_UNSUPPORTED;
  VbArgs g = {};
  g.A = R; g.info = const_cast<int*>(info); g.fill = fill;
  return vb_run(VB_INVERSE, p, g, cap_stream(stream));
}

}  // extern "C"
