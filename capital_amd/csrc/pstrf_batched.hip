// Batched pivoted Cholesky factorization for many small symmetric positive SEMIdefinite blocks (cap_dpstrf_batched, cap_dpstrf_vbatched):
// A_i[piv][:, piv] ~ R_i^T R_i with a rank cap and a stopping tolerance, 1 <= n <= 64, the rules of cap_dpstrf (csrc/pstrf.hip) in the
// layout of the batched factor (csrc/potrf_batched.hip).
//
// ONE WAVEFRONT PER GROUP OF BLOCKS, nothing between wavefronts: a workgroup is a single wave of 64 lanes, the grid is 1-D, there is no
// scratch, no atomic, no spin wait and no read of another workgroup's data.  The kernels are templated on the padded size NP = 8 / 16 /
// 32 / 64 (the smallest one >= n); a wave carries G = 64 / NP blocks in lane groups of NP lanes.
//
// STATE.  Lane c of a group owns column c of its block for the whole call: d_c, the remaining diagonal; sel_c, the step at which the
// column was chosen (-1: not yet); w[0 .. NP), its column of the factor W in natural column order, in registers - every register index is
// a compile-time constant, the steps are fully unrolled.  The upper triangle of A goes once to the packed LDS image of the factor
// kernel (PbImg<NP>); A(p, c) is image element (min(p, c), max(p, c)), the strictly lower triangle of A is never addressed and A is never
// written.  Row j of W also goes to an LDS copy (leading dimension NP + 1) as soon as step j has formed it: it is where the other lanes
// find w_i[p] (every lane of a group reads the same address: an LDS broadcast) and where the column-wise stores of R read from.
//
// STEP j of a block, the decision first (ps_better / ps_decide of pstrf.hip): the (d, index, saw-NaN) of the unselected lanes c < n are
// reduced over the group by a butterfly - the larger d wins, ties go to the lowest index; the rule is a total order, so every lane ends
// with the same record whatever the order of the exchanges.  A NaN among the unselected d: stop, info 2.  No candidate or !(d_p > tol_used):
// stop, info 0.  j == max_rank: stop, info 1.  In front of step 0, tol_used = tol < 0 ? n 2^-53 max_i a_ii : tol, per block.  Otherwise
//   for each unselected c != p:  t = A(p, c);  t = fma(-w_i[p], w_i[c], t) for i = 0 .. j - 1 ascending;  r = t / sqrt(d_p);
//                                w_j[c] = r;  d_c = fma(-r, r, d_c)
//   w_j[p] = sqrt(d_p),  w_j[c] = +0.0 for the columns chosen earlier,  sel_p = j
// with a correctly rounded square root and division.  THE BIT CONTRACT rests on this recurrence: a block's bits are a function of
// (n, max_rank, tol, its data) alone - every block sees the same instruction sequence on its own data, there is one load path whatever
// the alignment, and no lane reads anything of another group.
//
// STOPPING.  The blocks of one wave stop at different steps: a stopped group is a lane predicate (it keeps its rank and info and computes
// nothing more); the reductions run with all lanes, outside every divergent branch.  The wave itself leaves the step sequence only through
// wave-uniform branches: a step is skipped as a whole once no group of the wave is active any more.
//
// RESULTS per block: rank = the steps done; piv = the chosen pivots in order, then the unselected indices in increasing order (the place
// of an unselected column is rank + the number of unselected lanes below it: a ballot and a popcount); R[:, k] = W[:, piv[k]] with rows
// rank .. max_rank - 1 equal to +0.0, stored along columns from the LDS copy; resid: s = 0, s += d_c over the unselected c ascending;
// logdet (optional) = 2 sum_{j < rank} log r_jj added in ascending j as the batched factor does, NaN for info 2; info.  The whole
// max_rank x n rectangle of every R block is written, zeros included; rows >= max_rank, padding and gaps are not touched.
//
// THE PLAN ENTRY runs the same body with the group's own (n_i, min(max_rank, n_i)) from the plan's records: the loops of the coalesced
// load and stores run to the largest n of the wave (uniform), everything with an effect is a lane predicate on the group's own n.  R is
// the flat tensor of the plan's layout and gets every entry of every n_i x n_i block.
#include <math.h>

#include <utility>

#include "common.h"
#include "batched_small.h"     // the packed image of an upper triangle (PbImg)
#include "capital_amd.h"
#include "vbatch_plan.h"       // padded size, grid limit, dispatch, operand rule; the plan, its walk and a lane group's block lookup

namespace {

constexpr double PV_EPS = 0x1p-53;     // LAPACK's dlamch('Epsilon'): the default tolerance is n eps max_i a_ii

struct PvArgs {
  const double* A; double* R;
  int64_t* piv; int* rank; double* resid; double* logdet; int* info;
  double tol; int max_rank;
  int64_t lda, stride_a, ldr, stride_r, batch; int n;     // fixed size
  const VbRec* rec; const int64_t* list; int64_t count;   // one class of a plan
};

struct PvBlock {                       // what a lane group works on (n = 0: nothing)
  const double* A; int64_t lda;
  double* R; int64_t ldr;
  int64_t* piv;                        // the block's n entries
  int64_t out;                         // its index in rank / resid / logdet / info
  int n, cap, rrows;                   // rows, the most steps, the rows of R that are written
};

template <int NP>
struct PvLds {
  static constexpr int G = 64 / NP;
  static constexpr int LDW = NP + 1;   // odd: the column-wise reads of the store do not meet in one bank
  static constexpr int W = NP * LDW;
};

// the better of two records: larger value, then lower index; a record without a column loses (ps_better of pstrf.hip)
__device__ __forceinline__ void pv_better(double& v, int& i, double ov, int oi) {
  if (oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i))) { v = ov; i = oi; }
}

// the decision in front of step J for every group of the wave (all lanes take part in the exchanges): an active group either stops
// (active = false, rank = J, info) or goes on with pivot p of remaining diagonal dp
template <int NP>
__device__ __forceinline__ void pv_decide(const int J, int c, int n, int cap, double tol, double d, int sel, bool& active, int& rank, int& info,
                                          double& tol_used, double& dp, int& p) {
  const bool un = active && c < n && sel < 0;
  int nan = (un && d != d) ? 1 : 0;
  double v = (un && !nan) ? d : -INFINITY;
  int idx = (un && !nan) ? c : -1;
#pragma unroll
  for (int off = NP / 2; off >= 1; off >>= 1) {
    const double ov = __shfl_xor(v, off);
    const int oi = __shfl_xor(idx, off);
    nan |= __shfl_xor(nan, off);
    pv_better(v, idx, ov, oi);
  }
  if (J == 0) tol_used = tol < 0 ? (double)n * PV_EPS * v : tol;
  const int stop = nan ? 3 : (idx < 0 || !(v > tol_used)) ? 1 : (J == cap ? 2 : 0);
  if (active && stop) { active = false; rank = J; info = stop - 1; }
  dp = v; p = idx;
}

// step J of the active groups (J is a compile-time constant at every call once the callers are expanded: every index of w[] is static)
template <int NP>
__device__ __forceinline__ void pv_step(double (&w)[NP], const double* img, double* W, const int J, int c, int n, bool active, double dp, int p,
                                        double& d, int& sel, double& rdiag) {
  using Img = PbImg<NP>;
  constexpr int LDW = PvLds<NP>::LDW;
  if (active) {
    double r = 0.0;
    if (c < n && sel < 0) {
      const double sq = __dsqrt_rn(dp);
      if (c == p) { r = sq; sel = J; rdiag = sq; }
      else {
        double t = img[Img::at(c < p ? c : p, c < p ? p : c)];
#pragma unroll
        for (int i = 0; i < J; i++) t = fma(-W[i * LDW + p], w[i], t);
        r = t / sq;
        d = fma(-r, r, d);
      }
    }
    w[J] = r;
    W[J * LDW + c] = r;
  }
  __syncthreads();                       // (one wave: row J of the LDS copy is in place for the steps behind it)
}

template <int NP>
struct PvState {
  double w[NP];
  double d, rdiag, tol_used;
  int sel, rank, info;
  bool active;
};

// decision and step J; the step is skipped as a whole (a wave-uniform branch) once no group of the wave goes on
template <int NP>
__device__ __forceinline__ void pv_decide_step(PvState<NP>& st, const double* img, double* W, const int J, int c, int n, int cap, double tol) {
  if (!__any(st.active)) return;
  double dp; int p;
  pv_decide<NP>(J, c, n, cap, tol, st.d, st.sel, st.active, st.rank, st.info, st.tol_used, dp, p);
  if (!__any(st.active)) return;
  pv_step<NP>(st.w, img, W, J, c, n, st.active, dp, p, st.d, st.sel, st.rdiag);
}
// NP = 64: the 64 steps as a parameter pack, as the factor kernel has them (the unroller's size limit would leave them a loop, with the
// column in scratch)
template <int NP, int... J>
__device__ __forceinline__ void pv_decide_steps(PvState<NP>& st, const double* img, double* W, int c, int n, int cap, double tol,
                                                std::integer_sequence<int, J...>) {
  (pv_decide_step<NP>(st, img, W, J, c, n, cap, tol), ...);
}

// the whole call of one wave: b is this lane's group's block, nmax the largest n of the wave (uniform)
template <int NP>
__device__ __forceinline__ void pv_run(const PvBlock& b, int nmax, const PvArgs& g, double* s_img, double* s_w, double* s_x, int* s_piv) {
  using Img = PbImg<NP>;
  constexpr int LDW = PvLds<NP>::LDW;
  const int lane = threadIdx.x, grp = lane / NP, c = lane % NP, n = b.n;
  double* img = s_img + grp * Img::SIZE;
  double* W = s_w + grp * PvLds<NP>::W;

  vb_load_upper<Img>(b.A, b.lda, n, nmax, c, img);
  __syncthreads();
  PvState<NP> st;
#pragma unroll
  for (int i = 0; i < NP; i++) st.w[i] = 0.0;
  st.d = c < n ? img[Img::at(c, c)] : 0.0;
  st.rdiag = 1.0; st.tol_used = 0.0;
  st.sel = -1; st.rank = 0; st.info = 0;
  st.active = n > 0;

  if constexpr (NP < 64) {
#pragma unroll
    for (int j = 0; j < NP; j++) pv_decide_step<NP>(st, img, W, j, c, n, b.cap, g.tol);
  } else {
    pv_decide_steps<NP>(st, img, W, c, n, b.cap, g.tol, std::make_integer_sequence<int, NP>{});
  }
  if (__any(st.active)) {                // NP steps done (n = max_rank = NP): nothing is left to choose from
    double dp; int p;
    pv_decide<NP>(NP, c, n, b.cap, g.tol, st.d, st.sel, st.active, st.rank, st.info, st.tol_used, dp, p);
  }

  // piv: a chosen column goes to its step, an unselected one behind the rank chosen ones in index order
  const bool on = c < n, un = on && st.sel < 0;
  const unsigned long long bal = __ballot(un);
  unsigned long long mine = bal;
  if constexpr (NP < 64) mine = (bal >> (grp * NP)) & ((1ull << NP) - 1ull);
  const int pos = un ? st.rank + __popcll(mine & ((1ull << c) - 1ull)) : st.sel;
  if (on) { b.piv[pos] = c; s_piv[grp * NP + pos] = c; }
  s_x[lane] = st.d;
  __syncthreads();
  if (on && c == 0) {
    g.rank[b.out] = st.rank;
    if (g.info) g.info[b.out] = st.info;
    if (g.resid) {
      double s = 0.0;
      for (int q = 0; q < n; q++)
        if ((mine >> q) & 1ull) s += s_x[grp * NP + q];
      g.resid[b.out] = s;
    }
  }
  // R[:, k] = W[0:rank, piv[k]], zero below: lane c takes row c, so the stores run along the columns
#pragma unroll 4
  for (int k = 0; k < nmax; k++)
    if (k < n && c < b.rrows) b.R[c + (int64_t)k * b.ldr] = c < st.rank ? W[c * LDW + s_piv[grp * NP + k]] : 0.0;
  if (g.logdet) {                        // 2 sum_j log r_jj in ascending j: the lane of pivot j takes the logarithm, lane 0 of the group adds them in order
    __syncthreads();
    if (on && st.sel >= 0) s_x[grp * NP + st.sel] = log(st.rdiag);
    __syncthreads();
    if (on && c == 0) {
      double t = 0.0;
      for (int j = 0; j < st.rank; j++) t += s_x[grp * NP + j];
      g.logdet[b.out] = st.info == 2 ? (double)NAN : 2.0 * t;
    }
  }
}

template <int NP>
__global__ __launch_bounds__(64) void pstrf_batched_kernel(PvArgs g) {
  constexpr int G = 64 / NP;
  __shared__ double s_img[G * PbImg<NP>::SIZE];
  __shared__ double s_w[G * PvLds<NP>::W];
  __shared__ double s_x[64];
  __shared__ int s_piv[64];
  const int grp = threadIdx.x / NP;
  const int64_t blk = (int64_t)blockIdx.x * G + grp;
  const bool live = blk < g.batch;
  PvBlock b;
  b.A = g.A + (live ? blk * g.stride_a : 0); b.lda = g.lda;
  b.R = g.R + (live ? blk * g.stride_r : 0); b.ldr = g.ldr;
  b.piv = g.piv + (live ? blk * g.n : 0);
  b.out = live ? blk : 0;
  b.n = live ? g.n : 0; b.cap = g.max_rank; b.rrows = g.max_rank;
  pv_run<NP>(b, g.n, g, s_img, s_w, s_x, s_piv);
}

template <int NP>
__global__ __launch_bounds__(64) void pstrf_vbatched_kernel(PvArgs g) {
  constexpr int G = 64 / NP;
  __shared__ double s_img[G * PbImg<NP>::SIZE];
  __shared__ double s_w[G * PvLds<NP>::W];
  __shared__ double s_x[64];
  __shared__ int s_piv[64];
  const VbGroup v = vb_group<NP>(g.rec, g.list, g.count);
  PvBlock b;
  b.A = g.A + v.off; b.lda = v.ld;
  b.R = g.R + v.off; b.ldr = v.ld;
  b.piv = g.piv + v.row;
  b.out = v.blk;
  b.n = v.n; b.cap = g.max_rank < v.n ? g.max_rank : v.n; b.rrows = g.R ? v.n : 0;
  pv_run<NP>(b, v.nmax, g, s_img, s_w, s_x, s_piv);
}

}  // namespace

extern "C" {

int cap_dpstrf_batched(int uplo, int64_t n, int64_t max_rank, double tol, const double* A, int64_t lda, int64_t stride_a, double* R, int64_t ldr,
                       int64_t stride_r, int64_t* piv, int* rank, double* resid, double* logdet, int* info, int64_t batch, void* stream) {
  if (n < 0 || batch < 0 || max_rank < 0 || max_rank > n || tol != tol) return CAP_ERR_ARG;
  const bool work = n > 0 && batch > 0;
  if (work && (!A || !piv || !rank)) return CAP_ERR_ARG;
  if (work && max_rank > 0 && !R) return CAP_ERR_ARG;
  if (!vb_operand_ok(n, n, lda, stride_a, batch)) return CAP_ERR_ARG;
  if (max_rank > 0 && !vb_operand_ok(max_rank, n, ldr, stride_r, batch)) return CAP_ERR_ARG;
  if (uplo != CAP_UPPER) return CAP_ERR_UNSUPPORTED;    // as cap_dpstrf: in front of the empty case
  if (n > PB_MAX) return CAP_ERR_UNSUPPORTED;
  const int np = vb_padded(n);
  const int64_t nwg = vb_grid(batch, 64 / np);
  if (nwg < 0) return CAP_ERR_UNSUPPORTED;
  if (!work) return CAP_OK;
  PvArgs g = {};
  g.A = A; g.R = R; g.piv = piv; g.rank = rank; g.resid = resid; g.logdet = logdet; g.info = info;
  g.tol = tol; g.max_rank = (int)max_rank;
  g.lda = lda; g.stride_a = stride_a; g.ldr = ldr; g.stride_r = stride_r; g.batch = batch; g.n = (int)n;
  if (cap_acc_on()) {
    cap_acc_r(A, 0, (batch - 1) * stride_a + (n - 1) * lda + n, 1);
    if (max_rank > 0) cap_acc_w(R, 0, (batch - 1) * stride_r + (n - 1) * ldr + max_rank, 1);
    cap_acc_w(piv, 0, batch * n, 1);
    cap_acc_w(rank, 0, batch, 1, 0, 4);
    if (resid) cap_acc_w(resid, 0, batch, 1);
    if (logdet) cap_acc_w(logdet, 0, batch, 1);
    if (info) cap_acc_w(info, 0, batch, 1, 0, 4);
  }
  hipStream_t s = cap_stream(stream);
  vb_with_int<8, 16, 32, 64>(np, [&](auto NP) { hipLaunchKernelGGL(pstrf_batched_kernel<NP()>, dim3((unsigned)nwg), dim3(64), 0, s, g); });
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}

int cap_dpstrf_vbatched(const cap_vbatch_plan* p, int uplo, int64_t max_rank, double tol, const double* A, double* R, int64_t* piv, int* rank,
                        double* resid, double* logdet, int* info, void* stream) {
  if (!p || max_rank < 0 || tol != tol) return CAP_ERR_ARG;
  if (p->nonempty > 0 && (!A || !piv || !rank)) return CAP_ERR_ARG;
  if (p->nonempty > 0 && max_rank > 0 && !R) return CAP_ERR_ARG;
  if (uplo != CAP_UPPER) return CAP_ERR_UNSUPPORTED;
  if (p->nmax > PB_MAX) return CAP_ERR_UNSUPPORTED;
  if (p->nonempty == 0) return CAP_OK;
  if (p->device < 0) return CAP_ERR_HIP;
  PvArgs g = {};
  g.A = A; g.R = R; g.piv = piv; g.rank = rank; g.resid = resid; g.logdet = logdet; g.info = info;
  g.tol = tol; g.max_rank = (int)(max_rank < PB_MAX ? max_rank : PB_MAX);
  g.rec = p->d_rec;
  hipStream_t s = cap_stream(stream);
  return vb_for_each_class(p, [&](int cls, const int64_t* list, int64_t count, const std::vector<int64_t>& blocks, dim3 grid) {
    g.list = list;
    g.count = count;
    if (cap_acc_on()) {
      for (int64_t b : blocks) {
        const VbRec& r = p->rec[(size_t)b];
        cap_acc_r(A + r.off, r.ld, r.n, r.n, 1);
        if (R) cap_acc_w(R + r.off, r.ld, r.n, r.n);
        cap_acc_w(piv + r.row, 0, r.n, 1);
        cap_acc_w(rank + b, 0, 1, 1, 0, 4);
        if (resid) cap_acc_w(resid + b, 0, 1, 1);
        if (logdet) cap_acc_w(logdet + b, 0, 1, 1);
        if (info) cap_acc_w(info + b, 0, 1, 1, 0, 4);
      }
    }
    vb_with_int<8, 16, 32, 64>(8 << cls, [&](auto NP) { hipLaunchKernelGGL(pstrf_vbatched_kernel<NP()>, grid, dim3(64), 0, s, g); });
  });
}

}  // extern "C"
