// Pivoted Cholesky factorization with a rank cap and a stopping tolerance (cap_dpstrf, cholinv.hip; LAPACK's dpstrf): A[piv][:, piv] ~ R^T R
// for a symmetric positive SEMIdefinite A, left-looking, so that r steps cost O(n r^2) and A is only read - one row and its diagonal.
//
// State in `work`: the remaining diagonal d[n], sel[n] (the step at which a column was chosen, -1: not yet), the factor W (row j = step j,
// natural column order, column-major with leading dimension ldw >= max_rank: the j entries of a column are contiguous), two sets of
// per-workgroup partial results and one control block.  Step j, with p the unselected column of largest d (ties: lowest index):
//   W[j, c] = (A(p, c) - sum_{i<j} W[i, p] W[i, c]) / sqrt(d[p])  and  d[c] -= W[j, c]^2   for every unselected c != p,
//   W[j, p] = sqrt(d[p]),  W[j, c] = 0 for the columns chosen before,   sel[p] = j
// It stops at a NaN on the remaining diagonal (info 2), at d[p] <= tol or after n steps (info 0), or at step max_rank (info 1).
//
// ONE PLAIN LAUNCH PER STEP, no host synchronisation and nothing between workgroups inside a launch: workgroup b owns the columns
// [64 b, 64 b + 64) for the whole call.  A launch ends with every workgroup writing the (largest d, its column, saw-NaN) of its own
// unselected columns; the next launch starts with EVERY workgroup reading all of these records and reducing them itself - the same
// records in the same order, hence the same pivot and the same decision everywhere.  The launch boundary is the only synchronisation.
// The records alternate between two sets by the parity of the step, so a workgroup that is already writing its record of step j
// cannot disturb one that still reads the records of step j - 1.  Workgroup 0 notes the pivot in piv[j]; at the stopping decision it
// sets the control block's stop word instead, which turns the remaining step launches of the call into immediate exits (the host always
// enqueues max_rank of them: it cannot know the rank).
// A step in a workgroup: the pivot column W[0:j, p] goes to LDS (in chunks of PS_CHUNK entries), the 64 columns are streamed against it
// with LPC lanes per column - 4 / 16 / 64 by j (a kernel each), so that a wave's loads are whole 16-byte pieces of contiguous column
// entries whether the columns are short or long - the partial sums are folded by a butterfly inside the LPC lanes, and wave 0 finishes one column per
// lane: row j of W (a strided store, one element per column), d, and the record for the next step.  All orders of summation depend
// on (n, max_rank, j) alone: two calls give the same bits.
// The last launch (same grid) takes the decision that is still open after max_rank steps and writes the results: rank, info, resid (the
// remaining diagonal, summed by workgroup 0 as 256 consecutive pieces, the pieces in order), the tail of piv and R[:, k] = W[:, piv[k]] -
// a workgroup finds the places of its 64 columns from sel, a count over piv[0:rank] and a ballot, so no scan over n is needed.
#include <math.h>

#include "common.h"

namespace {

constexpr int PS_T = 256;             // threads of a workgroup
constexpr int PS_CW = 64;             // columns of a workgroup
constexpr int PS_CHUNK = 1024;        // entries of the pivot column in LDS at a time (even: chunks start on 16-byte pieces)
constexpr double PS_EPS = 0x1p-53;    // LAPACK's dlamch('Epsilon'): the default tolerance is n eps max_i a_ii

struct PsRec { double v; int idx; int nan; };       // a workgroup's best unselected column (idx -1: none) and whether it saw a NaN
struct PsCtl { int stopped; int info; long long rank; double tol; double pad; };

struct PsArgs {
  const double* A; int64_t lda;
  double* d; int* sel; PsRec* rec; PsCtl* ctl;     // rec: two sets of nwg records, set (j & 1) is read by step j
  double* W; int64_t ldw;
  double* R; int64_t ldr; int64_t* piv; int64_t* rank; double* resid; int* info;
  double tol;
  int n, max_rank, nwg, j;
};

// the better of two records: larger value, then lower index; a record without a column loses
__device__ __forceinline__ void ps_better(double& v, int& i, double ov, int oi) {
  if (oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i))) { v = ov; i = oi; }
}

__device__ __forceinline__ void ps_wave_best(double& v, int& i, int& nan) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double ov = __shfl_xor(v, off);
    const int oi = __shfl_xor(i, off);
    nan |= __shfl_xor(nan, off);
    ps_better(v, i, ov, oi);
  }
}

// every thread of the workgroup gets the reduction of the nwg records of set `set` and thread 0's `word` (s_*: LDS of PS_T / 64 entries)
__device__ __forceinline__ void ps_reduce_records(const PsArgs& g, int set, double* s_v, int* s_i, int* s_n, double& v, int& idx, int& nan,
                                                  int& word) {
  v = -INFINITY; idx = -1; nan = 0;
  const PsRec* rec = g.rec + (int64_t)set * g.nwg;
  for (int b = threadIdx.x; b < g.nwg; b += PS_T) {
    const PsRec r = rec[b];
    nan |= r.nan;
    ps_better(v, idx, r.v, r.idx);
  }
  ps_wave_best(v, idx, nan);
  if ((threadIdx.x & 63) == 0) { s_v[threadIdx.x >> 6] = v; s_i[threadIdx.x >> 6] = idx; s_n[threadIdx.x >> 6] = nan; }
  if (threadIdx.x == 0) s_n[PS_T / 64] = word;
  __syncthreads();
  v = s_v[0]; idx = s_i[0]; nan = s_n[0]; word = s_n[PS_T / 64];
#pragma unroll
  for (int w = 1; w < PS_T / 64; w++) { nan |= s_n[w]; ps_better(v, idx, s_v[w], s_i[w]); }
}

// the decision in front of step j from the reduced records: 0 = go on with pivot idx, else stop with info = return value - 1
// (tol_used: in front of step 0 it is formed here, later it is the control block's)
__device__ __forceinline__ int ps_decide(const PsArgs& g, int j, double v, int idx, int nan, double& tol_used) {
  if (j == 0) tol_used = g.tol < 0 ? (double)g.n * PS_EPS * v : g.tol;
  if (nan) return 3;
  if (idx < 0 || !(v > tol_used)) return 1;
  if (j == g.max_rank) return 2;
  return 0;
}

// d = diag(A), nothing selected, the records of step 0; one thread per column
__global__ __launch_bounds__(PS_CW) void pstrf_init_kernel(PsArgs g) {
  const int c = blockIdx.x * PS_CW + threadIdx.x;
  double v = -INFINITY; int idx = -1, nan = 0;
  if (c < g.n) {
    const double a = g.A[c + (int64_t)c * g.lda];
    g.d[c] = a;
    g.sel[c] = -1;
    if (a != a) nan = 1; else { v = a; idx = c; }
  }
  ps_wave_best(v, idx, nan);
  if (threadIdx.x == 0) {
    g.rec[blockIdx.x] = PsRec{v, idx, nan};
    if (blockIdx.x == 0) *g.ctl = PsCtl{0, 0, 0, 0.0, 0.0};
  }
}

// the dots of this workgroup's 64 columns with the pivot column, LPC lanes per column: group q = tid / LPC owns the LPC / 4 consecutive
// columns from q LPC / 4 on; lane l of the group takes the 16-byte pieces l, l + LPC, ... of every chunk, at most 8 columns at a time
template <int LPC>
__device__ __forceinline__ void ps_dots(const PsArgs& g, int j, int p, const int* s_sel, double* s_pc, double* s_dot) {
  constexpr int CPG = LPC / 4, NB = CPG < 8 ? CPG : 8;
  // (LPC = 64: the group is the wave, and saying so keeps the column addresses in scalar registers)
  const int grp = LPC == 64 ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : threadIdx.x / LPC, l = threadIdx.x % LPC;
  const int c0 = blockIdx.x * PS_CW + grp * CPG;
  double acc[CPG];
  bool on[CPG];
#pragma unroll
  for (int q = 0; q < CPG; q++) {
    acc[q] = 0.0;
    on[q] = c0 + q < g.n && s_sel[grp * CPG + q] < 0;
  }
  const double* col0 = g.W + (int64_t)c0 * g.ldw;      // columns of the group: col0 + q ldw (read only where on[q])
  const double* pcol = g.W + (int64_t)p * g.ldw;
  for (int k0 = 0; k0 < j; k0 += PS_CHUNK) {
    const int kc = min(PS_CHUNK, j - k0);
    if (k0) __syncthreads();                           // the previous chunk has been used
    for (int i = threadIdx.x; i < kc; i += PS_T) s_pc[i] = pcol[k0 + i];
    if ((kc & 1) && threadIdx.x == 0) s_pc[kc] = 0.0;  // an odd last entry (only the last chunk has one) is paired with a zero
    __syncthreads();
    const int npair = (kc + 1) >> 1;
#pragma unroll
    for (int q0 = 0; q0 < CPG; q0 += NB) {             // (a loop over the chunk per batch: NB loads in flight, not CPG)
#pragma unroll 1
      for (int ip = l; ip < npair; ip += LPC) {
        const d2 pv = *reinterpret_cast<const d2*>(s_pc + 2 * ip);
        const bool whole = 2 * ip + 1 < kc;
        d2 w[NB];
#pragma unroll
        for (int q = 0; q < NB; q++) {
          const double* src = col0 + (q0 + q) * g.ldw + k0 + 2 * ip;
          if (on[q0 + q]) {
            if (whole) w[q] = *reinterpret_cast<const d2*>(src);
            else { w[q].x = *src; w[q].y = 0.0; }
          }
        }
#pragma unroll
        for (int q = 0; q < NB; q++)
          if (on[q0 + q]) { acc[q0 + q] = fma(w[q].x, pv.x, acc[q0 + q]); acc[q0 + q] = fma(w[q].y, pv.y, acc[q0 + q]); }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < CPG; q++) {
#pragma unroll
    for (int off = LPC / 2; off >= 1; off >>= 1) acc[q] += __shfl_xor(acc[q], off);
    if (l == 0) s_dot[grp * CPG + q] = acc[q];
  }
}

// step j; LPC = 4 / 16 / 64 lanes per column for j <= 16 / <= 128 / above (chosen by the host: the short-column forms need few registers)
template <int LPC>
__global__ __launch_bounds__(PS_T, 4) void pstrf_step_kernel(PsArgs g) {   // four workgroups per CU: the 1024 of n = 65536 in one round
  __shared__ __attribute__((aligned(16))) double s_pc[PS_CHUNK + 2];
  __shared__ double s_dot[PS_CW];
  __shared__ double s_v[PS_T / 64];
  __shared__ int s_i[PS_T / 64], s_n[PS_T / 64 + 1];
  __shared__ int s_sel[PS_CW];
  const int j = g.j, t = threadIdx.x, c = blockIdx.x * PS_CW + t;
  // everything that does not depend on the pivot is requested first: the stop word (ONE read per workgroup - workgroup 0 of THIS launch
  // may be setting it, and the exit has to be the whole workgroup's), the tolerance, this workgroup's column state, the records
  int stopped = t == 0 ? g.ctl->stopped : 0;
  double tol_used = j > 0 ? g.ctl->tol : 0.0;
  int sc = 0;
  double dc = 0.0;
  if (t < PS_CW && c < g.n) { sc = g.sel[c]; dc = g.d[c]; }
  double dp; int p, nan;
  ps_reduce_records(g, j & 1, s_v, s_i, s_n, dp, p, nan, stopped);
  if (stopped) return;
  const int stop = ps_decide(g, j, dp, p, nan, tol_used);
  if (blockIdx.x == 0 && t == 0) {
    if (stop) { g.ctl->rank = j; g.ctl->info = stop - 1; g.ctl->stopped = 1; }
    else { g.piv[j] = p; if (j == 0) g.ctl->tol = tol_used; }
  }
  if (stop) return;
  // wave 0: one column per lane - its element of row p of A (upper triangle) is in flight while the dots are formed
  double a_pc = 0.0;
  if (t < PS_CW) {
    s_sel[t] = sc;
    if (sc < 0) a_pc = c >= p ? g.A[p + (int64_t)c * g.lda] : g.A[c + (int64_t)p * g.lda];
  }
  __syncthreads();
  ps_dots<LPC>(g, j, p, s_sel, s_pc, s_dot);
  __syncthreads();
  if (t >= 64) return;
  double bv = -INFINITY; int bi = -1, bn = 0;
  if (c < g.n) {
    double* wj = g.W + j + (int64_t)c * g.ldw;
    if (sc >= 0) *wj = 0.0;
    else if (c == p) { *wj = __dsqrt_rn(dp); g.sel[c] = j; }
    else {
      const double r = (a_pc - s_dot[t]) / __dsqrt_rn(dp);
      *wj = r;
      dc = fma(-r, r, dc);
      g.d[c] = dc;
      if (dc != dc) bn = 1; else { bv = dc; bi = c; }
    }
  }
  ps_wave_best(bv, bi, bn);
  if (t == 0) g.rec[(int64_t)((j + 1) & 1) * g.nwg + blockIdx.x] = PsRec{bv, bi, bn};
}

__global__ __launch_bounds__(PS_T) void pstrf_finish_kernel(PsArgs g) {
  __shared__ double s_v[PS_T / 64];
  __shared__ int s_i[PS_T / 64], s_n[PS_T / 64 + 1];
  __shared__ double s_sum[PS_T];
  __shared__ int s_cnt[PS_T / 64];
  __shared__ int64_t s_pos[PS_CW];
  const int t = threadIdx.x;
  int64_t rank; int info;
  if (g.ctl->stopped) { rank = g.ctl->rank; info = g.ctl->info; }        // (this launch does not write the control block)
  else {
    double v, tol_used = g.max_rank > 0 ? g.ctl->tol : 0.0; int idx, nan, word = 0;
    ps_reduce_records(g, g.max_rank & 1, s_v, s_i, s_n, v, idx, nan, word);
    rank = g.max_rank;
    info = ps_decide(g, g.max_rank, v, idx, nan, tol_used) - 1;
  }
  if (blockIdx.x == 0) {
    if (t == 0) { *g.rank = rank; if (g.info) *g.info = info; }
    if (g.resid) {                     // thread t sums its piece of the columns in order, thread 0 the 256 pieces in order
      const int per = (g.n + PS_T - 1) / PS_T;
      double s = 0.0;
      for (int c = t * per; c < min(g.n, (t + 1) * per); c++)
        if (g.sel[c] < 0) s += g.d[c];
      s_sum[t] = s;
      __syncthreads();
      if (t == 0) {
        double tot = 0.0;
        for (int i = 0; i < PS_T; i++) tot += s_sum[i];
        *g.resid = tot;
      }
    }
  }
  // places of my 64 columns: a chosen column goes to its step, an unselected one behind the rank chosen ones in index order -
  // rank + (unselected columns in front of it) = rank + c - (chosen columns in front of it)
  const int cbase = blockIdx.x * PS_CW;
  int before = 0;
  for (int64_t k = t; k < rank; k += PS_T) before += g.piv[k] < cbase ? 1 : 0;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) before += __shfl_xor(before, off);
  if ((t & 63) == 0) s_cnt[t >> 6] = before;
  __syncthreads();
  if (t < PS_CW) {
    const int c = cbase + t;
    const int sc = c < g.n ? g.sel[c] : 0;
    const unsigned long long un = __ballot(sc < 0);
    int64_t pos = sc;
    if (sc < 0) {
      before = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
      pos = rank + (cbase - before) + __popcll(un & ((1ull << t) - 1ull));
      g.piv[pos] = c;
    }
    s_pos[t] = pos;
  }
  __syncthreads();
  // R[:, place] = W[0:rank, c], zero below: a wave per column, lanes along the (contiguous) rows
  for (int q = t >> 6; q < PS_CW; q += PS_T / 64) {
    const int c = cbase + q;
    if (c >= g.n) break;
    const double* src = g.W + (int64_t)c * g.ldw;
    double* dst = g.R + s_pos[q] * g.ldr;
    for (int i = t & 63; i < g.max_rank; i += 64) dst[i] = i < rank ? src[i] : 0.0;
  }
}

struct PsLayout { int64_t ctl, d, sel, rec, W, total; };

// offsets in doubles from the 16-byte aligned start of the work area
PsLayout ps_layout(int64_t n, int64_t max_rank) {
  const int64_t nwg = cap_ceil_div(n, PS_CW), ldw = cap_round_up(max_rank, 2);
  PsLayout L;
  L.ctl = 0;
  L.d = L.ctl + (int64_t)sizeof(PsCtl) / 8;
  L.sel = L.d + cap_round_up(n, 2);
  L.rec = L.sel + cap_round_up(n, 4) / 2;
  L.W = L.rec + 2 * nwg * (int64_t)(sizeof(PsRec) / 8);
  L.total = L.W + ldw * n;
  return L;
}

}  // namespace

int64_t cap_pstrf_work_size(int64_t n, int64_t max_rank) {
  if (n <= 0 || max_rank < 0) return 0;
  return ps_layout(n, max_rank).total + 1;             // + 1: the work area starts at the first 16-byte boundary of `work`
}

int cap_pstrf_run(int64_t n, int64_t max_rank, double tol, const double* A, int64_t lda, double* R, int64_t ldr, int64_t* piv,
                  int64_t* rank, double* resid, int* info, double* work, hipStream_t s) {
  if (n <= 0) return CAP_OK;
  if (n > ((int64_t)1 << 30)) return CAP_ERR_ARG;        // column indices are ints
  static_assert(sizeof(PsCtl) == 32 && sizeof(PsRec) == 16, "work layout");
  double* base = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(work) + 15) & ~(uintptr_t)15);
  const PsLayout L = ps_layout(n, max_rank);
  PsArgs g;
  g.A = A; g.lda = lda;
  g.ctl = reinterpret_cast<PsCtl*>(base + L.ctl);
  g.d = base + L.d;
  g.sel = reinterpret_cast<int*>(base + L.sel);
  g.rec = reinterpret_cast<PsRec*>(base + L.rec);
  g.W = base + L.W; g.ldw = cap_round_up(max_rank, 2);
  g.R = R; g.ldr = ldr; g.piv = piv; g.rank = rank; g.resid = resid; g.info = info;
  g.tol = tol;
  g.n = (int)n; g.max_rank = (int)max_rank; g.nwg = (int)cap_ceil_div(n, PS_CW); g.j = 0;
  // access notes, the same for every launch of the call: A's upper triangle is read, the work area and the results are this call's own
  auto notes = [&]() {
    if (!cap_acc_on()) return;
    cap_acc_r(A, lda, n, n, 1);
    cap_acc_rw(base, 0, L.total, 1);
    cap_acc_rw(piv, 0, n, 1);
  };
  notes();
  hipLaunchKernelGGL(pstrf_init_kernel, dim3(g.nwg), dim3(PS_CW), 0, s, g);
  CAP_HIP(hipGetLastError());
  for (int j = 0; j < (int)max_rank; j++) {
    g.j = j;
    notes();
    if (j <= 16) hipLaunchKernelGGL(pstrf_step_kernel<4>, dim3(g.nwg), dim3(PS_T), 0, s, g);
    else if (j <= 128) hipLaunchKernelGGL(pstrf_step_kernel<16>, dim3(g.nwg), dim3(PS_T), 0, s, g);
    else hipLaunchKernelGGL(pstrf_step_kernel<64>, dim3(g.nwg), dim3(PS_T), 0, s, g);
    CAP_HIP(hipGetLastError());
  }
  g.j = (int)max_rank;
  notes();
  if (cap_acc_on()) {
    if (max_rank > 0) cap_acc_w(R, ldr, max_rank, n);
    cap_acc_w(rank, 0, 1, 1);
    if (resid) cap_acc_w(resid, 0, 1, 1);
    if (info) cap_acc_w(info, 0, 1, 1, 0, 4);
  }
  hipLaunchKernelGGL(pstrf_finish_kernel, dim3(g.nwg), dim3(PS_T), 0, s, g);
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}
