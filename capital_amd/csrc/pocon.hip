// LAPACK's dlacn2 on the device, for the operator diag(w) A^-1 and its transpose A^-1 diag(w) with A = R^T R: the 1-norm estimate behind
// cap_dpocon (w = 1, one column) and behind the forward error bound of cap_dpoerr (one w per right-hand side, up to 16 columns in
// lock-step, because the substitution of potrs.hip solves 16 columns for little more than the price of one).
//
// dlacn2 is a reverse-communication loop: "apply the operator to x, come back".  Here every column keeps its own state (the stage it
// comes back to, est, the last index, the iteration count, done) in device memory, and ONE STEP is one solve A^-1 with all columns
// followed by pocon_step_kernel, one workgroup per column, which scales by w where the stage's operator asks for it, takes the stage's
// decision and leaves the next vector.  The stages are dlacn2's, exactly: the start vector 1 / n; the sign vector; the stop at a
// repeated sign vector or an estimate that did not grow; the arg max with the lowest index winning ties; ITMAX = 5; the final
// alternating-sign vector with its 2 |x|_1 / (3 n) floor.  A finished column is frozen: later solves run on whatever it holds and are ignored.
// No host synchronisation: the launch sequence is fixed at the 11 solves dlacn2 can need.  The column that finishes last sets the skip
// word, which turns the solves behind it into immediate exits (cap_potrs_subst) and the step kernels too.  The inverses of R's diagonal
// blocks are the caller's, made once.  Every reduction (|x|_1, arg max, the sign comparison) is a strided partial per thread followed by
// a tree over the 256 threads: fixed order, two calls give the same bits.
#include <algorithm>

#include "common.h"

namespace {

constexpr int PC_T = 256;
constexpr int PC_MAXC = 16;
constexpr int PC_SOLVES = 11;         // 1 + 1 + 2 (ITMAX - 1) + 1
constexpr int PC_ITMAX = 5;
constexpr double PC_EPS = 0x1p-53;                        // dlamch('Epsilon')
constexpr double PC_SAFMIN = 2.2250738585072014e-308;     // dlamch('Safe minimum')

struct PcState { double est, xmax; int stage, j, iter, done, solves, pad; };   // 40 bytes
struct PcCtl { int skip, ndone, pad0, pad1; };

struct PcArgs {
  PcCtl* ctl; PcState* st;
  double* V; double* SG; int64_t ldv;      // the vectors x (solved in place) and the sign vectors, n x nc
  const double* W;                         // n x nc (ld ldv) or NULL: ones
  const double* Res; double* Den;          // init only: B - A X and |A||X| + |B| (becomes W)
  const double* X; int64_t ldx;
  const double* anorm; double* out; double* berr;
  const int* info; int* words;
  int n, nc, want_est;
};

__device__ __forceinline__ double pc_block_sum(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int w = PC_T / 2; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

__device__ __forceinline__ double pc_block_max(double v, double* sh) {     // plain max of non-negative values, NaN is dropped (as LAPACK)
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int w = PC_T / 2; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + w]);
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

__device__ __forceinline__ int pc_block_and(int v, int* shi) {
  shi[threadIdx.x] = v;
  __syncthreads();
  for (int w = PC_T / 2; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) shi[threadIdx.x] &= shi[threadIdx.x + w];
    __syncthreads();
  }
  const int r = shi[0];
  __syncthreads();
  return r;
}

// idamax: the largest |x_i| z_i = x_i, the lowest index among equals
__device__ __forceinline__ int pc_block_argmax(const double* x, int n, double* sh, int* shi) {
  double bv = -1.0; int bi = 0x7fffffff;
  for (int i = threadIdx.x; i < n; i += PC_T) {
    const double a = fabs(x[i]);
    if (a > bv) { bv = a; bi = i; }            // ascending i per thread: the first of equals stays
  }
  sh[threadIdx.x] = bv; shi[threadIdx.x] = bi;
  __syncthreads();
  for (int w = PC_T / 2; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) {
      const double ov = sh[threadIdx.x + w]; const int oi = shi[threadIdx.x + w];
      if (ov > sh[threadIdx.x] || (ov == sh[threadIdx.x] && oi < shi[threadIdx.x])) { sh[threadIdx.x] = ov; shi[threadIdx.x] = oi; }
    }
    __syncthreads();
  }
  int r = shi[0];
  __syncthreads();
  if (r >= n) r = 0;                            // every entry NaN: LAPACK's idamax answers the first
  return r;
}

// the start of every column (one workgroup each): the dporfs quantities when Res is given, x = 1 / n, stage 1
__global__ void __launch_bounds__(PC_T) pocon_init_kernel(const PcArgs g) {
  __shared__ double sh[PC_T];
  const int c = blockIdx.x, t = threadIdx.x, n = g.n;
  const bool bad = g.info && *g.info != 0;
  double xmax = 0.0;
  if (g.Res) {
    const double* res = g.Res + (int64_t)c * g.ldv;
    double* den = g.Den + (int64_t)c * g.ldv;
    const double* x = g.X + (int64_t)c * g.ldx;
    const double nz = (double)(n + 1), safe1 = nz * PC_SAFMIN, safe2 = safe1 / PC_EPS;
    double q = 0.0, xm = 0.0;
    for (int i = t; i < n; i += PC_T) {
      const double r = fabs(res[i]), d = den[i];
      if (d > safe2) { q = fmax(q, r / d); den[i] = r + nz * PC_EPS * d; }
      else { q = fmax(q, (r + safe1) / (d + safe1)); den[i] = r + nz * PC_EPS * d + safe1; }
      xm = fmax(xm, fabs(x[i]));
    }
    q = pc_block_max(q, sh);
    xmax = pc_block_max(xm, sh);
    if (t == 0 && g.berr) g.berr[c] = bad ? __builtin_nan("") : q;
  }
  if (!g.want_est) return;
  double* v = g.V + (int64_t)c * g.ldv;
  const double x0 = 1.0 / (double)n;
  for (int i = t; i < n; i += PC_T) v[i] = x0;
  if (t == 0) {
    g.st[c] = PcState{0.0, xmax, 1, 0, 0, 0, 0, 0};
    if (c == 0) *g.ctl = PcCtl{bad ? 1 : 0, 0, 0, 0};
  }
}

// x <- e_j
__device__ __forceinline__ void pc_unit(double* v, int n, int j) {
  for (int i = threadIdx.x; i < n; i += PC_T) v[i] = i == j ? 1.0 : 0.0;
}
// x_i <- (-1)^i (1 + i / (n - 1))
__device__ __forceinline__ void pc_altsgn(double* v, int n) {
  for (int i = threadIdx.x; i < n; i += PC_T) v[i] = ((i & 1) ? -1.0 : 1.0) * (1.0 + (double)i / (double)(n - 1));
}

__global__ void __launch_bounds__(PC_T) pocon_step_kernel(const PcArgs g) {
  __shared__ double sh[PC_T];
  __shared__ int shi[PC_T];
  __shared__ PcState s_st;
  __shared__ int s_skip;
  const int c = blockIdx.x, t = threadIdx.x, n = g.n;
  if (t == 0) { s_st = g.st[c]; s_skip = g.ctl->skip; }
  __syncthreads();
  PcState st = s_st;
  if (s_skip || st.done) return;
  double* v = g.V + (int64_t)c * g.ldv;
  double* sg = g.SG + (int64_t)c * g.ldv;
  const double* w = g.W ? g.W + (int64_t)c * g.ldv : nullptr;
  st.solves++;
  bool done = false;
  if (st.stage == 1) {                                   // x = diag(w) A^-1 (1 / n)
    if (n == 1) {
      st.est = fabs(w ? w[0] * v[0] : v[0]);
      done = true;
    } else {
      double a = 0.0;
      for (int i = t; i < n; i += PC_T) {
        const double wi = w ? w[i] : 1.0, xi = wi * v[i], s = xi > 0.0 ? 1.0 : -1.0;
        a += fabs(xi);
        sg[i] = s;
        v[i] = wi * s;                                   // next: A^-1 diag(w) sign
      }
      st.est = pc_block_sum(a, sh);
      st.stage = 2;
    }
  } else if (st.stage == 2 || st.stage == 4) {           // x = A^-1 diag(w) sign
    const int jlast = st.j;
    const int j = pc_block_argmax(v, n, sh, shi);
    const double xl = v[jlast], xj = fabs(v[j]);
    __syncthreads();                                     // v is read before it is rewritten
    st.j = j;
    if (st.stage == 2) { st.iter = 2; pc_unit(v, n, j); st.stage = 3; }
    else if (xl != xj && st.iter < PC_ITMAX) { st.iter++; pc_unit(v, n, j); st.stage = 3; }
    else { pc_altsgn(v, n); st.stage = 5; }
  } else if (st.stage == 3) {                            // x = diag(w) A^-1 e_j
    double a = 0.0; int same = 1;
    for (int i = t; i < n; i += PC_T) {
      const double xi = (w ? w[i] : 1.0) * v[i];
      a += fabs(xi);
      if ((xi > 0.0 ? 1.0 : -1.0) != sg[i]) same = 0;
    }
    const double estold = st.est;
    st.est = pc_block_sum(a, sh);
    same = pc_block_and(same, shi);
    if (same || st.est <= estold) { pc_altsgn(v, n); st.stage = 5; }
    else {
      for (int i = t; i < n; i += PC_T) {
        const double wi = w ? w[i] : 1.0, s = wi * v[i] > 0.0 ? 1.0 : -1.0;
        sg[i] = s;
        v[i] = wi * s;
      }
      st.stage = 4;
    }
  } else {                                               // stage 5: x = diag(w) A^-1 (alternating signs)
    double a = 0.0;
    for (int i = t; i < n; i += PC_T) a += fabs((w ? w[i] : 1.0) * v[i]);
    const double temp = 2.0 * (pc_block_sum(a, sh) / (double)(3 * (int64_t)n));
    if (temp > st.est) st.est = temp;
    done = true;
  }
  if (t == 0) {
    st.done = done ? 1 : 0;
    g.st[c] = st;
    // the column that finishes last closes the solves behind it (an integer count: the order of arrival does not matter)
    if (done && atomicAdd(&g.ctl->ndone, 1) == g.nc - 1) g.ctl->skip = 1;
  }
}

__global__ void pocon_finish_kernel(const PcArgs g) {
  const int c = threadIdx.x;
  const bool bad = g.info && *g.info != 0;
  if (c < g.nc) {
    const PcState st = g.st[c];
    double r;
    if (g.anorm) {
      const double a = *g.anorm;
      if (bad) r = 0.0;
      else if (a != a) r = a;
      else if (a == 0.0 || st.est == 0.0) r = 0.0;
      else r = (1.0 / st.est) / a;
    } else {
      r = st.est;
      if (st.xmax != 0.0) r /= st.xmax;
      if (bad) r = __builtin_nan("");
    }
    g.out[c] = r;
  }
  if (c == 0 && g.words) {
    int m = 0;
    for (int k = 0; k < g.nc; k++) m = max(m, g.st[k].solves);
    g.words[2] = m;
  }
}

struct PcLayout { int64_t ctl, st, ctr, V, SG, Y, S, total; };

PcLayout pc_layout(int64_t n, int64_t nc) {
  const int64_t ldv = cap_pocon_ld(n);
  PcLayout L;
  L.ctl = 0;
  L.st = L.ctl + 2;
  L.ctr = L.st + PC_MAXC * (int64_t)(sizeof(PcState) / 8);
  L.V = L.ctr + cap_round_up(PC_SOLVES * 2 * cap_potrs_ctr_ints(n), 2) / 2;
  L.SG = L.V + ldv * nc;
  L.Y = L.SG + ldv * nc;
  L.S = L.Y + ldv * nc;
  L.total = L.S + ldv * nc;
  return L;
}

}  // namespace

int64_t cap_pocon_ld(int64_t n) { return cap_round_up(n, cap_potrs_block()); }

int64_t cap_pocon_est_work(int64_t n, int64_t nc) {
  if (n <= 0 || nc <= 0) return 0;
  return pc_layout(n, std::min<int64_t>(nc, PC_MAXC)).total;
}

int cap_pocon_run(int64_t n, int64_t nc, const double* R, int64_t ldr, const double* Inv, const double* Res, double* Den, const double* X,
                  int64_t ldx, const double* anorm, double* out, double* berr, int want_est, const int* info, double* work, hipStream_t s) {
  if (n <= 0 || nc <= 0) return CAP_OK;
  if (nc > PC_MAXC || n > ((int64_t)1 << 24)) return CAP_ERR_ARG;
  static_assert(sizeof(PcState) == 40 && sizeof(PcCtl) == 16, "work layout");
  const PcLayout L = pc_layout(n, nc);
  const int64_t ldv = cap_pocon_ld(n), cw = cap_potrs_ctr_ints(n);
  int* words = nullptr;
  CAP_TRY(cap_potrs_words(&words));
  PcArgs g;
  g.ctl = reinterpret_cast<PcCtl*>(work + L.ctl);
  g.st = reinterpret_cast<PcState*>(work + L.st);
  g.V = work + L.V; g.SG = work + L.SG; g.ldv = ldv;
  g.W = Res ? Den : nullptr;
  g.Res = Res; g.Den = Den; g.X = X; g.ldx = ldx;
  g.anorm = anorm; g.out = out; g.berr = berr;
  g.info = info; g.words = words;
  g.n = (int)n; g.nc = (int)nc; g.want_est = want_est;
  int* ctr = reinterpret_cast<int*>(work + L.ctr);
  double* Y = work + L.Y; double* S = work + L.S;
  // access notes: the work area is this call's own; what the launches read of the caller's is named per launch
  auto notes = [&]() {
    if (!cap_acc_on()) return;
    cap_acc_rw(work, 0, L.total, 1);
    if (Res) { cap_acc_r(Res, ldv, n, nc); cap_acc_rw(Den, ldv, n, nc); }
    if (info) cap_acc_r(info, 1, 1, 1, 0, 4);
  };
  notes();
  if (cap_acc_on()) {
    if (Res) cap_acc_r(X, ldx, n, nc);
    if (berr) cap_acc_w(berr, 0, nc, 1);
  }
  hipLaunchKernelGGL(pocon_init_kernel, dim3((unsigned)nc), dim3(PC_T), 0, s, g);
  CAP_HIP(hipGetLastError());
  if (!want_est) return CAP_OK;
  // (no access note: a memset is no launch, the replay's stand-in records the window of a memset itself)
  CAP_HIP(hipMemsetAsync(ctr, 0, sizeof(int) * PC_SOLVES * 2 * cw, s));         // the counters of all 22 substitutions, once
  const int* skip = &g.ctl->skip;
  for (int k = 0; k < PC_SOLVES; k++) {
    CAP_TRY(cap_potrs_subst(1, n, nc, R, ldr, Inv, g.V, ldv, Y, ldv, S, ldv, ctr + (int64_t)(2 * k) * cw, nullptr, s, skip));
    CAP_TRY(cap_potrs_subst(0, n, nc, R, ldr, Inv, Y, ldv, g.V, ldv, S, ldv, ctr + (int64_t)(2 * k + 1) * cw, nullptr, s, skip));
    notes();
    hipLaunchKernelGGL(pocon_step_kernel, dim3((unsigned)nc), dim3(PC_T), 0, s, g);
    CAP_HIP(hipGetLastError());
  }
  notes();
  if (cap_acc_on()) {
    if (anorm) cap_acc_r(anorm, 0, 1, 1);
    cap_acc_w(out, 0, nc, 1);
    cap_acc_atomic(words, 4, 4);
  }
  hipLaunchKernelGGL(pocon_finish_kernel, dim3(1), dim3(64), 0, s, g);
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}

extern "C" int64_t cap_pocon_last_solves(void) {
  int* w = nullptr;
  if (cap_potrs_words(&w) != CAP_OK) return -1;
  int h[4] = {0, 0, 0, 0};
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(h, w, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return -1; }
  return h[2];
}
