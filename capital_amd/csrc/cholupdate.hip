// Rank-k update / downdate of the fp64 Cholesky factor (cap_dcholupdate / cap_cholinv_update, cholinv.hip): R'^T R' = R^T R + sigma V V^T.
//
// R (upper) is swept row by row with the working copy W = V^T (k x n).  At row r, with w_r = W[:, r]:
//   rho^2 = R_rr^2 + sigma |w_r|^2,  a = R_rr / rho,  b = sigma / rho,  g = 1 / (R_rr + rho)
//   for c > r:  R'_rc = a R_rc + b (w_r . w_c),   w_c -= w_r (R_rc + R'_rc) g,      then R_rr = rho
// sigma = +1: a Householder reflection on (R_rr; w_r).  sigma = -1: the hyperbolic reflection in its mixed form (the NEW R'_rc updates
// w_c), the numerically acceptable one for a downdate.  rho^2 <= 0 or not finite: A - V V^T is not positive definite; the 1-based row
// goes to `info` (first one wins) and the sweep carries on with NaN.  k > 16: consecutive passes of at most 16 columns of V.
//
// The sweep is cut into UT x UT tiles with two kinds of work item, in the shape of potrs.hip:
//   D_j      the diagonal tile R[j,j] (upper part) with W_j: its UT rows in order; publishes the reflector block of step j
//            (per row the k values of w_r and a, b, g)
//   T_{j,i}  i > j: tile R[j,i] with W_i: the UT reflections of step j; every column is a serial recurrence over the rows, the
//            columns are independent (one lane each).  Waits for D_j and for T_{j-1,i}: W_i receives the steps in order of j.
// A workgroup is ONE wavefront: 64 columns, the tile in LDS (43 KiB with the reflector block: three workgroups per CU).
// Two drivers run the same item code, so they give the same bits: stepwise (two launches per block row) and one-launch (workgroups
// claim items from a ticket counter in the order D_0, T_{0,1} .. T_{0,nb-1}, D_1, ..; an item waits only on LOWER tickets).
// Hand-offs as in potrs.hip (cdna_hip_programming.md section 6, Guideline 16): W_i and the reflector block are stored with agent-scope
// atomic stores, the wave drains them, a barrier, ONE lane stores the flag / count; the consumer polls relaxed from one lane, takes an
// agent-scope acquire and reads the payload with agent-scope loads.  The tiles of R are private to their item (plain loads / stores).
// Every spin is bounded.  Unlike the substitution this sweep is IN PLACE, so an item does all its waiting before its first store to
// global memory: after a give-up every item is either finished and counted (pub / parts) or untouched, and the recovery launch (one
// workgroup; returns at once when the state word is clear) finishes the remaining ones in ticket order from those counters.
// The first item that touches W_i (D_0 / T_{0,i}) reads the caller's V instead: no transposing copy, V is never written.
#include <algorithm>
#include <mutex>

#include "chud_step.h"   // dotk and the two row steps (UK_MAX, UH): shared with cholupdate_batched.hip
#include "common.h"

namespace {

constexpr int UT = 64;                // tile width = lanes of the one wavefront of a workgroup
constexpr int ULD = UT + 1;           // LDS leading dimension of the tile (odd: row-wise and column-wise reads hit distinct banks)
constexpr int CHUD_POLLS = 1 << 21;   // ~ 1 us per poll: a workgroup gives up after seconds (an item it waits for takes microseconds)
constexpr int CHUD_HDR = 4;           // counter words in front of pub / parts

struct ChudArgs {
  double* R; int64_t ldr;             // upper triangle, in place
  const double* V; int64_t ldv;       // the kp columns of this pass (never written)
  double* W; int64_t ldw;             // working copy: W[q ldw + c] = w_c[q]
  double* H;                          // reflector blocks: block j at H + j UT UH
  int* ctr;                           // [0] ticket, [1] state (1 = a workgroup gave up), [4, 4 + nb) published D_j, [4 + nb, 4 + 2 nb) steps applied to W_i
  int* words;                         // device-wide: [0] passes finished by the recovery launch, [1] injected give-ups pending
  int* info;                          // first failing row (1-based), may be NULL
  const int* skip;                    // != 0: the plan's factor had failed before this call - nothing is touched
  double sigma;
  int n, kp, nb, mode, j0;            // mode 0: one launch, 1: its recovery launch, 2: D_{j0} alone, 3: T_{j0, j0 + 1 + blockIdx.x}
};

__device__ __forceinline__ double gld(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void gst(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int ild(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void ist(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// one lane polls `w` until it reaches `target`, then the acquire; false: the spin expired or another workgroup gave up
__device__ __forceinline__ bool wait_geq(const int* w, int target, int* state, int* flag) {
  if (threadIdx.x == 0) {
    int polls = 0;
    bool ok = true;
    while (ild(w) < target) {
      __builtin_amdgcn_s_sleep(1);
      if (++polls >= CHUD_POLLS || ((polls & 63) == 0 && ild(state) != 0)) { ok = false; break; }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    *flag = ok;
  }
  __syncthreads();
  const bool ok = *flag != 0;
  __syncthreads();
  return ok;
}

// the storing wave drains its write-through stores, the workgroup meets, one lane publishes
__device__ __forceinline__ void publish(int* w, int v) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) ist(w, v);
}

// One work item.  j: block row, i: block column (i == j: the diagonal item D_j).  wait = false in the recovery launch and in the
// stepwise driver, whose order of launches is the order of the dependencies.  Returns false when a wait gave up (nothing stored yet).
template <int NK>
__device__ __forceinline__ bool chud_item(const ChudArgs& a, int j, int i, bool wait, double* Mt, double* Hs, int* flag) {
  const int c = threadIdx.x;                                     // row of the tile while it is moved, column while it is swept
  const bool diag = i == j;
  const int64_t r0 = (int64_t)j * UT, c0 = (int64_t)i * UT;
  const int rv = min(UT, a.n - (int)r0), cv = min(UT, a.n - (int)c0);   // rv == UT unless diag (a block row above another block is full)
  double* const T = a.R + r0 + c0 * a.ldr;
  int* const state = a.ctr + 1;
  int* const pub = a.ctr + CHUD_HDR;
  int* const parts = a.ctr + CHUD_HDR + a.nb;

  // ---- the tile, before any wait: lane = row, one column per load (512 contiguous bytes).  Every load is issued, its address clamped
  // into the tile - in D_j into the tile's UPPER part (row <= column) - and the value masked afterwards
  {
    double t[UT];
#pragma unroll
    for (int q = 0; q < UT; q++) {
      const int cc = min(q, cv - 1), rr = diag ? min(c, cc) : c;
      t[q] = T[rr + (int64_t)cc * a.ldr];
    }
#pragma unroll
    for (int q = 0; q < UT; q++) Mt[q * ULD + c] = (q < cv && c < rv && (!diag || c <= q)) ? t[q] : 0.0;
  }

  // ---- w_c: from V when this is the first item that touches W_i (read before the wait), else what T_{j-1,i} left
  const int64_t gc = c0 + min(c, cv - 1);
  double w[NK];
  if (j == 0) {
#pragma unroll
    for (int q = 0; q < NK; q++) w[q] = a.V[gc + (int64_t)min(q, a.kp - 1) * a.ldv];
  }
  if (wait) {
    if (j > 0 && !wait_geq(parts + i, j, state, flag)) return false;
    if (!diag && !wait_geq(pub + j, 1, state, flag)) return false;
  }
  if (j > 0) {
#pragma unroll
    for (int q = 0; q < NK; q++) w[q] = gld(a.W + gc + (int64_t)min(q, a.kp - 1) * a.ldw);
  }
#pragma unroll
  for (int q = 0; q < NK; q++)
    if (q >= a.kp || c >= cv) w[q] = 0.0;

  if (!diag) {
    // the reflector block of step j
    const double* Hj = a.H + (int64_t)j * UT * UH;
    double h[UH];
#pragma unroll
    for (int u = 0; u < UH; u++) h[u] = gld(Hj + c + UT * u);
#pragma unroll
    for (int u = 0; u < UH; u++) Hs[c + UT * u] = h[u];
  }
  __syncthreads();

  // ---- the sweep over the rows of the block: lane c owns column c of the tile and w_c
  double* const col = Mt + c * ULD;
  if (diag) {
    for (int r = 0; r < rv; r++) {
      if (c == r) {
        bool fail;
        const double rho = chud_reflector<NK>(w, col[r], a.sigma, Hs + r * UH, fail);
        if (fail && a.info) atomicCAS(a.info, 0, (int)r0 + r + 1);
        col[r] = rho;
      }
      __syncthreads();
      if (c > r) col[r] = chud_apply<NK>(Hs + r * UH, col[r], w);
    }
  } else {
    for (int r = 0; r < UT; r++) col[r] = chud_apply<NK>(Hs + r * UH, col[r], w);
  }
  __syncthreads();

  // ---- write back: the tile (D_j: its upper part), then the payload of the hand-off
  if (c < rv) {
#pragma unroll 8
    for (int q = 0; q < UT; q++)
      if (q < cv && (!diag || c <= q)) T[c + (int64_t)q * a.ldr] = Mt[q * ULD + c];
  }
  if (diag) {
    double* Hj = a.H + (int64_t)j * UT * UH;
#pragma unroll
    for (int u = 0; u < UH; u++) {
      const int e = c + UT * u, f = e % UH;           // the slots no row filled are published as zeros
      gst(Hj + e, (e / UH < rv && (f < NK || (f >= UK_MAX && f < UK_MAX + 3))) ? Hs[e] : 0.0);
    }
    publish(pub + j, 1);
  } else {
    if (c < cv) {
#pragma unroll
      for (int q = 0; q < NK; q++)
        if (q < a.kp) gst(a.W + c0 + c + (int64_t)q * a.ldw, w[q]);
    }
    publish(parts + i, j + 1);
  }
  __syncthreads();                          // LDS is free for the next item
  return true;
}

// the one-launch driver (mode 0) and its recovery launch (mode 1)
template <int NK>
__global__ void __launch_bounds__(UT) chud_sweep_kernel(const ChudArgs a) {
  __shared__ __attribute__((aligned(16))) double Mt[UT * ULD];
  __shared__ __attribute__((aligned(16))) double Hs[UT * UH];
  __shared__ int sh[2];                                       // [0] ticket, [1] wait result
  const int t = threadIdx.x, nb = a.nb;
  int* const state = a.ctr + 1;
  if (*a.skip != 0) return;

  if (a.mode == 1) {
    // one workgroup: nothing to do unless a workgroup of the launch in front gave up; then every item that is not counted yet
    if (t == 0) sh[0] = ild(state);
    __syncthreads();
    if (sh[0] == 0) return;
    for (int j = 0; j < nb; j++)
      for (int i = j; i < nb; i++) {
        if (t == 0) sh[0] = i == j ? ild(a.ctr + CHUD_HDR + j) >= 1 : ild(a.ctr + CHUD_HDR + nb + i) >= j + 1;
        __syncthreads();
        const bool done = sh[0] != 0;
        __syncthreads();
        if (!done) (void)chud_item<NK>(a, j, i, false, Mt, Hs, sh + 1);
      }
    if (t == 0) {
      ist(state, 0);
      if (a.words) atomicAdd(a.words, 1);
    }
    return;
  }

  const int total = nb * (nb + 1) / 2;
  int j = 0, jstart = 0;                      // block row of the last ticket and the first ticket of that row (tickets only grow)
  for (;;) {
    if (t == 0) {
      int tk = -1;
      if (ild(state) == 0) {
        tk = __hip_atomic_fetch_add(a.ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // test hook: the pass that hands out ticket 0 gives up at once while injections are pending
        if (tk == 0 && a.words && ild(a.words + 1) > 0) {
          atomicSub(a.words + 1, 1);
          ist(state, 1);
          tk = -1;
        }
      }
      sh[0] = tk;
    }
    __syncthreads();
    const int tk = sh[0];
    __syncthreads();
    if (tk < 0 || tk >= total) break;
    while (tk >= jstart + (nb - j)) { jstart += nb - j; j++; }
    if (!chud_item<NK>(a, j, j + (tk - jstart), true, Mt, Hs, sh + 1)) {
      if (t == 0) ist(state, 1);
      break;
    }
  }
}

// the stepwise driver: D_{j0} (mode 2, one workgroup) or all T_{j0, .} (mode 3)
template <int NK>
__global__ void __launch_bounds__(UT) chud_step_kernel(const ChudArgs a) {
  __shared__ __attribute__((aligned(16))) double Mt[UT * ULD];
  __shared__ __attribute__((aligned(16))) double Hs[UT * UH];
  __shared__ int sh[2];
  if (*a.skip != 0) return;
  (void)chud_item<NK>(a, a.j0, a.mode == 2 ? a.j0 : a.j0 + 1 + (int)blockIdx.x, false, Mt, Hs, sh + 1);
}

// skip = "the plan's factor had already failed" - taken once, in front of the passes (which write info themselves)
__global__ void chud_skip_kernel(const int* info, int* skip) { *skip = *info != 0; }

std::mutex g_words_mu;
int* g_words[16] = {};

int update_words(int** w) {
  int dev = 0;
  CAP_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= 16) return CAP_ERR_UNSUPPORTED;
  std::lock_guard<std::mutex> lk(g_words_mu);
  if (!g_words[dev]) {
    int* p = nullptr;
    CAP_HIP(hipMalloc((void**)&p, 4 * sizeof(int)));
    if (hipMemset(p, 0, 4 * sizeof(int)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
      (void)hipGetLastError(); (void)hipFree(p);
      return CAP_ERR_HIP;
    }
    g_words[dev] = p;
  }
  *w = g_words[dev];
  return CAP_OK;
}

int resident_wgs() {
  static int cached[16] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) { (void)hipGetLastError(); return 64; }
  if (cached[dev] > 0) return cached[dev];
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) { (void)hipGetLastError(); return 64; }
  cached[dev] = 3 * cus;            // three workgroups' LDS fit a CU
  return cached[dev];
}

template <int NK>
int launch_pass(ChudArgs g, bool one, hipStream_t s) {
  const int nb = g.nb;
  if (one) {
    const int items = nb * (nb + 1) / 2;
    g.mode = 0;
    hipLaunchKernelGGL(chud_sweep_kernel<NK>, dim3((unsigned)std::max(1, std::min(items, resident_wgs()))), dim3(UT), 0, s, g);
    CAP_HIP(hipGetLastError());
    g.mode = 1;
    cap_acc_none();                   // (the pass was noted once, in front of its first launch: cap_chud_run)
    hipLaunchKernelGGL(chud_sweep_kernel<NK>, dim3(1), dim3(UT), 0, s, g);
    CAP_HIP(hipGetLastError());
    return CAP_OK;
  }
  for (int j = 0; j < nb; j++) {
    g.j0 = j; g.mode = 2;
    if (j > 0) cap_acc_none();        // (the pass was noted once, in front of its first launch: cap_chud_run)
    hipLaunchKernelGGL(chud_step_kernel<NK>, dim3(1), dim3(UT), 0, s, g);
    CAP_HIP(hipGetLastError());
    if (j + 1 < nb) {
      g.mode = 3;
      cap_acc_none();
      hipLaunchKernelGGL(chud_step_kernel<NK>, dim3((unsigned)(nb - 1 - j)), dim3(UT), 0, s, g);
      CAP_HIP(hipGetLastError());
    }
  }
  return CAP_OK;
}

// work layout, in doubles: [skip word + counters (ints)][W: kp x ldw][H: nb reflector blocks]
int64_t chud_ldw(int64_t n) { return cap_round_up(n, UT); }
int64_t chud_ctr_doubles(int64_t n) { return cap_round_up(4 + CHUD_HDR + 2 * cap_ceil_div(n, UT), 4) / 2; }

}  // namespace

int64_t cap_chud_work_size(int64_t n, int64_t k) {
  if (n <= 0 || k <= 0) return 0;
  return chud_ctr_doubles(n) + std::min<int64_t>(k, UK_MAX) * chud_ldw(n) + cap_ceil_div(n, UT) * UT * UH;
}

// info_mode 0: `info` (may be NULL) is this call's own report, zeroed here.  1: `info` is the plan's report of its factor - a nonzero
// value leaves everything alone (decided on the device), a failing row of this call is written to it.
int cap_chud_run(int sign, int64_t n, int64_t k, double* R, int64_t ldr, const double* V, int64_t ldv, int* info, int info_mode,
                 double* work, int one, hipStream_t s) {
  if (n <= 0 || k <= 0) return CAP_OK;
  if (n > ((int64_t)1 << 21)) return CAP_ERR_ARG;         // nb (nb + 1) / 2 tickets in an int
  int* words = nullptr;
  CAP_TRY(update_words(&words));
  const int nb = (int)cap_ceil_div(n, UT);
  const int64_t cd = chud_ctr_doubles(n), ldw = chud_ldw(n), kp0 = std::min<int64_t>(k, UK_MAX);
  int* ints = reinterpret_cast<int*>(work);
  int* skip = ints;
  int* ctr = ints + 4;
  double* W = work + cd;
  double* H = W + kp0 * ldw;
  CAP_HIP(hipMemsetAsync(ints, 0, sizeof(double) * cd, s));
  if (info && info_mode == 0) CAP_HIP(hipMemsetAsync(info, 0, sizeof(int), s));
  if (info && info_mode == 1) {
    if (cap_acc_on()) { cap_acc_r(info, 1, 1, 1, 0, 4); cap_acc_w(skip, 1, 1, 1, 0, 4); }
    hipLaunchKernelGGL(chud_skip_kernel, dim3(1), dim3(1), 0, s, info, skip);
    CAP_HIP(hipGetLastError());
  }
  for (int64_t k0 = 0; k0 < k; k0 += UK_MAX) {
    const int kp = (int)std::min<int64_t>(UK_MAX, k - k0);
    if (k0 > 0) CAP_HIP(hipMemsetAsync(ctr, 0, sizeof(double) * cd - 4 * sizeof(int), s));
    ChudArgs g{R, ldr, V + k0 * ldv, ldv, W, ldw, H, ctr, words, info, skip, sign > 0 ? 1.0 : -1.0, (int)n, kp, nb, 0, 0};
    // access notes of the pass: R's upper triangle in place, the kp columns of V, the working copy and the reflector blocks, the
    // counter words, the device's fallback / injection words and the report
    if (cap_acc_on()) {
      cap_acc_rw(R, ldr, n, n, 1);
      cap_acc_r(V + k0 * ldv, ldv, n, kp);
      cap_acc_rw(W, ldw, n, kp);
      cap_acc_rw(H, 0, (int64_t)nb * UT * UH, 1);
      cap_acc_rw(ints, 0, 2 * cd, 1, 0, 4);
      cap_acc_atomic(words, 4, 4);
      if (info) cap_acc_atomic(info, 1, 4);
    }
    if (kp <= 1) CAP_TRY(launch_pass<1>(g, one != 0, s));
    else if (kp <= 2) CAP_TRY(launch_pass<2>(g, one != 0, s));
    else if (kp <= 4) CAP_TRY(launch_pass<4>(g, one != 0, s));
    else if (kp <= 8) CAP_TRY(launch_pass<8>(g, one != 0, s));
    else CAP_TRY(launch_pass<16>(g, one != 0, s));
  }
  return CAP_OK;
}

extern "C" int64_t cap_update_fallbacks(void) {
  int* w = nullptr;
  if (update_words(&w) != CAP_OK) return -1;
  int h[4] = {0, 0, 0, 0};
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(h, w, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return -1; }
  return h[0];
}

extern "C" int cap_update_inject_timeouts(int count) {
  if (count < 0) return CAP_ERR_ARG;
  int* w = nullptr;
  CAP_TRY(update_words(&w));
  CAP_HIP(hipDeviceSynchronize());
  CAP_HIP(hipMemcpy(w + 1, &count, sizeof(int), hipMemcpyHostToDevice));
  return CAP_OK;
}
