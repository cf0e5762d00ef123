// One-launch triangular substitution for the fp64 Cholesky solve (cap_cholinv_solve / cap_dpotrs, cholinv.hip).
//
// A solve with R^T R = A is two substitutions with a few right-hand sides (nrhs <= 16): forward R^T Y = B, backward R X = Y.  Each
// is ONE launch here.  The triangle is cut into PT x PT blocks; the work items of a substitution, in "step" coordinates (the forward
// order; the backward launch maps step b to block nb - 1 - b), are
//   D_j      the diagonal step: Y_j = Dinv_j^T (B_j - S_j)    (backward: X_j = Dinv_j (Y_j - S_j)), then Y_j is published
//   T_{j,i}  the tile product P = R_{j,i}^T Y_j               (backward: R_{i,j} X_j), added to the partial sum S_i
// Workgroups claim items from a ticket counter in device memory in the order D_0, T_{0,1} .. T_{0,nb-1}, D_1, T_{1,2} .. and an item
// waits only on items with a LOWER ticket, which running workgroups already hold: no co-residency, no grid barrier.  A workgroup
// loads its tile before it waits, so the stream of R runs ahead of the dependency chain.  S_i is summed in order of j (T_{j,i} waits
// until T_{j-1,i} has added its part), so the result does not depend on timing and is the one the recovery launch computes.
// Hand-offs (cdna_hip_programming.md section 6, Guideline 16): the payload (Y_j, S_i) is stored with agent-scope atomic stores (write
// through), every storing wave drains its stores, the workgroup meets at a barrier, then ONE lane stores the flag / count with an
// agent-scope atomic store.  The consumer polls that word relaxed from one lane, takes an agent-scope acquire, and reads the payload with
// agent-scope loads.  Every spin is bounded; a workgroup that gives up (or the test hook) sets the state word and every workgroup leaves.
// The recovery launch behind it (one workgroup) returns at once when the word is clear; otherwise it redoes the whole substitution in
// ticket order without waiting - the input is untouched, the outputs are rewritten - and counts itself in the device's fallback word.
// Block width and arithmetic: PT = 128 so that the tile a workgroup loads ahead of its wait fits the LDS (129 KiB with padding); the
// products are fp64 VALU FMAs: at nrhs <= 16 a tile is 8 bytes of R per 2 nrhs flops, under 25 TF at the chip's full HBM rate, a third
// of the VALU rate, and the MFMA would pad every product to 16 right-hand sides.  Measured (profiles/r07_potrs.txt), the launch is
// bound by its chain of dependent steps (two hand-offs per 128 rows), not by the tile stream or the arithmetic.
#include <algorithm>
#include <mutex>

#include "common.h"

namespace {

constexpr int PT = 128;               // block width
constexpr int PTHREADS = 256;
constexpr int PLD = PT + 1;           // LDS leading dimension of the tile (odd: both read directions hit 64 distinct banks)
constexpr int PNR_MAX = 16;
constexpr int POTRS_POLLS = 1 << 21;  // ~ 1 us per poll: a workgroup gives up after seconds (an item it waits for takes microseconds)
constexpr size_t POTRS_LDS_BYTES = (size_t)(PT * PLD + PT * PNR_MAX + 4) * sizeof(double);

struct PotrsArgs {
  const double* R; int64_t ldr;       // upper triangle, only off-diagonal blocks are read
  const double* Inv;                  // the nb inverses of the diagonal blocks, PT x PT each (ld PT), zero below the diagonal
  const double* In; int64_t ldin;     // right-hand sides (not written by this launch)
  double* Out; int64_t ldout;         // solution of this substitution
  double* S; int64_t lds;             // partial sums, block b at rows b PT
  int* ctr;                           // [0] ticket, [1] state (1 = a workgroup gave up), [2, 2 + nb) published D_j, [2 + nb, 2 + 2 nb) parts in S_i
  int* words;                         // device-wide: [0] substitutions finished by the recovery launch, [1] injected give-ups pending,
                                      // [2] solves the last condition estimate took (pocon.hip)
  const int* info;                    // != 0 after the factor: the outputs are NaN
  const int* skip;                    // optional: != 0 turns this launch and its recovery launch into immediate exits
  int n, nrhs, nb, fwd, recover;
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
      if (++polls >= POTRS_POLLS || ((polls & 63) == 0 && ild(state) != 0)) { ok = false; break; }
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

// every storing wave drains its write-through stores, the workgroup meets, one lane publishes
__device__ __forceinline__ void publish(int* w, int v) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) ist(w, v);
}

// One work item.  j: step of the item, i: step of the block it produces (i == j: the diagonal step D_j).  wait = false in the
// recovery launch, which runs the items in ticket order by itself.  Returns false when a wait gave up.
template <int NR>
__device__ __forceinline__ bool potrs_item(const PotrsArgs& a, int j, int i, bool wait, bool nan_out, double* Mt, double* V, int* flag) {
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const bool diag = i == j, tr = a.fwd != 0;
  const int J = tr ? j : a.nb - 1 - j, I = tr ? i : a.nb - 1 - i;      // physical blocks: input vector J, output block I
  const int rb = diag ? J : min(I, J), cb = diag ? J : max(I, J);      // block row / column of the tile
  const int rv = min(PT, a.n - rb * PT), cv = min(PT, a.n - cb * PT);
  const int wj = min(PT, a.n - J * PT), wi = min(PT, a.n - I * PT);
  const double* M = diag ? a.Inv + (int64_t)J * PT * PT : a.R + (int64_t)rb * PT + (int64_t)cb * PT * a.ldr;
  const int64_t ldm = diag ? PT : a.ldr;
  int* const state = a.ctr + 1;
  int* const pub = a.ctr + 2;
  int* const parts = a.ctr + 2 + a.nb;

  // ---- the tile, before any wait: column c = wid + 4 q, rows lane and lane + 64 (512 contiguous bytes per wave load).  Every load is
  // issued (addresses clamped into the block, the value masked afterwards): a load under a condition is waited for one at a time
  {
    double r[2 * PT / 4];
#pragma unroll
    for (int q = 0; q < PT / 4; q++) {
      const int c = min(wid + 4 * q, cv - 1);
#pragma unroll
      for (int h = 0; h < 2; h++) r[2 * q + h] = M[min(lane + 64 * h, rv - 1) + (int64_t)c * ldm];
    }
#pragma unroll
    for (int q = 0; q < PT / 4; q++)
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int c = wid + 4 * q, k = lane + 64 * h;
        Mt[c * PLD + k] = (k < rv && c < cv) ? r[2 * q + h] : 0.0;
      }
  }

  // ---- the vector operand V (PT x NR): D_j reads In_J - S_J (S_J complete once all j parts are in; In_J is read before the wait),
  // T_{j,i} reads the published output of D_j.  Element e = t + 256 u of V: row e / NR, right-hand side e % NR.
  constexpr int EV = (PT * NR + PTHREADS - 1) / PTHREADS;
  double vin[EV];
  int64_t voff[EV];
#pragma unroll
  for (int u = 0; u < EV; u++) {
    const int e = min(t + PTHREADS * u, PT * NR - 1), sr = min(e / NR, wj - 1), rr = min(e % NR, a.nrhs - 1);
    voff[u] = (int64_t)J * PT + sr;
    vin[u] = diag ? a.In[voff[u] + (int64_t)rr * a.ldin] : 0.0;
    voff[u] += (int64_t)rr * (diag ? a.lds : a.ldout);
  }
  // T_{j,i}: the parts of S_i from T_{0,i} .. T_{j-1,i} (normally long in) are fetched before the wait for D_j
  const int o = t & (PT - 1), h = t >> 7;         // output element (a column of the tile if transposed, else a row), half of the sum
  double sold[NR];
  if (!diag && j > 0) {
    if (wait && !wait_geq(parts + i, j, state, flag)) return false;
#pragma unroll
    for (int r = 0; r < NR; r++) sold[r] = gld(a.S + (int64_t)I * PT + min(o, wi - 1) + (int64_t)min(r, a.nrhs - 1) * a.lds);
  }
  if (wait) {
    const bool ok = diag ? (j == 0 || wait_geq(parts + j, j, state, flag)) : wait_geq(pub + j, 1, state, flag);
    if (!ok) return false;
  }
  if (!diag || j > 0) {
    double w[EV];
#pragma unroll
    for (int u = 0; u < EV; u++) w[u] = gld((diag ? a.S : a.Out) + voff[u]);
#pragma unroll
    for (int u = 0; u < EV; u++) vin[u] = diag ? vin[u] - w[u] : w[u];
  }
#pragma unroll
  for (int u = 0; u < EV; u++) {
    const int e = t + PTHREADS * u;
    if (e < PT * NR) V[e] = ((e / NR) < wj && (e % NR) < a.nrhs) ? vin[u] : 0.0;
  }
  __syncthreads();

  // ---- the product: half h of the summation index per thread, the halves added in LDS
  double acc[NR];
#pragma unroll
  for (int r = 0; r < NR; r++) acc[r] = 0.0;
  for (int ss = 0; ss < PT / 2; ss++) {
    const int s = (PT / 2) * h + ss;
    const double m = tr ? Mt[o * PLD + s] : Mt[s * PLD + o];
#pragma unroll
    for (int r = 0; r < NR; r++) acc[r] = fma(m, V[s * NR + r], acc[r]);
  }
  __syncthreads();                          // the tile is read: its space takes the second half's sums
  if (h == 1) {
#pragma unroll
    for (int r = 0; r < NR; r++) Mt[o * NR + r] = acc[r];
  }
  __syncthreads();
  if (h == 0) {
#pragma unroll
    for (int r = 0; r < NR; r++) acc[r] += Mt[o * NR + r];
  }

  if (diag) {
    if (h == 0 && o < wi) {
#pragma unroll
      for (int r = 0; r < NR; r++)
        if (r < a.nrhs) gst(a.Out + (int64_t)I * PT + o + (int64_t)r * a.ldout, nan_out ? __builtin_nan("") : acc[r]);
    }
    publish(pub + j, 1);
  } else {
    // S_i += P in order of j (the parts of T_{0,i} .. T_{j-1,i} were fetched above)
    if (h == 0 && o < wi) {
#pragma unroll
      for (int r = 0; r < NR; r++)
        if (r < a.nrhs) gst(a.S + (int64_t)I * PT + o + (int64_t)r * a.lds, j == 0 ? acc[r] : sold[r] + acc[r]);
    }
    publish(parts + i, j + 1);
  }
  __syncthreads();                          // LDS is free for the next item
  return true;
}

template <int NR>
__global__ void __launch_bounds__(PTHREADS) potrs_subst_kernel(const PotrsArgs a) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* Mt = lds;
  double* V = lds + PT * PLD;
  int* sh = reinterpret_cast<int*>(V + PT * PNR_MAX);      // [0] ticket, [1] wait result
  const int t = threadIdx.x, nb = a.nb;
  int* const state = a.ctr + 1;
  // the skip word is written by a launch in front of this one, never during it: every thread reads the same value
  if (a.skip && *a.skip != 0) return;
  const bool nan_out = a.info && *a.info != 0;

  if (a.recover) {
    // one workgroup: nothing to do unless a workgroup of the launch in front gave up
    if (t == 0) sh[0] = ild(state);
    __syncthreads();
    if (sh[0] == 0) return;
    for (int j = 0; j < nb; j++)
      for (int i = j; i < nb; i++) (void)potrs_item<NR>(a, j, i, false, nan_out, Mt, V, sh + 1);
    if (t == 0) {
      ist(state, 0);
      if (a.words) atomicAdd(a.words, 1);
    }
    return;
  }

  const int total = nb * (nb + 1) / 2;
  int j = 0, jstart = 0;                      // step of the last ticket and the first ticket of that step (tickets only grow)
  for (;;) {
    if (t == 0) {
      int tk = -1;
      if (ild(state) == 0) {
        tk = __hip_atomic_fetch_add(a.ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // test hook: the substitution that hands out ticket 0 gives up at once while injections are pending
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
    if (!potrs_item<NR>(a, j, j + (tk - jstart), true, nan_out, Mt, V, sh + 1)) {
      if (t == 0) ist(state, 1);
      break;
    }
  }
}

// NaN into X when the factor reported a failing pivot (the blocked path; the one-launch path writes them itself)
__global__ void potrs_nan_kernel(double* X, int64_t ldx, int64_t n, int64_t nrhs, const int* info) {
  if (*info == 0) return;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n * nrhs) X[e % n + (e / n) * ldx] = __builtin_nan("");
}

std::mutex g_words_mu;
int* g_words[16] = {};

int solve_words(int** w) {
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
  cached[dev] = cus;                // one workgroup per CU: the tile takes most of the LDS
  return cus;
}

template <int NR>
int launch_subst(const PotrsArgs& g, int wgs, hipStream_t s) {
  CAP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(potrs_subst_kernel<NR>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)POTRS_LDS_BYTES));
  hipLaunchKernelGGL(potrs_subst_kernel<NR>, dim3((unsigned)wgs), dim3(PTHREADS), POTRS_LDS_BYTES, s, g);
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}

}  // namespace

int64_t cap_potrs_block() { return PT; }
int64_t cap_potrs_ctr_ints(int64_t n) { return cap_round_up(2 + 2 * cap_ceil_div(n, PT), 4); }

int cap_potrs_subst(int fwd, int64_t n, int64_t nrhs, const double* R, int64_t ldr, const double* Inv, const double* In, int64_t ldin,
                    double* Out, int64_t ldout, double* S, int64_t lds, int* ctr, const int* info, hipStream_t s, const int* skip) {
  if (n <= 0 || nrhs <= 0) return CAP_OK;
  if (nrhs > PNR_MAX || n > ((int64_t)1 << 24)) return CAP_ERR_ARG;
  int* words = nullptr;
  CAP_TRY(solve_words(&words));
  const int nb = (int)cap_ceil_div(n, PT);
  PotrsArgs g{R, ldr, Inv, In, ldin, Out, ldout, S, lds, ctr, words, info, skip, (int)n, (int)nrhs, nb, fwd, 0};
  const int items = nb * (nb + 1) / 2;
  const int wgs = std::max(1, std::min(items, resident_wgs()));
  // access notes: the off-diagonal blocks of R's upper triangle, the block inverses, the input, the output and the partial sums this
  // launch writes, its counter words (zeroed by the caller on this stream), the device's fallback / injection words and the pivot report
  auto note = [&]() {
    if (!cap_acc_on()) return;
    cap_acc_r(R, ldr, n, n, 1);
    cap_acc_r(Inv, 0, (int64_t)nb * PT * PT, 1);
    cap_acc_r(In, ldin, n, nrhs);
    cap_acc_rw(Out, ldout, n, nrhs);
    cap_acc_rw(S, lds, n, nrhs);
    cap_acc_rw(ctr, 0, cap_potrs_ctr_ints(n), 1, 0, 4);
    cap_acc_atomic(words, 4, 4);
    if (info) cap_acc_r(info, 1, 1, 1, 0, 4);
    if (skip) cap_acc_r(skip, 1, 1, 1, 0, 4);
  };
  for (int rec = 0; rec < 2; rec++) {
    g.recover = rec;
    note();
    const int w = rec ? 1 : wgs;
    if (nrhs <= 1) CAP_TRY(launch_subst<1>(g, w, s));
    else if (nrhs <= 2) CAP_TRY(launch_subst<2>(g, w, s));
    else if (nrhs <= 4) CAP_TRY(launch_subst<4>(g, w, s));
    else if (nrhs <= 8) CAP_TRY(launch_subst<8>(g, w, s));
    else CAP_TRY(launch_subst<16>(g, w, s));
  }
  return CAP_OK;
}

int cap_potrs_nan_fill(double* X, int64_t ldx, int64_t n, int64_t nrhs, const int* info, hipStream_t s) {
  if (!info || n <= 0 || nrhs <= 0) return CAP_OK;
  if (cap_acc_on()) { cap_acc_w(X, ldx, n, nrhs); cap_acc_r(info, 1, 1, 1, 0, 4); }
  const int64_t e = n * nrhs;
  hipLaunchKernelGGL(potrs_nan_kernel, dim3((unsigned)cap_ceil_div(e, 256)), dim3(256), 0, s, X, ldx, n, nrhs, info);
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}

int cap_potrs_words(int** w) { return solve_words(w); }

extern "C" int64_t cap_solve_fallbacks(void) {
  int* w = nullptr;
  if (solve_words(&w) != CAP_OK) return -1;
  int h[4] = {0, 0, 0, 0};
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(h, w, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return -1; }
  return h[0];
}

extern "C" int cap_solve_inject_timeouts(int count) {
  if (count < 0) return CAP_ERR_ARG;
  int* w = nullptr;
  CAP_TRY(solve_words(&w));
  CAP_HIP(hipDeviceSynchronize());
  CAP_HIP(hipMemcpy(w + 1, &count, sizeof(int), hipMemcpyHostToDevice));
  return CAP_OK;
}
