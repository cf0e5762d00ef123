// Batched rank-k update / downdate of fp64 Cholesky factors (cap_dcholupdate_batched, cap_dcholupdate_vbatched): for every block
// R_i'^T R_i' = R_i^T R_i + sigma V_i V_i^T in place on the upper factor, 1 <= n <= 256, V_i n x k (never written).  The batched member of
// cholupdate.hip, in the shape of the batched factor: ONE launch per call (per non-empty size class on a plan) on a 1-D grid,
// no scratch, no memset, no atomics, nothing between workgroups.
//
// THE ARITHMETIC is the row recurrence at the head of cholupdate.hip, through the functions of chud_step.h that file runs too: a block gets
// the bits cap_dcholupdate gives for it alone.  k > 16: consecutive passes of at most 16 columns of V inside the launch, each a complete
// sweep; a pass of kp columns runs the instance NK = 1 / 2 / 4 / 8 / 16 >= kp with zero padding, as cap_chud_run chooses it.  A kernel is
// templated on NKL, the NK of the LAST pass; every pass in front of it has 16 columns.
//
// n <= 64: ONE WAVEFRONT PER 64 / NP BLOCKS (NP = 8 / 16 / 32 / 64, the smallest one >= n; lane groups of NP lanes; one wave per workgroup,
// so __syncthreads orders the wave's own LDS accesses).  Lane c of a group owns column c of its block - in the group's LDS image, leading
// dimension NP + 1 (odd, as ULD in cholupdate.hip) - and w_c (NK doubles in registers) for the whole pass.  The upper triangle is loaded
// once, swept row by row for every pass and stored once; V is read once, a row per lane.  At row r lane r forms the reflector (w_r, a, b, g)
// into the group's LDS slot (two slots, by the parity of r: one barrier per row), the lanes c > r apply it.
// 64 < n <= 256: ONE WORKGROUP OF FOUR WAVES PER BLOCK, lane c (0 .. 255) owns column c and w_c in registers for the whole pass; no W
// travels through memory.  The block is taken in strips of 64 rows: wave j - the owner of the strip's diagonal columns - loads the diagonal
// 64 x 64 tile into the LDS image, sweeps it (the D item of cholupdate.hip, wave-level synchronisation only), stores it and leaves the
// strip's reflector block (64 rows of UH doubles, 10 KiB) in LDS; after one workgroup barrier every lane with a column right of the tile
// applies the 64 reflections to its column of the strip (the T item: a serial recurrence per column), 16 rows at a time between registers and
// the block's own memory (L2).  STAGING: only the diagonal tile (32.5 KiB) and the reflector block are in LDS, 43 KiB per workgroup, so three
// workgroups fit a CU; a staged 64-row strip of 256 columns (128 KiB) would leave one.  A column of the strip is touched by its own lane
// alone, 16 contiguous doubles per step, so LDS would add a round trip and two barriers per strip and save nothing.
//
// info (may be NULL) is input and output: a block with info != 0 on entry is not touched; otherwise the first failing row (1-based) is
// written with a plain store - a block has one owner and its rows go in order - and the sweep carries on with NaN.
// Variable sizes: the group's own n is the lane predicate while the wave loops to its largest n (vb_wave_max of vbatch_plan.h, taken after
// the info word); no lane of a block reads another block's data, so a block's bits do not depend on its neighbours.
// SHARED (vbatch_plan.h): the argument rules, the grid and the dispatch of the entry points and the walk over a plan's classes.
// chud_vbatched_kernel keeps vb_group's lookup written out: through the shared function its instances compile to other machine code.
#include "chud_step.h"
#include "vbatch_plan.h"

namespace {

constexpr int CB_MAX = 256;
constexpr int CB_SMALL = 64;
constexpr int CB_T = 64;              // rows of a strip, lanes of a wave
constexpr int CB_LD = CB_T + 1;       // leading dimension of the diagonal tile's image
constexpr int CB_RC = 16;             // rows a lane holds at a time while it applies a strip's reflections

struct CbArgs {                        // fixed size
  double* R; int64_t ldr, stride_r;
  const double* V; int64_t ldv, stride_v;
  int64_t batch, k;
  int* info;
  double sigma;
  int n;
};

struct CvArgs {                        // one class of a plan
  const VbRec* rec;
  const int64_t* list; int64_t count;
  double* R;
  const double* V; int64_t ldv, k;
  int* info;
  double sigma;
};

// orders one wave's LDS stores before its later LDS loads of other lanes' data (a wave's LDS instructions execute in order)
__device__ __forceinline__ void cb_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ------------------------------------------------------------------------------------------------ n <= 64: a wavefront per 64 / NP blocks
// one pass of kp <= NK columns over the group's image; nmax: the largest n of the wave (uniform), n: the group's own (0: nothing to do)
template <int NP, int NK>
__device__ __forceinline__ void cb_small_pass(double* img, double* hs, int* first, int* info, const double* V, int64_t ldv, int kp, int n,
                                              int nmax, int c, double sigma) {
  constexpr int LD = NP + 1;
  double w[NK];
#pragma unroll
  for (int q = 0; q < NK; q++) {
    double t = 0.0;
    if (q < kp && c < n) t = V[c + (int64_t)q * ldv];
    w[q] = t;
  }
  double* const col = img + c * LD;
  for (int r = 0; r < nmax; r++) {
    double* const hr = hs + (r & 1) * UH;
    if (c == r && r < n) {
      bool fail;
      const double rho = chud_reflector<NK>(w, col[r], sigma, hr, fail);
      if (fail && *first == 0) {
        *first = r + 1;
        if (info) *info = r + 1;
      }
      col[r] = rho;
    }
    __syncthreads();
    if (c > r && c < n) col[r] = chud_apply<NK>(hr, col[r], w);
  }
}

// the whole call for one lane group: R, V, info are the group's own block, n = 0 for a group without one
template <int NP, int NKL>
__device__ __forceinline__ void cb_small(double* R, int64_t ldr, const double* V, int64_t ldv, int n, int* info, double sigma, int64_t k) {
  constexpr int G = 64 / NP, LD = NP + 1;
  __shared__ double s_img[G * NP * LD];
  __shared__ double s_h[G * 2 * UH];
  __shared__ int s_first[G];
  const int lane = threadIdx.x, grp = lane / NP, c = lane % NP;
  double* const img = s_img + grp * NP * LD;

  if (n > 0 && info && *info != 0) n = 0;          // a block that had failed before this call: every predicate below is false for it
  const int nmax = vb_wave_max(n);
  if (nmax == 0) return;
  if (c == 0) s_first[grp] = 0;

  // upper triangle -> image; lane r walks along row r, so a column is contiguous
#pragma unroll 8
  for (int cc = 0; cc < nmax; cc++)
    if (c <= cc && cc < n) img[cc * LD + c] = R[c + (int64_t)cc * ldr];
  __syncthreads();

  for (int64_t k0 = 0; k0 < k; k0 += UK_MAX) {
    const int kp = (int)(k - k0 < UK_MAX ? k - k0 : UK_MAX);
    const double* Vp = V + k0 * ldv;
    if constexpr (NKL == UK_MAX) {
      cb_small_pass<NP, UK_MAX>(img, s_h + grp * 2 * UH, s_first + grp, info, Vp, ldv, kp, n, nmax, c, sigma);
    } else {
      if (kp == UK_MAX) cb_small_pass<NP, UK_MAX>(img, s_h + grp * 2 * UH, s_first + grp, info, Vp, ldv, kp, n, nmax, c, sigma);
      else cb_small_pass<NP, NKL>(img, s_h + grp * 2 * UH, s_first + grp, info, Vp, ldv, kp, n, nmax, c, sigma);
    }
    __syncthreads();
  }

#pragma unroll 8
  for (int cc = 0; cc < nmax; cc++)
    if (c <= cc && cc < n) R[c + (int64_t)cc * ldr] = img[cc * LD + c];
}

template <int NP, int NKL>
__global__ __launch_bounds__(64) void chud_batched_kernel(CbArgs g) {
  constexpr int G = 64 / NP;
  const int64_t blk = (int64_t)blockIdx.x * G + threadIdx.x / NP;
  const bool live = blk < g.batch;
  const int64_t at = live ? blk : 0;
  cb_small<NP, NKL>(g.R + at * g.stride_r, g.ldr, g.V + at * g.stride_v, g.ldv, live ? g.n : 0, g.info ? g.info + at : nullptr, g.sigma, g.k);
}

template <int NP, int NKL>
__global__ __launch_bounds__(64) void chud_vbatched_kernel(CvArgs g) {
  constexpr int G = 64 / NP;
  const int64_t at = (int64_t)blockIdx.x * G + threadIdx.x / NP;
  int64_t blk = 0, off = 0, ld = 1, row = 0;       // vb_group's lookup; cb_small takes the wave's largest n itself, after the info word
  int n = 0;
  if (at < g.count) {
    blk = g.list[at];
    const VbRec r = g.rec[blk];
    off = r.off; ld = r.ld; row = r.row; n = (int)r.n;
  }
  cb_small<NP, NKL>(g.R + off, ld, g.V + row, g.ldv, n, g.info ? g.info + blk : nullptr, g.sigma, g.k);
}

// ------------------------------------------------------------------------------------------------ 64 < n <= 256: a workgroup per block
template <int NK>
__device__ __forceinline__ void cb_blocked_pass(double* R, int64_t ldr, const double* V, int64_t ldv, int kp, int n, int* info, double sigma,
                                                double* s_img, double* s_h, int* s_first) {
  const int c = threadIdx.x, lane = c & 63, wave = c >> 6;
  double w[NK];
#pragma unroll
  for (int q = 0; q < NK; q++) {
    double t = 0.0;
    if (q < kp && c < n) t = V[c + (int64_t)q * ldv];
    w[q] = t;
  }
  const int nb = (n + CB_T - 1) / CB_T;
  for (int j = 0; j < nb; j++) {
    const int r0 = j * CB_T;
    const int rv = n - r0 < CB_T ? n - r0 : CB_T;
    if (wave == j) {
      // D_j: the diagonal tile's upper part -> image (lane = row), the sweep (lane = column), back
      double* const D = R + r0 + (int64_t)r0 * ldr;
#pragma unroll 8
      for (int cc = 0; cc < rv; cc++)
        if (lane <= cc) s_img[cc * CB_LD + lane] = D[lane + (int64_t)cc * ldr];
      cb_wave_sync();
      double* const col = s_img + lane * CB_LD;
      for (int r = 0; r < rv; r++) {
        double* const hr = s_h + r * UH;
        if (lane == r) {
          bool fail;
          const double rho = chud_reflector<NK>(w, col[r], sigma, hr, fail);
          if (fail && *s_first == 0) {
            *s_first = r0 + r + 1;
            if (info) *info = r0 + r + 1;
          }
          col[r] = rho;
        }
        cb_wave_sync();
        if (lane > r && lane < rv) col[r] = chud_apply<NK>(hr, col[r], w);
      }
      cb_wave_sync();
#pragma unroll 8
      for (int cc = 0; cc < rv; cc++)
        if (lane <= cc) D[lane + (int64_t)cc * ldr] = s_img[cc * CB_LD + lane];
    }
    __syncthreads();
    // T_{j, .}: the 64 reflections on every column right of the tile (a full strip: rv == 64 whenever such a column exists)
    if (c >= r0 + CB_T && c < n) {
      double* const P = R + r0 + (int64_t)c * ldr;
      for (int rb = 0; rb < CB_T; rb += CB_RC) {
        double x[CB_RC];
#pragma unroll
        for (int u = 0; u < CB_RC; u++) x[u] = P[rb + u];
#pragma unroll
        for (int u = 0; u < CB_RC; u++) x[u] = chud_apply<NK>(s_h + (rb + u) * UH, x[u], w);
#pragma unroll
        for (int u = 0; u < CB_RC; u++) P[rb + u] = x[u];
      }
    }
    __syncthreads();                     // the reflector block is free for the next strip
  }
}

template <int NKL>
__device__ __forceinline__ void cb_blocked(double* R, int64_t ldr, const double* V, int64_t ldv, int n, int* info, double sigma, int64_t k) {
  __shared__ double s_img[CB_T * CB_LD];
  __shared__ double s_h[CB_T * UH];
  __shared__ int s_word[2];              // [0] the first failing row of this call, [1] the block had failed before it
  if (threadIdx.x == 0) {
    s_word[0] = 0;
    s_word[1] = info ? *info != 0 : 0;
  }
  __syncthreads();
  if (s_word[1] != 0) return;
  for (int64_t k0 = 0; k0 < k; k0 += UK_MAX) {
    const int kp = (int)(k - k0 < UK_MAX ? k - k0 : UK_MAX);
    const double* Vp = V + k0 * ldv;
    if constexpr (NKL == UK_MAX) {
      cb_blocked_pass<UK_MAX>(R, ldr, Vp, ldv, kp, n, info, sigma, s_img, s_h, s_word);
    } else {
      if (kp == UK_MAX) cb_blocked_pass<UK_MAX>(R, ldr, Vp, ldv, kp, n, info, sigma, s_img, s_h, s_word);
      else cb_blocked_pass<NKL>(R, ldr, Vp, ldv, kp, n, info, sigma, s_img, s_h, s_word);
    }
  }
}

template <int NKL>
__global__ __launch_bounds__(256) void chud_batched_blocked_kernel(CbArgs g) {
  const int64_t blk = blockIdx.x;
  cb_blocked<NKL>(g.R + blk * g.stride_r, g.ldr, g.V + blk * g.stride_v, g.ldv, g.n, g.info ? g.info + blk : nullptr, g.sigma, g.k);
}

template <int NKL>
__global__ __launch_bounds__(256) void chud_vbatched_blocked_kernel(CvArgs g) {
  const int64_t blk = g.list[blockIdx.x];
  const VbRec r = g.rec[blk];
  cb_blocked<NKL>(g.R + r.off, r.ld, g.V + r.row, g.ldv, (int)r.n, g.info ? g.info + blk : nullptr, g.sigma, g.k);
}

// ------------------------------------------------------------------------------------------------ host
// NK of the last pass: the smallest of 1, 2, 4, 8, 16 >= its column count (cap_chud_run's choice)
int cb_last_nk(int64_t k) {
  const int kp = (int)((k - 1) % UK_MAX) + 1;
  return kp <= 1 ? 1 : kp <= 2 ? 2 : kp <= 4 ? 4 : kp <= 8 ? 8 : 16;
}

// f(NP, NK) with the group size and the last pass's NK as template arguments
template <class F>
void cb_with(int np, int nk, F f) {
  vb_with_int<8, 16, 32, 64>(np, [&](auto NP) { vb_with_int<1, 2, 4, 8, 16>(nk, [&](auto NK) { f(NP, NK); }); });
}

}  // namespace

extern "C" {

int cap_dcholupdate_batched(int uplo, int sign, int64_t n, int64_t k, double* R, int64_t ldr, int64_t stride_r, const double* V, int64_t ldv,
                            int64_t stride_v, int64_t batch, int* info, void* stream) {
  if ((sign != 1 && sign != -1) || n < 0 || k < 0 || batch < 0) return CAP_ERR_ARG;
  if (n > 0 && k > 0 && batch > 0) {
    if (!R || !V || !vb_operand_ok(n, n, ldr, stride_r, batch) || !vb_operand_ok(n, k, ldv, stride_v, batch)) return CAP_ERR_ARG;
  }
  if (uplo != CAP_UPPER) return CAP_ERR_UNSUPPORTED;    // as cap_dpotrf_batched
  if (n > CB_MAX) return CAP_ERR_UNSUPPORTED;
  const int64_t nwg = vb_grid(batch, vb_per_group(vb_class(n)));
  if (n > CB_SMALL && nwg < 0) return CAP_ERR_UNSUPPORTED;     // a workgroup per block: refused in front of the empty case
  if (n == 0 || k == 0 || batch == 0) return CAP_OK;
  if (nwg < 0) return CAP_ERR_UNSUPPORTED;
  const int nkl = cb_last_nk(k);
  hipStream_t s = cap_stream(stream);
  if (cap_acc_on()) {
    for (int64_t i = 0; i < batch; i++) {
      cap_acc_rw(R + i * stride_r, ldr, n, n, 1);
      cap_acc_r(V + i * stride_v, ldv, n, k);
    }
    if (info) cap_acc_rw(info, 0, batch, 1, 0, 4);
  }
  CbArgs g;
  g.R = R; g.ldr = ldr; g.stride_r = stride_r; g.V = V; g.ldv = ldv; g.stride_v = stride_v; g.batch = batch; g.k = k; g.info = info;
  g.sigma = sign > 0 ? 1.0 : -1.0; g.n = (int)n;
  const dim3 grid((unsigned)nwg);
  if (n <= CB_SMALL) {
    cb_with(vb_padded(n), nkl, [&](auto NP, auto NK) { hipLaunchKernelGGL((chud_batched_kernel<NP(), NK()>), grid, dim3(64), 0, s, g); });
  } else {
    vb_with_int<1, 2, 4, 8, 16>(nkl, [&](auto NK) { hipLaunchKernelGGL((chud_batched_blocked_kernel<NK()>), grid, dim3(256), 0, s, g); });
  }
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}

int cap_dcholupdate_vbatched(const cap_vbatch_plan* p, int uplo, int sign, int64_t k, double* R, const double* V, int64_t ldv, int* info,
                             void* stream) {
  if (!p || (sign != 1 && sign != -1) || k < 0) return CAP_ERR_ARG;
  if (p->nonempty > 0 && k > 0 && (!R || !V)) return CAP_ERR_ARG;
  if (ldv < p->rows) return CAP_ERR_ARG;
  if (uplo != CAP_UPPER) return CAP_ERR_UNSUPPORTED;
  if (p->nonempty == 0 || k == 0) return CAP_OK;
  if (p->device < 0) return CAP_ERR_HIP;
  hipStream_t s = cap_stream(stream);
  const int nkl = cb_last_nk(k);
  CvArgs g;
  g.rec = p->d_rec; g.R = R; g.V = V; g.ldv = ldv; g.k = k; g.info = info; g.sigma = sign > 0 ? 1.0 : -1.0;
  return vb_for_each_class(p, [&](int cls, const int64_t* list, int64_t count, const std::vector<int64_t>& blocks, dim3 grid) {
    g.list = list;
    g.count = count;
    if (cap_acc_on()) {
      for (int64_t b : blocks) {
        const VbRec& r = p->rec[(size_t)b];
        cap_acc_rw(R + r.off, r.ld, r.n, r.n, 1);
        cap_acc_r(V + r.row, ldv, r.n, k);
        if (info) cap_acc_rw(info + b, 0, 1, 1, 0, 4);
      }
    }
    if (cls < 4) {
      cb_with(8 << cls, nkl, [&](auto NP, auto NK) { hipLaunchKernelGGL((chud_vbatched_kernel<NP(), NK()>), grid, dim3(64), 0, s, g); });
    } else {
      vb_with_int<1, 2, 4, 8, 16>(nkl, [&](auto NK) { hipLaunchKernelGGL((chud_vbatched_blocked_kernel<NK()>), grid, dim3(256), 0, s, g); });
    }
  });
}

}  // extern "C"
