// What the batched fp64 family shares outside its arithmetic (the arithmetic: batched_small.h, batched_blocked.h, batched_inverse.h,
// chud_step.h).  HOST: the size classes, the clipped product, the one-1-D-grid limit, the runtime-value-to-template-argument dispatch and the
// operand rule of the fixed-size entry points - used by all eight translation units (potrf_batched.hip, potrf_batched_blocked.hip,
// potri_batched.hip, potrf_vbatched.hip, cholupdate_batched.hip, trsm_batched.hip, syrk_batched.hip, symm_batched.hip).  THE PLAN
// (cap_vbatch_plan, built by potrf_vbatched.hip) as the five translation units that run on it see it - potrf_vbatched.hip (factor, solve,
// inverse), cholupdate_batched.hip (update / downdate), trsm_batched.hip (solves and products), syrk_batched.hip (rank-k products),
// symm_batched.hip (symmetric products, norms, rcond, error bounds) - with the walk over
// its classes (vb_for_each_class) and, DEVICE, a lane group's block lookup (vb_group, vb_wave_max, vb_load_upper).
#pragma once
#include <stdint.h>

#include <type_traits>
#include <vector>

#include "common.h"

// ------------------------------------------------------------------------------------------------ host: sizes, grids, dispatch, operands
constexpr int VB_CLASSES = 7;          // NP = 8, 16, 32, 64, then NBLK = 2, 3, 4

// the size class of a block of n rows, the lanes of its group (n <= 64: the smallest NP >= n) and the blocks a workgroup of the class carries
static inline int vb_class(int64_t n) { return n <= 8 ? 0 : n <= 16 ? 1 : n <= 32 ? 2 : n <= 64 ? 3 : n <= 128 ? 4 : n <= 192 ? 5 : 6; }
static inline int vb_padded(int64_t n) { return n <= 64 ? 8 << vb_class(n) : 64; }
static inline int vb_per_group(int cls) { return cls < 4 ? 64 / (8 << cls) : 1; }

static inline int64_t vb_clip(__int128 v) { return v > (__int128)INT64_MAX ? INT64_MAX : (int64_t)v; }
static inline int64_t vb_mul_clip(int64_t a, int64_t b) { return vb_clip((__int128)a * b); }

// workgroups of `items` at `per` a workgroup, or -1 where one 1-D grid does not hold them
static inline int64_t vb_grid(int64_t items, int per) {
  const int64_t nwg = cap_ceil_div(items, per);
  return nwg > 0x7fffffffLL ? -1 : nwg;
}

// f(std::integral_constant<int, V>) for the V of the list that equals v (the last one where none does): a runtime value as a template argument
template <int V, int... Rest, class F>
void vb_with_int(int v, F&& f) {
  if constexpr (sizeof...(Rest) == 0) f(std::integral_constant<int, V>{});
  else if (v == V) f(std::integral_constant<int, V>{});
  else vb_with_int<Rest...>(v, f);
}

// the rule of a fixed-size operand: `batch` column-major blocks of rows x cols, leading dimension ld, `stride` elements apart, do not overlap
static inline bool vb_operand_ok(int64_t rows, int64_t cols, int64_t ld, int64_t stride, int64_t batch) {
  return ld >= rows && (batch <= 1 || stride >= vb_mul_clip(ld, cols));
}

// ------------------------------------------------------------------------------------------------ the plan
struct VbRec {                         // one block, in batch order
  int64_t off, ld, row;                // offset of the block, its leading dimension, its first row of the stacked right-hand sides
  int64_t n;
};

struct cap_vbatch_plan {
  int64_t batch = 0, total = 0, rows = 0, nmax = 0;
  int nonempty = 0;
  std::vector<VbRec> rec;                      // host copies: the access notes and cap_vbatch_plan_table read them
  std::vector<int64_t> list[VB_CLASSES];
  int device = -1;                             // -1: made in a process without a device - a description only, no entry runs on it
  VbRec* d_rec = nullptr;
  int64_t* d_list = nullptr;                   // the class lists back to back
  int64_t list_at[VB_CLASSES] = {0, 0, 0, 0, 0, 0, 0};
};

// The launches of one call on a plan: one per non-empty class, in class order.  f(cls, list, count, blocks, grid) - the class, its block
// indices on the device and their number, the same indices on the host, the grid - adds the access notes of its blocks and launches; the
// notes of the records and of the list are written here in front of them, and the launch is checked here.
template <class F>
int vb_for_each_class(const cap_vbatch_plan* p, F&& f) {
  for (int cls = 0; cls < VB_CLASSES; cls++) {
    const std::vector<int64_t>& l = p->list[cls];
    if (l.empty()) continue;
    const int64_t* list = p->d_list + p->list_at[cls];
    const int64_t count = (int64_t)l.size();
    cap_acc_r(p->d_rec, 0, p->batch * (int64_t)(sizeof(VbRec) / 8), 1);
    cap_acc_r(list, 0, count, 1);
    f(cls, list, count, l, dim3((unsigned)cap_ceil_div(count, vb_per_group(cls))));
    CAP_HIP(hipGetLastError());
  }
  return CAP_OK;
}

// ------------------------------------------------------------------------------------------------ device: a lane group finds its block
// what a lane group of a wave-per-blocks kernel works on: its block (n = 0: none) and the largest n of its wave
struct VbGroup {
  int64_t blk, off, ld, row;
  int n, nmax;
};

// the largest m of the wave, in a scalar register
__device__ __forceinline__ int vb_wave_max(int m) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int t = __shfl_xor(m, o);
    m = t > m ? t : m;
  }
  return __builtin_amdgcn_readfirstlane(m);
}

// the block of this lane's group of NP lanes (blockIdx.x -> class list -> record) and the wave's largest n; a dead group (the tail of a
// class) has n = 0: every predicate on n is false for it
template <int NP>
__device__ __forceinline__ VbGroup vb_group(const VbRec* rec, const int64_t* list, int64_t count) {
  constexpr int G = 64 / NP;
  const int64_t at = (int64_t)blockIdx.x * G + threadIdx.x / NP;
  VbGroup v;
  v.blk = 0; v.off = 0; v.ld = 1; v.row = 0; v.n = 0;
  if (at < count) {
    v.blk = list[at];
    const VbRec r = rec[v.blk];
    v.off = r.off; v.ld = r.ld; v.row = r.row; v.n = (int)r.n;
  }
  int m = v.n;                         // vb_wave_max written out: through the call the compiler schedules the factor and inverse kernels differently
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int t = __shfl_xor(m, o);
    m = t > m ? t : m;
  }
  v.nmax = __builtin_amdgcn_readfirstlane(m);
  return v;
}

// upper triangle of the group's n x n block -> its image Img (PbImg<NP>, PiImg<NP>): the fixed-size load with the group's own n as a lane
// predicate; lane r of the group walks along row r, so a column is contiguous
template <class Img>
__device__ __forceinline__ void vb_load_upper(const double* M, int64_t ld, int n, int nmax, int r, double* s) {
#pragma unroll 8
  for (int c = 0; c < nmax; c++)
    if (r <= c && c < n) s[Img::at(r, c)] = M[r + (int64_t)c * ld];
}
