// RAGGED block-tridiagonal chains (cap_blocktri_plan, cap_dpotrf_blocktri_vbatched, cap_dpotrs_blocktri_vbatched,
// cap_dpotri_blocktri_vbatched): the factor, the solve and the selected inverse of blocktri_batched.hip / blocktri_potri_batched.hip for a
// batch whose chains have DIFFERENT lengths T_c >= 0, one n <= 64 per call.  D and E are one sequence of n x n slots each; chain c owns
// slots first_c .. first_c + T_c - 1, slot first_c + i of E couples its positions i and i + 1 (the chain's last slot of E is never
// addressed), the right-hand sides are stacked as cap_dpotrs_vbatched stacks them.  ONE launch per call on a 1-D grid over the plan's list
// of the chains SORTED BY T DESCENDING (stable): a workgroup is one wavefront, its G = 64 / NP lane groups carry G neighbours of that list -
// chains of neighbouring lengths - and the longest chains start first.  No scratch, no allocation, no memset, no atomics, no helper
// stream, nothing between workgroups; 64-bit offsets.
//
// THE BIT CONTRACT: every chain gets, bit for bit, what the fixed-size entry writes for it alone (T = T_c, batch = 1) - D, E, solutions,
// info, logdet.  The arithmetic is the fixed-size kernels' statement by statement (pb_factor_step, pb_forward_step, pb_backward_step,
// pi_invert, pi_product_row, the MFMA recurrence from a zero accumulator with the uncontracted epilogues); a chain's tiles exist only
// inside its own lane group (bt_tile, and the group test of every tile accessor), so no number of one chain meets a number of another.
//
// THE BODIES (bt_factor, bt_solve, bt_inverse) are blocktri_kernels.h's, the very ones of the fixed-size entries; here the chain of a lane
// group comes from the plan (BtPlan): blockIdx.x -> the sorted list -> the chain's record, the G chains of the wavefront in an LDS table,
// the walk as long as the longest of them.  WHO IS ALIVE AT A STEP is told there: every chain starts at step 0, descending walks at its
// own last position, a chain is active while step < T_c, and SELECTION (never arithmetic) keeps an ended chain's stale numbers out of
// memory, info and logdet.  EVERY ADDRESS AND PREDICATE is a function of
// blocktri_addr.h, swept lane by lane on the CPU over ragged plans (tests/test_blocktri_ragged_addr.py).
#include <algorithm>
#include <new>
#include <vector>

#include "blocktri_kernels.h"

struct cap_blocktri_plan {
  int64_t batch = 0, slots = 0, eslots = 0, rows = 0, tmax = 0;
  int64_t nonempty = 0;                // chains with T > 0
  std::vector<BtRec> rec;              // host copies: the access notes and cap_blocktri_plan_order read them
  std::vector<int64_t> order;          // the chains by T descending, stable
  int device = -1;                     // -1: made in a process without a device - a description only, no entry runs on it
  BtRec* d_rec = nullptr;
  int64_t* d_order = nullptr;
};

namespace {

template <int NP>
__global__ __launch_bounds__(64) void blocktri_vpotrf_kernel(BtArgs<BtPlan> g) { bt_factor<NP>(g); }

template <int NP>
__global__ __launch_bounds__(64) void blocktri_vpotrs_kernel(BtSolveArgs<BtPlan> g) { bt_solve<NP>(g); }

template <int NP>
__global__ __launch_bounds__(64) void blocktri_vpotri_kernel(BtArgs<BtPlan> g) { bt_inverse<NP>(g); }

// rule 3 of the entries for D and E: each operand is one chain of the plan's slots (D has a leading dimension even where it has no slot)
bool bv_operands_ok(const cap_blocktri_plan* p, int64_t n, int64_t ldd, int64_t step_d, int64_t lde, int64_t step_e) {
  return bt_operand_ok(n, std::max<int64_t>(p->slots, 1), ldd, step_d, 0, 1) && bt_operand_ok(n, p->eslots, lde, step_e, 0, 1);
}

// the geometry and the plan on the device
template <class Args>
void bv_setup(Args& g, const cap_blocktri_plan* p, int64_t n, int64_t ldd, int64_t step_d, int64_t lde, int64_t step_e) {
  g.lk.rec = p->d_rec; g.lk.order = p->d_order; g.lk.count = p->batch;
  bt_geo(g.gd, n, 0, 0, ldd, step_d, 0);
  bt_geo(g.ge, n, 0, 0, lde, step_e, 0);
}

// the access notes of the plan and of the chains' blocks: mode_d / mode_e are CAP_ACC_R or CAP_ACC_RW
void bv_notes(const cap_blocktri_plan* p, const BtGeo& gd, const BtGeo& ge, const double* D, const double* E, int mode_d, int tri, int mode_e) {
  cap_acc_r(p->d_rec, 0, p->batch * (int64_t)(sizeof(BtRec) / 8), 1);
  cap_acc_r(p->d_order, 0, p->batch, 1);
  for (const BtRec& r : p->rec) bt_note_chain(gd, ge, bt_chain_plan(gd, ge, r.first, r.T, r.row, 0), D, E, mode_d, tri, mode_e);
}

// info / logdet: only the entries of the chains that have a position
void bv_note_scalars(const cap_blocktri_plan* p, const void* v, int mode, int elem) {
  for (int64_t c = 0; c < p->batch; c++)
    if (p->rec[(size_t)c].T > 0) cap_acc(mode, (const char*)v + c * elem, 0, 1, 1, 0, elem);
}

}  // namespace

extern "C" {

int cap_blocktri_plan_destroy(cap_blocktri_plan* p) {
  if (!p) return CAP_OK;
  if (p->d_rec) (void)hipFree(p->d_rec);
  if (p->d_order) (void)hipFree(p->d_order);
  delete p;
  return CAP_OK;
}

int cap_blocktri_plan_create(int64_t batch, const int64_t* T, const int64_t* first, cap_blocktri_plan** out) {
  if (!out) return CAP_ERR_ARG;
  *out = nullptr;
  if (batch < 0 || (batch > 0 && !T)) return CAP_ERR_ARG;
  for (int64_t c = 0; c < batch; c++)
    if (T[c] < 0 || (first && first[c] < 0)) return CAP_ERR_ARG;
  cap_blocktri_plan* p = new (std::nothrow) cap_blocktri_plan;
  if (!p) return CAP_ERR_ALLOC;
  p->batch = batch;
  p->rec.resize((size_t)batch);
  __int128 row = 0;
  bool over = false;
  std::vector<std::pair<int64_t, int64_t>> win;      // (first slot, one past the last) of every non-empty chain
  for (int64_t c = 0; c < batch; c++) {
    BtRec& r = p->rec[(size_t)c];
    r.T = T[c];
    r.first = first ? first[c] : (int64_t)row;
    r.row = (int64_t)row;
    row += r.T;
    over = over || row > (__int128)INT64_MAX || (__int128)r.first + r.T > (__int128)INT64_MAX;
    if (over) break;
    if (r.T == 0) continue;
    win.emplace_back(r.first, r.first + r.T);
    p->nonempty++;
    p->slots = std::max(p->slots, r.first + r.T);
    if (r.T > 1) p->eslots = std::max(p->eslots, r.first + r.T - 1);
    p->tmax = std::max(p->tmax, r.T);
  }
  if (!over) {
    std::sort(win.begin(), win.end());
    for (size_t k = 1; k < win.size(); k++)
      if (win[k].first < win[k - 1].second) { delete p; return CAP_ERR_ARG; }      // two chains' slot ranges meet
  }
  if (over) { delete p; return CAP_ERR_ARG; }
  p->rows = (int64_t)row;
  p->order.resize((size_t)batch);
  for (int64_t c = 0; c < batch; c++) p->order[(size_t)c] = c;
  std::stable_sort(p->order.begin(), p->order.end(), [&](int64_t a, int64_t b) { return p->rec[(size_t)a].T > p->rec[(size_t)b].T; });
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); *out = p; return CAP_OK; }
  if (hipGetDevice(&p->device) != hipSuccess) { (void)hipGetLastError(); delete p; return CAP_ERR_HIP; }
  if (batch > 0) {
    if (hipMalloc((void**)&p->d_rec, sizeof(BtRec) * (size_t)batch) != hipSuccess ||
        hipMalloc((void**)&p->d_order, sizeof(int64_t) * (size_t)batch) != hipSuccess ||
        hipMemcpy(p->d_rec, p->rec.data(), sizeof(BtRec) * (size_t)batch, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(p->d_order, p->order.data(), sizeof(int64_t) * (size_t)batch, hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipGetLastError();
      cap_blocktri_plan_destroy(p);
      return CAP_ERR_ALLOC;
    }
  }
  *out = p;
  return CAP_OK;
}

int64_t cap_blocktri_plan_info(const cap_blocktri_plan* p, int what) {
  if (!p) return -1;
  switch (what) {
    case CAP_BLOCKTRI_BATCH: return p->batch;
    case CAP_BLOCKTRI_SLOTS: return p->slots;
    case CAP_BLOCKTRI_ESLOTS: return p->eslots;
    case CAP_BLOCKTRI_ROWS: return p->rows;
    case CAP_BLOCKTRI_TMAX: return p->tmax;
    default: return -1;
  }
}

int cap_blocktri_plan_order(const cap_blocktri_plan* p, int64_t* chains, int64_t cap) {
  if (!p || cap < 0 || (cap > 0 && !chains)) return CAP_ERR_ARG;
  const int64_t m = std::min(cap, p->batch);
  for (int64_t k = 0; k < m; k++) chains[k] = p->order[(size_t)k];
  return CAP_OK;
}

int cap_dpotrf_blocktri_vbatched(const cap_blocktri_plan* p, int uplo, int64_t n, double* D, int64_t ldd, int64_t step_d, double* E, int64_t lde,
                                 int64_t step_e, int* info, double* logdet, void* stream) {
  if (!p || n < 0) return CAP_ERR_ARG;
  const bool work = n > 0 && p->nonempty > 0;
  if (work && (!D || !info || (!E && p->eslots > 0))) return CAP_ERR_ARG;
  if (!bv_operands_ok(p, n, ldd, step_d, lde, step_e)) return CAP_ERR_ARG;
  int st;
  const int64_t nwg = bt_limits(uplo, n, p->tmax, p->batch, st);
  if (st != CAP_OK) return st;
  if (!work) return CAP_OK;
  if (p->device < 0) return CAP_ERR_HIP;
  hipStream_t s = cap_stream(stream);
  BtArgs<BtPlan> g = {};
  g.D = D; g.E = E; g.info = info; g.logdet = logdet;
  bv_setup(g, p, n, ldd, step_d, lde, step_e);
  if (cap_acc_on()) {
    bv_notes(p, g.gd, g.ge, D, E, CAP_ACC_RW, 1, CAP_ACC_RW);
    bv_note_scalars(p, info, CAP_ACC_W, 4);
    if (logdet) bv_note_scalars(p, logdet, CAP_ACC_W, 8);
  }
  vb_with_int<8, 16, 32, 64>(g.gd.NP, [&](auto NP) { st = bt_launch<blocktri_vpotrf_kernel<NP()>, 0>(g, nwg, s); });
  return st;
}

int cap_dpotrs_blocktri_vbatched(const cap_blocktri_plan* p, int uplo, int half, int64_t n, int64_t nrhs, const double* D, int64_t ldd, int64_t step_d,
                                 const double* E, int64_t lde, int64_t step_e, double* B, int64_t ldb, const int* info, void* stream) {
  if (!p || n < 0 || nrhs < 0) return CAP_ERR_ARG;
  const bool work = n > 0 && nrhs > 0 && p->nonempty > 0;
  if (work && (!D || !B || (!E && p->eslots > 0))) return CAP_ERR_ARG;
  if (!bv_operands_ok(p, n, ldd, step_d, lde, step_e) || (__int128)ldb < (__int128)p->rows * n) return CAP_ERR_ARG;
  if (half < 0 || half > 2) return CAP_ERR_ARG;
  int st;
  const int64_t nwg = bt_limits(uplo, n, p->tmax, p->batch, st);
  if (st != CAP_OK) return st;
  if (!work) return CAP_OK;
  if (p->device < 0) return CAP_ERR_HIP;
  hipStream_t s = cap_stream(stream);
  BtSolveArgs<BtPlan> g = {};
  g.D = D; g.E = E; g.B = B; g.ldb = ldb; g.nrhs = nrhs; g.info = info; g.half = half;
  bv_setup(g, p, n, ldd, step_d, lde, step_e);
  if (cap_acc_on()) {
    bv_notes(p, g.gd, g.ge, D, E, CAP_ACC_R, 1, CAP_ACC_R);
    for (const BtRec& r : p->rec) cap_acc_rw(B + r.row * n, ldb, r.T * n, nrhs);
    if (info) bv_note_scalars(p, info, CAP_ACC_R, 4);
  }
  vb_with_int<8, 16, 32, 64>(g.gd.NP, [&](auto NP) { st = bt_launch<blocktri_vpotrs_kernel<NP()>, 0>(g, nwg, s); });
  return st;
}

int cap_dpotri_blocktri_vbatched(const cap_blocktri_plan* p, int uplo, int fill, int64_t n, double* D, int64_t ldd, int64_t step_d, double* E, int64_t lde,
                                 int64_t step_e, const int* info, void* stream) {
  if (!p || n < 0) return CAP_ERR_ARG;
  const bool work = n > 0 && p->nonempty > 0;
  if (work && (!D || (!E && p->eslots > 0))) return CAP_ERR_ARG;
  if (!bv_operands_ok(p, n, ldd, step_d, lde, step_e)) return CAP_ERR_ARG;
  if (fill != 0 && fill != 1) return CAP_ERR_ARG;
  int st;
  const int64_t nwg = bt_limits(uplo, n, p->tmax, p->batch, st);
  if (st != CAP_OK) return st;
  if (!work) return CAP_OK;
  if (p->device < 0) return CAP_ERR_HIP;
  hipStream_t s = cap_stream(stream);
  BtArgs<BtPlan> g = {};
  g.D = D; g.E = E; g.info = const_cast<int*>(info); g.fill = fill;
  bv_setup(g, p, n, ldd, step_d, lde, step_e);
  if (cap_acc_on()) {
    bv_notes(p, g.gd, g.ge, D, E, CAP_ACC_RW, fill ? 0 : 1, CAP_ACC_RW);
    if (info) bv_note_scalars(p, info, CAP_ACC_R, 4);
  }
  vb_with_int<8, 16, 32, 64>(g.gd.NP, [&](auto NP) { st = bt_launch<blocktri_vpotri_kernel<NP()>, (int)bt_inv_lds_bytes<NP(), BtPlan>()>(g, nwg, s); });
  return st;
}

}  // extern "C"
