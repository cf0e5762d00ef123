// The variable-size batch plan (cap_vbatch_plan, built by potrf_vbatched.hip) as the translation units that run on it see it:
// potrf_vbatched.hip (factor, solve, inverse) and cholupdate_batched.hip (update / downdate).
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/capital_amd.h"

constexpr int VB_CLASSES = 7;          // NP = 8, 16, 32, 64, then NBLK = 2, 3, 4

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

static inline int vb_per_group(int cls) { return cls == 0 ? 8 : cls == 1 ? 4 : cls == 2 ? 2 : 1; }      // blocks per workgroup
