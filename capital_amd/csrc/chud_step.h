// The arithmetic of the rank-k update / downdate sweep that cholupdate.hip (one matrix of any size) and cholupdate_batched.hip (many blocks
// of up to 256 rows) share: the fixed-order dot product and the two row steps.  Both files run exactly these functions on a row, so a block
// gets the same bits from either - the recurrence is described at the head of cholupdate.hip.
#pragma once
#include <math.h>

#include "common.h"

namespace {

constexpr int UK_MAX = 16;            // columns of V per pass
constexpr int UH = UK_MAX + 4;        // doubles per row of a reflector block: w_r[0 .. 16), a, b, g, one unused

// sum_q x[q] y[q] in a fixed order: four interleaved partial sums (one for NK < 4), added pairwise
template <int NK>
__device__ __forceinline__ double dotk(const double* x, const double (&y)[NK]) {
  constexpr int P = NK >= 4 ? 4 : 1;
  double s[P];
#pragma unroll
  for (int p = 0; p < P; p++) s[p] = x[p] * y[p];
#pragma unroll
  for (int q = P; q < NK; q++) s[q % P] = fma(x[q], y[q], s[q % P]);
  if constexpr (P == 4) return (s[0] + s[1]) + (s[2] + s[3]);
  else return s[0];
}

// The diagonal row: from rr = R_rr and w = w_r the reflector of the row goes to hr (w_r, then a, b, g at UK_MAX ..); returns the new R_rr.
// fail: rho^2 is not a positive finite number - the row is NaN then.
template <int NK>
__device__ __forceinline__ double chud_reflector(const double (&w)[NK], double rr, double sigma, double* hr, bool& fail) {
  const double rho2 = fma(sigma, dotk<NK>(w, w), rr * rr);
  double rho = sqrt(rho2);
  fail = !(rho2 > 0.0) || !(rho2 <= 1.79769313486231570815e308);
  if (fail) rho = __builtin_nan("");
#pragma unroll
  for (int q = 0; q < NK; q++) hr[q] = w[q];
  hr[UK_MAX] = rr / rho; hr[UK_MAX + 1] = sigma / rho; hr[UK_MAX + 2] = 1.0 / (rr + rho);   // w_r = 0: a = 1 exactly, the row keeps its bits
  return rho;
}

// The reflector hr of row r applied to column c > r: x = R_rc, w = w_c (updated); returns R'_rc.
template <int NK>
__device__ __forceinline__ double chud_apply(const double* hr, double x, double (&w)[NK]) {
  const double y = fma(hr[UK_MAX], x, hr[UK_MAX + 1] * dotk<NK>(hr, w));
  const double s = (x + y) * hr[UK_MAX + 2];
#pragma unroll
  for (int q = 0; q < NK; q++) w[q] = fma(-hr[q], s, w[q]);
  return y;
}

}  // namespace
