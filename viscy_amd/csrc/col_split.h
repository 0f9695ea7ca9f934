// viscy_amd — the row split of the float64 column passes (pca_moment_kernel of pca.hip, lr_wcolsum_kernel of logreg.hip): a
// workgroup of CM_COLS x CM_LANES threads owns CM_COLS columns and one run of rows, writes its partial to a workspace row of its
// own, and a fold kernel adds the runs in ascending order.
#pragma once
#include "vsx_common.h"

#define CM_COLS 64           // columns per workgroup (one wave wide: coalesced along d)
#define CM_LANES 4           // row lanes per column
#define CM_MIN_ROWS 512      // rows per workgroup at least
#define CM_WANT_WGS 2048

// row splits of equal length, at least CM_MIN_ROWS rows each, about CM_WANT_WGS workgroups
static inline void cm_split(int64_t n, int d, int* splits, int64_t* rps) {
  const int64_t groups = (d + CM_COLS - 1) / CM_COLS;
  int64_t want = (CM_WANT_WGS + groups - 1) / groups;
  const int64_t most = (n + CM_MIN_ROWS - 1) / CM_MIN_ROWS;
  if (want > most) want = most;
  *rps = (n + want - 1) / want;
  *splits = (int)((n + *rps - 1) / *rps);
}

// out[col] = the splits' partials part[split][col] in ascending order, divided by div where div > 0.  grid ceil(d / 256)
static __global__ __launch_bounds__(256) void cm_fold_kernel(const double* __restrict__ part, int splits, int d, double div,
                                                             double* __restrict__ out) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= d) return;
  double tot = 0.0;
  for (int s = 0; s < splits; ++s) tot += part[(size_t)s * d + col];
  out[col] = div > 0.0 ? tot / div : tot;
}
