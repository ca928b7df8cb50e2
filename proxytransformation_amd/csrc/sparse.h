// Shared between sparse.hip (forward) and sparse_bwd.hip (backward): the gather-GEMM kernel lives in sparse.hip, the backward launches
// its transposed-weight instantiation through this one function.
#pragma once
#include "common.h"

namespace ptx {

// dfeats (n_in, Cin) = sum_j gz[nbr_t[:, j]] @ weight[j]^T with weight (kvol, Cin, Cout); Cin and Cout multiples of 64; nbr_t entries
// outside [0, n_out) count as absent.  One launch on st.
int sparse_conv_transposed(const float *gz, int n_out, const int32_t *nbr_t, int n_in, int kvol, const float *weight, int Cin, int Cout,
                           float *dfeats, hipStream_t st);

}  // namespace ptx
