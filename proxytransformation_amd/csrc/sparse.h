// What sparse.hip (kernel maps, convolution, max-pool), sparse_bwd.hip (their backward) and sparse_norm.hip (the norms) share: the
// streaming idiom of the row kernels, the staging and the blocked step of the two matrix-core kernels, the entry points' argument checks.
#pragma once
#include <initializer_list>

#include "common.h"
#include "mfma64.h"

namespace ptx {

constexpr int kSpMaxVol = 27;              // kernel_size <= 3
constexpr int kSpMaxCin = 1024;            // input channels of the neck's layers (ptx_sparse_conv3d_act, ptx_sparse_conv_transpose_gen)
// The streaming idiom of the row kernels: a 256-thread work-group owns a tile of kSpTile rows x 64 columns, thread = (row slot =
// tid >> 4, 4 channels = tid & 15), 16-byte accesses; column sums go through LDS as [16 slots][64 columns], slots added in ascending order.
constexpr int kSpTile = 256;

__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void st4(float *p, float4 v) { *reinterpret_cast<float4 *>(p) = v; }
// Component-wise arithmetic, one rounding per operation.  The value forms and the in-place forms are not interchangeable at will: which one
// a kernel uses decides how the compiler lays its loop out (profiles/sparse_refactor.txt), the bits are the same either way.
__device__ __forceinline__ float4 add4(float4 a, float4 b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; return a; }
__device__ __forceinline__ float4 sub4(float4 a, float4 b) { a.x -= b.x; a.y -= b.y; a.z -= b.z; a.w -= b.w; return a; }
__device__ __forceinline__ float4 mul4(float4 a, float4 b) { a.x *= b.x; a.y *= b.y; a.z *= b.z; a.w *= b.w; return a; }
__device__ __forceinline__ void acc4(float4 &sum, float4 v) { sum.x += v.x; sum.y += v.y; sum.z += v.z; sum.w += v.w; }                // sum += v
__device__ __forceinline__ void scale4(float4 &a, float4 b) { a.x *= b.x; a.y *= b.y; a.z *= b.z; a.w *= b.w; }                        // a *= b
__device__ __forceinline__ void mac4(float4 &sum, float4 a, float4 b) { sum.x += a.x * b.x; sum.y += a.y * b.y; sum.z += a.z * b.z; sum.w += a.w * b.w; }
// d *= [o > 0]: the gradient behind a ReLU whose result was o
__device__ __forceinline__ void relu_mask4(float4 &d, const float4 &o)
{
    d.x = o.x > 0.0f ? d.x : 0.0f; d.y = o.y > 0.0f ? d.y : 0.0f; d.z = o.z > 0.0f ? d.z : 0.0f; d.w = o.w > 0.0f ? d.w : 0.0f;
}
// the 16 row slots of s_red[.][tid] in ascending order (tid < 64)
__device__ __forceinline__ float slots16(const float (*s_red)[64], int tid)
{
    float v = s_red[0][tid];
#pragma unroll
    for (int s = 1; s < 16; ++s) v += s_red[s][tid];
    return v;
}

// Staging of k_sparse_conv's weight slab and of both operands of k_sparse_dweight: thread (k, n .. n + 3) writes its four values
// transposed into T[k / 32][n + q][k % 32] as four dwords -- with k = (lane & 15) + 16 i and n = 4 (4 wid + (lane >> 4)) the 32 lanes of a
// write group hold 16 k x 2 n-quads, banks k + 16 (quad & 1): conflict-free
__device__ __forceinline__ void stash_t4(float (*T)[64][LDT], int k, int n, float4 v)
{
    T[k >> 5][n + 0][k & 31] = v.x;
    T[k >> 5][n + 1][k & 31] = v.y;
    T[k >> 5][n + 2][k & 31] = v.z;
    T[k >> 5][n + 3][k & 31] = v.w;
}

}  // namespace ptx

// Blocked summation of the two matrix-core kernels: the staged panel's product (32 k, or 64 with second_; work-group uniform) is formed
// from zero and then added to the tile's running sum tot_[16].  Scope: PTX_G64_COMPUTE's (mfma64.h)
#define PTX_SPARSE_STEP(tot_, second_)                                       \
    do {                                                                     \
        f32x16 acc;                                                          \
        _Pragma("unroll") for (int i = 0; i < 16; ++i) acc[i] = 0.0f;        \
        PTX_G64_COMPUTE(0);                                                  \
        if (second_) PTX_G64_COMPUTE(1);                                     \
        _Pragma("unroll") for (int i = 0; i < 16; ++i) tot_[i] += acc[i];    \
    } while (0)

namespace ptx {

// ---- host: the entry points' argument checks ------------------------------------------------------------------------------------------
inline bool sp_aligned16(std::initializer_list<const void *> ptrs)
{
    uintptr_t bits = 0;
    for (const void *p : ptrs) bits |= reinterpret_cast<uintptr_t>(p);
    return (bits & 15) == 0;
}
// a channel count the 64-column kernels take: a multiple of 64 up to 512
inline bool sp_width_ok(int C) { return C >= 64 && C <= 512 && C % 64 == 0; }
inline int sp_workspace_fits(const char *who, size_t have, size_t need)
{
    if (have >= need) return PTX_OK;
    set_error("%s: workspace too small: %zu < %zu bytes", who, have, need);
    return PTX_ENOSPACE;
}
// one thread per (row, 4 channels) in work-groups of 256: the grid must fit
inline int sp_rows_fit(const char *who, int rows, int C)
{
    PTX_REQUIRE((long)rows * (C / 4) < (1l << 31) * 256, "%s: %d rows x %d channels is out of range", who, rows, C);
    return PTX_OK;
}

// dfeats (n_in, Cin) = sum_j gz[nbr_t[:, j]] @ weight[j]^T with weight (kvol, Cin, Cout); Cin and Cout multiples of 64; nbr_t entries
// outside [0, n_out) count as absent; nbr_t null with kvol = 8: the generative map nbr_t[i, j] = 8 i + j.  One launch on st: the gather-GEMM kernel lives in sparse.hip, the backward launches its
// transposed-weight instantiation through this one function.
int sparse_conv_transposed(const float *gz, int n_out, const int32_t *nbr_t, int n_in, int kvol, const float *weight, int Cin, int Cout,
                           float *dfeats, hipStream_t st);

}  // namespace ptx
