// The exact-fp32 matrix-core step of the 64x64 output tile (k_gemm64 of gemm.hip, k_sparse_conv of sparse.hip): a 4-wave work-group,
// wave (wr, wc) owns one 32x32 accumulator; both operands lie in LDS with k contiguous, As[buf][row][k] and Ws[buf][col][k].
#pragma once
#include "common.h"
#include "split3.h"

namespace ptx {

constexpr int BK = 32, LDT = BK + 4;   // 144-B LDS rows: 16-B aligned, b128 fragment reads conflict-free

// one BK-wide step of a wave's 32 x 32 accumulator from LDS buffer `buf`: A[buf][arow][k], W[buf][wrow][k], hh = lane >> 5.
// C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) (head.h: tile_row)
__device__ __forceinline__ void g64_step(const float (*A)[64][LDT], const float (*W)[64][LDT], int buf, int arow, int wrow, int hh, f32x16 &acc)
{
#pragma unroll
    for (int kk = 0; kk < BK / 8; ++kk) {
        const float4 a4 = *reinterpret_cast<const float4 *>(&A[buf][arow][kk * 8 + hh * 4]);
        const float4 b4 = *reinterpret_cast<const float4 *>(&W[buf][wrow][kk * 8 + hh * 4]);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b4.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b4.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b4.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b4.w, acc, 0, 0, 0);
    }
}

}  // namespace ptx

// The same step as a macro over As, Ws, acc, wr, wc, li, hh in scope, for gemm.hip, sparse.hip and sparse_bwd.hip: expressed through
// g64_step, k_sparse_conv and k_sparse_dweight compile to other instructions (profiles/head_refactor.txt), so the macro stays.
#define PTX_G64_COMPUTE(buf_)                                                              \
    do {                                                                                   \
        _Pragma("unroll") for (int kk = 0; kk < BK / 8; ++kk) {                            \
            const float4 a4 = *reinterpret_cast<const float4 *>(&As[buf_][wr * 32 + li][kk * 8 + hh * 4]); \
            const float4 b4 = *reinterpret_cast<const float4 *>(&Ws[buf_][wc * 32 + li][kk * 8 + hh * 4]); \
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b4.x, acc, 0, 0, 0);          \
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b4.y, acc, 0, 0, 0);          \
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b4.z, acc, 0, 0, 0);          \
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b4.w, acc, 0, 0, 0);          \
        }                                                                                  \
    } while (0)
