// What conv2d.hip (the forward) and conv2d_bwd.hip (the backward) of the dense 1x1 / 3x3 convolutions share: the launch arguments, the
// pixel operand's reader, the output pixel with the epilogue, and the two implicit-GEMM tiles (64 x 64 of mfma64.h; 16 output channels
// x 256 pixels below 64 rows), templated over the reader.  Orders of addition are part of each piece.
#pragma once
#include "head.h"

namespace ptx {

constexpr int kConvMaxImages = 64 * 64, kConvMaxSide = 32768;

// ---- 1x1 and 3x3: the 64 x 64 tile ------------------------------------------------------------------------------------------------------
struct ConvArgs {
    const float *x, *w, *scale, *shift, *residual; float *out;
    int C, Cout, H, W, Ho, Wo, stride, relu, K, vec;        // C: input channels; K = KS KS C; vec: 16-byte pixel requests (1x1)
    long total;                                             // N Ho Wo
};

// What the two tiles share.  A staging thread's four consecutive pixels of the flattened (image, y, x) index, each decoded on its own (a
// quad may span a row or an image), and their values at one k of the implicit GEMM: input channel k (1x1), or tap k / C of channel k % C
// (3x3; a tap outside the image is the padding: zero, never read).  Pixels behind the end and k >= K give zeros.
template <int KS>
struct ConvQuad {
    size_t base[4];                                         // 1x1: the pixel's element of channel 0; 3x3: the image's first element
    int iy0[4], ix0[4];                                     // 3x3: the tap (0,0) of the pixel's window
    bool have[4];
    __device__ __forceinline__ ConvQuad(const ConvArgs &a, long g_first)
    {
        const int HW = a.H * a.W, HoWo = a.Ho * a.Wo;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long g = g_first + q;
            have[q] = g < a.total;
            const long n = have[q] ? g / HoWo : 0;
            const int p = have[q] ? (int)(g - n * HoWo) : 0, oy = p / a.Wo, ox = p - oy * a.Wo;
            base[q] = (size_t)n * a.C * HW;
            if (KS == 1) base[q] += (size_t)(oy * a.stride) * a.W + ox * a.stride;
            iy0[q] = oy * a.stride - 1; ix0[q] = ox * a.stride - 1;
        }
    }
    __device__ __forceinline__ float4 load(const ConvArgs &a, int k) const
    {
        const int HW = a.H * a.W;
        float e[4] = {0.f, 0.f, 0.f, 0.f};
        if (k < a.K) {
            if (KS == 1) {
                if (a.vec) {                                // stride 1 on a map of a multiple of 4 pixels: the quad is 16 aligned bytes of one image
                    if (have[0]) {
                        const float4 v = ld4(a.x + base[0] + (size_t)k * HW);
                        e[0] = v.x; e[1] = v.y; e[2] = v.z; e[3] = v.w;
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (have[q]) e[q] = a.x[base[q] + (size_t)k * HW];
                }
            } else {
                const int tap = k / a.C, ci = k - tap * a.C, ty = tap / 3, tx = tap - 3 * ty;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int iy = iy0[q] + ty, ix = ix0[q] + tx;
                    if (have[q] && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) e[q] = a.x[base[q] + (size_t)ci * HW + (size_t)iy * a.W + ix];
                }
            }
        }
        return make_float4(e[0], e[1], e[2], e[3]);
    }
};

// An accumulator's pixel and the epilogue of both tiles: * scale, + shift (-ffp-contract=off: two roundings, like the restatement),
// + residual, ReLU that keeps a NaN.
struct ConvOutPixel {
    size_t first;                                           // element of output channel 0
    size_t plane;                                           // Ho Wo
    bool have;
    __device__ __forceinline__ ConvOutPixel(const ConvArgs &a, long g)
    {
        const int HoWo = a.Ho * a.Wo;
        have = g < a.total;
        const long n = have ? g / HoWo : 0;
        plane = (size_t)HoWo;
        first = (size_t)n * a.Cout * plane + (size_t)(have ? g - n * HoWo : 0);
    }
    __device__ __forceinline__ void store(const ConvArgs &a, int co, float v) const
    {
        const size_t at = first + (size_t)co * plane;
        if (a.scale) v = v * a.scale[co];
        if (a.shift) v = v + a.shift[co];
        if (a.residual) v = v + a.residual[at];
        if (a.relu) v = relu_nan(v);
        a.out[at] = v;
    }
};

// blockIdx = (pixel tile of 64, output-channel tile of 64).  Quad: the pixel operand's reader -- ConvQuad<KS> (the forward) or ConvQuadT<KS>
// (conv2d_bwd.hip: the data gradient)
template <class Quad>
__global__ __launch_bounds__(256) void k_conv_gemm(ConvArgs a)
{
    __shared__ __attribute__((aligned(16))) float As[2][64][LDT];       // [k / 32][output channel][k % 32]: the weight
    __shared__ __attribute__((aligned(16))) float Ws[2][64][LDT];       // [k / 32][pixel][k % 32]: the pixels, transposed
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1, li = lane & 31, hh = lane >> 5;
    const long g0 = (long)blockIdx.x * 64;
    const int co0 = blockIdx.y * 64;
    // staging.  Weight: thread (ar + 16 i, kq .. kq + 3).  Pixels: thread (k = wk + 16 i, pixels wn .. wn + 3), written transposed
    const int ar = tid >> 4, kq = (tid & 15) * 4;
    const int wk = lane & 15, wn = (wid * 4 + (lane >> 4)) * 4;
    const Quad px(a, g0 + wn);
    float4 av[4], wv[4];
    float tot[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) tot[i] = 0.0f;
    const int nsteps = (a.K + 63) >> 6;

    auto fetch = [&](int s) {
        const int c0 = s << 6;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = co0 + ar + 16 * i;
            wv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < a.Cout && c0 + kq < a.K) wv[i] = ld4(a.w + (size_t)row * a.K + c0 + kq);
            av[i] = px.load(a, c0 + wk + 16 * i);
        }
    };

    fetch(0);
    for (int s = 0; s < nsteps; ++s) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            st4(&As[kq >> 5][ar + 16 * i][kq & 31], wv[i]);
            stash_t4(Ws, wk + 16 * i, wn, av[i]);
        }
        __syncthreads();
        if (s + 1 < nsteps) fetch(s + 1);                   // in flight behind this step's matrix instructions
        PTX_SPARSE_STEP(tot, a.K - (s << 6) > 32);
        __syncthreads();
    }
    // C/D layout of the 32x32 MFMA: col = lane & 31 (the pixel), row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) (the output channel)
    const ConvOutPixel o(a, g0 + wc * 32 + li);
    if (!o.have) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = co0 + tile_row(r, wr, hh);
        if (co < a.Cout) o.store(a, co, tot[r]);
    }
}

// ---- 1x1 and 3x3 below 64 output channels: 16 output channels x 256 pixels ------------------------------------------------------------
// Layer1's and layer2's 16 / 32 planes (and 48): on the 64-row tile three quarters (half, a quarter) of every matrix instruction are
// zero rows.  Here a work-group owns 16 output channels x 256 pixels, wave w the pixels 64 w .. 64 w + 63 as four 16 x 16 accumulators
// of v_mfma_f32_16x16x4_f32 (A: lane l holds W[co = l & 15][k = l >> 4]; B: X[k = l >> 4][pixel = l & 15]; D register r: co = 4 (l >> 4)
// + r, pixel = l & 15).  Steps of 32 k.  The pixel operand stays k-major in LDS as it is in memory: thread (pixel quad = tid & 63,
// k = 8 (tid >> 6) + j) -- a wave reads 1 KiB of one channel at a time -- and a row pitch of 272 floats puts the four k of a fragment
// read on disjoint banks.  Blocked summation (a 32-wide step from zero, then added), ascending k; the epilogue of k_conv_gemm.
typedef float conv_f32x4 __attribute__((ext_vector_type(4)));
constexpr int kNarrowPx = 256, kNarrowPitch = kNarrowPx + 16;

// blockIdx = (pixel tile of 256, output-channel tile of 16)
template <class Quad>
__global__ __launch_bounds__(256) void k_conv_narrow(ConvArgs a)
{
    __shared__ __attribute__((aligned(16))) float Wa[16][LDT];                  // [output channel][k % 32]
    __shared__ __attribute__((aligned(16))) float Xs[32][kNarrowPitch];         // [k % 32][pixel]
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const long g0 = (long)blockIdx.x * kNarrowPx;
    const int co0 = blockIdx.y * 16;
    const int quad = lane * 4;                              // staging: this thread's four pixels, k = 8 wid + j
    const Quad px(a, g0 + quad);
    const int wrow = tid >> 3, wkq = (tid & 7) * 4;         // weight staging, threads 0 .. 127
    float4 av[8], wv = make_float4(0.f, 0.f, 0.f, 0.f);
    conv_f32x4 tot[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) tot[b] = conv_f32x4{0.f, 0.f, 0.f, 0.f};
    const int nsteps = (a.K + 31) >> 5;

    auto fetch = [&](int s) {
        const int c0 = s << 5;
        if (tid < 128) {
            wv = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c0 + wkq < a.K) wv = ld4(a.w + (size_t)(co0 + wrow) * a.K + c0 + wkq);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            av[j] = px.load(a, c0 + wid * 8 + j);
        }
    };

    fetch(0);
    const int fi = lane & 15, fk = lane >> 4;               // the fragments' row / column and k
    for (int s = 0; s < nsteps; ++s) {
        if (tid < 128) st4(&Wa[wrow][wkq], wv);
#pragma unroll
        for (int j = 0; j < 8; ++j) st4(&Xs[wid * 8 + j][quad], av[j]);
        __syncthreads();
        if (s + 1 < nsteps) fetch(s + 1);                   // in flight behind this step's matrix instructions
        const int nk = min(8, (a.K - (s << 5)) >> 2);       // K is a multiple of 16: whole groups of 4 k
        conv_f32x4 acc[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[b] = conv_f32x4{0.f, 0.f, 0.f, 0.f};
        for (int kk = 0; kk < nk; ++kk) {
            const float wa = Wa[fi][kk * 4 + fk];
#pragma unroll
            for (int b = 0; b < 4; ++b)
                acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa, Xs[kk * 4 + fk][wid * 64 + b * 16 + fi], acc[b], 0, 0, 0);
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) tot[b] += acc[b];
        __syncthreads();
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const ConvOutPixel o(a, g0 + wid * 64 + b * 16 + fi);
        if (!o.have) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) o.store(a, co0 + 4 * fk + r, tot[b][r]);
    }
}

}  // namespace ptx
