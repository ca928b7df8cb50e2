// The dense 2D convolutions of the image backbone (mmdet.ResNet, Bottleneck depths, every BatchNorm frozen): NCHW fp32 activations,
// three entry points.
//
//   ptx_conv_stem   7x7 stride 2 pad 3 convolution 3 -> C0, * scale + shift, ReLU and the 3x3 stride 2 pad 1 max-pool in ONE launch: a
//       work-group owns a tile of kStemTH x kStemTW pooled pixels of one image, stages the 31 x 71 x 3 input pixels it needs in LDS (uint8 or
//       float, (x - mean) / std applied there, zeros outside the image AFTER the normalisation), forms the 13 x 33 convolution outputs
//       behind them 16 channels at a time in plain FMA (K = 147: one LDS read feeds 16 FMAs whose weights arrive through the scalar
//       cache; the matrix pipe has nothing to add) and pools them out of LDS.  The half-resolution map is never written.
//   ptx_conv1x1 / ptx_conv3x3   implicit GEMM on the exact-fp32 matrix instruction, mfma64.h's 64 x 64 tile: rows = output channels (the
//       weight, k contiguous), columns = 64 pixels of the flattened (image, y, x) index -- a tile may span an image boundary, every
//       pixel is decoded on its own --, k = input channel (1x1) or (tap, input channel) (3x3, K = 9 C, no im2col buffer).  The pixel
//       operand is read along x (16-byte requests where the stride is 1 and the map a multiple of 4 pixels) and written transposed
//       into LDS (sparse.h: stash_t4).  Blocked summation (a 64-wide step from zero, then added: k_sparse_conv's order); the epilogue is
//       k_sparse_conv's too: * scale + shift (two roundings), + residual, ReLU -- which keeps a NaN, as torch's does.
//       Below 64 output channels (layer1's and layer2's 16 / 32 planes) the tile is 16 output channels x 256 pixels on
//       v_mfma_f32_16x16x4_f32 (k_conv_narrow): the 64-row tile would spend most of each matrix instruction on zero rows.
//
// fp32, no float atomics, a fixed k order: an image's bits do not depend on the batch or on its place in it.  Everything on the caller's
// stream, no host wait.  Held to the numpy restatement of proxytransformation_amd/image_backbone_host.py.
#include "conv2d.h"

namespace ptx {

constexpr int kStemTH = 6, kStemTW = 16;                                  // pooled pixels per work-group
constexpr int kStemCH = 2 * kStemTH + 1, kStemCW = 2 * kStemTW + 1;       // 13 x 33 convolution outputs behind them
constexpr int kStemIH = 2 * (kStemCH - 1) + 7, kStemIW = 2 * (kStemCW - 1) + 7;   // 31 x 71 input pixels behind those
constexpr int kStemCG = 16;                                               // output channels per pass

__device__ __forceinline__ float stem_pixel(const float *p) { return *p; }
__device__ __forceinline__ float stem_pixel(const uint8_t *p) { return (float)*p; }

// blockIdx = (pooled tile x, pooled tile y, image)
template <typename T>
__global__ __launch_bounds__(256) void k_conv_stem(const T *__restrict__ x, const float *__restrict__ w, const float *__restrict__ scale,
                                                   const float *__restrict__ shift, const float *__restrict__ mean,
                                                   const float *__restrict__ stdv, float *__restrict__ out, int H, int W, int h1, int w1,
                                                   int h2, int w2, int C0, int relu)
{
    __shared__ float s_in[3][kStemIH][kStemIW];
    __shared__ float s_cv[kStemCG][kStemCH * kStemCW];
    const int tid = threadIdx.x, n = blockIdx.z;
    const int py0 = blockIdx.y * kStemTH, px0 = blockIdx.x * kStemTW;
    const int cy0 = 2 * py0 - 1, cx0 = 2 * px0 - 1;         // the tile's first convolution output
    const int iy0 = 2 * cy0 - 3, ix0 = 2 * cx0 - 3;         // and its first input pixel
    for (int e = tid; e < 3 * kStemIH * kStemIW; e += 256) {
        const int c = e / (kStemIH * kStemIW), r = e - c * (kStemIH * kStemIW), y = r / kStemIW, xx = r - y * kStemIW;
        const int gy = iy0 + y, gx = ix0 + xx;
        float v = 0.0f;                                     // the padding: zero behind the normalisation
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            v = stem_pixel(x + (((size_t)n * 3 + c) * H + gy) * W + gx);
            if (mean) v = (v - mean[c]) / stdv[c];
        }
        s_in[c][y][xx] = v;
    }
    __syncthreads();
    for (int ch0 = 0; ch0 < C0; ch0 += kStemCG) {
        for (int pos = tid; pos < kStemCH * kStemCW; pos += 256) {
            const int cy = pos / kStemCW, cx = pos - cy * kStemCW;
            float acc[kStemCG];
#pragma unroll
            for (int j = 0; j < kStemCG; ++j) acc[j] = 0.0f;
            for (int c = 0; c < 3; ++c) {
#pragma unroll
                for (int ky = 0; ky < 7; ++ky) {
#pragma unroll
                    for (int kx = 0; kx < 7; ++kx) {
                        const float v = s_in[c][2 * cy + ky][2 * cx + kx];
                        const float *wr = w + (size_t)((c * 7 + ky) * 7 + kx) * C0 + ch0;      // work-group uniform
#pragma unroll
                        for (int j = 0; j < kStemCG; ++j) acc[j] = fmaf(v, wr[j], acc[j]);
                    }
                }
            }
            const bool inside = cy0 + cy >= 0 && cy0 + cy < h1 && cx0 + cx >= 0 && cx0 + cx < w1;
#pragma unroll
            for (int j = 0; j < kStemCG; ++j) {
                float v = acc[j];
                if (scale) v = v * scale[ch0 + j];
                if (shift) v = v + shift[ch0 + j];
                if (relu) v = relu_nan(v);
                s_cv[j][pos] = inside ? v : -INFINITY;      // the pool's padding
            }
        }
        __syncthreads();
        for (int e = tid; e < kStemCG * kStemTH * kStemTW; e += 256) {
            const int j = e / (kStemTH * kStemTW), r = e - j * (kStemTH * kStemTW), py = r / kStemTW, px = r - py * kStemTW;
            if (py0 + py >= h2 || px0 + px >= w2) continue;
            float m = -INFINITY;                            // torch's running maximum: a NaN replaces it and stays
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const float v = s_cv[j][(2 * py + dy) * kStemCW + 2 * px + dx];
                    if (v > m || v != v) m = v;
                }
            out[(((size_t)n * C0 + ch0 + j) * h2 + py0 + py) * w2 + px0 + px] = m;
        }
        __syncthreads();
    }
}

static int conv_launch(const char *who, int KS, const float *x, int N, int C, int H, int W, const float *weight, int Cout, int stride,
                       const float *scale, const float *shift, const float *residual, int relu, float *out, void *stream)
{
    PTX_REQUIRE(N >= 1 && N <= kConvMaxImages && H >= 1 && H <= kConvMaxSide && W >= 1 && W <= kConvMaxSide,
                "%s: N=%d H=%d W=%d (N: 1 to %d images; H, W: 1 to %d)", who, N, H, W, kConvMaxImages, kConvMaxSide);
    PTX_REQUIRE(stride == 1 || stride == 2, "%s: stride=%d (1 or 2)", who, stride);
    PTX_REQUIRE(relu == 0 || relu == 1, "%s: relu=%d (0 or 1)", who, relu);
    PTX_REQUIRE(x && weight && out, "%s: null argument", who);
    PTX_REQUIRE(x != out && residual != x, "%s: out must not be x (it may be residual), and residual must not be x", who);
    PTX_REQUIRE(sp_aligned16({x, weight}), "%s: x and weight must be 16-byte aligned", who);
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    PTX_REQUIRE((long)H * W < (1l << 30) && (long)Ho * Wo * N < (1l << 31) * 64, "%s: N=%d H=%d W=%d is out of range", who, N, H, W);
    ConvArgs a{};
    a.x = x; a.w = weight; a.scale = scale; a.shift = shift; a.residual = residual; a.out = out;
    a.C = C; a.Cout = Cout; a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo; a.stride = stride; a.relu = relu; a.K = KS * KS * C;
    a.total = (long)N * Ho * Wo;
    a.vec = KS == 1 && stride == 1 && (H * W) % 4 == 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // 16, 32, 48 output channels: the 16-wide tile -- except the strided 3x3 beyond 16 channels, where every 16-channel tile repeats the
    // scattered window reads and the 64-row tile measured faster (at 32 planes, 300 images of 120 x 120: 755 us, profiles/image_backbone.txt,
    // against 988 us for the 16-wide tile in a run that is not recorded there)
    if (Cout < 64 && !(KS == 3 && stride == 2 && Cout > 16)) {
        const dim3 grid((unsigned)((a.total + kNarrowPx - 1) / kNarrowPx), (unsigned)(Cout / 16));
        if (KS == 1) hipLaunchKernelGGL((k_conv_narrow<ConvQuad<1>>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((k_conv_narrow<ConvQuad<3>>), grid, dim3(256), 0, st, a);
        PTX_LAUNCHED(KS == 1 ? "k_conv_narrow<1>" : "k_conv_narrow<3>");
        return PTX_OK;
    }
    const dim3 grid((unsigned)((a.total + 63) / 64), (unsigned)cdiv(Cout, 64));
    if (KS == 1) hipLaunchKernelGGL((k_conv_gemm<ConvQuad<1>>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_conv_gemm<ConvQuad<3>>), grid, dim3(256), 0, st, a);
    PTX_LAUNCHED(KS == 1 ? "k_conv_gemm<1>" : "k_conv_gemm<3>");
    return PTX_OK;
}

}  // namespace ptx

using namespace ptx;

extern "C" {

int ptx_conv_stem(const void *x, int x_dtype, int N, int H, int W, const float *weight, int C0, const float *scale, const float *shift,
                  int relu, const float *mean, const float *std, float *out, void *stream)
{
    const char *who = "ptx_conv_stem";
    PTX_REQUIRE(x_dtype == 0 || x_dtype == 1, "%s: x_dtype=%d (0 float32, 1 uint8)", who, x_dtype);
    PTX_REQUIRE(N >= 1 && N <= kConvMaxImages && H >= 32 && H <= 2048 && W >= 32 && W <= 2048,
                "%s: N=%d H=%d W=%d (N: 1 to %d images; H, W: 32 to 2048)", who, N, H, W, kConvMaxImages);
    PTX_REQUIRE(C0 >= 16 && C0 <= 64 && C0 % 16 == 0, "%s: C0=%d (a multiple of 16 from 16 to 64)", who, C0);
    PTX_REQUIRE(relu == 0 || relu == 1, "%s: relu=%d (0 or 1)", who, relu);
    PTX_REQUIRE(x && weight && out, "%s: null argument", who);
    PTX_REQUIRE((mean == nullptr) == (std == nullptr), "%s: mean and std go together", who);
    PTX_REQUIRE(x_dtype == 1 || (reinterpret_cast<uintptr_t>(x) & 3) == 0, "%s: a float32 x must be 4-byte aligned", who);
    PTX_REQUIRE(sp_aligned16({weight}), "%s: weight must be 16-byte aligned", who);
    const int h1 = (H - 1) / 2 + 1, w1 = (W - 1) / 2 + 1, h2 = (h1 - 1) / 2 + 1, w2 = (w1 - 1) / 2 + 1;
    const dim3 grid(cdiv(w2, kStemTW), cdiv(h2, kStemTH), N);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (x_dtype == 0)
        hipLaunchKernelGGL((k_conv_stem<float>), grid, dim3(256), 0, st, static_cast<const float *>(x), weight, scale, shift, mean, std, out, H,
                           W, h1, w1, h2, w2, C0, relu);
    else
        hipLaunchKernelGGL((k_conv_stem<uint8_t>), grid, dim3(256), 0, st, static_cast<const uint8_t *>(x), weight, scale, shift, mean, std,
                           out, H, W, h1, w1, h2, w2, C0, relu);
    PTX_LAUNCHED("k_conv_stem");
    return PTX_OK;
}

int ptx_conv1x1(const float *x, int N, int Cin, int H, int W, const float *weight, int Cout, int stride, const float *scale,
                const float *shift, const float *residual, int relu, float *out, void *stream)
{
    const char *who = "ptx_conv1x1";
    PTX_REQUIRE(Cin >= 16 && Cin <= 2048 && Cin % 16 == 0 && Cout >= 16 && Cout <= 2048 && Cout % 16 == 0,
                "%s: Cin=%d Cout=%d (multiples of 16 from 16 to 2048)", who, Cin, Cout);
    return conv_launch(who, 1, x, N, Cin, H, W, weight, Cout, stride, scale, shift, residual, relu, out, stream);
}

int ptx_conv3x3(const float *x, int N, int C, int H, int W, const float *weight, int stride, const float *scale, const float *shift,
                const float *residual, int relu, float *out, void *stream)
{
    const char *who = "ptx_conv3x3";
    PTX_REQUIRE(C >= 16 && C <= 512 && C % 16 == 0, "%s: C=%d (a multiple of 16 from 16 to 512)", who, C);
    return conv_launch(who, 3, x, N, C, H, W, weight, C, stride, scale, shift, residual, relu, out, stream);
}

}  // extern "C"
