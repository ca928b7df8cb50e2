// Backward of the dense 1x1 / 3x3 convolutions of the image backbone (conv2d.hip) behind their epilogue * scale + shift, + residual, ReLU,
// with every BatchNorm frozen: scale and shift take no gradient, there is no dbias.  With z the convolution before the epilogue and
// out = relu((z * scale + shift) + residual), g = d loss / d out:
//
//   k_conv_epi_bwd     gz = g * [out > 0] * scale[co], dresidual = g * [out > 0] (relu_mask4's rule: a NaN out passes nothing): a launch
//                      of its own, one thread per element (per four where the output plane is a multiple of 4 pixels).
//   k_conv_wt          the weight operand (Cout, taps, Cin) re-laid as (Cin, taps, Cout) into the workspace: the data gradient's row
//                      operand with its k contiguous.  It runs inside every call that asks for dx, so an optimizer step needs no
//                      re-layout of its own and the cost is part of every timed call.
//   dx                 the forward's implicit GEMM with the roles of Cin and Cout swapped, on the forward's two tiles (conv2d.h:
//                      k_conv_gemm / k_conv_narrow, narrow below 64 rows = Cin) with the transposed reader ConvQuadT: columns = the
//                      pixels of the INPUT map, k = (ky, kx, co) ascending, input pixel (y, x) takes tap (ky, kx) from output
//                      ((y + 1 - ky) / s, (x + 1 - kx) / s) where both numerators are even (s = 2) and in range (1x1: (y / s, x / s)).
//                      Every element of dx is written: a pixel no output reads sums zeros.  Stride 2 multiplies the structurally
//                      absent taps by zero; the pixels are not split by parity class.  dx_accumulate: the tile's epilogue adds what dx
//                      held to the completed sum (ConvOutPixel's residual), one rounding.
//   k_conv_dweight<KS> dweight (Cout, K = taps Cin) = sum over the pixels (n, oy, ox) of gz[n, co, oy, ox] * x[n, ci, s oy - 1 + ky,
//                      s ox - 1 + kx]: grid (S pixel chunks) x (tiles of 64 co x 64 k), head.h's tile64_nt: both operands are read along
//                      the pixels, which is their k (gz: along its plane; x: through ConvQuad, the forward's padding rule -- a tap outside
//                      the image is never read), contraction in steps of 64 pixels, each from zero and then added, ascending.  The
//                      T = ceil(pixels / 64) steps are dealt to the S chunks evenly: chunk c owns steps [c T / S, (c + 1) T / S).  S > 1:
//                      every work-group writes its partial into slab c of the workspace, k_conv_slab_sum adds the slabs in ascending
//                      order (k_sparse_slab_sum's order).
//
// fp32 on the exact-fp32 matrix instruction, no float atomics: two calls give the same bits.  Everything on the caller's stream, no host
// wait.  Restated in numpy by proxytransformation_amd/image_backbone_grad_host.py.
#include "conv2d.h"

namespace ptx {

// ---- epilogue backward --------------------------------------------------------------------------------------------------------------
// t: an element of (N, Cout, plane), or with vec a quad of it (plane % 4 == 0: a quad lies in one channel)
__global__ __launch_bounds__(256) void k_conv_epi_bwd(const float *__restrict__ g, const float *__restrict__ out,
                                                      const float *__restrict__ scale, float *__restrict__ gz, float *__restrict__ dres,
                                                      long count, int plane, int Cout, int vec)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= count) return;
    if (vec) {
        const size_t at = (size_t)t * 4;
        const int co = (int)((at / plane) % Cout);
        float4 d = ld4(g + at);
        if (out) relu_mask4(d, ld4(out + at));
        if (dres) st4(dres + at, d);
        if (gz) {
            if (scale) { const float s = scale[co]; scale4(d, make_float4(s, s, s, s)); }
            st4(gz + at, d);
        }
        return;
    }
    const int co = (int)((t / plane) % Cout);
    float d = g[t];
    if (out) d = out[t] > 0.0f ? d : 0.0f;
    if (dres) dres[t] = d;
    if (gz) gz[t] = scale ? d * scale[co] : d;
}

// ---- the weight, re-laid: dst (Cin, T, Cout) = src (Cout, T, Cin).  grid (cdiv(Cout, 32), cdiv(Cin, 32), T) ----------------------------
__global__ __launch_bounds__(256) void k_conv_wt(const float *__restrict__ src, float *__restrict__ dst, int Cout, int T, int Cin)
{
    __shared__ float s_t[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5, tap = blockIdx.z;
    const int co0 = blockIdx.x * 32, ci0 = blockIdx.y * 32;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int co = co0 + ty + 8 * j, ci = ci0 + tx;
        if (co < Cout && ci < Cin) s_t[ty + 8 * j][tx] = src[((size_t)co * T + tap) * Cin + ci];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ci = ci0 + ty + 8 * j, co = co0 + tx;
        if (co < Cout && ci < Cin) dst[((size_t)ci * T + tap) * Cout + co] = s_t[tx][ty + 8 * j];
    }
}

// ---- the data gradient's pixel operand ----------------------------------------------------------------------------------------------
// ConvQuad run backwards.  ConvArgs here: x = gz with C its channels on the map H x W (the forward's OUTPUT map), Ho x Wo the map that
// is written (the forward's INPUT map), total = N Ho Wo, K = KS KS C with k = (tap, co).  A thread's four consecutive pixels of the
// written map and their values at one k: the element of gz that tap k / C of the forward took this pixel into, zero where there is
// none (an odd numerator at stride 2, outside the map) -- never read.
template <int KS>
struct ConvQuadT {
    size_t base[4];                                         // 1x1: the element of channel 0 this pixel reads; 3x3: the image's first element
    int py[4], px[4];                                       // 3x3: y + 1, x + 1
    bool have[4];
    __device__ __forceinline__ ConvQuadT(const ConvArgs &a, long g_first)
    {
        const int HW = a.H * a.W, HoWo = a.Ho * a.Wo;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long g = g_first + q;
            have[q] = g < a.total;
            const long n = have[q] ? g / HoWo : 0;
            const int p = have[q] ? (int)(g - n * HoWo) : 0, y = p / a.Wo, x = p - y * a.Wo;
            base[q] = (size_t)n * a.C * HW;
            if (KS == 1) {
                if (a.stride == 2 && ((y | x) & 1)) have[q] = false;       // no output reads an odd row or column
                base[q] += (size_t)(y / a.stride) * a.W + x / a.stride;
            }
            py[q] = y + 1; px[q] = x + 1;
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
                const int tap = k / a.C, co = k - tap * a.C, ty = tap / 3, tx = tap - 3 * ty;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    int ny = py[q] - ty, nx = px[q] - tx;   // s oy, s ox
                    bool ok = have[q] && ny >= 0 && nx >= 0;
                    if (a.stride == 2) {
                        ok = ok && !((ny | nx) & 1);
                        ny >>= 1; nx >>= 1;
                    }
                    if (ok && ny < a.H && nx < a.W) e[q] = a.x[base[q] + (size_t)co * HW + (size_t)ny * a.W + nx];
                }
            }
        }
        return make_float4(e[0], e[1], e[2], e[3]);
    }
};

// ---- dweight ------------------------------------------------------------------------------------------------------------------------
struct ConvDwArgs {
    ConvArgs c;                                             // the forward's arguments: x, C = Cin, the maps, the stride, K, total = N Ho Wo
    const float *gz; float *dst;
    int S; long T;                                          // chunks; steps of 64 pixels in all
    size_t slab;                                            // floats between the chunks' partials (0: one chunk, dst is dweight itself)
};

// blockIdx = (pixel chunk, tile of 64 output channels x 64 k)
template <int KS>
__global__ __launch_bounds__(256) void k_conv_dweight(ConvDwArgs d)
{
    const Tile64 t;
    ConvArgs a = d.c;
    const int nkt = (a.K + 63) >> 6;
    const int co0 = ((int)blockIdx.y / nkt) << 6, k0 = ((int)blockIdx.y % nkt) << 6;
    const long s0 = (long)blockIdx.x * d.T / d.S, s1 = ((long)blockIdx.x + 1) * d.T / d.S;
    const long p0 = s0 << 6;
    a.total = min(s1 << 6, a.total);                        // this chunk's end: the readers give zeros behind it
    const int HoWo = a.Ho * a.Wo;
    const int kq = (t.tid & 15) * 4;
    f32x16 tot;
#pragma unroll
    for (int i = 0; i < 16; ++i) tot[i] = 0.0f;
    struct Step { ConvQuad<KS> x; size_t g[4]; bool have[4]; };
    tile64_nt<true>(
        t, (int)(s1 - s0), tot,
        [&](int s) {
            const long g_first = p0 + ((long)s << 6) + kq;
            Step p{ConvQuad<KS>(a, g_first), {}, {}};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const ConvOutPixel o(a, g_first + q);             // gz's element of channel 0
                p.g[q] = o.first; p.have[q] = o.have;
            }
            return p;
        },
        [&](float4 &v, const Step &p, int row, int) {      // gz[., co0 + row, the step's pixels]
            float e[4] = {0.f, 0.f, 0.f, 0.f};
            const int co = co0 + row;
            if (co < a.Cout) {
                if (a.vec) {
                    if (p.have[0]) {
                        const float4 w = ld4(d.gz + p.g[0] + (size_t)co * HoWo);
                        e[0] = w.x; e[1] = w.y; e[2] = w.z; e[3] = w.w;
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (p.have[q]) e[q] = d.gz[p.g[q] + (size_t)co * HoWo];
                }
            }
            v = make_float4(e[0], e[1], e[2], e[3]);
        },
        [&](float4 &v, const Step &p, int row, int) { v = p.x.load(a, k0 + row); },      // x at k = (tap, ci), zeros beyond K
        [](int) {});
    float *dst = d.dst + (size_t)blockIdx.x * d.slab;
    const int k = k0 + t.col();
    if (k >= a.K) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = co0 + t.row(r);
        if (co < a.Cout) dst[(size_t)co * a.K + k] = tot[r];
    }
}

// dst (L) = slab 0 + slab 1 + ... + slab S-1, in that order; one thread per 4 floats (k_sparse_slab_sum's order)
__global__ __launch_bounds__(256) void k_conv_slab_sum(const float *__restrict__ ws, int S, size_t L, float *__restrict__ dst)
{
    const size_t e = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (e >= L) return;
    float4 v = ld4(ws + e);
    for (int s = 1; s < S; ++s) acc4(v, ld4(ws + (size_t)s * L + e));
    st4(dst + e, v);
}

// ---- the plan: a function of the shapes only ----------------------------------------------------------------------------------------
struct ConvDwPlan { int S; long T; size_t slab, wt_bytes, dw_bytes, total; };

static bool conv_bwd_shapes_ok(int KS, int N, int Cin, int Cout, int H, int W, int stride)
{
    const int top = KS == 1 ? 2048 : 512;
    if (KS != 1 && KS != 3) return false;
    if (KS == 3 && Cin != Cout) return false;
    if (Cin < 16 || Cin > top || Cin % 16 || Cout < 16 || Cout > top || Cout % 16) return false;
    if (N < 1 || N > kConvMaxImages || H < 1 || H > kConvMaxSide || W < 1 || W > kConvMaxSide) return false;
    if (stride != 1 && stride != 2) return false;
    return (long)H * W < (1l << 30) && (long)N * H * W < (1l << 31) * 64;
}

// The T = ceil(pixels / 64) steps go to S chunks: enough work-groups to cover the 256 CUs about four times over, at least 4 steps (256
// pixels) a chunk, a workspace of at most 256 MiB.  S never falls when N grows.
static ConvDwPlan conv_dw_plan(int KS, int N, int Cin, int Cout, int H, int W, int stride)
{
    ConvDwPlan P{};
    const int K = KS * KS * Cin;
    const long pixels = (long)N * ((H - 1) / stride + 1) * ((W - 1) / stride + 1);
    const long tiles = (long)cdiv(Cout, 64) * cdiv(K, 64);
    P.slab = (size_t)Cout * K;
    P.T = (pixels + 63) / 64;
    long S = (1024 + tiles - 1) / tiles;
    const long cap = (long)((size_t(256) << 20) / (P.slab * sizeof(float)));
    S = S > cap ? cap : S;
    S = S > (P.T + 3) / 4 ? (P.T + 3) / 4 : S;
    P.S = (int)(S < 1 ? 1 : S);
    P.wt_bytes = align_up(P.slab * sizeof(float), 256);
    P.dw_bytes = P.S > 1 ? align_up((size_t)P.S * P.slab * sizeof(float), 256) : 0;
    P.total = P.wt_bytes + P.dw_bytes;
    return P;
}

static bool conv_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    if (!a || !b) return false;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + nb && b0 < a0 + na;
}

static int conv_bwd(const char *who, int KS, const float *g, const float *out, const float *scale, int relu, const float *x, int N, int Cin,
                    int H, int W, const float *weight, int Cout, int stride, float *gz, float *dresidual, float *dx, int dx_accumulate,
                    float *dweight, void *workspace, size_t ws_bytes, void *stream)
{
    PTX_REQUIRE(N >= 1 && N <= kConvMaxImages && H >= 1 && H <= kConvMaxSide && W >= 1 && W <= kConvMaxSide,
                "%s: N=%d H=%d W=%d (N: 1 to %d images; H, W: 1 to %d)", who, N, H, W, kConvMaxImages, kConvMaxSide);
    PTX_REQUIRE(stride == 1 || stride == 2, "%s: stride=%d (1 or 2)", who, stride);
    PTX_REQUIRE(relu == 0 || relu == 1, "%s: relu=%d (0 or 1)", who, relu);
    PTX_REQUIRE(dx_accumulate == 0 || dx_accumulate == 1, "%s: dx_accumulate=%d (0 or 1)", who, dx_accumulate);
    PTX_REQUIRE(conv_bwd_shapes_ok(KS, N, Cin, Cout, H, W, stride), "%s: N=%d H=%d W=%d is out of range", who, N, H, W);
    const bool epi = relu != 0 || scale != nullptr, need_z = dx != nullptr || dweight != nullptr;
    PTX_REQUIRE(g, "%s: g is null", who);
    PTX_REQUIRE(!relu || out, "%s: relu needs the forward's out", who);
    PTX_REQUIRE(!(epi && need_z) || gz, "%s: gz is needed with relu / scale when dx or dweight is asked for", who);
    PTX_REQUIRE(!dx || weight, "%s: dx needs weight", who);
    PTX_REQUIRE(!dweight || x, "%s: dweight needs x", who);
    PTX_REQUIRE(sp_aligned16({g, out, scale, x, weight, gz, dresidual, dx, dweight, workspace}),
                "%s: every float buffer and the workspace must be 16-byte aligned", who);
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1, K = KS * KS * Cin;
    const long pixels = (long)N * Ho * Wo;
    const size_t n_g = (size_t)pixels * Cout * sizeof(float), n_x = (size_t)N * Cin * H * W * sizeof(float);
    const size_t n_w = (size_t)Cout * K * sizeof(float);
    PTX_REQUIRE((long)pixels * Cout < (1l << 31) * 256, "%s: N=%d Cout=%d on %d x %d is out of range", who, N, Cout, Ho, Wo);
    const ConvDwPlan P = conv_dw_plan(KS, N, Cin, Cout, H, W, stride);
    {
        const struct { const void *p; size_t n; const char *name; } ins[] = {{g, n_g, "g"}, {out, n_g, "out"},
            {scale, Cout * sizeof(float), "scale"}, {x, n_x, "x"}, {weight, n_w, "weight"}},
          outs[] = {{epi && need_z ? gz : nullptr, n_g, "gz"}, {dresidual, n_g, "dresidual"}, {dx, n_x, "dx"}, {dweight, n_w, "dweight"},
                    {workspace, ws_bytes < P.total ? ws_bytes : P.total, "workspace"}};
        for (size_t o = 0; o < sizeof(outs) / sizeof(outs[0]); ++o) {
            for (const auto &i : ins)
                PTX_REQUIRE(!conv_overlap(outs[o].p, outs[o].n, i.p, i.n), "%s: %s overlaps %s (outputs must not alias inputs)", who,
                            outs[o].name, i.name);
            for (size_t o2 = 0; o2 < o; ++o2)
                PTX_REQUIRE(!conv_overlap(outs[o].p, outs[o].n, outs[o2].p, outs[o2].n), "%s: %s overlaps %s (outputs must not alias)", who,
                            outs[o].name, outs[o2].name);
        }
    }
    if (dx != nullptr || (dweight != nullptr && P.S > 1)) {
        PTX_REQUIRE(workspace, "%s: workspace is null", who);
        PTX_TRY(sp_workspace_fits(who, ws_bytes, P.total));
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *ws = static_cast<char *>(workspace);
    if ((epi && need_z) || dresidual) {
        const int vec = (Ho * Wo) % 4 == 0;
        const long count = vec ? pixels * Cout / 4 : pixels * Cout;
        hipLaunchKernelGGL(k_conv_epi_bwd, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, g, relu ? out : nullptr, scale,
                           epi && need_z ? gz : nullptr, dresidual, count, Ho * Wo, Cout, vec);
        PTX_LAUNCHED("k_conv_epi_bwd");
    }
    const float *z = epi ? gz : g;
    if (dx) {
        float *wt = reinterpret_cast<float *>(ws);
        hipLaunchKernelGGL(k_conv_wt, dim3(cdiv(Cout, 32), cdiv(Cin, 32), KS * KS), dim3(256), 0, st, weight, wt, Cout, KS * KS, Cin);
        PTX_LAUNCHED("k_conv_wt");
        ConvArgs a{};
        a.x = z; a.w = wt; a.residual = dx_accumulate ? dx : nullptr; a.out = dx;
        a.C = Cout; a.Cout = Cin; a.H = Ho; a.W = Wo; a.Ho = H; a.Wo = W; a.stride = stride; a.K = KS * KS * Cout;
        a.total = (long)N * H * W;
        a.vec = KS == 1 && stride == 1 && (H * W) % 4 == 0;
        // the forward's choice of tile, with Cin the rows
        if (Cin < 64 && !(KS == 3 && stride == 2 && Cin > 16)) {
            const dim3 grid((unsigned)((a.total + kNarrowPx - 1) / kNarrowPx), (unsigned)(Cin / 16));
            if (KS == 1) hipLaunchKernelGGL((k_conv_narrow<ConvQuadT<1>>), grid, dim3(256), 0, st, a);
            else hipLaunchKernelGGL((k_conv_narrow<ConvQuadT<3>>), grid, dim3(256), 0, st, a);
            PTX_LAUNCHED("k_conv_narrow<T>");
        } else {
            const dim3 grid((unsigned)((a.total + 63) / 64), (unsigned)cdiv(Cin, 64));
            if (KS == 1) hipLaunchKernelGGL((k_conv_gemm<ConvQuadT<1>>), grid, dim3(256), 0, st, a);
            else hipLaunchKernelGGL((k_conv_gemm<ConvQuadT<3>>), grid, dim3(256), 0, st, a);
            PTX_LAUNCHED("k_conv_gemm<T>");
        }
    }
    if (dweight) {
        ConvDwArgs d{};
        d.c.x = x; d.c.C = Cin; d.c.Cout = Cout; d.c.H = H; d.c.W = W; d.c.Ho = Ho; d.c.Wo = Wo; d.c.stride = stride; d.c.K = K;
        d.c.total = pixels;
        d.c.vec = (Ho * Wo) % 4 == 0 && (KS != 1 || stride == 1);    // gz's quads, and the 1x1's x quads with them
        d.gz = z; d.S = P.S; d.T = P.T;
        d.slab = P.S > 1 ? P.slab : 0;
        d.dst = P.S > 1 ? reinterpret_cast<float *>(ws + P.wt_bytes) : dweight;
        const dim3 grid((unsigned)P.S, (unsigned)(cdiv(Cout, 64) * cdiv(K, 64)));
        if (KS == 1) hipLaunchKernelGGL((k_conv_dweight<1>), grid, dim3(256), 0, st, d);
        else hipLaunchKernelGGL((k_conv_dweight<3>), grid, dim3(256), 0, st, d);
        PTX_LAUNCHED(KS == 1 ? "k_conv_dweight<1>" : "k_conv_dweight<3>");
        if (P.S > 1) {
            hipLaunchKernelGGL(k_conv_slab_sum, dim3((unsigned)((P.slab / 4 + 255) / 256)), dim3(256), 0, st, d.dst, P.S, P.slab, dweight);
            PTX_LAUNCHED("k_conv_slab_sum");
        }
    }
    return PTX_OK;
}

}  // namespace ptx

using namespace ptx;

extern "C" {

size_t ptx_conv_bwd_workspace_bytes(int KS, int N, int Cin, int Cout, int H, int W, int stride)
{
    if (!conv_bwd_shapes_ok(KS, N, Cin, Cout, H, W, stride)) return 0;
    return conv_dw_plan(KS, N, Cin, Cout, H, W, stride).total;
}

int ptx_conv_dweight_chunks(int KS, int N, int Cin, int Cout, int H, int W, int stride)
{
    PTX_REQUIRE(conv_bwd_shapes_ok(KS, N, Cin, Cout, H, W, stride),
                "ptx_conv_dweight_chunks: KS=%d N=%d Cin=%d Cout=%d H=%d W=%d stride=%d (KS: 1 or 3; widths: multiples of 16 up to 2048 "
                "(1x1) / 512 (3x3, Cin = Cout); stride: 1 or 2)", KS, N, Cin, Cout, H, W, stride);
    return conv_dw_plan(KS, N, Cin, Cout, H, W, stride).S;
}

int ptx_conv1x1_bwd(const float *g, const float *out, const float *scale, int relu, const float *x, int N, int Cin, int H, int W,
                    const float *weight, int Cout, int stride, float *gz, float *dresidual, float *dx, int dx_accumulate, float *dweight,
                    void *workspace, size_t ws_bytes, void *stream)
{
    const char *who = "ptx_conv1x1_bwd";
    PTX_REQUIRE(Cin >= 16 && Cin <= 2048 && Cin % 16 == 0 && Cout >= 16 && Cout <= 2048 && Cout % 16 == 0,
                "%s: Cin=%d Cout=%d (multiples of 16 from 16 to 2048)", who, Cin, Cout);
    return conv_bwd(who, 1, g, out, scale, relu, x, N, Cin, H, W, weight, Cout, stride, gz, dresidual, dx, dx_accumulate, dweight, workspace,
                    ws_bytes, stream);
}

int ptx_conv3x3_bwd(const float *g, const float *out, const float *scale, int relu, const float *x, int N, int C, int H, int W,
                    const float *weight, int stride, float *gz, float *dresidual, float *dx, int dx_accumulate, float *dweight,
                    void *workspace, size_t ws_bytes, void *stream)
{
    const char *who = "ptx_conv3x3_bwd";
    PTX_REQUIRE(C >= 16 && C <= 512 && C % 16 == 0, "%s: C=%d (a multiple of 16 from 16 to 512)", who, C);
    return conv_bwd(who, 3, g, out, scale, relu, x, N, C, H, W, weight, C, stride, gz, dresidual, dx, dx_accumulate, dweight, workspace,
                    ws_bytes, stream);
}

}  // extern "C"
