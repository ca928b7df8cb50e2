// What closes the decoder's chain under autograd beside decoder_bwd.hip: PositionEmbeddingLearned with a training-mode BatchNorm (forward
// statistics and backward), the backward of the box head and of ContrastiveEmbed.
//
//   ptx_dec_posembed_stats  two launches.  k_pe_moments: work-group = (slab of rows, 64 channels), thread = (channel, one of 4 row lanes).
//       z = x W1^T + b1 is recomputed from the cin <= 9 inputs (fp32, ascending j, the bias last); per 256-row chunk the sum of z, then
//       the centred squares around the chunk's mean, both in double, the four row lanes added as (0 + 1) + (2 + 3); chunks and then slabs
//       are merged in ascending order by Chan's formula in double: never E[z^2] - E[z]^2.  k_pe_fold: one thread per channel merges the
//       slabs, folds the batch statistics and the affine into (w1', b1') in double (rounded once), keeps (mean, rstd) and applies the
//       running-statistics update `repeat` times as sequential fp32 updates.  The forward itself is ptx_dec_posembed on (w1', b1').
//   ptx_dec_posembed_hidden  h (n,C) = relu(x w1'^T + b1') in the forward's order (the forward's bits), for dW2 = dout^T h.
//   ptx_dec_posembed_bwd  four launches over the same slabs: with dh = dout W2 given, dpre = dh where the recomputed h > 0 (a NaN passes
//       nothing), zhat = (z - mean) rstd: dbeta = sum dpre, dgamma = sum dpre zhat; then dz = gamma rstd (dpre - dbeta / n - zhat dgamma / n),
//       dW1 = dz^T x, db1 = sum dz.  Products in fp32, every sum over rows in double in a fixed order (rows ascending per lane, lanes
//       (0 + 1) + (2 + 3), slabs ascending).
//   ptx_dec_boxes_bwd  k_dec_boxes_bwd over 16-row groups as k_head_boxes: the log-sizes p[3:6] recomputed in the forward's order,
//       dp = d for center and euler, dp = (expf(p) >= 0.02 ? d : 0) * expf(p) for the sizes (torch's exp().clamp(min): a NaN p gives NaN),
//       dh = dp W (k ascending); then dW = dp^T h through the slab reduction.  dbias = colsum(dp) is the caller's (ptx_op_colsum).
//   ptx_dec_scores_bwd  dhidden = dS text / sqrt(C) and dtext[b] = sum_{l,k} dS^T hidden / sqrt(C) as two tile64_nt launches on the
//       exact-fp32 matrix instruction; dS under a masked token or from column T on is never read (predicated loads), nor is the text row
//       of a masked token.  dbias = sum of the read dS: per (layer, scene) in double, then ascending.
//
// fp32, no float atomics, fixed summation orders (bitwise reproducible), everything on the caller's stream, no host wait.  Held to the
// numpy restatements of proxytransformation_amd/decoder_grad_host.py.
#include "head.h"
#include "dec_train_plan.h"

namespace ptx {

constexpr int kTrMaxPos = 9;

enum { TR_PE_SUMS = 0, TR_PE_DW1 = 1, TR_BOX_DW = 2 };

struct TrSlabArgs {
    const float *small;                                     // (n,na): x (posembed) or dp (boxes)
    const float *big;                                       // (n,C): dh (posembed) or h (boxes)
    const float *w1, *b1, *w1f, *b1f, *gamma, *stats, *dgb; // posembed: raw and folded first layer, (mean | rstd), (dbeta | dgamma)
    double *ws;                                             // (S,nv,C)
    long n;
    int C, na, nv, per;
};

// blockIdx = (slab, 64-channel tile); thread (channel tid & 63, row lane tid >> 6) walks rows lane, lane + 4, .. of every chunk
template <int MODE>
__global__ __launch_bounds__(256) void k_dec_slab(TrSlabArgs a)
{
    __shared__ float s_x[kTrChunk][kTrMaxVals];
    __shared__ double s_red[4][kTrMaxVals][64];
    const int tid = threadIdx.x, cl = tid & 63, q = tid >> 6;
    const int c = blockIdx.y * 64 + cl;
    float w1[kTrMaxPos], w1f[kTrMaxPos], b1 = 0.f, b1f = 0.f, mean = 0.f, rstd = 0.f, gr = 0.f, mb = 0.f, mg = 0.f;
    if (MODE != TR_BOX_DW) {
#pragma unroll
        for (int j = 0; j < kTrMaxPos; ++j) {
            w1[j] = j < a.na ? a.w1[c * a.na + j] : 0.0f;
            w1f[j] = j < a.na ? a.w1f[c * a.na + j] : 0.0f;
        }
        b1 = a.b1[c]; b1f = a.b1f[c]; mean = a.stats[c]; rstd = a.stats[a.C + c];
        if (MODE == TR_PE_DW1) {
            gr = a.gamma[c] * rstd;
            mb = a.dgb[c] / (float)a.n;
            mg = a.dgb[a.C + c] / (float)a.n;
        }
    }
    double acc[kTrMaxVals];
#pragma unroll
    for (int v = 0; v < kTrMaxVals; ++v) acc[v] = 0.0;
    const long chunk0 = (long)blockIdx.x * a.per;
    for (int ci = 0; ci < a.per; ++ci) {
        const long row0 = (chunk0 + ci) * kTrChunk;
        if (row0 >= a.n) break;                             // work-group uniform
        for (int e = tid; e < kTrChunk * a.na; e += 256) {
            const int r = e / a.na, j = e - r * a.na;
            s_x[r][j] = row0 + r < a.n ? a.small[(size_t)(row0 + r) * a.na + j] : 0.0f;
        }
        __syncthreads();
        for (int i = 0; i < kTrChunk / 4; ++i) {
            const int lr = q + 4 * i;
            const long row = row0 + lr;
            if (row >= a.n) break;
            const float big = a.big[(size_t)row * a.C + c];
            if (MODE == TR_BOX_DW) {
#pragma unroll
                for (int v = 0; v < kHeadReg; ++v) acc[v] += (double)(s_x[lr][v] * big);
            } else {
                float z = 0.0f, hf = 0.0f;
#pragma unroll
                for (int j = 0; j < kTrMaxPos; ++j)
                    if (j < a.na) { z = z + s_x[lr][j] * w1[j]; hf = hf + s_x[lr][j] * w1f[j]; }
                z = z + b1;
                hf = hf + b1f;                              // the forward's hidden value before its ReLU: a NaN passes nothing
                const float zh = (z - mean) * rstd;
                const float dpre = hf > 0.0f ? big : 0.0f;
                if (MODE == TR_PE_SUMS) {
                    acc[0] += (double)dpre;
                    acc[1] += (double)(dpre * zh);
                } else {
                    const float dz = gr * (dpre - mb - zh * mg);
#pragma unroll
                    for (int j = 0; j < kTrMaxPos; ++j)
                        if (j < a.na) acc[j] += (double)(dz * s_x[lr][j]);
                    acc[kTrMaxPos] += (double)dz;           // db1 rides in the last slot
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int v = 0; v < kTrMaxVals; ++v) s_red[q][v][cl] = acc[v];
    __syncthreads();
    if (q != 0) return;
    // the values of a mode: PE_SUMS 0, 1; BOX_DW 0 .. 8; PE_DW1 0 .. na - 1 and the last slot as value na
    for (int v = 0; v < a.nv; ++v) {
        const int src = (MODE == TR_PE_DW1 && v == a.nv - 1) ? kTrMaxPos : v;
        const double tot = (s_red[0][src][cl] + s_red[1][src][cl]) + (s_red[2][src][cl] + s_red[3][src][cl]);
        a.ws[((size_t)blockIdx.x * a.nv + v) * a.C + c] = tot;
    }
}

// out = the sum over the S slabs in ascending order, in double, rounded once: value v < nva of channel c goes to outa[c nva + v] (a
// (C,nva) matrix), value v >= nva to outb[(v - nva) C + c]
__global__ void k_dec_slab_finish(const double *ws, int S, int nv, int C, int nva, float *outa, float *outb)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv * C) return;
    const int v = i / C, c = i - v * C;
    double s = 0.0;
    for (int k = 0; k < S; ++k) s += ws[((size_t)k * nv + v) * C + c];
    if (v < nva) outa[(size_t)c * nva + v] = (float)s;
    else outb[(size_t)(v - nva) * C + c] = (float)s;
}

// ---- posembed: batch statistics -------------------------------------------------------------------------------------------------------
struct PeStatArgs {
    const float *x, *w1, *b1;
    double *ws;                                             // (S,2,C): mean, centred sum of squares of every slab
    long n;
    int C, cin, per;
};

__global__ __launch_bounds__(256) void k_pe_moments(PeStatArgs a)
{
    __shared__ float s_x[kTrChunk][kTrMaxVals];
    __shared__ double s_red[4][64];
    const int tid = threadIdx.x, cl = tid & 63, q = tid >> 6;
    const int c = blockIdx.y * 64 + cl;
    float w1[kTrMaxPos];
#pragma unroll
    for (int j = 0; j < kTrMaxPos; ++j) w1[j] = j < a.cin ? a.w1[c * a.cin + j] : 0.0f;
    const float b1 = a.b1[c];
    double cnt = 0.0, mean = 0.0, m2 = 0.0;                 // the slab so far; the four row lanes hold the same values
    const long chunk0 = (long)blockIdx.x * a.per;
    for (int ci = 0; ci < a.per; ++ci) {
        const long row0 = (chunk0 + ci) * kTrChunk;
        if (row0 >= a.n) break;                             // work-group uniform
        for (int e = tid; e < kTrChunk * a.cin; e += 256) {
            const int r = e / a.cin, j = e - r * a.cin;
            s_x[r][j] = row0 + r < a.n ? a.x[(size_t)(row0 + r) * a.cin + j] : 0.0f;
        }
        __syncthreads();
        const long left = a.n - row0;
        const int rows = left < kTrChunk ? (int)left : kTrChunk;
        auto zof = [&](int lr) {
            float z = 0.0f;
#pragma unroll
            for (int j = 0; j < kTrMaxPos; ++j)
                if (j < a.cin) z = z + s_x[lr][j] * w1[j];
            return z + b1;
        };
        double s = 0.0;
        for (int lr = q; lr < rows; lr += 4) s += (double)zof(lr);
        s_red[q][cl] = s;
        __syncthreads();
        const double cm = ((s_red[0][cl] + s_red[1][cl]) + (s_red[2][cl] + s_red[3][cl])) / (double)rows;
        __syncthreads();
        double ss = 0.0;
        for (int lr = q; lr < rows; lr += 4) {
            const double d = (double)zof(lr) - cm;
            ss += d * d;
        }
        s_red[q][cl] = ss;
        __syncthreads();
        const double cm2 = (s_red[0][cl] + s_red[1][cl]) + (s_red[2][cl] + s_red[3][cl]);
        const double tot = cnt + (double)rows, delta = cm - mean;      // Chan's merge of (cnt, mean, m2) with the chunk
        mean = mean + delta * ((double)rows / tot);
        m2 = m2 + cm2 + delta * delta * (cnt * (double)rows / tot);
        cnt = tot;
        __syncthreads();
    }
    if (q == 0) {
        a.ws[((size_t)blockIdx.x * 2 + 0) * a.C + c] = mean;
        a.ws[((size_t)blockIdx.x * 2 + 1) * a.C + c] = m2;
    }
}

struct PeFoldArgs {
    const double *ws;
    const float *w1, *b1, *gamma, *beta;
    float *run_mean, *run_var, *w1f, *b1f, *stats;
    long n;
    int C, cin, per, S, repeat;
    double eps;
    float momentum;
};

__global__ void k_pe_fold(PeFoldArgs a)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.C) return;
    double cnt = 0.0, mean = 0.0, m2 = 0.0;
    const long slab_rows = (long)a.per * kTrChunk;
    for (int s = 0; s < a.S; ++s) {
        const long left = a.n - (long)s * slab_rows;
        const double rows = (double)(left < slab_rows ? left : slab_rows);
        const double sm = a.ws[((size_t)s * 2 + 0) * a.C + c], sm2 = a.ws[((size_t)s * 2 + 1) * a.C + c];
        const double tot = cnt + rows, delta = sm - mean;
        mean = mean + delta * (rows / tot);
        m2 = m2 + sm2 + delta * delta * (cnt * rows / tot);
        cnt = tot;
    }
    const double rstd = 1.0 / sqrt(m2 / (double)a.n + a.eps);         // the biased variance normalises
    const double sc = (double)a.gamma[c] * rstd;
    for (int j = 0; j < a.cin; ++j) a.w1f[c * a.cin + j] = (float)((double)a.w1[c * a.cin + j] * sc);
    a.b1f[c] = (float)(((double)a.b1[c] - mean) * sc + (double)a.beta[c]);
    a.stats[c] = (float)mean;
    a.stats[a.C + c] = (float)rstd;
    if (a.run_mean != nullptr && a.repeat > 0) {            // nn.BatchNorm1d's update, `repeat` calls on the same rows: the unbiased variance
        const float bm = (float)mean, bv = (float)(m2 / (double)(a.n - 1)), keep = 1.0f - a.momentum;
        float rm = a.run_mean[c], rv = a.run_var[c];
        for (int r = 0; r < a.repeat; ++r) {
            rm = keep * rm + a.momentum * bm;
            rv = keep * rv + a.momentum * bv;
        }
        a.run_mean[c] = rm;
        a.run_var[c] = rv;
    }
}

__global__ void k_pe_hidden(const float *x, long n, int cin, const float *w1f, const float *b1f, int C, float *h)
{
    const long total = n * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long row = i / C;
        const int c = (int)(i - row * C);
        float v = 0.0f;
        for (int j = 0; j < cin; ++j) v = v + x[(size_t)row * cin + j] * w1f[c * cin + j];
        h[i] = relu_nan(v + b1f[c]);
    }
}

// ---- boxes ------------------------------------------------------------------------------------------------------------------------
struct BoxBwdArgs {
    const float *h, *weight, *bias, *dboxes;                // (n,C), (9,C), (9) or null, (n,9)
    float *dh, *dp;                                         // (n,C), (n,9)
    int n, C;
};

__global__ __launch_bounds__(256) void k_dec_boxes_bwd(BoxBwdArgs a)
{
    __shared__ __attribute__((aligned(16))) float s_w[kHeadReg * 512];
    for (int e = threadIdx.x; e < kHeadReg * a.C; e += 256) s_w[e] = a.weight[e];
    __syncthreads();
    const int l = threadIdx.x & 15;
    const long row = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int nm = a.C >> 6;
    const bool have = row < a.n;
    float4 x[8];
#pragma unroll
    for (int m = 0; m < 8; ++m)
        x[m] = (m < nm && have) ? ld4(a.h + (size_t)row * a.C + 64 * m + 4 * l) : make_float4(0.f, 0.f, 0.f, 0.f);
    float mine = 0.0f;
#pragma unroll
    for (int k = 3; k < 6; ++k) {                           // the log-sizes as the forward forms them
        float s = row_dot16(x, nm, &s_w[k * a.C], l);
        if (a.bias) s = s + a.bias[k];
        if (k == l) mine = s;
    }
    float dp = 0.0f;
    if (have && l < kHeadReg) {
        dp = a.dboxes[(size_t)row * kHeadReg + l];
        if (l >= 3 && l < 6) {
            const float e = expf(mine);
            dp = (e >= 0.02f ? dp : 0.0f) * e;              // clamp(min) passes where exp(p) >= 0.02, then exp's own factor
        }
        a.dp[(size_t)row * kHeadReg + l] = dp;
    }
    float4 g[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) g[m] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < kHeadReg; ++k) {
        const float dk = __shfl(dp, k, 16);
#pragma unroll
        for (int m = 0; m < 8; ++m)
            if (m < nm) {
                const float4 w4 = ld4(&s_w[k * a.C + 64 * m + 4 * l]);
                g[m].x = g[m].x + dk * w4.x; g[m].y = g[m].y + dk * w4.y; g[m].z = g[m].z + dk * w4.z; g[m].w = g[m].w + dk * w4.w;
            }
    }
#pragma unroll
    for (int m = 0; m < 8; ++m)
        if (m < nm && have) st4(a.dh + (size_t)row * a.C + 64 * m + 4 * l, g[m]);
}

// ---- scores -----------------------------------------------------------------------------------------------------------------------
struct ScoreBwdArgs {
    const float *ds, *hidden, *text;                        // (NL,B,K,M), (NL,B,K,C), (B,T,C)
    const uint8_t *mask;                                    // (B,T), 1 = a token
    float *dhidden, *dtext;
    double *ws;                                             // (NL B)
    int NL, B, K, C, T, M, scaled;
    float divisor;
};

// blockIdx = (row tile of the K queries, 64-channel tile, layer * B + scene): dhidden = dS text over the tokens
__global__ __launch_bounds__(256) void k_dec_scores_dh(ScoreBwdArgs a)
{
    const Tile64 t;
    const int row0 = blockIdx.x * 64, col0 = blockIdx.y * 64, z = blockIdx.z, b = z % a.B;
    const float *ds = a.ds + (size_t)z * a.K * a.M;
    const float *text = a.text + (size_t)b * a.T * a.C;
    const uint8_t *mask = a.mask + (size_t)b * a.T;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    tile64_nt<false>(
        t, (a.T + 63) >> 6, acc,
        [](int s) { return s << 6; },
        [&](float4 &v, int t0, int row, int kq) {
            float e[4] = {0.f, 0.f, 0.f, 0.f};
            const int grow = row0 + row;
            if (grow < a.K) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int tok = t0 + kq + i;
                    if (tok < a.T && mask[tok] != 0) e[i] = ds[(size_t)grow * a.M + tok];      // never read under the mask
                }
            }
            v = make_float4(e[0], e[1], e[2], e[3]);
        },
        [&](float4 &v, int t0, int row, int kq) {
            float e[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int tok = t0 + kq + i;
                if (tok < a.T && mask[tok] != 0) e[i] = text[(size_t)tok * a.C + col0 + row];
            }
            v = make_float4(e[0], e[1], e[2], e[3]);
        },
        [](int) {});
    const int n = col0 + t.col();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = row0 + t.row(r);
        if (row < a.K) a.dhidden[((size_t)z * a.K + row) * a.C + n] = a.scaled ? acc[r] / a.divisor : acc[r];
    }
}

// blockIdx = (row tile of the T tokens, 64-channel tile, scene): dtext = dS^T hidden over r = layer * K + query, ascending
__global__ __launch_bounds__(256) void k_dec_scores_dtext(ScoreBwdArgs a)
{
    const Tile64 t;
    const int row0 = blockIdx.x * 64, col0 = blockIdx.y * 64, b = blockIdx.z;
    const uint8_t *mask = a.mask + (size_t)b * a.T;
    const int R = a.NL * a.K;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    tile64_nt<false>(
        t, (R + 63) >> 6, acc,
        [](int s) { return s << 6; },
        [&](float4 &v, int r0, int row, int kq) {
            float e[4] = {0.f, 0.f, 0.f, 0.f};
            const int tok = row0 + row;
            if (tok < a.T && mask[tok] != 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int r = r0 + kq + i;
                    if (r < R) {
                        const int l = r / a.K, k = r - l * a.K;
                        e[i] = a.ds[(((size_t)l * a.B + b) * a.K + k) * a.M + tok];
                    }
                }
            }
            v = make_float4(e[0], e[1], e[2], e[3]);
        },
        [&](float4 &v, int r0, int row, int kq) {
            float e[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = r0 + kq + i;
                if (r < R) {
                    const int l = r / a.K, k = r - l * a.K;
                    e[i] = a.hidden[(((size_t)l * a.B + b) * a.K + k) * a.C + col0 + row];
                }
            }
            v = make_float4(e[0], e[1], e[2], e[3]);
        },
        [](int) {});
    const int n = col0 + t.col();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int tok = row0 + t.row(r);
        if (tok < a.T) a.dtext[((size_t)b * a.T + tok) * a.C + n] = a.scaled ? acc[r] / a.divisor : acc[r];
    }
}

// blockIdx = layer * B + scene: the sum of the dS that count, elements ascending per thread, in double
__global__ __launch_bounds__(256) void k_dec_scores_dbias(ScoreBwdArgs a)
{
    __shared__ double s_red[256];
    const int z = blockIdx.x, b = z % a.B, tid = threadIdx.x;
    const float *ds = a.ds + (size_t)z * a.K * a.M;
    const uint8_t *mask = a.mask + (size_t)b * a.T;
    double s = 0.0;
    const int total = a.K * a.T;
    for (int e = tid; e < total; e += 256) {
        const int k = e / a.T, tok = e - k * a.T;
        if (mask[tok] != 0) s += (double)ds[(size_t)k * a.M + tok];
    }
    s_red[tid] = s;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (tid < w) s_red[tid] = s_red[tid] + s_red[tid + w];
        __syncthreads();
    }
    if (tid == 0) a.ws[z] = s_red[0];
}

static int tr_slab_launch(int mode, const TrSlabArgs &a, int S, hipStream_t st)
{
    const dim3 grid(S, a.C / 64);
    if (mode == TR_PE_SUMS) hipLaunchKernelGGL((k_dec_slab<TR_PE_SUMS>), grid, dim3(256), 0, st, a);
    else if (mode == TR_PE_DW1) hipLaunchKernelGGL((k_dec_slab<TR_PE_DW1>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_dec_slab<TR_BOX_DW>), grid, dim3(256), 0, st, a);
    PTX_LAUNCHED("k_dec_slab");
    return PTX_OK;
}

static int tr_finish_launch(const double *ws, int S, int nv, int C, int nva, float *outa, float *outb, hipStream_t st)
{
    hipLaunchKernelGGL(k_dec_slab_finish, dim3(cdiv(nv * C, 256)), dim3(256), 0, st, ws, S, nv, C, nva, outa, outb);
    PTX_LAUNCHED("k_dec_slab_finish");
    return PTX_OK;
}

static int tr_rows_ok(const char *who, long n)
{
    PTX_REQUIRE(n >= 1 && n <= (1l << 24), "%s: n=%ld rows (1 to 2^24)", who, n);
    return PTX_OK;
}

}  // namespace ptx

using namespace ptx;

extern "C" {

size_t ptx_dec_train_workspace_bytes(long n, int C, int nv)
{
    return tr_workspace_bytes(n, C, nv);
}

int ptx_dec_posembed_stats(const float *x, long n, int cin, const float *w1, const float *b1, const float *gamma, const float *beta, int C,
                           double eps, float momentum, int repeat, float *run_mean, float *run_var, float *w1f, float *b1f, float *stats,
                           void *workspace, size_t ws_bytes, void *stream)
{
    const char *who = "ptx_dec_posembed_stats";
    PTX_TRY(tr_rows_ok(who, n));
    PTX_REQUIRE(n >= 2, "%s: n=%ld (batch statistics need more than one row)", who, n);
    PTX_REQUIRE(cin >= 1 && cin <= kTrMaxPos && sp_width_ok(C), "%s: cin=%d C=%d (cin: 1 to %d; C: a multiple of 64 up to 512)", who, cin, C,
                kTrMaxPos);
    PTX_REQUIRE(eps > 0.0 && momentum >= 0.0f && momentum <= 1.0f && repeat >= 0 && repeat <= 64,
                "%s: eps=%g momentum=%g repeat=%d (eps > 0; momentum: 0 to 1; repeat: 0 to 64)", who, eps, (double)momentum, repeat);
    PTX_REQUIRE(x && w1 && b1 && gamma && beta && w1f && b1f && stats && workspace && (run_mean != nullptr) == (run_var != nullptr),
                "%s: null argument", who);
    PTX_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "%s: the workspace must be 8-byte aligned", who);
    PTX_TRY(sp_workspace_fits(who, ws_bytes, ptx_dec_train_workspace_bytes(n, C, 2)));
    const TrPlan p = tr_plan(n);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const PeStatArgs m{x, w1, b1, static_cast<double *>(workspace), n, C, cin, p.per};
    hipLaunchKernelGGL(k_pe_moments, dim3(p.S, C / 64), dim3(256), 0, st, m);
    PTX_LAUNCHED("k_pe_moments");
    const PeFoldArgs f{static_cast<const double *>(workspace), w1, b1, gamma, beta, run_mean, run_var, w1f, b1f, stats, n, C, cin, p.per, p.S,
                       repeat, eps, momentum};
    hipLaunchKernelGGL(k_pe_fold, dim3(cdiv(C, 64)), dim3(64), 0, st, f);
    PTX_LAUNCHED("k_pe_fold");
    return PTX_OK;
}

int ptx_dec_posembed_hidden(const float *x, long n, int cin, const float *w1f, const float *b1f, int C, float *h, void *stream)
{
    const char *who = "ptx_dec_posembed_hidden";
    PTX_TRY(tr_rows_ok(who, n));
    PTX_REQUIRE(cin >= 1 && cin <= kTrMaxPos && sp_width_ok(C), "%s: cin=%d C=%d (cin: 1 to %d; C: a multiple of 64 up to 512)", who, cin, C,
                kTrMaxPos);
    PTX_REQUIRE(x && w1f && b1f && h, "%s: null argument", who);
    const long blocks = (n * C + 255) / 256;
    hipLaunchKernelGGL(k_pe_hidden, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, static_cast<hipStream_t>(stream), x, n, cin,
                       w1f, b1f, C, h);
    PTX_LAUNCHED("k_pe_hidden");
    return PTX_OK;
}

int ptx_dec_posembed_bwd(const float *x, long n, int cin, const float *w1, const float *b1, const float *gamma, const float *stats,
                         const float *w1f, const float *b1f, const float *dh, int C, float *dgb, float *dw1, float *db1, void *workspace,
                         size_t ws_bytes, void *stream)
{
    const char *who = "ptx_dec_posembed_bwd";
    PTX_TRY(tr_rows_ok(who, n));
    PTX_REQUIRE(cin >= 1 && cin <= kTrMaxPos && sp_width_ok(C), "%s: cin=%d C=%d (cin: 1 to %d; C: a multiple of 64 up to 512)", who, cin, C,
                kTrMaxPos);
    PTX_REQUIRE(x && w1 && b1 && gamma && stats && w1f && b1f && dh && dgb && dw1 && db1 && workspace, "%s: null argument", who);
    PTX_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "%s: the workspace must be 8-byte aligned", who);
    PTX_TRY(sp_workspace_fits(who, ws_bytes, ptx_dec_train_workspace_bytes(n, C, cin + 1 > 2 ? cin + 1 : 2)));
    const TrPlan p = tr_plan(n);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double *ws = static_cast<double *>(workspace);
    TrSlabArgs a{};
    a.small = x; a.big = dh; a.w1 = w1; a.b1 = b1; a.w1f = w1f; a.b1f = b1f; a.gamma = gamma; a.stats = stats; a.dgb = dgb; a.ws = ws;
    a.n = n; a.C = C; a.na = cin; a.per = p.per;
    a.nv = 2;
    PTX_TRY(tr_slab_launch(TR_PE_SUMS, a, p.S, st));
    PTX_TRY(tr_finish_launch(ws, p.S, 2, C, 0, nullptr, dgb, st));
    a.nv = cin + 1;
    PTX_TRY(tr_slab_launch(TR_PE_DW1, a, p.S, st));
    PTX_TRY(tr_finish_launch(ws, p.S, cin + 1, C, cin, dw1, db1, st));
    return PTX_OK;
}

int ptx_dec_boxes_bwd(const float *h, const float *weight, const float *bias, int C, long n, const float *dboxes, float *dh, float *dp,
                      float *dweight, void *workspace, size_t ws_bytes, void *stream)
{
    const char *who = "ptx_dec_boxes_bwd";
    PTX_TRY(tr_rows_ok(who, n));
    PTX_REQUIRE(sp_width_ok(C), "%s: C=%d (a multiple of 64 up to 512)", who, C);
    PTX_REQUIRE(h && weight && dboxes && dh && dp && dweight && workspace, "%s: null argument", who);
    PTX_REQUIRE(sp_aligned16({h, dh}), "%s: h and dh must be 16-byte aligned", who);
    PTX_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "%s: the workspace must be 8-byte aligned", who);
    PTX_TRY(sp_workspace_fits(who, ws_bytes, ptx_dec_train_workspace_bytes(n, C, kHeadReg)));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const BoxBwdArgs b{h, weight, bias, dboxes, dh, dp, (int)n, C};
    hipLaunchKernelGGL(k_dec_boxes_bwd, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, st, b);
    PTX_LAUNCHED("k_dec_boxes_bwd");
    const TrPlan p = tr_plan(n);
    TrSlabArgs a{};
    a.small = dp; a.big = h; a.ws = static_cast<double *>(workspace); a.n = n; a.C = C; a.na = kHeadReg; a.nv = kHeadReg; a.per = p.per;
    PTX_TRY(tr_slab_launch(TR_BOX_DW, a, p.S, st));
    PTX_TRY(tr_finish_launch(a.ws, p.S, kHeadReg, C, 0, nullptr, dweight, st));
    return PTX_OK;
}

int ptx_dec_scores_bwd(const float *dscores, const float *hidden, int NL, int B, int K, int C, const float *text, const uint8_t *text_mask,
                       int T, int max_text_len, int scaled, float *dhidden, float *dtext, float *dbias, void *workspace, size_t ws_bytes,
                       void *stream)
{
    const char *who = "ptx_dec_scores_bwd";
    PTX_REQUIRE(NL >= 1 && NL <= 64 && B >= 1 && B <= kHeadMaxScenes && K >= 1 && K <= kHeadMaxK && sp_width_ok(C),
                "%s: NL=%d B=%d K=%d C=%d (NL, B: 1 to 64; K: 1 to 1024; C: a multiple of 64 up to 512)", who, NL, B, K, C);
    PTX_REQUIRE(T >= 1 && T <= max_text_len && max_text_len <= kHeadMaxText && (scaled == 0 || scaled == 1),
                "%s: T=%d max_text_len=%d scaled=%d (1 <= T <= max_text_len <= %d; scaled: 0 or 1)", who, T, max_text_len, scaled, kHeadMaxText);
    PTX_REQUIRE(dscores && hidden && text && text_mask && dhidden && dtext && (dbias == nullptr || workspace != nullptr), "%s: null argument", who);
    PTX_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "%s: the workspace must be 8-byte aligned", who);
    if (dbias) PTX_TRY(sp_workspace_fits(who, ws_bytes, (size_t)NL * B * sizeof(double)));
    hipStream_t st = static_cast<hipStream_t>(stream);
    ScoreBwdArgs a{};
    a.ds = dscores; a.hidden = hidden; a.text = text; a.mask = text_mask; a.dhidden = dhidden; a.dtext = dtext;
    a.ws = static_cast<double *>(workspace); a.NL = NL; a.B = B; a.K = K; a.C = C; a.T = T; a.M = max_text_len; a.scaled = scaled;
    a.divisor = sqrtf((float)C);
    hipLaunchKernelGGL(k_dec_scores_dh, dim3(cdiv(K, 64), C / 64, NL * B), dim3(256), 0, st, a);
    PTX_LAUNCHED("k_dec_scores_dh");
    hipLaunchKernelGGL(k_dec_scores_dtext, dim3(cdiv(T, 64), C / 64, B), dim3(256), 0, st, a);
    PTX_LAUNCHED("k_dec_scores_dtext");
    if (dbias) {
        hipLaunchKernelGGL(k_dec_scores_dbias, dim3(NL * B), dim3(256), 0, st, a);
        PTX_LAUNCHED("k_dec_scores_dbias");
        PTX_TRY(tr_finish_launch(a.ws, NL * B, 1, 1, 0, nullptr, dbias, st));
    }
    return PTX_OK;
}

}  // extern "C"
