// Backward of the row operations of the sparse neck (neck.hip) -- what a loss behind `feats, scores, coords = self.neck_3d(x, batch_size)`
// needs to reach the backbone.  The reference prunes under torch.no_grad() (necks/mink_neck.py:163-186): the prune scores, the
// trilinear lookup and the top-k carry no gradient; the features and cls_preds do.
//
//   ptx_neck_rows_gather    out[i] = dest[i] >= 0 ? g[dest[i]] : +0.0, one thread per (row, 4 channels), 16-byte accesses.  It is the
//       backward of all three row routings: dA = g[a_dest] and dB = g[b_dest] of the union (ptx_neck_union_add_dest records the output
//       row of every input row; a matched pair reads the same row of g) and dU of the prune from the dest ptx_neck_topk_prune writes.
//       Pure copies: bit for bit.
//   ptx_neck_head_bwd       conv_cls (kernel 1, with bias) given dcls (n, K): dfeats = dcls @ W^T, one thread per (row, 4 channels), the
//       classes added in ascending order; dW (C, K) = feats^T @ dcls and dbias = sum_rows dcls as per-tile partials (256 rows: four
//       row groups of 64 rows each in ascending row order, the groups in ascending order) which k_neck_head_bwd_total adds in ascending
//       tile order.  These two contract over ALL rows into a handful of numbers (K of them for dbias): the products are exact in double
//       and the sums are kept in double, rounded to fp32 once at the end.  The prune score is detached, as in the reference.
//
// fp32, no float atomics, fixed summation orders (bitwise reproducible), everything on the caller's stream, no host wait.  Held to the
// numpy restatements of proxytransformation_amd/neck_host.py.
#include "sparse.h"

namespace ptx {

constexpr int kNeckHeadMaxClasses = 16;

__global__ __launch_bounds__(256) void k_neck_rows_gather(const float *__restrict__ g, const int32_t *__restrict__ dest, int n, int C, int n_src,
                                                          float *__restrict__ out)
{
    const int c4n = C >> 2;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const int r = (int)(t / c4n), c4 = (int)(t - (long)r * c4n);
    if (r >= n) return;
    const int d = dest[r];
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (d >= 0 && d < n_src) v = ld4(g + (size_t)d * C + c4 * 4);
    st4(out + (size_t)r * C + c4 * 4, v);
}

// one thread per (row, 4 channels): dfeats[row, c] = sum over ascending k of dcls[row, k] * W[c, k]
__global__ __launch_bounds__(256) void k_neck_head_dfeats(const float *__restrict__ dcls, const float *__restrict__ weight, int n, int C, int K,
                                                          float *__restrict__ dfeats)
{
    __shared__ __attribute__((aligned(16))) float s_w[kNeckHeadMaxClasses * 512];         // [class][channel]
    for (int e = threadIdx.x; e < C * K; e += 256) s_w[(e % K) * C + e / K] = weight[e];  // weight (C, K)
    __syncthreads();
    const int c4n = C >> 2;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const int r = (int)(t / c4n), c4 = (int)(t - (long)r * c4n);
    if (r >= n) return;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < K; ++k) {
        const float d = dcls[(size_t)r * K + k];
        const float4 w = ld4(&s_w[k * C + c4 * 4]);
        acc.x += d * w.x; acc.y += d * w.y; acc.z += d * w.z; acc.w += d * w.w;
    }
    st4(dfeats + (size_t)r * C + c4 * 4, acc);
}

// grid (tiles of 256 rows, C / 64).  part (tiles, C * K + K) double: the tile's feats^T @ dcls (C, K) and, behind it, its column sums of dcls (K;
// written by the work-groups with blockIdx.y == 0).  Thread = (channel = tid & 63, row group = tid >> 6): group q takes rows 64 q .. 64 q
// + 63 of the tile in ascending order; the four groups are added in ascending order
__global__ __launch_bounds__(256) void k_neck_head_dw(const float *__restrict__ feats, const float *__restrict__ dcls, int n, int C, int K,
                                                      double *__restrict__ part)
{
    __shared__ float s_d[256 * kNeckHeadMaxClasses];                                      // the tile's dcls, [row][class]
    __shared__ double s_p[4][kNeckHeadMaxClasses][64];
    const int tid = threadIdx.x, ch = tid & 63, q = tid >> 6;
    const int row0 = blockIdx.x * 256, cnt = min(256, n - row0);
    for (int e = tid; e < cnt * K; e += 256) s_d[e] = dcls[(size_t)row0 * K + e];
    __syncthreads();
    double acc[kNeckHeadMaxClasses];
#pragma unroll
    for (int k = 0; k < kNeckHeadMaxClasses; ++k) acc[k] = 0.0;
    const int c = blockIdx.y * 64 + ch;
    const int r1 = min(64 * q + 64, cnt);
    for (int r = 64 * q; r < r1; ++r) {
        const double x = (double)feats[(size_t)(row0 + r) * C + c];
#pragma unroll
        for (int k = 0; k < kNeckHeadMaxClasses; ++k) {
            if (k < K) acc[k] += x * (double)s_d[r * K + k];             // (the product of two floats is exact in double)
        }
    }
#pragma unroll
    for (int k = 0; k < kNeckHeadMaxClasses; ++k) s_p[q][k][ch] = acc[k];
    __syncthreads();
    double *dst = part + (size_t)blockIdx.x * ((size_t)C * K + K);
    for (int e = tid; e < 64 * K; e += 256) {
        const int k = e % K, cc = e / K;
        dst[(size_t)(blockIdx.y * 64 + cc) * K + k] = ((s_p[0][k][cc] + s_p[1][k][cc]) + s_p[2][k][cc]) + s_p[3][k][cc];
    }
    if (blockIdx.y == 0 && tid < K) {
        double s = 0.0;
        for (int r = 0; r < cnt; ++r) s += (double)s_d[r * K + tid];
        dst[(size_t)C * K + tid] = s;
    }
}

// one thread per element of (C * K + K): the tiles' partials added in ascending tile order in double, rounded once -> dweight (C, K),
// dbias (K), each optional
__global__ __launch_bounds__(256) void k_neck_head_bwd_total(const double *__restrict__ part, int T, int C, int K, float *__restrict__ dweight,
                                                             float *__restrict__ dbias)
{
    const int L = C * K + K;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= L) return;
    double s = 0.0;
    for (int t = 0; t < T; ++t) s += part[(size_t)t * L + e];
    if (e < C * K) {
        if (dweight) dweight[e] = (float)s;
    } else if (dbias) {
        dbias[e - C * K] = (float)s;
    }
}

static bool head_bwd_ok(int n, int C, int K) { return n >= 0 && n <= (1 << 30) && sp_width_ok(C) && K >= 1 && K <= kNeckHeadMaxClasses; }

}  // namespace ptx

using namespace ptx;

extern "C" {

int ptx_neck_rows_gather(const float *g, int n_src, const int32_t *dest, int n, int C, float *out, void *stream)
{
    const char *who = "ptx_neck_rows_gather";
    PTX_REQUIRE(n >= 0 && n <= (1 << 30) && n_src >= 0 && n_src <= (1 << 30) && C >= 4 && C <= 4096 && C % 4 == 0,
                "%s: n_src=%d n=%d C=%d (rows: up to 2^30; C: a multiple of 4 up to 4096)", who, n_src, n, C);
    if (n == 0) return PTX_OK;                              // zero rows: no launch
    PTX_REQUIRE(dest && out && (g || n_src == 0), "%s: null argument", who);
    PTX_REQUIRE(sp_aligned16({g, out}), "%s: g and out must be 16-byte aligned", who);
    PTX_TRY(sp_rows_fit(who, n, C));
    const long threads = (long)n * (C / 4);
    hipLaunchKernelGGL(k_neck_rows_gather, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), g, dest, n, C,
                       n_src, out);
    PTX_LAUNCHED("k_neck_rows_gather");
    return PTX_OK;
}

size_t ptx_neck_head_bwd_workspace_bytes(int n, int C, int num_classes)
{
    if (!head_bwd_ok(n, C, num_classes)) return 0;
    return align_up((size_t)cdiv(n > 0 ? n : 1, 256) * ((size_t)C * num_classes + num_classes) * sizeof(double), 256);
}

int ptx_neck_head_bwd(const float *dcls, const float *feats, const float *weight, int n, int C, int num_classes, float *dfeats, float *dweight,
                      float *dbias, void *workspace, size_t ws_bytes, void *stream)
{
    const char *who = "ptx_neck_head_bwd";
    const int K = num_classes;
    PTX_REQUIRE(head_bwd_ok(n, C, K), "%s: n=%d C=%d num_classes=%d (C: a multiple of 64 up to 512; num_classes: 1 to %d)", who, n, C, K,
                kNeckHeadMaxClasses);
    PTX_REQUIRE((dcls || n == 0) && (!dfeats || weight || n == 0) && (!(dweight || dbias) || feats || n == 0),
                "%s: null argument (dcls; weight for dfeats; feats for dweight / dbias)", who);
    PTX_REQUIRE(sp_aligned16({feats, dfeats, workspace}), "%s: feats, dfeats and the workspace must be 16-byte aligned", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n > 0 && dfeats) {
        PTX_TRY(sp_rows_fit(who, n, C));
        const long threads = (long)n * (C / 4);
        hipLaunchKernelGGL(k_neck_head_dfeats, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, dcls, weight, n, C, K, dfeats);
        PTX_LAUNCHED("k_neck_head_dfeats");
    }
    if (!dweight && !dbias) return PTX_OK;
    if (n == 0) {
        if (dweight) PTX_HIP(hipMemsetAsync(dweight, 0, (size_t)C * K * sizeof(float), st));
        if (dbias) PTX_HIP(hipMemsetAsync(dbias, 0, (size_t)K * sizeof(float), st));
        return PTX_OK;
    }
    PTX_REQUIRE(workspace, "%s: workspace is null", who);
    PTX_TRY(sp_workspace_fits(who, ws_bytes, ptx_neck_head_bwd_workspace_bytes(n, C, K)));
    const int T = cdiv(n, 256);
    double *part = static_cast<double *>(workspace);
    hipLaunchKernelGGL(k_neck_head_dw, dim3(T, C / 64), dim3(256), 0, st, feats, dcls, n, C, K, part);
    PTX_LAUNCHED("k_neck_head_dw");
    hipLaunchKernelGGL(k_neck_head_bwd_total, dim3(cdiv(C * K + K, 256)), dim3(256), 0, st, static_cast<const double *>(part), T, C, K, dweight,
                       dbias);
    PTX_LAUNCHED("k_neck_head_bwd_total");
    return PTX_OK;
}

}  // extern "C"
