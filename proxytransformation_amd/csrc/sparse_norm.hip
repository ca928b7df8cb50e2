// Instance norm / training batch norm on the voxel rows: column moments per row segment -> normalise -> affine (+ residual)(+ ReLU),
// forward and backward -- MinkowskiInstanceNorm (mink_resnet.py:67, segments = scenes) and a training MinkowskiBatchNorm (one segment
// over all rows) are the same kernels.
//
// Rows x (n, C) fp32, C a multiple of 64 up to 512; segments as a host array of ends (ptx_sparse_kernel_map's in_scene_end).  The rows
// are cut into tiles of 256 that never straddle a segment; the host passes the tile prefix of every segment in the kernel arguments and
// a work-group finds its segment from them.  The streaming idiom and its helpers: sparse.h.
//
//   forward   k_sparse_norm_stats     per tile and column (mean, M2 about the tile's own mean): the tile's 16 rows per thread stay in
//                                     registers between the two sums; row slots added in ascending order;
//             k_sparse_norm_finalise  a segment's tiles merged with Chan's formula: 16 slots take contiguous runs of tiles in
//                                     ascending order, then the slots in ascending order; writes stats (mean, rstd) and, for a
//                                     training batch norm, the running statistics (unbiased variance M2 / (n - 1));
//             k_sparse_norm_apply     out = relu?(((x - mean) * rstd) * weight + bias (+ residual)): x read once, out written once.
//   backward  k_sparse_norm_bwd_sums  gy = g * [out > 0]; per tile and column sum gy and sum gy * xhat (xhat recomputed from x and
//                                     stats); dresidual = gy written here when asked for;
//             k_sparse_norm_bwd_finalise  per segment a = mean gy, b = mean gy * xhat (tiles in the same blocked ascending order);
//                                     dbias / dweight = the segments' sums in ascending order;
//             k_sparse_norm_bwd_apply dx = weight * rstd * ((gy - a) - xhat * b).
//
// The _act entry points (the neck's training BatchNorms) put an activation selector in the place of the ReLU flag: 0 none, 1 ReLU,
// 2 ELU with alpha = 1, v > 0 ? v : expm1f(v).  Backward of the ELU from the saved result: gy = g * (out > 0 ? 1 : out + 1) -- a NaN out
// gives a NaN gy and is never dropped.  Selectors 0 and 1 run the instantiations the older entry points run.
//
// No float atomics, a fixed order everywhere: two calls on the same inputs give the same bits.  The variance is never E[x^2] - E[x]^2.
// Everything runs on the caller's stream; no host wait.
#include "sparse.h"

namespace ptx {

constexpr int kSnMaxSeg = 64;

struct SnSegs {
    int S;
    int end[kSnMaxSeg];                    // end of every segment's rows
    int tile0[kSnMaxSeg + 1];              // tiles before every segment; tile0[S] = all tiles
};

struct SnTile { int seg, row0, cnt; };

// work-group uniform: the segment of tile `tile` (< sg.tile0[sg.S]), its first row and its rows (1 .. 256)
__device__ __forceinline__ SnTile sn_locate(const SnSegs &sg, int tile)
{
    int s = 0;
    while (s + 1 < sg.S && tile >= sg.tile0[s + 1]) ++s;
    const int start = s ? sg.end[s - 1] : 0;
    SnTile t;
    t.seg = s;
    t.row0 = start + (tile - sg.tile0[s]) * kSpTile;
    t.cnt = min(kSpTile, sg.end[s] - t.row0);
    return t;
}

// ---- forward ----------------------------------------------------------------------------------------------------------------------
// grid (tiles, C / 64).  part (tiles, 2, C): the tile's mean and its M2 about that mean
__global__ __launch_bounds__(256) void k_sparse_norm_stats(const float *__restrict__ x, SnSegs sg, int C, float *__restrict__ part)
{
    __shared__ __attribute__((aligned(16))) float s_red[16][64];
    __shared__ __attribute__((aligned(16))) float s_mean[64];
    const int tid = threadIdx.x, c4 = tid & 15, slot = tid >> 4;
    const int col = blockIdx.y * 64 + c4 * 4;
    const SnTile t = sn_locate(sg, blockIdx.x);
    float4 v[kSpTile / 16];
    float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < kSpTile / 16; ++i) {
        const int r = slot + 16 * i;
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < t.cnt) v[i] = ld4(x + (size_t)(t.row0 + r) * C + col);
        acc4(sum, v[i]);
    }
    st4(&s_red[slot][c4 * 4], sum);
    __syncthreads();
    if (tid < 64) s_mean[tid] = slots16(s_red, tid) / (float)t.cnt;
    __syncthreads();
    const float4 m = ld4(&s_mean[c4 * 4]);
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < kSpTile / 16; ++i) {
        if (slot + 16 * i < t.cnt) {
            const float4 d = sub4(v[i], m);
            mac4(q, d, d);
        }
    }
    st4(&s_red[slot][c4 * 4], q);                           // (every read of the first sums lies before the second barrier)
    __syncthreads();
    if (tid < 64) {
        float *dst = part + (size_t)blockIdx.x * 2 * C + blockIdx.y * 64 + tid;
        dst[0] = s_mean[tid];
        dst[C] = slots16(s_red, tid);
    }
}

// Chan et al.: (n, mean, M2) += (nb, mb, qb)
__device__ __forceinline__ void sn_merge(int &n, float &mean, float &m2, int nb, float mb, float qb)
{
    const int nt = n + nb;
    const float f = (float)nb / (float)nt, d = mb - mean;
    m2 += qb + (d * d) * ((float)n * f);
    mean += d * f;
    n = nt;
}

// grid (S, C / 64).  stats (S, 2, C) = (mean, 1 / sqrt(M2 / n + eps)); an empty segment: (0, 0).  run_mean / run_var (C), both or
// neither, S == 1 and n >= 2 (the host checks): (1 - momentum) * old + momentum * (mean, M2 / (n - 1))
__global__ __launch_bounds__(256) void k_sparse_norm_finalise(const float *__restrict__ part, SnSegs sg, int C, float eps,
                                                              float *__restrict__ stats, float *__restrict__ run_mean,
                                                              float *__restrict__ run_var, float momentum)
{
    __shared__ __attribute__((aligned(16))) float s_mean[16][64];
    __shared__ __attribute__((aligned(16))) float s_m2[16][64];
    __shared__ int s_n[16];
    const int tid = threadIdx.x, c4 = tid & 15, slot = tid >> 4;
    const int col = blockIdx.y * 64 + c4 * 4;
    const int s = blockIdx.x;
    const int n = sg.end[s] - (s ? sg.end[s - 1] : 0);
    const int t0 = sg.tile0[s], nt = sg.tile0[s + 1] - t0;
    const int per = (nt + 15) >> 4;
    const int ta = min(slot * per, nt), tb = min(ta + per, nt);
    int cn = 0;
    float4 mean = make_float4(0.f, 0.f, 0.f, 0.f), m2 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t = ta; t < tb; ++t) {
        const int nb = min(kSpTile, n - t * kSpTile);
        const float *src = part + (size_t)(t0 + t) * 2 * C + col;
        const float4 pm = ld4(src), pq = ld4(src + C);
        int k;
        k = cn; sn_merge(k, mean.x, m2.x, nb, pm.x, pq.x);
        k = cn; sn_merge(k, mean.y, m2.y, nb, pm.y, pq.y);
        k = cn; sn_merge(k, mean.z, m2.z, nb, pm.z, pq.z);
        k = cn; sn_merge(k, mean.w, m2.w, nb, pm.w, pq.w);
        cn = k;
    }
    st4(&s_mean[slot][c4 * 4], mean);
    st4(&s_m2[slot][c4 * 4], m2);
    if (c4 == 0) s_n[slot] = cn;
    __syncthreads();
    if (tid < 64) {
        int k = 0;
        float mu = 0.0f, q = 0.0f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (s_n[i] > 0) sn_merge(k, mu, q, s_n[i], s_mean[i][tid], s_m2[i][tid]);
        }
        const int c = blockIdx.y * 64 + tid;
        float *dst = stats + (size_t)s * 2 * C + c;
        dst[0] = n > 0 ? mu : 0.0f;
        dst[C] = n > 0 ? 1.0f / sqrtf(q / (float)n + eps) : 0.0f;
        if (run_mean != nullptr && n > 1) {
            run_mean[c] = (1.0f - momentum) * run_mean[c] + momentum * mu;
            run_var[c] = (1.0f - momentum) * run_var[c] + momentum * (q / (float)(n - 1));
        }
    }
}

// d *= (o > 0 ? 1 : o + 1): the gradient behind an ELU (alpha = 1) whose result was o; a NaN o makes d NaN
__device__ __forceinline__ void elu_mask4(float4 &d, const float4 &o)
{
    d.x = o.x > 0.0f ? d.x : d.x * (o.x + 1.0f); d.y = o.y > 0.0f ? d.y : d.y * (o.y + 1.0f);
    d.z = o.z > 0.0f ? d.z : d.z * (o.z + 1.0f); d.w = o.w > 0.0f ? d.w : d.w * (o.w + 1.0f);
}

// grid (tiles, C / 64).  weight / bias (C) and residual (n, C) each optional.  ELU: the activation is the ELU, `relu` is not read
template <bool ELU>
__global__ __launch_bounds__(256) void k_sparse_norm_apply(const float *__restrict__ x, SnSegs sg, int C, const float *__restrict__ stats,
                                                           const float *__restrict__ weight, const float *__restrict__ bias,
                                                           const float *__restrict__ residual, int relu, float *__restrict__ out)
{
    const int tid = threadIdx.x, c4 = tid & 15, slot = tid >> 4;
    const int col = blockIdx.y * 64 + c4 * 4;
    const SnTile t = sn_locate(sg, blockIdx.x);
    const float4 mu = ld4(stats + (size_t)t.seg * 2 * C + col), rs = ld4(stats + (size_t)t.seg * 2 * C + C + col);
    float4 w = make_float4(1.f, 1.f, 1.f, 1.f), b = make_float4(0.f, 0.f, 0.f, 0.f);
    if (weight) w = ld4(weight + col);
    if (bias) b = ld4(bias + col);
#pragma unroll 4
    for (int i = 0; i < kSpTile / 16; ++i) {
        const int r = slot + 16 * i;
        if (r >= t.cnt) break;
        const size_t at = (size_t)(t.row0 + r) * C + col;
        const float4 v = ld4(x + at);
        float4 y = mul4(sub4(v, mu), rs);
        if (weight) scale4(y, w);
        if (bias) acc4(y, b);
        if (residual) acc4(y, ld4(residual + at));
        if (ELU) {
            y.x = y.x > 0.0f ? y.x : expm1f(y.x); y.y = y.y > 0.0f ? y.y : expm1f(y.y);
            y.z = y.z > 0.0f ? y.z : expm1f(y.z); y.w = y.w > 0.0f ? y.w : expm1f(y.w);
        } else if (relu) { y.x = fmaxf(y.x, 0.0f); y.y = fmaxf(y.y, 0.0f); y.z = fmaxf(y.z, 0.0f); y.w = fmaxf(y.w, 0.0f); }
        st4(out + at, y);
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------
// grid (tiles, C / 64).  part (tiles, 2, C): sum gy and sum gy * xhat of the tile; out: the forward's result when it had a ReLU, else
// null; dres (n, C) = gy, optional.  ELU: out is the result of an ELU, gy = g * (out > 0 ? 1 : out + 1)
template <bool ELU>
__global__ __launch_bounds__(256) void k_sparse_norm_bwd_sums(const float *__restrict__ g, const float *__restrict__ x,
                                                              const float *__restrict__ out, SnSegs sg, int C,
                                                              const float *__restrict__ stats, float *__restrict__ dres,
                                                              float *__restrict__ part)
{
    __shared__ __attribute__((aligned(16))) float s_a[16][64];
    __shared__ __attribute__((aligned(16))) float s_b[16][64];
    const int tid = threadIdx.x, c4 = tid & 15, slot = tid >> 4;
    const int col = blockIdx.y * 64 + c4 * 4;
    const SnTile t = sn_locate(sg, blockIdx.x);
    const float4 mu = ld4(stats + (size_t)t.seg * 2 * C + col), rs = ld4(stats + (size_t)t.seg * 2 * C + C + col);
    float4 sa = make_float4(0.f, 0.f, 0.f, 0.f), sb = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
    for (int i = 0; i < kSpTile / 16; ++i) {
        const int r = slot + 16 * i;
        if (r >= t.cnt) break;
        const size_t at = (size_t)(t.row0 + r) * C + col;
        float4 d = ld4(g + at);
        if (out) {
            if (ELU) elu_mask4(d, ld4(out + at));
            else relu_mask4(d, ld4(out + at));
        }
        if (dres) st4(dres + at, d);
        const float4 v = ld4(x + at);
        sa = add4(sa, d);
        mac4(sb, d, mul4(sub4(v, mu), rs));
    }
    st4(&s_a[slot][c4 * 4], sa);
    st4(&s_b[slot][c4 * 4], sb);
    __syncthreads();
    if (tid < 64) {
        float *dst = part + (size_t)blockIdx.x * 2 * C + blockIdx.y * 64 + tid;
        dst[0] = slots16(s_a, tid);
        dst[C] = slots16(s_b, tid);
    }
}

// grid (S, C / 64), k_sparse_norm_finalise's shape.  seg (S, 2, C) = (a, b) = the segment's sums / its rows; tot (S, 2, C) = the sums
// themselves, for k_sparse_norm_bwd_total -- with one segment they ARE dbias / dweight (C), each optional, and are written here.  A
// segment's tiles: 16 slots take contiguous runs in ascending order, then the slots in ascending order
__global__ __launch_bounds__(256) void k_sparse_norm_bwd_finalise(const float *__restrict__ part, SnSegs sg, int C, float *__restrict__ seg,
                                                                  float *__restrict__ tot, float *__restrict__ dbias,
                                                                  float *__restrict__ dweight)
{
    __shared__ __attribute__((aligned(16))) float s_a[16][64];
    __shared__ __attribute__((aligned(16))) float s_b[16][64];
    const int tid = threadIdx.x, c4 = tid & 15, slot = tid >> 4;
    const int col = blockIdx.y * 64 + c4 * 4;
    const int s = blockIdx.x;
    const int n = sg.end[s] - (s ? sg.end[s - 1] : 0);
    const int t0 = sg.tile0[s], nt = sg.tile0[s + 1] - t0;
    const int per = (nt + 15) >> 4;
    const int ta = min(slot * per, nt), tb = min(ta + per, nt);
    float4 sa = make_float4(0.f, 0.f, 0.f, 0.f), sb = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t = ta; t < tb; ++t) {
        const float *src = part + (size_t)(t0 + t) * 2 * C + col;
        const float4 pa = ld4(src), pb = ld4(src + C);
        acc4(sa, pa);
        acc4(sb, pb);
    }
    st4(&s_a[slot][c4 * 4], sa);
    st4(&s_b[slot][c4 * 4], sb);
    __syncthreads();
    if (tid < 64) {
        const float a = slots16(s_a, tid), b = slots16(s_b, tid);
        const int c = blockIdx.y * 64 + tid;
        const size_t at = (size_t)s * 2 * C + c;
        seg[at] = n > 0 ? a / (float)n : 0.0f;
        seg[at + C] = n > 0 ? b / (float)n : 0.0f;
        if (sg.S > 1) {
            tot[at] = a;
            tot[at + C] = b;
        } else {
            if (dbias) dbias[c] = a;
            if (dweight) dweight[c] = b;
        }
    }
}

// grid C / 64, 64 threads; S > 1.  dbias / dweight (C), each optional = the segments' sums added in ascending order
__global__ __launch_bounds__(64) void k_sparse_norm_bwd_total(const float *__restrict__ tot, int S, int C, float *__restrict__ dbias,
                                                              float *__restrict__ dweight)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    float a = 0.0f, b = 0.0f;
    for (int s = 0; s < S; ++s) {
        a += tot[(size_t)s * 2 * C + c];
        b += tot[(size_t)s * 2 * C + C + c];
    }
    if (dbias) dbias[c] = a;
    if (dweight) dweight[c] = b;
}

// grid (tiles, C / 64).  gy: dresidual as k_sparse_norm_bwd_sums wrote it (then g / out are not read), else null
template <bool ELU>
__global__ __launch_bounds__(256) void k_sparse_norm_bwd_apply(const float *__restrict__ g, const float *__restrict__ x,
                                                               const float *__restrict__ out, const float *__restrict__ gy, SnSegs sg,
                                                               int C, const float *__restrict__ stats, const float *__restrict__ seg,
                                                               const float *__restrict__ weight, float *__restrict__ dx)
{
    const int tid = threadIdx.x, c4 = tid & 15, slot = tid >> 4;
    const int col = blockIdx.y * 64 + c4 * 4;
    const SnTile t = sn_locate(sg, blockIdx.x);
    const size_t so = (size_t)t.seg * 2 * C + col;
    const float4 mu = ld4(stats + so), rs = ld4(stats + so + C), a = ld4(seg + so), b = ld4(seg + so + C);
    float4 k = rs;                                          // weight * rstd
    if (weight) k = mul4(ld4(weight + col), rs);
#pragma unroll 4
    for (int i = 0; i < kSpTile / 16; ++i) {
        const int r = slot + 16 * i;
        if (r >= t.cnt) break;
        const size_t at = (size_t)(t.row0 + r) * C + col;
        float4 d;
        if (gy) {
            d = ld4(gy + at);
        } else {
            d = ld4(g + at);
            if (out) {
                if (ELU) elu_mask4(d, ld4(out + at));
                else relu_mask4(d, ld4(out + at));
            }
        }
        const float4 v = ld4(x + at);
        st4(dx + at, mul4(k, sub4(sub4(d, a), mul4(mul4(sub4(v, mu), rs), b))));
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
struct SnPlan { size_t part_bytes, seg_bytes, total; };
// a function of the shapes only: at most n / 256 + S tiles
static SnPlan sn_plan(int n, int S, int C)
{
    SnPlan P{};
    P.part_bytes = align_up(((size_t)n / kSpTile + (size_t)S) * 2 * C * sizeof(float), 256);
    P.seg_bytes = align_up((size_t)S * 2 * C * sizeof(float), 256);
    P.total = P.part_bytes + 2 * P.seg_bytes + 256;         // the tile partials, the segments' means, the segments' sums
    return P;
}

// the segment table of a call; PTX_EINVAL with a message when the ends are not a partition of the n rows
static int sn_segments(const char *who, const int32_t *seg_end, int S, int n, int C, SnSegs &sg)
{
    PTX_REQUIRE(n >= 0 && S >= 1 && S <= kSnMaxSeg && sp_width_ok(C), "%s: n=%d S=%d C=%d (S: 1 to 64 segments; C: a multiple of 64 up to 512)",
                who, n, S, C);
    PTX_REQUIRE(seg_end != nullptr, "%s: seg_end is null", who);
    sg.S = S;
    sg.tile0[0] = 0;
    int prev = 0;
    for (int s = 0; s < S; ++s) {
        PTX_REQUIRE(seg_end[s] >= prev && seg_end[s] <= n, "%s: seg_end[%d] = %d after %d with n = %d (ends must ascend up to n)", who, s,
                    seg_end[s], prev, n);
        sg.end[s] = seg_end[s];
        sg.tile0[s + 1] = sg.tile0[s] + cdiv(seg_end[s] - prev, kSpTile);
        prev = seg_end[s];
    }
    PTX_REQUIRE(prev == n, "%s: seg_end[%d] = %d, but there are n = %d rows", who, S - 1, prev, n);
    for (int s = S; s < kSnMaxSeg; ++s) sg.end[s] = n, sg.tile0[s + 1] = sg.tile0[S];
    return PTX_OK;
}

}  // namespace ptx

using namespace ptx;

// both forward entry points (act: 0 none, 1 ReLU, 2 ELU) and both backward ones; `who` names the one that was called in its messages
static int sn_fwd(const char *who, const float *x, const int32_t *seg_end, int S, int n, int C, float eps, const float *weight, const float *bias,
                        const float *residual, int act, float *running_mean, float *running_var, float momentum, float *stats, float *out,
                        void *workspace, size_t ws_bytes, void *stream)
{
    SnSegs sg;
    PTX_TRY(sn_segments(who, seg_end, S, n, C, sg));
    PTX_REQUIRE(eps >= 0.0f && eps < 1.0f, "%s: eps = %g is outside [0, 1)", who, (double)eps);
    PTX_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "%s: running_mean and running_var go together", who);
    if (running_mean) {
        PTX_REQUIRE(S == 1 && n >= 2, "%s: running statistics need one segment of at least 2 rows, got S=%d n=%d", who, S, n);
        PTX_REQUIRE(momentum >= 0.0f && momentum <= 1.0f, "%s: momentum = %g is outside [0, 1]", who, (double)momentum);
    }
    PTX_REQUIRE(stats != nullptr && ((x && out) || n == 0), "%s: null argument (x, out and stats are needed)", who);
    PTX_REQUIRE(sp_aligned16({x, weight, bias, residual, stats, out, workspace}),
                "%s: every float buffer and the workspace must be 16-byte aligned", who);
    const SnPlan P = sn_plan(n, S, C);
    const int T = sg.tile0[S];
    if (T > 0) {
        PTX_REQUIRE(workspace, "%s: workspace is null", who);
        PTX_TRY(sp_workspace_fits(who, ws_bytes, P.total));
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *part = static_cast<float *>(workspace);
    if (T > 0) {
        hipLaunchKernelGGL(k_sparse_norm_stats, dim3(T, C / 64), dim3(256), 0, st, x, sg, C, part);
        PTX_LAUNCHED("k_sparse_norm_stats");
    }
    hipLaunchKernelGGL(k_sparse_norm_finalise, dim3(S, C / 64), dim3(256), 0, st, part, sg, C, eps, stats, running_mean, running_var, momentum);
    PTX_LAUNCHED("k_sparse_norm_finalise");
    if (T > 0) {
        if (act == 2)
            hipLaunchKernelGGL(k_sparse_norm_apply<true>, dim3(T, C / 64), dim3(256), 0, st, x, sg, C, stats, weight, bias, residual, 0, out);
        else
            hipLaunchKernelGGL(k_sparse_norm_apply<false>, dim3(T, C / 64), dim3(256), 0, st, x, sg, C, stats, weight, bias, residual, act != 0, out);
        PTX_LAUNCHED("k_sparse_norm_apply");
    }
    return PTX_OK;
}

static int sn_bwd(const char *who, bool elu, const float *g, const float *x, const float *out, const int32_t *seg_end, int S, int n, int C,
                  const float *stats, const float *weight, float *dx, float *dweight, float *dbias, float *dresidual, void *workspace,
                  size_t ws_bytes, void *stream)
{
    SnSegs sg;
    PTX_TRY(sn_segments(who, seg_end, S, n, C, sg));
    PTX_REQUIRE(stats != nullptr && ((g && x) || n == 0), "%s: null argument (g, x and stats are needed)", who);
    PTX_REQUIRE(sp_aligned16({g, x, out, stats, weight, dx, dweight, dbias, dresidual, workspace}),
                "%s: every float buffer and the workspace must be 16-byte aligned", who);
    const SnPlan P = sn_plan(n, S, C);
    PTX_REQUIRE(workspace, "%s: workspace is null", who);
    PTX_TRY(sp_workspace_fits(who, ws_bytes, P.total));
    const int T = sg.tile0[S];
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *part = static_cast<float *>(workspace);
    float *seg = reinterpret_cast<float *>(static_cast<char *>(workspace) + P.part_bytes);
    float *tot = reinterpret_cast<float *>(static_cast<char *>(workspace) + P.part_bytes + P.seg_bytes);
    const bool sums = dx != nullptr || dweight != nullptr || dbias != nullptr;
    if (T > 0 && (sums || dresidual)) {
        if (elu) hipLaunchKernelGGL(k_sparse_norm_bwd_sums<true>, dim3(T, C / 64), dim3(256), 0, st, g, x, out, sg, C, stats, dresidual, part);
        else hipLaunchKernelGGL(k_sparse_norm_bwd_sums<false>, dim3(T, C / 64), dim3(256), 0, st, g, x, out, sg, C, stats, dresidual, part);
        PTX_LAUNCHED("k_sparse_norm_bwd_sums");
    }
    if (sums) {
        hipLaunchKernelGGL(k_sparse_norm_bwd_finalise, dim3(S, C / 64), dim3(256), 0, st, part, sg, C, seg, tot, dbias, dweight);
        PTX_LAUNCHED("k_sparse_norm_bwd_finalise");
        if (S > 1 && (dbias || dweight)) {
            hipLaunchKernelGGL(k_sparse_norm_bwd_total, dim3(C / 64), dim3(64), 0, st, static_cast<const float *>(tot), S, C, dbias, dweight);
            PTX_LAUNCHED("k_sparse_norm_bwd_total");
        }
    }
    if (T > 0 && dx) {
        if (elu)
            hipLaunchKernelGGL(k_sparse_norm_bwd_apply<true>, dim3(T, C / 64), dim3(256), 0, st, g, x, out, static_cast<const float *>(dresidual), sg,
                               C, stats, seg, weight, dx);
        else
            hipLaunchKernelGGL(k_sparse_norm_bwd_apply<false>, dim3(T, C / 64), dim3(256), 0, st, g, x, out, static_cast<const float *>(dresidual), sg,
                               C, stats, seg, weight, dx);
        PTX_LAUNCHED("k_sparse_norm_bwd_apply");
    }
    return PTX_OK;
}


extern "C" {

size_t ptx_sparse_norm_workspace_bytes(int n, int S, int C)
{
    if (n < 0 || S < 1 || S > kSnMaxSeg || !sp_width_ok(C)) return 0;
    return sn_plan(n, S, C).total;
}

int ptx_sparse_norm_fwd(const float *x, const int32_t *seg_end, int S, int n, int C, float eps, const float *weight, const float *bias,
                        const float *residual, int relu, float *running_mean, float *running_var, float momentum, float *stats, float *out,
                        void *workspace, size_t ws_bytes, void *stream)
{
    return sn_fwd("ptx_sparse_norm_fwd", x, seg_end, S, n, C, eps, weight, bias, residual, relu != 0, running_mean, running_var, momentum, stats, out,
                  workspace, ws_bytes, stream);
}

int ptx_sparse_norm_fwd_act(const float *x, const int32_t *seg_end, int S, int n, int C, float eps, const float *weight, const float *bias,
                            const float *residual, int act, float *running_mean, float *running_var, float momentum, float *stats, float *out,
                            void *workspace, size_t ws_bytes, void *stream)
{
    PTX_REQUIRE(act >= 0 && act <= 2, "ptx_sparse_norm_fwd_act: act=%d (0 none, 1 ReLU, 2 ELU)", act);
    return sn_fwd("ptx_sparse_norm_fwd_act", x, seg_end, S, n, C, eps, weight, bias, residual, act, running_mean, running_var, momentum, stats, out,
                  workspace, ws_bytes, stream);
}

int ptx_sparse_norm_apply(const float *x, const int32_t *seg_end, int S, int n, int C, const float *stats, const float *weight,
                          const float *bias, const float *residual, int relu, float *out, void *stream)
{
    SnSegs sg;
    PTX_TRY(sn_segments("ptx_sparse_norm_apply", seg_end, S, n, C, sg));
    PTX_REQUIRE(stats != nullptr && ((x && out) || n == 0), "ptx_sparse_norm_apply: null argument (x, stats and out are needed)");
    PTX_REQUIRE(sp_aligned16({x, weight, bias, residual, stats, out}), "ptx_sparse_norm_apply: every float buffer must be 16-byte aligned");
    const int T = sg.tile0[S];
    if (T == 0) return PTX_OK;
    hipLaunchKernelGGL(k_sparse_norm_apply<false>, dim3(T, C / 64), dim3(256), 0, static_cast<hipStream_t>(stream), x, sg, C, stats, weight, bias,
                       residual, relu != 0, out);
    PTX_LAUNCHED("k_sparse_norm_apply");
    return PTX_OK;
}

int ptx_sparse_norm_bwd(const float *g, const float *x, const float *out, const int32_t *seg_end, int S, int n, int C, const float *stats,
                        const float *weight, float *dx, float *dweight, float *dbias, float *dresidual, void *workspace, size_t ws_bytes,
                        void *stream)
{
    return sn_bwd("ptx_sparse_norm_bwd", false, g, x, out, seg_end, S, n, C, stats, weight, dx, dweight, dbias, dresidual, workspace, ws_bytes, stream);
}

int ptx_sparse_norm_bwd_act(const float *g, const float *x, const float *out, int act, const int32_t *seg_end, int S, int n, int C,
                            const float *stats, const float *weight, float *dx, float *dweight, float *dbias, float *dresidual, void *workspace,
                            size_t ws_bytes, void *stream)
{
    PTX_REQUIRE(act >= 0 && act <= 2, "ptx_sparse_norm_bwd_act: act=%d (0 none, 1 ReLU, 2 ELU)", act);
    PTX_REQUIRE(act == 0 || out != nullptr || n == 0, "ptx_sparse_norm_bwd_act: act=%d needs the forward's out", act);
    return sn_bwd("ptx_sparse_norm_bwd_act", act == 2, g, x, act ? out : nullptr, seg_end, S, n, C, stats, weight, dx, dweight, dbias, dresidual,
                  workspace, ws_bytes, stream);
}

}  // extern "C"
