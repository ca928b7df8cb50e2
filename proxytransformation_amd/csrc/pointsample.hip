// Image feature -> point sampling: batch_point_sample of the reference
// (models/layers/fusion_layers/point_fusion.py:208-313) as its detector calls it after the sparse backbone
// (detectors/sparse_featfusion_grounder_preshape.py:428-444: aligned=False -> nearest, zeros padding, align_corners=True,
// valid_flag=True): every point is projected into all V views, the nearest feature-map pixel of every view is gathered,
// the samples are summed and divided by the number of views in which the point is inside the (padded) image with
// positive depth.
//
// Layout: the feature maps arrive channels-first (V,C,H,W); gathering C channels of one pixel from that layout touches C
// cache lines.  k_feat_transpose makes one channels-last copy (V,H*W,C) (HBM-bound, V*C*H*W*4 B each way, caller-owned
// workspace); k_point_sample then runs one wave per point: lanes = views for the projection (ballot of the views that
// hit a pixel), lanes = channels for the gather (256 B contiguous per view and 64 channels).
#include "common.h"
#include "imgstore.h"
#include "pointsample.h"

namespace ptx {

// (V, C, HW) -> (V, HW, C), 32 x 32 tiles through LDS
__global__ __launch_bounds__(256) void k_feat_transpose(const void *__restrict__ in, int dt, int C, int HW, float *__restrict__ out)
{
    __shared__ float tile[32][33];
    const int v = blockIdx.z, c0 = blockIdx.y * 32, p0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;             // 32 x 8
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int c = c0 + ty + 8 * r, p = p0 + tx;
        tile[ty + 8 * r][tx] = (c < C && p < HW) ? img_load(in, ((size_t)v * C + c) * HW + p, dt) : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int p = p0 + ty + 8 * r, c = c0 + tx;
        if (p < HW && c < C) out[((size_t)v * HW + p) * C + c] = tile[tx][ty + 8 * r];
    }
}

__global__ __launch_bounds__(256) void k_point_sample(PsArgs a)
{
    const int n = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (n >= a.N) return;
    const int lane = lane_id();
    float x, y, z;
    ps_point(a, n, x, y, z);
    ps_pre(a.pre, x, y, z);
    float acc[kPsMaxQ];
    const int nvalid = ps_accumulate(a, x, y, z, lane, acc);
    const float den = (float)(nvalid > 1 ? nvalid : 1);
#pragma unroll
    for (int q = 0; q < kPsMaxQ; ++q) {
        const int c = lane + 64 * q;
        if (c < a.C) a.out[(size_t)n * a.C + c] = nvalid > 0 ? __fdiv_rn(acc[q], den) : 0.0f;
    }
    if (a.valid_num && lane == 0) a.valid_num[n] = nvalid;
}

// ---------------------------------------------------------------------------------------------------------------- backward
// out = A f is linear in the feature maps, so dfeat = A^T dout:  dfeat[v, c, y, x] = sum over the (point, view) pairs that
// land on that pixel of  w * (dout[n, c] / valid_num[n])  (the reference's own graph: the division's backward, then
// grid_sample's).  No float atomics: an inverted index per (view, pixel) is built from the geometry alone -- integer counts
// (k_psb_index<false>), a scan (k_psb_scan, k_psb_scan_top), a fill (k_psb_index<true>) -- every list is put in ascending point
// order (k_psb_order; a point reaches a pixel of a view through at most one neighbour), and k_point_sample_grad writes every
// element of the channels-first gradient exactly once, the sum of its list in that order (zeros where the list is empty).
constexpr int kPsbScan = 2048;          // elements per work-group of the scan: 256 threads x 8

struct PsbIndex {
    int32_t *cnt;           // (D + 1) hits per pixel, D = V * H * W: counted, then counted back down to 0 by the fill
    int32_t *off;           // (D + 1) exclusive scan of cnt inside its chunk of kPsbScan elements
    int32_t *bsum;          // exclusive scan of the chunk totals: list d starts at off[d] + bsum[d / kPsbScan]
    int2 *raw, *sorted;     // (n, bits of w) in arrival order / in ascending n
};
__device__ __forceinline__ int psb_start(const PsbIndex &ix, int d) { return ix.off[d] + ix.bsum[d / kPsbScan]; }

template <bool FILL>
__device__ __forceinline__ void psb_emit(const PsbIndex &ix, int d, int n, float w)
{
    if (!FILL) { atomicAdd(&ix.cnt[d], 1); return; }
    const int slot = atomicSub(&ix.cnt[d], 1) - 1;
    ix.raw[psb_start(ix, d) + slot] = make_int2(n, __float_as_int(w));
}

// one thread per (point, view); a.valid_num: the forward's divisor (points with none contribute nothing)
template <bool FILL>
__global__ __launch_bounds__(256) void k_psb_index(PsArgs a, PsbIndex ix)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int n = (int)(i / a.V), v = (int)(i % a.V);
    if (n >= a.N || a.valid_num[n] <= 0) return;
    float x, y, z;
    ps_point(a, n, x, y, z);
    ps_pre(a.pre, x, y, z);
    const PsHit h = ps_project(a, x, y, z, v);
    if (!h.inb) return;
    const int d0 = v * a.H * a.W;
    if (!a.bilinear) { psb_emit<FILL>(ix, d0 + h.pix, n, 1.0f); return; }
    const float gx = __fsub_rn(1.0f, h.wx1), gy = __fsub_rn(1.0f, h.wy1);
    const float w[4] = {__fmul_rn(gx, gy), __fmul_rn(h.wx1, gy), __fmul_rn(gx, h.wy1), __fmul_rn(h.wx1, h.wy1)};   // as the forward
#pragma unroll
    for (int k = 0; k < 4; ++k) {                               // nw, ne, sw, se
        const int xx = h.x0 + (k & 1), yy = h.y0 + (k >> 1);
        if (xx < 0 || xx >= a.W || yy < 0 || yy >= a.H) continue;
        psb_emit<FILL>(ix, d0 + yy * a.W + xx, n, w[k]);
    }
}

// exclusive scan of the work-group's 256 values; wsum: 4 ints of LDS
__device__ __forceinline__ int psb_block_scan(int t, int *wsum, int &total)
{
    const int lane = lane_id(), w = threadIdx.x >> 6;
    int inc = t;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) { if (i < w) before += wsum[i]; total += wsum[i]; }
    __syncthreads();
    return before + inc - t;
}

__global__ __launch_bounds__(256) void k_psb_scan(const int32_t *__restrict__ cnt, int n, int32_t *__restrict__ off, int32_t *__restrict__ bsum)
{
    __shared__ int wsum[4];
    const int base = blockIdx.x * kPsbScan + threadIdx.x * 8;
    int c[8], t = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) { c[j] = base + j < n ? cnt[base + j] : 0; t += c[j]; }
    int total;
    int run = psb_block_scan(t, wsum, total);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (base + j < n) off[base + j] = run;
        run += c[j];
    }
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// the chunk totals, in place, by one work-group
__global__ __launch_bounds__(256) void k_psb_scan_top(int32_t *__restrict__ bsum, int nb)
{
    __shared__ int wsum[4];
    int carry = 0;
    for (int b0 = 0; b0 < nb; b0 += 256) {
        const int b = b0 + threadIdx.x;
        const int t = b < nb ? bsum[b] : 0;
        int total;
        const int ex = psb_block_scan(t, wsum, total);
        if (b < nb) bsum[b] = carry + ex;
        carry += total;
    }
}

// raw -> sorted: every list in ascending point order (the keys of a list are distinct), by counting the smaller keys.  One lane
// per pixel for lists of up to 32 entries (the detector's clouds: at most 7); the wave shares a longer list, lane = entry.
__global__ __launch_bounds__(256) void k_psb_order(PsbIndex ix, int D)
{
    const int d = blockIdx.x * 256 + threadIdx.x, lane = lane_id();
    int start = 0, len = 0;
    if (d < D) { start = psb_start(ix, d); len = psb_start(ix, d + 1) - start; }
    if (len <= 32) {
        for (int i = 0; i < len; ++i) {
            const int2 e = ix.raw[start + i];
            int rank = 0;
            for (int j = 0; j < len; ++j) rank += ix.raw[start + j].x < e.x;
            ix.sorted[start + rank] = e;
        }
    }
    unsigned long long big = __ballot(len > 32);
    while (big) {
        const int l = __ffsll((long long)big) - 1;
        big &= big - 1;
        const int s = __builtin_amdgcn_readlane(start, l), m = __builtin_amdgcn_readlane(len, l);
        for (int i = lane; i < m; i += 64) {
            const int2 e = ix.raw[s + i];
            int rank = 0;
            for (int j = 0; j < m; ++j) rank += ix.raw[s + j].x < e.x;
            ix.sorted[s + rank] = e;
        }
    }
}

// dfeat (V, C, H*W) in storage type DT.  A work-group owns 64 pixels x 64 channels of one view.  Summing: a wave takes 16 of the
// pixels, lanes = channels, so a dout row is read as 256 contiguous bytes; the sums cross over through LDS and are stored with
// lanes = pixels, 64 consecutive elements of a channel row per store.
struct PsbGrad {
    PsbIndex ix; const float *dout; const int32_t *valid_num; void *dfeat;
    int C, HW, ptiles;      // ptiles = ceil(HW / 64)
    size_t ldo;             // floats between two rows of dout (>= C: a column block of a wider matrix)
};

template <int DT>
__global__ __launch_bounds__(256) void k_point_sample_grad(PsbGrad g)
{
    __shared__ float tile[64][65];
    const int v = blockIdx.x / g.ptiles, p0 = (blockIdx.x % g.ptiles) * 64, c0 = blockIdx.y * 64;
    const int lane = lane_id(), w = threadIdx.x >> 6;
    int start = 0, len = 0;
    if (p0 + lane < g.HW) {
        const int d = v * g.HW + p0 + lane;
        start = psb_start(g.ix, d);
        len = psb_start(g.ix, d + 1) - start;
    }
    const int c = c0 + lane;
    for (int i = 0; i < 16; ++i) {
        const int p = w * 16 + i;
        const int s = __builtin_amdgcn_readlane(start, p), m = __builtin_amdgcn_readlane(len, p);
        float acc = 0.0f;
        for (int e0 = 0; e0 < m; e0 += 64) {
            const int cnt = min(64, m - e0);
            int en = 0;
            float ew = 0.0f, ed = 1.0f;
            if (lane < cnt) {
                const int2 e = g.ix.sorted[s + e0 + lane];
                en = e.x; ew = __int_as_float(e.y); ed = (float)g.valid_num[en];
            }
            for (int j = 0; j < cnt; ++j) {
                const int n = __builtin_amdgcn_readlane(en, j);
                const float wj = PTX_LANE_F(ew, j), dj = PTX_LANE_F(ed, j);
                if (c < g.C) acc = __fadd_rn(acc, __fmul_rn(wj, __fdiv_rn(g.dout[(size_t)n * g.ldo + c], dj)));
            }
        }
        tile[lane][p] = acc;
    }
    __syncthreads();
    const int p = p0 + lane;
#pragma unroll 4
    for (int r = 0; r < 16; ++r) {
        const int cc = w * 16 + r;
        if (c0 + cc < g.C && p < g.HW) img_store<DT>(g.dfeat, ((size_t)v * g.C + c0 + cc) * g.HW + p, tile[cc][lane]);
    }
}

struct PsbLayout { size_t cnt, off, bsum, raw, sorted, total; int D, nb; long long E; };
// false: a size outside the 32-bit index range of the kernels
static bool psb_layout(int N, int V, int H, int W, int bilinear, PsbLayout &L)
{
    const long long D = (long long)V * H * W, E = (long long)N * V * (bilinear ? 4 : 1);
    if (D + 1 > INT32_MAX - kPsbScan || E > INT32_MAX - 256) return false;
    L.D = (int)D; L.E = E; L.nb = cdiv(L.D + 1, kPsbScan);
    size_t o = 0;
    L.cnt = o;    o += align_up((size_t)(D + 1) * 4, 256);
    L.off = o;    o += align_up((size_t)(D + 1) * 4, 256);
    L.bsum = o;   o += align_up((size_t)L.nb * 4, 256);
    L.raw = o;    o += align_up((size_t)E * 8, 256);
    L.sorted = o; o += align_up((size_t)E * 8, 256);
    L.total = o;
    return true;
}

size_t psb_bytes(int N, int V, int H, int W, int bilinear)
{
    PsbLayout L;
    if (N < 1 || V < 1 || H < 1 || W < 1 || !psb_layout(N, V, H, W, bilinear, L)) return 0;
    return L.total;
}

int psb_run(const char *who, const PsArgs &a, const float *dout, size_t ldo, void *dfeats, int feat_dtype, void *workspace,
            size_t ws_bytes, hipStream_t st)
{
    const int N = a.N, V = a.V, C = a.C, H = a.H, W = a.W;
    PTX_REQUIRE(N >= 1 && V >= 1 && C >= 1 && C <= 64 * kPsMaxQ && H >= 1 && W >= 1 && feat_dtype >= 0 && feat_dtype <= 2 &&
                a.pad_h > 0.0f && a.pad_w > 0.0f && ldo >= (size_t)C, "%s: N=%d V=%d C=%d (<= %d) H=%d W=%d dtype=%d pad=(%g, %g)", who, N, V,
                C, 64 * kPsMaxQ, H, W, feat_dtype, (double)a.pad_h, (double)a.pad_w);
    PsbLayout L;
    const int ptiles = cdiv(H * W, 64);
    PTX_REQUIRE(psb_layout(N, V, H, W, a.bilinear, L) && (long long)V * ptiles <= INT32_MAX,
                "%s: N=%d V=%d H=%d W=%d: more (point, view) pairs or pixels than 32-bit indices hold", who, N, V, H, W);
    if (ws_bytes < L.total) { set_error("%s: workspace too small: %zu < %zu bytes", who, ws_bytes, L.total); return PTX_ENOSPACE; }
    char *ws = static_cast<char *>(workspace);
    PsbIndex ix{reinterpret_cast<int32_t *>(ws + L.cnt), reinterpret_cast<int32_t *>(ws + L.off), reinterpret_cast<int32_t *>(ws + L.bsum),
                reinterpret_cast<int2 *>(ws + L.raw), reinterpret_cast<int2 *>(ws + L.sorted)};
    const int pair_blocks = (int)(((long long)N * V + 255) / 256);
    PTX_HIP(hipMemsetAsync(ix.cnt, 0, (size_t)(L.D + 1) * 4, st));
    hipLaunchKernelGGL(k_psb_index<false>, dim3(pair_blocks), dim3(256), 0, st, a, ix);
    PTX_LAUNCHED("k_psb_index<count>");
    hipLaunchKernelGGL(k_psb_scan, dim3(L.nb), dim3(256), 0, st, ix.cnt, L.D + 1, ix.off, ix.bsum);
    PTX_LAUNCHED("k_psb_scan");
    hipLaunchKernelGGL(k_psb_scan_top, dim3(1), dim3(256), 0, st, ix.bsum, L.nb);
    PTX_LAUNCHED("k_psb_scan_top");
    hipLaunchKernelGGL(k_psb_index<true>, dim3(pair_blocks), dim3(256), 0, st, a, ix);
    PTX_LAUNCHED("k_psb_index<fill>");
    hipLaunchKernelGGL(k_psb_order, dim3(cdiv(L.D, 256)), dim3(256), 0, st, ix, L.D);
    PTX_LAUNCHED("k_psb_order");
    PsbGrad g{ix, dout, a.valid_num, dfeats, C, H * W, ptiles, ldo};
    const dim3 grid(V * ptiles, cdiv(C, 64));
    if (feat_dtype == 0) hipLaunchKernelGGL(k_point_sample_grad<0>, grid, dim3(256), 0, st, g);
    else if (feat_dtype == 1) hipLaunchKernelGGL(k_point_sample_grad<1>, grid, dim3(256), 0, st, g);
    else hipLaunchKernelGGL(k_point_sample_grad<2>, grid, dim3(256), 0, st, g);
    PTX_LAUNCHED("k_point_sample_grad");
    return PTX_OK;
}

}  // namespace ptx

using namespace ptx;

extern "C" {

/* out (cols, rows) = in (rows, cols)^T, fp32 (train mode: transposed weights for the input-gradient GEMMs) */
int ptx_op_transpose(const float *in, int rows, int cols, float *out, void *stream)
{
    PTX_REQUIRE(in && out && rows >= 1 && cols >= 1, "ptx_op_transpose: bad arguments");
    hipLaunchKernelGGL(k_feat_transpose, dim3(cdiv(cols, 32), cdiv(rows, 32), 1), dim3(256), 0, static_cast<hipStream_t>(stream),
                       in, 0, rows, cols, out);
    PTX_LAUNCHED("k_feat_transpose");
    return PTX_OK;
}

size_t ptx_point_sample_workspace_bytes(int V, int C, int H, int W)
{
    if (V < 1 || C < 1 || C > 64 * kPsMaxQ || H < 1 || W < 1) return 0;
    return align_up((size_t)V * C * H * W * sizeof(float), 256);
}

/* the channels-last copy alone (ABI 12): what ptx_point_sample does first.  A caller that knows the feature maps before it knows the
 * points (the detector: the 2D backbone runs before the neck) makes the copies early, on another stream, and samples with feats = NULL */
int ptx_point_sample_prepare(const void *feats, int feat_dtype, int V, int C, int H, int W, void *workspace, size_t ws_bytes, void *stream)
{
    PTX_REQUIRE(feats && workspace && V >= 1 && C >= 1 && C <= 64 * kPsMaxQ && H >= 1 && W >= 1 && feat_dtype >= 0 && feat_dtype <= 2,
                "ptx_point_sample_prepare: V=%d C=%d (<= %d) H=%d W=%d dtype=%d", V, C, 64 * kPsMaxQ, H, W, feat_dtype);
    const size_t need = ptx_point_sample_workspace_bytes(V, C, H, W);
    if (ws_bytes < need) { set_error("ptx_point_sample_prepare: workspace too small: %zu < %zu bytes", ws_bytes, need); return PTX_ENOSPACE; }
    hipLaunchKernelGGL(k_feat_transpose, dim3(cdiv(H * W, 32), cdiv(C, 32), V), dim3(256), 0, static_cast<hipStream_t>(stream), feats,
                       feat_dtype, C, H * W, static_cast<float *>(workspace));
    PTX_LAUNCHED("k_feat_transpose");
    return PTX_OK;
}

int ptx_point_sample(const float *points, int N, const void *feats, int feat_dtype, int V, int C, int H, int W,
                     const float *proj, const float *pre, float scale_w, float scale_h, float crop_w, float crop_h, int flip,
                     float ori_w, float pad_h, float pad_w, int bilinear, float *out, int32_t *valid_num, void *workspace,
                     size_t ws_bytes, void *stream)
{
    PTX_REQUIRE(points && proj && out && workspace, "ptx_point_sample: null argument");       // feats == NULL: workspace prepared
    PTX_REQUIRE(N >= 1 && V >= 1 && C >= 1 && C <= 64 * kPsMaxQ && H >= 1 && W >= 1 && feat_dtype >= 0 && feat_dtype <= 2 &&
                pad_h > 0.0f && pad_w > 0.0f, "ptx_point_sample: N=%d V=%d C=%d (<= %d) H=%d W=%d dtype=%d", N, V, C,
                64 * kPsMaxQ, H, W, feat_dtype);
    const size_t need = ptx_point_sample_workspace_bytes(V, C, H, W);
    if (ws_bytes < need) { set_error("ptx_point_sample: workspace too small: %zu < %zu bytes", ws_bytes, need); return PTX_ENOSPACE; }
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *featT = static_cast<float *>(workspace);
    if (feats != nullptr) {
        hipLaunchKernelGGL(k_feat_transpose, dim3(cdiv(H * W, 32), cdiv(C, 32), V), dim3(256), 0, st, feats, feat_dtype, C, H * W, featT);
        PTX_LAUNCHED("k_feat_transpose");
    }
    PsArgs a{points, N, featT, V, C, H, W, proj, pre, scale_w, scale_h, crop_w, crop_h, flip, ori_w, pad_h, pad_w, out, valid_num, bilinear ? 1 : 0,
             nullptr, 0.0f};
    hipLaunchKernelGGL(k_point_sample, dim3(cdiv(N, 4)), dim3(256), 0, st, a);
    PTX_LAUNCHED("k_point_sample");
    return PTX_OK;
}

/* Bytes of ptx_point_sample_bwd's workspace: the (view, pixel) lists sized for every (point, view[, neighbour]) pair. */
size_t ptx_point_sample_bwd_workspace_bytes(int N, int V, int H, int W, int bilinear)
{
    return psb_bytes(N, V, H, W, bilinear);
}

int ptx_point_sample_bwd(const float *points, int N, const float *dout, const int32_t *valid_num, int V, int C, int H, int W,
                         const float *proj, const float *pre, float scale_w, float scale_h, float crop_w, float crop_h, int flip,
                         float ori_w, float pad_h, float pad_w, int bilinear, void *dfeats, int feat_dtype, void *workspace,
                         size_t ws_bytes, void *stream)
{
    PTX_REQUIRE(points && dout && valid_num && proj && dfeats && workspace, "ptx_point_sample_bwd: null argument");
    PsArgs a{points, N, nullptr, V, C, H, W, proj, pre, scale_w, scale_h, crop_w, crop_h, flip, ori_w, pad_h, pad_w, nullptr,
             const_cast<int32_t *>(valid_num), bilinear ? 1 : 0, nullptr, 0.0f};
    return psb_run("ptx_point_sample_bwd", a, dout, (size_t)C, dfeats, feat_dtype, workspace, ws_bytes, static_cast<hipStream_t>(stream));
}

}  // extern "C"
