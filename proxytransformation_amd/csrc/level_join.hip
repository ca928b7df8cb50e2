// Level join (detectors/sparse_featfusion_grounder_preshape.py:428-479 for ONE backbone level, every scene at once): the rows of a
// sparse level get their sampled image features appended,
//     out[r] = [ level_feats[r] (Cb) | batch_point_sample(scene of r)(coords[r, 1:4] * voxel_size) (Ci) ],
// in one launch instead of B sampling calls, a concatenation over the scenes and one over the channels.  The sampling is
// pointsample.h's: the point, the projection, the sum over the views and the division are the statements k_point_sample runs, so
// the bits are those of the per-scene calls.  What differs per scene travels in a table (the kLj* word offsets below, then the matrices), and
// the channels-last feature copies of ptx_point_sample_prepare are read where they lie, one pointer per scene in the launch's
// arguments.
#include "common.h"
#include "pointsample.h"

namespace ptx {

constexpr int kLjMaxB = 64;
constexpr int kLjSceneWords = 32;       // the table of one scene, in 32-bit words (include/proxyt.h: ptx_level_join)
// word offsets inside a scene's table
constexpr int kLjPre = 0, kLjHasPre = 12, kLjSx = 13, kLjSy = 14, kLjCx = 15, kLjCy = 16, kLjFlip = 17, kLjOriW = 18, kLjPadH = 19,
              kLjPadW = 20;

struct LjArgs {
    const int32_t *coords; int n;               // (n, 4) rows (scene, x, y, z)
    const float *feats; int Cb;                 // (n, Cb)
    const float *tables;                        // B x kLjSceneWords, then proj (B, V, 16)
    int B, V, Ci, H, W; float voxel_size; int bilinear;
    float *out; int32_t *valid_num;             // (n, Cb + Ci); (n) or NULL
    const float *featT[kLjMaxB];                // scene b's channels-last maps (V, H*W, Ci)
};

// The arguments of scene b's sampling.  Two copies of the same table come in: `tables` is READ here (the scalars), `tables_dev` is
// only pointed into (a.proj, a.pre: what the kernels dereference).  On the device both are the device copy; on the host `tables`
// must be the HOST copy -- handing the device copy there makes the host read device memory.
__host__ __device__ __forceinline__ PsArgs lj_scene(const float *tables, const float *tables_dev, int b, int B, int V, int Ci, int H,
                                                    int W, int bilinear, float voxel_size)
{
    const float *t = tables + (size_t)b * kLjSceneWords;
    const float *td = tables_dev + (size_t)b * kLjSceneWords;
    PsArgs a{};
    a.V = V; a.C = Ci; a.H = H; a.W = W;
    a.proj = tables_dev + (size_t)B * kLjSceneWords + (size_t)b * V * 16;
    a.pre = t[kLjHasPre] != 0.0f ? td + kLjPre : nullptr;
    a.sx = t[kLjSx]; a.sy = t[kLjSy]; a.cx = t[kLjCx]; a.cy = t[kLjCy];
    a.flip = t[kLjFlip] != 0.0f;
    a.ori_w = t[kLjOriW]; a.pad_h = t[kLjPadH]; a.pad_w = t[kLjPadW];
    a.bilinear = bilinear;
    a.voxel_size = voxel_size;
    return a;
}

// one wave per row, four rows per work-group (as k_point_sample); lanes = views for the projection, = channels for both copies
__global__ __launch_bounds__(256) void k_level_join(LjArgs g)
{
    const int r = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (r >= g.n) return;
    const int lane = lane_id();
    const int ld = g.Cb + g.Ci;
    float *o = g.out + (size_t)r * ld;
    // the level's own columns, 16 bytes per lane (Cb and Cb + Ci are multiples of 64 floats; the bases are checked on the host)
    const float4 *f4 = reinterpret_cast<const float4 *>(g.feats + (size_t)r * g.Cb);
    float4 *o4 = reinterpret_cast<float4 *>(o);
    for (int c = lane; c < g.Cb / 4; c += 64) o4[c] = f4[c];
    const int b = __builtin_amdgcn_readfirstlane(g.coords[(size_t)r * 4]);
    float acc[kPsMaxQ] = {};
    int nvalid = 0;
    if (b >= 0 && b < g.B) {                                    // a scene index outside the tables: no view sees the row
        PsArgs a = lj_scene(/* read */ g.tables, /* pointed into */ g.tables, b, g.B, g.V, g.Ci, g.H, g.W, g.bilinear, g.voxel_size);
        a.coords = g.coords; a.featT = g.featT[b];
        float x, y, z;
        ps_point(a, r, x, y, z);
        ps_pre(a.pre, x, y, z);
        nvalid = ps_accumulate(a, x, y, z, lane, acc);
    }
    const float den = (float)(nvalid > 1 ? nvalid : 1);
#pragma unroll
    for (int q = 0; q < kPsMaxQ; ++q) {
        const int c = lane + 64 * q;
        if (c < g.Ci) o[g.Cb + c] = nvalid > 0 ? __fdiv_rn(acc[q], den) : 0.0f;
    }
    if (g.valid_num && lane == 0) g.valid_num[r] = nvalid;
}

// dst (n, C) = the first C columns of src (n, ld); C a multiple of 4, rows 16-byte aligned
__global__ __launch_bounds__(256) void k_lj_take_cols(const float *__restrict__ src, size_t ld, int C4, long long total4, float *__restrict__ dst)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const long long r = i / C4;
    const int c = (int)(i % C4);
    reinterpret_cast<float4 *>(dst)[i] = *reinterpret_cast<const float4 *>(src + (size_t)r * ld + 4 * (size_t)c);
}

static bool lj_width(int C) { return C >= 64 && C <= 64 * kPsMaxQ && C % 64 == 0; }

// the checks both directions share; tables: the HOST copy
static int lj_check(const char *who, int n, int Cb, const float *tables, int B, int V, int Ci, int H, int W, float voxel_size)
{
    PTX_REQUIRE(tables, "%s: null tables", who);
    PTX_REQUIRE(n >= 0 && B >= 1 && B <= kLjMaxB && V >= 1 && H >= 1 && W >= 1 && voxel_size > 0.0f,
                "%s: n=%d B=%d (1..%d) V=%d H=%d W=%d voxel_size=%g", who, n, B, kLjMaxB, V, H, W, (double)voxel_size);
    PTX_REQUIRE(lj_width(Cb) && lj_width(Ci), "%s: Cb=%d Ci=%d (multiples of 64 up to %d)", who, Cb, Ci, 64 * kPsMaxQ);
    for (int b = 0; b < B; ++b) {
        const float *t = tables + (size_t)b * kLjSceneWords;
        PTX_REQUIRE(t[kLjPadH] > 0.0f && t[kLjPadW] > 0.0f, "%s: scene %d: pad=(%g, %g)", who, b, (double)t[kLjPadH], (double)t[kLjPadW]);
    }
    return PTX_OK;
}

}  // namespace ptx

using namespace ptx;

extern "C" {

size_t ptx_level_join_table_floats(int B, int V)
{
    if (B < 1 || B > kLjMaxB || V < 1) return 0;
    return (size_t)B * kLjSceneWords + (size_t)B * V * 16;
}

int ptx_level_join(const int32_t *coords, int n, const float *level_feats, int Cb, const float *const *featT, const float *tables_host,
                   const float *tables_dev, int B, int V, int Ci, int H, int W, float voxel_size, int bilinear, float *out,
                   int32_t *valid_num, void *stream)
{
    if (int rc = lj_check("ptx_level_join", n, Cb, tables_host, B, V, Ci, H, W, voxel_size)) return rc;
    if (n == 0) return PTX_OK;
    PTX_REQUIRE(coords && level_feats && featT && tables_dev && out, "ptx_level_join: null argument");
    PTX_REQUIRE(n <= INT32_MAX - 4, "ptx_level_join: n=%d", n);
    PTX_REQUIRE((reinterpret_cast<uintptr_t>(level_feats) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0,
                "ptx_level_join: level_feats and out must be 16-byte aligned");
    LjArgs g{coords, n, level_feats, Cb, tables_dev, B, V, Ci, H, W, voxel_size, bilinear ? 1 : 0, out, valid_num, {}};
    for (int b = 0; b < B; ++b) {
        PTX_REQUIRE(featT[b], "ptx_level_join: scene %d: null feature workspace", b);
        g.featT[b] = featT[b];
    }
    hipLaunchKernelGGL(k_level_join, dim3(cdiv(n, 4)), dim3(256), 0, static_cast<hipStream_t>(stream), g);
    PTX_LAUNCHED("k_level_join");
    return PTX_OK;
}

size_t ptx_level_join_bwd_workspace_bytes(int max_rows, int V, int H, int W, int bilinear)
{
    return psb_bytes(max_rows, V, H, W, bilinear);
}

int ptx_level_join_bwd(const int32_t *coords, int n, const int32_t *scene_end, const float *g, int Cb, const int32_t *valid_num,
                       const float *tables_host, const float *tables_dev, int B, int V, int Ci, int H, int W, float voxel_size,
                       int bilinear, float *dlevel_feats, void *dimg, int feat_dtype, void *workspace, size_t ws_bytes, void *stream)
{
    if (int rc = lj_check("ptx_level_join_bwd", n, Cb, tables_host, B, V, Ci, H, W, voxel_size)) return rc;
    PTX_REQUIRE(scene_end && tables_dev && (dlevel_feats || dimg), "ptx_level_join_bwd: null argument");
    PTX_REQUIRE(n == 0 || (coords && g), "ptx_level_join_bwd: null argument");
    PTX_REQUIRE((reinterpret_cast<uintptr_t>(g) & 15) == 0 && (reinterpret_cast<uintptr_t>(dlevel_feats) & 15) == 0,
                "ptx_level_join_bwd: g and dlevel_feats must be 16-byte aligned");
    PTX_REQUIRE(!dimg || (feat_dtype >= 0 && feat_dtype <= 2 && (n == 0 || valid_num)), "ptx_level_join_bwd: dtype=%d", feat_dtype);
    int prev = 0, max_rows = 0;
    for (int b = 0; b < B; ++b) {
        PTX_REQUIRE(scene_end[b] >= prev && scene_end[b] <= n, "ptx_level_join_bwd: scene_end[%d]=%d (previous %d, n=%d)", b, scene_end[b], prev, n);
        max_rows = scene_end[b] - prev > max_rows ? scene_end[b] - prev : max_rows;
        prev = scene_end[b];
    }
    PTX_REQUIRE(prev == n, "ptx_level_join_bwd: scene_end[%d]=%d != n=%d", B - 1, prev, n);
    const size_t img_elems = (size_t)V * Ci * H * W, esz = feat_dtype == 0 ? 4 : 2;
    if (dimg && max_rows > 0) {
        const size_t need = psb_bytes(max_rows, V, H, W, bilinear);
        PTX_REQUIRE(need != 0 && (long long)V * cdiv(H * W, 64) <= INT32_MAX,
                    "ptx_level_join_bwd: rows=%d V=%d H=%d W=%d: more (point, view) pairs or pixels than 32-bit indices hold", max_rows, V, H, W);
        if (!workspace || ws_bytes < need) { set_error("ptx_level_join_bwd: workspace too small: %zu < %zu bytes", ws_bytes, need); return PTX_ENOSPACE; }
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t ld = (size_t)Cb + Ci;
    if (dlevel_feats && n > 0) {
        const long long total4 = (long long)n * (Cb / 4);
        hipLaunchKernelGGL(k_lj_take_cols, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, g, ld, Cb / 4, total4, dlevel_feats);
        PTX_LAUNCHED("k_lj_take_cols");
    }
    if (!dimg) return PTX_OK;
    prev = 0;
    for (int b = 0; b < B; ++b) {                               // scene by scene: the index of ptx_point_sample_bwd on the scene's rows
        const int r0 = prev, nb = scene_end[b] - prev;
        prev = scene_end[b];
        char *dst = static_cast<char *>(dimg) + (size_t)b * img_elems * esz;
        if (nb == 0) {                                          // no row of this scene at this level: its maps get zeros
            PTX_HIP(hipMemsetAsync(dst, 0, img_elems * esz, st));
            continue;
        }
        PsArgs a = lj_scene(/* read: host copy */ tables_host, /* pointed into: device copy */ tables_dev, b, B, V, Ci, H, W, bilinear ? 1 : 0, voxel_size);
        a.N = nb;
        a.coords = coords + (size_t)r0 * 4;
        a.valid_num = const_cast<int32_t *>(valid_num) + r0;
        if (int rc = psb_run("ptx_level_join_bwd", a, g + (size_t)r0 * ld + Cb, ld, dst, feat_dtype, workspace, ws_bytes, st)) return rc;
    }
    return PTX_OK;
}

}  // extern "C"
