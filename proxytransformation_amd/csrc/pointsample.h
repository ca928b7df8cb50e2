// The point-sampling arithmetic that more than one kernel file runs (pointsample.hip: one scene per call; level_join.hip: every scene
// of a backbone level in one launch): where a point lands in a view, the sum over the views, and the host entry of the backward's
// inverted index.  One statement of the rounded steps: whoever samples calls these and gets the same bits.
#pragma once
#include "common.h"

namespace ptx {

struct PsArgs {
    const float *points; int N;
    const float *featT; int V, C, H, W;
    const float *proj; const float *pre;
    float sx, sy, cx, cy; int flip; float ori_w, pad_h, pad_w;
    float *out; int32_t *valid_num;
    int bilinear;       // aligned=True: F.grid_sample(mode='bilinear'); 0: 'nearest' (what the detector asks for)
    // points == NULL: point n = (float)coords[n, 1:4] * voxel_size, the rows of a sparse level (scene, x, y, z) read in place
    const int32_t *coords; float voxel_size;
};

constexpr int kPsMaxQ = 8;      // C <= 512

// point n of the call: the (N,3) array, or a level's integer row times the voxel size (one rounded multiply, as ptx_voxel_coarsen
// and the neck form it)
__device__ __forceinline__ void ps_point(const PsArgs &a, int n, float &x, float &y, float &z)
{
    if (a.points) {
        x = a.points[(size_t)n * 3]; y = a.points[(size_t)n * 3 + 1]; z = a.points[(size_t)n * 3 + 2];
    } else {
        const int32_t *c = a.coords + (size_t)n * 4;
        x = __fmul_rn((float)c[1], a.voxel_size); y = __fmul_rn((float)c[2], a.voxel_size); z = __fmul_rn((float)c[3], a.voxel_size);
    }
}

// the reverse 3D augmentation, composed by the host into one affine (pre == NULL: none)
__device__ __forceinline__ void ps_pre(const float *A, float &x, float &y, float &z)
{
    if (!A) return;
    const float nx = fmaf(A[2], z, fmaf(A[1], y, A[0] * x)) + A[3];
    const float ny = fmaf(A[6], z, fmaf(A[5], y, A[4] * x)) + A[7];
    const float nz = fmaf(A[10], z, fmaf(A[9], y, A[8] * x)) + A[11];
    x = nx; y = ny; z = nz;
}

// Where point (x, y, z) lands in view v.  nearest: pix = y * W + x of the sampled pixel; bilinear: (x0, y0) = the north-west
// neighbour (possibly outside the map) and the weights of the +1 neighbours.  inb: the view contributes a sample; valid: it counts
// in the divisor.  The forward and the backward's index (k_psb_index) both call this: one statement of the rounded steps.
struct PsHit { bool inb, valid; int pix, x0, y0; float wx1, wy1; };
__device__ __forceinline__ PsHit ps_project(const PsArgs &a, float x, float y, float z, int v)
{
    PsHit h{false, false, 0, 0, 0, 0.0f, 0.0f};
    const float *P = a.proj + (size_t)v * 16;
    // q = [x y z 1] P^T (structures/bbox_3d/utils.py:322-327), one rounding per step, in this order
    float q[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
        q[r] = __fadd_rn(fmaf(z, P[4 * r + 2], fmaf(y, P[4 * r + 1], __fmul_rn(x, P[4 * r]))), P[4 * r + 3]);
    const float zc = fmaxf(q[2], 1e-3f);
    float cx = __fsub_rn(__fmul_rn(__fdiv_rn(q[0], zc), a.sx), a.cx);        // scale -> crop (point_fusion.py:266-267)
    const float cy = __fsub_rn(__fmul_rn(__fdiv_rn(q[1], zc), a.sy), a.cy);
    if (a.flip) cx = __fsub_rn(a.ori_w, cx);                                  // horizontal flip (:276)
    const float nx = __fsub_rn(__fmul_rn(__fdiv_rn(cx, a.pad_w), 2.0f), 1.0f);
    const float ny = __fsub_rn(__fmul_rn(__fdiv_rn(cy, a.pad_h), 2.0f), 1.0f);
    // grid_sample, align_corners=True (unnormalise: ((g + 1) / 2) * (size - 1)), zeros padding
    const float ix = __fmul_rn(__fdiv_rn(__fadd_rn(nx, 1.0f), 2.0f), (float)(a.W - 1));
    const float iy = __fmul_rn(__fdiv_rn(__fadd_rn(ny, 1.0f), 2.0f), (float)(a.H - 1));
    if (!a.bilinear) {                                  // nearest: round half to even
        const float fx = rintf(ix), fy = rintf(iy);
        h.inb = fx >= 0.0f && fx <= (float)(a.W - 1) && fy >= 0.0f && fy <= (float)(a.H - 1);
        if (h.inb) h.pix = (int)fy * a.W + (int)fx;
    } else {                                            // the four neighbours, those outside the map count as 0
        const float x0 = floorf(ix), y0 = floorf(iy);
        h.wx1 = __fsub_rn(ix, x0); h.wy1 = __fsub_rn(iy, y0);
        // a point whose four neighbours are all outside contributes nothing (also covers inf / nan coordinates)
        h.inb = x0 >= -1.0f && x0 <= (float)(a.W - 1) && y0 >= -1.0f && y0 <= (float)(a.H - 1);
        if (h.inb) { h.x0 = (int)x0; h.y0 = (int)y0; }
    }
    h.valid = cx < a.pad_w && cx > 0.0f && cy < a.pad_h && cy > 0.0f && q[2] > 0.0f;     // :300-301
    return h;
}

// One wave, one point: project it into all V views (lanes = views), gather from the channels-last maps a.featT (lanes = channels)
// and sum the views in ascending order (the reference sums dim 0).  acc[q]: channel lane + 64 q; returns the divisor's count.
__device__ __forceinline__ int ps_accumulate(const PsArgs &a, float x, float y, float z, int lane, float (&acc)[kPsMaxQ])
{
#pragma unroll
    for (int q = 0; q < kPsMaxQ; ++q) acc[q] = 0.0f;
    int nvalid = 0;
    const int HW = a.H * a.W;
    for (int v0 = 0; v0 < a.V; v0 += 64) {
        const int v = v0 + lane;
        PsHit h{};
        if (v < a.V) h = ps_project(a, x, y, z, v);
        const bool inb = h.inb, valid = h.valid;
        const int pix = h.pix, cx0 = h.x0, cy0 = h.y0;
        const float wx1 = h.wx1, wy1 = h.wy1;
        nvalid += __popcll(__ballot(valid));
        unsigned long long hit = __ballot(inb);
        while (hit) {                                           // views in ascending order (the reference sums dim 0)
            const int l = __ffsll((long long)hit) - 1;
            hit &= hit - 1;
            if (!a.bilinear) {
                const int px = __builtin_amdgcn_readlane(pix, l);
                const float *f = a.featT + ((size_t)(v0 + l) * HW + px) * a.C;
#pragma unroll
                for (int q = 0; q < kPsMaxQ; ++q) {
                    const int c = lane + 64 * q;
                    if (c < a.C) acc[q] += f[c];
                }
            } else {
                const int x0 = __builtin_amdgcn_readlane(cx0, l), y0 = __builtin_amdgcn_readlane(cy0, l);
                const float fx = PTX_LANE_F(wx1, l), fy = PTX_LANE_F(wy1, l);
                const float gx = __fsub_rn(1.0f, fx), gy = __fsub_rn(1.0f, fy);
                // weights as torch's grid sampler forms them: nw = (x1 - ix)(y1 - iy), ne = (ix - x0)(y1 - iy), ...
                const float w[4] = {__fmul_rn(gx, gy), __fmul_rn(fx, gy), __fmul_rn(gx, fy), __fmul_rn(fx, fy)};
                const float *fv = a.featT + (size_t)(v0 + l) * HW * a.C;
                float s[kPsMaxQ];
#pragma unroll
                for (int q = 0; q < kPsMaxQ; ++q) s[q] = 0.0f;
#pragma unroll
                for (int k = 0; k < 4; ++k) {                   // nw, ne, sw, se
                    const int xx = x0 + (k & 1), yy = y0 + (k >> 1);
                    if (xx < 0 || xx >= a.W || yy < 0 || yy >= a.H) continue;      // wave-uniform
                    const float *f = fv + ((size_t)yy * a.W + xx) * a.C;
#pragma unroll
                    for (int q = 0; q < kPsMaxQ; ++q) {
                        const int c = lane + 64 * q;
                        if (c < a.C) s[q] = __fadd_rn(s[q], __fmul_rn(f[c], w[k]));
                    }
                }
#pragma unroll
                for (int q = 0; q < kPsMaxQ; ++q) acc[q] += s[q];
            }
        }
    }
    return nvalid;
}

// The backward of one scene's sampling with respect to its feature maps (pointsample.hip; what ptx_point_sample_bwd runs): the
// inverted index from a's geometry and a.valid_num, then dfeats (V,C,H,W) in storage type feat_dtype, every element written once.
// dout: row n at dout + n * ldo, a.C columns (a column block of a wider matrix is read in place).  Checks the sizes and the
// workspace (psb_bytes) on the host and enqueues nothing when one fails.
size_t psb_bytes(int N, int V, int H, int W, int bilinear);                    // 0: outside the 32-bit index range
int psb_run(const char *who, const PsArgs &a, const float *dout, size_t ldo, void *dfeats, int feat_dtype, void *workspace,
            size_t ws_bytes, hipStream_t st);

}  // namespace ptx
