// The grounding loss (GroundingHead.loss, dense_heads/grounding_head.py:606-824, as the shipped configuration runs it) on gfx950;
// proxytransformation_amd/grounding_loss_host.py restates every launch in numpy and is the specification.
//
//   ptx_gl_iou       IoU of two 9-DoF oriented boxes for every pair of two lists (the exact intersection volume of two convex hexahedra)
//   ptx_gl_cost      the Hungarian matching costs of every (layer, query, ground-truth box) in one launch:
//                    BinaryFocalLossCost + BBox3DL1Cost - IoU3DCost
//   ptx_gl_loss_fwd  focal classification loss and decoupled corner (Chamfer) box loss of every layer: per-query partial sums, then
//                    one work-group per layer adds them in a fixed order
//   ptx_gl_loss_bwd  their gradients by the scores and the predicted boxes
//   ptx_gl_predict   predict_by_feat's max_t sigmoid(score) per query
//
// 16 lanes serve one pair (IoU, cost) or one query (loss): lane f < 12 clips face f of the pair, the lanes stride over the text tokens,
// lane k < 4 takes Chamfer term k.  Sums over lanes go through xor shuffles or a sequential read of the lanes in order: no float
// atomics, and two launches on the same inputs give the same bits.  Every loop over clip vertices runs to kGlPoly.
#include "head.h"

namespace ptx {

constexpr int kGlPoly = 12;                                 // a quad clipped by six planes has at most ten vertices
constexpr double kGlCoplanar = 1e-5;                        // grounding_loss_host.COPLANAR_TOL
constexpr float kGlEps = 1e-12f;                            // FocalLossCost's eps

// THE IoU RUNS IN DOUBLE, IN THE PLANE OF THE FACE IT CLIPS.  Two boxes that nearly coincide (a converged prediction and its target) have
// pairs of faces tilted by theta ~ 1e-2 .. 1e-5 against each other; the line such a pair meets in lies where two distances of the order
// theta x size cancel, so any error e in a vertex, an axis or a distance moves it by e / theta, each of the two faces' lanes moves it on
// its own, and the strip between the two lines is counted twice or not at all: an IoU error of about 0.3 eps / theta -- 4.5e-4 at
// theta = 1e-4 in fp32 (measured; the float64 specification moves by 1e-6 under an ulp there).  So the boxes' axes come from double
// sines and cosines (orthonormal to 1e-16), a face's polygon is kept in the face's own two coordinates (u, v) (exactly planar), a clip
// plane is the affine function D0 + u Du + v Dv of them, and the areas are 2D cross products.
struct GlBox { double c[3], h[3], ax[3][3]; };              // centre, half sizes, ax[m] = column m of R

// Rz Rx Ry from the cosines / sines (c, s) and the "ones" u of the three factors: u = 1 everywhere gives R; the derivative by angle k
// takes (c_k, s_k, u_k) = (-sin, cos, 0)
template <typename F>
__device__ __forceinline__ void gl_rot(const F c[3], const F s[3], const F u[3], F R[3][3])
{
    const F M[3][3] = {{c[0] * u[1], -s[0] * c[1], s[0] * s[1]}, {s[0] * u[1], c[0] * c[1], -c[0] * s[1]}, {F(0), u[0] * s[1], u[0] * c[1]}};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        R[r][0] = M[r][0] * c[2] - M[r][2] * s[2];
        R[r][1] = M[r][1] * u[2];
        R[r][2] = M[r][0] * s[2] + M[r][2] * c[2];
    }
}

__device__ __forceinline__ void gl_angles(const float *a, float c[3], float s[3])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) { c[k] = cosf(a[k]); s[k] = sinf(a[k]); }
}

__device__ __forceinline__ GlBox gl_box(const float *b, float cx, float cy, float cz)
{
    GlBox o;
    double c[3], s[3], R[3][3];
    const double u[3] = {1.0, 1.0, 1.0};
#pragma unroll
    for (int k = 0; k < 3; ++k) { c[k] = cos((double)b[6 + k]); s[k] = sin((double)b[6 + k]); }
    gl_rot(c, s, u, R);
    o.c[0] = (double)b[0] - (double)cx; o.c[1] = (double)b[1] - (double)cy; o.c[2] = (double)b[2] - (double)cz;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        o.h[m] = (double)b[3 + m] * 0.5;
#pragma unroll
        for (int r = 0; r < 3; ++r) o.ax[m][r] = R[r][m];
    }
    return o;
}

// axis m of the box by a runtime index, without indexing the struct's arrays dynamically
__device__ __forceinline__ void gl_axis(const GlBox &X, int m, double a[3], double &h)
{
#pragma unroll
    for (int r = 0; r < 3; ++r) a[r] = m == 0 ? X.ax[0][r] : (m == 1 ? X.ax[1][r] : X.ax[2][r]);
    h = m == 0 ? X.h[0] : (m == 1 ? X.h[1] : X.h[2]);
}

// the signed distance of p to the plane of face f = 2 m + (sigma < 0), positive outside
__device__ __forceinline__ double gl_dist(const GlBox &X, int f, const double p[3])
{
    double a[3], h;
    gl_axis(X, f >> 1, a, h);
    const double sg = (f & 1) ? -1.0 : 1.0;
    return sg * (a[0] * (p[0] - X.c[0]) + a[1] * (p[1] - X.c[1]) + a[2] * (p[2] - X.c[2])) - h;
}

// the in-plane axes of face f: u = m + 1, v = m + 2 (mod 3)
__device__ __forceinline__ void gl_face_axes(int f, int &m, int &iu, int &iv)
{
    m = f >> 1; iu = m == 2 ? 0 : m + 1; iv = iu == 2 ? 0 : iu + 1;
}

// vertex k of face f: c + sigma h_m a_m + su h_u a_u + sv h_v a_v with (su, sv) = (+,+), (-,+), (-,-), (+,-)
__device__ __forceinline__ void gl_quad(const GlBox &X, int f, int k, double p[3])
{
    int m, iu, iv;
    gl_face_axes(f, m, iu, iv);
    double am[3], au[3], av[3], hm, hu, hv;
    gl_axis(X, m, am, hm); gl_axis(X, iu, au, hu); gl_axis(X, iv, av, hv);
    const double sg = (f & 1) ? -1.0 : 1.0, su = (k == 0 || k == 3) ? 1.0 : -1.0, sv = k < 2 ? 1.0 : -1.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) p[r] = X.c[r] + sg * hm * am[r] + su * hu * au[r] + sv * hv * av[r];
}

// THE COPLANARITY RULE (grounding_loss_host.py): face i of the first box and face j of the second are coplanar when all four vertices of
// each lie within tol of the other's plane.  0: not; +1: coplanar, facing the same way; -1: coplanar, facing each other.  Always called
// as (A, i, B, j), whichever face the lane is clipping: the same arithmetic gives the same decision in both directions.
__device__ __forceinline__ int gl_coplanar(const GlBox &A, int i, const GlBox &B, int j, double tol)
{
    double d = 0.0, p[3];
    bool nan = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        gl_quad(A, i, k, p);
        const double da = fabs(gl_dist(B, j, p));
        gl_quad(B, j, k, p);
        const double db = fabs(gl_dist(A, i, p));
        nan = nan || !(da == da) || !(db == db);
        d = fmax(d, fmax(da, db));
    }
    if (nan || !(d <= tol)) return 0;
    double na[3], nb[3], h;
    gl_axis(A, i >> 1, na, h); gl_axis(B, j >> 1, nb, h);
    const double dot = (na[0] * nb[0] + na[1] * nb[1] + na[2] * nb[2]) * (((i ^ j) & 1) ? -1.0 : 1.0);
    return dot > 0.0 ? 1 : -1;
}

// IoU of boxes b1, b2 (9 values each) by the 16 lanes of a group (lane = 0 .. 15): every lane returns the same value.  NaN for a box
// with a NaN, an inf or a non-positive size.
__device__ float gl_pair_iou(const float *b1, const float *b2, int lane)
{
    float v1[9], v2[9];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        v1[i] = b1[i]; v2[i] = b2[i];
        ok = ok && fabsf(v1[i]) < INFINITY && fabsf(v2[i]) < INFINITY;
    }
#pragma unroll
    for (int i = 3; i < 6; ++i) ok = ok && v1[i] > 0.0f && v2[i] > 0.0f;
    if (!ok) return NAN;                                    // the whole group takes this branch
    const double va = (double)v1[3] * v1[4] * v1[5], vb = (double)v2[3] * v2[4] * v2[5];
    const GlBox A = gl_box(v1, v1[0], v1[1], v1[2]), B = gl_box(v2, v1[0], v1[1], v1[2]);
    const double ra = sqrt(A.h[0] * A.h[0] + A.h[1] * A.h[1] + A.h[2] * A.h[2]);
    const double rb = sqrt(B.h[0] * B.h[0] + B.h[1] * B.h[1] + B.h[2] * B.h[2]);
    double vi = 0.0;
    if (B.c[0] * B.c[0] + B.c[1] * B.c[1] + B.c[2] * B.c[2] <= (ra + rb) * (ra + rb)) {      // else: too far apart to meet
        double contrib = 0.0;
        if (lane < 12) {
            const bool first = lane < 6;
            const int fx = first ? lane : lane - 6;
            const GlBox X = first ? A : B, Y = first ? B : A;
            const double tol = kGlCoplanar * (double)fmaxf(fmaxf(fmaxf(v1[3], v1[4]), v1[5]), fmaxf(fmaxf(v2[3], v2[4]), v2[5]));
            // the face: its point o = c + sigma h_m a_m, its axes a_u, a_v, and the quad (+-h_u, +-h_v) in them
            int fm, iu, iv;
            gl_face_axes(fx, fm, iu, iv);
            double am[3], au[3], av[3], hm, hu, hv, o[3];
            gl_axis(X, fm, am, hm); gl_axis(X, iu, au, hu); gl_axis(X, iv, av, hv);
            const double sg = (fx & 1) ? -1.0 : 1.0;
#pragma unroll
            for (int r = 0; r < 3; ++r) o[r] = X.c[r] + sg * hm * am[r] - Y.c[r];
            double poly[kGlPoly][2], next[kGlPoly][2], d[kGlPoly];
            int n = 4;
            poly[0][0] = hu; poly[0][1] = hv; poly[1][0] = -hu; poly[1][1] = hv;
            poly[2][0] = -hu; poly[2][1] = -hv; poly[3][0] = hu; poly[3][1] = -hv;
            for (int j = 0; j < 6 && n >= 3; ++j) {
                const int flag = first ? gl_coplanar(A, fx, B, j, tol) : gl_coplanar(A, j, B, fx, tol);
                if (flag == 1 && first) continue;           // the shared surface: the first box's face stands for it
                if (flag != 0) { n = 0; break; }
                // plane j of Y on this face: d(u, v) = D0 + u Du + v Dv, positive outside
                double an[3], hy;
                gl_axis(Y, j >> 1, an, hy);
                const double sj = (j & 1) ? -1.0 : 1.0;
                const double D0 = sj * (an[0] * o[0] + an[1] * o[1] + an[2] * o[2]) - hy;
                const double Du = sj * (an[0] * au[0] + an[1] * au[1] + an[2] * au[2]);
                const double Dv = sj * (an[0] * av[0] + an[1] * av[1] + an[2] * av[2]);
                for (int k = 0; k < kGlPoly; ++k)
                    if (k < n) d[k] = D0 + (poly[k][0] * Du + poly[k][1] * Dv);
                int m = 0;
                for (int k = 0; k < kGlPoly; ++k) {
                    if (k >= n) continue;
                    const int k2 = k + 1 == n ? 0 : k + 1;
                    const bool in1 = d[k] <= 0.0, in2 = d[k2] <= 0.0;
                    if (in1 && m < kGlPoly) {
                        next[m][0] = poly[k][0]; next[m][1] = poly[k][1];
                        ++m;
                    }
                    if (in1 != in2 && m < kGlPoly) {        // the new vertex from the inside end, whichever way the edge is walked
                        const int ki = in1 ? k : k2, ko = in1 ? k2 : k;
                        const double t = d[ki] / (d[ki] - d[ko]);
                        next[m][0] = poly[ki][0] + t * (poly[ko][0] - poly[ki][0]);
                        next[m][1] = poly[ki][1] + t * (poly[ko][1] - poly[ki][1]);
                        ++m;
                    }
                }
                n = m;
                for (int k = 0; k < kGlPoly; ++k)
                    if (k < n) { poly[k][0] = next[k][0]; poly[k][1] = next[k][1]; }
            }
            if (n >= 3) {
                double twice = 0.0;
                for (int k = 1; k < kGlPoly - 1; ++k) {
                    if (k + 1 >= n) continue;
                    const double a0 = poly[k][0] - poly[0][0], a1 = poly[k][1] - poly[0][1];
                    const double c0 = poly[k + 1][0] - poly[0][0], c1 = poly[k + 1][1] - poly[0][1];
                    twice += a0 * c1 - a1 * c0;
                }
                const double height = hm + sg * (am[0] * X.c[0] + am[1] * X.c[1] + am[2] * X.c[2]);
                contrib = height * (0.5 * fabs(twice)) / 3.0;
            }
        }
        for (int f = 0; f < 12; ++f) vi += __shfl(contrib, f, 16);      // the first box's faces, then the second's
        vi = fmin(fmax(vi, 0.0), fmin(va, vb));
    }
    return (float)(vi / (va + vb - vi));
}

__global__ __launch_bounds__(256) void k_gl_iou(const float *b1, const float *b2, long pairs, int M, float *out)
{
    const long p = ((long)blockIdx.x * 256 + threadIdx.x) >> 4;
    if (p >= pairs) return;                                 // whole groups of 16
    const int lane = threadIdx.x & 15;
    const float v = gl_pair_iou(b1 + (p / M) * 9, b2 + (p % M) * 9, lane);
    if (lane == 0) out[p] = v;
}

// ---- the focal terms ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float gl_pow(float v, float gamma) { return gamma == 2.0f ? v * v : powf(v, gamma); }

struct GlArgs {
    const float *scores, *boxes;                            // (NL,B,K,M), (NL,B,K,9)
    const uint8_t *mask;                                    // (B,T)
    const float *gt, *pm;                                   // (SG,9), (SG,M)
    const int32_t *gt_offset, *gt_scene, *assign;           // (B+1), (SG), (NL,B,K)
    const float *g_cls, *g_box;                             // (NL) upstream gradients or null (ones)
    int NL, B, K, M, T, SG;
    float alpha, gamma, w_cls, w_l1, w_iou, dw[4], cls_scale, box_weight;
    float *cost, *rows, *losses, *dscores, *dboxes;         // (NL,K,SG), (2,NL,B,K), (2,NL), (NL,B,K,M), (NL,B,K,9)
    int32_t *counts;                                        // (NL) matched pairs of a layer
};

__global__ __launch_bounds__(256) void k_gl_cost(GlArgs a)
{
    const long p = ((long)blockIdx.x * 256 + threadIdx.x) >> 4;
    const long per_layer = (long)a.K * a.SG;
    if (p >= per_layer * a.NL) return;
    const int lane = threadIdx.x & 15;
    const int l = (int)(p / per_layer), q = (int)((p % per_layer) / a.SG), gg = (int)(p % a.SG);
    const int b = a.gt_scene[gg];
    if (b < 0 || b >= a.B) {
        if (lane == 0) a.cost[p] = NAN;
        return;
    }
    const long row = ((long)l * a.B + b) * a.K + q;
    const float *x = a.scores + row * a.M, *y = a.pm + (long)gg * a.M;
    const uint8_t *mask = a.mask + (long)b * a.T;
    float cls = 0.0f;
    for (int t = lane; t < a.T; t += 16) {
        if (!mask[t]) continue;                             // a masked token is never read
        const float xv = x[t], yv = y[t];
        const float pr = 1.0f / (1.0f + expf(-xv)), om = 1.0f / (1.0f + expf(xv));
        const float pos = -logf(pr + kGlEps) * a.alpha * gl_pow(om, a.gamma);
        const float neg = -logf(om + kGlEps) * (1.0f - a.alpha) * gl_pow(pr, a.gamma);
        cls += pos * yv + neg * (1.0f - yv);
    }
    cls = sum16(cls);
    const float l1 = sum16(lane < 9 ? fabsf(a.boxes[row * 9 + lane] - a.gt[(long)gg * 9 + lane]) : 0.0f);
    const float iou = gl_pair_iou(a.boxes + row * 9, a.gt + (long)gg * 9, lane);
    if (lane == 0) a.cost[p] = a.w_cls * cls + a.w_l1 * l1 - a.w_iou * iou;
}

__global__ __launch_bounds__(256) void k_gl_predict(const float *scores, long n, int M, float *out)
{
    const long row = ((long)blockIdx.x * 256 + threadIdx.x) >> 4;
    if (row >= n) return;
    const int lane = threadIdx.x & 15;
    float m = -INFINITY;
    bool nan = false;
    for (int t = lane; t < M; t += 16) {
        const float v = scores[row * M + t];
        nan = nan || !(v == v);
        m = fmaxf(m, v);
    }
#pragma unroll
    for (int s = 8; s >= 1; s >>= 1) {
        m = fmaxf(m, __shfl_xor(m, s, 16));
        const int other = __shfl_xor((int)nan, s, 16);      // (not behind "nan ||": a lane that skips the shuffle hands its partner nothing)
        nan = nan || other;
    }
    if (lane == 0) out[row] = nan ? NAN : 1.0f / (1.0f + expf(-m));
}

// ---- the loss -------------------------------------------------------------------------------------------------------------------------
// the matched ground-truth row of query (l, b, q): offset[b] + assign, or -1
__device__ __forceinline__ int gl_matched(const GlArgs &a, long row, int b)
{
    const int g = a.assign[row], lo = a.gt_offset[b], hi = a.gt_offset[b + 1];
    return (g >= 0 && lo >= 0 && hi <= a.SG && g < hi - lo) ? lo + g : -1;
}

// mmdet's sigmoid focal loss of one element and its derivative by x
__device__ __forceinline__ void gl_focal(float x, float y, float alpha, float gamma, float &loss, float &dx)
{
    const float pr = 1.0f / (1.0f + expf(-x)), om = 1.0f / (1.0f + expf(x));
    const float pt = om * y + pr * (1.0f - y), aw = alpha * y + (1.0f - alpha) * (1.0f - y);
    const float bce = fmaxf(x, 0.0f) - x * y + log1pf(expf(-fabsf(x)));
    const float w = aw * gl_pow(pt, gamma);
    loss = bce * w;
    const float dpow = gamma == 2.0f ? 2.0f * pt : gamma * powf(pt, gamma - 1.0f);
    dx = (pr - y) * w + bce * aw * dpow * (1.0f - 2.0f * y) * pr * om;
}

__device__ __forceinline__ void gl_corners(const float *box, float T[8][3])
{
    float c[3], s[3], R[3][3];
    const float u[3] = {1.0f, 1.0f, 1.0f};
    gl_angles(box + 6, c, s);
    gl_rot(c, s, u, R);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float lx = ((k & 4) ? -0.5f : 0.5f) * box[3], ly = ((k & 2) ? -0.5f : 0.5f) * box[4], lz = ((k & 1) ? -0.5f : 0.5f) * box[5];
#pragma unroll
        for (int r = 0; r < 3; ++r) T[k][r] = box[r] + (R[r][0] * lx + R[r][1] * ly + R[r][2] * lz);
    }
}

// One Chamfer term: sum over the 8 corners of the source box of the smallest L1 distance to a target corner (ties: the lower corner);
// grad (9 values, or null): its gradient by the source box, d|u|/du = 0 at 0
__device__ float gl_chamfer(const float *src, const float T[8][3], float *grad)
{
    float c[3], s[3], R[3][3], dR[3][3][3];
    const float u[3] = {1.0f, 1.0f, 1.0f};
    gl_angles(src + 6, c, s);
    gl_rot(c, s, u, R);
    if (grad) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float ck[3] = {c[0], c[1], c[2]}, sk[3] = {s[0], s[1], s[2]}, uk[3] = {1.0f, 1.0f, 1.0f};
            ck[k] = -s[k]; sk[k] = c[k]; uk[k] = 0.0f;
            gl_rot(ck, sk, uk, dR[k]);
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) grad[i] = 0.0f;
    }
    float total = 0.0f;
#pragma unroll 1
    for (int k = 0; k < 8; ++k) {
        const float sgn[3] = {(k & 4) ? -1.0f : 1.0f, (k & 2) ? -1.0f : 1.0f, (k & 1) ? -1.0f : 1.0f};
        const float loc[3] = {sgn[0] * 0.5f * src[3], sgn[1] * 0.5f * src[4], sgn[2] * 0.5f * src[5]};
        float S[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) S[r] = src[r] + (R[r][0] * loc[0] + R[r][1] * loc[1] + R[r][2] * loc[2]);
        float best = fabsf(S[0] - T[0][0]) + fabsf(S[1] - T[0][1]) + fabsf(S[2] - T[0][2]);
        float e[3] = {S[0] - T[0][0], S[1] - T[0][1], S[2] - T[0][2]};
#pragma unroll
        for (int j = 1; j < 8; ++j) {
            const float e0 = S[0] - T[j][0], e1 = S[1] - T[j][1], e2 = S[2] - T[j][2];
            const float dj = fabsf(e0) + fabsf(e1) + fabsf(e2);
            if (dj < best) { best = dj; e[0] = e0; e[1] = e1; e[2] = e2; }
        }
        total += best;
        if (grad) {
            float sg[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) sg[r] = e[r] > 0.0f ? 1.0f : (e[r] < 0.0f ? -1.0f : 0.0f);
#pragma unroll
            for (int r = 0; r < 3; ++r) grad[r] += sg[r];
#pragma unroll
            for (int m = 0; m < 3; ++m) grad[3 + m] += (sg[0] * R[0][m] + sg[1] * R[1][m] + sg[2] * R[2][m]) * sgn[m] * 0.5f;
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                float acc = 0.0f;
#pragma unroll
                for (int r = 0; r < 3; ++r) acc += sg[r] * (dR[m][r][0] * loc[0] + dR[m][r][1] * loc[1] + dR[m][r][2] * loc[2]);
                grad[6 + m] += acc;
            }
        }
    }
    return total;
}

// the source box of decoupled term k: (pred centre | target), (pred size | target), (pred euler | target), the prediction
__device__ __forceinline__ void gl_source(int k, const float *pred, const float *tgt, float src[9])
{
#pragma unroll
    for (int i = 0; i < 9; ++i) src[i] = (k == 3 || i / 3 == k) ? pred[i] : tgt[i];
}

// 16 lanes per query (l, b, q): rows[0][row] = the query's classification sum, rows[1][row] = its weighted Chamfer sum (0: unmatched)
__global__ __launch_bounds__(256) void k_gl_loss_rows(GlArgs a)
{
    const long row = ((long)blockIdx.x * 256 + threadIdx.x) >> 4;
    const long nrows = (long)a.NL * a.B * a.K;
    if (row >= nrows) return;
    const int lane = threadIdx.x & 15, b = (int)((row / a.K) % a.B);
    const int gg = gl_matched(a, row, b);
    const float *x = a.scores + row * a.M;
    const uint8_t *mask = a.mask + (long)b * a.T;
    float cls = 0.0f;
    for (int t = lane; t < a.T; t += 16) {
        if (!mask[t]) continue;
        float loss, dx;
        gl_focal(x[t], gg >= 0 ? a.pm[(long)gg * a.M + t] : 0.0f, a.alpha, a.gamma, loss, dx);
        cls += loss;
    }
    cls = sum16(cls);
    float term = 0.0f;
    if (gg >= 0 && lane < 4) {
        float T[8][3], src[9];
        gl_corners(a.gt + (long)gg * 9, T);
        gl_source(lane, a.boxes + row * 9, a.gt + (long)gg * 9, src);
        term = a.dw[lane] * gl_chamfer(src, T, nullptr);
    }
    float box = 0.0f;
    for (int k = 0; k < 4; ++k) box += __shfl(term, k, 16);
    if (lane == 0) { a.rows[row] = cls; a.rows[nrows + row] = box; }
}

// one work-group per layer: thread t adds the queries t, t + 256, .. in order, then a fixed tree
__global__ __launch_bounds__(256) void k_gl_loss_sum(GlArgs a)
{
    __shared__ float s_c[256], s_b[256];
    __shared__ int s_n[256];
    const int l = blockIdx.x, tid = threadIdx.x, per = a.B * a.K;
    const long nrows = (long)a.NL * per;
    float c = 0.0f, bx = 0.0f;
    int n = 0;
    for (int i = tid; i < per; i += 256) {
        const long row = (long)l * per + i;
        c += a.rows[row]; bx += a.rows[nrows + row];
        n += gl_matched(a, row, i / a.K) >= 0;
    }
    s_c[tid] = c; s_b[tid] = bx; s_n[tid] = n;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) { s_c[tid] += s_c[tid + s]; s_b[tid] += s_b[tid + s]; s_n[tid] += s_n[tid + s]; }
        __syncthreads();
    }
    if (tid == 0) {
        a.losses[l] = s_c[0] * a.cls_scale;
        a.losses[a.NL + l] = s_b[0] * (a.box_weight / ((float)s_n[0] * 8.0f));
        a.counts[l] = s_n[0];
    }
}

__global__ __launch_bounds__(256) void k_gl_loss_bwd(GlArgs a)
{
    __shared__ float s_g[16][4][9];
    const long row = ((long)blockIdx.x * 256 + threadIdx.x) >> 4;
    const long nrows = (long)a.NL * a.B * a.K;
    const bool live = row < nrows;
    const int lane = threadIdx.x & 15, grp = threadIdx.x >> 4;
    int gg = -1, l = 0, b = 0;
    if (live) {
        l = (int)(row / ((long)a.B * a.K)); b = (int)((row / a.K) % a.B);
        gg = gl_matched(a, row, b);
        const float up = (a.g_cls ? a.g_cls[l] : 1.0f) * a.cls_scale;
        const float *x = a.scores + row * a.M;
        const uint8_t *mask = a.mask + (long)b * a.T;
        for (int t = lane; t < a.M; t += 16) {
            float dx = 0.0f;                                // exactly 0 on a masked token and from T on
            if (t < a.T && mask[t]) {
                float loss;
                gl_focal(x[t], gg >= 0 ? a.pm[(long)gg * a.M + t] : 0.0f, a.alpha, a.gamma, loss, dx);
                dx = dx * up;
            }
            a.dscores[row * a.M + t] = dx;
        }
    }
    if (gg >= 0 && lane < 4) {
        float T[8][3], src[9], grad[9];
        gl_corners(a.gt + (long)gg * 9, T);
        gl_source(lane, a.boxes + row * 9, a.gt + (long)gg * 9, src);
        gl_chamfer(src, T, grad);
#pragma unroll
        for (int i = 0; i < 9; ++i) s_g[grp][lane][i] = a.dw[lane] * grad[i];
    }
    __syncthreads();
    if (live && lane < 9) {
        float g = 0.0f;                                     // exactly 0 for an unmatched query
        if (gg >= 0) {
            const float up = (a.g_box ? a.g_box[l] : 1.0f) * (a.box_weight / ((float)a.counts[l] * 8.0f));
            g = (s_g[grp][lane / 3][lane] + s_g[grp][3][lane]) * up;
        }
        a.dboxes[row * 9 + lane] = g;
    }
}

static int gl_shape_ok(const char *who, int NL, int B, int K, int M, int T, int SG)
{
    PTX_REQUIRE(NL >= 1 && NL <= 64 && B >= 1 && B <= kHeadMaxScenes && K >= 1 && K <= kHeadMaxK,
                "%s: NL=%d B=%d K=%d (NL, B: 1 to 64; K: 1 to 1024)", who, NL, B, K);
    PTX_REQUIRE(T >= 1 && T <= M && M <= kHeadMaxText && SG >= 1 && SG <= (1 << 16),
                "%s: T=%d M=%d SG=%d (1 <= T <= M <= %d; 1 to 65536 ground-truth boxes)", who, T, M, SG, kHeadMaxText);
    return PTX_OK;
}

static int gl_focal_ok(const char *who, float alpha, float gamma)
{
    PTX_REQUIRE(alpha >= 0.0f && alpha <= 1.0f && gamma >= 1.0f && gamma <= 8.0f, "%s: alpha=%g gamma=%g (alpha: 0 to 1; gamma: 1 to 8)", who,
                (double)alpha, (double)gamma);
    return PTX_OK;
}

}  // namespace ptx

using namespace ptx;

extern "C" {

int ptx_gl_iou(const float *boxes1, int N, const float *boxes2, int M, float *out, void *stream)
{
    const char *who = "ptx_gl_iou";
    PTX_REQUIRE(N >= 1 && M >= 1 && N <= (1 << 20) && M <= (1 << 20) && (long)N * M <= (1l << 26),
                "%s: N=%d M=%d (1 to 2^20 boxes each, at most 2^26 pairs)", who, N, M);
    PTX_REQUIRE(boxes1 && boxes2 && out, "%s: null argument", who);
    const long pairs = (long)N * M;
    hipLaunchKernelGGL(k_gl_iou, dim3((unsigned)((pairs + 15) / 16)), dim3(256), 0, static_cast<hipStream_t>(stream), boxes1, boxes2, pairs, M, out);
    PTX_LAUNCHED("k_gl_iou");
    return PTX_OK;
}

int ptx_gl_cost(const float *scores, const float *boxes, int NL, int B, int K, int M, const uint8_t *text_mask, int T, const float *gt_boxes,
                const float *positive_maps, const int32_t *gt_scene, int SG, float alpha, float gamma, float w_cls, float w_l1, float w_iou,
                float *cost, void *stream)
{
    const char *who = "ptx_gl_cost";
    PTX_TRY(gl_shape_ok(who, NL, B, K, M, T, SG));
    PTX_TRY(gl_focal_ok(who, alpha, gamma));
    PTX_REQUIRE(scores && boxes && text_mask && gt_boxes && positive_maps && gt_scene && cost, "%s: null argument", who);
    GlArgs a{};
    a.scores = scores; a.boxes = boxes; a.mask = text_mask; a.gt = gt_boxes; a.pm = positive_maps; a.gt_scene = gt_scene;
    a.NL = NL; a.B = B; a.K = K; a.M = M; a.T = T; a.SG = SG; a.alpha = alpha; a.gamma = gamma; a.w_cls = w_cls; a.w_l1 = w_l1; a.w_iou = w_iou;
    a.cost = cost;
    const long pairs = (long)NL * K * SG;
    hipLaunchKernelGGL(k_gl_cost, dim3((unsigned)((pairs + 15) / 16)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    PTX_LAUNCHED("k_gl_cost");
    return PTX_OK;
}

static int gl_loss_args(const char *who, GlArgs &a, const float *scores, const float *boxes, int NL, int B, int K, int M, const uint8_t *text_mask,
                        int T, const float *gt_boxes, const float *positive_maps, const int32_t *gt_offset, int SG, const int32_t *assign,
                        float alpha, float gamma, const float *decouple_weights, float cls_scale, float box_weight)
{
    PTX_TRY(gl_shape_ok(who, NL, B, K, M, T, SG));
    PTX_TRY(gl_focal_ok(who, alpha, gamma));
    PTX_REQUIRE(scores && boxes && text_mask && gt_boxes && positive_maps && gt_offset && assign && decouple_weights, "%s: null argument", who);
    a.scores = scores; a.boxes = boxes; a.mask = text_mask; a.gt = gt_boxes; a.pm = positive_maps; a.gt_offset = gt_offset; a.assign = assign;
    a.NL = NL; a.B = B; a.K = K; a.M = M; a.T = T; a.SG = SG; a.alpha = alpha; a.gamma = gamma; a.cls_scale = cls_scale; a.box_weight = box_weight;
    for (int i = 0; i < 4; ++i) a.dw[i] = decouple_weights[i];
    return PTX_OK;
}

int ptx_gl_loss_fwd(const float *scores, const float *boxes, int NL, int B, int K, int M, const uint8_t *text_mask, int T, const float *gt_boxes,
                    const float *positive_maps, const int32_t *gt_offset, int SG, const int32_t *assign, float alpha, float gamma,
                    const float *decouple_weights, float cls_scale, float box_weight, float *rows, float *losses, int32_t *counts, void *stream)
{
    const char *who = "ptx_gl_loss_fwd";
    GlArgs a{};
    PTX_TRY(gl_loss_args(who, a, scores, boxes, NL, B, K, M, text_mask, T, gt_boxes, positive_maps, gt_offset, SG, assign, alpha, gamma,
                         decouple_weights, cls_scale, box_weight));
    PTX_REQUIRE(rows && losses && counts, "%s: null argument", who);
    a.rows = rows; a.losses = losses; a.counts = counts;
    const long nrows = (long)NL * B * K;
    hipLaunchKernelGGL(k_gl_loss_rows, dim3((unsigned)((nrows + 15) / 16)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    PTX_LAUNCHED("k_gl_loss_rows");
    hipLaunchKernelGGL(k_gl_loss_sum, dim3(NL), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    PTX_LAUNCHED("k_gl_loss_sum");
    return PTX_OK;
}

int ptx_gl_loss_bwd(const float *scores, const float *boxes, int NL, int B, int K, int M, const uint8_t *text_mask, int T, const float *gt_boxes,
                    const float *positive_maps, const int32_t *gt_offset, int SG, const int32_t *assign, float alpha, float gamma,
                    const float *decouple_weights, float cls_scale, float box_weight, const float *g_cls, const float *g_box,
                    const int32_t *counts, float *dscores, float *dboxes, void *stream)
{
    const char *who = "ptx_gl_loss_bwd";
    GlArgs a{};
    PTX_TRY(gl_loss_args(who, a, scores, boxes, NL, B, K, M, text_mask, T, gt_boxes, positive_maps, gt_offset, SG, assign, alpha, gamma,
                         decouple_weights, cls_scale, box_weight));
    PTX_REQUIRE(counts && dscores && dboxes, "%s: null argument", who);
    a.g_cls = g_cls; a.g_box = g_box; a.counts = const_cast<int32_t *>(counts); a.dscores = dscores; a.dboxes = dboxes;
    const long nrows = (long)NL * B * K;
    hipLaunchKernelGGL(k_gl_loss_bwd, dim3((unsigned)((nrows + 15) / 16)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    PTX_LAUNCHED("k_gl_loss_bwd");
    return PTX_OK;
}

int ptx_gl_predict(const float *scores, long n, int M, float *out, void *stream)
{
    const char *who = "ptx_gl_predict";
    PTX_REQUIRE(n >= 1 && n <= (1l << 26) && M >= 1 && M <= kHeadMaxText, "%s: n=%ld M=%d (n: 1 to 2^26 queries; M: 1 to %d)", who, n, M, kHeadMaxText);
    PTX_REQUIRE(scores && out, "%s: null argument", who);
    hipLaunchKernelGGL(k_gl_predict, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, static_cast<hipStream_t>(stream), scores, n, M, out);
    PTX_LAUNCHED("k_gl_predict");
    return PTX_OK;
}

}  // extern "C"
