// The backward of the decoder's flash attention and of its (double) LayerNorm: the operators of decoder.hip under autograd.  The Linear's
// backward is plumbing over ptx_op_gemm / ptx_op_colsum / ptx_op_eltwise (proxytransformation_amd/decoder.py) and has no kernel here.
//
//   ptx_dec_attention_bwd  two launches, no atomics.  With (m, l) per (scene, head, query) from ptx_dec_attention_stats the probabilities
//       are recomputed from the same (Q scale) K^T product the forward forms: P = expf(S - m) / l; then D = rowsum(dO * O),
//       dP = dO V^T, dS = P (dP - D), dV = P^T dO, dQ = scale dS K, dK = dS^T (Q scale).
//       k_dec_attn_dq    work-group = (64 queries, head, scene): key tiles of 64 in ascending order, a tile that is masked throughout is
//           skipped as in the forward; writes dq and D.
//       k_dec_attn_dkv   work-group = (64 keys, head, scene): query tiles of 64 in ascending order; writes dk and dv.  A key tile that
//           is masked throughout writes zeros and returns.
//       Every element of dq, dk, dv is written exactly once.  A masked key and its value are never read (predicated loads): zeros go to
//       their dk / dv, to every key of a scene whose queries have no key (l == 0) and to the dq of such queries.
//       All four products run on the exact-fp32 matrix instruction.  S and dP (sums over the head dimension) are g64_step on operands
//       with d contiguous, as in the forward.  Their results sit in the C/D layout (column = key on the lane, 16 query rows in the
//       registers), so dS is formed in registers.  The products that sum over keys (dq) or queries (dk, dv) take their A operand from an
//       LDS image with that index contiguous -- [query][key] as the forward's Ps for dq, the transposed [key][query] image (one b128 store
//       per four registers) for dk / dv -- and their B operand row by row from the tile that is already staged ([row][d], d on the lane:
//       conflict-free b32 reads), as the forward's P V does.
//       HD = 64: wave (wr, wc) owns a 32 x 32 block [32 wr .., 32 wc ..] of each result over all 64 summands of a tile; HD = 32: wave
//       (wr, wc) owns rows 32 wr .. over the summands 32 wc .. 32 wc + 31 of every tile, the two halves are added (wc = 0 first) at the end.
//       LDS (dynamic): dq 92 928 B (HD 64) / 56 064 B (HD 32); dkv 111 360 B / 74 496 B: one work-group per CU at HD = 64.
//   ptx_dec_ln_bwd  one launch, 16 lanes per row as k_dec_ln: the mean first, then the centred squares, recomputed; with the second norm
//       the first one's result and its statistics are recomputed too and dx = LN1^T(dy + LN2^T(dy2)).  Writes dx and the per-row terms
//       xhat * g and g whose column sums (ptx_op_colsum, in double) are dweight / dbias.
//
// fp32, fixed summation orders (bitwise reproducible), everything on the caller's stream, no host wait.  Held to the numpy restatements of
// proxytransformation_amd/decoder_grad_host.py.
#include "head.h"

namespace ptx {

struct DecAttnBwdArgs {
    const float *q, *k, *v;                                 // (B,Kq,.) / (B,L,.) with row strides ldq / ldk / ldv; head h at column h HD
    const uint8_t *mask;                                    // (B,L), 1 = ignore the key; null: no key is masked
    const float *out, *stats, *dout;                        // (B,Kq,H HD), (B,H,Kq,2), (B,Kq,H HD)
    float *dq, *dk, *dv;                                    // (B,Kq,H HD), (B,L,H HD), (B,L,H HD)
    float *D;                                               // (B,H,Kq): written by k_dec_attn_dq, read by k_dec_attn_dkv
    int B, Kq, L, H;
    long ldq, ldk, ldv;
    float scale;
};

constexpr int kTileF = 64 * LDT;                            // floats of one [64][LDT] LDS image
typedef float (*Lds64)[64][LDT];

template <int HD> constexpr size_t dec_dq_lds() { return (size_t)(4 * (HD / 32) + 2) * kTileF * 4 + 3 * 64 * 4; }
template <int HD> constexpr size_t dec_dkv_lds() { return (size_t)(4 * (HD / 32) + 4) * kTileF * 4 + 3 * 64 * 4; }

// acc (rows 32 wr .., columns on the lane) += A[h2][32 wr + li][k] * Bt[nb][32 h2 + k][li] over the 32 summands k of half h2: A with the
// summed index contiguous, Bt a staged [row][d] tile read row by row
__device__ __forceinline__ void bwd_half(const float (*A)[64][LDT], const float (*Bt)[64][LDT], int h2, int nb, int wr, int li, int hh, f32x16 &acc)
{
#pragma unroll
    for (int kk = 0; kk < BK / 8; ++kk) {
        const int k0 = kk * 8 + hh * 4;
        const float4 a4 = ld4(&A[h2][wr * 32 + li][k0]);
        const float *bp = &Bt[nb][h2 * 32 + k0][li];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, bp[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, bp[LDT], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, bp[2 * LDT], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, bp[3 * LDT], acc, 0, 0, 0);
    }
}

// P and dS of accumulator r from the logit s and dP = dp: zeros on a masked key and for a query without a key
__device__ __forceinline__ void bwd_p_ds(float s, float dp, bool valid, float m, float l, float D, float &p, float &ds)
{
    p = 0.0f; ds = 0.0f;
    if (valid && l != 0.0f) {
        p = expf(s - m) / l;
        ds = p * (dp - D);
    }
}

// blockIdx = (query tile, head, scene)
template <int HD>
__global__ __launch_bounds__(256) void k_dec_attn_dq(DecAttnBwdArgs a)
{
    constexpr int NB = HD / 32;
    constexpr int TPR = HD / 4, RPP = 256 / TPR, NP = 64 / RPP;      // staging: float4s per row, rows per pass, passes
    extern __shared__ __attribute__((aligned(16))) float dec_bwd_lds[];
    Lds64 Qs = reinterpret_cast<Lds64>(dec_bwd_lds);                 // [d >> 5][query][d & 31], scaled
    Lds64 Gs = reinterpret_cast<Lds64>(dec_bwd_lds + NB * kTileF);   // dO, the same layout
    Lds64 Ks = reinterpret_cast<Lds64>(dec_bwd_lds + 2 * NB * kTileF);   // [d >> 5][key][d & 31]
    Lds64 Vs = reinterpret_cast<Lds64>(dec_bwd_lds + 3 * NB * kTileF);
    Lds64 Ps = reinterpret_cast<Lds64>(dec_bwd_lds + 4 * NB * kTileF);   // dS: [key >> 5][query][key & 31]
    float *s_m = dec_bwd_lds + (4 * NB + 2) * kTileF, *s_l = s_m + 64, *s_D = s_l + 64;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1, li = lane & 31, hh = lane >> 5;
    const int q0 = blockIdx.x * 64, head = blockIdx.y, b = blockIdx.z;
    const size_t C = (size_t)a.H * HD;
    const float *qb = a.q + (size_t)b * a.Kq * a.ldq + head * HD;
    const float *kb = a.k + (size_t)b * a.L * a.ldk + head * HD;
    const float *vb = a.v + (size_t)b * a.L * a.ldv + head * HD;
    const float *ob = a.out + (size_t)b * a.Kq * C + head * HD;
    const float *gb = a.dout + (size_t)b * a.Kq * C + head * HD;
    const uint8_t *mb = a.mask ? a.mask + (size_t)b * a.L : nullptr;
    const int sr = tid / TPR, sd = (tid % TPR) * 4;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int row = sr + RPP * i;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f), g = v;
        if (q0 + row < a.Kq) {
            v = ld4(qb + (size_t)(q0 + row) * a.ldq + sd);
            v.x = v.x * a.scale; v.y = v.y * a.scale; v.z = v.z * a.scale; v.w = v.w * a.scale;
            g = ld4(gb + (size_t)(q0 + row) * C + sd);
        }
        st4(&Qs[sd >> 5][row][sd & 31], v);
        st4(&Gs[sd >> 5][row][sd & 31], g);
    }
    {                                                       // D = sum_c dO O: four threads per query, HD / 4 channels each in ascending order
        const int srow = tid >> 2, qd = tid & 3;
        const bool have = q0 + srow < a.Kq;
        float d = 0.0f;
        if (have) {
#pragma unroll
            for (int j = 0; j < HD / 16; ++j) {
                const float4 o4 = ld4(ob + (size_t)(q0 + srow) * C + qd * (HD / 4) + 4 * j);
                const float4 g4 = ld4(gb + (size_t)(q0 + srow) * C + qd * (HD / 4) + 4 * j);
                d = d + g4.x * o4.x; d = d + g4.y * o4.y; d = d + g4.z * o4.z; d = d + g4.w * o4.w;
            }
        }
        d = d + __shfl_xor(d, 1, 64);
        d = d + __shfl_xor(d, 2, 64);
        if (qd == 0) {
            const size_t at = ((size_t)b * a.H + head) * a.Kq + q0 + srow;
            s_D[srow] = d;
            s_m[srow] = have ? a.stats[at * 2] : 0.0f;
            s_l[srow] = have ? a.stats[at * 2 + 1] : 0.0f;
            if (have) a.D[at] = d;
        }
    }
    float4 kv[NP], vv[NP];
    auto fetch = [&](int t) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int key = t * 64 + sr + RPP * i;
            kv[i] = vv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (key < a.L && (mb == nullptr || mb[key] == 0)) {      // a masked key is never read
                kv[i] = ld4(kb + (size_t)key * a.ldk + sd);
                vv[i] = ld4(vb + (size_t)key * a.ldv + sd);
            }
        }
    };
    f32x16 dq;
#pragma unroll
    for (int i = 0; i < 16; ++i) dq[i] = 0.0f;
    const int ntiles = (a.L + 63) >> 6;
    const int nb = HD == 64 ? wc : 0;
    fetch(0);
    for (int t = 0; t < ntiles; ++t) {
        const int mykey = t * 64 + lane;
        const unsigned long long bits = __ballot(mykey < a.L && (mb == nullptr || mb[mykey] == 0));
        if (bits == 0ull) {                                 // masked throughout (work-group uniform)
            if (t + 1 < ntiles) fetch(t + 1);
            continue;
        }
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            st4(&Ks[sd >> 5][sr + RPP * i][sd & 31], kv[i]);
            st4(&Vs[sd >> 5][sr + RPP * i][sd & 31], vv[i]);
        }
        __syncthreads();
        if (t + 1 < ntiles) fetch(t + 1);
        {
            f32x16 s, dp;
#pragma unroll
            for (int i = 0; i < 16; ++i) { s[i] = 0.0f; dp[i] = 0.0f; }
#pragma unroll
            for (int h2 = 0; h2 < NB; ++h2) g64_step(Qs, Ks, h2, wr * 32 + li, wc * 32 + li, hh, s);
#pragma unroll
            for (int h2 = 0; h2 < NB; ++h2) g64_step(Gs, Vs, h2, wr * 32 + li, wc * 32 + li, hh, dp);
            const bool valid = (bits >> (wc * 32 + li)) & 1ull;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = tile_row(r, wr, hh);
                float p, ds;
                bwd_p_ds(s[r], dp[r], valid, s_m[row], s_l[row], s_D[row], p, ds);
                Ps[wc][row][li] = ds;
            }
        }
        __syncthreads();
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
            if (HD == 32 && h2 != wc) continue;
            bwd_half(Ps, Ks, h2, nb, wr, li, hh, dq);
        }
        __syncthreads();
    }
    if (HD == 32) {
        if (wc == 1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) Ps[0][tile_row(r, wr, hh)][li] = dq[r];
        }
        __syncthreads();
        if (wc == 1) return;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = tile_row(r, wr, hh);
        float v = dq[r];
        if (HD == 32) v = v + Ps[0][row][li];
        if (q0 + row < a.Kq) a.dq[((size_t)b * a.Kq + q0 + row) * C + head * HD + nb * 32 + li] = v * a.scale;
    }
}

// blockIdx = (key tile, head, scene)
template <int HD>
__global__ __launch_bounds__(256) void k_dec_attn_dkv(DecAttnBwdArgs a)
{
    constexpr int NB = HD / 32;
    constexpr int TPR = HD / 4, RPP = 256 / TPR, NP = 64 / RPP;
    extern __shared__ __attribute__((aligned(16))) float dec_bwd_lds[];
    Lds64 Qs = reinterpret_cast<Lds64>(dec_bwd_lds);                 // [d >> 5][query][d & 31], scaled
    Lds64 Gs = reinterpret_cast<Lds64>(dec_bwd_lds + NB * kTileF);
    Lds64 Ks = reinterpret_cast<Lds64>(dec_bwd_lds + 2 * NB * kTileF);
    Lds64 Vs = reinterpret_cast<Lds64>(dec_bwd_lds + 3 * NB * kTileF);
    Lds64 Pt = reinterpret_cast<Lds64>(dec_bwd_lds + 4 * NB * kTileF);          // P^T: [query >> 5][key][query & 31]
    Lds64 St = reinterpret_cast<Lds64>(dec_bwd_lds + (4 * NB + 2) * kTileF);    // dS^T, the same layout
    float *s_m = dec_bwd_lds + (4 * NB + 4) * kTileF, *s_l = s_m + 64, *s_D = s_l + 64;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1, li = lane & 31, hh = lane >> 5;
    const int k0 = blockIdx.x * 64, head = blockIdx.y, b = blockIdx.z;
    const size_t C = (size_t)a.H * HD;
    const float *qb = a.q + (size_t)b * a.Kq * a.ldq + head * HD;
    const float *kb = a.k + (size_t)b * a.L * a.ldk + head * HD;
    const float *vb = a.v + (size_t)b * a.L * a.ldv + head * HD;
    const float *gb = a.dout + (size_t)b * a.Kq * C + head * HD;
    const uint8_t *mb = a.mask ? a.mask + (size_t)b * a.L : nullptr;
    const int sr = tid / TPR, sd = (tid % TPR) * 4;
    const unsigned long long bits = __ballot(k0 + lane < a.L && (mb == nullptr || mb[k0 + lane] == 0));
    if (bits == 0ull) {                                     // masked throughout (work-group uniform): zeros, nothing read
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int key = k0 + sr + RPP * i;
            if (key < a.L) {
                st4(a.dk + ((size_t)b * a.L + key) * C + head * HD + sd, make_float4(0.f, 0.f, 0.f, 0.f));
                st4(a.dv + ((size_t)b * a.L + key) * C + head * HD + sd, make_float4(0.f, 0.f, 0.f, 0.f));
            }
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int row = sr + RPP * i, key = k0 + row;
        float4 kq = make_float4(0.f, 0.f, 0.f, 0.f), vq = kq;
        if ((bits >> row) & 1ull) {                         // a masked key is never read
            kq = ld4(kb + (size_t)key * a.ldk + sd);
            vq = ld4(vb + (size_t)key * a.ldv + sd);
        }
        st4(&Ks[sd >> 5][row][sd & 31], kq);
        st4(&Vs[sd >> 5][row][sd & 31], vq);
    }
    float4 qv[NP], gv[NP];
    auto fetch = [&](int t) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int row = t * 64 + sr + RPP * i;
            qv[i] = gv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < a.Kq) {
                float4 v = ld4(qb + (size_t)row * a.ldq + sd);
                v.x = v.x * a.scale; v.y = v.y * a.scale; v.z = v.z * a.scale; v.w = v.w * a.scale;
                qv[i] = v;
                gv[i] = ld4(gb + (size_t)row * C + sd);
            }
        }
    };
    f32x16 dk, dv;
#pragma unroll
    for (int i = 0; i < 16; ++i) { dk[i] = 0.0f; dv[i] = 0.0f; }
    const int ntiles = (a.Kq + 63) >> 6;
    const int nb = HD == 64 ? wc : 0;
    const bool valid = (bits >> (wc * 32 + li)) & 1ull;     // the key of this lane's column of S
    fetch(0);
    for (int t = 0; t < ntiles; ++t) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            st4(&Qs[sd >> 5][sr + RPP * i][sd & 31], qv[i]);
            st4(&Gs[sd >> 5][sr + RPP * i][sd & 31], gv[i]);
        }
        if (tid < 64) {
            const int row = t * 64 + tid;
            const bool have = row < a.Kq;
            const size_t at = ((size_t)b * a.H + head) * a.Kq + row;
            s_m[tid] = have ? a.stats[at * 2] : 0.0f;
            s_l[tid] = have ? a.stats[at * 2 + 1] : 0.0f;
            s_D[tid] = have ? a.D[at] : 0.0f;
        }
        __syncthreads();
        if (t + 1 < ntiles) fetch(t + 1);
        {
            f32x16 s, dp;
#pragma unroll
            for (int i = 0; i < 16; ++i) { s[i] = 0.0f; dp[i] = 0.0f; }
#pragma unroll
            for (int h2 = 0; h2 < NB; ++h2) g64_step(Qs, Ks, h2, wr * 32 + li, wc * 32 + li, hh, s);
#pragma unroll
            for (int h2 = 0; h2 < NB; ++h2) g64_step(Gs, Vs, h2, wr * 32 + li, wc * 32 + li, hh, dp);
#pragma unroll
            for (int g = 0; g < 4; ++g) {                   // registers 4 g .. 4 g + 3: queries 8 g + 4 hh .. + 3 of the wave's 32
                float p[4], ds[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int row = tile_row(4 * g + j, wr, hh);
                    bwd_p_ds(s[4 * g + j], dp[4 * g + j], valid, s_m[row], s_l[row], s_D[row], p[j], ds[j]);
                }
                st4(&Pt[wr][wc * 32 + li][8 * g + 4 * hh], make_float4(p[0], p[1], p[2], p[3]));
                st4(&St[wr][wc * 32 + li][8 * g + 4 * hh], make_float4(ds[0], ds[1], ds[2], ds[3]));
            }
        }
        __syncthreads();
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
            if (HD == 32 && h2 != wc) continue;
            bwd_half(Pt, Gs, h2, nb, wr, li, hh, dv);
            bwd_half(St, Qs, h2, nb, wr, li, hh, dk);
        }
        __syncthreads();
    }
    if (HD == 32) {
        if (wc == 1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                Pt[0][tile_row(r, wr, hh)][li] = dv[r];
                St[0][tile_row(r, wr, hh)][li] = dk[r];
            }
        }
        __syncthreads();
        if (wc == 1) return;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = tile_row(r, wr, hh), key = k0 + row;
        float xv = dv[r], xk = dk[r];
        if (HD == 32) { xv = xv + Pt[0][row][li]; xk = xk + St[0][row][li]; }
        if (!((bits >> row) & 1ull)) { xv = 0.0f; xk = 0.0f; }       // a masked key: zeros
        if (key < a.L) {
            const size_t at = ((size_t)b * a.L + key) * C + head * HD + nb * 32 + li;
            a.dv[at] = xv;
            a.dk[at] = xk;
        }
    }
}

// ---- LayerNorm ------------------------------------------------------------------------------------------------------------------------
struct DecLnBwdArgs {
    const float *x, *w, *b, *w2, *dy, *dy2;
    float *dx, *xdy, *g1, *xdy2;
    int n, C;
    float eps;
};

// k_dec_ln's statistics of a row held by 16 lanes: x becomes xhat = (x - mean) / sqrtf(var + eps); returns the denominator
__device__ __forceinline__ float dec_ln_hat(float4 (&x)[8], int nm, int C, float eps)
{
    float s = 0.0f;
#pragma unroll
    for (int m = 0; m < 8; ++m)
        if (m < nm) { s = s + x[m].x; s = s + x[m].y; s = s + x[m].z; s = s + x[m].w; }
    const float mean = sum16(s) / (float)C;
    float ss = 0.0f;
#pragma unroll
    for (int m = 0; m < 8; ++m)
        if (m < nm) {
            x[m].x = x[m].x - mean; x[m].y = x[m].y - mean; x[m].z = x[m].z - mean; x[m].w = x[m].w - mean;
            ss = ss + x[m].x * x[m].x; ss = ss + x[m].y * x[m].y; ss = ss + x[m].z * x[m].z; ss = ss + x[m].w * x[m].w;
        }
    const float den = sqrtf(sum16(ss) / (float)C + eps);
#pragma unroll
    for (int m = 0; m < 8; ++m)
        if (m < nm) { x[m].x = x[m].x / den; x[m].y = x[m].y / den; x[m].z = x[m].z / den; x[m].w = x[m].w / den; }
    return den;
}

// g (the gradient of a norm's result) becomes the gradient of its operand: (g w - mean(g w) - xhat mean(g w xhat)) / den
__device__ __forceinline__ void dec_ln_back(float4 (&g)[8], const float4 (&xh)[8], int nm, int C, float den, const float *w, int l)
{
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int m = 0; m < 8; ++m)
        if (m < nm) {
            g[m] = mul4(g[m], ld4(w + 64 * m + 4 * l));
            s1 = s1 + g[m].x; s1 = s1 + g[m].y; s1 = s1 + g[m].z; s1 = s1 + g[m].w;
            s2 = s2 + g[m].x * xh[m].x; s2 = s2 + g[m].y * xh[m].y; s2 = s2 + g[m].z * xh[m].z; s2 = s2 + g[m].w * xh[m].w;
        }
    const float m1 = sum16(s1) / (float)C, m2 = sum16(s2) / (float)C;
#pragma unroll
    for (int m = 0; m < 8; ++m)
        if (m < nm) {
            g[m].x = (g[m].x - m1 - xh[m].x * m2) / den; g[m].y = (g[m].y - m1 - xh[m].y * m2) / den;
            g[m].z = (g[m].z - m1 - xh[m].z * m2) / den; g[m].w = (g[m].w - m1 - xh[m].w * m2) / den;
        }
}

__global__ __launch_bounds__(256) void k_dec_ln_bwd(DecLnBwdArgs a)
{
    const int l = threadIdx.x & 15;
    const long row = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int nm = a.C >> 6;
    const bool have = row < a.n;                            // a row behind the end computes on zeros and stores nothing
    const size_t base = (size_t)(have ? row : 0) * a.C + 4 * l;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 xh[8], g[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        xh[m] = (m < nm && have) ? ld4(a.x + base + 64 * m) : zero;
        g[m] = (m < nm && have && a.dy) ? ld4(a.dy + base + 64 * m) : zero;
    }
    const float den = dec_ln_hat(xh, nm, a.C, a.eps);
    if (a.w2 != nullptr) {                                  // g += LN2^T(dy2) at the recomputed first result
        float4 yh[8], g2[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            yh[m] = zero;
            if (m < nm) {
                const float4 w4 = ld4(a.w + 64 * m + 4 * l), b4 = ld4(a.b + 64 * m + 4 * l);
                yh[m] = make_float4(xh[m].x * w4.x + b4.x, xh[m].y * w4.y + b4.y, xh[m].z * w4.z + b4.z, xh[m].w * w4.w + b4.w);
            }
            g2[m] = (m < nm && have && a.dy2) ? ld4(a.dy2 + base + 64 * m) : zero;
        }
        const float den2 = dec_ln_hat(yh, nm, a.C, a.eps);
#pragma unroll
        for (int m = 0; m < 8; ++m)
            if (m < nm && have) st4(a.xdy2 + base + 64 * m, mul4(yh[m], g2[m]));
        dec_ln_back(g2, yh, nm, a.C, den2, a.w2, l);
#pragma unroll
        for (int m = 0; m < 8; ++m)
            if (m < nm) {
                g[m] = add4(g[m], g2[m]);
                if (have) st4(a.g1 + base + 64 * m, g[m]);
            }
    }
#pragma unroll
    for (int m = 0; m < 8; ++m)
        if (m < nm && have) st4(a.xdy + base + 64 * m, mul4(xh[m], g[m]));
    dec_ln_back(g, xh, nm, a.C, den, a.w, l);
#pragma unroll
    for (int m = 0; m < 8; ++m)
        if (m < nm && have) st4(a.dx + base + 64 * m, g[m]);
}

template <int HD>
static int dec_attention_bwd_launch(const DecAttnBwdArgs &a, hipStream_t st)
{
    // more than 64 KB of dynamic LDS needs the attribute (per device: set at every call, as the fused MLP does)
    PTX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_dec_attn_dq<HD>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)dec_dq_lds<HD>()));
    PTX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_dec_attn_dkv<HD>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)dec_dkv_lds<HD>()));
    hipLaunchKernelGGL((k_dec_attn_dq<HD>), dim3(cdiv(a.Kq, 64), a.H, a.B), dim3(256), dec_dq_lds<HD>(), st, a);
    PTX_LAUNCHED("k_dec_attn_dq");
    hipLaunchKernelGGL((k_dec_attn_dkv<HD>), dim3(cdiv(a.L, 64), a.H, a.B), dim3(256), dec_dkv_lds<HD>(), st, a);
    PTX_LAUNCHED("k_dec_attn_dkv");
    return PTX_OK;
}

}  // namespace ptx

using namespace ptx;

extern "C" {

int ptx_dec_attention_bwd(const float *q, long ldq, const float *k, long ldk, const float *v, long ldv, const uint8_t *mask, int B, int Kq,
                          int L, int H, int hd, const float *out, const float *stats, const float *dout, float *dq, float *dk, float *dv,
                          float *rowdot, void *stream)
{
    const char *who = "ptx_dec_attention_bwd";
    PTX_REQUIRE(B >= 1 && B <= kHeadMaxScenes && Kq >= 1 && Kq <= kHeadMaxK && L >= 1 && L <= (1 << 24),
                "%s: B=%d Kq=%d L=%d (B: 1 to 64; Kq: 1 to 1024; L: 1 to 2^24)", who, B, Kq, L);
    PTX_REQUIRE((hd == 32 || hd == 64) && H >= 1 && H * hd <= 512, "%s: H=%d hd=%d (hd: 32 or 64; H hd up to 512)", who, H, hd);
    const long C = (long)H * hd;
    PTX_REQUIRE(ldq >= C && ldk >= C && ldv >= C && ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0 && ldq <= (1 << 20) && ldk <= (1 << 20) &&
                    ldv <= (1 << 20),
                "%s: ldq=%ld ldk=%ld ldv=%ld (row strides: multiples of 4 from H hd=%ld to 2^20)", who, ldq, ldk, ldv, C);
    PTX_REQUIRE(q && k && v && out && stats && dout && dq && dk && dv && rowdot, "%s: null argument", who);
    PTX_REQUIRE(sp_aligned16({q, k, v, out, dout, dq, dk, dv}), "%s: q, k, v, out, dout, dq, dk and dv must be 16-byte aligned", who);
    DecAttnBwdArgs a{};
    a.q = q; a.k = k; a.v = v; a.mask = mask; a.out = out; a.stats = stats; a.dout = dout; a.dq = dq; a.dk = dk; a.dv = dv; a.D = rowdot;
    a.B = B; a.Kq = Kq; a.L = L; a.H = H; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv;
    a.scale = 1.0f / sqrtf((float)hd);
    if (hd == 64) return dec_attention_bwd_launch<64>(a, static_cast<hipStream_t>(stream));
    return dec_attention_bwd_launch<32>(a, static_cast<hipStream_t>(stream));
}

int ptx_dec_ln_bwd(const float *x, long n, int C, const float *weight, const float *bias, float eps, const float *weight2, const float *dy,
                   const float *dy2, float *dx, float *xdy, float *g1, float *xdy2, void *stream)
{
    const char *who = "ptx_dec_ln_bwd";
    PTX_REQUIRE(n >= 1 && n <= (1l << 30), "%s: n=%ld rows (1 to 2^30)", who, n);
    PTX_REQUIRE(sp_width_ok(C) && eps > 0.0f, "%s: C=%d eps=%g (C: a multiple of 64 up to 512; eps > 0)", who, C, (double)eps);
    PTX_REQUIRE(x && weight && dx && xdy && (dy || dy2), "%s: null argument", who);
    PTX_REQUIRE(weight2 ? (bias && g1 && xdy2) : (dy && !dy2 && !g1 && !xdy2),
                "%s: the second LayerNorm needs weight2, bias, g1 and xdy2 together; without it dy alone", who);
    PTX_REQUIRE(sp_aligned16({x, weight, bias, weight2, dy, dy2, dx, xdy, g1, xdy2}), "%s: the operands must be 16-byte aligned", who);
    const DecLnBwdArgs a{x, weight, bias, weight2, dy, dy2, dx, xdy, g1, xdy2, (int)n, C, eps};
    hipLaunchKernelGGL(k_dec_ln_bwd, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    PTX_LAUNCHED("k_dec_ln_bwd");
    return PTX_OK;
}

}  // extern "C"
