// The transformer decoder behind the query selection: the eval forward of SparseFeatureFusionTransformerDecoder
// (models/layers/ground_transformer/decoder.py) and the per-layer text scores of GroundingHead.forward (dense_heads/grounding_head.py:427-467).
//
//   ptx_dec_posembed   PositionEmbeddingLearned in eval: Conv1d(cin -> C, k=1) with the BatchNorm folded in by the caller, ReLU (a NaN
//       kept), Conv1d(C -> C, k=1), one launch: the 64 x 64 tile of the second layer forms its operand -- 64 rows x 64 hidden channels of
//       the first layer, cin <= 9 products each -- while it stages it, so the hidden tensor never exists.
//   ptx_dec_linear     out (n,Cout) = act((x + add) @ W^T + bias) (+ residual): the add is fused into the operand load and applies to the
//       output columns below add_cols only, so one launch gives [q|k|v] of a self attention (positions on q and k, none on v) or the keys
//       and values of every layer's scene attention.
//   ptx_dec_attention  one flash-style kernel: work-group = (64 queries, head, scene), key tiles of 64 in ascending order, the running
//       maximum and sum per query, heads merged in the output.  Both products run on the exact-fp32 matrix instruction.  A masked key is
//       never read (predicated loads), a key tile that is masked throughout is skipped, a query without a key gets zeros.
//       ptx_dec_attention_stats: the same kernel, which then also stores the final (m, l) of every query for the backward
//       (decoder_bwd.hip); the store is null-checked, the arithmetic and the bits of `out` are the same.
//   ptx_dec_ln         LayerNorm over rows of width C: the mean first, then the centred sum of squares; optionally a second LayerNorm of
//       the first one's result (the decoder's `norm` behind `norms[3]`), both written.
//   ptx_dec_boxes      the last Linear (C -> 9) of a regression branch and the baseline box decode against the query coordinates:
//       k_head_boxes<false> (head.h).
//   ptx_dec_scores     ContrastiveEmbed in full: (NL,B,K,max_text_len) with -inf on masked tokens and behind T.
//
// posembed, linear and scores are instantiations of head.h's tile64_nt, accumulating straight through (the query selection's launches
// add per 64-wide block: both orders are recorded behaviour); the Linear epilogue, ContrastiveEmbed's value rule and the 16-lane row sums
// are head.h's too.
//
// fp32, no float atomics, fixed summation orders (bitwise reproducible), everything on the caller's stream, no host wait.  Held to the
// numpy restatements of proxytransformation_amd/decoder_host.py.
#include "head.h"

namespace ptx {

constexpr int kDecMaxCin = 2048, kDecMaxCout = 4096, kDecMaxPos = 9;

// ---- the 64 x 64 NT tile: linear, posembed, scores ------------------------------------------------------------------------------------
enum { DEC_LINEAR = 0, DEC_POSEMBED = 1, DEC_SCORES = 2 };

struct DecGemmArgs {
    const float *x;                                         // (n,Cin); posembed: (n,cin0); scores: (NL B K,Cin)
    const float *add;                                       // linear: (n,Cin) added to x for the column tiles below add_cols, or null
    const float *w;                                         // (Cout,Cin) with k contiguous; scores: the text rows (B,T,Cin)
    const float *bias, *residual; float *out;
    const float *w1, *b1;                                   // posembed: the folded first layer (Cin,cin0), (Cin)
    const uint8_t *mask;                                    // scores: (B,T), 1 = a token
    int n, Cin, Cout, add_cols, relu, cin0;
    int B, K, T, ldo, scaled;
    float divisor;
};

// LINEAR / POSEMBED: blockIdx = (row tile, column tile) of out (n,Cout).
// SCORES: blockIdx = (row tile of the K queries, column tile of ldo = max_text_len, layer * B + scene).
template <int MODE>
__global__ __launch_bounds__(256) void k_dec_gemm(DecGemmArgs a)
{
    __shared__ float s_x[MODE == DEC_POSEMBED ? 64 : 1][kDecMaxPos + 1];
    const Tile64 t;
    const int tid = t.tid;
    const int row0 = blockIdx.x * 64, col0 = blockIdx.y * 64;
    const int z = MODE == DEC_SCORES ? blockIdx.z : 0;
    const int nrows = MODE == DEC_SCORES ? a.K : a.n;
    const size_t rbase = (size_t)z * (MODE == DEC_SCORES ? a.K : 0);
    const int ncols = MODE == DEC_SCORES ? a.T : a.Cout;
    if (MODE == DEC_SCORES && col0 >= a.T) {                // a tile behind the tokens (work-group uniform)
        for (int e = tid; e < 64 * 64; e += 256) {
            const int row = row0 + (e >> 6), col = col0 + (e & 63);
            if (row < nrows && col < a.ldo) a.out[(rbase + row) * a.ldo + col] = -INFINITY;
        }
        return;
    }
    const float *wbase = a.w + (MODE == DEC_SCORES ? (size_t)(z % a.B) * a.T * a.Cin : 0);
    const bool use_add = MODE == DEC_LINEAR && a.add != nullptr && col0 < a.add_cols;
    if (MODE == DEC_POSEMBED) {
        for (int e = tid; e < 64 * a.cin0; e += 256) {
            const int r = e / a.cin0, j = e - r * a.cin0;
            s_x[r][j] = row0 + r < a.n ? a.x[(size_t)(row0 + r) * a.cin0 + j] : 0.0f;
        }
        __syncthreads();
    }
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;

    tile64_nt<false>(
        t, a.Cin >> 6, acc,
        [](int s) { return s << 6; },                       // the first channel of step s
        [&](float4 &v, int c0, int row, int kq) {
            const int grow = row0 + row;
            if (MODE == DEC_POSEMBED) {                     // the first layer's 4 hidden channels of this row, cin0 products each
                float h[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int k = c0 + kq + q;
                    float v = 0.0f;
                    for (int j = 0; j < a.cin0; ++j) v = v + s_x[row][j] * a.w1[k * a.cin0 + j];
                    h[q] = relu_nan(v + a.b1[k]);
                }
                v = make_float4(h[0], h[1], h[2], h[3]);
            } else {
                v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (grow < nrows) {
                    v = ld4(a.x + (rbase + grow) * a.Cin + c0 + kq);
                    if (use_add) v = add4(v, ld4(a.add + (size_t)grow * a.Cin + c0 + kq));
                }
            }
        },
        [&](float4 &v, int c0, int row, int kq) {
            v = col0 + row < ncols ? ld4(wbase + (size_t)(col0 + row) * a.Cin + c0 + kq) : make_float4(0.f, 0.f, 0.f, 0.f);
        },
        [](int) {});
    const int n = col0 + t.col();
    if (MODE == DEC_SCORES) {
        if (n >= a.ldo) return;
        const bool valid = n < a.T && a.mask[(size_t)(z % a.B) * a.T + n] != 0;
        const float bias = a.bias ? a.bias[0] : 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = row0 + t.row(r);
            if (row < nrows) a.out[(rbase + row) * a.ldo + n] = contrastive_value(acc[r], valid, a.scaled, a.divisor, a.bias != nullptr, bias);
        }
        return;
    }
    linear_store(t, acc, row0, nrows, n, a.Cout, a.bias, a.relu, a.residual, a.out);
}

// ---- attention ------------------------------------------------------------------------------------------------------------------------
struct DecAttnArgs {
    const float *q, *k, *v;                                 // (B,Kq,.) / (B,L,.) with row strides ldq / ldk / ldv; head h at column h HD
    const uint8_t *mask;                                    // (B,L), 1 = ignore the key; null: no key is masked
    float *out;                                             // (B,Kq,H HD)
    float *stats;                                           // (B,H,Kq,2) or null: the final maximum and sum (m, l); l == 0: no key
    int B, Kq, L, H;
    long ldq, ldk, ldv;
    float scale;
};

// blockIdx = (query tile, head, scene).  Per key tile of 64: S = (Q scale) K^T on the matrix cores into LDS; four threads per query take
// the 64 logits (16 each): new running maximum, p = expf(s - m) written over S, l = l alpha + sum p (the 16 in ascending order, the four
// quarters as (q0 + q1) + (q2 + q3)); O = O alpha + P V on the matrix cores.  HD = 64: wave (wr, wc) owns O[32 wr .., 32 wc ..] over all 64
// keys; HD = 32: wave (wr, wc) owns O[32 wr .., 0 .. 31] over the keys 32 wc .. 32 wc + 31 of every tile, and the two halves are added
// (wc = 0 first) at the end.  The next tile's K and V are in flight in registers behind the current tile's arithmetic.
template <int HD>
__global__ __launch_bounds__(256) void k_dec_attn(DecAttnArgs a)
{
    constexpr int NB = HD / 32;                             // 32-wide halves of the head dimension
    constexpr int TPR = HD / 4, RPP = 256 / TPR, NP = 64 / RPP;      // staging: float4s per row, rows per pass, passes
    __shared__ __attribute__((aligned(16))) float Qs[NB][64][LDT];   // [d >> 5][query][d & 31]
    __shared__ __attribute__((aligned(16))) float Ks[NB][64][LDT];   // [d >> 5][key][d & 31]
    __shared__ __attribute__((aligned(16))) float Ps[2][64][LDT];    // [key >> 5][query][key & 31]
    __shared__ __attribute__((aligned(16))) float Vs[64][HD + 4];    // [key][d]
    __shared__ float s_alpha[64], s_l[64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1, li = lane & 31, hh = lane >> 5;
    const int q0 = blockIdx.x * 64, head = blockIdx.y, b = blockIdx.z;
    const float *qb = a.q + (size_t)b * a.Kq * a.ldq + head * HD;
    const float *kb = a.k + (size_t)b * a.L * a.ldk + head * HD;
    const float *vb = a.v + (size_t)b * a.L * a.ldv + head * HD;
    const uint8_t *mb = a.mask ? a.mask + (size_t)b * a.L : nullptr;
    const int sr = tid / TPR, sd = (tid % TPR) * 4;         // staging: thread (sr + RPP i, sd .. sd + 3)
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int row = sr + RPP * i;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q0 + row < a.Kq) {
            v = ld4(qb + (size_t)(q0 + row) * a.ldq + sd);
            v.x = v.x * a.scale; v.y = v.y * a.scale; v.z = v.z * a.scale; v.w = v.w * a.scale;
        }
        st4(&Qs[sd >> 5][row][sd & 31], v);
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
    f32x16 o;
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = 0.0f;
    const int srow = tid >> 2, qd = tid & 3;                // soft-max: thread (query srow, keys 16 qd .. 16 qd + 15 of the tile)
    float m_run = -INFINITY, l_run = 0.0f;
    const int ntiles = (a.L + 63) >> 6;
    fetch(0);
    for (int t = 0; t < ntiles; ++t) {
        const int mykey = t * 64 + lane;
        const unsigned long long bits = __ballot(mykey < a.L && (mb == nullptr || mb[mykey] == 0));
        if (bits == 0ull) {                                 // masked throughout (wave- and work-group-uniform): nothing to add
            if (t + 1 < ntiles) fetch(t + 1);
            continue;
        }
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            st4(&Ks[sd >> 5][sr + RPP * i][sd & 31], kv[i]);
            st4(&Vs[sr + RPP * i][sd], vv[i]);
        }
        __syncthreads();
        if (t + 1 < ntiles) fetch(t + 1);
        {
            f32x16 s;
#pragma unroll
            for (int i = 0; i < 16; ++i) s[i] = 0.0f;
#pragma unroll
            for (int h2 = 0; h2 < NB; ++h2) g64_step(Qs, Ks, h2, wr * 32 + li, wc * 32 + li, hh, s);
#pragma unroll
            for (int r = 0; r < 16; ++r) Ps[wc][tile_row(r, wr, hh)][li] = s[r];
        }
        __syncthreads();
        {
            float *prow = &Ps[qd >> 1][srow][(qd & 1) * 16];
            float s[16];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4 v = ld4(prow + 4 * j);
                s[4 * j] = v.x; s[4 * j + 1] = v.y; s[4 * j + 2] = v.z; s[4 * j + 3] = v.w;
            }
            const unsigned mine = (unsigned)(bits >> (qd * 16)) & 0xFFFFu;
            float mx = -INFINITY;
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if ((mine >> j) & 1u) mx = fmaxf(mx, s[j]);
            mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
            const float m_new = fmaxf(m_run, mx);
            const float alpha = m_run == -INFINITY ? 1.0f : expf(m_run - m_new);
            float sum = 0.0f;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                s[j] = ((mine >> j) & 1u) ? expf(s[j] - m_new) : 0.0f;
                sum = sum + s[j];
            }
            sum = sum + __shfl_xor(sum, 1, 64);
            sum = sum + __shfl_xor(sum, 2, 64);
            l_run = l_run * alpha + sum;
            m_run = m_new;
#pragma unroll
            for (int j = 0; j < 4; ++j) st4(prow + 4 * j, make_float4(s[4 * j], s[4 * j + 1], s[4 * j + 2], s[4 * j + 3]));
            if (qd == 0) s_alpha[srow] = alpha;
        }
        __syncthreads();
        {
            f32x16 pv;
#pragma unroll
            for (int i = 0; i < 16; ++i) pv[i] = 0.0f;
            const int col = (HD == 64 ? wc * 32 : 0) + li;
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) {
                if (HD == 32 && h2 != wc) continue;
#pragma unroll
                for (int kk = 0; kk < BK / 8; ++kk) {
                    const int k0 = kk * 8 + hh * 4;
                    const float4 p4 = ld4(&Ps[h2][wr * 32 + li][k0]);
                    const float *vp = &Vs[h2 * 32 + k0][col];
                    pv = __builtin_amdgcn_mfma_f32_32x32x2f32(p4.x, vp[0], pv, 0, 0, 0);
                    pv = __builtin_amdgcn_mfma_f32_32x32x2f32(p4.y, vp[HD + 4], pv, 0, 0, 0);
                    pv = __builtin_amdgcn_mfma_f32_32x32x2f32(p4.z, vp[2 * (HD + 4)], pv, 0, 0, 0);
                    pv = __builtin_amdgcn_mfma_f32_32x32x2f32(p4.w, vp[3 * (HD + 4)], pv, 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) o[r] = o[r] * s_alpha[tile_row(r, wr, hh)] + pv[r];
        }
        __syncthreads();
    }
    if (qd == 0) s_l[srow] = l_run;
    if (a.stats != nullptr && qd == 0 && q0 + srow < a.Kq) {   // what the backward recomputes P from
        float *st = a.stats + (((size_t)b * a.H + head) * a.Kq + q0 + srow) * 2;
        st[0] = m_run; st[1] = l_run;
    }
    if (HD == 32 && wc == 1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) Ps[0][tile_row(r, wr, hh)][li] = o[r];
    }
    __syncthreads();
    if (HD == 32 && wc == 1) return;
    const int col = (HD == 64 ? wc * 32 : 0) + li;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = tile_row(r, wr, hh);
        float v = o[r];
        if (HD == 32) v = v + Ps[0][row][li];
        const float l = s_l[row];
        v = l == 0.0f ? 0.0f : v / l;                      // no key at all: zeros
        if (q0 + row < a.Kq) a.out[((size_t)b * a.Kq + q0 + row) * ((size_t)a.H * HD) + head * HD + col] = v;
    }
}

// ---- LayerNorm ------------------------------------------------------------------------------------------------------------------------
struct DecLnArgs {
    const float *x, *w, *b, *w2, *b2;
    float *out, *out2;
    int n, C;
    float eps;
};

// 16 lanes hold a row (head.h's layout).  mean = (sum in ascending channel order per lane, then sum16) / C, then the centred squares the
// same way: never E[x^2] - E[x]^2.
__device__ __forceinline__ void dec_ln_row(float4 (&x)[8], int nm, int C, float eps, const float *w, const float *b, int l)
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
        if (m < nm) {
            const float4 g = ld4(w + 64 * m + 4 * l), h = ld4(b + 64 * m + 4 * l);
            x[m].x = x[m].x / den * g.x + h.x; x[m].y = x[m].y / den * g.y + h.y;
            x[m].z = x[m].z / den * g.z + h.z; x[m].w = x[m].w / den * g.w + h.w;
        }
}

__global__ __launch_bounds__(256) void k_dec_ln(DecLnArgs a)
{
    const int l = threadIdx.x & 15;
    const long row = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int nm = a.C >> 6;
    const bool have = row < a.n;
    float4 x[8];
#pragma unroll
    for (int m = 0; m < 8; ++m)
        x[m] = (m < nm && have) ? ld4(a.x + (size_t)row * a.C + 64 * m + 4 * l) : make_float4(0.f, 0.f, 0.f, 0.f);
    dec_ln_row(x, nm, a.C, a.eps, a.w, a.b, l);
#pragma unroll
    for (int m = 0; m < 8; ++m)
        if (m < nm && have) st4(a.out + (size_t)row * a.C + 64 * m + 4 * l, x[m]);
    if (a.out2 == nullptr) return;
    dec_ln_row(x, nm, a.C, a.eps, a.w2, a.b2, l);
#pragma unroll
    for (int m = 0; m < 8; ++m)
        if (m < nm && have) st4(a.out2 + (size_t)row * a.C + 64 * m + 4 * l, x[m]);
}

static int dec_rows_ok(const char *who, long n)
{
    PTX_REQUIRE(n >= 1 && n <= (1l << 30), "%s: n=%ld rows (1 to 2^30)", who, n);
    return PTX_OK;
}

}  // namespace ptx

using namespace ptx;

extern "C" {

int ptx_dec_posembed(const float *x, long n, int cin, const float *w1, const float *b1, const float *w2, const float *b2, int C, float *out,
                     void *stream)
{
    const char *who = "ptx_dec_posembed";
    PTX_TRY(dec_rows_ok(who, n));
    PTX_REQUIRE(cin >= 1 && cin <= kDecMaxPos && sp_width_ok(C), "%s: cin=%d C=%d (cin: 1 to %d; C: a multiple of 64 up to 512)", who, cin, C,
                kDecMaxPos);
    PTX_REQUIRE(x && w1 && b1 && w2 && b2 && out, "%s: null argument", who);
    PTX_REQUIRE(sp_aligned16({w2, out}), "%s: w2 and out must be 16-byte aligned", who);
    DecGemmArgs a{};
    a.x = x; a.w1 = w1; a.b1 = b1; a.w = w2; a.bias = b2; a.out = out; a.n = (int)n; a.Cin = C; a.Cout = C; a.cin0 = cin;
    hipLaunchKernelGGL((k_dec_gemm<DEC_POSEMBED>), dim3(cdiv((int)n, 64), C / 64), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    PTX_LAUNCHED("k_dec_gemm<posembed>");
    return PTX_OK;
}

int ptx_dec_linear(const float *x, const float *add, int add_cols, long n, const float *weight, const float *bias, int Cin, int Cout, int relu,
                   const float *residual, float *out, void *stream)
{
    const char *who = "ptx_dec_linear";
    PTX_TRY(dec_rows_ok(who, n));
    PTX_REQUIRE(Cin >= 64 && Cin <= kDecMaxCin && Cin % 64 == 0 && Cout >= 64 && Cout <= kDecMaxCout && Cout % 64 == 0,
                "%s: Cin=%d Cout=%d (multiples of 64; Cin up to %d, Cout up to %d)", who, Cin, Cout, kDecMaxCin, kDecMaxCout);
    PTX_REQUIRE((relu == 0 || relu == 1) && add_cols >= 0 && add_cols <= Cout && add_cols % 64 == 0,
                "%s: relu=%d add_cols=%d (relu: 0 or 1; add_cols: a multiple of 64 from 0 to Cout=%d)", who, relu, add_cols, Cout);
    PTX_REQUIRE(x && weight && out, "%s: null argument", who);
    PTX_REQUIRE(sp_aligned16({x, add, weight}), "%s: x, add and weight must be 16-byte aligned", who);
    DecGemmArgs a{};
    a.x = x; a.add = add; a.add_cols = add_cols; a.w = weight; a.bias = bias; a.residual = residual; a.out = out;
    a.n = (int)n; a.Cin = Cin; a.Cout = Cout; a.relu = relu;
    hipLaunchKernelGGL((k_dec_gemm<DEC_LINEAR>), dim3(cdiv((int)n, 64), Cout / 64), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    PTX_LAUNCHED("k_dec_gemm<linear>");
    return PTX_OK;
}

static int dec_attention(const char *who, const float *q, long ldq, const float *k, long ldk, const float *v, long ldv, const uint8_t *mask,
                         int B, int Kq, int L, int H, int hd, float *out, float *stats, bool want_stats, void *stream)
{
    PTX_REQUIRE(B >= 1 && B <= kHeadMaxScenes && Kq >= 1 && Kq <= kHeadMaxK && L >= 1 && L <= (1 << 24),
                "%s: B=%d Kq=%d L=%d (B: 1 to 64; Kq: 1 to 1024; L: 1 to 2^24)", who, B, Kq, L);
    PTX_REQUIRE((hd == 32 || hd == 64) && H >= 1 && H * hd <= 512, "%s: H=%d hd=%d (hd: 32 or 64; H hd up to 512)", who, H, hd);
    const long C = (long)H * hd;
    PTX_REQUIRE(ldq >= C && ldk >= C && ldv >= C && ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0 && ldq <= (1 << 20) && ldk <= (1 << 20) &&
                    ldv <= (1 << 20),
                "%s: ldq=%ld ldk=%ld ldv=%ld (row strides: multiples of 4 from H hd=%ld to 2^20)", who, ldq, ldk, ldv, C);
    PTX_REQUIRE(q && k && v && out && (stats || !want_stats), "%s: null argument", who);
    PTX_REQUIRE(sp_aligned16({q, k, v}), "%s: q, k and v must be 16-byte aligned", who);
    DecAttnArgs a{};
    a.q = q; a.k = k; a.v = v; a.mask = mask; a.out = out; a.stats = stats; a.B = B; a.Kq = Kq; a.L = L; a.H = H; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv;
    a.scale = 1.0f / sqrtf((float)hd);
    const dim3 grid(cdiv(Kq, 64), H, B);
    if (hd == 64) hipLaunchKernelGGL((k_dec_attn<64>), grid, dim3(256), 0, static_cast<hipStream_t>(stream), a);
    else hipLaunchKernelGGL((k_dec_attn<32>), grid, dim3(256), 0, static_cast<hipStream_t>(stream), a);
    PTX_LAUNCHED("k_dec_attn");
    return PTX_OK;
}

int ptx_dec_attention(const float *q, long ldq, const float *k, long ldk, const float *v, long ldv, const uint8_t *mask, int B, int Kq, int L,
                      int H, int hd, float *out, void *stream)
{
    return dec_attention("ptx_dec_attention", q, ldq, k, ldk, v, ldv, mask, B, Kq, L, H, hd, out, nullptr, false, stream);
}

int ptx_dec_attention_stats(const float *q, long ldq, const float *k, long ldk, const float *v, long ldv, const uint8_t *mask, int B, int Kq,
                            int L, int H, int hd, float *out, float *stats, void *stream)
{
    return dec_attention("ptx_dec_attention_stats", q, ldq, k, ldk, v, ldv, mask, B, Kq, L, H, hd, out, stats, true, stream);
}

int ptx_dec_ln(const float *x, long n, int C, const float *weight, const float *bias, float eps, float *out, const float *weight2,
               const float *bias2, float *out2, void *stream)
{
    const char *who = "ptx_dec_ln";
    PTX_TRY(dec_rows_ok(who, n));
    PTX_REQUIRE(sp_width_ok(C) && eps > 0.0f, "%s: C=%d eps=%g (C: a multiple of 64 up to 512; eps > 0)", who, C, (double)eps);
    PTX_REQUIRE(x && weight && bias && out, "%s: null argument", who);
    PTX_REQUIRE((out2 == nullptr) == (weight2 == nullptr) && (out2 == nullptr) == (bias2 == nullptr),
                "%s: the second LayerNorm needs weight2, bias2 and out2 together", who);
    PTX_REQUIRE(sp_aligned16({x, weight, bias, out, weight2, bias2, out2}), "%s: the operands must be 16-byte aligned", who);
    const DecLnArgs a{x, weight, bias, weight2, bias2, out, out2, (int)n, C, eps};
    hipLaunchKernelGGL(k_dec_ln, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    PTX_LAUNCHED("k_dec_ln");
    return PTX_OK;
}

int ptx_dec_boxes(const float *h, const float *weight, const float *bias, int C, const float *coords, long n, float *boxes, void *stream)
{
    const char *who = "ptx_dec_boxes";
    PTX_TRY(dec_rows_ok(who, n));
    PTX_REQUIRE(sp_width_ok(C), "%s: C=%d (a multiple of 64 up to 512)", who, C);
    PTX_REQUIRE(h && weight && coords && boxes, "%s: null argument", who);
    PTX_REQUIRE(sp_aligned16({h}), "%s: h must be 16-byte aligned", who);
    const HeadBoxArgs a{h, weight, bias, nullptr, coords, nullptr, nullptr, nullptr, boxes, (int)n, 0, 0, C};
    hipLaunchKernelGGL((k_head_boxes<false>), dim3((unsigned)((n + 15) / 16)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    PTX_LAUNCHED("k_head_boxes");
    return PTX_OK;
}

int ptx_dec_scores(const float *hidden, int NL, int B, int K, int C, const float *text, const uint8_t *text_mask, int T, int max_text_len,
                   int scaled, const float *bias, float *out, void *stream)
{
    const char *who = "ptx_dec_scores";
    PTX_REQUIRE(NL >= 1 && NL <= 64 && B >= 1 && B <= kHeadMaxScenes && K >= 1 && K <= kHeadMaxK && sp_width_ok(C),
                "%s: NL=%d B=%d K=%d C=%d (NL, B: 1 to 64; K: 1 to 1024; C: a multiple of 64 up to 512)", who, NL, B, K, C);
    PTX_REQUIRE(T >= 1 && T <= max_text_len && max_text_len <= kHeadMaxText && (scaled == 0 || scaled == 1),
                "%s: T=%d max_text_len=%d scaled=%d (1 <= T <= max_text_len <= %d; scaled: 0 or 1)", who, T, max_text_len, scaled, kHeadMaxText);
    PTX_REQUIRE(hidden && text && text_mask && out, "%s: null argument", who);
    PTX_REQUIRE(sp_aligned16({hidden, text}), "%s: hidden and text must be 16-byte aligned", who);
    DecGemmArgs a{};
    a.x = hidden; a.w = text; a.bias = bias; a.out = out; a.mask = text_mask; a.Cin = C; a.B = B; a.K = K; a.T = T; a.ldo = max_text_len;
    a.scaled = scaled; a.divisor = sqrtf((float)C);
    hipLaunchKernelGGL((k_dec_gemm<DEC_SCORES>), dim3(cdiv(K, 64), cdiv(max_text_len, 64), NL * B), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a);
    PTX_LAUNCHED("k_dec_gemm<scores>");
    return PTX_OK;
}

}  // extern "C"
