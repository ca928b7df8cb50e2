// Query selection behind the neck: `pre_decoder` of the detector (detectors/sparse_featfusion_grounder_preshape.py:498-580) -- the lists
// `feats, scores, coords = self.neck_3d(...)` returns become the transformer decoder's operands.
//
//   ptx_qs_pack     the B per-scene (L_b,C) features and (L_b,3) coordinates are copied into (B,Lmax,C) / (B,Lmax,3) with zeros behind
//       them; the padding mask (B,Lmax) and the negated text mask (B,T) are written by the same launch.  The B source pointers and row
//       counts travel by value in the kernel-argument struct.
//   ptx_qs_score    ContrastiveEmbed and its max over the tokens (grounding_head.py:62-99, `enc_outputs_class.max(-1)[0]`): one
//       work-group per (scene, 64-row tile) multiplies the tile by the scene's text rows on the exact-fp32 matrix instruction, 64 tokens at
//       a time (head.h's tile64_nt in its blocked order), and keeps the running maximum of the unmasked columns in registers:
//       the (B,L,max_text_len) tensor never exists.  Division by a positive constant and addition of a constant are monotone, so the
//       maximum is taken of the raw products and scale and bias are applied once; a NaN among the unmasked products makes the score NaN
//       (torch.max's rule; k_neck_head's flag), padded rows and scenes without a token get -inf.
//   ptx_qs_topk     torch.topk(score, K, dim=1, sorted=True)[1]: one work-group per scene runs topk_threshold (head.h) for
//       the K-th key, collects the K kept rows as (key, ~row) pairs in LDS and sorts them (bitonic, at most 1024): descending key, the
//       lower row first among equal keys (integer LDS counters only; the sort makes the result independent of their order).  Also
//       writes the inverse index (B,Lmax) of the backward.
//   ptx_qs_linear   one Linear (+ ReLU) of the regression branch over the K selected rows only: the same tile and order (nn.Linear's
//       (out,in) weight has k contiguous already), rows gathered through the index; head.h's linear_store, ReLU keeps a NaN.
//   ptx_qs_decode   the last Linear (C -> 9), `_bbox_pred_to_bbox` (baseline coder, 9 values) and the gathers of query / query_coords:
//       k_head_boxes<true> (head.h).
//   ptx_qs_bwd      dfeats_b[r] = dfeats_padded[b,r] (+ dquery[b,q] where index[b,q] = r) through the inverse index: no atomics.
//
// fp32, no float atomics, fixed summation orders (bitwise reproducible), everything on the caller's stream, no host wait.  Held to the
// numpy restatements of proxytransformation_amd/query_select_host.py.
#include "head.h"

namespace ptx {

struct QsRows { int32_t n[kHeadMaxScenes]; };

// ---- pack ---------------------------------------------------------------------------------------------------------------------
struct QsPackArgs {
    const float *feats[kHeadMaxScenes]; const float *xyz[kHeadMaxScenes]; QsRows rows;
    const uint8_t *text_mask;                               // (B,T), 1 = a token
    float *out_feats, *out_coords; uint8_t *pad_mask, *text_attn;
    int B, C, Lmax, T;
};

// thread = (row, 4 channels) of scene blockIdx.y; the row's first thread also writes its coordinates and its mask byte
__global__ __launch_bounds__(256) void k_qs_pack(QsPackArgs a)
{
    const int b = blockIdx.y;
    if (blockIdx.x == 0)
        for (int t = threadIdx.x; t < a.T; t += 256) a.text_attn[(size_t)b * a.T + t] = a.text_mask[(size_t)b * a.T + t] ? 0 : 1;
    const int c4n = a.C >> 2;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const int r = (int)(t / c4n), c4 = (int)(t - (long)r * c4n);
    if (r >= a.Lmax) return;
    const bool have = r < a.rows.n[b];
    const size_t o = (size_t)b * a.Lmax + r;
    st4(a.out_feats + o * a.C + c4 * 4, have ? ld4(a.feats[b] + (size_t)r * a.C + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f));
    if (c4 == 0) {
        const float *p = a.xyz[b] + (size_t)r * 3;
        a.out_coords[o * 3 + 0] = have ? p[0] : 0.0f;
        a.out_coords[o * 3 + 1] = have ? p[1] : 0.0f;
        a.out_coords[o * 3 + 2] = have ? p[2] : 0.0f;
        a.pad_mask[o] = have ? 0 : 1;
    }
}

// ---- score / linear: the 64 x 64 NT tile ------------------------------------------------------------------------------------------
struct QsGemmArgs {
    const float *x;                                         // rows of width C: the padded features (score), the source rows (linear)
    const float *w;                                         // (n, C) with k contiguous: the text rows (B,T,C), an nn.Linear weight (Cout,C)
    const float *bias; float *out;
    const long long *index;                                 // linear: (B,K) rows to gather, row = b * Lmax + index; null: the rows themselves
    const uint8_t *text_mask;
    QsRows rows;
    int B, Lmax, C, T, K, n_src, n_out, Cout, scaled, relu;
    float divisor;
};

// SCORE: blockIdx = (row tile, scene); columns = tokens, looped in tiles of 64; out (B,Lmax) = max over the unmasked tokens.
// else: blockIdx = (row tile, column tile) of out (n_out,Cout) = act(x[gather] @ w^T + bias).
template <bool SCORE>
__global__ __launch_bounds__(256) void k_qs_gemm(QsGemmArgs a)
{
    __shared__ int s_src[64];
    __shared__ float s_max[2][64];
    __shared__ int s_nan[2][64];
    const Tile64 t;
    const int tid = t.tid;
    const int row0 = blockIdx.x * 64;
    const int b = SCORE ? blockIdx.y : 0, col0 = SCORE ? 0 : blockIdx.y * 64;
    const int Lb = SCORE ? a.rows.n[b] : 0;
    if (SCORE && row0 >= Lb) {                              // a tile of padding (work-group uniform)
        if (tid < 64 && row0 + tid < a.Lmax) a.out[(size_t)b * a.Lmax + row0 + tid] = -INFINITY;
        return;
    }
    if (tid < 64) {                                         // the tile's source rows, -1: a zero row
        const int row = row0 + tid;
        long src = -1;
        if (SCORE) {
            if (row < Lb) src = (long)b * a.Lmax + row;
        } else if (row < a.n_out) {
            src = row;
            if (a.index) {
                const long long i = a.index[row];
                src = (i >= 0 && i < a.Lmax) ? (long)(row / a.K) * a.Lmax + i : -1;
            }
            if (src >= a.n_src) src = -1;
        }
        s_src[tid] = (int)src;
    }
    __syncthreads();
    const int nchunk = a.C >> 6;
    const int ncols = SCORE ? a.T : a.Cout;
    const int nsteps = (SCORE ? (a.T + 63) >> 6 : 1) * nchunk;
    const float *wbase = a.w + (SCORE ? (size_t)b * a.T * a.C : 0);
    f32x16 tot;
    float best[16];
    int nan = 0;                                            // bit r: a NaN among the unmasked columns of accumulator row r
#pragma unroll
    for (int i = 0; i < 16; ++i) { tot[i] = 0.0f; best[i] = -INFINITY; }

    tile64_nt<true>(
        t, nsteps, tot,
        [&](int s) { return make_int2((s % nchunk) << 6, col0 + ((s / nchunk) << 6)); },       // (first channel, first column) of step s
        [&](float4 &v, int2 p, int row, int kq) {
            const int src = s_src[row];
            v = src >= 0 ? ld4(a.x + (size_t)src * a.C + p.x + kq) : make_float4(0.f, 0.f, 0.f, 0.f);
        },
        [&](float4 &v, int2 p, int row, int kq) {
            v = p.y + row < ncols ? ld4(wbase + (size_t)(p.y + row) * a.C + p.x + kq) : make_float4(0.f, 0.f, 0.f, 0.f);
        },
        [&](int s) {
            if (SCORE && (s + 1) % nchunk == 0) {           // a token tile is complete: fold its unmasked columns into the running maximum
                const int tok = ((s / nchunk) << 6) + t.col();
                const bool valid = tok < a.T && a.text_mask[(size_t)b * a.T + tok] != 0;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if (valid) {
                        best[r] = fmaxf(best[r], tot[r]);
                        nan |= (tot[r] != tot[r]) ? (1 << r) : 0;
                    }
                    tot[r] = 0.0f;
                }
            }
        });
    if (!SCORE) {
        linear_store(t, tot, row0, a.n_out, col0 + t.col(), a.Cout, a.bias, a.relu, nullptr, a.out);
        return;
    }
    // the 32 columns of a wave half by xor 16, 8, 4, 2, 1 (the maximum and the flags are order-free), the two column halves through LDS
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
        for (int d = 16; d >= 1; d >>= 1) best[r] = fmaxf(best[r], __shfl_xor(best[r], d, 64));
    }
#pragma unroll
    for (int d = 16; d >= 1; d >>= 1) nan |= __shfl_xor(nan, d, 64);
    if (t.li == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s_max[t.wc][t.row(r)] = best[r];
            s_nan[t.wc][t.row(r)] = (nan >> r) & 1;
        }
    }
    __syncthreads();
    if (tid < 64 && row0 + tid < a.Lmax) {
        const bool valid = row0 + tid < Lb;
        const float v = contrastive_value(fmaxf(s_max[0][tid], s_max[1][tid]), valid, a.scaled, a.divisor, a.bias != nullptr,
                                          a.bias ? a.bias[0] : 0.0f);
        a.out[(size_t)b * a.Lmax + row0 + tid] = valid && (s_nan[0][tid] | s_nan[1][tid]) ? __builtin_nanf("") : v;
    }
}

// ---- sorted top-k -----------------------------------------------------------------------------------------------------------------
struct QsTopkArgs {
    const float *score; long long *index; int32_t *inv;     // (B,Lmax), (B,K), (B,Lmax) or null
    QsRows rows;
    int B, Lmax, K;
};

// One work-group per scene.  (1) topk_threshold (head.h) finds the K-th largest key.  (2) Every thread walks a contiguous run of rows:
// rows above the threshold key take a slot from an integer LDS counter (there are exactly K - need of them; their order in LDS is
// arbitrary, the sort below puts them in place), rows AT the threshold are counted, a prefix scan over the threads ranks them in row
// order and the first `need` follow.  (3) The K pairs key << 32 | ~row are distinct: a bitonic sort of the next power of two, descending,
// gives larger key first and the lower row first among equal keys whatever the order they arrived in.
__global__ __launch_bounds__(256) void k_qs_topk(QsTopkArgs a)
{
    __shared__ TopkLds s_topk;
    __shared__ int s_cnt;
    __shared__ unsigned long long s_pair[kHeadMaxK];        // key << 32 | ~row: descending = larger key first, lower row first
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int hi = a.rows.n[b];                             // >= K (the host checks)
    const float *sc = a.score + (size_t)b * a.Lmax;
    if (a.inv)
        for (int i = tid; i < a.Lmax; i += 256) a.inv[(size_t)b * a.Lmax + i] = -1;
    int P = 1;
    while (P < a.K) P <<= 1;
    for (int p = tid; p < P; p += 256) s_pair[p] = 0ull;    // below every real pair (~row > 0)
    if (tid == 0) s_cnt = 0;
    int need;
    const uint32_t prefix = topk_threshold(sc, 0, hi, a.K, s_topk, need);
    // prefix: the K-th largest key; K - need rows lie above it, `need` of the rows that carry it follow, the lowest row indices first
    const int per = (hi + 255) >> 8, lo_t = min(tid * per, hi), hi_t = min(lo_t + per, hi);
    const int n_above = a.K - need;
    int eq = 0;
    for (int i = lo_t; i < hi_t; ++i) {
        const uint32_t key = topk_key(sc[i]);
        if (key > prefix) {
            const int slot = atomicAdd(&s_cnt, 1);
            if (slot < n_above) s_pair[slot] = ((unsigned long long)key << 32) | (uint32_t)~(uint32_t)i;
        }
        eq += key == prefix;
    }
    int inc = eq;                                           // rows at the threshold in this and the earlier threads of the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    __syncthreads();                                        // (the last pass's reads of s_topk.w are done)
    if (lane == 63) s_topk.w[wid] = inc;
    __syncthreads();
    int rank = inc - eq;
    for (int w = 0; w < wid; ++w) rank += s_topk.w[w];
    if (eq > 0 && rank < need) {
        for (int i = lo_t; i < hi_t && rank < need; ++i) {
            if (topk_key(sc[i]) != prefix) continue;
            s_pair[n_above + rank] = ((unsigned long long)prefix << 32) | (uint32_t)~(uint32_t)i;
            ++rank;
        }
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += 256) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i + j;
                const unsigned long long x = s_pair[i], y = s_pair[l];
                const bool desc = (i & k) == 0;
                if (desc ? x < y : x > y) { s_pair[i] = y; s_pair[l] = x; }
            }
            __syncthreads();
        }
    }
    for (int q = tid; q < a.K; q += 256) {
        const int row = (int)(~(uint32_t)s_pair[q]);
        if (row < 0 || row >= hi) continue;                 // (never: K <= rows)
        a.index[(size_t)b * a.K + q] = row;
        if (a.inv) a.inv[(size_t)b * a.Lmax + row] = q;
    }
}

// ---- backward -------------------------------------------------------------------------------------------------------------------
struct QsBwdArgs {
    const float *dfeats, *dquery; const int32_t *inv;       // (B,Lmax,C) or null, (B,K,C) or null, (B,Lmax)
    float *out;                                             // (sum of the rows, C): scene b at row start[b]
    QsRows rows; int32_t start[kHeadMaxScenes];
    int B, Lmax, K, C;
};

__global__ __launch_bounds__(256) void k_qs_bwd(QsBwdArgs a)
{
    const int b = blockIdx.y, c4n = a.C >> 2;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const int r = (int)(t / c4n), c4 = (int)(t - (long)r * c4n);
    if (r >= a.rows.n[b]) return;
    const size_t o = (size_t)b * a.Lmax + r;
    float4 v = a.dfeats ? ld4(a.dfeats + o * a.C + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    const int q = a.inv[o];
    if (a.dquery && q >= 0 && q < a.K) v = add4(v, ld4(a.dquery + ((size_t)b * a.K + q) * a.C + c4 * 4));
    st4(a.out + ((size_t)a.start[b] + r) * a.C + c4 * 4, v);
}

// the shape every entry point shares; the row counts: B ints of 0 .. Lmax
static int qs_shape(const char *who, int B, int Lmax, int C, const int32_t *rows, QsRows &out, long &total)
{
    PTX_REQUIRE(B >= 1 && B <= kHeadMaxScenes && Lmax >= 1 && Lmax <= (1 << 24) && sp_width_ok(C),
                "%s: B=%d Lmax=%d C=%d (B: 1 to 64; Lmax: 1 to 2^24; C: a multiple of 64 up to 512)", who, B, Lmax, C);
    PTX_REQUIRE(rows != nullptr, "%s: rows is null", who);
    total = 0;
    for (int b = 0; b < B; ++b) {
        PTX_REQUIRE(rows[b] >= 0 && rows[b] <= Lmax, "%s: rows[%d]=%d is outside 0 .. Lmax=%d", who, b, rows[b], Lmax);
        out.n[b] = rows[b];
        total += rows[b];
    }
    return PTX_OK;
}

static int qs_select_shape(const char *who, int B, int K, int Lmax, int C)
{
    PTX_REQUIRE(B >= 1 && B <= kHeadMaxScenes && K >= 1 && K <= kHeadMaxK && Lmax >= K && Lmax <= (1 << 24) && sp_width_ok(C),
                "%s: B=%d K=%d Lmax=%d C=%d (B: 1 to 64; K: 1 to 1024 and at most Lmax; Lmax up to 2^24; C: a multiple of 64 up to 512)", who,
                B, K, Lmax, C);
    return PTX_OK;
}

}  // namespace ptx

using namespace ptx;

extern "C" {

int ptx_qs_pack(const float *const *feats, const float *const *xyz, const int32_t *rows, int B, int C, int Lmax, const uint8_t *text_mask,
                int T, float *out_feats, float *out_coords, uint8_t *pad_mask, uint8_t *text_attn, void *stream)
{
    const char *who = "ptx_qs_pack";
    QsPackArgs a{};
    long total;
    PTX_TRY(qs_shape(who, B, Lmax, C, rows, a.rows, total));
    PTX_REQUIRE(T >= 1 && T <= kHeadMaxText, "%s: T=%d (1 to %d text tokens)", who, T, kHeadMaxText);
    PTX_REQUIRE(feats && xyz && text_mask && out_feats && out_coords && pad_mask && text_attn, "%s: null argument", who);
    for (int b = 0; b < B; ++b) {
        PTX_REQUIRE(rows[b] == 0 || (feats[b] && xyz[b]), "%s: scene %d has %d rows and a null pointer", who, b, rows[b]);
        PTX_REQUIRE(sp_aligned16({feats[b]}), "%s: the features of scene %d must be 16-byte aligned", who, b);
        a.feats[b] = feats[b]; a.xyz[b] = xyz[b];
    }
    PTX_REQUIRE(sp_aligned16({out_feats}), "%s: out_feats must be 16-byte aligned", who);
    a.text_mask = text_mask; a.out_feats = out_feats; a.out_coords = out_coords; a.pad_mask = pad_mask; a.text_attn = text_attn;
    a.B = B; a.C = C; a.Lmax = Lmax; a.T = T;
    const long threads = (long)Lmax * (C / 4);
    hipLaunchKernelGGL(k_qs_pack, dim3((unsigned)((threads + 255) / 256), B), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    PTX_LAUNCHED("k_qs_pack");
    return PTX_OK;
}

int ptx_qs_score(const float *feats, const int32_t *rows, int B, int Lmax, int C, const float *text, const uint8_t *text_mask, int T,
                 int scaled, const float *bias, float *score, void *stream)
{
    const char *who = "ptx_qs_score";
    QsGemmArgs a{};
    long total;
    PTX_TRY(qs_shape(who, B, Lmax, C, rows, a.rows, total));
    PTX_REQUIRE(T >= 1 && T <= kHeadMaxText && (scaled == 0 || scaled == 1), "%s: T=%d scaled=%d (1 to %d text tokens; scaled: 0 or 1)", who, T,
                scaled, kHeadMaxText);
    PTX_REQUIRE(feats && text && text_mask && score, "%s: null argument", who);
    PTX_REQUIRE(sp_aligned16({feats, text}), "%s: feats and text must be 16-byte aligned", who);
    a.x = feats; a.w = text; a.bias = bias; a.out = score; a.text_mask = text_mask;
    a.B = B; a.Lmax = Lmax; a.C = C; a.T = T; a.scaled = scaled; a.divisor = sqrtf((float)C);
    hipLaunchKernelGGL((k_qs_gemm<true>), dim3(cdiv(Lmax, 64), B), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    PTX_LAUNCHED("k_qs_gemm<score>");
    return PTX_OK;
}

int ptx_qs_topk(const float *score, const int32_t *rows, int B, int Lmax, int K, int64_t *index, int32_t *inv, void *stream)
{
    const char *who = "ptx_qs_topk";
    QsTopkArgs a{};
    long total;
    PTX_TRY(qs_select_shape(who, B, K, Lmax, 64));
    PTX_TRY(qs_shape(who, B, Lmax, 64, rows, a.rows, total));
    for (int b = 0; b < B; ++b) PTX_REQUIRE(rows[b] >= K, "%s: rows[%d]=%d is below K=%d", who, b, rows[b], K);
    PTX_REQUIRE(score && index, "%s: null argument", who);
    a.score = score; a.index = reinterpret_cast<long long *>(index); a.inv = inv; a.B = B; a.Lmax = Lmax; a.K = K;
    hipLaunchKernelGGL(k_qs_topk, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    PTX_LAUNCHED("k_qs_topk");
    return PTX_OK;
}

int ptx_qs_linear(const float *x, int n_src, const int64_t *index, int B, int K, int Lmax, const float *weight, const float *bias, int Cin,
                  int Cout, int relu, float *out, void *stream)
{
    const char *who = "ptx_qs_linear";
    PTX_TRY(qs_select_shape(who, B, K, index ? Lmax : K, Cin));
    PTX_REQUIRE(sp_width_ok(Cout) && n_src >= 1 && n_src <= (1 << 30) && (relu == 0 || relu == 1) && (index || n_src == B * K),
                "%s: Cout=%d n_src=%d relu=%d (Cout: a multiple of 64 up to 512; without an index n_src = B K = %d)", who, Cout, n_src, relu,
                B * K);
    PTX_REQUIRE(x && weight && out, "%s: null argument", who);
    PTX_REQUIRE(sp_aligned16({x, weight}), "%s: x and weight must be 16-byte aligned", who);
    QsGemmArgs a{};
    a.x = x; a.w = weight; a.bias = bias; a.out = out; a.index = reinterpret_cast<const long long *>(index);
    a.B = B; a.Lmax = Lmax; a.C = Cin; a.K = K; a.n_src = n_src; a.n_out = B * K; a.Cout = Cout; a.relu = relu;
    hipLaunchKernelGGL((k_qs_gemm<false>), dim3(cdiv(B * K, 64), Cout / 64), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    PTX_LAUNCHED("k_qs_gemm<linear>");
    return PTX_OK;
}

int ptx_qs_decode(const float *h, const float *weight, const float *bias, int C, const float *feats, const float *coords,
                  const int64_t *index, int B, int K, int Lmax, float *query, float *qcoords, float *boxes, void *stream)
{
    const char *who = "ptx_qs_decode";
    PTX_TRY(qs_select_shape(who, B, K, Lmax, C));
    PTX_REQUIRE(weight && feats && coords && index && query && qcoords && boxes, "%s: null argument", who);
    PTX_REQUIRE(sp_aligned16({h, feats, query}), "%s: h, feats and query must be 16-byte aligned", who);
    const HeadBoxArgs a{h, weight, bias, feats, coords, reinterpret_cast<const long long *>(index), query, qcoords, boxes, B * K, K, Lmax, C};
    hipLaunchKernelGGL((k_head_boxes<true>), dim3(cdiv(B * K, 16)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    PTX_LAUNCHED("k_head_boxes");
    return PTX_OK;
}

int ptx_qs_bwd(const float *dfeats, const float *dquery, const int32_t *inv, const int32_t *rows, int B, int Lmax, int K, int C, float *out,
               void *stream)
{
    const char *who = "ptx_qs_bwd";
    QsBwdArgs a{};
    long total;
    PTX_TRY(qs_select_shape(who, B, K, Lmax, C));
    PTX_TRY(qs_shape(who, B, Lmax, C, rows, a.rows, total));
    PTX_REQUIRE(total < (1l << 30), "%s: %ld rows is out of range", who, total);
    if (total == 0) return PTX_OK;
    PTX_REQUIRE(inv && out, "%s: null argument", who);
    PTX_REQUIRE(sp_aligned16({dfeats, dquery, out}), "%s: the gradients must be 16-byte aligned", who);
    a.dfeats = dfeats; a.dquery = dquery; a.inv = inv; a.out = out; a.B = B; a.Lmax = Lmax; a.K = K; a.C = C;
    for (int b = 0, s = 0; b < B; ++b) { a.start[b] = s; s += rows[b]; }
    const long threads = (long)Lmax * (C / 4);
    hipLaunchKernelGGL(k_qs_bwd, dim3((unsigned)((threads + 255) / 256), B), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    PTX_LAUNCHED("k_qs_bwd");
    return PTX_OK;
}

}  // extern "C"
