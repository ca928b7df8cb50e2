// The text encoder in front of text_feat_map: the eval forward of CLIPTextModel (12 pre-norm layers at the shipped shape, head dimension 64,
// quick-GELU, a causal mask plus the tokenizer's padding mask) up to last_hidden_state.
//
//   ptx_txt_embed       x[b,t] = token_embedding[ids[b,t]] + position_embedding[t]; an id outside [0, vocab) reads nothing and fills its row
//       with NaN.
//   ptx_txt_ln_linear   out (n,Cout) = act(LayerNorm(x) @ W^T + bias), two launches: the mean and 1 / sqrt(var + eps) of every row once (16
//       lanes per row, head.h's order, the centred variance: never E[x^2] - E[x]^2), then head.h's 64 x 64 tile normalises x while it
//       stages it, so the normalised tensor never exists.  act: none or quick-GELU v / (1 + expf(-1.702 v)).  [q|k|v] and fc1.
//   ptx_txt_attention   causal self attention on the [q|k|v] rows: work-group = (16 queries, head, text); key j is admitted for query t
//       iff j <= t and mask[b,j].  The whole row at once (T <= 256): the scores of the admitted keys into LDS with their maximum, then
//       p = expf(s - m) and its sum, then P V over the admitted keys in ascending order.  A key that is masked, or behind the tile's last
//       query, is never read; a key tile without an admitted key is skipped; a query without an admitted key gets zeros.
//   ptx_txt_linear      out (n,Cout) = x @ W^T + bias (+ residual) at Cin up to 5120: ptx_dec_linear's tile, accumulating straight through in
//       ascending k.  Beyond 768 input channels the contraction is cut into slices of equal length (a function of Cin alone, so a row's
//       bits do not depend on how many rows there are); each slice writes its sums to the workspace and a second launch adds them in
//       ascending order, then the bias, then the residual.  out_proj and fc2.
//   ptx_txt_ln          LayerNorm over rows of width C up to 1280 (final_layer_norm), the same statistics as ptx_txt_ln_linear.
//
// fp32, no float atomics, fixed summation orders (bitwise reproducible), everything on the caller's stream, no host wait.  Held to the
// numpy restatement of proxytransformation_amd/text_encoder_host.py.
#include "head.h"

namespace ptx {

constexpr int kTxtMaxC = 1280, kTxtMaxI = 5120, kTxtMaxT = 256, kTxtSlice = 768, kTxtQ = 16;

// the slices of a contraction over Cin channels: a function of Cin alone
static inline int txt_ksplit(int Cin) { return (Cin + kTxtSlice - 1) / kTxtSlice; }
static inline int txt_slice_steps(int Cin) { return cdiv(Cin >> 6, txt_ksplit(Cin)); }

// ---- rows of 16 lanes ---------------------------------------------------------------------------------------------------------------
// mean and 1 / sqrt(var + eps) of a row of C = 64 nm channels, by the row's 16 lanes (lane l: channels 64 m + 4 l .. + 3, m ascending, then
// sum16): the mean first, then the centred squares.  Every lane ends with the same pair.  The lane's share of the row is loaded once, all
// of it in flight together.
constexpr int kTxtMaxNm = kTxtMaxC / 64;
__device__ __forceinline__ void txt_row_stats(const float *x, int nm, int C, float eps, int l, float &mean, float &rstd)
{
    float4 v[kTxtMaxNm];
#pragma unroll
    for (int m = 0; m < kTxtMaxNm; ++m) v[m] = m < nm ? ld4(x + 64 * m + 4 * l) : make_float4(0.f, 0.f, 0.f, 0.f);
    float s = 0.0f;
#pragma unroll
    for (int m = 0; m < kTxtMaxNm; ++m)
        if (m < nm) { s = s + v[m].x; s = s + v[m].y; s = s + v[m].z; s = s + v[m].w; }
    mean = sum16(s) / (float)C;
    float ss = 0.0f;
#pragma unroll
    for (int m = 0; m < kTxtMaxNm; ++m)
        if (m < nm) {
            const float dx = v[m].x - mean, dy = v[m].y - mean, dz = v[m].z - mean, dw = v[m].w - mean;
            ss = ss + dx * dx; ss = ss + dy * dy; ss = ss + dz * dz; ss = ss + dw * dw;
        }
    rstd = 1.0f / sqrtf(sum16(ss) / (float)C + eps);
}

__device__ __forceinline__ float4 txt_normalise(float4 v, float mean, float rstd, float4 g, float4 h)
{
    v.x = (v.x - mean) * rstd * g.x + h.x; v.y = (v.y - mean) * rstd * g.y + h.y;
    v.z = (v.z - mean) * rstd * g.z + h.z; v.w = (v.w - mean) * rstd * g.w + h.w;
    return v;
}

struct TxtEmbedArgs {
    const long long *ids; const float *tok, *pos; float *out;
    int n, T, vocab, C;
};

// one thread per four channels of a row
__global__ __launch_bounds__(256) void k_txt_embed(TxtEmbedArgs a)
{
    const int c4 = a.C >> 2;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)a.n * c4) return;
    const int row = (int)(e / c4), c = (int)(e - (long)row * c4) * 4;
    const long long id = a.ids[row];
    float4 v = make_float4(NAN, NAN, NAN, NAN);
    if (id >= 0 && id < a.vocab) v = add4(ld4(a.tok + (size_t)id * a.C + c), ld4(a.pos + (size_t)(row % a.T) * a.C + c));
    st4(a.out + (size_t)row * a.C + c, v);
}

struct TxtLnArgs {
    const float *x, *w, *b; float *out;
    int n, C;
    float eps;
};

__global__ __launch_bounds__(256) void k_txt_ln(TxtLnArgs a)
{
    const int l = threadIdx.x & 15, nm = a.C >> 6;
    const long row = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const float *x = a.x + (size_t)(row < a.n ? row : a.n - 1) * a.C;      // a row behind the end repeats the last one and stores nothing
    float mean, rstd;
    txt_row_stats(x, nm, a.C, a.eps, l, mean, rstd);
    if (row >= a.n) return;
    for (int m = 0; m < nm; ++m) {
        const int c = 64 * m + 4 * l;
        st4(a.out + (size_t)row * a.C + c, txt_normalise(ld4(x + c), mean, rstd, ld4(a.w + c), ld4(a.b + c)));
    }
}

// stats (n,2) = (mean, rstd) of every row: what the tile of ptx_txt_ln_linear normalises with.  In the tile itself the same work took a
// third of the launch: every column tile repeated it for its 64 rows, four rows per thread one after the other (profiles/text_encoder.txt)
__global__ __launch_bounds__(256) void k_txt_stats(const float *x, int n, int C, float eps, float *stats)
{
    const int l = threadIdx.x & 15;
    const long row = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
    float mean, rstd;
    txt_row_stats(x + (size_t)(row < n ? row : n - 1) * C, C >> 6, C, eps, l, mean, rstd);
    if (row < n && l == 0) { stats[2 * row] = mean; stats[2 * row + 1] = rstd; }
}

// ---- the 64 x 64 NT tile: LayerNorm -> Linear, Linear + residual --------------------------------------------------------------------------
struct TxtGemmArgs {
    const float *x;                                         // (n,Cin)
    const float *ln_w, *ln_b, *stats;                       // LN: (Cin), (Cin), (n,2) = (mean, rstd) per row
    const float *w;                                         // (Cout,Cin) with k contiguous
    const float *bias, *residual; float *out;               // (Cout) or null, (n,Cout) or null, (n,Cout)
    float *part;                                            // sliced: (slices,n,Cout), the sums of each slice; else null
    int n, Cin, Cout, act, slice_steps;
};

// blockIdx = (row tile, column tile, slice of the contraction)
template <bool LN>
__global__ __launch_bounds__(256) void k_txt_gemm(TxtGemmArgs a)
{
    const Tile64 t;
    const int row0 = blockIdx.x * 64, col0 = blockIdx.y * 64;
    const int nsteps_all = a.Cin >> 6, s0 = blockIdx.z * a.slice_steps;
    const int nsteps = min(a.slice_steps, nsteps_all - s0);
    const int ar = t.tid >> 4;
    float mean[4] = {0.f, 0.f, 0.f, 0.f}, rstd[4] = {0.f, 0.f, 0.f, 0.f};      // of the staging rows ar + 16 i
    if (LN) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int grow = row0 + ar + 16 * i;
            if (grow < a.n) { mean[i] = a.stats[2 * grow]; rstd[i] = a.stats[2 * grow + 1]; }
        }
    }
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;

    // head.h's tile64_nt<false> -- the same staging, the same straight-through order -- except that a quad of x is normalised when it is
    // STORED to LDS, a step after its load: normalised in the load (tile64_nt's a_quad) the arithmetic waits for the load in front of the
    // step's matrix instructions instead of behind them (profiles/text_encoder.txt: 50 -> 41 us per [q|k|v] launch)
    __shared__ __attribute__((aligned(16))) float As[2][64][LDT];
    __shared__ __attribute__((aligned(16))) float Ws[2][64][LDT];
    const int kq = (t.tid & 15) * 4;
    float4 av[4], wv[4], g4 = make_float4(0.f, 0.f, 0.f, 0.f), h4 = g4;
    auto fetch = [&](int s) {
        const int c0 = ((s0 + s) << 6) + kq;
        if (LN) { g4 = ld4(a.ln_w + c0); h4 = ld4(a.ln_b + c0); }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int grow = row0 + ar + 16 * i;
            av[i] = grow < a.n ? ld4(a.x + (size_t)grow * a.Cin + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
            wv[i] = ld4(a.w + (size_t)(col0 + ar + 16 * i) * a.Cin + c0);
        }
    };
    fetch(0);
    for (int s = 0; s < nsteps; ++s) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float4 v = av[i];
            if (LN && row0 + ar + 16 * i < a.n) v = txt_normalise(v, mean[i], rstd[i], g4, h4);
            st4(&As[kq >> 5][ar + 16 * i][kq & 31], v);
            st4(&Ws[kq >> 5][ar + 16 * i][kq & 31], wv[i]);
        }
        __syncthreads();
        if (s + 1 < nsteps) fetch(s + 1);                   // in flight behind this step's matrix instructions
        g64_step(As, Ws, 0, t.wr * 32 + t.li, t.wc * 32 + t.li, t.hh, acc);
        g64_step(As, Ws, 1, t.wr * 32 + t.li, t.wc * 32 + t.li, t.hh, acc);
        __syncthreads();
    }
    const int col = col0 + t.col();
    if (a.part != nullptr) {                                // a slice's sums; k_txt_slices finishes
        float *part = a.part + (size_t)blockIdx.z * a.n * a.Cout;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = row0 + t.row(r);
            if (row < a.n) part[(size_t)row * a.Cout + col] = acc[r];
        }
        return;
    }
    const float b = a.bias ? a.bias[col] : 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = row0 + t.row(r);
        if (row >= a.n) continue;
        float v = acc[r];
        if (a.bias) v = v + b;
        if (a.act) v = v / (1.0f + expf(-1.702f * v));
        if (a.residual) v = v + a.residual[(size_t)row * a.Cout + col];
        a.out[(size_t)row * a.Cout + col] = v;
    }
}

// out = ((slice 0 + slice 1) + ...) + bias (+ residual): one thread per four columns of a row
__global__ __launch_bounds__(256) void k_txt_slices(const float *part, int slices, int n, int Cout, const float *bias, const float *residual,
                                                    float *out)
{
    const int c4 = Cout >> 2;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)n * c4) return;
    const int row = (int)(e / c4), c = (int)(e - (long)row * c4) * 4;
    const size_t at = (size_t)row * Cout + c, plane = (size_t)n * Cout;
    float4 v = ld4(part + at);
    for (int z = 1; z < slices; ++z) v = add4(v, ld4(part + z * plane + at));
    if (bias) v = add4(v, ld4(bias + c));
    if (residual) v = add4(v, ld4(residual + at));
    st4(out + at, v);
}

// ---- causal attention -----------------------------------------------------------------------------------------------------------------
struct TxtAttnArgs {
    const float *qkv;                                       // (B,T,3 C): [q|k|v], head h at column h 64 of each
    const uint8_t *mask;                                    // (B,T), 1 = a token; null: every key is one
    float *out;                                             // (B,T,C)
    int B, T, H;
};

// blockIdx = (query tile of 16, head, text); thread = (query tid >> 4, lane l = tid & 15).  Key tiles of 64 up to the tile's last query:
// K staged in LDS, lane l takes the whole 64-channel product of the keys l, l + 16, l + 32, l + 48 of the tile (ascending channels) for
// its query; the maximum and the sum of p over the lane's keys in ascending order, then across the 16 lanes (xor 8, 4, 2, 1).  Then V
// staged the same way, lane l owns the output channels 4 l .. 4 l + 3 and adds p v over the admitted keys in ascending order.
__global__ __launch_bounds__(256) void k_txt_attn(TxtAttnArgs a)
{
    __shared__ __attribute__((aligned(16))) float Qs[kTxtQ][64];
    __shared__ __attribute__((aligned(16))) float KV[64][68];
    __shared__ float S[kTxtQ][kTxtMaxT];
    const int tid = threadIdx.x, l = tid & 15, qi = tid >> 4, lane = tid & 63;
    const int q0 = blockIdx.x * kTxtQ, head = blockIdx.y, b = blockIdx.z;
    const int C = a.H * 64;
    const size_t ld = 3 * (size_t)C;
    const float *base = a.qkv + (size_t)b * a.T * ld + head * 64;
    const uint8_t *mb = a.mask ? a.mask + (size_t)b * a.T : nullptr;
    const int t = q0 + qi;                                  // this thread's query
    const bool have = t < a.T;
    const int last = min(q0 + kTxtQ - 1, a.T - 1);          // the last key a query of this tile admits
    const int ntiles = (last >> 6) + 1;
    {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (have) {
            v = ld4(base + (size_t)t * ld + 4 * l);
            v.x = v.x * 0.125f; v.y = v.y * 0.125f; v.z = v.z * 0.125f; v.w = v.w * 0.125f;
        }
        st4(&Qs[qi][4 * l], v);
    }
    // the keys of tile kt that are tokens and not behind `last`: the same 64 bits in every wave
    auto tile_bits = [&](int kt) {
        const int key = kt * 64 + lane;
        return __ballot(key <= last && (mb == nullptr || mb[key] != 0));
    };
    auto stage = [&](int kt, unsigned long long bits, int col0) {      // rows of the others stay zero: never read from memory
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int kk = qi + 16 * i;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if ((bits >> kk) & 1ull) v = ld4(base + (size_t)(kt * 64 + kk) * ld + col0 + 4 * l);
            st4(&KV[kk][4 * l], v);
        }
    };
    float mx = -INFINITY;
    for (int kt = 0; kt < ntiles; ++kt) {
        const unsigned long long bits = tile_bits(kt);
        if (bits == 0ull) continue;                         // no admitted key (work-group uniform)
        __syncthreads();
        stage(kt, bits, C);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int kk = l + 16 * i, key = kt * 64 + kk;
            if (!(have && ((bits >> kk) & 1ull) && key <= t)) continue;
            float s = 0.0f;
#pragma unroll
            for (int d = 0; d < 16; ++d) {
                const float4 q4 = ld4(&Qs[qi][4 * d]), k4 = ld4(&KV[kk][4 * d]);
                s = s + q4.x * k4.x; s = s + q4.y * k4.y; s = s + q4.z * k4.z; s = s + q4.w * k4.w;
            }
            S[qi][key] = s;
            mx = fmaxf(mx, s);
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 8, 16)); mx = fmaxf(mx, __shfl_xor(mx, 4, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 2, 16)); mx = fmaxf(mx, __shfl_xor(mx, 1, 16));
    float sum = 0.0f;
    for (int kt = 0; kt < ntiles; ++kt) {                   // each lane over the scores it wrote itself
        const unsigned long long bits = tile_bits(kt);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int kk = l + 16 * i, key = kt * 64 + kk;
            if (!(have && ((bits >> kk) & 1ull) && key <= t)) continue;
            const float p = expf(S[qi][key] - mx);
            S[qi][key] = p;
            sum = sum + p;
        }
    }
    sum = sum16(sum);
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int kt = 0; kt < ntiles; ++kt) {
        const unsigned long long bits = tile_bits(kt);
        if (bits == 0ull) continue;
        __syncthreads();                                    // the tile before is read, and every p is written
        stage(kt, bits, 2 * C);
        __syncthreads();
        if (!have) continue;
        for (int kk = 0; kk < 64; ++kk) {
            const int key = kt * 64 + kk;
            if (key > t) break;
            if (!((bits >> kk) & 1ull)) continue;
            const float p = S[qi][key];
            const float4 v4 = ld4(&KV[kk][4 * l]);
            o.x = o.x + p * v4.x; o.y = o.y + p * v4.y; o.z = o.z + p * v4.z; o.w = o.w + p * v4.w;
        }
    }
    if (!have) return;
    if (sum == 0.0f) o = make_float4(0.f, 0.f, 0.f, 0.f);   // no admitted key: zeros
    else { o.x = o.x / sum; o.y = o.y / sum; o.z = o.z / sum; o.w = o.w / sum; }
    st4(a.out + ((size_t)b * a.T + t) * C + head * 64 + 4 * l, o);
}

static int txt_rows_ok(const char *who, long n)
{
    PTX_REQUIRE(n >= 1 && n <= (long)kHeadMaxScenes * kTxtMaxT, "%s: n=%ld rows (1 to %ld)", who, n, (long)kHeadMaxScenes * kTxtMaxT);
    return PTX_OK;
}

}  // namespace ptx

using namespace ptx;

extern "C" {

int ptx_txt_embed(const long long *ids, int B, int T, const float *token_embedding, const float *position_embedding, int vocab, int positions,
                  int C, float *out, void *stream)
{
    const char *who = "ptx_txt_embed";
    PTX_REQUIRE(B >= 1 && B <= kHeadMaxScenes && T >= 1 && T <= kTxtMaxT && T <= positions,
                "%s: B=%d T=%d positions=%d (B: 1 to %d; T: 1 to %d and no more than the position table)", who, B, T, positions,
                kHeadMaxScenes, kTxtMaxT);
    PTX_REQUIRE(vocab >= 1 && C >= 64 && C <= kTxtMaxC && C % 64 == 0, "%s: vocab=%d C=%d (vocab >= 1; C: a multiple of 64 up to %d)", who,
                vocab, C, kTxtMaxC);
    PTX_REQUIRE(ids && token_embedding && position_embedding && out, "%s: null argument", who);
    PTX_REQUIRE(sp_aligned16({token_embedding, position_embedding, out}), "%s: the tables and out must be 16-byte aligned", who);
    const TxtEmbedArgs a{ids, token_embedding, position_embedding, out, B * T, T, vocab, C};
    hipLaunchKernelGGL(k_txt_embed, dim3((unsigned)(((long)B * T * (C / 4) + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    PTX_LAUNCHED("k_txt_embed");
    return PTX_OK;
}

int ptx_txt_ln_linear(const float *x, long n, const float *ln_weight, const float *ln_bias, float eps, const float *weight, const float *bias,
                      int Cin, int Cout, int act, float *out, float *stats, void *stream)
{
    const char *who = "ptx_txt_ln_linear";
    PTX_TRY(txt_rows_ok(who, n));
    PTX_REQUIRE(Cin >= 64 && Cin <= kTxtMaxC && Cin % 64 == 0 && Cout >= 64 && Cout <= kTxtMaxI && Cout % 64 == 0,
                "%s: Cin=%d Cout=%d (multiples of 64; Cin up to %d, Cout up to %d)", who, Cin, Cout, kTxtMaxC, kTxtMaxI);
    PTX_REQUIRE((act == 0 || act == 1) && eps > 0.0f, "%s: act=%d eps=%g (act: 0 none, 1 quick-GELU; eps > 0)", who, act, (double)eps);
    PTX_REQUIRE(x && ln_weight && ln_bias && weight && out && stats, "%s: null argument", who);
    PTX_REQUIRE(sp_aligned16({x, ln_weight, ln_bias, weight}), "%s: x, the norm's parameters and weight must be 16-byte aligned", who);
    hipLaunchKernelGGL(k_txt_stats, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, static_cast<hipStream_t>(stream), x, (int)n, Cin, eps, stats);
    PTX_LAUNCHED("k_txt_stats");
    TxtGemmArgs a{};
    a.x = x; a.ln_w = ln_weight; a.ln_b = ln_bias; a.stats = stats; a.w = weight; a.bias = bias; a.out = out; a.n = (int)n; a.Cin = Cin; a.Cout = Cout;
    a.act = act; a.slice_steps = Cin >> 6;
    hipLaunchKernelGGL((k_txt_gemm<true>), dim3(cdiv((int)n, 64), Cout / 64, 1), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    PTX_LAUNCHED("k_txt_gemm<ln>");
    return PTX_OK;
}

int ptx_txt_attention(const float *qkv, const uint8_t *mask, int B, int T, int H, float *out, void *stream)
{
    const char *who = "ptx_txt_attention";
    PTX_REQUIRE(B >= 1 && B <= kHeadMaxScenes && T >= 1 && T <= kTxtMaxT && H >= 1 && H * 64 <= kTxtMaxC,
                "%s: B=%d T=%d H=%d (B: 1 to %d; T: 1 to %d; H heads of 64 up to a width of %d)", who, B, T, H, kHeadMaxScenes, kTxtMaxT, kTxtMaxC);
    PTX_REQUIRE(qkv && out, "%s: null argument", who);
    PTX_REQUIRE(sp_aligned16({qkv, out}), "%s: qkv and out must be 16-byte aligned", who);
    const TxtAttnArgs a{qkv, mask, out, B, T, H};
    hipLaunchKernelGGL(k_txt_attn, dim3(cdiv(T, kTxtQ), H, B), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    PTX_LAUNCHED("k_txt_attn");
    return PTX_OK;
}

size_t ptx_txt_linear_workspace_bytes(long n, int Cin, int Cout)
{
    if (n < 1 || n > (long)kHeadMaxScenes * kTxtMaxT || Cin < 64 || Cin > kTxtMaxI || Cin % 64 || Cout < 64 || Cout > kTxtMaxI || Cout % 64) return 0;
    const int slices = txt_ksplit(Cin);
    return slices > 1 ? (size_t)slices * (size_t)n * Cout * sizeof(float) : 0;
}

int ptx_txt_linear(const float *x, long n, const float *weight, const float *bias, int Cin, int Cout, const float *residual, float *out,
                   void *workspace, size_t ws_bytes, void *stream)
{
    const char *who = "ptx_txt_linear";
    PTX_TRY(txt_rows_ok(who, n));
    PTX_REQUIRE(Cin >= 64 && Cin <= kTxtMaxI && Cin % 64 == 0 && Cout >= 64 && Cout <= kTxtMaxI && Cout % 64 == 0,
                "%s: Cin=%d Cout=%d (multiples of 64 up to %d)", who, Cin, Cout, kTxtMaxI);
    PTX_REQUIRE(x && weight && out, "%s: null argument", who);
    PTX_REQUIRE(x != out, "%s: out must not be x (it may be residual)", who);
    PTX_REQUIRE(sp_aligned16({x, weight, bias, residual, out, workspace}), "%s: the operands must be 16-byte aligned", who);
    const int slices = txt_ksplit(Cin);
    const size_t need = ptx_txt_linear_workspace_bytes(n, Cin, Cout);
    if (need) {
        PTX_REQUIRE(workspace != nullptr, "%s: Cin=%d is cut into %d slices and needs a workspace", who, Cin, slices);
        PTX_TRY(sp_workspace_fits(who, ws_bytes, need));
    }
    TxtGemmArgs a{};
    a.x = x; a.w = weight; a.bias = bias; a.residual = residual; a.out = out; a.n = (int)n; a.Cin = Cin; a.Cout = Cout;
    a.slice_steps = txt_slice_steps(Cin); a.part = slices > 1 ? static_cast<float *>(workspace) : nullptr;
    hipLaunchKernelGGL((k_txt_gemm<false>), dim3(cdiv((int)n, 64), Cout / 64, slices), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    PTX_LAUNCHED("k_txt_gemm<linear>");
    if (slices > 1) {
        hipLaunchKernelGGL(k_txt_slices, dim3((unsigned)((n * (Cout / 4) + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                           a.part, slices, (int)n, Cout, bias, residual, out);
        PTX_LAUNCHED("k_txt_slices");
    }
    return PTX_OK;
}

int ptx_txt_ln(const float *x, long n, int C, const float *weight, const float *bias, float eps, float *out, void *stream)
{
    const char *who = "ptx_txt_ln";
    PTX_TRY(txt_rows_ok(who, n));
    PTX_REQUIRE(C >= 64 && C <= kTxtMaxC && C % 64 == 0 && eps > 0.0f, "%s: C=%d eps=%g (C: a multiple of 64 up to %d; eps > 0)", who, C,
                (double)eps, kTxtMaxC);
    PTX_REQUIRE(x && weight && bias && out, "%s: null argument", who);
    PTX_REQUIRE(sp_aligned16({x, weight, bias, out}), "%s: the operands must be 16-byte aligned", who);
    const TxtLnArgs a{x, weight, bias, out, (int)n, C, eps};
    hipLaunchKernelGGL(k_txt_ln, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    PTX_LAUNCHED("k_txt_ln");
    return PTX_OK;
}

}  // extern "C"
