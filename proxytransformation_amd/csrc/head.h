// What query_select.hip, decoder.hip, neck.hip and text_encoder.hip share: the limits of the stages behind the neck, the main loop of the 64 x 64 NT tile
// on the exact-fp32 matrix instruction with its C/D row formula and the two epilogues, the 16-lane row reduction with the 9-value box
// head, and the radix threshold search of the two top-k kernels.  Orders of addition are part of each piece: the callers' bits depend
// on them.
#pragma once
#include "sparse.h"
#include "train_rules.h"

namespace ptx {

constexpr int kHeadMaxScenes = 64, kHeadMaxK = 1024, kHeadMaxText = 256, kHeadReg = 9;

// ---- the 64 x 64 NT tile --------------------------------------------------------------------------------------------------------
// C/D layout of the 32x32 MFMA: col = lane & 31; accumulator r of wave row wr, lane half hh is this row of the tile
__device__ __forceinline__ int tile_row(int r, int wr, int hh) { return wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh; }

// a thread's place in the tile's 4-wave work-group: wave (wr, wc) owns a 32 x 32 accumulator, li = lane & 31 its column, hh = lane >> 5
struct Tile64 {
    int tid, wr, wc, li, hh;
    __device__ __forceinline__ Tile64() : tid(threadIdx.x), wr(tid >> 7), wc((tid >> 6) & 1), li(tid & 31), hh((tid >> 5) & 1) {}
    __device__ __forceinline__ int row(int r) const { return tile_row(r, wr, hh); }       // tile row of accumulator r
    __device__ __forceinline__ int col() const { return wc * 32 + li; }                   // tile column of the accumulator
};

// out tile (64 x 64) = A (64 x 64 nsteps) @ W^T, both operands with k contiguous, by a 4-wave work-group: wave (wr, wc) owns the 32 x 32
// accumulator `tot` (rows t.row(r), column t.col()).  Staging: thread (ar + 16 i, kq .. kq + 3), 16 lanes = one 256-B row piece; the
// next step's quads are in flight in registers behind this step's matrix instructions.  p = at(s) says where step s reads (formed once
// per step: a division in it is not repeated per quad); a_quad(v, p, row, kq) / w_quad(v, p, row, kq) write to v a thread's four values
// of tile row / tile column `row` at k offset kq of that step (zeros outside the operand); done(s) runs after step s behind the second
// barrier.  BLOCKED: each 64-wide step is summed from zero and then added to `tot` (k_sparse_conv's order, the query selection's);
// otherwise the steps accumulate straight through (the decoder's).  Both orders are recorded behaviour.
template <bool BLOCKED, class At, class AQuad, class WQuad, class Done>
__device__ __forceinline__ void tile64_nt(const Tile64 &t, int nsteps, f32x16 &tot, At at, AQuad a_quad, WQuad w_quad, Done done)
{
    __shared__ __attribute__((aligned(16))) float As[2][64][LDT];
    __shared__ __attribute__((aligned(16))) float Ws[2][64][LDT];
    const int wr = t.wr, wc = t.wc, li = t.li, hh = t.hh;
    const int ar = t.tid >> 4, kq = (t.tid & 15) * 4;
    float4 av[4], wv[4];
    auto fetch = [&](int s) {
        const auto p = at(s);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            a_quad(av[i], p, ar + 16 * i, kq);
            w_quad(wv[i], p, ar + 16 * i, kq);
        }
    };
    fetch(0);
    for (int s = 0; s < nsteps; ++s) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            st4(&As[kq >> 5][ar + 16 * i][kq & 31], av[i]);
            st4(&Ws[kq >> 5][ar + 16 * i][kq & 31], wv[i]);
        }
        __syncthreads();
        if (s + 1 < nsteps) fetch(s + 1);                   // in flight behind this step's matrix instructions
        if (BLOCKED) {
            f32x16 acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
            g64_step(As, Ws, 0, wr * 32 + li, wc * 32 + li, hh, acc);
            g64_step(As, Ws, 1, wr * 32 + li, wc * 32 + li, hh, acc);
#pragma unroll
            for (int i = 0; i < 16; ++i) tot[i] += acc[i];
        } else {
            g64_step(As, Ws, 0, wr * 32 + li, wc * 32 + li, hh, tot);
            g64_step(As, Ws, 1, wr * 32 + li, wc * 32 + li, hh, tot);
        }
        __syncthreads();
        done(s);
    }
}

// The epilogue of a Linear: out[row, n] = act(tot + bias[n]) (+ residual[row, n]) on the rows below nrows; the ReLU keeps a NaN.
__device__ __forceinline__ void linear_store(const Tile64 &t, const f32x16 &tot, int row0, int nrows, int n, int ld, const float *bias,
                                             int relu, const float *residual, float *out)
{
    const float b = bias ? bias[n] : 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = row0 + t.row(r);
        if (row >= nrows) continue;
        float v = tot[r];
        if (bias) v = v + b;
        if (relu) v = relu_nan(v);
        if (residual) v = v + residual[(size_t)row * ld + n];
        out[(size_t)row * ld + n] = v;
    }
}

// ContrastiveEmbed's value of a product (grounding_head.py:62-99): / sqrt(C) when scaled, + bias, -inf under the mask
// (the caller loads bias[0] once: behind a store the compiler would load it again)
__device__ __forceinline__ float contrastive_value(float v, bool valid, int scaled, float divisor, bool has_bias, float bias)
{
    if (scaled) v = v / divisor;
    if (has_bias) v = v + bias;
    return valid ? v : -INFINITY;
}

// ---- 16 lanes per row -----------------------------------------------------------------------------------------------------------
// Lane l of a row's 16 holds channels 64 m + 4 l .. + 3 as x[m] (one 256-B piece of the row per 16 lanes and m).  The 16 partial sums are
// added by xor 8, 4, 2, 1: every lane ends with the same total.
__device__ __forceinline__ float sum16(float s)
{
    s = s + __shfl_xor(s, 8, 16); s = s + __shfl_xor(s, 4, 16); s = s + __shfl_xor(s, 2, 16); s = s + __shfl_xor(s, 1, 16);
    return s;
}

// x . w over the C = 64 nm channels: the lane's products in ascending channel order, then sum16
__device__ __forceinline__ float row_dot16(const float4 (&x)[8], int nm, const float *w, int l)
{
    float s = 0.0f;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        if (m < nm) {
            const float4 w4 = ld4(w + 64 * m + 4 * l);
            s = s + x[m].x * w4.x; s = s + x[m].y * w4.y; s = s + x[m].z * w4.z; s = s + x[m].w * w4.w;
        }
    }
    return sum16(s);
}

// The last Linear (C -> 9) of a regression branch and the baseline box decode: work-group = 16 rows x 16 lanes, lane l < 9 finishes box
// value l -- center = p + coords, size = max(expf(p), 0.02) with a NaN kept, euler = p.  GATHER (ptx_qs_decode): row (b, q) reads
// feats / coords at b * Lmax + index[b, q]; the same 16 lanes copy them to query / qcoords, and h may be null (the gathered features
// themselves).  Otherwise (ptx_dec_boxes) the rows are h's and coords' own.
struct HeadBoxArgs {
    const float *h, *weight, *bias;                         // (n,C) [GATHER: or null], (9,C), (9) or null
    const float *feats, *coords; const long long *index;    // GATHER: (B,Lmax,C), (B,Lmax,3), (B,K); else coords (n,3) alone
    float *query, *qcoords, *boxes;                         // GATHER: (n,C), (n,3); (n,9)
    int n, K, Lmax, C;
};

template <bool GATHER>
__global__ __launch_bounds__(256) void k_head_boxes(HeadBoxArgs a)
{
    __shared__ __attribute__((aligned(16))) float s_w[kHeadReg * 512];
    for (int e = threadIdx.x; e < kHeadReg * a.C; e += 256) s_w[e] = a.weight[e];
    __syncthreads();
    const int l = threadIdx.x & 15;
    const long row = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int nm = a.C >> 6;
    long src = -1;                                          // the row of coords (and feats), -1: none
    if (row < a.n) {
        src = row;
        if (GATHER) {
            const long long i = a.index[row];
            src = (i >= 0 && i < a.Lmax) ? (row / a.K) * a.Lmax + i : -1;
        }
    }
    float4 x[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        x[m] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (m < nm && src >= 0) {
            if (GATHER) {
                const float4 f = ld4(a.feats + (size_t)src * a.C + 64 * m + 4 * l);
                st4(a.query + (size_t)row * a.C + 64 * m + 4 * l, f);
                x[m] = a.h ? ld4(a.h + (size_t)row * a.C + 64 * m + 4 * l) : f;
            } else {
                x[m] = ld4(a.h + (size_t)row * a.C + 64 * m + 4 * l);
            }
        }
    }
    float mine = 0.0f;
#pragma unroll
    for (int k = 0; k < kHeadReg; ++k) {
        float s = row_dot16(x, nm, &s_w[k * a.C], l);
        if (a.bias) s = s + a.bias[k];
        if (k == l) mine = s;
    }
    if (src < 0 || l >= kHeadReg) return;
    if (l < 3) {
        const float c = a.coords[(size_t)src * 3 + l];
        if (GATHER) a.qcoords[(size_t)row * 3 + l] = c;
        mine = mine + c;
    } else if (l < 6) {
        mine = max_nan(expf(mine), 0.02f);
    }
    a.boxes[(size_t)row * kHeadReg + l] = mine;
}

// ---- top-k ------------------------------------------------------------------------------------------------------------------------
// the order of the scores as unsigned integers: larger score, larger key; -0.0 and +0.0 share one.  A NaN orders by its bits: above +inf
// with the sign bit clear, below -inf with it set (neck_host.topk_key restates it)
__device__ __forceinline__ uint32_t topk_key(float s)
{
    uint32_t u = __float_as_uint(s);
    if ((u << 1) == 0u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// LDS of topk_threshold; w is free for the caller's own scans once it has returned (behind a barrier)
struct TopkLds { int hist[256]; int w[4]; uint32_t prefix; int need; };

// The k-th largest key among sc[lo .. hi) (hi - lo >= k >= 1), by all 256 threads of the work-group: a radix select, 4 passes of 8
// bits over LDS histograms of integer counts.  Thread d owns digit d of a pass and takes the count of the larger digits from a suffix
// scan (shuffles inside a wave, the four wave totals through LDS); exactly one digit holds the k-th key.  Returns the key; `need` (>= 1)
// of the rows that carry it belong to the k, everything above it does.
__device__ __forceinline__ uint32_t topk_threshold(const float *sc, int lo, int hi, int k, TopkLds &s, int &need)
{
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    uint32_t prefix = 0u, known = 0u;                       // the threshold key's bits found so far
    need = k;                                               // rows still to take among those that match `prefix`
    for (int shift = 24; shift >= 0; shift -= 8) {
        s.hist[tid] = 0;
        __syncthreads();
        for (int i = lo + tid; i < hi; i += 256) {
            const uint32_t key = topk_key(sc[i]);
            if ((key & known) == prefix) atomicAdd(&s.hist[(key >> shift) & 255u], 1);
        }
        __syncthreads();
        const int h = s.hist[tid];
        int suf = h;                                        // candidates with a digit >= tid inside this wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_down(suf, d, 64);
            if (lane + d < 64) suf += o;
        }
        if (lane == 0) s.w[wid] = suf;
        __syncthreads();
        int above = suf - h;                                // candidates with a larger digit
        for (int w = wid + 1; w < 4; ++w) above += s.w[w];
        if (above < need && need <= above + h) {            // exactly one digit: the candidates are at least `need`
            s.prefix = prefix | ((uint32_t)tid << shift);
            s.need = need - above;
        }
        __syncthreads();
        prefix = s.prefix; need = s.need; known |= 255u << shift;
    }
    return prefix;
}

}  // namespace ptx
