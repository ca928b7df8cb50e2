// Backward of the sparse convolution and the sparse max-pool (sparse.hip) -- MinkowskiEngine's coordinate manager run backwards.
//
//   ptx_sparse_kernel_map_transpose   nbr_t (n_in, kvol): nbr_t[i, j] = o with nbr[o, j] == i, else -1.  For a fixed (i, j) at most one
//       such o exists (its coordinate is coord_i - offset_j and output rows are distinct): a fill plus one plain store per (o, j).
//   ptx_sparse_conv3d_bwd             with z the convolution before the epilogue and out = relu(((z + bias) * scale + shift) + residual):
//       k_sparse_epi_bwd     gz = g * [out > 0] * scale, dresidual = g * [out > 0], per-256-row column sums of gz (16 rows per thread,
//                            then the 16 row slots in ascending order); k_sparse_colsum adds those tiles the same way -> dbias;
//       dfeats[i] = sum_j gz[nbr_t[i, j]] @ weight[j]^T   k_sparse_conv<WT> of sparse.hip over the transposed map (the weight slab read
//                            with k contiguous); Cin = 3 (the stem): k_sparse_dfeats_stem, one wave per input row;
//       dweight[j] = sum_o feats[nbr[o, j]]^T @ gz[o]     k_sparse_dweight: grid (S row chunks) x (kvol * Cin/64 * Cout/64); a work-group
//                            compacts the present (o, idx) pairs of its offset, 1024 rows at a time, into an LDS list in ascending o and
//                            runs dense 64-pair steps on the exact-fp32 matrix instruction (mfma64.h), both operands written to LDS
//                            transposed (pair index contiguous; stash_t4 of sparse.h); the next step's loads are in
//                            flight behind this step's matrix instructions.  Blocked summation like the forward: a step's product from
//                            zero, then added to the running sum.  S > 1: every work-group writes its 64 x 64 partial into slab
//                            blockIdx.x of the workspace (a chunk without a pair writes zeros: no memset), k_sparse_slab_sum adds the
//                            slabs in ascending order.  Cin = 3: k_sparse_dweight_stem, VALU, 64-row blocks from zero.
//   ptx_sparse_conv_transpose_gen_bwd the same two products for the generative transposed convolution (kernel 2, stride 2: output row
//       8 i + j is child j of input row i), without tables: dfeats[i] = sum_j g[8 i + j] @ kernel[j]^T is the dense (n, 8 Cout) @
//       (8 Cout, Cin) product through k_sparse_conv<WT>, dkernel[j] = feats^T @ g[j::8] through k_sparse_dweight with its slabs; both
//       kernels form the map from the row index where the table pointer is null.
//   ptx_sparse_max_pool3d_bwd         routes each gradient to the offset ptx_sparse_max_pool3d_arg (sparse.hip) recorded.
//
// No float atomics anywhere: every output is bitwise reproducible.  Everything runs on the caller's stream; no host wait.
#include "sparse.h"

namespace ptx {

constexpr int kDwSub = 1024;               // rows compacted into LDS at a time

// ---- transposed kernel map ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sparse_map_transpose(const int32_t *__restrict__ nbr, long total, int kvol, int n_in,
                                                              int32_t *__restrict__ nbr_t)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int i = nbr[t];
    if (i < 0 || i >= n_in) return;
    const int o = (int)(t / kvol), j = (int)(t - (long)o * kvol);
    nbr_t[(size_t)i * kvol + j] = o;
}

// ---- epilogue backward ----------------------------------------------------------------------------------------------------
// grid (cdiv(n_out, kSpTile), Cout / 64), the streaming idiom of sparse.h; gz / dres / part each optional
__global__ __launch_bounds__(256) void k_sparse_epi_bwd(const float *__restrict__ g, const float *__restrict__ out,
                                                        const float *__restrict__ scale, float *__restrict__ gz, float *__restrict__ dres,
                                                        float *__restrict__ part, int n_out, int Cout)
{
    __shared__ __attribute__((aligned(16))) float s_sum[16][64];
    const int tid = threadIdx.x, c4 = tid & 15, slot = tid >> 4;
    const int col = blockIdx.y * 64 + c4 * 4;
    float4 sc = make_float4(1.f, 1.f, 1.f, 1.f);
    if (scale) sc = *reinterpret_cast<const float4 *>(scale + col);
    float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
    for (int i = 0; i < kSpTile / 16; ++i) {
        const int row = blockIdx.x * kSpTile + slot + 16 * i;
        if (row >= n_out) break;
        const size_t at = (size_t)row * Cout + col;
        float4 d = ld4(g + at);
        if (out) relu_mask4(d, ld4(out + at));
        if (dres) st4(dres + at, d);
        float4 z = d;
        if (scale) scale4(z, sc);
        if (gz) st4(gz + at, z);
        sum = add4(sum, z);
    }
    if (part == nullptr) return;
    st4(&s_sum[slot][c4 * 4], sum);
    __syncthreads();
    if (tid < 64) part[(size_t)blockIdx.x * Cout + blockIdx.y * 64 + tid] = slots16(s_sum, tid);
}

// dst (C) = the column sums of part (T, C): 16 row slots stride over the tiles, then the slots in ascending order.  grid C / 64
__global__ __launch_bounds__(256) void k_sparse_colsum(const float *__restrict__ part, int T, int C, float *__restrict__ dst)
{
    __shared__ __attribute__((aligned(16))) float s_sum[16][64];
    const int tid = threadIdx.x, c4 = tid & 15, slot = tid >> 4;
    const int col = blockIdx.x * 64 + c4 * 4;
    float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t = slot; t < T; t += 16) acc4(sum, ld4(part + (size_t)t * C + col));
    st4(&s_sum[slot][c4 * 4], sum);
    __syncthreads();
    if (tid < 64) dst[blockIdx.x * 64 + tid] = slots16(s_sum, tid);
}

// ---- dweight ----------------------------------------------------------------------------------------------------------------
struct SpDwArgs {
    const float *feats, *gz; const int32_t *nbr; float *dst;
    int n_in, n_out, kvol, Cin, Cout, R;   // R: rows per chunk (blockIdx.x)
    size_t slab;                           // floats between the chunks' partials (0: one chunk, dst is dweight itself)
};

__global__ __launch_bounds__(256) void k_sparse_dweight(SpDwArgs a)
{
    __shared__ __attribute__((aligned(16))) float As[2][64][LDT];       // [pair / 32][input channel][pair % 32]
    __shared__ __attribute__((aligned(16))) float Ws[2][64][LDT];       // [pair / 32][output channel][pair % 32]
    __shared__ int32_t s_o[kDwSub], s_i[kDwSub];                        // the present pairs of this offset, ascending o
    __shared__ int s_wcnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1, li = lane & 31, hh = lane >> 5;
    const int nct = a.Cout >> 6, mct = a.Cin >> 6;
    const int tile = blockIdx.y;
    const int cout0 = (tile % nct) << 6, cin0 = ((tile / nct) % mct) << 6, j = tile / (nct * mct);
    const int r0 = blockIdx.x * a.R, r1 = min(r0 + a.R, a.n_out);
    // staging: thread (pair = wk + 16 i, channels wn .. wn + 3) of both operands, written transposed (stash_t4)
    const int wk = lane & 15, wn = (wid * 4 + (lane >> 4)) * 4;
    float4 av[4], wv[4];
    float tot[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) tot[i] = 0.0f;

    for (int sub = r0; sub < r1; sub += kDwSub) {
        int cnt = 0;                                        // work-group uniform
        for (int pass = 0; pass < kDwSub / 256 && sub + pass * 256 < r1; ++pass) {
            const int o = sub + pass * 256 + tid;
            int idx = -1;
            if (o < r1) idx = a.nbr ? a.nbr[(size_t)o * a.kvol + j] : ((o & 7) == j ? o >> 3 : -1);      // no table: the generative map
            if (idx >= a.n_in) idx = -1;                    // (never from ptx_sparse_kernel_map)
            const unsigned long long vote = __ballot(idx >= 0);
            if (lane == 0) s_wcnt[wid] = __popcll(vote);
            __syncthreads();
            int base = cnt, all = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const int c = s_wcnt[w];
                if (w < wid) base += c;
                all += c;
            }
            if (idx >= 0) {
                const int pos = base + __popcll(vote & ((1ull << lane) - 1ull));
                s_o[pos] = o;
                s_i[pos] = idx;
            }
            cnt += all;
            __syncthreads();
        }
        const int nsteps = (cnt + 63) >> 6;

        auto fetch = [&](int s) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int p = s * 64 + wk + 16 * i;
                av[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                wv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (p < cnt) {
                    av[i] = ld4(a.feats + (size_t)s_i[p] * a.Cin + cin0 + wn);
                    wv[i] = ld4(a.gz + (size_t)s_o[p] * a.Cout + cout0 + wn);
                }
            }
        };
        auto stash = [&]() {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                stash_t4(As, wk + 16 * i, wn, av[i]);
                stash_t4(Ws, wk + 16 * i, wn, wv[i]);
            }
        };

        if (nsteps > 0) fetch(0);
        for (int s = 0; s < nsteps; ++s) {
            stash();
            __syncthreads();
            if (s + 1 < nsteps) fetch(s + 1);               // in flight behind this step's matrix instructions
            PTX_SPARSE_STEP(tot, cnt - s * 64 > 32);
            __syncthreads();
        }
    }
    // C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
    float *dst = a.dst + (size_t)blockIdx.x * a.slab + ((size_t)j * a.Cin + cin0) * a.Cout + cout0 + wc * 32 + li;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
        dst[(size_t)row * a.Cout] = tot[r];
    }
}

// the stem, Cin = 3: dweight (27, 3, Cout).  grid (S, kvol, Cout / 64); wave w takes the w-th quarter of the chunk's rows, lane = output
// channel; 64 rows at a time: their neighbour and its 3 features are loaded by the 64 lanes and broadcast, the block's products are
// summed from zero in ascending o and added to the running sum; the four waves are combined in ascending order.
__global__ __launch_bounds__(256) void k_sparse_dweight_stem(SpDwArgs a)
{
    __shared__ float s_sum[4][3][64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int j = blockIdx.y, n = blockIdx.z * 64 + lane;
    const int r0 = blockIdx.x * a.R, r1 = min(r0 + a.R, a.n_out);
    const int q = (a.R + 3) >> 2;
    const int my0 = min(r0 + wid * q, r1), my1 = min(my0 + q, r1);
    float tot[3] = {0.0f, 0.0f, 0.0f};
    for (int o0 = my0; o0 < my1; o0 += 64) {
        const int o = o0 + lane;
        int idx = o < my1 ? a.nbr[(size_t)o * a.kvol + j] : -1;
        if (idx >= a.n_in) idx = -1;
        float f[3] = {0.0f, 0.0f, 0.0f};
        if (idx >= 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) f[c] = a.feats[(size_t)idx * 3 + c];
        }
        unsigned long long vote = __ballot(idx >= 0);
        float acc[3] = {0.0f, 0.0f, 0.0f};
        while (vote != 0ull) {
            const int t = __ffsll((long long)vote) - 1;
            vote &= vote - 1ull;
            const float gv = a.gz[(size_t)(o0 + t) * a.Cout + n];
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = fmaf(__shfl(f[c], t), gv, acc[c]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) tot[c] += acc[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) s_sum[wid][c][lane] = tot[c];
    __syncthreads();
    if (wid == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = ((s_sum[0][c][lane] + s_sum[1][c][lane]) + s_sum[2][c][lane]) + s_sum[3][c][lane];
            a.dst[(size_t)blockIdx.x * a.slab + ((size_t)j * 3 + c) * a.Cout + n] = v;
        }
    }
}

// dst (L) = slab 0 + slab 1 + ... + slab S-1, in that order; one thread per 4 floats
__global__ __launch_bounds__(256) void k_sparse_slab_sum(const float *__restrict__ ws, int S, size_t L, float *__restrict__ dst)
{
    const size_t e = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (e >= L) return;
    float4 v = ld4(ws + e);
    for (int s = 1; s < S; ++s) acc4(v, ld4(ws + (size_t)s * L + e));
    st4(dst + e, v);
}

// the stem's dfeats (n_in, 3): one wave per input row; the row's kvol transposed neighbours are loaded by the lanes, the present ones
// visited in ascending j; lane = output channel (+ 64, ...); a fixed-order lane reduction (wave_sum) closes each of the 3 sums
__global__ __launch_bounds__(256) void k_sparse_dfeats_stem(const float *__restrict__ gz, const int32_t *__restrict__ nbr_t,
                                                            const float *__restrict__ weight, float *__restrict__ dfeats, int n_in,
                                                            int n_out, int kvol, int Cout)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wid;
    if (i >= n_in) return;                                  // (the whole wave)
    int o = lane < kvol ? nbr_t[(size_t)i * kvol + lane] : -1;
    if (o >= n_out) o = -1;
    unsigned long long vote = __ballot(o >= 0);
    float acc[3] = {0.0f, 0.0f, 0.0f};
    while (vote != 0ull) {
        const int j = __ffsll((long long)vote) - 1;
        vote &= vote - 1ull;
        const int oj = __shfl(o, j);
        for (int n = lane; n < Cout; n += 64) {
            const float gv = gz[(size_t)oj * Cout + n];
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = fmaf(gv, weight[((size_t)j * 3 + c) * Cout + n], acc[c]);
        }
    }
    const float d0 = wave_sum(acc[0]), d1 = wave_sum(acc[1]), d2 = wave_sum(acc[2]);
    if (lane == 0) {
        dfeats[(size_t)i * 3 + 0] = d0;
        dfeats[(size_t)i * 3 + 1] = d1;
        dfeats[(size_t)i * 3 + 2] = d2;
    }
}

// ---- max-pool ---------------------------------------------------------------------------------------------------------------
// one thread per (input row, 4 channels): dfeats[i, c] = sum over ascending j of [arg[nbr_t[i, j], c] == j] * g[nbr_t[i, j], c]
__global__ __launch_bounds__(256) void k_sparse_max_pool_bwd(const float *__restrict__ g, const uint8_t *__restrict__ arg,
                                                             const int32_t *__restrict__ nbr_t, int n_in, int n_out, int kvol, int C,
                                                             float *__restrict__ dfeats)
{
    const int c4n = C >> 2;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const int i = (int)(t / c4n), c4 = (int)(t - (long)i * c4n);
    if (i >= n_in) return;
    float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = 0; j < kvol; ++j) {
        const int o = nbr_t[(size_t)i * kvol + j];
        if (o < 0 || o >= n_out) continue;
        const uchar4 w = *reinterpret_cast<const uchar4 *>(arg + (size_t)o * C + c4 * 4);
        const float4 x = *reinterpret_cast<const float4 *>(g + (size_t)o * C + c4 * 4);       // (through ld4 the loop is laid out differently)
        if (w.x == j) d.x += x.x;
        if (w.y == j) d.y += x.y;
        if (w.z == j) d.z += x.z;
        if (w.w == j) d.w += x.w;
    }
    st4(dfeats + (size_t)i * C + c4 * 4, d);
}

// ---- the split of dweight over the rows: a function of the shapes only ------------------------------------------------------
struct DwPlan { int R, S; size_t slab, dw_bytes, part_bytes, total; };
static bool bwd_widths_ok(int kvol, int Cin, int Cout)
{
    const bool stem = Cin == 3 && kvol == 27;
    return (kvol == 1 || kvol == 8 || kvol == 27) && sp_width_ok(Cout) && (stem || (Cin >= 64 && Cin <= kSpMaxCin && Cin % 64 == 0));
}
static DwPlan dw_plan(int n_out, int kvol, int Cin, int Cout)
{
    DwPlan P{};
    const bool stem = Cin == 3;
    const long tiles = stem ? (long)kvol * (Cout / 64) : (long)kvol * (Cin / 64) * (Cout / 64);
    P.slab = (size_t)kvol * Cin * Cout;
    // enough work-groups to cover the 256 CUs about four times over, a workspace of at most 256 MiB, chunks of at least 256 rows (the
    // stem: 1024, 256 per wave) in multiples of 64
    long target = (1024 + tiles - 1) / tiles;
    const long cap = (long)((size_t(256) << 20) / (P.slab * sizeof(float)));
    target = target > cap ? cap : target;
    target = target < 1 ? 1 : target;
    const int least = stem ? 1024 : 256;
    long R = ((long)n_out + target - 1) / target;
    R = (R + 63) / 64 * 64;
    P.R = (int)(R < least ? least : R);
    P.S = cdiv(n_out, P.R);
    P.dw_bytes = P.S > 1 ? align_up((size_t)P.S * P.slab * sizeof(float), 256) : 0;
    P.part_bytes = align_up((size_t)cdiv(n_out > 0 ? n_out : 1, kSpTile) * Cout * sizeof(float), 256);
    P.total = P.dw_bytes + P.part_bytes + 256;
    return P;
}

}  // namespace ptx

using namespace ptx;

extern "C" {

int ptx_sparse_kernel_map_transpose(const int32_t *nbr, int n_out, int kvol, int n_in, int32_t *nbr_t, void *stream)
{
    PTX_REQUIRE(n_out >= 0 && n_in >= 0 && kvol >= 1 && kvol <= kSpMaxVol && (long)n_out * kvol < (1l << 31) && (long)n_in * kvol < (1l << 31),
                "ptx_sparse_kernel_map_transpose: n_out=%d kvol=%d n_in=%d (kvol: 1 to 27; rows x kvol below 2^31)", n_out, kvol, n_in);
    if (n_in == 0) return PTX_OK;
    PTX_REQUIRE(nbr_t && (nbr || n_out == 0), "ptx_sparse_kernel_map_transpose: null argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    PTX_HIP(hipMemsetAsync(nbr_t, 0xff, (size_t)n_in * kvol * sizeof(int32_t), st));       // -1
    const long total = (long)n_out * kvol;
    if (total == 0) return PTX_OK;
    hipLaunchKernelGGL(k_sparse_map_transpose, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, nbr, total, kvol, n_in, nbr_t);
    PTX_LAUNCHED("k_sparse_map_transpose");
    return PTX_OK;
}

size_t ptx_sparse_conv3d_bwd_workspace_bytes(int n_out, int kvol, int Cin, int Cout)
{
    if (n_out < 0 || !bwd_widths_ok(kvol, Cin, Cout)) return 0;
    return dw_plan(n_out, kvol, Cin, Cout).total;
}

// ptx_sparse_conv3d_bwd and, with `gen` (no tables: output row o = 8 i + j is child j of input row i, kvol = 8, no epilogue),
// ptx_sparse_conv_transpose_gen_bwd; `who` names the one that was called in its messages
static int conv_bwd(const char *who, bool gen, const float *g, const float *out, const float *scale, int relu, const float *feats, int n_in,
                    const int32_t *nbr, const int32_t *nbr_t, int n_out, int kvol, const float *weight, int Cin, int Cout, float *gz,
                    float *dresidual, float *dbias, float *dfeats, float *dweight, void *workspace, size_t ws_bytes, void *stream)
{
    PTX_REQUIRE(n_in >= 0 && n_out >= 0 && bwd_widths_ok(kvol, Cin, Cout),
                "%s: n_in=%d n_out=%d Cin=%d Cout=%d kvol=%d (kvol: 1, 8 or 27; Cin: 3 with 27 offsets, or a multiple of 64 "
                "up to %d; Cout: a multiple of 64 up to 512)", who, n_in, n_out, Cin, Cout, kvol, kSpMaxCin);
    PTX_REQUIRE((long)n_out * kvol < (1l << 31) && (long)n_in * kvol < (1l << 31), "%s: %d / %d rows x %d offsets is out of range", who, n_out,
                n_in, kvol);
    const bool stem = Cin == 3, epi = relu != 0 || scale != nullptr;
    const bool need_z = dfeats != nullptr || dweight != nullptr;       // the GEMMs read gz
    PTX_REQUIRE(g || n_out == 0, "%s: g is null", who);
    PTX_REQUIRE(!relu || out || n_out == 0, "%s: relu needs the forward's out", who);
    PTX_REQUIRE(!(epi && need_z) || gz || n_out == 0, "%s: gz is needed with relu / scale when dfeats or dweight is asked for", who);
    PTX_REQUIRE(!dfeats || (((nbr_t || gen) && weight) || n_out == 0 || n_in == 0), "%s: dfeats needs nbr_t and weight", who);
    PTX_REQUIRE(!dweight || (((nbr || gen) && feats) || n_out == 0 || n_in == 0), "%s: dweight needs nbr and feats", who);
    PTX_REQUIRE(sp_aligned16({g, out, scale, feats, weight, gz, dresidual, dfeats, dweight, workspace}),
                "%s: every float buffer and the workspace must be 16-byte aligned", who);
    const DwPlan P = dw_plan(n_out, kvol, Cin, Cout);
    const bool use_ws = dbias != nullptr || (dweight != nullptr && P.S > 1);
    if (use_ws && n_out > 0) {
        PTX_REQUIRE(workspace, "%s: workspace is null", who);
        PTX_TRY(sp_workspace_fits(who, ws_bytes, P.total));
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_out == 0 || n_in == 0) {                          // no pair anywhere
        if (dfeats && n_in > 0) PTX_HIP(hipMemsetAsync(dfeats, 0, (size_t)n_in * Cin * sizeof(float), st));
        if (dweight) PTX_HIP(hipMemsetAsync(dweight, 0, P.slab * sizeof(float), st));
        if (n_out == 0) {
            if (dbias) PTX_HIP(hipMemsetAsync(dbias, 0, (size_t)Cout * sizeof(float), st));
            return PTX_OK;
        }
    }
    char *ws = static_cast<char *>(workspace);
    float *part = dbias ? reinterpret_cast<float *>(ws + P.dw_bytes) : nullptr;
    const int T = cdiv(n_out, kSpTile);
    if ((epi && gz) || dbias || dresidual) {
        hipLaunchKernelGGL(k_sparse_epi_bwd, dim3(T, Cout / 64), dim3(256), 0, st, g, relu ? out : nullptr, scale, epi ? gz : nullptr, dresidual,
                           part, n_out, Cout);
        PTX_LAUNCHED("k_sparse_epi_bwd");
        if (dbias) {
            hipLaunchKernelGGL(k_sparse_colsum, dim3(Cout / 64), dim3(256), 0, st, part, T, Cout, dbias);
            PTX_LAUNCHED("k_sparse_colsum");
        }
    }
    if (n_in == 0) return PTX_OK;
    const float *z = epi ? gz : g;
    if (dfeats) {
        if (stem) {
            hipLaunchKernelGGL(k_sparse_dfeats_stem, dim3(cdiv(n_in, 4)), dim3(256), 0, st, z, nbr_t, weight, dfeats, n_in, n_out, kvol, Cout);
            PTX_LAUNCHED("k_sparse_dfeats_stem");
        } else {
            PTX_TRY(sparse_conv_transposed(z, n_out, nbr_t, n_in, kvol, weight, Cin, Cout, dfeats, st));
        }
    }
    if (dweight) {
        float *dst = P.S > 1 ? reinterpret_cast<float *>(ws) : dweight;
        const SpDwArgs a{feats, z, nbr, dst, n_in, n_out, kvol, Cin, Cout, P.R, P.S > 1 ? P.slab : 0};
        if (stem) {
            hipLaunchKernelGGL(k_sparse_dweight_stem, dim3(P.S, kvol, Cout / 64), dim3(256), 0, st, a);
            PTX_LAUNCHED("k_sparse_dweight_stem");
        } else {
            hipLaunchKernelGGL(k_sparse_dweight, dim3(P.S, kvol * (Cin / 64) * (Cout / 64)), dim3(256), 0, st, a);
            PTX_LAUNCHED("k_sparse_dweight");
        }
        if (P.S > 1) {
            hipLaunchKernelGGL(k_sparse_slab_sum, dim3((unsigned)((P.slab / 4 + 255) / 256)), dim3(256), 0, st, dst, P.S, P.slab, dweight);
            PTX_LAUNCHED("k_sparse_slab_sum");
        }
    }
    return PTX_OK;
}

int ptx_sparse_conv3d_bwd(const float *g, const float *out, const float *scale, int relu, const float *feats, int n_in, const int32_t *nbr,
                          const int32_t *nbr_t, int n_out, int kvol, const float *weight, int Cin, int Cout, float *gz, float *dresidual,
                          float *dbias, float *dfeats, float *dweight, void *workspace, size_t ws_bytes, void *stream)
{
    return conv_bwd("ptx_sparse_conv3d_bwd", false, g, out, scale, relu, feats, n_in, nbr, nbr_t, n_out, kvol, weight, Cin, Cout, gz, dresidual,
                    dbias, dfeats, dweight, workspace, ws_bytes, stream);
}

// the generative transposed convolution's rows: n parents, 8 n children; 8 n x 8 offsets must stay below 2^31
static bool gen_rows_ok(int n) { return n >= 0 && n <= (1 << 24); }

size_t ptx_sparse_conv_transpose_gen_bwd_workspace_bytes(int n, int Cin, int Cout)
{
    if (!gen_rows_ok(n) || Cin == 3 || !bwd_widths_ok(8, Cin, Cout)) return 0;
    return dw_plan(8 * n, 8, Cin, Cout).total;
}

int ptx_sparse_conv_transpose_gen_bwd(const float *g, const float *feats, int n, const float *weight, int Cin, int Cout, float *dfeats,
                                      float *dweight, void *workspace, size_t ws_bytes, void *stream)
{
    PTX_REQUIRE(gen_rows_ok(n) && Cin != 3, "ptx_sparse_conv_transpose_gen_bwd: n=%d Cin=%d (at most 2^24 rows; Cin: a multiple of 64 up to %d)", n,
                Cin, kSpMaxCin);
    return conv_bwd("ptx_sparse_conv_transpose_gen_bwd", true, g, nullptr, nullptr, 0, feats, n, nullptr, nullptr, 8 * n, 8, weight, Cin, Cout,
                    nullptr, nullptr, nullptr, dfeats, dweight, workspace, ws_bytes, stream);
}

int ptx_sparse_max_pool3d_bwd(const float *g, const uint8_t *arg, const int32_t *nbr_t, int n_in, int n_out, int kvol, int C, float *dfeats,
                              void *stream)
{
    PTX_REQUIRE(n_in >= 0 && n_out >= 0 && kvol >= 1 && kvol <= kSpMaxVol && C >= 4 && C % 4 == 0,
                "ptx_sparse_max_pool3d_bwd: n_in=%d n_out=%d kvol=%d C=%d (C: a multiple of 4)", n_in, n_out, kvol, C);
    if (n_in == 0) return PTX_OK;
    PTX_REQUIRE(nbr_t && dfeats && ((g && arg) || n_out == 0), "ptx_sparse_max_pool3d_bwd: null argument");
    PTX_REQUIRE(sp_aligned16({g, dfeats}) && (reinterpret_cast<uintptr_t>(arg) & 3) == 0,
                "ptx_sparse_max_pool3d_bwd: g and dfeats must be 16-byte aligned, arg 4-byte aligned");
    PTX_TRY(sp_rows_fit("ptx_sparse_max_pool3d_bwd", n_in, C));
    const long threads = (long)n_in * (C / 4);
    hipLaunchKernelGGL(k_sparse_max_pool_bwd, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), g, arg,
                       nbr_t, n_in, n_out, kvol, C, dfeats);
    PTX_LAUNCHED("k_sparse_max_pool_bwd");
    return PTX_OK;
}

}  // extern "C"
