// Sparse 3D convolution on the voxel rows -- the primitive of `x = self.backbone_3d(x)` (detectors/
// sparse_featfusion_grounder_preshape.py:398; backbones/mink_resnet.py:57-78: MinkowskiConvolution / MinkowskiMaxPooling of a
// MinkResNet).  MinkowskiEngine's part that torch has no substitute for is the coordinate manager: "which input row lies at
// offset d from this output row".  Two pieces:
//
//   ptx_sparse_kernel_map   the neighbour table nbr (n_out, k^3) of a (kernel_size, stride) pair over the rows of a level:
//       stride 2: the output rows are the coarser level's, emitted by ptx_voxel_coarsen itself (voxel.hip: the distinct
//                 floor(c / 2ts) * 2ts per scene in first-occurrence order -- no second dedup);
//       the input rows are hashed by k_vox_insert into a second table of the same layout (voxel.h: same key packing, the
//                 value is the row's index); k_sparse_query, one thread per (output row, offset), probes it with plain loads;
//       the row count goes to the host through pinned words like ptx_voxel_coarsen's (ptx_wait_counts, no device synchronise).
//   ptx_sparse_conv3d       out[o] = sum_j feats[nbr[o,j]] @ weight[j], output-stationary: a 4-wave work-group owns 64 output rows x
//       64 output channels and loops over the offsets (one without a present neighbour in the tile is skipped: the vote is a
//       ballot over the tile's 64 rows) and over Cin in 64-channel chunks: the 64 indexed rows are gathered into LDS as whole 256-B
//       pieces (16 lanes x 16 B per row, zeros for -1), the 64 x 64 slab of weight[j] beside them (transposed on the way in, so
//       that both operands have k contiguous), and the product runs on v_mfma_f32_32x32x2_f32 with k_gemm64's fragment step
//       (mfma64.h).  Blocked summation in registers: every step's product (at most 64 terms) is formed from zero and then added
//       to the tile's running sum -- one unbroken chain of 27 Cin matrix-instruction updates measured 9.6 x the error of the
//       per-offset fp32 products of the restatement on rows with all 27 neighbours.  Fixed order, no float atomics: bitwise
//       reproducible.
//       Epilogue in registers: + bias, * scale + shift (a folded eval BatchNorm), + residual, ReLU.
//   ptx_sparse_max_pool3d   out[o] = max_j feats[nbr[o,j]] over the present neighbours.
//   ptx_sparse_conv3d_act, ptx_sparse_conv_transpose_gen   the sparse neck's convolutions (neck.py; the rest of the neck is neck.hip):
//       the same kernel with an activation selector (ELU) and Cin up to 1024, and as a generative transposed convolution (kernel 2,
//       stride 2: 8 children per row, no table) -- the NECK template parameter of k_sparse_conv.
//
// The offset index j (row of `weight`) counts x fastest, then y, then z -- our reading of MinkowskiEngine's region iterator,
// "parity unpinned" against ME itself, bit-exact against the host restatement (proxytransformation_amd/sparse.py).
#include "voxel.h"
#include "sparse.h"

namespace ptx {

// ---- kernel map -----------------------------------------------------------------------------------------------------------
struct KmapArgs {
    const int32_t *coords_out;             // (n_out,4): the input rows themselves at stride 1
    const unsigned long long *keys; const int32_t *first; unsigned int mask;      // the index table of the input rows
    int B, ncap, shift, ts, k, kvol, n_in;
    const int32_t *cw;                     // stride 2: {rows, overflow, scene ends} as the coarsening published them (device); else null
    const int32_t *index_overflow;         // input rows whose shifted coordinate left +-2^18
    int32_t *nbr; int32_t *count_words; int32_t *out_scene_end;
    int32_t in_end[64];
};

__global__ __launch_bounds__(256) void k_sparse_query(KmapArgs a)
{
    int n_out = a.n_in;
    if (a.cw != nullptr) {
        n_out = a.cw[0];
        if (n_out < 0 || n_out > a.n_in) n_out = 0;          // a broken emit (PTX_VOX_BROKEN): the host raises, nothing is read here
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // sizes for the host (system scope: the words may be device-mapped pinned host memory it polls); the count last
        for (int b = 0; b < a.B; ++b)
            __hip_atomic_store(a.out_scene_end + b, a.cw != nullptr ? a.cw[2 + b] : a.in_end[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(a.count_words + 1, a.index_overflow[0] + (a.cw != nullptr ? a.cw[1] : 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(a.count_words, a.cw != nullptr ? a.cw[0] : a.n_in, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const int o = (int)(t / a.kvol), j = (int)(t - (long)o * a.kvol);
    if (o >= n_out) return;
    const int4 c = *reinterpret_cast<const int4 *>(a.coords_out + (size_t)o * 4);
    // offset j: x fastest, then y, then z; odd k centred on the output coordinate, even k from it upwards
    const int half = (a.k & 1) ? a.k / 2 : 0;
    const int d[3] = {j % a.k - half, (j / a.k) % a.k - half, j / (a.k * a.k) - half};
    const int p[3] = {c.y + d[0] * a.ts, c.z + d[1] * a.ts, c.w + d[2] * a.ts};
    const int b = c.x;
    int found = -1;
    if (b >= 0 && b < a.B) {
        const int v[3] = {p[0] >> a.shift, p[1] >> a.shift, p[2] >> a.shift};      // exact: every coordinate is a multiple of ts = 1 << shift
        const int gi = vox_find(a.keys, a.first, a.mask, b, v);                    // b * ncap + i of the row that claimed the slot
        if (gi >= 0) found = (b > 0 ? a.in_end[b - 1] : 0) + (gi - b * a.ncap);
    }
    a.nbr[t] = found;
}

struct KmapLayout { size_t coarse, index, points, words, total, table; };
static KmapLayout kmap_layout(int B, int ncap)
{
    KmapLayout L{};
    L.table = align_up(vox_layout(B, ncap).total, 256);
    L.coarse = 0; L.index = L.table;
    L.points = 2 * L.table;                                 // the positions ptx_voxel_coarsen emits beside its rows (unused here)
    L.words = L.points + align_up((size_t)B * ncap * 3 * sizeof(float), 256);
    L.total = L.words + 512;                                // 2 + 64 int32
    return L;
}

// ---- convolution ------------------------------------------------------------------------------------------------------------
struct SpConvArgs {
    const float *feats; const int32_t *nbr; const float *weight;
    const float *bias, *scale, *shift, *residual; float *out;
    int n_in, n_out, kvol, Cin, Cout, relu;                 // relu: NECK instantiations read it as the activation selector (0, 1 ReLU, 2 ELU)
};

// STEM: Cin = 3 (ME.MinkowskiConvolution(3, 64, kernel_size=3, stride=2), mink_resnet.py:57-60): the 27 offsets x 3 channels are one
// K = 81 panel (weight (27,3,Cout) IS the (81,Cout) matrix), padded with zeros to the two 64-wide steps of the loop below.
// WT (the backward's dfeats = sum_j gz[nbr_t[:, j]] @ weight[j]^T, sparse_bwd.hip): the slab is read as (kvol, Cout, Cin) of this launch,
// i.e. k is contiguous in memory already and goes into LDS as 16-byte pieces like the gathered rows; same arithmetic, same order.
// NECK (the layers of neck.py; the backbone's instantiations are untouched by it): 1 -- the activation behind the epilogue is a selector
// (0 none, 1 ReLU, 2 ELU alpha = 1: v > 0 ? v : expm1f(v)); 2 -- also GENERATIVE (MinkowskiGenerativeConvolutionTranspose, kernel 2,
// stride 2): no neighbour table, blockIdx.z = j is the one offset, tile row r reads input row r and writes output row 8 r + j, so the
// launch is the dense product (n, Cin) @ (Cin, 8 Cout) in the same steps.
template <bool STEM, bool WT, int NECK = 0>
__global__ __launch_bounds__(256) void k_sparse_conv(SpConvArgs a)
{
    __shared__ __attribute__((aligned(16))) float As[2][64][LDT];       // [k / 32][row][k % 32]: a 64-channel piece of 64 gathered rows
    __shared__ __attribute__((aligned(16))) float Ws[2][64][LDT];       // [k / 32][col][k % 32]: the slab of weight[j], transposed
    __shared__ int32_t s_nbr[64 * kSpMaxVol];
    __shared__ int s_list[kSpMaxVol + 1];                               // offsets with a neighbour in this tile; [kSpMaxVol]: how many
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1, li = lane & 31, hh = lane >> 5;
    const int row0 = blockIdx.x * 64, col0 = blockIdx.y * 64;
    const int kvol = a.kvol;
    for (int e = tid; NECK != 2 && e < 64 * kvol; e += 256) {
        int v = -1;
        // WT without a table: the generative map, row i reads 8 i + j
        if (row0 + e / kvol < a.n_out) v = (WT && a.nbr == nullptr) ? row0 * kvol + e : a.nbr[(size_t)row0 * kvol + e];
        if (v >= a.n_in) v = -1;                            // (never from ptx_sparse_kernel_map)
        s_nbr[e] = v;
    }
    __syncthreads();
    if (NECK == 2) {
        if (tid == 0) { s_list[0] = blockIdx.z; s_list[kSpMaxVol] = 1; }
    } else if (wid == 0) {                                         // the vote: one ballot over the tile's 64 rows per offset
        int cnt = 0;
        for (int j = 0; j < kvol; ++j) {
            if (__ballot(s_nbr[lane * kvol + j] >= 0) != 0ull) {
                if (lane == 0) s_list[cnt] = j;
                ++cnt;
            }
        }
        if (lane == 0) s_list[kSpMaxVol] = cnt;
    }
    __syncthreads();
    const int nchunk = STEM ? 2 : (a.Cin + 63) >> 6;
    const int nsteps = STEM ? (s_list[kSpMaxVol] > 0 ? 2 : 0) : s_list[kSpMaxVol] * nchunk;
    // staging.  A: thread (ar + 16 i, kq .. kq + 3), 16 lanes = one 256-B row piece.  W: thread (k = wk + 16 i, n = wn .. wn + 3), written
    // transposed (stash_t4)
    const int ar = tid >> 4, kq = (tid & 15) * 4;
    const int wk = lane & 15, wn = (wid * 4 + (lane >> 4)) * 4;
    static_assert(!(STEM && WT), "the stem's dfeats has a kernel of its own");
    float4 av[4], wv[4];
    float tot[16];                                          // the tile's running sum; a step's product is formed apart and added to it
#pragma unroll
    for (int i = 0; i < 16; ++i) tot[i] = 0.0f;
    // epilogue operands are requested up front (k_gemm64)
    const int n = col0 + wc * 32 + li;
    const float bias = a.bias ? a.bias[n] : 0.0f, scale = a.scale ? a.scale[n] : 1.0f, shift = a.shift ? a.shift[n] : 0.0f;
    float resv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = row0 + wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
        resv[r] = (a.residual && row < a.n_out) ? a.residual[(size_t)row * a.Cout + n] : 0.0f;
    }

    auto fetch = [&](int s) {
        const int c0 = (STEM ? s : s % nchunk) << 6;
        const int j = STEM ? 0 : s_list[s / nchunk];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = ar + 16 * i;
            if (STEM) {
                float e[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int k = c0 + kq + q, jj = k / 3;
                    const int idx = k < 81 ? s_nbr[row * kSpMaxVol + jj] : -1;
                    e[q] = idx >= 0 ? a.feats[(size_t)idx * 3 + (k - 3 * jj)] : 0.0f;
                }
                av[i] = make_float4(e[0], e[1], e[2], e[3]);
            } else {
                const int idx = NECK == 2 ? (row0 + row < a.n_out ? row0 + row : -1) : s_nbr[row * kvol + j];
                av[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (idx >= 0 && c0 + kq < a.Cin) av[i] = ld4(a.feats + (size_t)idx * a.Cin + c0 + kq);
            }
            wv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (WT) {                                       // column col0 + row of the slab, k = c0 + kq .. + 3 contiguous (Cin % 64 == 0)
                wv[i] = ld4(a.weight + ((size_t)j * a.Cout + col0 + row) * a.Cin + c0 + kq);
            } else {
                const int k = c0 + wk + 16 * i;             // row of the (kvol * Cin, Cout) weight matrix, minus j * Cin
                const bool wok = STEM ? k < 81 : k < a.Cin;
                if (wok) wv[i] = ld4(a.weight + ((size_t)j * a.Cin + k) * a.Cout + col0 + wn);
            }
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            st4(&As[kq >> 5][ar + 16 * i][kq & 31], av[i]);
            if (WT) st4(&Ws[kq >> 5][ar + 16 * i][kq & 31], wv[i]);
            else stash_t4(Ws, wk + 16 * i, wn, wv[i]);
        }
    };

    if (nsteps > 0) fetch(0);
    for (int s = 0; s < nsteps; ++s) {
        stash();
        __syncthreads();
        if (s + 1 < nsteps) fetch(s + 1);                   // in flight behind this step's matrix instructions
        const int c0 = (STEM ? s : s % nchunk) << 6;
        PTX_SPARSE_STEP(tot, (STEM ? 84 : a.Cin) - c0 > 32);
        __syncthreads();
    }
    // C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = row0 + wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
        float v = tot[r];
        if (a.bias) v = v + bias;
        if (a.scale) v = v * scale;                         // (-ffp-contract=off: two roundings, like the restatement)
        if (a.shift) v = v + shift;
        if (a.residual) v = v + resv[r];
        if (NECK == 0) {
            if (a.relu) v = fmaxf(v, 0.0f);
        } else if (a.relu == 1) {
            v = fmaxf(v, 0.0f);
        } else if (a.relu == 2) {
            v = v > 0.0f ? v : expm1f(v);
        }
        if (row < a.n_out) a.out[((size_t)row * (NECK == 2 ? 8 : 1) + (NECK == 2 ? blockIdx.z : 0)) * a.Cout + n] = v;
    }
}

// ---- max-pool: one thread per (output row, 4 channels) ------------------------------------------------------------------------
// ARG: also the offset that supplied the maximum: the first present neighbour, replaced only by a strictly larger value -- ties go to
// the smallest j; 255 for a row without neighbours
template <bool ARG>
__global__ __launch_bounds__(256) void k_sparse_max_pool(const float *__restrict__ feats, const int32_t *__restrict__ nbr, int n_out,
                                                         int kvol, int C, float *__restrict__ out, uint8_t *__restrict__ arg)
{
    const int c4n = C >> 2;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const int o = (int)(t / c4n), c4 = (int)(t - (long)o * c4n);
    if (o >= n_out) return;
    float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    uchar4 w = make_uchar4(255, 255, 255, 255);
    for (int j = 0; j < kvol; ++j) {
        const int idx = nbr[(size_t)o * kvol + j];
        if (idx < 0) continue;
        const float4 x = *reinterpret_cast<const float4 *>(feats + (size_t)idx * C + c4 * 4);
        if (ARG) {
            if (x.x > m.x || w.x == 255) w.x = (unsigned char)j;
            if (x.y > m.y || w.y == 255) w.y = (unsigned char)j;
            if (x.z > m.z || w.z == 255) w.z = (unsigned char)j;
            if (x.w > m.w || w.w == 255) w.w = (unsigned char)j;
        }
        m.x = fmaxf(m.x, x.x); m.y = fmaxf(m.y, x.y); m.z = fmaxf(m.z, x.z); m.w = fmaxf(m.w, x.w);
    }
    *reinterpret_cast<float4 *>(out + (size_t)o * C + c4 * 4) = m;
    if (ARG) *reinterpret_cast<uchar4 *>(arg + (size_t)o * C + c4 * 4) = w;
}

// both pool entry points: `who` names the one that was called in its messages
template <bool ARG>
static int sparse_max_pool(const char *who, const float *feats, const int32_t *nbr, int n_out, int kvol, int C, float *out, uint8_t *arg,
                           void *stream)
{
    PTX_REQUIRE(n_out >= 0 && kvol >= 1 && kvol <= kSpMaxVol && C >= 4 && C % 4 == 0, "%s: n_out=%d kvol=%d C=%d (C: a multiple of 4)", who,
                n_out, kvol, C);
    if (n_out == 0) return PTX_OK;
    PTX_REQUIRE(feats && nbr && out && (arg || !ARG), "%s: null argument", who);
    PTX_REQUIRE(sp_aligned16({feats, out}) && (reinterpret_cast<uintptr_t>(arg) & 3) == 0, "%s: feats and out must be 16-byte aligned%s", who,
                ARG ? ", arg 4-byte aligned" : "");
    PTX_TRY(sp_rows_fit(who, n_out, C));
    const long threads = (long)n_out * (C / 4);
    hipLaunchKernelGGL(k_sparse_max_pool<ARG>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), feats, nbr,
                       n_out, kvol, C, out, arg);
    PTX_LAUNCHED(ARG ? "k_sparse_max_pool_arg" : "k_sparse_max_pool");
    return PTX_OK;
}

// dfeats (n_in, Cin) = sum_j gz[nbr_t[:, j]] @ weight[j]^T: the forward kernel over the transposed map, rows and widths swapped
int sparse_conv_transposed(const float *gz, int n_out, const int32_t *nbr_t, int n_in, int kvol, const float *weight, int Cin, int Cout,
                           float *dfeats, hipStream_t st)
{
    if (n_in == 0) return PTX_OK;
    const SpConvArgs a{gz, nbr_t, weight, nullptr, nullptr, nullptr, nullptr, dfeats, n_out, n_in, kvol, Cout, Cin, 0};
    hipLaunchKernelGGL((k_sparse_conv<false, true>), dim3(cdiv(n_in, 64), Cin / 64), dim3(256), 0, st, a);
    PTX_LAUNCHED("k_sparse_conv (transposed)");
    return PTX_OK;
}

// the children of row i: rows 8 i + j at coords[i] + offset j of kernel_offsets(2) at the finer stride `half` (x fastest, then y, then z)
__global__ __launch_bounds__(256) void k_gen_coords(const int32_t *__restrict__ coords, int n, int half, int32_t *__restrict__ out)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= 8 * n) return;
    int4 c = *reinterpret_cast<const int4 *>(coords + (size_t)(t >> 3) * 4);
    c.y += (t & 1) * half; c.z += ((t >> 1) & 1) * half; c.w += ((t >> 2) & 1) * half;
    *reinterpret_cast<int4 *>(out + (size_t)t * 4) = c;
}

// ptx_sparse_conv3d (NECK 0: Cin up to 512, `act` a flag) and ptx_sparse_conv3d_act (NECK 1: Cin up to kSpMaxCin, `act` the selector):
// `who` names the one that was called in its messages
template <int NECK>
static int sparse_conv(const char *who, int cin_max, const float *feats, int n_in, const int32_t *nbr, int n_out, int kvol, const float *weight,
                       int Cin, int Cout, const float *bias, const float *scale, const float *shift, const float *residual, int act, float *out,
                       void *stream)
{
    PTX_REQUIRE(n_in >= 0 && n_out >= 0 && (kvol == 1 || kvol == 8 || kvol == 27), "%s: n_in=%d n_out=%d kvol=%d (kvol: 1, 8 or 27)", who, n_in,
                n_out, kvol);
    const bool stem = Cin == 3;
    PTX_REQUIRE(sp_width_ok(Cout) && ((stem && kvol == 27) || (Cin >= 16 && Cin <= cin_max && Cin % 16 == 0)),
                "%s: Cin=%d Cout=%d kvol=%d (Cin: 3 with 27 offsets, or a multiple of 16 up to %d; Cout: a multiple of 64 up to 512)", who, Cin,
                Cout, kvol, cin_max);
    if (n_out == 0) return PTX_OK;
    PTX_REQUIRE((feats || n_in == 0) && nbr && weight && out, "%s: null argument", who);
    PTX_REQUIRE(sp_aligned16({feats, weight}), "%s: feats and weight must be 16-byte aligned", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const SpConvArgs a{feats, nbr, weight, bias, scale, shift, residual, out, n_in, n_out, kvol, Cin, Cout, act};
    const dim3 grid(cdiv(n_out, 64), Cout / 64);
    if (stem) hipLaunchKernelGGL((k_sparse_conv<true, false, NECK>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_sparse_conv<false, false, NECK>), grid, dim3(256), 0, st, a);
    PTX_LAUNCHED("k_sparse_conv");
    return PTX_OK;
}

}  // namespace ptx

using namespace ptx;

extern "C" {

size_t ptx_sparse_kernel_map_workspace_bytes(int B, int ncap)
{
    if (B < 1 || ncap < 1 || B > 64 || (long)B * ncap > (1l << 30)) return 0;
    return kmap_layout(B, ncap).total;
}

int ptx_sparse_kernel_map(const int32_t *coords_in, const int32_t *in_scene_end, int B, int tensor_stride, int kernel_size, int stride,
                          int32_t *coords_out, int32_t *out_scene_end, int32_t *nbr, int32_t *count_words, void *workspace,
                          size_t ws_bytes, void *stream)
{
    PTX_REQUIRE(coords_in && in_scene_end && out_scene_end && nbr && count_words && workspace && (coords_out || stride == 1),
                "ptx_sparse_kernel_map: null argument");
    PTX_REQUIRE(B >= 1 && B <= 64 && tensor_stride >= 1 && (tensor_stride & (tensor_stride - 1)) == 0 && tensor_stride <= (1 << 15) &&
                    kernel_size >= 1 && kernel_size <= 3 && (stride == 1 || stride == 2),
                "ptx_sparse_kernel_map: B=%d tensor_stride=%d kernel_size=%d stride=%d (B <= 64; tensor_stride: a power of two up to 2^15; "
                "kernel_size 1, 2 or 3; stride 1 or 2)", B, tensor_stride, kernel_size, stride);
    int ncap = 1, prev = 0;
    for (int b = 0; b < B; ++b) {
        PTX_REQUIRE(in_scene_end[b] >= prev, "ptx_sparse_kernel_map: scene ends must not decrease");
        ncap = in_scene_end[b] - prev > ncap ? in_scene_end[b] - prev : ncap;
        prev = in_scene_end[b];
    }
    const int n_in = prev, kvol = kernel_size * kernel_size * kernel_size;
    PTX_REQUIRE((long)B * ncap <= (1l << 30) && (long)n_in * kvol < (1l << 31), "ptx_sparse_kernel_map: %d rows x %d offsets is out of range",
                n_in, kvol);
    const KmapLayout L = kmap_layout(B, ncap);
    PTX_TRY(sp_workspace_fits("ptx_sparse_kernel_map", ws_bytes, L.total));
    PTX_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "ptx_sparse_kernel_map: workspace must be 256-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *ws = static_cast<char *>(workspace);
    int32_t *cw = reinterpret_cast<int32_t *>(ws + L.words);
    int shift = 0;
    while ((1 << shift) < tensor_stride) ++shift;
    if (stride == 2)        // the output rows: the coarser level's, by the quantisation kernels themselves
        PTX_TRY(ptx_voxel_coarsen(coords_in, in_scene_end, B, 2 * tensor_stride, 1.0f, coords_out, reinterpret_cast<float *>(ws + L.points),
                                  cw, cw + 2, ws + L.coarse, L.table, stream));
    PTX_TRY(vox_index_rows(coords_in, in_scene_end, B, ncap, shift, ws + L.index, st));
    const VoxLayout V = vox_layout(B, ncap);
    KmapArgs a{stride == 2 ? coords_out : coords_in,
               reinterpret_cast<const unsigned long long *>(ws + L.index + V.keys), reinterpret_cast<const int32_t *>(ws + L.index + V.first),
               V.slots - 1, B, ncap, shift, tensor_stride, kernel_size, kvol, n_in, stride == 2 ? cw : nullptr,
               reinterpret_cast<const int32_t *>(ws + L.index + V.overflow), nbr, count_words, out_scene_end, {}};
    for (int b = 0; b < B; ++b) a.in_end[b] = in_scene_end[b];
    const long threads = (long)n_in * kvol;
    hipLaunchKernelGGL(k_sparse_query, dim3((unsigned)(threads > 0 ? (threads + 255) / 256 : 1)), dim3(256), 0, st, a);
    PTX_LAUNCHED("k_sparse_query");
    return PTX_OK;
}

int ptx_sparse_conv3d(const float *feats, int n_in, const int32_t *nbr, int n_out, int kvol, const float *weight, int Cin, int Cout,
                      const float *bias, const float *scale, const float *shift, const float *residual, int relu, float *out,
                      void *stream)
{
    return sparse_conv<0>("ptx_sparse_conv3d", 512, feats, n_in, nbr, n_out, kvol, weight, Cin, Cout, bias, scale, shift, residual, relu, out,
                          stream);
}

int ptx_sparse_conv3d_act(const float *feats, int n_in, const int32_t *nbr, int n_out, int kvol, const float *weight, int Cin, int Cout,
                          const float *bias, const float *scale, const float *shift, const float *residual, int act, float *out,
                          void *stream)
{
    PTX_REQUIRE(act >= 0 && act <= 2, "ptx_sparse_conv3d_act: act=%d (0 none, 1 ReLU, 2 ELU)", act);
    return sparse_conv<1>("ptx_sparse_conv3d_act", kSpMaxCin, feats, n_in, nbr, n_out, kvol, weight, Cin, Cout, bias, scale, shift, residual,
                          act, out, stream);
}

int ptx_sparse_conv_transpose_gen(const int32_t *coords, int n, int tensor_stride, const float *feats, const float *weight, int Cin, int Cout,
                                  const float *scale, const float *shift, int act, int32_t *coords_out, float *out, void *stream)
{
    PTX_REQUIRE(n >= 0 && n <= (1 << 27) && tensor_stride >= 2 && (tensor_stride & (tensor_stride - 1)) == 0 && tensor_stride <= (1 << 15),
                "ptx_sparse_conv_transpose_gen: n=%d tensor_stride=%d (at most 2^27 rows; tensor_stride: a power of two from 2 to 2^15)", n,
                tensor_stride);
    PTX_REQUIRE(sp_width_ok(Cout) && Cin >= 64 && Cin <= kSpMaxCin && Cin % 64 == 0 && act >= 0 && act <= 2,
                "ptx_sparse_conv_transpose_gen: Cin=%d Cout=%d act=%d (Cin: a multiple of 64 up to %d; Cout: a multiple of 64 up to 512; act: 0 "
                "none, 1 ReLU, 2 ELU)", Cin, Cout, act, kSpMaxCin);
    if (n == 0) return PTX_OK;
    PTX_REQUIRE(coords && feats && weight && coords_out && out, "ptx_sparse_conv_transpose_gen: null argument");
    PTX_REQUIRE(sp_aligned16({feats, weight, coords, coords_out}),
                "ptx_sparse_conv_transpose_gen: coords, feats, weight and coords_out must be 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_gen_coords, dim3(cdiv(8 * n, 256)), dim3(256), 0, st, coords, n, tensor_stride / 2, coords_out);
    PTX_LAUNCHED("k_gen_coords");
    const SpConvArgs a{feats, nullptr, weight, nullptr, scale, shift, nullptr, out, n, n, 8, Cin, Cout, act};
    hipLaunchKernelGGL((k_sparse_conv<false, false, 2>), dim3(cdiv(n, 64), Cout / 64, 8), dim3(256), 0, st, a);
    PTX_LAUNCHED("k_sparse_conv (generative)");
    return PTX_OK;
}

int ptx_sparse_max_pool3d(const float *feats, const int32_t *nbr, int n_out, int kvol, int C, float *out, void *stream)
{
    return sparse_max_pool<false>("ptx_sparse_max_pool3d", feats, nbr, n_out, kvol, C, out, nullptr, stream);
}

int ptx_sparse_max_pool3d_arg(const float *feats, const int32_t *nbr, int n_out, int kvol, int C, float *out, uint8_t *arg, void *stream)
{
    return sparse_max_pool<true>("ptx_sparse_max_pool3d_arg", feats, nbr, n_out, kvol, C, out, arg, stream);
}

}  // extern "C"
