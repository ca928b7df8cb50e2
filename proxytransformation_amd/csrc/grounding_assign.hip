// Hungarian matching on the device (ptx_gl_assign): the rectangular shortest-augmenting-path solver (Jonker-Volgenant as Crouse states
// it, the form scipy's linear_sum_assignment uses) on every (layer, scene) column range of ptx_gl_cost's matrices, ONE WAVE per problem.
// proxytransformation_amd/grounding_loss_host.py (sap_assign_host) restates it in numpy float64 and is the specification, bit for bit:
// every comparison below is a comparison of doubles formed by the same additions and subtractions in the same order.
//
// The smaller side of the K x G_b matrix supplies the rows (n = min(K, G_b), taken in increasing index), the larger the columns
// (m = max(K, G_b)).  Column j lives in lane j & 63, slot j >> 6 (16 slots at m = 1024): its path cost, its dual and its "scanned" bit
// are registers; what is read by index -- the row duals, col4row, row4col, the predecessors and the tree's rows -- is LDS.
// THE TIE RULE: among the columns not yet scanned that share the smallest path cost, the lowest column index is taken.
//
// A work-group is one wave: its __syncthreads() are no hardware barrier worth the name, they keep the compiler from moving one lane's
// LDS read above another lane's LDS write (it reasons about one thread's addresses).
//
// TERMINATION: n augmentations, at most n + 1 tree steps each (a step scans one column out; a tree holds the new row and at most n - 1
// matched ones), at most 16 slots per step, a walk back of at most n + 1 edges.  No loop's exit depends on data alone.  After the NaN /
// inf mapping every entry is finite, so every step finds a column; should one not (or a predecessor be out of range), the problem stops
// augmenting and the rows it has not matched stay -1.
#include <climits>

#include "head.h"

namespace ptx {

constexpr int kGaMaxRows = 256, kGaMaxCols = 1024, kGaSlots = kGaMaxCols / kWave;
constexpr int kGaStageFloats = 32768;                       // 128 KiB of the 160: the transposed matrix when it fits (256 x 128, 1024 x 32)

// _solve's nan_to_num(cost, 100, 100, -100)
__device__ __forceinline__ float ga_map(float c)
{
    if (c != c) return 100.0f;
    if (c == INFINITY) return 100.0f;
    if (c == -INFINITY) return -100.0f;
    return c;
}

template <int N>
__device__ __forceinline__ double ga_ror(double v)
{
    const long long b = __double_as_longlong(v);
    const int lo = PTX_ROR_I((int)b, N), hi = PTX_ROR_I((int)(b >> 32), N);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

__device__ __forceinline__ double ga_lane(double v, int l)
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)b, l), hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

__device__ __forceinline__ double ga_min(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ int ga_min(int a, int b) { return b < a ? b : a; }

// every lane ends with the smallest value of the 64 (no NaN among them)
__device__ __forceinline__ double ga_wave_min(double v)
{
    v = ga_min(v, ga_ror<8>(v)); v = ga_min(v, ga_ror<4>(v)); v = ga_min(v, ga_ror<2>(v)); v = ga_min(v, ga_ror<1>(v));
    return ga_min(ga_min(ga_lane(v, 0), ga_lane(v, 16)), ga_min(ga_lane(v, 32), ga_lane(v, 48)));
}

__device__ __forceinline__ int ga_wave_min(int v)
{
    v = ga_min(v, PTX_ROR_I(v, 8)); v = ga_min(v, PTX_ROR_I(v, 4)); v = ga_min(v, PTX_ROR_I(v, 2)); v = ga_min(v, PTX_ROR_I(v, 1));
    return ga_min(ga_min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
                  ga_min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

struct GaArgs {
    const float *cost; const int32_t *gt_offset; int32_t *assign;
    int NL, B, K, SG, max_g, staged;
};

__global__ __launch_bounds__(64) void k_gl_assign(GaArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float ga_stage[];      // [n][m], mapped, when a.staged
    __shared__ double s_u[kGaMaxRows];                      // row duals
    __shared__ double s_d[kGaMaxRows + 2];                  // the path cost at which tree row t was reached
    __shared__ int s_tree[kGaMaxRows + 2];                  // the tree's rows in the order they were reached
    __shared__ int s_col4row[kGaMaxRows];
    __shared__ int s_row4col[kGaMaxCols];
    __shared__ int s_path[kGaMaxCols];                      // predecessor row of a column
    __shared__ int s_ok;

    const int lane = threadIdx.x;
    const int l = blockIdx.x / a.B, b = blockIdx.x % a.B;
    const int K = a.K, SG = a.SG;
    int32_t *out = a.assign + ((size_t)l * a.B + b) * K;
    const int lo = a.gt_offset[b], hi = a.gt_offset[b + 1];
    const int G = hi - lo;
    if (lo < 0 || hi < lo || hi > SG || G > a.max_g || G == 0) {          // nothing of cost is read
        for (int k = lane; k < K; k += kWave) out[k] = -1;
        return;
    }
    const bool qrows = G > K;                               // the rows are the queries (else the boxes)
    const int n = qrows ? K : G, m = qrows ? G : K;
    const int nslots = (m + kWave - 1) / kWave;
    const float *cl = a.cost + (size_t)l * K * SG + lo;     // element (query k, box g) at cl[k * SG + g]

    if (a.staged) {                                         // read as the matrix lies, written transposed when the rows are the boxes
        const int total = K * G;
        for (int e = lane; e < total; e += kWave) {
            const int k = e / G, g = e - k * G;
            ga_stage[qrows ? e : g * K + k] = ga_map(cl[(size_t)k * SG + g]);
        }
    }
    for (int i = lane; i < n; i += kWave) { s_u[i] = 0.0; s_col4row[i] = -1; }
    for (int j = lane; j < m; j += kWave) { s_row4col[j] = -1; s_path[j] = -1; }
    if (lane == 0) s_ok = 1;
    __syncthreads();

    double v[kGaSlots];
#pragma unroll
    for (int s = 0; s < kGaSlots; ++s) v[s] = 0.0;

    bool ok = true;
    for (int cur = 0; cur < n && ok; ++cur) {
        double spc[kGaSlots];
#pragma unroll
        for (int s = 0; s < kGaSlots; ++s) spc[s] = INFINITY;
        unsigned scanned = 0u;                              // bit s: this lane's column of slot s has left the remaining set
        double min_val = 0.0;
        int i = cur, sink = -1, steps = 0;
        for (int t = 0; t <= n && sink < 0 && ok; ++t) {
            const double ui = s_u[i];
            double best = INFINITY;
            int best_j = INT_MAX;
#pragma unroll
            for (int s = 0; s < kGaSlots; ++s) {
                const int j = s * kWave + lane;
                if (s < nslots && j < m && !((scanned >> s) & 1u)) {
                    const float c = a.staged ? ga_stage[i * m + j] : ga_map(qrows ? cl[(size_t)i * SG + j] : cl[(size_t)j * SG + i]);
                    const double r = ((min_val + (double)c) - ui) - v[s];        // additions and subtractions in this order, no product
                    if (r < spc[s]) { spc[s] = r; s_path[j] = i; }
                    if (spc[s] < best) { best = spc[s]; best_j = j; }            // ascending j: the lane's lowest index on a tie
                }
            }
            const double lowest = ga_wave_min(best);
            const int j = ga_wave_min(best == lowest ? best_j : INT_MAX);         // the tie rule: the lowest column index
            if (!(lowest < INFINITY) || j >= m) { ok = false; break; }
            min_val = lowest;
            if (lane == (j & 63)) scanned |= 1u << (j >> 6);
            steps = t + 1;
            const int r4c = __builtin_amdgcn_readfirstlane(s_row4col[j]);   // (one address: the value is the wave's)
            if (r4c < 0) {
                sink = j;
            } else {
                i = r4c;
                if (lane == 0) { s_tree[t + 1] = i; s_d[t + 1] = lowest; }
            }
        }
        if (sink < 0) ok = false;
        if (!ok) break;
        __syncthreads();                                    // s_path, s_tree, s_d of the search are visible

        // the duals: u[cur] += min_val; u[i] += min_val - spc[col4row[i]] for the other rows of the tree (spc of a scanned column is the
        // `lowest` of its step: s_d); v[j] -= min_val - spc[j] on the scanned columns
        if (lane == 0) s_u[cur] = s_u[cur] + min_val;
        for (int t = 1 + lane; t < steps; t += kWave) {
            const int r = s_tree[t];
            s_u[r] = s_u[r] + (min_val - s_d[t]);
        }
#pragma unroll
        for (int s = 0; s < kGaSlots; ++s)
            if ((scanned >> s) & 1u) v[s] = v[s] - (min_val - spc[s]);

        if (lane == 0) {                                    // walk back from the sink: at most `steps` edges
            int j = sink, good = 0;
            for (int t = 0; t < steps; ++t) {
                const int r = s_path[j];
                if (r < 0 || r >= n) break;
                s_row4col[j] = r;
                const int next = s_col4row[r];
                s_col4row[r] = j;
                j = next;
                if (r == cur) { good = 1; break; }
                if (j < 0 || j >= m) break;
            }
            if (!good) s_ok = 0;
        }
        __syncthreads();
        ok = __builtin_amdgcn_readfirstlane(s_ok) != 0;
    }

    // every entry of the scene is written: the matched box of query k, else -1
    for (int k = lane; k < K; k += kWave) out[k] = qrows ? s_col4row[k] : s_row4col[k];
}

}  // namespace ptx

using namespace ptx;

extern "C" {

int ptx_gl_assign(const float *cost, int NL, int B, int K, const int32_t *gt_offset, int SG, int max_g, int32_t *assign, void *stream)
{
    const char *who = "ptx_gl_assign";
    PTX_REQUIRE(NL >= 1 && NL <= 64 && B >= 1 && B <= kHeadMaxScenes && K >= 1 && K <= kHeadMaxK,
                "%s: NL=%d B=%d K=%d (NL, B: 1 to 64; K: 1 to 1024)", who, NL, B, K);
    PTX_REQUIRE(SG >= 1 && SG <= (1 << 16) && max_g >= 1 && max_g <= SG, "%s: SG=%d max_g=%d (1 to 65536 ground-truth boxes; 1 <= max_g <= SG)",
                who, SG, max_g);
    const int n = K < max_g ? K : max_g, m = K < max_g ? max_g : K;
    PTX_REQUIRE(n <= kGaMaxRows && m <= kGaMaxCols, "%s: K=%d max_g=%d (the device solver takes min(K, G_b) <= %d and max(K, G_b) <= %d)", who,
                K, max_g, kGaMaxRows, kGaMaxCols);
    PTX_REQUIRE(cost && gt_offset && assign, "%s: null argument", who);
    GaArgs a{};
    a.cost = cost; a.gt_offset = gt_offset; a.assign = assign;
    a.NL = NL; a.B = B; a.K = K; a.SG = SG; a.max_g = max_g;
    a.staged = n * m <= kGaStageFloats;
    const int lds = a.staged ? n * m * (int)sizeof(float) : 0;
    if (lds > 32 * 1024)
        PTX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_gl_assign), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    hipLaunchKernelGGL(k_gl_assign, dim3((unsigned)(NL * B)), dim3(kWave), (size_t)lds, static_cast<hipStream_t>(stream), a);
    PTX_LAUNCHED("k_gl_assign");
    return PTX_OK;
}

}  // extern "C"
