// What train_ops.hip (one launch per operator) and train_fused.hip (the fused block) must agree on bit for bit: the dropout rule and the
// exact GELU pair of the training step, and the NaN rule of ReLU, clamp and max pooling.  A (seed, element) pair draws the same mask in either file because both read it from here.
#pragma once
#include "common.h"

namespace ptx {

// ------------------------------------------------------------------------------ dropout / DropPath
// A counter-based generator: element i of stream `seed` is kept iff the hash of (seed, i) maps at or above p; kept values are scaled by
// 1 / (1 - p).  The mask is a pure function of (seed, index), so the backward pass recomputes it.
__device__ __forceinline__ uint32_t drop_mix32(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((x ^ (x >> 31)) >> 32);
}
__host__ __device__ __forceinline__ uint64_t drop_stream(uint64_t seed) { return seed * 0x100000001B3ull; }      // + element index = hash input
__host__ __device__ __forceinline__ uint32_t drop_thresh(float p) { return (uint32_t)((double)p * 4294967296.0); }
__host__ __device__ __forceinline__ float drop_keep_scale(float p) { return 1.0f / (1.0f - p); }

// One dropout site as a kernel argument (made on the host); p == 0 is the identity.
struct Drop1 { uint64_t seed; uint32_t thresh; float ks; int on; };
static inline Drop1 make_drop(float p, uint64_t seed)
{
    Drop1 d;
    d.on = p > 0.0f ? 1 : 0; d.seed = drop_stream(seed);
    d.thresh = drop_thresh(p); d.ks = drop_keep_scale(p);
    return d;
}
__device__ __forceinline__ float drop_apply(const Drop1 &d, float v, uint64_t i)
{
    if (!d.on) return v;
    return drop_mix32(d.seed + i) >= d.thresh ? v * d.ks : 0.0f;
}

// ------------------------------------------------------------------------------ GELU, exact (erff) form, and its derivative
// (common.h's gelu_erf is the eval path's polynomial approximation: not interchangeable with these)
__device__ __forceinline__ float gelu_exact(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }
__device__ __forceinline__ float gelu_exact_g(float x)
{
    const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752440f));
    return cdf + x * 0.3989422804014327f * expf(-0.5f * x * x);
}

// ------------------------------------------------------------------------------ NaN rule of the forward values
// fmaxf / fminf return the other operand when one is NaN; nn.ReLU, torch.min / torch.max and torch.max(dim) of the reference return
// the NaN (and, for the pooling, the index of the first one).  A diverged run must show NaN here as it does there.  On every other
// input these give the bits fmaxf / fminf and a plain `>` gave.
__device__ __forceinline__ float relu_nan(float v) { return v != v ? v : fmaxf(v, 0.0f); }
__device__ __forceinline__ float min_nan(float a, float b) { return (a != a || b != b) ? a + b : fminf(a, b); }
__device__ __forceinline__ float max_nan(float a, float b) { return (a != a || b != b) ? a + b : fmaxf(a, b); }
// running first-arg-max: does v replace best?  (best stays once it is NaN: the first NaN keeps the arg)
__device__ __forceinline__ bool max_takes(float v, float best) { return v > best || (v != v && best == best); }

}  // namespace ptx
