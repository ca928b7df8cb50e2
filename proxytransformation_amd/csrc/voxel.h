// The hash table of the voxel quantisation (voxel.hip), shared with the kernel maps of the sparse convolution (sparse.hip):
// key packing, hash, argument block and workspace layout.  The kernels themselves stay in voxel.hip and are launched from there.
#pragma once
#include "common.h"

namespace ptx {

constexpr int kVoxBias = 1 << 18;          // voxel indices in [-2^18, 2^18): +-2.6 km at 1 cm

struct VoxArgs {
    const float *points; const int32_t *counts; int B, Ncap; float voxel_size;
    unsigned long long *keys; uint32_t *owner; int32_t *first; int32_t *slot_of; int32_t *row_of_slot; unsigned long long *tile_word;
    unsigned int mask;
    int32_t *coords; float *feats; int32_t *inverse; int32_t *overflow; int32_t *nvox_overflow;
    int32_t *scene_end;                    // optional (ptx_voxelize_ex): rows written up to and including scene b
    // coarsening mode (ptx_voxel_coarsen): the "points" are the integer voxel rows of a finer level -- coords_in (rows,4) int32
    // (scene, x, y, z), scene b's rows [in_end[b-1], in_end[b]) -- and the voxel of a row is its coordinate >> shift (floor division
    // by the power-of-two stride); the emitted row carries floor(c / s) * s and the "feature" that coordinate times voxel_size
    const int32_t *coords_in; int shift; int32_t in_end[64];
    int32_t *rep_out;                      // optional (ptx_voxelize_rep): flat padded index b * Ncap + i of the point each row keeps
};

__device__ __forceinline__ int vox_count(const VoxArgs &a, int b)
{
    return a.coords_in == nullptr ? a.counts[b] : a.in_end[b] - (b > 0 ? a.in_end[b - 1] : 0);
}

__device__ __forceinline__ bool vox_key(const VoxArgs &a, int b, int i, int (&v)[3], unsigned long long &key)
{
    bool ok = true;
    if (a.coords_in != nullptr) {
        const int32_t *c = a.coords_in + ((size_t)(b > 0 ? a.in_end[b - 1] : 0) + i) * 4;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            v[d] = c[1 + d] >> a.shift;                                   // arithmetic shift = floor division by the stride
            ok = ok && v[d] >= -kVoxBias && v[d] < kVoxBias;
        }
    } else {
        const float *p = a.points + ((size_t)b * a.Ncap + i) * 3;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float q = floorf(__fdiv_rn(p[d], a.voxel_size));        // torch: floor(p / voxel_size), fp32
            v[d] = (int)q;
            // a NaN quotient converts to 0 and would pass the integer check: only a finite quotient can be inside the range
            ok = ok && __builtin_isfinite(q) && v[d] >= -kVoxBias && v[d] < kVoxBias;
        }
    }
    key = ((unsigned long long)b << 57) | ((unsigned long long)(v[0] + kVoxBias) << 38) |
          ((unsigned long long)(v[1] + kVoxBias) << 19) | (unsigned long long)(v[2] + kVoxBias);
    return ok;
}

__device__ __forceinline__ unsigned int vox_hash(unsigned long long k)
{
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return (unsigned int)k;
}

// The lookup of an index table (vox_index_rows below): first[slot] = b * ncap + i of the row of scene b at voxel v, or -1 when there is
// none.  Plain loads; a voxel outside the key range cannot be a row.  (The table is at most half full: an empty slot ends the probe.)
__device__ __forceinline__ int vox_find(const unsigned long long *keys, const int32_t *first, unsigned int mask, int b, const int (&v)[3])
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if (v[i] < -kVoxBias || v[i] >= kVoxBias) return -1;
    const unsigned long long key = ((unsigned long long)b << 57) | ((unsigned long long)(v[0] + kVoxBias) << 38) |
                                   ((unsigned long long)(v[1] + kVoxBias) << 19) | (unsigned long long)(v[2] + kVoxBias);
    const unsigned long long k1 = key + 1ull;
    unsigned int slot = vox_hash(key) & mask;
    for (unsigned int probes = 0; probes <= mask; ++probes) {
        const unsigned long long cur = keys[slot];
        if (cur == 0ull) break;
        if (cur == k1) return first[slot];
        slot = (slot + 1) & mask;
    }
    return -1;
}

struct VoxLayout { size_t zero_begin, keys, owner, tile_word, overflow, zero_bytes, first, slot_of, row_of_slot, total; unsigned int slots; };
inline VoxLayout vox_layout(int B, int Ncap)
{
    VoxLayout L{};
    const size_t total = (size_t)B * Ncap;
    unsigned int slots = 1024;
    while ((size_t)slots < 2 * total) slots <<= 1;
    L.slots = slots;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o += align_up(bytes, 256); return r; };
    L.zero_begin = o;                                       // cleared by ONE memset per call
    L.keys = take((size_t)slots * 8); L.owner = take((size_t)slots * 4);
    L.tile_word = take((size_t)B * cdiv(Ncap, kTilePts) * 8); L.overflow = take(8);
    L.zero_bytes = o - L.zero_begin;
    L.first = take((size_t)slots * 4); L.slot_of = take(total * 4); L.row_of_slot = take((size_t)slots * 4);
    L.total = o;
    return L;
}

// index mode (ptx_sparse_kernel_map): the rows of coords_in, scene b = [in_scene_end[b-1], in_scene_end[b]), hashed by k_vox_insert at
// coordinate >> shift into a table laid out by vox_layout(B, ncap) at `ws` (one memset + one launch).  Afterwards keys[slot] = key + 1
// and first[slot] = b * ncap + i of a row with that key; the overflow word counts rows whose shifted coordinate left +-2^18.
int vox_index_rows(const int32_t *coords_in, const int32_t *in_scene_end, int B, int ncap, int shift, char *ws, hipStream_t st);

}  // namespace ptx
