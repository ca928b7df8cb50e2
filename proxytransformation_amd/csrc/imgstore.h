// Storage types of the image features (PtxShape.img_dtype: 0 = fp32, 1 = bf16, 2 = fp16), device code only.
// Every kernel that reads img_feat widens to fp32 on load and does all arithmetic in fp32, so the storage type is
// one load and one conversion per kernel: this header owns both, in the three forms the kernels use --
//   img_load            one element as float (storage type as a template argument, or as a run-time value)
//   img_store           one float rounded to the storage type (the gradients of the features)
//   ImgStore<DT>::px4   4 consecutive pixels of a row, one streaming load at ELEMENT alignment, widened to float[4]
//   ImgStore<DT>::px8   8 consecutive pixels of a row, default cache policy, widened to float[8]
// A row (one channel of one image) is hw elements long and hw may be odd (15 x 15 = 225), so a row starts at element
// alignment only: 4 B for fp32, 2 B for the 16-bit types; gfx950 global_load_dwordx2 / x4 accept that.
#pragma once
#include <hip/hip_runtime.h>

namespace ptx {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));           // 16-B load at 4-B alignment
typedef unsigned int u2u2 __attribute__((ext_vector_type(2), aligned(2)));    // 8-B load at 2-B alignment
typedef unsigned int u4u2 __attribute__((ext_vector_type(4), aligned(2)));    // 16-B load at 2-B alignment

// element `off` of `base` as float.  The template form is for loads on a hot path: a run-time type test inside a
// fetch makes every load its own basic block (train_ops.hip, k_bgemm)
__device__ __forceinline__ float img_load(const void *base, size_t off, int dt)
{
    if (dt == 0) return static_cast<const float *>(base)[off];
    const unsigned short u = static_cast<const unsigned short *>(base)[off];
    if (dt == 1) return __uint_as_float((unsigned int)u << 16);
    return (float)__builtin_bit_cast(_Float16, u);
}
template <int DT>
__device__ __forceinline__ float img_load(const void *base, size_t off) { return img_load(base, off, DT); }

// one element stored in storage type DT, rounded once from fp32 (bf16: to nearest even, like tensor.to(torch.bfloat16))
template <int DT>
__device__ __forceinline__ void img_store(void *base, size_t off, float v)
{
    if (DT == 0) { static_cast<float *>(base)[off] = v; return; }
    if (DT == 1) {
        unsigned int u = __float_as_uint(v);
        if ((u & 0x7f800000u) != 0x7f800000u) u += 0x7fffu + ((u >> 16) & 1u);
        static_cast<unsigned short *>(base)[off] = (unsigned short)(u >> 16);
        return;
    }
    static_cast<unsigned short *>(base)[off] = __builtin_bit_cast(unsigned short, (_Float16)v);
}

template <int DT>   // 1 = bf16, 2 = fp16; fp32 below
struct ImgStore {
    typedef unsigned short elem;
    typedef u32x2 px4;
    typedef u32x4 px8;
    static __device__ __forceinline__ px4 load4_nt(const elem *p) { return __builtin_nontemporal_load(reinterpret_cast<const u2u2 *>(p)); }
    // pixels a + b .. a + b + 7 of `row`
    static __device__ __forceinline__ px8 load8(const elem *row, int a, int b) { return *reinterpret_cast<const u4u2 *>(row + a + b); }
    // element 2i = low half of dword i
    static __device__ __forceinline__ void widen2(unsigned int d, float &lo, float &hi)
    {
        if (DT == 1) { lo = __uint_as_float(d << 16); hi = __uint_as_float(d & 0xffff0000u); }
        else {
            lo = (float)__builtin_bit_cast(_Float16, (unsigned short)(d & 0xffffu));
            hi = (float)__builtin_bit_cast(_Float16, (unsigned short)(d >> 16));
        }
    }
    static __device__ __forceinline__ void widen4(const px4 &d, float (&v)[4])
    {
        widen2(d[0], v[0], v[1]); widen2(d[1], v[2], v[3]);
    }
    static __device__ __forceinline__ void widen8(const px8 &d, float (&v)[8])
    {
#pragma unroll
        for (int i = 0; i < 4; ++i) widen2(d[i], v[2 * i], v[2 * i + 1]);
    }
};

template <>
struct ImgStore<0> {
    typedef float elem;
    typedef f4u px4;
    struct px8 { f4u lo, hi; };
    static __device__ __forceinline__ px4 load4_nt(const elem *p) { return __builtin_nontemporal_load(reinterpret_cast<const f4u *>(p)); }
    static __device__ __forceinline__ px8 load8(const elem *row, int a, int b)
    {
        const int p0 = a + b;
        return px8{*reinterpret_cast<const f4u *>(row + p0), *reinterpret_cast<const f4u *>(row + p0 + 4)};
    }
    static __device__ __forceinline__ void widen4(const px4 &d, float (&v)[4]) { v[0] = d.x; v[1] = d.y; v[2] = d.z; v[3] = d.w; }
    static __device__ __forceinline__ void widen8(const px8 &d, float (&v)[8])
    {
        v[0] = d.lo.x; v[1] = d.lo.y; v[2] = d.lo.z; v[3] = d.lo.w; v[4] = d.hi.x; v[5] = d.hi.y; v[6] = d.hi.z; v[7] = d.hi.w;
    }
};

}  // namespace ptx
