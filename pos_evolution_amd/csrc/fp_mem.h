// fp_mem.h -- an fp value or an XYZZ point to and from global memory, device only.  Two forms, each named for what it assumes of
// the address; a call site picks one and keeps it (the forms differ in speed, not in result).
//
//   fp_words   twelve dword accesses: no alignment assumed beyond the word's own (the Miller workspace, the batch's rows)
//   fp_vec16   three uint4 accesses: the address is 16-byte aligned (point tables, registry rows, workgroup partials)
//
// XYZZ points lie as [x y zz zzz] x 12 words (g1x) and [x0 x1 y0 y1 zz0 zz1 zzz0 zzz1] x 12 words (g2x: a lane of the pair moves
// its own halves, chosen by `role`).
#pragma once
#include "g2.h"

namespace posevo {

struct fp_words {
    static __device__ __forceinline__ void ld(fp& r, const uint32_t* __restrict__ p)
    {
#pragma unroll
        for (int j = 0; j < 12; ++j) r.l[j] = p[j];
    }
    static __device__ __forceinline__ void st(uint32_t* __restrict__ p, const fp& a)
    {
#pragma unroll
        for (int j = 0; j < 12; ++j) p[j] = a.l[j];
    }
};
struct fp_vec16 {
    static __device__ __forceinline__ void ld(fp& v, const uint32_t* __restrict__ src)
    {
        const uint4* s = reinterpret_cast<const uint4*>(src);
        const uint4 a = s[0], b = s[1], c = s[2];
        v.l[0] = a.x; v.l[1] = a.y; v.l[2] = a.z; v.l[3] = a.w;
        v.l[4] = b.x; v.l[5] = b.y; v.l[6] = b.z; v.l[7] = b.w;
        v.l[8] = c.x; v.l[9] = c.y; v.l[10] = c.z; v.l[11] = c.w;
    }
    static __device__ __forceinline__ void st(uint32_t* __restrict__ dst, const fp& v)
    {
        uint4* d = reinterpret_cast<uint4*>(dst);
        d[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
        d[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
        d[2] = make_uint4(v.l[8], v.l[9], v.l[10], v.l[11]);
    }
};

template <class M>
__device__ __forceinline__ void g1x_st(uint32_t* __restrict__ dst, const g1x& p)
{
    M::st(dst, p.x);
    M::st(dst + 12, p.y);
    M::st(dst + 24, p.zz);
    M::st(dst + 36, p.zzz);
}
template <class M>
__device__ __forceinline__ void g2x_st(uint32_t* __restrict__ dst, const g2x& p, bool role)
{
    const int o = role ? 12 : 0;
    M::st(dst + o, p.x);
    M::st(dst + 24 + o, p.y);
    M::st(dst + 48 + o, p.zz);
    M::st(dst + 72 + o, p.zzz);
}
template <class M>
__device__ __forceinline__ void g2x_ld(g2x& p, const uint32_t* __restrict__ src, bool role)
{
    const int o = role ? 12 : 0;
    M::ld(p.x, src + o);
    M::ld(p.y, src + 24 + o);
    M::ld(p.zz, src + 48 + o);
    M::ld(p.zzz, src + 72 + o);
}

}  // namespace posevo
