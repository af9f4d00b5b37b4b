// fp_sqrt.h -- square roots in Fp381 (p = 3 mod 4) for the point decompression kernels, device only.
#pragma once
#include "g1.h"
#include "fp381_s29.h"

namespace posevo {

#ifndef POSEVO_POW_INLINE
#define POSEVO_POW_INLINE __noinline__
#endif
static __device__ const uint32_t FP_HALF[12] = {0xffffd555u, 0xdcff7fffu, 0x58a9ffffu, 0x0f55ffffu, 0x7b587b12u, 0xb3986950u,
                                                0x79c2895fu, 0xb23ba5c2u, 0x21a5d66bu, 0x258dd3dbu, 0x1cbff34du, 0x0d0088f5u};     // (p-1)/2

__device__ __forceinline__ bool limbs_gt(const fp& a, const uint32_t* b)  // a > b as 384-bit integers
{
    bool gt = false, eq = true;
#pragma unroll
    for (int j = 11; j >= 0; --j) {
        gt = gt || (eq && a.l[j] > b[j]);
        eq = eq && a.l[j] == b[j];
    }
    return gt;
}
__device__ __forceinline__ bool fp_is_canonical(const fp& x)  // x < p
{
    uint32_t br = 0;
#pragma unroll
    for (int j = 0; j < 12; ++j) (void)__builtin_subc(x.l[j], fp_p_limb(j), br, &br);
    return br != 0;
}
// a (Montgomery form, any representation of a residue) is "larger" than its negation: plain value > (p-1)/2
__device__ __forceinline__ bool fp_is_larger_half(const fp& a_mont)
{
    fp plain;
    fp_from_mont(plain, a_mont);
    return limbs_gt(plain, FP_HALF);
}
// r = a / 2 (works on Montgomery representatives: halving is linear)
__device__ __forceinline__ void fp_half(fp& r, const fp& a)
{
    uint32_t t[13], c = 0;
    const uint32_t odd = a.l[0] & 1u;
#pragma unroll
    for (int j = 0; j < 12; ++j) t[j] = __builtin_addc(a.l[j], odd ? fp_p_limb(j) : 0u, c, &c);
    t[12] = c;
#pragma unroll
    for (int j = 0; j < 12; ++j) r.l[j] = (t[j] >> 1) | (t[j + 1] << 31);
}
// w = a^((p-3)/4).  With it: a * w = a^((p+1)/4) is the square root of a when a is a quadratic residue (the caller checks
// its square), and then w = 1 / sqrt(a) as well ((a w) w = a^((p-1)/2) = 1) -- the G2 decompression needs both.  When a is NOT a
// residue, (a w)^2 = -a and (a w) w = -1.
// The chain itself runs in the 29-bit form (fp381_s29.h, fq_pow_pm3d4: why, and the windows; the products are
// fp381_lazy.inc's); Montgomery words in, canonical Montgomery words out, one product each way.
__device__ POSEVO_POW_INLINE void fp_pow_pm3d4(fp& w, const fp& a)
{
    fq x, r;
    fq_from_mont32(x, a.l);
    fq_pow_pm3d4(r, x);
    fq_to_mont32(w.l, r);
}
__device__ __forceinline__ void fp_sqrt_candidate(fp& r, const fp& a)
{
    fp w;
    fp_pow_pm3d4(w, a);
    fp_mul(r, w, a);
}
// true iff a is a square; then r^2 == a
__device__ __forceinline__ bool fp_sqrt(fp& r, const fp& a)
{
    fp t;
    fp_sqrt_candidate(r, a);
    fp_sqr(t, r);
    return fp_eq(t, a);
}

// A square root of a = a0 + a1 u in Fp2 = Fp[u]/(u^2 + 1), BOTH components in one lane (the G2 decompression's lane per point;
// the hash-to-curve map, whose lane pair tries its two candidates at once).  y0, y1 and st come in as zero; st stays 0 iff a is a
// square, then (y0 + y1 u)^2 == a; otherwise it becomes 2 ("not on the curve", the decompression's status).
// The "complex method" (p = 3 mod 4): s = sqrt(norm) in Fp, d = (a0 + s)/2, w = d^((p-3)/4):
// y = d w + (a1 w / 2) u if d is a residue, -(a1 w / 2) + (d w) u otherwise -- two windowed Fp exponentiations, no inversion, no
// second attempt.  Which of the two roots comes out is the caller's to settle.
__device__ __forceinline__ void f2_sqrt_lane(fp& y0, fp& y1, int32_t& st, const fp& a0, const fp& a1)
{
    if (fp_is_zero(a1)) {  // a in Fp: t = a0^((p+1)/4) squares to a0 (y = t) or to -a0 (y = u t: -1 is a non-residue)
        fp t, c;
        fp_sqrt_candidate(t, a0);
        fp_sqr(c, t);
        if (fp_eq(c, a0)) y0 = t;
        else y1 = t;
    } else {
        fp n, t, s, d, w, v, c;
        fp_sqr(n, a0);
        fp_sqr(t, a1);
        fp_add(n, n, t);
        if (!fp_sqrt(s, n)) st = 2;  // the norm of a square is a square in Fp
        else {
            // exactly one of d = (a0 + s)/2 and d' = (a0 - s)/2 = -a1^2 / (4 d) is a square.  ONE exponentiation serves both
            // cases and the division: w = d^((p-3)/4), t = d w, v = a1 w / 2.
            //   d a residue:  t^2 = d, w = 1/t:        y = t + v u       (y0^2 - y1^2 = d - a1^2/(4d) = a0, 2 y0 y1 = a1)
            //   otherwise:    t^2 = -d, w^2 = -1/d:    y = -v + t u      (v^2 + d = d' + d = a0, -2 v t = -a1 d w^2 = a1)
            fp_add(d, a0, s);
            fp_half(d, d);
            fp_pow_pm3d4(w, d);
            fp_mul(t, d, w);
            fp_mul(v, a1, w);
            fp_half(v, v);
            fp_sqr(c, t);
            if (fp_eq(c, d)) { y0 = t; y1 = v; }
            else { fp_neg(y0, v); y1 = t; }
        }
    }
    if (st == 0) {  // belt and braces: y^2 == a
        fp t0, t1, t2;
        fp_sqr(t0, y0);
        fp_sqr(t1, y1);
        fp_sub(t0, t0, t1);
        fp_mul(t2, y0, y1);
        fp_dbl(t2, t2);
        if (!fp_eq(t0, a0) || !fp_eq(t2, a1)) st = 2;
    }
}

}  // namespace posevo
