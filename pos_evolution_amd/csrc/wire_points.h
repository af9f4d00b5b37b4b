// wire_points.h -- uncompressed wire bytes to a Montgomery point, with the curve equation, device only (k_bls_prepare,
// k_bls_batch_settle).  Flag bits live in the leading byte alone (0x80 compressed: refused here, 0x40 infinity); fp_load_be48
// masks them in every 48-byte element, so an element that has none gets its top limb read again in full.
#pragma once
#include "g2.h"

namespace posevo {

__device__ __forceinline__ void fp_set_small_mont(fp& r, uint32_t v)
{
    fp t;
    fp_set_zero(t);
    t.l[0] = v;
    fp_to_mont(r, t);
}
// 96 wire bytes -> (x, y) in Montgomery form, zero for the identity; returns "not a point of y^2 = x^3 + 4"
__device__ __forceinline__ bool wire_load_g1(fp& mx, fp& my, bool& inf, const uint8_t* __restrict__ a)
{
    fp_set_zero(mx);
    fp_set_zero(my);
    inf = (a[0] & 0x40) != 0;
    if (inf) return false;
    fp x, y, t, u, four;
    fp_load_be48(x, a);
    fp_load_be48(y, a + 48);
    y.l[11] = __builtin_bswap32(reinterpret_cast<const uint32_t*>(a + 48)[0]);  // only the leading byte has flags
    bool bad = (a[0] & 0x80) != 0 || !fp_is_canonical(x) || !fp_is_canonical(y);
    fp_to_mont(mx, x);
    fp_to_mont(my, y);
    fp_set_small_mont(four, 4);
    fp_sqr(t, mx);
    fp_mul(t, t, mx);
    fp_add(t, t, four);
    fp_sqr(u, my);
    bad |= !fp_eq(t, u);
    return bad;
}
// 192 wire bytes (c1 first) -> this lane's halves of (x, y); returns "not a point of y^2 = x^3 + 4 (1 + u)" (pair-wide)
__device__ __forceinline__ bool wire_load_g2(fp& mx, fp& my, bool& inf, const uint8_t* __restrict__ b, bool role)
{
    fp_set_zero(mx);
    fp_set_zero(my);
    inf = (b[0] & 0x40) != 0;
    bool bad = false;
    if (!inf) {  // both lanes of the pair take this branch
        fp x, y, t, u, four;
        const uint8_t* xs = b + (role ? 0 : 48);
        const uint8_t* ys = b + 96 + (role ? 0 : 48);
        fp_load_be48(x, xs);
        if (!role) x.l[11] = __builtin_bswap32(reinterpret_cast<const uint32_t*>(xs)[0]);
        fp_load_be48(y, ys);
        y.l[11] = __builtin_bswap32(reinterpret_cast<const uint32_t*>(ys)[0]);
        bad = (b[0] & 0x80) != 0 || !fp_is_canonical(x) || !fp_is_canonical(y);
        fp_to_mont(mx, x);
        fp_to_mont(my, y);
        fp_set_small_mont(four, 4);
        f2_sqr(t, mx, role);
        f2_mul(t, t, mx, role);
        fp_add(t, t, four);
        f2_sqr(u, my, role);
        bad |= !fp_eq(t, u);
    }
    return !pair_and(!bad);
}

}  // namespace posevo
