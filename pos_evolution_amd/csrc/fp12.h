// fp12.h -- the extension tower of BLS12-381 over the Montgomery 12 x 32 fp (fp381.h) and the lane-pair Fp2 (g2.h), device only.
//
//   Fp2 = Fp[u]/(u^2 + 1), xi = 1 + u, Fp6 = Fp2[v]/(v^3 - xi), Fp12 = Fp6[w]/(w^2 - v).
// With v = w^2 this is Fp2[w]/(w^6 - xi): an Fp12 value is six Fp2 coefficients c_0 .. c_5 of w^0 .. w^5, c_(2i+j) the
// coefficient of v^i w^j of the tower.
//
// Layout (component-parallel, the idea of g2.h carried on): SIX LANE PAIRS of a 16-lane row make one Fp12 value -- lane pair k
// (lanes 2k, 2k+1 of the row) holds c_k, one Fp component per lane; lanes 12 .. 15 of the row idle.  A wave is four rows.
// Values live in a SLOT FILE in LDS, word-major per wave: word j of slot s of lane L at lds[(s * 12 + j) * 64 + L] (conflict
// free for a wave-wide access).  An Fp12 value is one slot over the row's 12 lanes; a lane reads the coefficients of other
// lane pairs from their lanes of the slot and exchanges the two halves of an Fp2 value with its partner through DPP (fp_xchg),
// as g2.h does.  Nothing of an Fp12 value is held in registers across operations: a lane's working set is a handful of fp
// values, which is what keeps these kernels free of scratch (a one-lane Fp12 value alone is 144 VGPRs).
//
// Every operation here COMPUTES the calling lane's component of the result into registers and writes nothing: the caller
// separates the reads of a slot from its overwrite with a barrier (the workgroup is one wave).
#pragma once
#include "g2.h"

namespace posevo {

struct bls_lane {
    uint32_t* lds;  // the wave's slot file
    int lane;       // 0 .. 63
    int row;        // first lane of the 16-lane row
    int k;          // coefficient index 0 .. 5 (idle lanes: 0, they never store)
    bool role;      // Fp2 component
    bool act;       // lane < 12 within the row
};

__device__ __forceinline__ bls_lane bls_lane_init(uint32_t* lds)
{
    bls_lane c;
    c.lds = lds;
    c.lane = (int)(threadIdx.x & 63);
    c.row = c.lane & ~15;
    const int in_row = c.lane & 15;
    c.act = in_row < 12;
    c.k = c.act ? (in_row >> 1) : 0;
    c.role = (c.lane & 1) != 0;
    return c;
}
__device__ __forceinline__ void slot_ld(fp& r, const uint32_t* lds, int s, int lane)
{
#pragma unroll
    for (int j = 0; j < 12; ++j) r.l[j] = lds[(s * 12 + j) * 64 + lane];
}
__device__ __forceinline__ void slot_st(uint32_t* lds, int s, int lane, const fp& a)
{
#pragma unroll
    for (int j = 0; j < 12; ++j) lds[(s * 12 + j) * 64 + lane] = a.l[j];
}
// this lane's component of coefficient i of the Fp12 value in slot s
__device__ __forceinline__ void f12_coeff(fp& r, const bls_lane& c, int s, int i) { slot_ld(r, c.lds, s, c.row + 2 * i + (int)c.role); }
// this lane's component of the Fp12 one: the Montgomery one in the c0 lane of lane pair 0, zero everywhere else
__device__ __forceinline__ void f12_one_coeff(fp& r, const bls_lane& c)
{
    fp_set_zero(r);
    if (c.k == 0 && !c.role) fp_set_one(r);
}

// r = xi * a = (a0 - a1) + (a0 + a1) u
__device__ __forceinline__ void f2_mul_xi(fp& r, const fp& a, bool role)
{
    fp o, s, d;
    fp_xchg(o, a);
    fp_add(s, o, a);
    fp_sub(d, a, o);
    fp_select(r, role, s, d);
}
__device__ __forceinline__ void f2_conj(fp& r, const fp& a, bool role)
{
    fp n;
    fp_neg(n, a);
    fp_select(r, role, n, a);
}
// Montgomery in, Montgomery out, inlined (the called forms of g1.h keep state across a call in scratch)
__device__ __forceinline__ void fp_inv_inline(fp& r, const fp& a)
{
    uint32_t plain[12];
    sg_modinv(plain, a.l, SG_PINV30);  // (aR)^-1 as a plain integer = a^-1 R^-1
    fp t, r3;
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        t.l[j] = plain[j];
        r3.l[j] = fp_r3_limb(j);
    }
    fp_mul(r, t, r3);
}
// r = a^-1 = conj(a) / (a0^2 + a1^2), Montgomery form (f2_inv_plain's formula)
__device__ __forceinline__ void f2_inv(fp& r, const fp& a, bool role)
{
    fp sq, sqo, n, ni, t, nt;
    fp_sqr(sq, a);
    fp_xchg(sqo, sq);
    fp_add(n, sq, sqo);
    fp_inv_inline(ni, n);
    fp_mul(t, a, ni);
    fp_neg(nt, t);
    fp_select(r, role, nt, t);
}

// One term of a product: acc += x * y, into the plain sum s or, when the term wraps past w^6, into the sum w that xi multiplies.
__device__ __forceinline__ void f12_acc(fp& s, fp& w, const fp& x, const fp& y, bool wrap, bool role)
{
    fp t, s2, w2;
    f2_mul(t, x, y, role);
    fp_add(s2, s, t);
    fp_add(w2, w, t);
    fp_select(s, wrap, s, s2);
    fp_select(w, wrap, w2, w);
}
__device__ __forceinline__ void f12_fold(fp& r, const fp& s, const fp& w, bool role)
{
    fp x;
    f2_mul_xi(x, w, role);
    fp_add(r, s, x);
}

// r = a * b: c_k = sum_{i + j = k} a_i b_j + xi sum_{i + j = k + 6} a_i b_j -- 6 Fp2 products per lane pair = 12 Fp products
// per lane (schoolbook over the six coefficients: 144 lane products against 54 of Karatsuba in one lane, at a twelfth of the
// registers and a depth of 12)
__device__ __forceinline__ void f12_mul(fp& r, const bls_lane& c, int sa, int sb)
{
    fp s, w;
    fp_set_zero(s);
    fp_set_zero(w);
#pragma unroll 1
    for (int i = 0; i < 6; ++i) {
        const bool wrap = i > c.k;
        const int j = c.k - i + (wrap ? 6 : 0);
        fp x, y;
        f12_coeff(x, c, sa, i);
        f12_coeff(y, c, sb, j);
        f12_acc(s, w, x, y, wrap, c.role);
    }
    f12_fold(r, s, w, c.role);
}
// the general squaring is the product with itself (the Miller loop's 63 squarings; the final exponentiation squares
// cyclotomically)
__device__ __forceinline__ void f12_sqr(fp& r, const bls_lane& c, int sa) { f12_mul(r, c, sa, sa); }

// r = f * (l0 + l2 w^2 + l3 w^3), the line in slots sl, sl + 1, sl + 2 of lane pair `owner` of the row: 3 Fp2 products
__device__ __forceinline__ void f12_mul_line(fp& r, const bls_lane& c, int sf, int sl, int owner)
{
    fp s, w;
    fp_set_zero(s);
    fp_set_zero(w);
#pragma unroll 1
    for (int t = 0; t < 3; ++t) {
        const int sh = t == 0 ? 0 : t + 1;  // 0, 2, 3
        const bool wrap = c.k < sh;
        const int j = c.k - sh + (wrap ? 6 : 0);
        fp x, y;
        f12_coeff(x, c, sf, j);
        f12_coeff(y, c, sl + t, owner);
        f12_acc(s, w, x, y, wrap, c.role);
    }
    f12_fold(r, s, w, c.role);
}

// a^(p^6): w -> -w
__device__ __forceinline__ void f12_conj(fp& r, const bls_lane& c, int sa)
{
    fp a, n;
    slot_ld(a, c.lds, sa, c.lane);
    fp_neg(n, a);
    fp_select(r, (c.k & 1) != 0, n, a);
}
// a^(p^n), n = 1, 2, 3: c_k^(p^n) * xi^(k (p^n - 1) / 6); frob = BLS_FROB[n - 1] of bls_consts.inc
__device__ __forceinline__ void f12_frobenius(fp& r, const bls_lane& c, int sa, int n, const uint32_t (*frob)[2][12])
{
    fp a, x, g;
    slot_ld(a, c.lds, sa, c.lane);
    f2_conj(x, a, c.role);
    fp_select(x, (n & 1) != 0, x, a);
#pragma unroll
    for (int j = 0; j < 12; ++j) g.l[j] = frob[c.k][(int)c.role][j];
    f2_mul(r, x, g, c.role);
}
// Granger-Scott squaring in the cyclotomic subgroup: with A_i = c_i + c_(i+3) s (s = w^3, s^2 = xi),
//   a^2 = (3 A_0^2 - 2 conj A_0) + (3 s A_2^2 + 2 conj A_1) w + (3 A_1^2 - 2 conj A_2) w^2.
// Lane pair k squares ONE Fp4 value (x + y s)^2 = (x^2 + xi y^2) + ((x + y)^2 - x^2 - y^2) s and keeps one half of it:
// 3 Fp products per lane against 12.  (cj, part, plus) = BLS_CYCLO_J / _PART / _PLUS [k].
__device__ __forceinline__ void f12_cyclo_sqr(fp& r, const bls_lane& c, int sa, int cj, int part, bool plus)
{
    fp x, y, x2, y2, t, hi, lo, xh, own;
    f12_coeff(x, c, sa, cj);
    f12_coeff(y, c, sa, cj + 3);
    f2_sqr(x2, x, c.role);
    f2_sqr(y2, y, c.role);
    fp_add(t, x, y);
    f2_sqr(hi, t, c.role);
    fp_sub(hi, hi, x2);
    fp_sub(hi, hi, y2);
    f2_mul_xi(t, y2, c.role);
    fp_add(lo, x2, t);
    f2_mul_xi(xh, hi, c.role);
    fp_select(t, part == 1, hi, xh);
    fp_select(t, part == 0, lo, t);
    fp_dbl(x, t);
    fp_add(t, x, t);  // 3 part
    slot_ld(own, c.lds, sa, c.lane);
    fp_dbl(own, own);
    fp_add(x, t, own);
    fp_sub(y, t, own);
    fp_select(r, plus, x, y);
}
// r = a / n0, n0 in Fp2 the coefficient 0 of the value in slot sn (all its other coefficients are zero): the last step of
// the inversion a^-1 = conj(a) B / (a conj(a) B), B = b^(p^2) b^(p^4), b = a conj(a)
__device__ __forceinline__ void f12_scale_inv(fp& r, const bls_lane& c, int sa, int sn)
{
    fp a, n, i;
    slot_ld(a, c.lds, sa, c.lane);
    f12_coeff(n, c, sn, 0);
    f2_inv(i, n, c.role);
    f2_mul(r, a, i, c.role);
}

}  // namespace posevo
