// fp381_s30.h -- BLS12-381 base field in 13 signed limbs of 30 bits ("S30"), Montgomery constant R = 2^390.
//
// The accumulation's and the tree's field form since round 7 (g1_s30.h, g1_kernels.hip).  It is fp381_s29.h's form made
// one limb narrower: the column of the interleaved (FIPS) Montgomery product -- up to 13 a_i b_j + 13 m_i p_j terms -- still
// fits a signed 64-bit accumulator, because EVERY factor is a balanced digit, |d| <= 2^29 + small:
//   * product operands: limbs 0..11 |l| <= 2^29 + 16, the top limb |l| <= 2^24 (values below ~2^384, a few p);
//   * Montgomery digits m = digit(acc n0inv) in [-2^29, 2^29) (S29: [0, 2^29));
//   * the limbs of p, written as balanced digits (fp381_s30_consts.inc).
// Column 12, the widest, holds 11 full a b terms and 12 full m p terms (the ones with a top limb or p's top limb are
// < 2^54): 23 (2^29 + 16)^2 + small ~ 2^62.6 < 2^63; tests/test_host_fp30.py derives every column's bound from the limb
// bounds above and also runs the product with every column recomputed in 128 bits.  One v_mad_i64_i32 per limb product,
// 13^2 + 13^2 = 338 per product (S29: 392), 91 + 169 = 260 per squaring (S29: 301).
//
// The price of the width: S29 fed a limb-wise difference of two balanced values (|limb| <= 2^29) straight into a product;
// here such a difference (|limb| <= 2^30) goes through ONE carry pass first (fq_sub_norm: four instructions per limb, no
// chain).  Registry rows are stored as balanced digits (fq_from_mont32).
//
// Lazy, signed values.  With m signed, a product lies in (a b / R - p/2, a b / R + p/2) -- |m| <= 2^29 (R - 1) / (2^30 - 1),
// so |m p / R| < (p / 2)(1 + 2^-29).  R / p ~ 2^9.3: operands within 4 p give |a b / R| < 0.03 p, i.e. every product
// of the formulas lies in (-0.53 p, 0.53 p) and everything they compute stays within +-3 p.  Equality with zero is a filter
// on the low 30 bits against the multiples of p a value can be (FQ_KP_LO .. FQ_KP_LO + FQ_KP_N - 1: -8 .. 8), and an
// exact comparison behind it (fq_is_zero_modp).
//
// Names live in posevo::s30 so that this form and S29 (which sits in posevo itself, and which the square roots keep) can
// share a translation unit.  Host + device, plain C++, like fp381_s29.h; the point formulas over it: g1_s30.h (g1_lazy.inc).
#pragma once
#include <stdint.h>

#include "pe_hd.h"

// The column accumulator of the products.  A host test build may define it as a checked 128-bit type (tests/native/fp30_host.cpp);
// the code below uses only  T acc = 0;  acc += int64;  acc >>= n;  (int64_t)acc.
#ifndef PE_FQ30_ACC
#define PE_FQ30_ACC int64_t
#endif

namespace posevo {
namespace s30 {

constexpr int FQ_B = 30, FQ_N = 13;
constexpr int32_t FQ_MASK = (1 << FQ_B) - 1;

#include "fp381_s30_consts.inc"

struct fq {
    int32_t l[FQ_N];  // value = sum l[i] 2^(30 i); limbs 0..11 nominally balanced digits in [-2^29, 2^29), the top limb the rest
};

PE_HD void fq_set_zero(fq& r)
{
#pragma unroll
    for (int i = 0; i < FQ_N; ++i) r.l[i] = 0;
}
PE_HD void fq_set_one(fq& r)
{
#pragma unroll
    for (int i = 0; i < FQ_N; ++i) r.l[i] = FQ_ONE[i];
}
PE_HD bool fq_limbs_zero(const fq& a)  // all limbs zero (the encoding of "no point"); NOT a test mod p
{
    int32_t o = 0;
#pragma unroll
    for (int i = 0; i < FQ_N; ++i) o |= a.l[i];
    return o == 0;
}

// r = a - b, limb by limb.  NOT a product operand (|limb| up to 2^30 + 4): the same-x filter reads it, and the carry
// pass below makes one of it.
PE_HD void fq_sub(fq& r, const fq& a, const fq& b)
{
#pragma unroll
    for (int i = 0; i < FQ_N; ++i) r.l[i] = a.l[i] - b.l[i];
}
// The balanced digit of a value: its low 30 bits read as a signed number in [-2^29, 2^29) (signed on purpose: see fp381_s29.h,
// a signed x signed 32 x 32 -> 64 multiply is one v_mad_i64_i32).
PE_HD int32_t fq_digit(int64_t v) { return (int32_t)((uint32_t)v << (32 - FQ_B)) >> (32 - FQ_B); }
PE_HD int32_t fq_digit32(int32_t v) { return (int32_t)((uint32_t)v << (32 - FQ_B)) >> (32 - FQ_B); }
// The carry that goes with fq_digit32: (v - digit) / 2^30 = floor(v / 2^30) + bit 29, computed without forming v - digit
// (which leaves the int32 range for |v| near 2^31).  In [-2, 2] for any int32 v.
PE_HD int32_t fq_carry32(int32_t v) { return (v >> FQ_B) + (int32_t)(((uint32_t)v >> (FQ_B - 1)) & 1u); }
// One carry pass: limbs 0..11 back to balanced digits plus the lower neighbour's carry, the top limb absorbs its carry-in.
// Any int32 limbs in; out |limb| <= 2^29 + 2 (limbs 0..11).  No chain: every limb looks at its lower neighbour only.
PE_HD void fq_norm(fq& r, const fq& a)
{
    int32_t c[FQ_N], o[FQ_N];
#pragma unroll
    for (int i = 0; i < FQ_N - 1; ++i) {
        o[i] = fq_digit32(a.l[i]);
        c[i] = fq_carry32(a.l[i]);
    }
#pragma unroll
    for (int i = 1; i < FQ_N - 1; ++i) o[i] += c[i - 1];
    o[FQ_N - 1] = a.l[FQ_N - 1] + c[FQ_N - 2];
#pragma unroll
    for (int i = 0; i < FQ_N; ++i) r.l[i] = o[i];
}
// r = a + b, r = a - b, r = a - b - 2c, each with one carry pass: the shapes the XYZZ formulas need.  Limb sums must stay in
// int32: a + b and a - b of two normed or product values (|limb| <= 2^29 + 2) do; a - b - 2c is for three PRODUCT
// outputs, whose limbs are exact digits in [-2^29, 2^29): the sum lies in [-2^31 + 3, 2^31 - 1].
PE_HD void fq_add(fq& r, const fq& a, const fq& b)
{
    fq t;
#pragma unroll
    for (int i = 0; i < FQ_N; ++i) t.l[i] = a.l[i] + b.l[i];
    fq_norm(r, t);
}
PE_HD void fq_sub_norm(fq& r, const fq& a, const fq& b)
{
    fq t;
    fq_sub(t, a, b);
    fq_norm(r, t);
}
PE_HD void fq_sub_sub2_norm(fq& r, const fq& a, const fq& b, const fq& c)  // a - b - 2c, a, b, c products
{
    fq t;
#pragma unroll
    for (int i = 0; i < FQ_N; ++i) t.l[i] = a.l[i] - b.l[i] - 2 * c.l[i];
    fq_norm(r, t);
}

// r = a b / R mod p in lazy form: (a b + m p) / 2^390 with m = sum m_k 2^(30 k), m_k in [-2^29, 2^29), i.e.
// r in (a b / R - (p/2)(1 + 2^-29), a b / R + (p/2)(1 + 2^-29)).
// Operands: limbs 0..11 |l| <= 2^29 + 16, top limb |l| <= 2^24.  Output: limbs 0..11 exact digits in [-2^29, 2^29), the top
// limb |l| < 2^21 for outputs within +-0.6 p.
PE_HD void fq_mul(fq& r, const fq& a, const fq& b)
{
    int32_t m[FQ_N];
    PE_FQ30_ACC acc = 0;
#pragma unroll
    for (int k = 0; k < FQ_N; ++k) {
#pragma unroll
        for (int i = 0; i <= k; ++i) acc += (int64_t)a.l[i] * b.l[k - i];
#pragma unroll
        for (int i = 0; i < k; ++i) acc += (int64_t)m[i] * FQ_P[k - i];
        m[k] = fq_digit32((int32_t)((uint32_t)(int64_t)acc * FQ_N0INV));
        acc += (int64_t)m[k] * FQ_P[0];
        acc >>= FQ_B;  // exact: the low 30 bits are zero now
    }
#pragma unroll
    for (int k = FQ_N; k < 2 * FQ_N - 1; ++k) {
#pragma unroll
        for (int i = k - (FQ_N - 1); i < FQ_N; ++i) acc += (int64_t)a.l[i] * b.l[k - i];
#pragma unroll
        for (int i = k - (FQ_N - 1); i < FQ_N; ++i) acc += (int64_t)m[i] * FQ_P[k - i];
        r.l[k - FQ_N] = fq_digit((int64_t)acc);
        acc += int64_t(1) << (FQ_B - 1);
        acc >>= FQ_B;  // = (acc - digit) / 2^30: round to nearest
    }
    r.l[FQ_N - 1] = (int32_t)(int64_t)acc;
}
// r = a^2 / R: the cross products once, against the doubled operand (|2 a_i a_j| <= 2^59 + small: column 12 holds five of
// them, one square, 12 full m p terms and small ones -- the product's bound).  Same operand and output bounds as fq_mul.
PE_HD void fq_sqr(fq& r, const fq& a)
{
    int32_t m[FQ_N], d[FQ_N];
#pragma unroll
    for (int i = 0; i < FQ_N; ++i) d[i] = 2 * a.l[i];
    PE_FQ30_ACC acc = 0;
#pragma unroll
    for (int k = 0; k < FQ_N; ++k) {
#pragma unroll
        for (int i = 0; 2 * i < k; ++i) acc += (int64_t)d[i] * a.l[k - i];
        if ((k & 1) == 0) acc += (int64_t)a.l[k / 2] * a.l[k / 2];
#pragma unroll
        for (int i = 0; i < k; ++i) acc += (int64_t)m[i] * FQ_P[k - i];
        m[k] = fq_digit32((int32_t)((uint32_t)(int64_t)acc * FQ_N0INV));
        acc += (int64_t)m[k] * FQ_P[0];
        acc >>= FQ_B;
    }
#pragma unroll
    for (int k = FQ_N; k < 2 * FQ_N - 1; ++k) {
#pragma unroll
        for (int i = k - (FQ_N - 1); 2 * i < k; ++i) acc += (int64_t)d[i] * a.l[k - i];
        if ((k & 1) == 0) acc += (int64_t)a.l[k / 2] * a.l[k / 2];
#pragma unroll
        for (int i = k - (FQ_N - 1); i < FQ_N; ++i) acc += (int64_t)m[i] * FQ_P[k - i];
        r.l[k - FQ_N] = fq_digit((int64_t)acc);
        acc += int64_t(1) << (FQ_B - 1);
        acc >>= FQ_B;
    }
    r.l[FQ_N - 1] = (int32_t)(int64_t)acc;
}

// ---- exact, slow: canonical limbs and comparisons mod p (rare paths and the hand-over to the 12 x 32 form) ----
// Full carry propagation: limbs 0..11 in [0, 2^30), the top limb signed -- the unique such representation of the value.
// Input limbs |l| <= 2^30 + 8.
PE_HD void fq_carry(fq& r, const fq& a)
{
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < FQ_N - 1; ++i) {
        const int32_t v = a.l[i] + c;
        r.l[i] = v & FQ_MASK;
        c = v >> FQ_B;
    }
    r.l[FQ_N - 1] = a.l[FQ_N - 1] + c;
}
// Full carry propagation to balanced digits: limbs 0..11 in [-2^29, 2^29), the top limb signed (what the registry table
// stores).  Input limbs |l| <= 2^30 + 8.
PE_HD void fq_balance(fq& r, const fq& a)
{
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < FQ_N - 1; ++i) {
        const int32_t v = a.l[i] + c;
        r.l[i] = fq_digit32(v);
        c = fq_carry32(v);
    }
    r.l[FQ_N - 1] = a.l[FQ_N - 1] + c;
}
PE_HD bool fq_eq_limbs(const fq& a, const int32_t* b)
{
    int32_t o = 0;
#pragma unroll
    for (int i = 0; i < FQ_N; ++i) o |= a.l[i] ^ b[i];
    return o == 0;
}
// value == 0 mod p, for a value in [FQ_KP_LO p, (FQ_KP_LO + FQ_KP_N) p) = [-8 p, 9 p) (everything the formulas compare
// lies within +-3 p: a product within 0.53 p, X3 within 2.2 p, their differences).  The filter first: value = k p  =>
// k = value p^-1 (mod 2^30), and the value's low 30 bits are limb 0's: one multiply says whether k is one of the 17 small
// multiples possible.
PE_HD bool fq_maybe_zero_modp(const fq& a)
{
    const uint32_t k = (0u - (uint32_t)a.l[0] * FQ_N0INV) & (uint32_t)FQ_MASK;  // FQ_N0INV = -p^-1
    return ((k - (uint32_t)FQ_KP_LO) & (uint32_t)FQ_MASK) < (uint32_t)FQ_KP_N;
}
PE_HD bool fq_is_zero_modp_exact(const fq& a)
{
    fq c;
    fq_carry(c, a);
    bool hit = false;
    for (int k = 0; k < FQ_KP_N; ++k) hit = hit || fq_eq_limbs(c, FQ_KP + FQ_N * k);
    return hit;
}
PE_HD bool fq_is_zero_modp(const fq& a) { return fq_maybe_zero_modp(a) && fq_is_zero_modp_exact(a); }

// The unique representative in [0, p) with carried limbs (0..11 in [0, 2^30)).  fq_canonical: any value in [-8 p, 9 p);
// fq_canonical_near: a value in (-p, 2 p) -- what a product gives -- in three carry chains.
PE_HD void fq_canonical(fq& r, const fq& a)
{
    fq c, t, u;
    fq_carry(c, a);
    for (int round = 0; round < 9 && c.l[FQ_N - 1] < 0; ++round) {  // negative: add p until it is not
#pragma unroll
        for (int i = 0; i < FQ_N; ++i) t.l[i] = c.l[i] + FQ_P_CARRIED[i];
        fq_carry(c, t);
    }
    for (int round = 0; round < 9; ++round) {  // subtract p while the result stays non-negative
#pragma unroll
        for (int i = 0; i < FQ_N; ++i) t.l[i] = c.l[i] - FQ_P_CARRIED[i];
        fq_carry(u, t);
        if (u.l[FQ_N - 1] < 0) break;  // went below zero: c is the representative
        c = u;
    }
    r = c;
}
PE_HD void fq_canonical_near(fq& r, const fq& a)
{
    fq c, t, lo, hi;
    fq_carry(c, a);
#pragma unroll
    for (int i = 0; i < FQ_N; ++i) t.l[i] = c.l[i] + FQ_P_CARRIED[i];
    fq_carry(lo, t);  // value + p: the answer when the value is negative
#pragma unroll
    for (int i = 0; i < FQ_N; ++i) t.l[i] = c.l[i] - FQ_P_CARRIED[i];
    fq_carry(hi, t);  // value - p: the answer when that is not negative
    const bool neg = c.l[FQ_N - 1] < 0, big = hi.l[FQ_N - 1] >= 0;
#pragma unroll
    for (int i = 0; i < FQ_N; ++i) r.l[i] = neg ? lo.l[i] : big ? hi.l[i] : c.l[i];
}

// ---- hand-over to / from the 12 x 32-bit Montgomery form of fp381.h (R32 = 2^384, canonical) ----
// words[12] (little-endian 32-bit limbs of a value < 2^384) -> carried 30-bit limbs of the same integer
PE_HD void fq_from_words32(fq& r, const uint32_t* w)
{
#pragma unroll
    for (int i = 0; i < FQ_N; ++i) {
        const int bit = FQ_B * i, lo = bit >> 5, sh = bit & 31;
        uint64_t v = lo < 12 ? (uint64_t)w[lo] : 0u;
        if (lo + 1 < 12) v |= (uint64_t)w[lo + 1] << 32;
        r.l[i] = (int32_t)((uint32_t)(v >> sh) & (uint32_t)FQ_MASK);
    }
}
// carried limbs of a value in [0, 2^384) -> words[12]
PE_HD void fq_to_words32(uint32_t* w, const fq& a)
{
#pragma unroll
    for (int j = 0; j < 12; ++j) w[j] = 0;
#pragma unroll
    for (int i = 0; i < FQ_N; ++i) {
        const int bit = FQ_B * i, lo = bit >> 5, sh = bit & 31;
        const uint64_t v = (uint64_t)(uint32_t)a.l[i] << sh;
        if (lo < 12) w[lo] |= (uint32_t)v;
        if (lo + 1 < 12) w[lo + 1] |= (uint32_t)(v >> 32);
    }
}
// x 2^384 mod p (words, canonical) -> x R mod p in [0, p) as BALANCED digits: what the registry table of this form stores
PE_HD void fq_from_mont32(fq& r, const uint32_t* w)
{
    fq a, an, k, t, c;
    fq_from_words32(a, w);
    fq_norm(an, a);  // carried limbs (up to 2^30 - 1) are no product operands
#pragma unroll
    for (int i = 0; i < FQ_N; ++i) k.l[i] = FQ_FROM_R32[i];
    fq_mul(t, an, k);
    fq_canonical_near(c, t);
    fq_balance(r, c);
}
// x R (lazy, a product operand) -> x 2^384 mod p, canonical words: what k_g1_finish reads
PE_HD void fq_to_mont32(uint32_t* w, const fq& a)
{
    fq k, t, c;
#pragma unroll
    for (int i = 0; i < FQ_N; ++i) k.l[i] = FQ_TO_R32[i];
    fq_mul(t, a, k);
    fq_canonical_near(c, t);
    fq_to_words32(w, c);
}

}  // namespace s30
}  // namespace posevo
