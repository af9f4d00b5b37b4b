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
// The arithmetic itself is fp381_lazy.inc, one text for this form and S29; this header holds what is S30's own: the bounds
// above, the form's numbers, the four places where the forms differ, and the balanced registry rows.
//
// Names live in posevo::s30 so that this form and S29 (which sits in posevo itself, and which the square roots keep) can
// share a translation unit.  Host + device, plain C++, like fp381_s29.h; the point formulas over it: g1_s30.h (g1_lazy.inc).
#pragma once
#include <stdint.h>

#include "pe_hd.h"

// The column accumulator of the products.  A host test build may define it as a checked 128-bit type (tests/native/fp30_host.cpp);
// fp381_lazy.inc uses only  T acc = 0;  acc += int64;  acc >>= n;  (int64_t)acc.
#ifndef PE_FQ30_ACC
#define PE_FQ30_ACC int64_t
#endif

namespace posevo {
namespace s30 {

constexpr int FQ_B = 30, FQ_N = 13;
constexpr int32_t FQ_MASK = (1 << FQ_B) - 1;

#include "fp381_s30_consts.inc"

// ---- what fp381_lazy.inc computes, in this form's numbers ----
// fq: limbs 0..11 nominally balanced digits in [-2^29, 2^29), the top limb the rest.
// fq_sub: NOT a product operand (|limb| up to 2^30 + 4): the same-x filter reads it, and a carry pass makes one of it
//   (fq_sub_norm).
// fq_norm: any int32 limbs in; out |limb| <= 2^29 + 2 (limbs 0..11).
// fq_add, fq_sub_norm, fq_sub_sub2_norm: the limb sums must stay in int32.  a + b and a - b of two normed or product values
//   (|limb| <= 2^29 + 2) do; a - b - 2c is for three PRODUCT outputs, whose limbs are exact digits in [-2^29, 2^29): the sum
//   lies in [-2^31 + 3, 2^31 - 1].
// fq_mul: r = a b / R mod p, (a b + m p) / 2^390 with m = sum m_k 2^(30 k), m_k in [-2^29, 2^29), i.e.
//   r in (a b / R - (p/2)(1 + 2^-29), a b / R + (p/2)(1 + 2^-29)).  Operands: limbs 0..11 |l| <= 2^29 + 16, top limb
//   |l| <= 2^24 (the column-12 bound above).  Output: limbs 0..11 exact digits in [-2^29, 2^29), the top limb |l| < 2^21 for
//   outputs within +-0.6 p.
// fq_sqr: |2 a_i a_j| <= 2^59 + small: column 12 holds five of them, one square, 12 full m p terms and small ones -- the
//   product's bound.  Same operand and output bounds as fq_mul.
// fq_carry, fq_balance: input limbs |l| <= 2^30 + 8.
// fq_is_zero_modp: a value in [-8 p, 9 p), 17 multiples (everything the formulas compare lies within +-3 p: a product within
//   0.53 p, X3 within 2.2 p, their differences).

// The four places where this form differs from S29 (fp381_lazy.inc says what each is for).
using fq_acc = PE_FQ30_ACC;
PE_HD int32_t fq_digit32(int32_t v);  // fp381_lazy.inc
// Montgomery digits balanced, in [-2^29, 2^29): every factor of a column term is then a balanced digit.
PE_HD int32_t fq_mont_digit(uint32_t v) { return fq_digit32((int32_t)v); }
// The carry that goes with fq_digit32: (v - digit) / 2^30 = floor(v / 2^30) + bit 29, computed without forming v - digit
// (which leaves the int32 range for |v| near 2^31).  In [-2, 2] for any int32 v.
PE_HD int32_t fq_carry32(int32_t v) { return (v >> FQ_B) + (int32_t)(((uint32_t)v >> (FQ_B - 1)) & 1u); }
PE_HD int32_t fq_norm_carry(int32_t v, int32_t) { return fq_carry32(v); }
// FQ_P is in balanced digits for the products; the exact reductions work on carried limbs.
PE_HD int32_t fq_p_carried(int i) { return FQ_P_CARRIED[i]; }

#include "fp381_lazy.inc"

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

}  // namespace s30
}  // namespace posevo
