// fp381_s29.h -- BLS12-381 base field in 14 signed limbs of 29 bits ("S29"), Montgomery constant R' = 2^406.
//
// Why this form next to fp381.h (12 x 32 bits, R = 2^384): half of that product's 689 instructions are carry
// handling -- v_mad_u64_u32 has a carry-out but no carry-in, a full 32 x 32 product plus a 64-bit accumulator overflows,
// every limb product pays a v_addc_co_u32 (288 per product), plus ~65 moves that slide the 96-bit column accumulator and
// the conditional subtraction.  With 29-bit limbs a column of the interleaved (FIPS) Montgomery product -- up to 14
// a_i b_j + 14 m_i n_j terms of <= 2^58 -- fits a signed 64-bit accumulator (28 x 2^58 < 2^63): one v_mad_i64_i32 per
// limb product and nothing else, ~505 instructions per product instead of 689, written in plain C++ (no inline assembly:
// the compiler sees the whole product and the same source compiles for the host, where tests/test_host_fp29.py holds it
// against Python integers).
// The price is 392 multiply-adds per product instead of 288.  Round 3 wrote this form and could not run it; by the
// per-instruction timings of round 1 it predicted a wash (the carry add behind a multiply-add "three quarters hidden").
// Round 4 measured (tools/fpbench29, tools/icbench, tools/accbench): 14 % more dependent products per second,
// 25 % more mixed adds (the squaring is 301 multiply-adds), and the accumulation kernel 158 us against 183 for a million
// points -- a mixed add of 3 738 multiply-adds runs at the multiplier's issue rate, the simple instructions around them are
// free and carries are not.  It was the accumulation's form in rounds 4-6 and the tree's in round 6; since round 7 both compute in
// S30 (fp381_s30.h: 13 balanced limbs of 30 bits, 338 multiply-adds per product).  What remains on S29: the square roots of
// the decompression kernels (fp_sqrt.h, fq_pow_pm3d4 below) and the tools that measure this form (over g1_s29.h, which runs
// the point formulas the kernels run over S30: g1_lazy.inc); finish and the wire formats stay in fp381.h.
//
// Lazy, signed values.  R' / p > 2^25, so a product of operands of magnitude < 2^386 (32 p) comes out in (-eps, p + eps)
// with no final subtraction; a - b is a plain limb-wise subtraction (limbs of both signs are fine in the next product as
// long as |limb| <= 2^29 + small; products and carry passes leave BALANCED digits, |limb| <= 2^28 + small, so one
// subtraction stays inside); sums of three terms pass through ONE carry pass (fq_norm: four instructions per limb, no
// dependency chain).  A value is a residue mod p in redundant form: equality with zero is a filter on the low 29 bits
// against the few multiples of p the value can be, and an exact comparison behind it (fq_is_zero_modp).
//
// The arithmetic itself is fp381_lazy.inc, one text for this form and S30; this header holds what is S29's own: the reasons
// and measurements above, the form's numbers, the four places where the forms differ, and the square root's power.
//
// Replaces (as fp381.h does): the field arithmetic under bls.Aggregate's point additions, reference call sites pe:736,
// pe:976 (the reference holds no BLS arithmetic; oracle/g1.py restates it).
#pragma once
#include <stdint.h>

#include "pe_hd.h"

namespace posevo {

constexpr int FQ_B = 29, FQ_N = 14;
constexpr int32_t FQ_MASK = (1 << FQ_B) - 1;

#include "fp381_s29_consts.inc"

// ---- what fp381_lazy.inc computes, in this form's numbers ----
// fq: limbs 0..12 nominally balanced digits in [-2^28, 2^28), the top limb the rest.
// fq_sub: two balanced operands (|limb| <= 2^28 + c) or two table rows (canonical limbs in [0, 2^29)) give
//   |limb| <= 2^29 + 2c -- what the products accept: a limb-wise difference may feed a product.
// fq_mul: r = a b / R' mod p, (a b + m p) / 2^406 with m in [0, 2^406), i.e. r in (a b / R', a b / R' + p).  Operand limbs
//   |.| <= 2^29 + 16: a column holds up to 14 a_i b_j + 14 m_i p_j terms of <= 2^58 + small, 28 x 2^58 < 2^63.  Output limbs
//   0..12 balanced digits in [-2^28, 2^28), top limb small.
// fq_sqr: |2 a_i a_j| <= 2^59: a column of 7 of them, one square and 14 m p terms stays below 2^63.
// fq_is_zero_modp: a value in [-8 p, 17 p) (FQ_KP_LO, FQ_KP_N = 25); everything the point formulas produce is far inside.

// The four places where this form differs from S30 (fp381_lazy.inc says what each is for).
using fq_acc = int64_t;
// Montgomery digits in [0, 2^29): what keeps a product in (a b / R', a b / R' + p).
PE_HD int32_t fq_mont_digit(uint32_t v) { return (int32_t)(v & (uint32_t)FQ_MASK); }
// fq_norm's carry, exact, through v - digit: the limbs that come in are at most 2^30 + small in magnitude (the three-term
// sums of the formulas), |carry| <= 4 for inputs below 2^31 in magnitude, and v - digit must stay in int32.
PE_HD int32_t fq_norm_carry(int32_t v, int32_t digit) { return (v - digit) >> FQ_B; }
// FQ_P is carried already (limbs 0..12 in [0, 2^29)): the products and the exact reductions read the same array.
PE_HD int32_t fq_p_carried(int i) { return FQ_P[i]; }

#include "fp381_lazy.inc"

// x 2^384 mod p (words, canonical) -> x R' mod p, canonical S29 limbs: what the registry table of this form stores
PE_HD void fq_from_mont32(fq& r, const uint32_t* w)
{
    fq a, k, t;
    fq_from_words32(a, w);
#pragma unroll
    for (int i = 0; i < FQ_N; ++i) k.l[i] = FQ_FROM_R32[i];
    fq_mul(t, a, k);
    fq_canonical_near(r, t);
}

// ---- a^((p-3)/4): the exponentiation under every square root of the decompression kernels (fp_sqrt.h) ----
// One lane per point there: a chain of ~460 dependent products.  This form's column sums are independent multiply-adds: the
// chain runs at the multiplier's issue rate (301 / 392 multiply-adds per squaring / product).
// The exponent is a constant, so the schedule is too (tools/gen_fq_consts.py: sliding windows of at most four bits over the
// ODD powers a, a^3 .. a^15): 375 squarings + 78 products + 8 for the table.  The table is EIGHT values held in registers and
// picked by a wave-uniform selector -- rounds 4-5 indexed a 16-entry table at run time, i.e. kept it in scratch: 1120 bytes per
// lane, 147 MB for a chip full of waves, which the runtime hands out per dispatch (profiles/r06_sig_*: the kernel measured
// 15 ms, the call around it 35-50).  No scratch now.
PE_HD void fq_pick_odd(fq& r, uint32_t v, const fq& t1, const fq& t3, const fq& t5, const fq& t7, const fq& t9, const fq& t11,
                       const fq& t13, const fq& t15)
{
#pragma unroll
    for (int i = 0; i < FQ_N; ++i)
        r.l[i] = v == 1 ? t1.l[i] : v == 3 ? t3.l[i] : v == 5 ? t5.l[i] : v == 7 ? t7.l[i] : v == 9 ? t9.l[i]
               : v == 11 ? t11.l[i] : v == 13 ? t13.l[i] : t15.l[i];
}
PE_HD void fq_pow_pm3d4(fq& w, const fq& a)  // a: limbs as the products accept them (|limb| <= 2^29 + 16), any residue
{
    fq t1, t3, t5, t7, t9, t11, t13, t15, a2;
    fq_norm(t1, a);  // balanced digits: signed x signed multiplies below
    fq_sqr(a2, t1);
    fq_mul(t3, t1, a2);
    fq_mul(t5, t3, a2);
    fq_mul(t7, t5, a2);
    fq_mul(t9, t7, a2);
    fq_mul(t11, t9, a2);
    fq_mul(t13, t11, a2);
    fq_mul(t15, t13, a2);
    fq acc;
    fq_pick_odd(acc, FQ_PM3D4_FIRST, t1, t3, t5, t7, t9, t11, t13, t15);
    constexpr int n_sched = (int)(sizeof(FQ_PM3D4_SW) / sizeof(FQ_PM3D4_SW[0]));
#pragma nounroll
    for (int i = 0; i < n_sched; ++i) {
        const uint32_t e = FQ_PM3D4_SW[i];
        const uint32_t n_sq = e & 0xFFu, v = e >> 8;
#pragma nounroll
        for (uint32_t k = 0; k < n_sq; ++k) fq_sqr(acc, acc);
        if (v) {
            fq m;
            fq_pick_odd(m, v, t1, t3, t5, t7, t9, t11, t13, t15);
            fq_mul(acc, acc, m);
        }
    }
    w = acc;
}

}  // namespace posevo
