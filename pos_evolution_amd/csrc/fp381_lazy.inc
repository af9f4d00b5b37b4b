// fp381_lazy.inc -- the BLS12-381 base field in FQ_N signed limbs of B = FQ_B bits, lazy Montgomery with R = 2^(B FQ_N),
// written once for both lazy forms.  Included inside the form's namespace by fp381_s29.h (B = 29, FQ_N = 14, namespace
// posevo) and fp381_s30.h (B = 30, FQ_N = 13, namespace posevo::s30): no include guard, no namespace of its own, like
// g1_lazy.inc, the point formulas over it.  Host + device, plain C++: tests/test_host_fp29.py and tests/test_host_fp30.py run
// this text on the CPU against Python integers, the gfx950 kernels compile it in both forms.
//
// The bounds below are in terms of B; what they come to in numbers -- which column is the widest and how close to 2^63 it
// gets, what may feed a product -- is argued in each form header, because it differs.  Before it includes this file the
// form header defines FQ_B, FQ_N, FQ_MASK, its constants (FQ_N0INV, FQ_P, FQ_ONE, FQ_TO_R32, FQ_FROM_R32, FQ_KP_LO,
// FQ_KP_N, FQ_KP) and the four places where the forms differ:
//   fq_acc                     the products' column accumulator: a signed 64-bit integer, or a type that checks one.  Used
//                              only as  fq_acc acc = 0;  acc += int64;  acc >>= n;  (int64_t)acc;
//   fq_mont_digit(v)           the Montgomery digit of v = (uint32_t)acc * FQ_N0INV: v mod 2^B, in [0, 2^B) or balanced;
//   fq_norm_carry(v, digit)    the carry of fq_norm: (v - digit) / 2^B for digit = fq_digit32(v);
//   fq_p_carried(i)            limb i of p with limbs 0..FQ_N-2 in [0, 2^B): what the exact reductions add and subtract.

struct fq {
    int32_t l[FQ_N];  // value = sum l[i] 2^(B i); limbs 0..FQ_N-2 nominally balanced digits, the top limb the rest
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
PE_HD bool fq_limbs_zero(const fq& a)  // all limbs zero (the table's encoding of "no point"); NOT a test mod p
{
    int32_t o = 0;
#pragma unroll
    for (int i = 0; i < FQ_N; ++i) o |= a.l[i];
    return o == 0;
}

// r = a - b, limb by limb.  |limbs| add up: two balanced operands (|limb| <= 2^(B-1) + c) give |limb| <= 2^B + 2c.  Whether
// that may feed a product is the form's matter (fq_sub_operand in g1_s29.h / g1_s30.h).
PE_HD void fq_sub(fq& r, const fq& a, const fq& b)
{
#pragma unroll
    for (int i = 0; i < FQ_N; ++i) r.l[i] = a.l[i] - b.l[i];
}
// The balanced digit of a value: its low B bits read as a signed number in [-2^(B-1), 2^(B-1)).  Balanced on purpose: a limb
// the compiler can prove non-negative turns the next product's sign extension into a zero extension, and a signed x unsigned
// 32 x 32 -> 64 multiply is TWO v_mad_u64_u32 plus fix-ups on gfx950 where signed x signed is one v_mad_i64_i32.
PE_HD int32_t fq_digit(int64_t v) { return (int32_t)((uint32_t)v << (32 - FQ_B)) >> (32 - FQ_B); }
PE_HD int32_t fq_digit32(int32_t v) { return (int32_t)((uint32_t)v << (32 - FQ_B)) >> (32 - FQ_B); }
// One carry pass: limbs 0..FQ_N-2 back to balanced digits plus the lower neighbour's carry, the top limb absorbs its
// carry-in.  No chain: every limb looks at its lower neighbour only.  Which limbs may come in, and how small the carries
// are: at the form's fq_norm_carry.
PE_HD void fq_norm(fq& r, const fq& a)
{
    int32_t c[FQ_N], o[FQ_N];
#pragma unroll
    for (int i = 0; i < FQ_N - 1; ++i) {
        o[i] = fq_digit32(a.l[i]);
        c[i] = fq_norm_carry(a.l[i], o[i]);
    }
#pragma unroll
    for (int i = 1; i < FQ_N - 1; ++i) o[i] += c[i - 1];
    o[FQ_N - 1] = a.l[FQ_N - 1] + c[FQ_N - 2];
#pragma unroll
    for (int i = 0; i < FQ_N; ++i) r.l[i] = o[i];
}
// r = a + b, r = a - b, r = a - b - 2c, each with one carry pass: the shapes the XYZZ formulas need.  The limb sums must
// stay inside what the form's fq_norm takes.
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
PE_HD void fq_sub_sub2_norm(fq& r, const fq& a, const fq& b, const fq& c)  // a - b - 2c
{
    fq t;
#pragma unroll
    for (int i = 0; i < FQ_N; ++i) t.l[i] = a.l[i] - b.l[i] - 2 * c.l[i];
    fq_norm(r, t);
}

// r = a b / R mod p in lazy form: (a b + m p) / R with m = sum m_k 2^(B k), m_k = fq_mont_digit(..), so that
// r - a b / R = m p / R: in (0, p) for digits in [0, 2^B), within (p/2)(1 + 2^(1-B)) of zero for balanced ones.
// Interleaved (FIPS): column k sums the a_i b_j and m_i p_j with i + j = k, up to 2 FQ_N terms, in ONE signed 64-bit
// accumulator -- the operand bounds under which no column leaves it are the form header's.
// Output: limbs 0..FQ_N-2 exact balanced digits in [-2^(B-1), 2^(B-1)), the top limb the (small) rest.
PE_HD void fq_mul(fq& r, const fq& a, const fq& b)
{
    int32_t m[FQ_N];
    fq_acc acc = 0;
#pragma unroll
    for (int k = 0; k < FQ_N; ++k) {
#pragma unroll
        for (int i = 0; i <= k; ++i) acc += (int64_t)a.l[i] * b.l[k - i];
#pragma unroll
        for (int i = 0; i < k; ++i) acc += (int64_t)m[i] * FQ_P[k - i];
        m[k] = fq_mont_digit((uint32_t)(int64_t)acc * FQ_N0INV);
        acc += (int64_t)m[k] * FQ_P[0];
        acc >>= FQ_B;  // exact: the low B bits are zero now
    }
#pragma unroll
    for (int k = FQ_N; k < 2 * FQ_N - 1; ++k) {
#pragma unroll
        for (int i = k - (FQ_N - 1); i < FQ_N; ++i) acc += (int64_t)a.l[i] * b.l[k - i];
#pragma unroll
        for (int i = k - (FQ_N - 1); i < FQ_N; ++i) acc += (int64_t)m[i] * FQ_P[k - i];
        r.l[k - FQ_N] = fq_digit((int64_t)acc);
        acc += int64_t(1) << (FQ_B - 1);
        acc >>= FQ_B;  // = (acc - digit) / 2^B: round to nearest
    }
    r.l[FQ_N - 1] = (int32_t)(int64_t)acc;
}
// r = a^2 / R: the cross products once, against the doubled operand (|2 a_i a_j| is twice a product term: a column holds
// half as many of them, and one square).  Same operand and output bounds as fq_mul.
PE_HD void fq_sqr(fq& r, const fq& a)
{
    int32_t m[FQ_N], d[FQ_N];
#pragma unroll
    for (int i = 0; i < FQ_N; ++i) d[i] = 2 * a.l[i];
    fq_acc acc = 0;
#pragma unroll
    for (int k = 0; k < FQ_N; ++k) {
#pragma unroll
        for (int i = 0; 2 * i < k; ++i) acc += (int64_t)d[i] * a.l[k - i];
        if ((k & 1) == 0) acc += (int64_t)a.l[k / 2] * a.l[k / 2];
#pragma unroll
        for (int i = 0; i < k; ++i) acc += (int64_t)m[i] * FQ_P[k - i];
        m[k] = fq_mont_digit((uint32_t)(int64_t)acc * FQ_N0INV);
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

// ---- exact, slow: carried limbs and comparisons mod p (rare paths and the hand-over to the 12 x 32 form) ----
// Full carry propagation: limbs 0..FQ_N-2 in [0, 2^B), the top limb signed -- the unique such representation of the
// value ("carried", "canonical limbs").  Input limbs |l| <= 2^B + 8.
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
PE_HD bool fq_eq_limbs(const fq& a, const int32_t* b)
{
    int32_t o = 0;
#pragma unroll
    for (int i = 0; i < FQ_N; ++i) o |= a.l[i] ^ b[i];
    return o == 0;
}
// value == 0 mod p, for a value in [FQ_KP_LO p, (FQ_KP_LO + FQ_KP_N) p) (how far inside the formulas' values lie: the form
// header).  The filter first: value = k p  =>  k = value p^-1 (mod 2^B), and the value's low B bits are limb 0's (every
// other limb weighs a multiple of 2^B): one multiply says whether k is one of the FQ_KP_N small multiples possible.
PE_HD bool fq_maybe_zero_modp(const fq& a)
{
    const uint32_t k = (0u - (uint32_t)a.l[0] * FQ_N0INV) & (uint32_t)FQ_MASK;  // FQ_N0INV = -p^-1
    return ((k - (uint32_t)FQ_KP_LO) & (uint32_t)FQ_MASK) < (uint32_t)FQ_KP_N;
}
PE_HD bool fq_is_zero_modp_exact(const fq& a)  // against FQ_KP: the carried limbs of those multiples
{
    fq c;
    fq_carry(c, a);
    bool hit = false;
    for (int k = 0; k < FQ_KP_N; ++k) hit = hit || fq_eq_limbs(c, FQ_KP + FQ_N * k);
    return hit;
}
PE_HD bool fq_is_zero_modp(const fq& a) { return fq_maybe_zero_modp(a) && fq_is_zero_modp_exact(a); }

// The unique representative in [0, p) with carried limbs.  fq_canonical: any value in [-8 p, 9 p); fq_canonical_near:
// a value in (-p, 2 p) -- what a product gives -- in three carry chains.
PE_HD void fq_canonical(fq& r, const fq& a)
{
    fq c, t, u;
    fq_carry(c, a);
    for (int round = 0; round < 9 && c.l[FQ_N - 1] < 0; ++round) {  // negative: add p until it is not
#pragma unroll
        for (int i = 0; i < FQ_N; ++i) t.l[i] = c.l[i] + fq_p_carried(i);
        fq_carry(c, t);
    }
    for (int round = 0; round < 9; ++round) {  // subtract p while the result stays non-negative
#pragma unroll
        for (int i = 0; i < FQ_N; ++i) t.l[i] = c.l[i] - fq_p_carried(i);
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
    for (int i = 0; i < FQ_N; ++i) t.l[i] = c.l[i] + fq_p_carried(i);
    fq_carry(lo, t);  // value + p: the answer when the value is negative
#pragma unroll
    for (int i = 0; i < FQ_N; ++i) t.l[i] = c.l[i] - fq_p_carried(i);
    fq_carry(hi, t);  // value - p: the answer when that is not negative
    const bool neg = c.l[FQ_N - 1] < 0, big = hi.l[FQ_N - 1] >= 0;
#pragma unroll
    for (int i = 0; i < FQ_N; ++i) r.l[i] = neg ? lo.l[i] : big ? hi.l[i] : c.l[i];
}

// ---- hand-over to / from the 12 x 32-bit Montgomery form of fp381.h (R32 = 2^384, canonical) ----
// words[12] (little-endian 32-bit limbs of a value < 2^384) -> carried B-bit limbs of the same integer
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
// x R (lazy, a product operand) -> x 2^384 mod p, canonical words: what k_g1_finish reads.  (The way in, fq_from_mont32,
// is the form's: the table of each form stores its rows differently.)
PE_HD void fq_to_mont32(uint32_t* w, const fq& a)
{
    fq k, t, c;
#pragma unroll
    for (int i = 0; i < FQ_N; ++i) k.l[i] = FQ_TO_R32[i];
    fq_mul(t, a, k);
    fq_canonical_near(c, t);
    fq_to_words32(w, c);
}
