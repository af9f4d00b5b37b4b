// Host build of the S30 field / G1 code (pos_evolution_amd/csrc/fp381_s30.h, g1_s30.h) behind a C interface, for
// tests/test_host_fp30.py:  g++ -O2 -shared -fPIC tests/native/fp30_host.cpp -o <tmp>/libfp30.so
// The SAME source the gfx950 kernels compile; no GPU involved.
// -DFP30_COLUMN_CHECK: the products' column accumulator becomes a 128-bit integer that records every value it takes; a value
// outside the int64 range (where the device's 64-bit accumulator would wrap) is counted (fq30_column_report).
#include <string.h>

#include <stdint.h>

#ifdef FP30_COLUMN_CHECK
namespace fp30_check {
static long long n_overflow = 0;
static __int128 worst = 0;
struct acc128 {
    __int128 v;
    acc128(int64_t x = 0) : v(x) {}
    void note()
    {
        const __int128 a = v < 0 ? -v : v;
        if (a > worst) worst = a;
        if (v > (__int128)INT64_MAX || v < (__int128)INT64_MIN) ++n_overflow;
    }
    acc128& operator+=(int64_t x) { v += x; note(); return *this; }
    acc128& operator>>=(int s) { v >>= s; return *this; }
    explicit operator int64_t() const { return (int64_t)v; }
};
}  // namespace fp30_check
#define PE_FQ30_ACC fp30_check::acc128
#endif

#include "../../pos_evolution_amd/csrc/g1_s30.h"

using namespace posevo::s30;

extern "C" {

// overflows seen so far, and log2 of the largest |column value| (as a double) since the last reset
long long fq30_column_report(double* worst_log2, int reset)
{
#ifdef FP30_COLUMN_CHECK
    double w = 0;
    __int128 v = fp30_check::worst;
    while (v > 1) { v >>= 1; w += 1; }
    *worst_log2 = w;
    const long long n = fp30_check::n_overflow;
    if (reset) { fp30_check::n_overflow = 0; fp30_check::worst = 0; }
    return n;
#else
    (void)reset;
    *worst_log2 = -1;
    return -1;
#endif
}

void fq30_mul(const int32_t* a, const int32_t* b, int32_t* r)
{
    fq x, y, z;
    memcpy(x.l, a, sizeof(x.l));
    memcpy(y.l, b, sizeof(y.l));
    fq_mul(z, x, y);
    memcpy(r, z.l, sizeof(z.l));
}
void fq30_sqr(const int32_t* a, int32_t* r)
{
    fq x, z;
    memcpy(x.l, a, sizeof(x.l));
    fq_sqr(z, x);
    memcpy(r, z.l, sizeof(z.l));
}
void fq30_norm(const int32_t* a, int32_t* r)
{
    fq x, z;
    memcpy(x.l, a, sizeof(x.l));
    fq_norm(z, x);
    memcpy(r, z.l, sizeof(z.l));
}
// shape 0: a - b, 1: a - b - 2c, 2: a + b (one carry pass each)
void fq30_combine(const int32_t* a, const int32_t* b, const int32_t* c, int shape, int32_t* r)
{
    fq x, y, w, z;
    memcpy(x.l, a, sizeof(x.l));
    memcpy(y.l, b, sizeof(y.l));
    memcpy(w.l, c, sizeof(w.l));
    if (shape == 0) fq_sub_norm(z, x, y);
    else if (shape == 1) fq_sub_sub2_norm(z, x, y, w);
    else fq_add(z, x, y);
    memcpy(r, z.l, sizeof(z.l));
}
void fq30_canonical(const int32_t* a, int32_t* r, int near)
{
    fq x, z;
    memcpy(x.l, a, sizeof(x.l));
    if (near) fq_canonical_near(z, x);
    else fq_canonical(z, x);
    memcpy(r, z.l, sizeof(z.l));
}
int fq30_is_zero_modp(const int32_t* a, int* filter)
{
    fq x;
    memcpy(x.l, a, sizeof(x.l));
    *filter = fq_maybe_zero_modp(x) ? 1 : 0;
    return fq_is_zero_modp(x) ? 1 : 0;
}
void fq30_from_mont32(const uint32_t* w12, int32_t* r)
{
    fq z;
    fq_from_mont32(z, w12);
    memcpy(r, z.l, sizeof(z.l));
}
void fq30_to_mont32(const int32_t* a, uint32_t* w12)
{
    fq x;
    memcpy(x.l, a, sizeof(x.l));
    fq_to_mont32(w12, x);
}
void fq30_words(const uint32_t* w12, int32_t* r, uint32_t* back)
{
    fq z;
    fq_from_words32(z, w12);
    memcpy(r, z.l, sizeof(z.l));
    fq_to_words32(back, z);
}

static void track(const g1q& a, int32_t& worst_limb, int32_t& worst_top)
{
    const fq* cs[4] = {&a.x, &a.y, &a.zz, &a.zzz};
    for (const fq* c : cs) {
        for (int i = 0; i < FQ_N - 1; ++i) {
            const int32_t v = c->l[i] < 0 ? -c->l[i] : c->l[i];
            if (v > worst_limb) worst_limb = v;
        }
        const int32_t t = c->l[FQ_N - 1] < 0 ? -c->l[FQ_N - 1] : c->l[FQ_N - 1];
        if (t > worst_top) worst_top = t;
    }
}
static bool row_of(const uint32_t* row, fq& qx, fq& qy)
{
    uint32_t any = 0;
    for (int k = 0; k < 24; ++k) any |= row[k];
    fq_from_mont32(qx, row);
    fq_from_mont32(qy, row + 12);
    return any != 0;
}

// One lane's run: n registry rows (x, y as 12-word Montgomery values of the 32-bit form, all zero = no point) added into an
// empty accumulator in order with the complete mixed add; out = the 48 XYZZ words.  worst[0] / worst[1] receive the largest
// |limb| (limbs 0..11) / |top limb| any accumulator coordinate held between adds: the bounds the products rely on.
void g1q30_run(const uint32_t* rows24, int n, uint32_t* out48, int32_t* worst)
{
    g1q acc;
    g1q_set_inf(acc);
    int32_t wl = 0, wt = 0;
    for (int j = 0; j < n; ++j) {
        fq qx, qy;
        const bool any = row_of(rows24 + 24 * j, qx, qy);
        g1q_add_affine(acc, qx, qy, !any);
        track(acc, wl, wt);
    }
    if (worst) { worst[0] = wl; worst[1] = wt; }
    g1q_to_words32(out48, acc);
}

// The same run the way k_g1_accumulate does it: first point as the accumulator (g1q_set_first), every later one through the
// general body alone (g1q_madd_fast); a same-x case only raises the flag and the run is then redone by the complete add.
void g1q30_run_kernel_way(const uint32_t* rows24, int n, uint32_t* out48, int32_t* worst, int* took_slow_path)
{
    g1q acc;
    g1q_set_inf(acc);
    bool exc = false;
    int32_t wl = 0, wt = 0;
    for (int j = 0; j < n; ++j) {
        fq qx, qy;
        if (!row_of(rows24 + 24 * j, qx, qy)) continue;
        if (acc.inf) g1q_set_first(acc, qx, qy);
        else g1q_madd_fast(acc, qx, qy, exc);
        if (exc) break;  // the kernel's lane goes on over garbage; nothing of it is used
        track(acc, wl, wt);
    }
    *took_slow_path = exc ? 1 : 0;
    if (worst) { worst[0] = wl; worst[1] = wt; }
    if (exc) {
        g1q30_run(rows24, n, out48, nullptr);
        return;
    }
    g1q_to_words32(out48, acc);
}

// k_g1_accumulate + k_g1_tree at the level of their formulas: lanes of k rows each accumulate the kernel's way, and the lanes'
// accumulators -- handed over as they are, lazy limbs and all, all limbs zero for infinity -- are reduced pairwise, level by
// level, with the complete add g1q_add.  out = the 48 words k_g1_finish reads.
void g1q30_tree_run(const uint32_t* rows24, int n, int k, uint32_t* out48, int32_t* worst)
{
    const int lanes = (n + k - 1) / k;
    g1q* acc = new g1q[lanes > 0 ? lanes : 1];
    for (int l = 0; l < lanes; ++l) {
        const int cnt = (l + 1) * k <= n ? k : n - l * k;
        g1q a;
        g1q_set_inf(a);
        bool exc = false;
        for (int j = 0; j < cnt; ++j) {
            fq qx, qy;
            if (!row_of(rows24 + 24 * (l * k + j), qx, qy)) continue;
            if (a.inf) g1q_set_first(a, qx, qy);
            else g1q_madd_fast(a, qx, qy, exc);
        }
        if (exc) {  // the kernel's second run of the lane
            g1q_set_inf(a);
            for (int j = 0; j < cnt; ++j) {
                fq qx, qy;
                const bool any = row_of(rows24 + 24 * (l * k + j), qx, qy);
                g1q_add_affine(a, qx, qy, !any);
            }
        }
        if (a.inf) g1q_set_inf(a);  // all limbs zero: what the hand-over writes for an empty lane
        acc[l] = a;
    }
    int32_t wl = 0, wt = 0;
    for (int m = lanes; m > 1; m = (m + 1) / 2) {
        for (int i = 0; i < m / 2; ++i) {
            g1q a = acc[2 * i];
            a.inf = fq_limbs_zero(a.zz);  // the tree learns "infinity" from the limbs, not from a flag
            g1q b = acc[2 * i + 1];
            b.inf = fq_limbs_zero(b.zz);
            a.affine = b.affine = false;
            g1q_add(a, b);
            if (a.inf) g1q_set_inf(a);
            acc[i] = a;
            track(a, wl, wt);
        }
        if (m & 1) acc[m / 2] = acc[m - 1];
    }
    if (worst) { worst[0] = wl; worst[1] = wt; }
    if (lanes == 0) {
        for (int w = 0; w < 48; ++w) out48[w] = 0;
    } else {
        g1q r = acc[0];
        r.inf = fq_limbs_zero(r.zz);
        g1q_to_words32(out48, r);
    }
    delete[] acc;
}

}  // extern "C"
