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

}  // extern "C"

#include "g1q_runs.inc"

extern "C" {

// The runs of g1q_runs.inc; worst[0] / worst[1] (optional): the largest |limb| (limbs 0..11) / |top limb| they report.
void g1q30_run(const uint32_t* rows24, int n, uint32_t* out48, int32_t* worst) { lane_run(rows24, n, out48, worst); }
void g1q30_run_kernel_way(const uint32_t* rows24, int n, uint32_t* out48, int32_t* worst, int* took_slow_path)
{
    lane_run_kernel_way(rows24, n, out48, worst, took_slow_path);
}
void g1q30_tree_run(const uint32_t* rows24, int n, int k, uint32_t* out48, int32_t* worst) { tree_run(rows24, n, k, out48, worst); }

}  // extern "C"
