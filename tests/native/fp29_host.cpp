// Host build of the S29 field / G1 code (pos_evolution_amd/csrc/fp381_s29.h, g1_s29.h) behind a C interface, for
// tests/test_host_fp29.py:  g++ -O2 -shared -fPIC tests/native/fp29_host.cpp -o <tmp>/libfp29.so
// The SAME source hipcc compiles for gfx950: the field form is what the square roots of the decompression kernels run, the
// point formulas (g1_lazy.inc) are what the accumulation and the tree run over S30.  No GPU involved.
#include <string.h>

#include "../../pos_evolution_amd/csrc/g1_s29.h"

using namespace posevo;

extern "C" {

void fq29_mul(const int32_t* a, const int32_t* b, int32_t* r)
{
    fq x, y, z;
    memcpy(x.l, a, sizeof(x.l));
    memcpy(y.l, b, sizeof(y.l));
    fq_mul(z, x, y);
    memcpy(r, z.l, sizeof(z.l));
}
void fq29_sqr(const int32_t* a, int32_t* r)
{
    fq x, z;
    memcpy(x.l, a, sizeof(x.l));
    fq_sqr(z, x);
    memcpy(r, z.l, sizeof(z.l));
}
void fq29_norm(const int32_t* a, int32_t* r)
{
    fq x, z;
    memcpy(x.l, a, sizeof(x.l));
    fq_norm(z, x);
    memcpy(r, z.l, sizeof(z.l));
}
void fq29_canonical(const int32_t* a, int32_t* r, int near)
{
    fq x, z;
    memcpy(x.l, a, sizeof(x.l));
    if (near) fq_canonical_near(z, x);
    else fq_canonical(z, x);
    memcpy(r, z.l, sizeof(z.l));
}
int fq29_is_zero_modp(const int32_t* a, int* filter)
{
    fq x;
    memcpy(x.l, a, sizeof(x.l));
    *filter = fq_maybe_zero_modp(x) ? 1 : 0;
    return fq_is_zero_modp(x) ? 1 : 0;
}
void fq29_from_mont32(const uint32_t* w12, int32_t* r)
{
    fq z;
    fq_from_mont32(z, w12);
    memcpy(r, z.l, sizeof(z.l));
}
void fq29_to_mont32(const int32_t* a, uint32_t* w12)
{
    fq x;
    memcpy(x.l, a, sizeof(x.l));
    fq_to_mont32(w12, x);
}
void fq29_words(const uint32_t* w12, int32_t* r, uint32_t* back)
{
    fq z;
    fq_from_words32(z, w12);
    memcpy(r, z.l, sizeof(z.l));
    fq_to_words32(back, z);
}

}  // extern "C"

#include "g1q_runs.inc"

extern "C" {

// The runs of g1q_runs.inc.  max_abs_limb (optional) receives the largest |limb| (the top limb apart) they report.
void g1q_run(const uint32_t* rows24, int n, uint32_t* out48, int32_t* max_abs_limb)
{
    int32_t worst[2];
    lane_run(rows24, n, out48, worst);
    if (max_abs_limb) *max_abs_limb = worst[0];
}
void g1q_run_kernel_way(const uint32_t* rows24, int n, uint32_t* out48, int32_t* max_abs_limb, int* took_slow_path)
{
    int32_t worst[2];
    lane_run_kernel_way(rows24, n, out48, worst, took_slow_path);
    if (max_abs_limb) *max_abs_limb = worst[0];
}
void g1q_tree_run(const uint32_t* rows24, int n, int k, uint32_t* out48, int32_t* max_abs_limb)
{
    int32_t worst[2];
    tree_run(rows24, n, k, out48, worst);
    if (max_abs_limb) *max_abs_limb = worst[0];
}

// fp_sqrt.h's fp_pow_pm3d4 as the decompression kernels run it: Montgomery words (R = 2^384) in and out
void fq29_pow_pm3d4_words(const uint32_t* in12, uint32_t* out12, int32_t* max_abs_limb)
{
    fq x, r;
    fq_from_mont32(x, in12);
    fq_pow_pm3d4(r, x);
    int32_t worst = 0;
    for (int i = 0; i < FQ_N - 1; ++i) {
        const int32_t v = r.l[i] < 0 ? -r.l[i] : r.l[i];
        if (v > worst) worst = v;
    }
    if (max_abs_limb) *max_abs_limb = worst;
    fq_to_mont32(out12, r);
}

}  // extern "C"
