// h2c_kernels.hip -- hash_to_curve for G2 on gfx950: message points H(m) from messages (host side: engine_h2c.cpp).
//
// The suite is BLS12381G2_XMD:SHA-256_SSWU_RO_ of RFC 9380; tests/hash_to_curve_model.py is the specification, byte for byte.
//
//   k_h2c_expand   one lane per message: expand_message_xmd with SHA-256 to 256 bytes (b0, then b1 .. b8: 19 compressions for a
//                  32-byte message under a 43-byte DST), the four 512-bit values reduced mod p: (u0, u1) as Montgomery words
//   k_h2c_load_u   pe_map_to_g2's seam: canonical big-endian (u0, u1) to the same words
//   k_h2c_map      one lane PAIR per u, 2n of them: the simplified SWU map onto E' and the 3-isogeny to E2, the point left as XYZZ
//   k_h2c_finish   one lane pair per message: the two points added (the complete add: they may be equal or opposite), the
//                  cofactor cleared by psi, one inversion to affine, the 192-byte wire form
//
// Fp is 12 x 32 Montgomery (fp381.h), Fp2 the lane-pair form of g2.h.  The map's square root is the G2 decompression's
// (f2_sqrt_lane, fp_sqrt.h: both components in ONE lane), and the pair spends its two lanes on it: the lane of c0 tries g(x1) while
// the lane of c1 tries g(x2) -- exactly one of the two is a square (u = 0 apart, where both are and x1 is taken) -- then the pair
// takes x1 if its root exists, else x2.  The isogeny costs no inversion: with d = x - x0,
//     X = (x d^2 + v d + u_Q) / (3 d)^2        Y = -y (d^3 - v d - 2 u_Q) / (3 d)^3
// are the XYZZ coordinates (ZZ = (3 d)^2, ZZZ = (3 d)^3) that g2.h's additions take; d = 0 is the kernel of the isogeny and lands
// on ZZ = 0, the identity.  The SWU map itself inverts once (1 / tv1): sgn0 needs y as a field element, not as a fraction.
// Bound: integer VALU; per message ~2 x 2.2 k Montgomery products per lane in k_h2c_map and ~3.6 k in k_h2c_finish.
#ifndef POSEVO_POW_INLINE
#define POSEVO_POW_INLINE __forceinline__
#endif
#include "g2.h"
#include "fp_sqrt.h"
#include "fp_mem.h"
#include "h2c_expand.h"
#include "kernels.h"

namespace posevo {

static_assert(H2C_POINT_WORDS == G2X_WORDS, "kernels.h restates the size of an XYZZ point");

namespace {
#include "h2c_consts.inc"

__device__ __forceinline__ void h2c_const(fp& r, const uint32_t (&c)[2][12], bool role)
{
#pragma unroll
    for (int j = 0; j < 12; ++j) r.l[j] = c[role ? 1 : 0][j];
}

// 64 uniform bytes (hi | lo, 8 big-endian words each) mod p, as Montgomery words: hi 2^256 + lo, both below 2^256 < p
__device__ __forceinline__ void h2c_reduce(fp& r, const uint32_t (&hi)[8], const uint32_t (&lo)[8])
{
    fp h, l, c, hm, lm, t;
    fp_set_zero(h);
    fp_set_zero(l);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        h.l[j] = hi[7 - j];
        l.l[j] = lo[7 - j];
    }
    // (the halves' upper four limbs reach the product as literal zeros: its accumulator operands are early-clobber for exactly this,
    // tools/gen_fp_mul.py; tests/test_gpu_fp_device.py holds this very shape)
#pragma unroll
    for (int j = 0; j < 12; ++j) c.l[j] = H2C_2P256[j];
    fp_to_mont(hm, h);
    fp_to_mont(lm, l);
    fp_mul(t, hm, c);
    fp_add(r, t, lm);
}

// ---- Fp2 helpers in the lane-pair form
// a^-1, Montgomery in and out; a == 0 yields 0
__device__ __forceinline__ void f2_inv(fp& r, const fp& a, bool role)
{
    fp sq, sqo, n, ni, t, nt;
    fp_sqr(sq, a);
    fp_xchg(sqo, sq);
    fp_add(n, sq, sqo);
    fp_inv(ni, n);
    fp_mul(t, a, ni);
    fp_neg(nt, t);
    fp_select(r, role, nt, t);
}
// sgn0 of RFC 9380 for m = 2: c0 mod 2, and c1 mod 2 where c0 == 0
__device__ __forceinline__ bool f2_sgn0(const fp& a, bool role)
{
    fp plain;
    fp_from_mont(plain, a);
    const int mine = (int)(plain.l[0] & 1u) | (fp_is_zero(plain) ? 2 : 0);
    const int other = __shfl_xor(mine, 1, 64);
    const int c0 = role ? other : mine, c1 = role ? mine : other;
    return ((c0 & 2) ? c1 : c0) & 1;
}
__device__ __forceinline__ void f2_conj(fp& r, const fp& a, bool role)
{
    fp n;
    fp_neg(n, a);
    fp_select(r, role, n, a);
}
// g(x) = x (x^2 + A') + B' on E'
__device__ __forceinline__ void h2c_g(fp& r, const fp& x, const fp& A, const fp& B, bool role)
{
    fp t;
    f2_sqr(t, x, role);
    fp_add(t, t, A);
    f2_mul(r, t, x, role);
    fp_add(r, r, B);
}
__device__ __forceinline__ void fp_times9(fp& r, const fp& a)
{
    fp t;
    fp_dbl(t, a);
    fp_dbl(t, t);
    fp_dbl(t, t);
    fp_add(r, t, a);
}

// ---- points of E2 as XYZZ
__device__ __forceinline__ void g2x_neg(g2x& p) { fp_neg(p.y, p.y); }
// psi = twist o Frobenius o untwist on fractions: the conjugate of every coordinate (ZZ^3 = ZZZ^2 survives), times c_x and c_y
__device__ __forceinline__ g2x g2x_psi(const g2x& p, bool role)
{
    g2x r;
    fp c, t;
    f2_conj(t, p.x, role);
    h2c_const(c, H2C_PSI_CX, role);
    f2_mul(r.x, t, c, role);
    f2_conj(t, p.y, role);
    h2c_const(c, H2C_PSI_CY, role);
    f2_mul(r.y, t, c, role);
    f2_conj(r.zz, p.zz, role);
    f2_conj(r.zzz, p.zzz, role);
    return r;
}
// [|c|] P, c = -0xd201000000010000 the curve's parameter: 63 doublings, 5 additions; left to right, bit 63 is the leading one
__device__ __forceinline__ g2x g2x_mul_abs_c(const g2x& base, bool role)
{
    const uint32_t C_HI = 0xd2010000u, C_LO = 0x00010000u;
    g2x acc = base;
#pragma unroll 1
    for (int b = 62; b >= 0; --b) {
        acc = g2x_double(acc, role);
        const uint32_t w = b >= 32 ? C_HI : C_LO;
        if ((w >> (b & 31)) & 1u) g2x_add(acc, base, role);
    }
    return acc;
}
}  // namespace

// ---------------------------------------------------------------- hash_to_field
// msgs: n messages of msg_len bytes, back to back; dst: dst_len bytes.  u_mont: 48 words per message, u0.c0 | u0.c1 | u1.c0 | u1.c1.
__global__ void __launch_bounds__(64)
k_h2c_expand(const uint8_t* __restrict__ msgs, uint32_t n, uint32_t msg_len, const uint8_t* __restrict__ dst, uint32_t dst_len,
             uint32_t* __restrict__ u_mont)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    H2cText t;
    t.msg = msgs + (size_t)msg_len * i;
    t.dst = dst;
    t.msg_len = msg_len;
    t.dst_len = dst_len;
    uint32_t b0[8];
    h2c_b0(b0, t);
    uint32_t prev[8], head[8], hi[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) prev[j] = 0;  // b1 = H(b0 | 1 | DST'): b0 xor nothing
#pragma unroll 1
    for (uint32_t idx = 1; idx <= 8; ++idx) {
#pragma unroll
        for (int j = 0; j < 8; ++j) head[j] = b0[j] ^ prev[j];
        h2c_bi(prev, head, idx, t);
        if (idx & 1) {
#pragma unroll
            for (int j = 0; j < 8; ++j) hi[j] = prev[j];
        } else {  // element idx / 2 - 1 of the four is (b_{idx-1} | b_idx)
            fp e;
            h2c_reduce(e, hi, prev);
            fp_vec16::st(u_mont + 48ull * i + 12 * (idx / 2 - 1), e);
        }
    }
}
void launch_h2c_expand(hipStream_t s, const uint8_t* msgs, uint32_t n, uint32_t msg_len, const uint8_t* dst, uint32_t dst_len,
                       uint32_t* u_mont)
{
    if (n == 0) return;
    hipLaunchKernelGGL(k_h2c_expand, dim3((n + 63) / 64), dim3(64), 0, s, msgs, n, msg_len, dst, dst_len, u_mont);
}

// n_words 48-byte big-endian values (canonical: the host has checked) -> Montgomery words, one lane each
__global__ void __launch_bounds__(256)
k_h2c_load_u(const uint8_t* __restrict__ be48, uint32_t n_words, uint32_t* __restrict__ u_mont)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_words) return;
    fp v;
    fp_load_be48(v, be48 + 48ull * i);
    v.l[11] = __builtin_bswap32(reinterpret_cast<const uint32_t*>(be48 + 48ull * i)[0]);  // no flag bits here
    fp_to_mont(v, v);
    fp_vec16::st(u_mont + 12ull * i, v);
}
void launch_h2c_load_u(hipStream_t s, const uint8_t* be48, uint32_t n_words, uint32_t* u_mont)
{
    if (n_words == 0) return;
    hipLaunchKernelGGL(k_h2c_load_u, dim3((n_words + 255) / 256), dim3(256), 0, s, be48, n_words, u_mont);
}

// ---------------------------------------------------------------- SWU + isogeny
// u_mont: n_u values of 24 words (c0 | c1); out_xyzz: n_u points of G2X_WORDS words, on E2, not yet in G2.
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1)))
k_h2c_map(const uint32_t* __restrict__ u_mont, uint32_t n_u, uint32_t* __restrict__ out_xyzz)
{
    const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t i = lane >> 1;
    const bool role = lane & 1;
    if (i >= n_u) return;  // both lanes of a pair
    fp u, A, B, c, t, zu2, tv1, x1, x2, g1, g2;
    fp_vec16::ld(u, u_mont + 24ull * i + (role ? 12 : 0));
    h2c_const(A, H2C_A, role);
    h2c_const(B, H2C_B, role);
    // tv1 = Z^2 u^4 + Z u^2;  x1 = (-B'/A') (1 + 1/tv1), or B'/(Z A') where tv1 == 0;  x2 = Z u^2 x1
    f2_sqr(t, u, role);
    h2c_const(c, H2C_Z, role);
    f2_mul(zu2, c, t, role);
    f2_sqr(t, zu2, role);
    fp_add(tv1, t, zu2);
    const bool exceptional = f2_is_zero(tv1);
    f2_inv(t, tv1, role);
    f2_set_one(c, role);
    fp_add(t, t, c);
    h2c_const(c, H2C_MBA, role);
    f2_mul(x1, c, t, role);
    h2c_const(c, H2C_X1_EXC, role);
    fp_select(x1, exceptional, c, x1);
    f2_mul(x2, zu2, x1, role);
    h2c_g(g1, x1, A, B, role);
    h2c_g(g2, x2, A, B, role);
    // the lane of c0 gathers g(x1), the lane of c1 g(x2); each takes the root of its own
    fp a0, a1, r0, r1;
    fp_select(c, role, g1, g2);
    fp_xchg(t, c);
    fp_select(a0, role, t, g1);
    fp_select(a1, role, g2, t);
    fp_set_zero(r0);
    fp_set_zero(r1);
    int32_t st = 0;
    f2_sqrt_lane(r0, r1, st, a0, a1);
    const bool ok = st == 0;
    const bool ok_other = __shfl_xor((int)ok, 1, 64) != 0;
    const bool take1 = role ? ok_other : ok;             // g(x1) is a square: x1, else x2
    const bool any = ok || ok_other;
    // the chosen root's halves: the lane that found it keeps its own component and sends the other
    fp x, y;
    fp_select(c, role, r0, r1);
    fp_xchg(t, c);
    fp_select(c, role, r1, r0);
    fp_select(y, take1 != role, c, t);
    fp_select(x, take1, x1, x2);
    if (f2_sgn0(y, role) != f2_sgn0(u, role)) fp_neg(y, y);
    // the isogeny, d = x - x0
    g2x p;
    fp d, d2, d3, vd, uq;
    h2c_const(c, H2C_X0, role);
    fp_sub(d, x, c);
    f2_sqr(d2, d, role);
    f2_mul(d3, d2, d, role);
    h2c_const(c, H2C_V, role);
    f2_mul(vd, c, d, role);
    h2c_const(uq, H2C_UQ, role);
    f2_mul(t, x, d2, role);
    fp_add(t, t, vd);
    fp_add(p.x, t, uq);
    fp_sub(t, d3, vd);
    fp_sub(t, t, uq);
    fp_sub(t, t, uq);
    f2_mul(c, y, t, role);
    fp_neg(p.y, c);
    fp_times9(p.zz, d2);
    fp_times9(t, d3);
    fp_dbl(c, t);
    fp_add(p.zzz, c, t);
    if (f2_is_zero(d) || !any) g2x_set_inf(p);  // the isogeny's kernel (no root at all cannot happen: it would be the identity too)
    g2x_st<fp_vec16>(out_xyzz + (size_t)G2X_WORDS * i, p, role);
}
void launch_h2c_map(hipStream_t s, const uint32_t* u_mont, uint32_t n_u, uint32_t* out_xyzz)
{
    if (n_u == 0) return;
    hipLaunchKernelGGL(k_h2c_map, dim3((2 * n_u + 63) / 64), dim3(64), 0, s, u_mont, n_u, out_xyzz);
}

// ---------------------------------------------------------------- add, clear the cofactor, wire form
// pts_xyzz: 2 n points, message i's are 2 i and 2 i + 1.  out_be192: 192 bytes per message (x.c1 | x.c0 | y.c1 | y.c0; the
// identity: 0x40 and zeros).  status (nullable): 0, or 1 where H is the identity.
// h(P) = [c^2 - c - 1] P + [c - 1] psi(P) + psi^2(2 P) (Budroni-Pintore), as   t1 = [c] P;  t2 = psi(P);
// t3 = psi^2(2 P) - t2;  t2 = [c] (t1 + t2);  Q = t3 + t2 - t1 - P   with c < 0: the products run over |c| and change sign.
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1)))
k_h2c_finish(const uint32_t* __restrict__ pts_xyzz, uint32_t n, uint8_t* __restrict__ out_be192, int32_t* __restrict__ status)
{
    const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t i = lane >> 1;
    const bool role = lane & 1;
    if (i >= n) return;
    g2x P, q;
    g2x_ld<fp_vec16>(P, pts_xyzz + (size_t)G2X_WORDS * (2ull * i), role);
    g2x_ld<fp_vec16>(q, pts_xyzz + (size_t)G2X_WORDS * (2ull * i + 1), role);
    g2x_add(P, q, role);
    g2x a = g2x_mul_abs_c(P, role);  // -t1
    g2x s = g2x_psi(P, role);
    q = a;
    g2x_neg(q);
    g2x_add(s, q, role);             // t1 + psi(P)
    g2x b = g2x_mul_abs_c(s, role);  // -t2
    g2x acc = g2x_double(P, role);
    acc = g2x_psi(acc, role);
    acc = g2x_psi(acc, role);
    q = g2x_psi(P, role);
    g2x_neg(q);
    g2x_add(acc, q, role);
    g2x_neg(b);
    g2x_add(acc, b, role);
    g2x_add(acc, a, role);
    g2x_neg(P);
    g2x_add(acc, P, role);
    // wire order: role 1 (c1) writes the leading 48 bytes of each coordinate
    uint8_t* o = out_be192 + 192ull * i;
    uint8_t* ox = o + (role ? 0 : 48);
    uint8_t* oy = o + 96 + (role ? 0 : 48);
    const bool inf = g2x_is_inf(acc);
    if (status && !role) status[i] = inf ? 1 : 0;
    if (inf) {
        uint32_t* wx = reinterpret_cast<uint32_t*>(ox);
        uint32_t* wy = reinterpret_cast<uint32_t*>(oy);
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            wx[j] = 0;
            wy[j] = 0;
        }
        if (role) wx[0] = 0x40u;  // byte 0 of the point
        return;
    }
    fp x, y;
    g2x_to_affine_plain(x, y, acc, role);
    fp_store_be48(ox, x);
    fp_store_be48(oy, y);
}
void launch_h2c_finish(hipStream_t s, const uint32_t* pts_xyzz, uint32_t n, uint8_t* out_be192, int32_t* status)
{
    if (n == 0) return;
    hipLaunchKernelGGL(k_h2c_finish, dim3((2 * n + 63) / 64), dim3(64), 0, s, pts_xyzz, n, out_be192, status);
}

}  // namespace posevo
