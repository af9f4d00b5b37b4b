// fp_device_ops.hip -- the 12 x 32 Montgomery field ops of pos_evolution_amd/csrc applied ON THE DEVICE to chosen operands: a
// stand-alone program (its own main, nothing of the engine, no libposevo.so) for tests/test_gpu_fp_device.py; the integer model
// and the op table are tests/fp_device_model.py.
//
//   fp_device_ops IN OUT
//
// IN is a sequence of sections: u32 op id, u32 n, then n records of NIN operands, twelve little-endian u32 limbs each.  Every
// section is one kernel launch; OUT receives the sections' results in order, n records of NOUT u32 each (the result's limbs, and
// a flag or status word where the op has one).  One lane per record; the Fp2 ops of g2.h take one lane PAIR per record (role =
// lane & 1 holds component c_role), the grid padded to whole waves so that both lanes of every pair run every exchange.
// Exit status: 0, 2 on a HIP error, 3 on a malformed file.  No timing, no retries.
//
// Built with the library's own flags (csrc/Makefile: --offload-arch=gfx950 -O3 -std=c++17) and the INLINE product: what is held
// here is what hipcc makes of fp381_mul.inc's asm statements inside each caller, constants and all.  The constant-operand
// family (OpMulConst and after) hands the product operands whose upper limbs are literal zeros, with no register barrier.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "fp381.h"
#include "fp_inv_safegcd.h"
#include "fp_sqrt.h"
#include "g2.h"
#include "fp12.h"  // f2_mul_xi only

#ifdef POSEVO_FP_MUL_CALLED
#error "the called product hides constants behind the call: this harness holds the inline one"
#endif

using namespace posevo;

namespace {

__device__ __forceinline__ void put(uint32_t* o, const fp& a)
{
#pragma unroll
    for (int j = 0; j < 12; ++j) o[j] = a.l[j];
}

// ---- Fp ops: run(in, out), in = NIN loaded operands, out = NOUT words
struct OpAdd { static constexpr int NIN = 2, NOUT = 12; static __device__ void run(const fp* x, uint32_t* o) { fp r; fp_add(r, x[0], x[1]); put(o, r); } };
struct OpSub { static constexpr int NIN = 2, NOUT = 12; static __device__ void run(const fp* x, uint32_t* o) { fp r; fp_sub(r, x[0], x[1]); put(o, r); } };
struct OpNeg { static constexpr int NIN = 1, NOUT = 12; static __device__ void run(const fp* x, uint32_t* o) { fp r; fp_neg(r, x[0]); put(o, r); } };
struct OpDbl { static constexpr int NIN = 1, NOUT = 12; static __device__ void run(const fp* x, uint32_t* o) { fp r; fp_dbl(r, x[0]); put(o, r); } };
struct OpMul { static constexpr int NIN = 2, NOUT = 12; static __device__ void run(const fp* x, uint32_t* o) { fp r; fp_mul(r, x[0], x[1]); put(o, r); } };
struct OpSqr { static constexpr int NIN = 1, NOUT = 12; static __device__ void run(const fp* x, uint32_t* o) { fp r; fp_sqr(r, x[0]); put(o, r); } };
struct OpToMont { static constexpr int NIN = 1, NOUT = 12; static __device__ void run(const fp* x, uint32_t* o) { fp r; fp_to_mont(r, x[0]); put(o, r); } };
struct OpFromMont { static constexpr int NIN = 1, NOUT = 12; static __device__ void run(const fp* x, uint32_t* o) { fp r; fp_from_mont(r, x[0]); put(o, r); } };
struct OpInv { static constexpr int NIN = 1, NOUT = 12; static __device__ void run(const fp* x, uint32_t* o) { fp r; fp_inv(r, x[0]); put(o, r); } };
struct OpInvPlain { static constexpr int NIN = 1, NOUT = 12; static __device__ void run(const fp* x, uint32_t* o) { fp r; fp_inv_plain(r, x[0]); put(o, r); } };
struct OpSqrt {
    static constexpr int NIN = 1, NOUT = 13;
    static __device__ void run(const fp* x, uint32_t* o)
    {
        fp r;
        const bool ok = fp_sqrt(r, x[0]);
        put(o, r);
        o[12] = ok ? 1u : 0u;
    }
};
struct OpHalf { static constexpr int NIN = 1, NOUT = 12; static __device__ void run(const fp* x, uint32_t* o) { fp r; fp_half(r, x[0]); put(o, r); } };
struct OpIsLargerHalf { static constexpr int NIN = 1, NOUT = 1; static __device__ void run(const fp* x, uint32_t* o) { o[0] = fp_is_larger_half(x[0]) ? 1u : 0u; } };
struct OpIsCanonical { static constexpr int NIN = 1, NOUT = 1; static __device__ void run(const fp* x, uint32_t* o) { o[0] = fp_is_canonical(x[0]) ? 1u : 0u; } };
// the operand's twelve words are the 48 bytes; out: the limbs fp_load_be48 makes of them, then the bytes fp_store_be48 writes back
struct OpBe48 {
    static constexpr int NIN = 1, NOUT = 24;
    static __device__ void run(const fp* x, uint32_t* o)
    {
        fp r;
        fp_load_be48(r, reinterpret_cast<const uint8_t*>(x[0].l));
        put(o, r);
        fp_store_be48(reinterpret_cast<uint8_t*>(o + 12), r);
    }
};
// both components in one lane: (a0, a1) -> y0, y1, status
struct OpF2SqrtLane {
    static constexpr int NIN = 2, NOUT = 25;
    static __device__ void run(const fp* x, uint32_t* o)
    {
        fp y0, y1;
        int32_t st = 0;
        fp_set_zero(y0);
        fp_set_zero(y1);
        f2_sqrt_lane(y0, y1, st, x[0], x[1]);
        put(o, y0);
        put(o + 12, y1);
        o[24] = (uint32_t)st;
    }
};

// ---- the constant-operand family: limbs j >= K of the named operand are literal zeros IN THE KERNEL, no register barrier
enum { SIDE_A = 0, SIDE_B = 1, SIDE_BOTH = 2 };
template <int K>
__device__ __forceinline__ void cut(fp& r, const fp& a)
{
#pragma unroll
    for (int j = 0; j < 12; ++j) r.l[j] = j < K ? a.l[j] : 0u;
}
template <int K, int SIDE>
struct OpMulConst {
    static constexpr int NIN = 2, NOUT = 12;
    static __device__ void run(const fp* x, uint32_t* o)
    {
        fp a = x[0], b = x[1], r;
        if (SIDE == SIDE_A || SIDE == SIDE_BOTH) cut<K>(a, x[0]);
        if (SIDE == SIDE_B || SIDE == SIDE_BOTH) cut<K>(b, x[1]);
        fp_mul(r, a, b);
        put(o, r);
    }
};
template <int K>
struct OpToMontConst {
    static constexpr int NIN = 1, NOUT = 12;
    static __device__ void run(const fp* x, uint32_t* o)
    {
        fp a, r;
        cut<K>(a, x[0]);
        fp_to_mont(r, a);
        put(o, r);
    }
};
template <int K>
struct OpFromMontConst {
    static constexpr int NIN = 1, NOUT = 12;
    static __device__ void run(const fp* x, uint32_t* o)
    {
        fp a, r;
        cut<K>(a, x[0]);
        fp_from_mont(r, a);
        put(o, r);
    }
};
// a low literal over literal zeros: fp_from_mont's {1, 0, ...} and the curve kernels' four = {4, 0, ...}
template <uint32_t V>
__device__ __forceinline__ void literal(fp& r)
{
    fp_set_zero(r);
    r.l[0] = V;
}
template <uint32_t V>
struct OpMulLiteralB {
    static constexpr int NIN = 1, NOUT = 12;
    static __device__ void run(const fp* x, uint32_t* o)
    {
        fp c, r;
        literal<V>(c);
        fp_mul(r, x[0], c);
        put(o, r);
    }
};
template <uint32_t V>
struct OpMulLiteralA {
    static constexpr int NIN = 1, NOUT = 12;
    static __device__ void run(const fp* x, uint32_t* o)
    {
        fp c, r;
        literal<V>(c);
        fp_mul(r, c, x[0]);
        put(o, r);
    }
};
// x + to_mont(literal): the shape of rhs = x^3 + four in k_g1_decompress and wire_points.h
template <uint32_t V>
struct OpAddToMontLiteral {
    static constexpr int NIN = 1, NOUT = 12;
    static __device__ void run(const fp* x, uint32_t* o)
    {
        fp c, r;
        literal<V>(c);
        fp_to_mont(c, c);
        fp_add(r, x[0], c);
        put(o, r);
    }
};

// h2c_kernels.hip's h2c_reduce restated (the original sits in an anonymous namespace): hi 2^256 + lo from two halves of eight
// BIG-endian words -- two fp_to_mont, one fp_mul by the Montgomery form of 2^256, one fp_add.  BARRIER: the original's register
// barrier on the halves' limbs, or none.
__device__ const uint32_t TWO_P256_MONT[12] = {0xc5ce820fu, 0x075b3cd7u, 0x1c3edb0bu, 0x3ec6ba62u, 0x2bff6bceu, 0x168a13d8u,
                                               0xf8c449d2u, 0x87663c4bu, 0xddc8d830u, 0x15f34c83u, 0x9caa2e85u, 0x0f9628b4u};
template <bool BARRIER>
struct OpH2cReduce {
    static constexpr int NIN = 2, NOUT = 12;
    static __device__ void run(const fp* x, uint32_t* o)
    {
        uint32_t hi[8], lo[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            hi[j] = x[0].l[7 - j];
            lo[j] = x[1].l[7 - j];
        }
        fp h, l, c, hm, lm, t, r;
        fp_set_zero(h);
        fp_set_zero(l);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            h.l[j] = hi[7 - j];
            l.l[j] = lo[7 - j];
        }
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            if (BARRIER) {
                asm volatile("" : "+v"(h.l[j]));
                asm volatile("" : "+v"(l.l[j]));
            }
            c.l[j] = TWO_P256_MONT[j];
        }
        fp_to_mont(hm, h);
        fp_to_mont(lm, l);
        fp_mul(t, hm, c);
        fp_add(r, t, lm);
        put(o, r);
    }
};

// ---- Fp2 ops in the lane-pair form: x = this lane's components of the NIN / 2 operands, o = this lane's half of the result
struct OpF2Mul { static constexpr int NIN = 4, NOUT = 24; static __device__ void run(const fp* x, uint32_t* o, bool role) { fp r; f2_mul(r, x[0], x[1], role); put(o, r); } };
struct OpF2Sqr { static constexpr int NIN = 2, NOUT = 24; static __device__ void run(const fp* x, uint32_t* o, bool role) { fp r; f2_sqr(r, x[0], role); put(o, r); } };
struct OpF2InvPlain { static constexpr int NIN = 2, NOUT = 24; static __device__ void run(const fp* x, uint32_t* o, bool role) { fp r; f2_inv_plain(r, x[0], role); put(o, r); } };
struct OpF2MulXi { static constexpr int NIN = 2, NOUT = 24; static __device__ void run(const fp* x, uint32_t* o, bool role) { fp r; f2_mul_xi(r, x[0], role); put(o, r); } };
struct OpF2IsZero { static constexpr int NIN = 2, NOUT = 2; static __device__ void run(const fp* x, uint32_t* o, bool) { o[0] = f2_is_zero(x[0]) ? 1u : 0u; } };

template <class Op>
__global__ void k_lane(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fp x[Op::NIN];
    uint32_t o[Op::NOUT];
#pragma unroll
    for (int k = 0; k < Op::NIN; ++k)
#pragma unroll
        for (int j = 0; j < 12; ++j) x[k].l[j] = in[((size_t)i * Op::NIN + k) * 12 + j];
    Op::run(x, o);
#pragma unroll
    for (int j = 0; j < Op::NOUT; ++j) out[(size_t)i * Op::NOUT + j] = o[j];
}
// lanes past the last record compute on zeros and store nothing: no lane leaves before the exchanges
template <class Op>
__global__ void k_pair(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n)
{
    constexpr int NV = Op::NIN / 2, HALF_OUT = Op::NOUT / 2;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t i = t >> 1;
    const bool role = (t & 1) != 0;
    const bool live = i < n;
    fp x[NV];
    uint32_t o[HALF_OUT];
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
        for (int j = 0; j < 12; ++j) x[k].l[j] = live ? in[((size_t)i * Op::NIN + 2 * k + (role ? 1 : 0)) * 12 + j] : 0u;
    Op::run(x, o, role);
    if (!live) return;
#pragma unroll
    for (int j = 0; j < HALF_OUT; ++j) out[(size_t)i * Op::NOUT + (role ? HALF_OUT : 0) + j] = o[j];
}

struct OpEntry {
    uint32_t id;
    int nin, nout;
    bool pair;
    void (*kernel)(const uint32_t*, uint32_t*, uint32_t);
};
template <class Op>
OpEntry lane_op(uint32_t id) { return {id, Op::NIN, Op::NOUT, false, k_lane<Op>}; }
template <class Op>
OpEntry pair_op(uint32_t id) { return {id, Op::NIN, Op::NOUT, true, k_pair<Op>}; }

template <int K>
void add_const_family(std::vector<OpEntry>& v)
{
    v.push_back(lane_op<OpMulConst<K, SIDE_A>>(100 + K));
    v.push_back(lane_op<OpMulConst<K, SIDE_B>>(113 + K));
    v.push_back(lane_op<OpMulConst<K, SIDE_BOTH>>(126 + K));
    v.push_back(lane_op<OpToMontConst<K>>(140 + K));
    v.push_back(lane_op<OpFromMontConst<K>>(160 + K));
    if constexpr (K < 12) add_const_family<K + 1>(v);
}
std::vector<OpEntry> op_table()
{
    std::vector<OpEntry> v = {
        lane_op<OpAdd>(1), lane_op<OpSub>(2), lane_op<OpNeg>(3), lane_op<OpDbl>(4), lane_op<OpMul>(5), lane_op<OpSqr>(6),
        lane_op<OpToMont>(7), lane_op<OpFromMont>(8), lane_op<OpInv>(9), lane_op<OpInvPlain>(10), lane_op<OpSqrt>(11),
        lane_op<OpHalf>(12), lane_op<OpIsLargerHalf>(13), lane_op<OpIsCanonical>(14), lane_op<OpBe48>(15),
        pair_op<OpF2Mul>(20), pair_op<OpF2Sqr>(21), pair_op<OpF2InvPlain>(22), pair_op<OpF2IsZero>(23), pair_op<OpF2MulXi>(24),
        lane_op<OpF2SqrtLane>(25),
        lane_op<OpH2cReduce<true>>(180), lane_op<OpH2cReduce<false>>(181),
        lane_op<OpMulLiteralB<1>>(190), lane_op<OpMulLiteralB<4>>(191), lane_op<OpMulLiteralA<1>>(192), lane_op<OpMulLiteralA<4>>(193),
        lane_op<OpAddToMontLiteral<1>>(194), lane_op<OpAddToMontLiteral<4>>(195),
    };
    add_const_family<0>(v);
    return v;
}

#define HIP_OK(call)                                                                                       \
    do {                                                                                                   \
        const hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) {                                                                            \
            fprintf(stderr, "HIP error: %s at %s:%d (%s)\n", hipGetErrorString(e_), __FILE__, __LINE__, #call); \
            exit(2);                                                                                       \
        }                                                                                                  \
    } while (0)

[[noreturn]] void malformed(const char* what)
{
    fprintf(stderr, "fp_device_ops: %s\n", what);
    exit(3);
}

std::vector<uint32_t> read_words(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) malformed("cannot open the operand file");
    std::vector<uint32_t> w;
    uint32_t buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) {
        if (got % 4) malformed("the operand file is no whole number of words");
        w.insert(w.end(), buf, buf + got / 4);
    }
    fclose(f);
    return w;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 3) malformed("usage: fp_device_ops IN OUT");
    const std::vector<OpEntry> table = op_table();
    const std::vector<uint32_t> in = read_words(argv[1]);
    constexpr uint32_t MAX_RECORDS = 1u << 20;
    std::vector<uint32_t> result;
    size_t at = 0;
    while (at < in.size()) {
        if (in.size() - at < 2) malformed("a section header is cut short");
        const uint32_t id = in[at], n = in[at + 1];
        at += 2;
        const OpEntry* op = nullptr;
        for (const OpEntry& e : table)
            if (e.id == id) op = &e;
        if (!op) malformed("unknown op id");
        if (n > MAX_RECORDS) malformed("too many records in one section");
        const size_t in_words = (size_t)n * op->nin * 12, out_words = (size_t)n * op->nout;
        if (in.size() - at < in_words) malformed("a section's records are cut short");
        if (n == 0) continue;
        uint32_t *d_in = nullptr, *d_out = nullptr;
        HIP_OK(hipMalloc(&d_in, in_words * 4));
        HIP_OK(hipMalloc(&d_out, out_words * 4));
        HIP_OK(hipMemcpy(d_in, in.data() + at, in_words * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemset(d_out, 0xee, out_words * 4));
        const size_t lanes = op->pair ? 2 * (size_t)n : n;
        const uint32_t blocks = (uint32_t)((lanes + 63) / 64);
        hipLaunchKernelGGL(op->kernel, dim3(blocks), dim3(64), 0, 0, d_in, d_out, n);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        const size_t base = result.size();
        result.resize(base + out_words);
        HIP_OK(hipMemcpy(result.data() + base, d_out, out_words * 4, hipMemcpyDeviceToHost));
        HIP_OK(hipFree(d_in));
        HIP_OK(hipFree(d_out));
        at += in_words;
    }
    FILE* f = fopen(argv[2], "wb");
    if (!f) malformed("cannot open the output file");
    if (!result.empty() && fwrite(result.data(), 4, result.size(), f) != result.size()) malformed("short write");
    if (fclose(f) != 0) malformed("short write");
    return 0;
}
