// sha256.h -- SHA-256 for the message shapes the engine hashes, one text for the gfx950 kernels, the host side of the
// library and a plain host compiler (tests/native/sha256_host.cpp):
//   sha256_one_block   a message of at most 55 bytes, given as its one padded block (the shuffle's and the sampler's hashes)
//   sha256_64          a message of exactly 64 bytes: a Merkle node H(left || right) of SSZ (ssz_kernels.hip, engine_ssz.cpp)
//   sha256_compress    one compression over a running state: messages of any length (h2c_kernels.hip)
// Words are SHA's big-endian words throughout: word i of a message is bytes 4i .. 4i + 3 read big-endian, word i of a digest
// is written back the same way.
#pragma once
#include <stdint.h>

#include "pe_hd.h"

namespace posevo {

PE_HD_CONST uint32_t SHA_K[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98,
    0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786,
    0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8,
    0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13,
    0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819,
    0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a,
    0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7,
    0xc67178f2};

PE_HD uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

// SHA-256 of a message that fits one block (<= 55 bytes), given as 16 big-endian words already padded.
PE_HD void sha256_one_block(const uint32_t (&w_in)[16], uint32_t (&out)[8])
{
    uint32_t w[64];
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = w_in[i];
#pragma unroll
    for (int i = 16; i < 64; ++i) {
        const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
        const uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
        w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t a = 0x6a09e667, b = 0xbb67ae85, c = 0x3c6ef372, d = 0xa54ff53a, e = 0x510e527f, f = 0x9b05688c,
             g = 0x1f83d9ab, h = 0x5be0cd19;
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        const uint32_t S1 = rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25);
        const uint32_t ch = (e & f) ^ (~e & g);
        const uint32_t t1 = h + S1 + ch + SHA_K[i] + w[i];
        const uint32_t S0 = rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22);
        const uint32_t mj = (a & b) ^ (a & c) ^ (b & c);
        const uint32_t t2 = S0 + mj;
        h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    out[0] = a + 0x6a09e667; out[1] = b + 0xbb67ae85; out[2] = c + 0x3c6ef372; out[3] = d + 0xa54ff53a;
    out[4] = e + 0x510e527f; out[5] = f + 0x9b05688c; out[6] = g + 0x1f83d9ab; out[7] = h + 0x5be0cd19;
}

// The second block of every 64-byte message is the same: 0x80, 55 zero bytes, the bit length 512.  Its 64 schedule words
// are therefore constants; the table is formed by the compiler, and the second compression of sha256_64 computes no schedule.
struct Sha256Pad64 {
    uint32_t w[64];
};
constexpr uint32_t sha256_rotr_const(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
constexpr Sha256Pad64 sha256_pad64_make()
{
    Sha256Pad64 t{};
    t.w[0] = 0x80000000u;
    t.w[15] = 512;
    for (int i = 16; i < 64; ++i) {
        const uint32_t s0 = sha256_rotr_const(t.w[i - 15], 7) ^ sha256_rotr_const(t.w[i - 15], 18) ^ (t.w[i - 15] >> 3);
        const uint32_t s1 = sha256_rotr_const(t.w[i - 2], 17) ^ sha256_rotr_const(t.w[i - 2], 19) ^ (t.w[i - 2] >> 10);
        t.w[i] = t.w[i - 16] + s0 + t.w[i - 7] + s1;
    }
    return t;
}
PE_HD_CONST Sha256Pad64 SHA_PAD64 = sha256_pad64_make();

// One round: (a .. h) rotate by name at the call sites, so the eight working words never move between registers.
#define PE_SHA_ROUND(a, b, c, d, e, f, g, h, kw)                                       \
    do {                                                                               \
        const uint32_t t1_ = (h) + (rotr((e), 6) ^ rotr((e), 11) ^ rotr((e), 25)) +    \
                             (((e) & (f)) ^ (~(e) & (g))) + (kw);                      \
        const uint32_t t2_ = (rotr((a), 2) ^ rotr((a), 13) ^ rotr((a), 22)) +          \
                             (((a) & (b)) ^ ((a) & (c)) ^ ((b) & (c)));                \
        (d) += t1_;                                                                    \
        (h) = t1_ + t2_;                                                               \
    } while (0)
#define PE_SHA_ROUNDS8(s, KW)                                          \
    do {                                                               \
        PE_SHA_ROUND(s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], KW(0)); \
        PE_SHA_ROUND(s[7], s[0], s[1], s[2], s[3], s[4], s[5], s[6], KW(1)); \
        PE_SHA_ROUND(s[6], s[7], s[0], s[1], s[2], s[3], s[4], s[5], KW(2)); \
        PE_SHA_ROUND(s[5], s[6], s[7], s[0], s[1], s[2], s[3], s[4], KW(3)); \
        PE_SHA_ROUND(s[4], s[5], s[6], s[7], s[0], s[1], s[2], s[3], KW(4)); \
        PE_SHA_ROUND(s[3], s[4], s[5], s[6], s[7], s[0], s[1], s[2], KW(5)); \
        PE_SHA_ROUND(s[2], s[3], s[4], s[5], s[6], s[7], s[0], s[1], KW(6)); \
        PE_SHA_ROUND(s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[0], KW(7)); \
    } while (0)

// SHA-256 of exactly 64 bytes: one compression from the IV over the message (a rolling 16-word schedule: the fully
// unrolled text keeps 16 + 8 + 8 words live, not 64), one from there over the constant padding block.
PE_HD void sha256_64(const uint32_t in[16], uint32_t out[8])
{
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = in[i];
    uint32_t s[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
#pragma unroll
    for (int base = 0; base < 64; base += 8) {
        if (base >= 16) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int i = base + j;
                const uint32_t x15 = w[(i - 15) & 15], x2 = w[(i - 2) & 15];
                const uint32_t s0 = rotr(x15, 7) ^ rotr(x15, 18) ^ (x15 >> 3);
                const uint32_t s1 = rotr(x2, 17) ^ rotr(x2, 19) ^ (x2 >> 10);
                w[i & 15] = w[i & 15] + s0 + w[(i - 7) & 15] + s1;
            }
        }
#define PE_SHA_KW(j) (SHA_K[base + (j)] + w[(base + (j)) & 15])
        PE_SHA_ROUNDS8(s, PE_SHA_KW);
#undef PE_SHA_KW
    }
    uint32_t mid[8];
    const uint32_t iv[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        mid[i] = s[i] + iv[i];
        s[i] = mid[i];
    }
#pragma unroll
    for (int base = 0; base < 64; base += 8) {
#define PE_SHA_KW(j) (SHA_K[base + (j)] + SHA_PAD64.w[base + (j)])
        PE_SHA_ROUNDS8(s, PE_SHA_KW);
#undef PE_SHA_KW
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = s[i] + mid[i];
}
// One compression of a message of any length: s (the IV to begin with) takes the block w, 16 big-endian words, which the
// rolling schedule overwrites.  Padding is the caller's (hash_to_field's expander, h2c_kernels.hip).
PE_HD void sha256_compress(uint32_t (&s)[8], uint32_t (&w)[16])
{
    uint32_t in[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) in[i] = s[i];
#pragma unroll
    for (int base = 0; base < 64; base += 8) {
        if (base >= 16) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int i = base + j;
                const uint32_t x15 = w[(i - 15) & 15], x2 = w[(i - 2) & 15];
                const uint32_t s0 = rotr(x15, 7) ^ rotr(x15, 18) ^ (x15 >> 3);
                const uint32_t s1 = rotr(x2, 17) ^ rotr(x2, 19) ^ (x2 >> 10);
                w[i & 15] = w[i & 15] + s0 + w[(i - 7) & 15] + s1;
            }
        }
#define PE_SHA_KW(j) (SHA_K[base + (j)] + w[(base + (j)) & 15])
        PE_SHA_ROUNDS8(s, PE_SHA_KW);
#undef PE_SHA_KW
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] += in[i];
}
#undef PE_SHA_ROUNDS8
#undef PE_SHA_ROUND

}  // namespace posevo
