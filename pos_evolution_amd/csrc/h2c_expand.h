// h2c_expand.h -- expand_message_xmd of RFC 9380 over SHA-256, to the 256 bytes hash_to_field takes for G2: one text for
// k_h2c_expand (h2c_kernels.hip) and a plain host compiler (tests/native/h2c_expand_host.cpp holds it to hashlib).
//     b0 = H(0^64 | msg | I2OSP(256, 2) | 0 | DST')    b1 = H(b0 | 1 | DST')    b_i = H((b0 xor b_{i-1}) | i | DST')
// The message blocks are never laid out in memory: every word of a block is put together from the bytes at its positions, so
// the sixteen words stay in registers whatever the lengths are.
#pragma once
#include "sha256.h"

namespace posevo {

// ---- expand_message_xmd: the bytes of the two message shapes, by position
struct H2cText {
    const uint8_t* msg;
    const uint8_t* dst;
    uint32_t msg_len, dst_len;
};
// padding: 0x80 behind the `total` message bytes, zeros, the bit length in the last 8 bytes of the last block
PE_HD uint32_t h2c_pad_byte(uint32_t pos, uint32_t total, uint32_t n_blocks)
{
    if (pos == total) return 0x80u;
    const uint32_t tail = 64 * n_blocks - 4;  // the length is below 2^32 bits: its upper word is zero
    if (pos >= tail) return ((total * 8u) >> (8 * (3 - (pos - tail)))) & 0xFFu;
    return 0;
}
// b0's message: 64 zero bytes | msg | I2OSP(256, 2) | 0 | DST | len(DST)
PE_HD uint32_t h2c_b0_byte(const H2cText& t, uint32_t pos, uint32_t total, uint32_t n_blocks)
{
    if (pos < 64) return 0;
    uint32_t q = pos - 64;
    if (q < t.msg_len) return t.msg[q];
    q -= t.msg_len;
    if (q < 3) return q == 0 ? 1u : 0u;
    q -= 3;
    if (q < t.dst_len) return t.dst[q];
    if (q == t.dst_len) return t.dst_len;
    return h2c_pad_byte(pos, total, n_blocks);
}
// b_i's message past its first 32 bytes (which are words, not bytes: zero here): i | DST | len(DST)
PE_HD uint32_t h2c_bi_byte(const H2cText& t, uint32_t idx, uint32_t pos, uint32_t total, uint32_t n_blocks)
{
    if (pos < 32) return 0;
    uint32_t q = pos - 32;
    if (q == 0) return idx;
    q -= 1;
    if (q < t.dst_len) return t.dst[q];
    if (q == t.dst_len) return t.dst_len;
    return h2c_pad_byte(pos, total, n_blocks);
}
PE_HD void h2c_iv(uint32_t (&s)[8])
{
    s[0] = 0x6a09e667; s[1] = 0xbb67ae85; s[2] = 0x3c6ef372; s[3] = 0xa54ff53a;
    s[4] = 0x510e527f; s[5] = 0x9b05688c; s[6] = 0x1f83d9ab; s[7] = 0x5be0cd19;
}
// b0 = H(64 zero bytes | msg | I2OSP(256, 2) | 0 | DST')
PE_HD void h2c_b0(uint32_t (&out)[8], const H2cText& t)
{
    const uint32_t total = 64 + t.msg_len + 3 + t.dst_len + 1, n_blocks = (total + 9 + 63) / 64;
    h2c_iv(out);
#pragma unroll 1
    for (uint32_t blk = 0; blk < n_blocks; ++blk) {
        uint32_t w[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint32_t p = 64 * blk + 4 * j;
            w[j] = (h2c_b0_byte(t, p, total, n_blocks) << 24) | (h2c_b0_byte(t, p + 1, total, n_blocks) << 16) |
                   (h2c_b0_byte(t, p + 2, total, n_blocks) << 8) | h2c_b0_byte(t, p + 3, total, n_blocks);
        }
        sha256_compress(out, w);
    }
}
// H(head | idx | DST'): head = 32 bytes as 8 words
PE_HD void h2c_bi(uint32_t (&out)[8], const uint32_t (&head)[8], uint32_t idx, const H2cText& t)
{
    const uint32_t total = 32 + 1 + t.dst_len + 1, n_blocks = (total + 9 + 63) / 64;
    h2c_iv(out);
#pragma unroll 1
    for (uint32_t blk = 0; blk < n_blocks; ++blk) {
        uint32_t w[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint32_t p = 64 * blk + 4 * j;
            w[j] = (h2c_bi_byte(t, idx, p, total, n_blocks) << 24) | (h2c_bi_byte(t, idx, p + 1, total, n_blocks) << 16) |
                   (h2c_bi_byte(t, idx, p + 2, total, n_blocks) << 8) | h2c_bi_byte(t, idx, p + 3, total, n_blocks);
            if (j < 8 && blk == 0) w[j] = head[j];
        }
        sha256_compress(out, w);
    }
}

}  // namespace posevo
