// pos_evolution_amd/csrc/sha256.h compiled for the HOST by a plain C++ compiler, from the very header the gfx950 kernels and
// engine_ssz.cpp include: tests/test_ssz_model.py holds both functions to hashlib.  With -DSHH_MAIN the file is a stand-alone
// program (its own main) for a run under -fsanitize=address,undefined: the zero hashes against their known answers, the
// padding table against the schedule computed the long way, and the two functions against each other's territory.
#include <string.h>

#include "../../pos_evolution_amd/csrc/sha256.h"

using namespace posevo;

namespace {

uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
void put_be32(uint32_t w, uint8_t* p)
{
    p[0] = (uint8_t)(w >> 24);
    p[1] = (uint8_t)(w >> 16);
    p[2] = (uint8_t)(w >> 8);
    p[3] = (uint8_t)w;
}

}  // namespace

extern "C" {

// digests of n messages of 64 bytes each
void shh_sha256_64(const uint8_t* msgs, uint64_t n, uint8_t* out32)
{
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t w[16], d[8];
        for (int k = 0; k < 16; ++k) w[k] = be32(msgs + 64 * i + 4 * k);
        sha256_64(w, d);
        for (int k = 0; k < 8; ++k) put_be32(d[k], out32 + 32 * i + 4 * k);
    }
}

// digest of one message of len <= 55 bytes: padded here into its one block.  -> 0, or 1 where len does not fit
int shh_sha256_one_block(const uint8_t* msg, uint32_t len, uint8_t* out32)
{
    if (len > 55) return 1;
    uint8_t block[64];
    memset(block, 0, sizeof block);
    if (len) memcpy(block, msg, len);
    block[len] = 0x80;
    put_be32(len * 8, block + 60);
    uint32_t w[16], d[8];
    for (int k = 0; k < 16; ++k) w[k] = be32(block + 4 * k);
    sha256_one_block(w, d);
    for (int k = 0; k < 8; ++k) put_be32(d[k], out32 + 4 * k);
    return 0;
}

}  // extern "C"

#ifdef SHH_MAIN
#include <stdio.h>
int main()
{
    // Z[1] .. Z[3]: the first and last words of the known answers
    static const uint32_t want[3][2] = {{0xf5a5fd42u, 0x2759fb4bu}, {0xdb56114eu, 0x748b5d71u}, {0xc78009fdu, 0x105ab33cu}};
    uint32_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < 3; ++k) {
        uint32_t msg[16], next[8];
        memcpy(msg, z, 32);
        memcpy(msg + 8, z, 32);
        sha256_64(msg, next);
        memcpy(z, next, 32);
        if (z[0] != want[k][0] || z[7] != want[k][1]) {
            printf("Z[%d] wrong\n", k + 1);
            return 1;
        }
    }
    // the padding block's schedule, the long way
    uint32_t w[64];
    memset(w, 0, sizeof w);
    w[0] = 0x80000000u;
    w[15] = 512;
    for (int i = 16; i < 64; ++i)
        w[i] = w[i - 16] + (rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3)) + w[i - 7] +
               (rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10));
    for (int i = 0; i < 64; ++i)
        if (w[i] != SHA_PAD64.w[i]) {
            printf("SHA_PAD64.w[%d] wrong\n", i);
            return 1;
        }
    // every one-block length, all-zero and all-0xFF: the digest changes with each length and value (no byte dropped), and a
    // length that does not fit is refused
    uint8_t msg[64], prev[32], dig[32];
    memset(prev, 0, sizeof prev);
    long hashed = 0;
    for (int fill = 0; fill < 2; ++fill) {
        memset(msg, fill ? 0xFF : 0x00, sizeof msg);
        for (uint32_t len = 0; len <= 55; ++len) {
            if (shh_sha256_one_block(msg, len, dig)) return 1;
            if (memcmp(dig, prev, 32) == 0) {
                printf("one-block digest of length %u repeats\n", len);
                return 1;
            }
            memcpy(prev, dig, 32);
            ++hashed;
        }
        shh_sha256_64(msg, 1, dig);
        ++hashed;
    }
    if (shh_sha256_one_block(msg, 56, dig) != 1) return 1;
    printf("sha256_host: zero hashes and padding table exact, %ld messages hashed\n", hashed);
    return 0;
}
#endif
