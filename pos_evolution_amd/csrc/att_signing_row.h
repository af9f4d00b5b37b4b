// att_signing_row.h -- the message an attestation's signature is over, from ONE attestation row: is_valid_indexed_attestation's
// signing_root = compute_signing_root(indexed_attestation.data, get_domain(state, DOMAIN_BEACON_ATTESTER, data.target.epoch)).
// The reference names both calls and holds no text of them; the conventions are the consensus specification's and SSZ's
// [UPSTREAM-MEMORY], restated in tests/att_signing_model.py:
//   hash_tree_root(Checkpoint)       H(u64_chunk(epoch) || root)
//   hash_tree_root(AttestationData)  merkleize of five chunks to depth 3: slot, index, beacon_block_root, the roots of source
//                                    and target; chunks 5 .. 7 are zero, so the node over chunks 6 and 7 is the constant Z[1]
//   compute_signing_root             hash_tree_root(SigningData(object_root, domain)) = H(object_root || domain)
//   get_domain                       over the current fork version from fork.epoch on, over the previous one before it
// Nine hashes of 64 bytes per row.  One text for k_att_signing_roots (att_signing_kernels.hip) and a plain host compiler
// (tests/native/att_signing_row_host.cpp, held to the model by tests/test_att_signing_host.py), like deposit_row.h and
// registry_row.h.
//
// Hash words are SHA's big-endian words (sha256.h); an attestation row is the 144 bytes of pe_attestation read as 36 words in
// memory order.  Only the first 32 words -- AttestationData -- enter: bits_offset, n_bits, flags and reserved0 do not.
#pragma once
#include <stdint.h>

#include "pe_hd.h"
#include "sha256.h"

namespace posevo {

constexpr uint32_t ATT_ROW_WORDS = 36;  // slot 2 | index 2 | beacon_block_root 8 | source 2 + 8 | target 2 + 8 | the rest 4
constexpr uint32_t ATT_W_SLOT = 0, ATT_W_INDEX = 2, ATT_W_BLOCK_ROOT = 4, ATT_W_SOURCE_EPOCH = 12, ATT_W_SOURCE_ROOT = 14,
                   ATT_W_TARGET_EPOCH = 22, ATT_W_TARGET_ROOT = 24;

// Z[1] = H(0^64): the node over two zero chunks
PE_HD_CONST uint32_t ATT_ZERO_NODE1[8] = {0xf5a5fd42u, 0xd16a2030u, 0x2798ef6eu, 0xd309979bu,
                                          0x43003d23u, 0x20d9f0e8u, 0xea9831a9u, 0x2759fb4bu};

// pe_attester_domains (include/posevo.h) with the two domains as hash words
struct AttDomains {
    uint64_t fork_epoch;
    uint32_t previous[8], current[8];
};
PE_HD void att_domains_load(uint64_t fork_epoch, const uint8_t previous32[32], const uint8_t current32[32], AttDomains& d)
{
    d.fork_epoch = fork_epoch;
    for (int k = 0; k < 8; ++k) {
        d.previous[k] = ((uint32_t)previous32[4 * k] << 24) | ((uint32_t)previous32[4 * k + 1] << 16) |
                        ((uint32_t)previous32[4 * k + 2] << 8) | previous32[4 * k + 3];
        d.current[k] = ((uint32_t)current32[4 * k] << 24) | ((uint32_t)current32[4 * k + 1] << 16) |
                       ((uint32_t)current32[4 * k + 2] << 8) | current32[4 * k + 3];
    }
}

PE_HD uint64_t att_row_u64(const uint32_t* row, uint32_t w) { return (uint64_t)row[w] | ((uint64_t)row[w + 1] << 32); }
// get_domain's choice: fork.previous_version if epoch < fork.epoch else fork.current_version
PE_HD bool att_domain_is_current(uint64_t target_epoch, uint64_t fork_epoch) { return target_epoch >= fork_epoch; }

// a uint64 of the row as the first 8 bytes of a chunk: its two words in memory order, byte-swapped into hash words
PE_HD void att_u64_chunk(const uint32_t* row, uint32_t w, uint32_t* msg)
{
    msg[0] = __builtin_bswap32(row[w]);
    msg[1] = __builtin_bswap32(row[w + 1]);
    for (int k = 2; k < 8; ++k) msg[k] = 0;
}
PE_HD void att_root_chunk(const uint32_t* row, uint32_t w, uint32_t* msg)
{
    for (int k = 0; k < 8; ++k) msg[k] = __builtin_bswap32(row[w + k]);
}

// Nine hashes through ONE copy of sha256_64's text (the loop is not unrolled on the device), two values of 8 words alive
// between them:
//   0  x = H(source.epoch || source.root)        hash_tree_root(source)
//   1  x = H(beacon_block_root || x)             chunks 2, 3
//   2  y = H(slot || index)                      chunks 0, 1
//   3  x = H(y || x)                             chunks 0 .. 3
//   4  y = H(target.epoch || target.root)        hash_tree_root(target)
//   5  y = H(y || 0)                             chunks 4, 5
//   6  y = H(y || Z[1])                          chunks 4 .. 7
//   7  x = H(x || y)                             hash_tree_root(AttestationData)
//   8  x = H(x || domain)                        the signing root
// data_root (nullable): step 7's value.
PE_HD void att_signing_root(const uint32_t* row, const AttDomains& d, uint32_t* data_root, uint32_t signing_root[8])
{
    uint32_t x[8] = {}, y[8] = {};
    const bool current = att_domain_is_current(att_row_u64(row, ATT_W_TARGET_EPOCH), d.fork_epoch);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int i = 0; i < 9; ++i) {
        uint32_t msg[16], dig[8];
        if (i == 0) {
            att_u64_chunk(row, ATT_W_SOURCE_EPOCH, msg);
            att_root_chunk(row, ATT_W_SOURCE_ROOT, msg + 8);
        } else if (i == 1) {
            att_root_chunk(row, ATT_W_BLOCK_ROOT, msg);
            for (int k = 0; k < 8; ++k) msg[8 + k] = x[k];
        } else if (i == 2) {
            att_u64_chunk(row, ATT_W_SLOT, msg);
            att_u64_chunk(row, ATT_W_INDEX, msg + 8);
        } else if (i == 3) {
            for (int k = 0; k < 8; ++k) {
                msg[k] = y[k];
                msg[8 + k] = x[k];
            }
        } else if (i == 4) {
            att_u64_chunk(row, ATT_W_TARGET_EPOCH, msg);
            att_root_chunk(row, ATT_W_TARGET_ROOT, msg + 8);
        } else if (i == 5 || i == 6) {
            for (int k = 0; k < 8; ++k) {
                msg[k] = y[k];
                msg[8 + k] = i == 5 ? 0u : ATT_ZERO_NODE1[k];
            }
        } else if (i == 7) {
            for (int k = 0; k < 8; ++k) {
                msg[k] = x[k];
                msg[8 + k] = y[k];
            }
        } else {  // 8
            for (int k = 0; k < 8; ++k) {
                msg[k] = x[k];
                msg[8 + k] = current ? d.current[k] : d.previous[k];
            }
        }
        sha256_64(msg, dig);
        const bool to_y = i == 2 || i == 4 || i == 5 || i == 6;
        for (int k = 0; k < 8; ++k) {
            if (to_y) y[k] = dig[k];
            else x[k] = dig[k];
        }
        if (i == 7 && data_root)
            for (int k = 0; k < 8; ++k) data_root[k] = dig[k];
    }
    for (int k = 0; k < 8; ++k) signing_root[k] = x[k];
}

}  // namespace posevo
