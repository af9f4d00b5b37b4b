// deposit_row.h -- what process_deposit (pe:139-175) asks of ONE deposit: the roots it hashes, the Merkle branch it walks, the
// slot its pubkey's leaf takes in the pubkey index, the status it gets once the registry, the batch before it and its
// signature's verdict are known, and the validator it creates (get_validator_from_deposit: the reference names it, pe:166, and
// holds the fields it fills, pe:36-45; its text is the consensus specification's [UPSTREAM-MEMORY], restated in
// tests/deposits_model.py).  One text for the kernels of deposit_kernels.hip, the host step of engine_deposit.cpp and a plain
// host compiler (tests/native/deposit_row_host.cpp, held to the model by tests/test_deposits_model.py), like registry_row.h
// and reward_row.h.
//
// Hash words are SHA's big-endian words (sha256.h); a deposit row is the 184 bytes of pe_deposit_data read as 46 words in
// memory order.
#pragma once
#include <stdint.h>

#include "pe_hd.h"
#include "sha256.h"

namespace posevo {

constexpr uint32_t DEPOSIT_NONE = 0xFFFFFFFFu;
constexpr uint32_t DEPOSIT_ROW_WORDS = 46;     // pubkey 12 | withdrawal_credentials 8 | amount 2 | signature 24
constexpr uint32_t DEPOSIT_PROOF_NODES = 33;   // DEPOSIT_CONTRACT_TREE_DEPTH + 1 (pe:106, pe:144)
constexpr uint64_t DEPOSIT_MAX_AMOUNT = 1ull << 63;  // increase_balance does not saturate: the sums of one call stay below 2^64
constexpr uint32_t DEPOSIT_MIN_SLOTS = 64;

// pe_deposit_status (include/posevo.h)
constexpr int32_t DEPOSIT_APPENDED = 0, DEPOSIT_TOPUP = 1, DEPOSIT_IGNORED_BAD_SIGNATURE = 2, DEPOSIT_BAD_PROOF = 3;

// pe_deposit_params (include/posevo.h)
struct DepositParams {
    uint64_t effective_balance_increment;
    uint64_t max_effective_balance;
    uint64_t far_future_epoch;
};

// get_validator_from_deposit without the two byte strings it copies
struct DepositValidator {
    uint64_t effective_balance;
    uint64_t activation_eligibility_epoch, activation_epoch, exit_epoch, withdrawable_epoch;
    uint32_t slashed;
    uint32_t increments;  // effective_balance // increment: the working-state view's 16-bit column
};

PE_HD uint64_t deposit_effective_balance(uint64_t amount, uint64_t increment, uint64_t max_effective_balance)
{
    const uint64_t floor = amount - amount % increment;
    return floor < max_effective_balance ? floor : max_effective_balance;
}

PE_HD DepositValidator deposit_validator(uint64_t amount, const DepositParams& P)
{
    DepositValidator v;
    v.effective_balance = deposit_effective_balance(amount, P.effective_balance_increment, P.max_effective_balance);
    v.activation_eligibility_epoch = v.activation_epoch = v.exit_epoch = v.withdrawable_epoch = P.far_future_epoch;
    v.slashed = 0;
    v.increments = (uint32_t)(v.effective_balance / P.effective_balance_increment);
    return v;
}

// The pubkey index: a power of two of u32 slots, at least twice the keys it must hold; a key starts at the first four bytes
// of its leaf, read little-endian, and probes linearly.
PE_HD uint32_t deposit_index_slots(uint64_t n_keys)
{
    uint32_t t = DEPOSIT_MIN_SLOTS;
    while ((uint64_t)t < 2 * n_keys && t < 0x80000000u) t <<= 1;
    return t;
}
PE_HD uint32_t deposit_slot(uint32_t leaf_word0_le, uint32_t mask) { return leaf_word0_le & mask; }

// The status of the deposit at batch position `pos`.  reg_index: the lowest registry index that holds its pubkey, or
// DEPOSIT_NONE; first_valid: the first batch position of its pubkey whose signature verifies, or DEPOSIT_NONE (read for new
// keys only).  Sequential semantics in closed form: before first_valid the key is unknown and the signature false (ignored),
// at first_valid the validator is created, after it the key is in the registry and the signature is not looked at.
PE_HD int32_t deposit_status(bool proof_ok, uint32_t reg_index, uint32_t pos, uint32_t first_valid)
{
    if (!proof_ok) return DEPOSIT_BAD_PROOF;
    if (reg_index != DEPOSIT_NONE) return DEPOSIT_TOPUP;
    if (first_valid == DEPOSIT_NONE || pos < first_valid) return DEPOSIT_IGNORED_BAD_SIGNATURE;
    return pos == first_valid ? DEPOSIT_APPENDED : DEPOSIT_TOPUP;
}

// ------------------------------------------------------------------ hashing
struct DepositRoots {
    uint32_t pubkey_leaf[8];   // hash_tree_root(BLSPubkey): H(pubkey || 16 zero bytes), the leaf the registry keeps
    uint32_t data_root[8];     // hash_tree_root(DepositData): the leaf of the deposit tree
    uint32_t message_root[8];  // hash_tree_root(DepositMessage)
};

// a uint64 as the first 8 bytes of a chunk (little-endian bytes as two big-endian words)
PE_HD void deposit_u64_chunk(uint64_t v, uint32_t* w)
{
    w[0] = __builtin_bswap32((uint32_t)v);
    w[1] = __builtin_bswap32((uint32_t)(v >> 32));
    for (int k = 2; k < 8; ++k) w[k] = 0;
}
PE_HD uint64_t deposit_amount(const uint32_t* row) { return (uint64_t)row[20] | ((uint64_t)row[21] << 32); }

// Nine hashes through ONE copy of sha256_64's text (the loop is not unrolled on the device): 0 the pubkey's leaf, 1 H(leaf ||
// credentials), 2 H(amount || 0), 3 the message's root, 4 .. 6 the signature's three chunks padded to four, 7 H(amount ||
// signature root), 8 the data's root.
PE_HD void deposit_roots(const uint32_t* row, DepositRoots& r)
{
    uint32_t head[8] = {}, sig01[8] = {}, tmp[8] = {}, dig[8];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int i = 0; i < 9; ++i) {
        uint32_t msg[16];
        if (i == 0) {
            for (int k = 0; k < 12; ++k) msg[k] = __builtin_bswap32(row[k]);
            for (int k = 12; k < 16; ++k) msg[k] = 0;
        } else if (i == 1) {
            for (int k = 0; k < 8; ++k) msg[k] = r.pubkey_leaf[k];
            for (int k = 0; k < 8; ++k) msg[8 + k] = __builtin_bswap32(row[12 + k]);
        } else if (i == 2) {
            deposit_u64_chunk(deposit_amount(row), msg);
            for (int k = 8; k < 16; ++k) msg[k] = 0;
        } else if (i == 3 || i == 8) {
            for (int k = 0; k < 8; ++k) msg[k] = head[k];
            for (int k = 0; k < 8; ++k) msg[8 + k] = tmp[k];
        } else if (i == 4) {
            for (int k = 0; k < 16; ++k) msg[k] = __builtin_bswap32(row[22 + k]);
        } else if (i == 5) {
            for (int k = 0; k < 8; ++k) msg[k] = __builtin_bswap32(row[38 + k]);
            for (int k = 8; k < 16; ++k) msg[k] = 0;
        } else if (i == 6) {
            for (int k = 0; k < 8; ++k) msg[k] = sig01[k];
            for (int k = 0; k < 8; ++k) msg[8 + k] = tmp[k];
        } else {  // 7
            deposit_u64_chunk(deposit_amount(row), msg);
            for (int k = 0; k < 8; ++k) msg[8 + k] = tmp[k];
        }
        sha256_64(msg, dig);
        for (int k = 0; k < 8; ++k) {
            if (i == 0) r.pubkey_leaf[k] = dig[k];
            else if (i == 1) head[k] = dig[k];
            else if (i == 3) r.message_root[k] = dig[k];
            else if (i == 4) sig01[k] = dig[k];
            else if (i == 8) r.data_root[k] = dig[k];
            else tmp[k] = dig[k];  // 2, 5, 6, 7: read by the next step
        }
    }
}

// compute_signing_root: hash_tree_root(SigningData(object_root, domain)) = H(object_root || domain)
PE_HD void deposit_signing_root(const uint32_t message_root[8], const uint32_t domain[8], uint32_t out[8])
{
    uint32_t msg[16];
    for (int k = 0; k < 8; ++k) {
        msg[k] = message_root[k];
        msg[8 + k] = domain[k];
    }
    sha256_64(msg, out);
}

// is_valid_merkle_branch(leaf, branch, 33, index, root): branch = 33 nodes of 8 words in memory order
PE_HD bool deposit_branch_ok(const uint32_t leaf[8], const uint32_t* branch, uint64_t index, const uint32_t root[8])
{
    uint32_t value[8];
    for (int k = 0; k < 8; ++k) value[k] = leaf[k];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (uint32_t i = 0; i < DEPOSIT_PROOF_NODES; ++i) {
        uint32_t msg[16];
        const bool right = (index >> i) & 1;  // index // 2^i % 2: this node is a right child
        for (int k = 0; k < 8; ++k) {
            const uint32_t b = __builtin_bswap32(branch[8 * i + k]);
            msg[k] = right ? b : value[k];
            msg[8 + k] = right ? value[k] : b;
        }
        sha256_64(msg, value);
    }
    bool same = true;
    for (int k = 0; k < 8; ++k) same = same && value[k] == root[k];
    return same;
}

}  // namespace posevo
