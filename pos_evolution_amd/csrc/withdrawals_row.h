// withdrawals_row.h -- what Capella's process_withdrawals and process_bls_to_execution_change ask of ONE validator, ONE sweep
// position, ONE withdrawal and ONE address change, given the scalars of the call (has_eth1_withdrawal_credential,
// is_fully_withdrawable_validator, is_partially_withdrawable_validator, get_expected_withdrawals, process_withdrawals and
// process_bls_to_execution_change, restated in tests/withdrawals_model.py: the reference holds the Validator fields, pe:36-45,
// and `balances`, pe:112, not these functions' text).  One text for the kernels of withdrawal_kernels.hip, the host steps of
// engine_withdrawals.cpp and a plain host compiler (tests/native/withdrawals_row_host.cpp, held to the model by
// tests/test_withdrawals_row_host.py), like block_ops_row.h.
//
// The sweep visits position j = 0 .. bound - 1, validator (start + j) mod n, bound = min(n, max_validators_per_sweep) <= n:
// no validator is visited twice, so every position's predicate reads the state before the call and the loop's "stop at the
// k-th hit" is "the first k hits in position order".  Of two address changes that name one validator the first POTENT one --
// every check but "no earlier change took effect" holds -- wins: a per-validator minimum over positions, as block_ops_row.h's.
// Credentials are the 32 bytes in memory order, read as 8 little-endian words; hash words are SHA's big-endian words
// (sha256.h).  Every comparison is the specification's unsigned 64-bit.
#pragma once
#include <stdint.h>

#include "deposit_row.h"
#include "pe_hd.h"
#include "sha256.h"

namespace posevo {

// ------------------------------------------------------------------ withdrawals
constexpr uint32_t WD_NONE = 0, WD_FULL = 1, WD_PARTIAL = 2;  // what a swept position yields
constexpr uint32_t WD_MAX_PER_PAYLOAD = 64;                   // the largest max_withdrawals_per_payload a call takes
constexpr uint32_t WD_WORDS = 11;                             // pe_withdrawal, 44 bytes packed: index | validator_index | address | amount
constexpr uint32_t WD_RECORD_WORDS = 12;                      // ... as the kernels leave it: the 11 words and the kind
// pe_wd_status (include/posevo.h; engine_withdrawals.cpp asserts the equality)
constexpr uint32_t WD_OK = 0, WD_COUNT_MISMATCH = 80, WD_INDEX_MISMATCH = 81, WD_VALIDATOR_MISMATCH = 82,
                   WD_ADDRESS_MISMATCH = 83, WD_AMOUNT_MISMATCH = 84;

// pe_withdrawals_params (include/posevo.h)
struct WithdrawalsParams {
    uint64_t max_effective_balance;
    uint64_t max_withdrawals_per_payload;
    uint64_t max_validators_per_sweep;
    uint64_t eth1_prefix;
};

// has_eth1_withdrawal_credential: credentials[:1] == ETH1_ADDRESS_WITHDRAWAL_PREFIX.  cred_word0: bytes 0 .. 3
PE_HD bool withdrawals_has_eth1(uint32_t cred_word0, uint32_t prefix) { return (cred_word0 & 0xFFu) == prefix; }
// is_fully_withdrawable_validator
PE_HD bool withdrawals_fully(uint32_t cred_word0, uint32_t prefix, uint64_t withdrawable_epoch, uint64_t balance, uint64_t epoch)
{
    return withdrawals_has_eth1(cred_word0, prefix) && withdrawable_epoch <= epoch && balance > 0;
}
// is_partially_withdrawable_validator
PE_HD bool withdrawals_partially(uint32_t cred_word0, uint32_t prefix, uint64_t effective_balance, uint64_t balance,
                                 uint64_t max_effective_balance)
{
    return withdrawals_has_eth1(cred_word0, prefix) && effective_balance == max_effective_balance && balance > max_effective_balance;
}
// get_expected_withdrawals' if / elif over one visited validator
PE_HD uint32_t withdrawals_kind(uint32_t cred_word0, uint32_t prefix, uint64_t withdrawable_epoch, uint64_t effective_balance,
                                uint64_t balance, uint64_t epoch, uint64_t max_effective_balance)
{
    if (withdrawals_fully(cred_word0, prefix, withdrawable_epoch, balance, epoch)) return WD_FULL;
    if (withdrawals_partially(cred_word0, prefix, effective_balance, balance, max_effective_balance)) return WD_PARTIAL;
    return WD_NONE;
}
PE_HD uint64_t withdrawals_amount(uint32_t kind, uint64_t balance, uint64_t max_effective_balance)
{
    return kind == WD_FULL ? balance : balance - max_effective_balance;
}
PE_HD uint64_t withdrawals_bound(uint64_t n, uint64_t max_validators_per_sweep)
{
    return n < max_validators_per_sweep ? n : max_validators_per_sweep;
}
// the validator at sweep position j < bound <= n; start < n, so the sum stays below 2 n
PE_HD uint64_t withdrawals_validator(uint64_t start, uint64_t j, uint64_t n)
{
    const uint64_t v = start + j;
    return v >= n ? v - n : v;
}
// process_withdrawals' next_withdrawal_validator_index: behind the last withdrawal's validator where the list is full, else
// start + MAX_VALIDATORS_PER_WITHDRAWALS_SWEEP -- the parameter, not the bound -- mod n (the residues are added: no wrap)
PE_HD uint64_t withdrawals_next_validator(uint64_t start, uint64_t n, uint64_t max_validators_per_sweep, uint64_t count,
                                          uint64_t max_withdrawals_per_payload, uint64_t last_validator)
{
    if (count == max_withdrawals_per_payload) return (last_validator + 1) % n;
    return (start % n + max_validators_per_sweep % n) % n;
}
// One withdrawal as pe_withdrawal holds it, in 11 words; cred: the validator's credentials, the address is bytes 12 .. 31
PE_HD void withdrawals_record(uint32_t* w, uint64_t index, uint64_t validator, const uint32_t* cred, uint64_t amount)
{
    w[0] = (uint32_t)index;
    w[1] = (uint32_t)(index >> 32);
    w[2] = (uint32_t)validator;
    w[3] = (uint32_t)(validator >> 32);
    for (int k = 0; k < 5; ++k) w[4 + k] = cred[3 + k];
    w[9] = (uint32_t)amount;
    w[10] = (uint32_t)(amount >> 32);
}
PE_HD uint64_t withdrawals_u64(const uint32_t* w) { return (uint64_t)w[0] | ((uint64_t)w[1] << 32); }

// Every refusal that needs no device: 0 = none, else which (engine_withdrawals.cpp holds the texts)
PE_HD int withdrawals_check_params(const WithdrawalsParams& P, uint64_t n, uint64_t start, uint64_t next_index, bool have_payload,
                                   uint64_t n_payload)
{
    if (n == 0) return 1;
    if (start >= n) return 2;
    if (P.max_effective_balance == 0 || P.max_withdrawals_per_payload == 0 || P.max_validators_per_sweep == 0 || P.eth1_prefix == 0)
        return 3;
    if (P.eth1_prefix > 0xFF) return 4;
    if (P.max_withdrawals_per_payload > WD_MAX_PER_PAYLOAD) return 5;
    if (have_payload && n_payload > P.max_withdrawals_per_payload) return 6;
    if (next_index + P.max_withdrawals_per_payload < next_index) return 7;
    return 0;
}

// process_withdrawals' asserts over a payload: the lengths first, then entry by entry, field by field.  -> WD_*; *first: the
// first differing entry (the shorter length where the lengths differ).  Both lists in WD_WORDS words an entry.
PE_HD uint32_t withdrawals_compare(const uint32_t* expected, uint32_t count, const uint32_t* payload, uint32_t n_payload,
                                   uint32_t* first)
{
    *first = 0;
    if (count != n_payload) {
        *first = count < n_payload ? count : n_payload;
        return WD_COUNT_MISMATCH;
    }
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t *e = expected + WD_WORDS * i, *p = payload + WD_WORDS * i;
        uint32_t s = WD_OK;
        if (e[0] != p[0] || e[1] != p[1]) s = WD_INDEX_MISMATCH;
        else if (e[2] != p[2] || e[3] != p[3]) s = WD_VALIDATOR_MISMATCH;
        else if (e[4] != p[4] || e[5] != p[5] || e[6] != p[6] || e[7] != p[7] || e[8] != p[8]) s = WD_ADDRESS_MISMATCH;
        else if (e[9] != p[9] || e[10] != p[10]) s = WD_AMOUNT_MISMATCH;
        if (s != WD_OK) {
            *first = i;
            return s;
        }
    }
    return WD_OK;
}

// hash_tree_root(Withdrawal): four chunks -- index, validator_index, address || 0^12, amount
PE_HD void withdrawal_root(const uint32_t* w, uint32_t out[8])
{
    uint32_t msg[16], left[8], right[8];
    deposit_u64_chunk(withdrawals_u64(w), msg);
    deposit_u64_chunk(withdrawals_u64(w + 2), msg + 8);
    sha256_64(msg, left);
    for (int k = 0; k < 5; ++k) msg[k] = __builtin_bswap32(w[4 + k]);
    for (int k = 5; k < 8; ++k) msg[k] = 0;
    deposit_u64_chunk(withdrawals_u64(w + 9), msg + 8);
    sha256_64(msg, right);
    for (int k = 0; k < 8; ++k) {
        msg[k] = left[k];
        msg[8 + k] = right[k];
    }
    sha256_64(msg, out);
}
// hash_tree_root(List[Withdrawal, limit]) of count <= limit <= WD_MAX_PER_PAYLOAD entries: merkleize over the next power of
// two of the limit with zero subtrees, mixed with the length.  The host step's (a handful of hashes over what it read back).
PE_HD void withdrawals_list_root(const uint32_t* list, uint32_t count, uint32_t limit, uint32_t out[8])
{
    uint32_t level[WD_MAX_PER_PAYLOAD][8], zero[8] = {}, msg[16];
    for (uint32_t i = 0; i < count; ++i) withdrawal_root(list + WD_WORDS * i, level[i]);
    uint32_t len = count;
    for (uint32_t width = 1; width < limit; width <<= 1) {  // one level per doubling: ceil(log2(limit)) of them
        const uint32_t pairs = (len + 1) / 2;
        for (uint32_t i = 0; i < pairs; ++i) {
            for (int k = 0; k < 8; ++k) {
                msg[k] = level[2 * i][k];
                msg[8 + k] = 2 * i + 1 < len ? level[2 * i + 1][k] : zero[k];
            }
            sha256_64(msg, level[i]);
        }
        len = pairs;
        for (int k = 0; k < 8; ++k) msg[k] = msg[8 + k] = zero[k];
        sha256_64(msg, zero);
    }
    for (int k = 0; k < 8; ++k) msg[k] = len ? level[0][k] : zero[k];
    deposit_u64_chunk(count, msg + 8);
    sha256_64(msg, out);
}

// What one call found and leaves: the host step of pe_process_withdrawals behind the read-back of the records
struct WithdrawalsOutcome {
    uint64_t next_withdrawal_index, next_withdrawal_validator_index;
    uint64_t n_full, n_partial, total_gwei;  // the total is cut at 2^64 - 1
    uint32_t status, first_mismatch;
    uint32_t root[8];
};
// records: count entries of WD_RECORD_WORDS words; list: room for count entries of WD_WORDS words (the caller's array)
PE_HD void withdrawals_outcome(const WithdrawalsParams& P, uint64_t n, uint64_t start, uint64_t next_index, const uint32_t* records,
                               uint32_t count, uint32_t* list, const uint32_t* payload, bool have_payload, uint32_t n_payload,
                               WithdrawalsOutcome* o)
{
    o->n_full = o->n_partial = o->total_gwei = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t* r = records + WD_RECORD_WORDS * i;
        for (uint32_t k = 0; k < WD_WORDS; ++k) list[WD_WORDS * i + k] = r[k];
        o->n_full += r[WD_WORDS] == WD_FULL;
        o->n_partial += r[WD_WORDS] == WD_PARTIAL;
        const uint64_t amount = withdrawals_u64(r + 9), sum = o->total_gwei + amount;
        o->total_gwei = sum < amount ? ~0ull : sum;
    }
    o->next_withdrawal_index = next_index + count;
    o->next_withdrawal_validator_index = withdrawals_next_validator(
        start, n, P.max_validators_per_sweep, count, P.max_withdrawals_per_payload,
        count ? withdrawals_u64(records + WD_RECORD_WORDS * (count - 1) + 2) : 0);
    o->status = WD_OK;
    o->first_mismatch = 0;
    if (have_payload) o->status = withdrawals_compare(list, count, payload, n_payload, &o->first_mismatch);
    withdrawals_list_root(list, count, (uint32_t)P.max_withdrawals_per_payload, o->root);
}

// ------------------------------------------------------------------ BLS-to-execution changes
constexpr uint32_t CRED_CHANGE_WORDS = 20;  // pe_bls_change, 80 bytes: validator_index 2 | from_bls_pubkey 12 | address 5 | flags 1
constexpr uint32_t CRED_FLAG_SIGNATURE_VALID = 1u;
constexpr uint32_t CRED_BLS_PREFIX = 0x00, CRED_ETH1_PREFIX = 0x01;
constexpr uint32_t CRED_NONE = 0xFFFFFFFFu;  // no position in the per-validator table
// pe_cred_status (include/posevo.h)
constexpr uint32_t CRED_OK = 0, CRED_BAD_INDEX = 96, CRED_NOT_BLS = 97, CRED_PUBKEY_MISMATCH = 98, CRED_BAD_SIGNATURE = 99;
// what a change's own fields and the validator's credentials BEFORE the call decide
constexpr uint32_t CRED_CHECK_INDEX = 1u, CRED_CHECK_PREFIX = 2u, CRED_CHECK_HASH = 4u, CRED_CHECK_VERDICT = 8u, CRED_CHECK_ALL = 15u;

PE_HD uint64_t bls_change_index(const uint32_t* c) { return withdrawals_u64(c); }
// credentials[1:] == hash(from_bls_pubkey)[1:]: the plain SHA-256 of the 48 bytes, one block; byte 0 is not compared
PE_HD bool bls_change_hash_ok(const uint32_t* c, const uint32_t* cred)
{
    uint32_t msg[16], dig[8];
    for (int k = 0; k < 12; ++k) msg[k] = __builtin_bswap32(c[2 + k]);
    msg[12] = 0x80000000u;
    msg[13] = msg[14] = 0;
    msg[15] = 384;
    sha256_one_block(msg, dig);
    bool same = ((__builtin_bswap32(cred[0]) ^ dig[0]) & 0x00FFFFFFu) == 0;
    for (int k = 1; k < 8; ++k) same = same && __builtin_bswap32(cred[k]) == dig[k];
    return same;
}
// cred: the validator's credentials where index_ok, else not read
PE_HD uint32_t bls_change_checks(const uint32_t* c, bool index_ok, const uint32_t* cred)
{
    uint32_t ok = (c[19] & CRED_FLAG_SIGNATURE_VALID) ? CRED_CHECK_VERDICT : 0u;
    if (!index_ok) return ok;
    ok |= CRED_CHECK_INDEX;
    if ((cred[0] & 0xFFu) == CRED_BLS_PREFIX) ok |= CRED_CHECK_PREFIX;
    if (bls_change_hash_ok(c, cred)) ok |= CRED_CHECK_HASH;
    return ok;
}
// process_bls_to_execution_change's asserts in their order.  changed_earlier: an earlier change of the call took effect on
// the validator, whose credentials then begin with 0x01
PE_HD uint32_t bls_change_status(uint32_t checks, bool changed_earlier)
{
    if (!(checks & CRED_CHECK_INDEX)) return CRED_BAD_INDEX;
    if (!(checks & CRED_CHECK_PREFIX) || changed_earlier) return CRED_NOT_BLS;
    if (!(checks & CRED_CHECK_HASH)) return CRED_PUBKEY_MISMATCH;
    if (!(checks & CRED_CHECK_VERDICT)) return CRED_BAD_SIGNATURE;
    return CRED_OK;
}
// ETH1_ADDRESS_WITHDRAWAL_PREFIX + b'\x00' * 11 + to_execution_address
PE_HD void bls_change_credentials(const uint32_t* c, uint32_t cred[8])
{
    cred[0] = CRED_ETH1_PREFIX;
    cred[1] = cred[2] = 0;
    for (int k = 0; k < 5; ++k) cred[3 + k] = c[14 + k];
}
// compute_signing_root(BLSToExecutionChange, domain): five hashes through one copy of sha256_64's text -- 0 the pubkey's leaf,
// 1 H(index || leaf), 2 H(address || 0), 3 the message's root, 4 H(root || domain)
PE_HD void bls_change_signing_root(const uint32_t* c, const uint32_t domain[8], uint32_t out[8])
{
    uint32_t left[8] = {}, dig[8] = {};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int i = 0; i < 5; ++i) {
        uint32_t msg[16];
        if (i == 0) {
            for (int k = 0; k < 12; ++k) msg[k] = __builtin_bswap32(c[2 + k]);
            for (int k = 12; k < 16; ++k) msg[k] = 0;
        } else if (i == 1) {
            deposit_u64_chunk(bls_change_index(c), msg);
            for (int k = 0; k < 8; ++k) msg[8 + k] = dig[k];
        } else if (i == 2) {
            for (int k = 0; k < 5; ++k) msg[k] = __builtin_bswap32(c[14 + k]);
            for (int k = 5; k < 16; ++k) msg[k] = 0;
        } else {  // 3, 4
            for (int k = 0; k < 8; ++k) {
                msg[k] = left[k];
                msg[8 + k] = i == 3 ? dig[k] : domain[k];
            }
        }
        sha256_64(msg, dig);
        if (i == 1 || i == 3)
            for (int k = 0; k < 8; ++k) left[k] = dig[k];
    }
    for (int k = 0; k < 8; ++k) out[k] = dig[k];
}

}  // namespace posevo
