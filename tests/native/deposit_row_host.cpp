// The hashing, the index's slot rule, the status rule and get_validator_from_deposit of pos_evolution_amd/csrc/deposit_row.h
// compiled for the HOST by a plain C++ compiler, from the very header engine_deposit.cpp and the gfx950 kernels include:
// tests/test_deposits_model.py holds them against tests/deposits_model.py.  With -DDPH_MAIN the file is a stand-alone program
// (its own main) that runs a small batch through the same functions, for a run under -fsanitize=address,undefined.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../pos_evolution_amd/csrc/deposit_row.h"

using namespace posevo;

namespace {

void words_to_bytes(const uint32_t w[8], uint8_t* out)
{
    for (int k = 0; k < 8; ++k) {
        out[4 * k] = (uint8_t)(w[k] >> 24);
        out[4 * k + 1] = (uint8_t)(w[k] >> 16);
        out[4 * k + 2] = (uint8_t)(w[k] >> 8);
        out[4 * k + 3] = (uint8_t)w[k];
    }
}
void bytes_to_words(const uint8_t* b, uint32_t w[8])
{
    for (int k = 0; k < 8; ++k)
        w[k] = ((uint32_t)b[4 * k] << 24) | ((uint32_t)b[4 * k + 1] << 16) | ((uint32_t)b[4 * k + 2] << 8) | b[4 * k + 3];
}
uint32_t le_word0(const uint8_t* leaf) { return leaf[0] | ((uint32_t)leaf[1] << 8) | ((uint32_t)leaf[2] << 16) | ((uint32_t)leaf[3] << 24); }

// the open-addressing table of k_deposit_index_build, sequentially: entry = the lowest key with the slot's leaf
struct Table {
    std::vector<uint32_t> tab;
    uint32_t mask;
    explicit Table(uint32_t slots) : tab(slots, DEPOSIT_NONE), mask(slots - 1) {}
    uint32_t insert(const uint8_t* leaves, uint32_t v)
    {
        uint32_t slot = deposit_slot(le_word0(leaves + 32 * (size_t)v), mask);
        for (;;) {
            if (tab[slot] == DEPOSIT_NONE) { tab[slot] = v; return slot; }
            if (memcmp(leaves + 32 * (size_t)tab[slot], leaves + 32 * (size_t)v, 32) == 0) {
                if (v < tab[slot]) tab[slot] = v;
                return slot;
            }
            slot = (slot + 1) & mask;
        }
    }
    uint32_t find(const uint8_t* leaves, const uint8_t* leaf, uint32_t* probes) const
    {
        uint32_t slot = deposit_slot(le_word0(leaf), mask);
        for (*probes = 1;; ++*probes) {
            if (tab[slot] == DEPOSIT_NONE) return DEPOSIT_NONE;
            if (memcmp(leaves + 32 * (size_t)tab[slot], leaf, 32) == 0) return tab[slot];
            slot = (slot + 1) & mask;
        }
    }
};

}  // namespace

extern "C" {

// one deposit's roots as digest bytes; branch (nullable): 33 x 32 bytes -> *out_branch_ok
int dph_roots(const uint8_t* row184, const uint8_t* domain32, const uint8_t* branch, uint64_t index, const uint8_t* root32,
              uint8_t* out_leaf, uint8_t* out_data_root, uint8_t* out_signing_root, int* out_branch_ok)
{
    uint32_t row[DEPOSIT_ROW_WORDS];
    memcpy(row, row184, sizeof row);
    DepositRoots r;
    deposit_roots(row, r);
    words_to_bytes(r.pubkey_leaf, out_leaf);
    words_to_bytes(r.data_root, out_data_root);
    uint32_t dom[8], sr[8];
    bytes_to_words(domain32, dom);
    deposit_signing_root(r.message_root, dom, sr);
    words_to_bytes(sr, out_signing_root);
    if (branch) {
        uint32_t b[8 * DEPOSIT_PROOF_NODES], rt[8];
        memcpy(b, branch, sizeof b);
        bytes_to_words(root32, rt);
        *out_branch_ok = deposit_branch_ok(r.data_root, b, index, rt) ? 1 : 0;
    }
    return 0;
}

// A whole batch the way pe_process_deposits resolves it, over host arrays: the registry's index, the probe, the batch's own
// table, the first valid position per key, the status rule and the ordered count.  out_validator: 7 words per deposit, written
// for creators (effective balance, the four epochs, slashed, increments).  out_probes: the longest probe sequence a lookup took.
int dph_process(uint32_t n_reg, const uint8_t* reg_leaves, uint32_t n, const uint8_t* rows184, const uint8_t* sig_ok,
                const uint8_t* proof_ok, const uint64_t params[3], int32_t* status, uint32_t* index, uint64_t* out_validator,
                uint32_t* out_slots, uint32_t* out_probes)
{
    const DepositParams P{params[0], params[1], params[2]};
    Table reg(deposit_index_slots((uint64_t)n_reg + n));
    for (uint32_t v = 0; v < n_reg; ++v) reg.insert(reg_leaves, v);
    *out_slots = reg.mask + 1;
    *out_probes = 0;
    std::vector<uint8_t> leaf(32 * (size_t)n);
    std::vector<uint32_t> hit(n), key_slot(n, DEPOSIT_NONE);
    Table batch(deposit_index_slots(n));
    std::vector<uint32_t> first_valid(batch.tab.size(), DEPOSIT_NONE);
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t row[DEPOSIT_ROW_WORDS];
        memcpy(row, rows184 + 184 * (size_t)i, sizeof row);
        DepositRoots r;
        deposit_roots(row, r);
        words_to_bytes(r.pubkey_leaf, &leaf[32 * (size_t)i]);
        uint32_t probes;
        hit[i] = reg.find(reg_leaves, &leaf[32 * (size_t)i], &probes);
        if (probes > *out_probes) *out_probes = probes;
    }
    for (uint32_t i = 0; i < n; ++i)
        if (hit[i] == DEPOSIT_NONE) key_slot[i] = batch.insert(leaf.data(), i);
    for (uint32_t i = 0; i < n; ++i)
        if (hit[i] == DEPOSIT_NONE && sig_ok[i] && i < first_valid[key_slot[i]]) first_valid[key_slot[i]] = i;
    std::vector<uint32_t> rank(n);
    uint32_t creators = 0;
    for (uint32_t i = 0; i < n; ++i) {
        rank[i] = creators;
        creators += hit[i] == DEPOSIT_NONE && first_valid[key_slot[i]] == i;
    }
    bool any_bad = false;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t fv = hit[i] == DEPOSIT_NONE ? first_valid[key_slot[i]] : DEPOSIT_NONE;
        status[i] = deposit_status(proof_ok[i] != 0, hit[i], i, fv);
        any_bad = any_bad || status[i] == DEPOSIT_BAD_PROOF;
        index[i] = DEPOSIT_NONE;
        if (status[i] == DEPOSIT_TOPUP) index[i] = hit[i] != DEPOSIT_NONE ? hit[i] : n_reg + rank[fv];
        if (status[i] == DEPOSIT_APPENDED) {
            index[i] = n_reg + rank[i];
            uint32_t row[DEPOSIT_ROW_WORDS];
            memcpy(row, rows184 + 184 * (size_t)i, sizeof row);
            const DepositValidator v = deposit_validator(deposit_amount(row), P);
            uint64_t* o = out_validator + 7 * (size_t)i;
            o[0] = v.effective_balance;
            o[1] = v.activation_eligibility_epoch;
            o[2] = v.activation_epoch;
            o[3] = v.exit_epoch;
            o[4] = v.withdrawable_epoch;
            o[5] = v.slashed;
            o[6] = v.increments;
        }
    }
    if (any_bad)
        for (uint32_t i = 0; i < n; ++i) index[i] = DEPOSIT_NONE;
    return any_bad ? 1 : 0;
}

}  // extern "C"

#ifdef DPH_MAIN
int main()
{
    // four registry keys (two equal), a batch: top-up of the duplicate, new key invalid, new key valid, top-up of it, unknown invalid
    const uint32_t n_reg = 4, n = 5;
    std::vector<uint8_t> rows(184 * n, 0), reg_leaves(32 * n_reg);
    const uint8_t key_of[n] = {7, 9, 9, 9, 11};
    for (uint32_t i = 0; i < n; ++i) {
        memset(&rows[184 * i], key_of[i], 48);
        const uint64_t amount = 32000000000ull + i;
        memcpy(&rows[184 * i + 80], &amount, 8);
    }
    uint8_t leaf[32], data_root[32], signing[32], domain[32] = {3};
    for (uint32_t v = 0; v < n_reg; ++v) {
        std::vector<uint8_t> row(184, 0);
        memset(row.data(), v == 0 ? 1 : 7, 48);  // validators 1, 2, 3 share key 7
        dph_roots(row.data(), domain, nullptr, 0, nullptr, leaf, data_root, signing, nullptr);
        memcpy(&reg_leaves[32 * v], leaf, 32);
    }
    const uint8_t sig_ok[n] = {0, 0, 1, 0, 0}, proof_ok[n] = {1, 1, 1, 1, 1};
    const uint64_t params[3] = {1000000000ull, 32000000000ull, ~0ull};
    int32_t status[n];
    uint32_t index[n], slots, probes;
    uint64_t val[7 * n];
    if (dph_process(n_reg, reg_leaves.data(), n, rows.data(), sig_ok, proof_ok, params, status, index, val, &slots, &probes)) return 1;
    const int32_t want_status[n] = {DEPOSIT_TOPUP, DEPOSIT_IGNORED_BAD_SIGNATURE, DEPOSIT_APPENDED, DEPOSIT_TOPUP, DEPOSIT_IGNORED_BAD_SIGNATURE};
    const uint32_t want_index[n] = {1, DEPOSIT_NONE, 4, 4, DEPOSIT_NONE};
    for (uint32_t i = 0; i < n; ++i)
        if (status[i] != want_status[i] || index[i] != want_index[i]) { printf("deposit %u: %d %u\n", i, status[i], index[i]); return 2; }
    if (val[7 * 2] != 32000000000ull || val[7 * 2 + 1] != ~0ull || val[7 * 2 + 6] != 32) return 3;
    // a branch of the deposit's own making verifies, a flipped sibling does not
    std::vector<uint8_t> branch(32 * DEPOSIT_PROOF_NODES);
    for (size_t k = 0; k < branch.size(); ++k) branch[k] = (uint8_t)(k * 7 + 1);
    dph_roots(rows.data(), domain, nullptr, 0, nullptr, leaf, data_root, signing, nullptr);
    uint32_t value[8], b[8 * DEPOSIT_PROOF_NODES];
    memcpy(b, branch.data(), sizeof b);
    bytes_to_words(data_root, value);
    const uint64_t idx = 0x100000005ull;
    for (uint32_t i = 0; i < DEPOSIT_PROOF_NODES; ++i) {
        uint32_t msg[16];
        for (int k = 0; k < 8; ++k) {
            const uint32_t s = __builtin_bswap32(b[8 * i + k]);
            msg[k] = (idx >> i) & 1 ? s : value[k];
            msg[8 + k] = (idx >> i) & 1 ? value[k] : s;
        }
        sha256_64(msg, value);
    }
    uint8_t root[32];
    words_to_bytes(value, root);
    int ok = 0;
    dph_roots(rows.data(), domain, branch.data(), idx, root, leaf, data_root, signing, &ok);
    if (!ok) return 4;
    branch[32 * 31] ^= 1;
    dph_roots(rows.data(), domain, branch.data(), idx, root, leaf, data_root, signing, &ok);
    if (ok) return 5;
    printf("deposit rules exact (%u slots, %u probes)\n", slots, probes);
    return 0;
}
#endif
