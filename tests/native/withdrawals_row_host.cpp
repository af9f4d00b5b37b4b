// pos_evolution_amd/csrc/withdrawals_row.h compiled for the HOST by a plain C++ compiler, from the very header
// engine_withdrawals.cpp and the gfx950 kernels include: a whole pe_process_withdrawals and a whole
// pe_process_bls_to_execution_changes over host arrays in the kernels' steps (a kind per position, counts per workgroup of 256,
// their exclusive scan, ranks, the records of rank < k, the host step, one writing pass; the checks, the per-validator minimum,
// the statuses, one writing pass).  tests/test_withdrawals_row_host.py holds it against tests/withdrawals_model.py.  With
// -DWRH_MAIN the file is a stand-alone program (its own main) that holds the same calls to sequential loops on small random
// registries, for a run under -fsanitize=address,undefined.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../pos_evolution_amd/csrc/withdrawals_row.h"

using namespace posevo;

extern "C" {

unsigned wrh_record_words() { return WD_WORDS; }
unsigned wrh_change_words() { return CRED_CHANGE_WORDS; }

// params = the four words of pe_withdrawals_params; payload: n_payload entries of 11 words, have_payload 0: none.
// out_list: room for 64 entries of 11 words; out_result: next index, next validator, n_full, n_partial, total, count, status,
// first mismatch, applied; out_root: 32 bytes.  -> 0, else withdrawals_check_params' code, 8: apply without a payload (nothing
// written).
int wrh_process_withdrawals(uint64_t n, const uint8_t* cred, const uint64_t* wdr, const uint64_t* eff, uint64_t* bal, uint64_t epoch,
                            uint64_t next_index, uint64_t start, const uint64_t params[4], const uint32_t* payload, uint32_t n_payload,
                            int have_payload, int apply, uint32_t* out_list, uint64_t out_result[9], uint8_t out_root[32])
{
    WithdrawalsParams P;
    memcpy(&P, params, sizeof P);
    if (apply && !have_payload) return 8;
    if (const int rc = withdrawals_check_params(P, n, start, next_index, have_payload != 0, n_payload)) return rc;
    const uint32_t bound = (uint32_t)withdrawals_bound(n, P.max_validators_per_sweep), k = (uint32_t)P.max_withdrawals_per_payload;
    const uint32_t WG = 256, n_wg = (bound + WG - 1) / WG;
    auto cred_words = [&](uint64_t v, uint32_t* w) { memcpy(w, cred + 32 * v, 32); };
    // k_withdrawals_flag
    std::vector<uint8_t> kind(bound);
    std::vector<uint32_t> wg_count(n_wg, 0), wg_off(n_wg, 0);
    for (uint32_t j = 0; j < bound; ++j) {
        const uint64_t v = withdrawals_validator(start, j, n);
        uint32_t c[8];
        cred_words(v, c);
        kind[j] = (uint8_t)withdrawals_kind(c[0], (uint32_t)P.eth1_prefix, wdr[v], eff[v], bal[v], epoch, P.max_effective_balance);
        wg_count[j / WG] += kind[j] != WD_NONE;
    }
    // k_withdrawals_scan
    uint32_t total = 0;
    for (uint32_t g = 0; g < n_wg; ++g) {
        wg_off[g] = total;
        total += wg_count[g];
    }
    // k_withdrawals_select
    std::vector<uint32_t> records((size_t)WD_RECORD_WORDS * WD_MAX_PER_PAYLOAD, 0);
    for (uint32_t g = 0; g < n_wg; ++g) {
        if (wg_off[g] >= k) continue;
        uint32_t rank = wg_off[g];
        for (uint32_t j = g * WG; j < std::min(bound, (g + 1) * WG); ++j) {
            if (kind[j] == WD_NONE) continue;
            if (rank < k) {
                const uint64_t v = withdrawals_validator(start, j, n);
                uint32_t c[8];
                cred_words(v, c);
                uint32_t* r = records.data() + (size_t)WD_RECORD_WORDS * rank;
                withdrawals_record(r, next_index + rank, v, c, withdrawals_amount(kind[j], bal[v], P.max_effective_balance));
                r[WD_WORDS] = kind[j];
            }
            ++rank;
        }
    }
    // the host step
    const uint32_t count = std::min(total, k);
    WithdrawalsOutcome o;
    withdrawals_outcome(P, n, start, next_index, records.data(), count, out_list, payload, have_payload != 0, n_payload, &o);
    const bool applied = apply && o.status == WD_OK;
    // k_withdrawals_apply
    if (applied)
        for (uint32_t i = 0; i < count; ++i) {
            const uint32_t* r = records.data() + (size_t)WD_RECORD_WORDS * i;
            const uint64_t v = withdrawals_u64(r + 2), amount = withdrawals_u64(r + 9);
            bal[v] = amount > bal[v] ? 0 : bal[v] - amount;
        }
    const uint64_t res[9] = {o.next_withdrawal_index, o.next_withdrawal_validator_index, o.n_full, o.n_partial, o.total_gwei, count,
                             o.status, o.first_mismatch, applied ? 1ull : 0ull};
    memcpy(out_result, res, sizeof res);
    for (int i = 0; i < 8; ++i) {
        const uint32_t be = __builtin_bswap32(o.root[i]);
        memcpy(out_root + 4 * i, &be, 4);
    }
    return 0;
}

// changes: n_changes entries of 20 words.  -> the number of invalid changes; the credentials are written only where it is 0.
uint32_t wrh_bls_changes(uint64_t n, uint8_t* cred, const uint32_t* changes, uint32_t n_changes, int32_t* status)
{
    std::vector<uint32_t> first(std::max<uint64_t>(n, 1), CRED_NONE), checks(n_changes);
    // k_bls_changes_claim
    for (uint32_t p = 0; p < n_changes; ++p) {
        const uint32_t* c = changes + (size_t)CRED_CHANGE_WORDS * p;
        const uint64_t v = bls_change_index(c);
        uint32_t w[8] = {};
        if (v < n) memcpy(w, cred + 32 * v, 32);
        checks[p] = bls_change_checks(c, v < n, w);
        if (checks[p] == CRED_CHECK_ALL) first[v] = std::min(first[v], p);
    }
    // k_bls_changes_resolve
    uint32_t n_invalid = 0;
    for (uint32_t p = 0; p < n_changes; ++p) {
        const uint64_t v = bls_change_index(changes + (size_t)CRED_CHANGE_WORDS * p);
        status[p] = (int32_t)bls_change_status(checks[p], (checks[p] & CRED_CHECK_INDEX) && first[v] < p);
        n_invalid += status[p] != (int32_t)CRED_OK;
    }
    // k_bls_changes_apply
    if (!n_invalid)
        for (uint32_t p = 0; p < n_changes; ++p) {
            const uint32_t* c = changes + (size_t)CRED_CHANGE_WORDS * p;
            uint32_t w[8];
            bls_change_credentials(c, w);
            memcpy(cred + 32 * bls_change_index(c), w, 32);
        }
    return n_invalid;
}

void wrh_signing_roots(const uint32_t* changes, uint32_t n_changes, const uint8_t domain[32], uint8_t* out_roots)
{
    uint32_t dom[8];
    for (int k = 0; k < 8; ++k) {
        uint32_t le;
        memcpy(&le, domain + 4 * k, 4);
        dom[k] = __builtin_bswap32(le);
    }
    for (uint32_t p = 0; p < n_changes; ++p) {
        uint32_t out[8];
        bls_change_signing_root(changes + (size_t)CRED_CHANGE_WORDS * p, dom, out);
        for (int k = 0; k < 8; ++k) {
            const uint32_t be = __builtin_bswap32(out[k]);
            memcpy(out_roots + 32 * (size_t)p + 4 * k, &be, 4);
        }
    }
}

// the plain SHA-256 of 48 key bytes as bls_change_hash_ok computes it: 1 where credentials[1:] match
int wrh_hash_ok(const uint32_t* change, const uint8_t cred[32])
{
    uint32_t w[8];
    memcpy(w, cred, 32);
    return bls_change_hash_ok(change, w) ? 1 : 0;
}

}  // extern "C"

#ifdef WRH_MAIN
int main()
{
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    auto next = [&]() {
        seed ^= seed << 13;
        seed ^= seed >> 7;
        seed ^= seed << 17;
        return seed;
    };
    const uint64_t MAXEB = 32000000000ull, FAR = ~0ull;
    long checked = 0;
    for (int round = 0; round < 300; ++round) {
        const uint64_t n = 1 + next() % 700, epoch = 5 + next() % 3;
        const uint64_t k = 1 + next() % 20, sweep = 1 + next() % 900, start = next() % n, next_index = next() % 1000;
        std::vector<uint8_t> cred(32 * n);
        std::vector<uint64_t> wdr(n), eff(n), bal(n);
        const uint64_t dense = 1 + next() % 40;
        for (uint64_t v = 0; v < n; ++v) {
            for (int b = 0; b < 32; ++b) cred[32 * v + b] = (uint8_t)next();
            cred[32 * v] = next() % dense == 0 ? 1 : (uint8_t)(next() % 3);
            const uint64_t wd[4] = {epoch - 1, epoch, epoch + 1, FAR}, bl[6] = {0, 1, MAXEB - 1, MAXEB, MAXEB + 1, MAXEB + 77};
            wdr[v] = wd[next() % 4];
            eff[v] = next() % 4 ? MAXEB : MAXEB - 1000000000ull;
            bal[v] = bl[next() % 6];
        }
        // the sequential loop
        std::vector<uint64_t> b2(bal);
        std::vector<uint32_t> want;
        uint64_t wi = next_index, vi = start, count = 0, last = 0;
        for (uint64_t t = 0; t < std::min(n, sweep); ++t) {
            const bool prefix = cred[32 * vi] == 1;
            uint64_t amount = 0;
            bool hit = false;
            if (prefix && wdr[vi] <= epoch && bal[vi] > 0) hit = true, amount = bal[vi];
            else if (prefix && eff[vi] == MAXEB && bal[vi] > MAXEB) hit = true, amount = bal[vi] - MAXEB;
            if (hit) {
                uint32_t w[WD_WORDS], c[8];
                memcpy(c, &cred[32 * vi], 32);
                withdrawals_record(w, wi, vi, c, amount);
                want.insert(want.end(), w, w + WD_WORDS);
                b2[vi] -= amount;
                ++wi, ++count, last = vi;
            }
            if (count == k) break;
            vi = (vi + 1) % n;
        }
        const uint64_t want_next = count == k ? (last + 1) % n : (start + sweep) % n;
        const uint64_t params[4] = {MAXEB, k, sweep, 1};
        std::vector<uint32_t> list(WD_WORDS * WD_MAX_PER_PAYLOAD);
        std::vector<uint64_t> b1(bal);
        uint64_t res[9];
        uint8_t root[32];
        if (wrh_process_withdrawals(n, cred.data(), wdr.data(), eff.data(), b1.data(), epoch, next_index, start, params, want.data(),
                                    (uint32_t)count, 1, 1, list.data(), res, root))
            return 2;
        list.resize(WD_WORDS * count);
        if (list != want || b1 != b2 || res[0] != wi || res[1] != want_next || res[5] != count || res[6] != 0 || res[8] != 1) {
            printf("round %d: the sweep and the sequential loop differ\n", round);
            return 1;
        }
        checked += (long)count;

        // address changes: a few validators with the credentials of a key, named once or twice, with every kind of fault
        const uint32_t n_changes = 1 + (uint32_t)(next() % 12);
        std::vector<uint32_t> changes((size_t)CRED_CHANGE_WORDS * n_changes);
        for (uint32_t p = 0; p < n_changes; ++p) {
            uint32_t* c = &changes[(size_t)CRED_CHANGE_WORDS * p];
            const uint64_t v = next() % 8 == 0 ? n + next() % 3 : next() % std::min<uint64_t>(n, 6);
            c[0] = (uint32_t)v;
            c[1] = 0;
            for (int w = 2; w < 14; ++w) c[w] = (uint32_t)(v * 2654435761u + w);  // the key of validator v
            for (int w = 14; w < 19; ++w) c[w] = (uint32_t)next();
            c[19] = next() % 6 ? 1 : 0;
            if (next() % 7 == 0) c[5] ^= 1;  // another key
        }
        for (uint64_t v = 0; v < std::min<uint64_t>(n, 6); ++v) {  // credentials: 0x00 || H(key)[1:], some left as they are
            if (next() % 5 == 0) continue;
            uint32_t msg[16], dig[8];
            for (int w = 2; w < 14; ++w) msg[w - 2] = __builtin_bswap32((uint32_t)(v * 2654435761u + w));
            msg[12] = 0x80000000u, msg[13] = msg[14] = 0, msg[15] = 384;
            sha256_one_block(msg, dig);
            for (int w = 0; w < 8; ++w) {
                const uint32_t be = __builtin_bswap32(dig[w]);
                memcpy(&cred[32 * v + 4 * w], &be, 4);
            }
            cred[32 * v] = 0;
        }
        std::vector<uint8_t> c2(cred), c1(cred);
        std::vector<int32_t> want_st(n_changes), got_st(n_changes);
        bool all_valid = true;
        for (uint32_t p = 0; p < n_changes; ++p) {
            const uint32_t* c = &changes[(size_t)CRED_CHANGE_WORDS * p];
            const uint64_t v = c[0];
            int32_t st = 0;
            if (v >= n) st = CRED_BAD_INDEX;
            else if (c2[32 * v] != 0) st = CRED_NOT_BLS;
            else if (!wrh_hash_ok(c, &c2[32 * v])) st = CRED_PUBKEY_MISMATCH;
            else if (!(c[19] & 1)) st = CRED_BAD_SIGNATURE;
            else {
                memset(&c2[32 * v], 0, 12);
                c2[32 * v] = 1;
                memcpy(&c2[32 * v + 12], c + 14, 20);
            }
            want_st[p] = st;
            all_valid = all_valid && st == 0;
        }
        if (!all_valid) c2 = cred;
        wrh_bls_changes(n, c1.data(), changes.data(), n_changes, got_st.data());
        if (got_st != want_st || c1 != c2) {
            printf("round %d: the changes and the sequential loop differ\n", round);
            return 1;
        }
        checked += n_changes;
    }
    printf("withdrawals_row_host: %ld withdrawals and changes, closed form exact\n", checked);
    return 0;
}
#endif
