// engine_withdrawals.cpp -- Capella over the resident registry: pe_process_withdrawals (get_expected_withdrawals and
// process_withdrawals), pe_process_bls_to_execution_changes and pe_bls_change_signing_roots (restated in
// tests/withdrawals_model.py).  The pattern of pe_process_block_operations: read-only passes (withdrawal_kernels.hip), a host
// step, one writing pass.  The predicates, the record, the comparison with the payload, the next indices, the list root, the
// change's status rule and every refusal are withdrawals_row.h, the one text the kernels and the host-compiled test share.
// Synchronous, one GPU; a call's inputs and scratch are one Layout in d_withdrawals.
#include "engine_internal.h"
#include "withdrawals_row.h"

using namespace posevo;

static_assert(sizeof(pe_withdrawal) == 4 * WD_WORDS && sizeof(pe_withdrawal) == 44 && offsetof(pe_withdrawal, validator_index) == 8 &&
              offsetof(pe_withdrawal, address) == 16 && offsetof(pe_withdrawal, amount) == 36,
              "withdrawals_row.h: a withdrawal is pe_withdrawal in 11 words");
static_assert(sizeof(pe_bls_change) == 4 * CRED_CHANGE_WORDS && offsetof(pe_bls_change, from_bls_pubkey) == 8 &&
              offsetof(pe_bls_change, to_execution_address) == 56 && offsetof(pe_bls_change, flags) == 76,
              "withdrawals_row.h: a change is pe_bls_change in 20 words");
static_assert(sizeof(pe_withdrawals_params) == sizeof(WithdrawalsParams), "withdrawals_row.h: WithdrawalsParams is pe_withdrawals_params");
static_assert(WD_OK == PE_WD_OK && WD_COUNT_MISMATCH == PE_WD_COUNT_MISMATCH && WD_INDEX_MISMATCH == PE_WD_INDEX_MISMATCH &&
              WD_VALIDATOR_MISMATCH == PE_WD_VALIDATOR_MISMATCH && WD_ADDRESS_MISMATCH == PE_WD_ADDRESS_MISMATCH &&
              WD_AMOUNT_MISMATCH == PE_WD_AMOUNT_MISMATCH, "withdrawals_row.h: WD_* are the PE_WD_* of include/posevo.h");
static_assert(CRED_OK == PE_CRED_OK && CRED_BAD_INDEX == PE_CRED_BAD_INDEX && CRED_NOT_BLS == PE_CRED_NOT_BLS &&
              CRED_PUBKEY_MISMATCH == PE_CRED_PUBKEY_MISMATCH && CRED_BAD_SIGNATURE == PE_CRED_BAD_SIGNATURE &&
              CRED_FLAG_SIGNATURE_VALID == PE_CRED_FLAG_SIGNATURE_VALID, "withdrawals_row.h: CRED_* are the PE_CRED_* of include/posevo.h");

extern "C" {

void pe_withdrawals_params_default(pe_withdrawals_params* out)
{
    if (!out) return;
    out->max_effective_balance = 32000000000ull;
    out->max_withdrawals_per_payload = 16;
    out->max_validators_per_sweep = 16384;
    out->eth1_prefix = 0x01;
}

int pe_process_withdrawals(pe_engine* h, uint64_t current_epoch, uint64_t next_withdrawal_index, uint64_t next_withdrawal_validator_index,
                           const pe_withdrawals_params* params, const pe_withdrawal* payload, uint32_t n_payload, uint32_t flags,
                           pe_withdrawal* out_withdrawals, pe_withdrawals_result* out)
{
    const bool have_payload = flags & PE_WD_PAYLOAD, apply = flags & PE_WD_APPLY;
    if (!h || !params || !out || (have_payload && n_payload && !payload)) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));
    static const char who[] = "pe_process_withdrawals";
    if (h->dist_ready()) return refuse_dist(h, who);
    if (!h->epochs_set) return fail(h, PE_ERR_STATE, std::string(who) + ": no registry epochs (pe_registry_set_epochs first)");
    if (!h->balances_set) return fail(h, PE_ERR_STATE, std::string(who) + ": no resident balances (pe_state_set_balances first)");
    if (!h->static_set) return fail(h, PE_ERR_STATE, std::string(who) + ": no resident credentials (pe_registry_set_static first)");
    const uint64_t n = h->n_val;
    if (h->state_view_set && n && h->d_sbalance.cap < 8 * n)
        return fail(h, PE_ERR_STATE, std::string(who) + ": the working-state view does not cover the registry");
    if (n >= 0x100000000ull) return fail(h, PE_ERR_CAPACITY, std::string(who) + ": 2^32 or more validators");
    if (flags & ~(PE_WD_APPLY | PE_WD_PAYLOAD)) return fail(h, PE_ERR_INVALID_ARG, std::string(who) + ": unknown flag bits");
    if (apply && !have_payload) return fail(h, PE_ERR_INVALID_ARG, std::string(who) + ": PE_WD_APPLY without PE_WD_PAYLOAD");
    WithdrawalsParams P;
    memcpy(&P, params, sizeof P);
    static const char* const refusal[] = {"", "the registry is empty", "next_withdrawal_validator_index lies outside the registry",
                                          "a parameter is 0", "eth1_prefix is not one byte", "max_withdrawals_per_payload above 64",
                                          "the payload holds more than max_withdrawals_per_payload withdrawals",
                                          "next_withdrawal_index + max_withdrawals_per_payload exceeds 64 bits"};
    if (const int rc = withdrawals_check_params(P, n, next_withdrawal_validator_index, next_withdrawal_index, have_payload, n_payload))
        return fail(h, PE_ERR_INVALID_ARG, std::string(who) + ": " + refusal[rc]);

    WithdrawalsSweep S;
    S.n = n;
    S.start = next_withdrawal_validator_index;
    S.current_epoch = current_epoch;
    S.max_effective_balance = P.max_effective_balance;
    S.next_index = next_withdrawal_index;
    S.bound = (uint32_t)withdrawals_bound(n, P.max_validators_per_sweep);
    S.k = (uint32_t)P.max_withdrawals_per_payload;
    S.prefix = (uint32_t)P.eth1_prefix;
    const uint32_t n_wg = withdrawals_workgroups(S.bound);

    // ---- the call's scratch; the total and the records travel as ONE copy out
    Layout L;
    const auto r_kind = L.take<uint8_t>(S.bound);
    const auto r_wg_count = L.take<uint32_t>(n_wg), r_wg_off = L.take<uint32_t>(n_wg);
    const auto r_out = L.take<uint32_t>(4 + (size_t)WD_RECORD_WORDS * WD_MAX_PER_PAYLOAD);
    const auto r_total = r_out.part<uint32_t>(0, 1), r_records = r_out.part<uint32_t>(16, (size_t)WD_RECORD_WORDS * WD_MAX_PER_PAYLOAD);
    Workspace w;
    HIP_TRY(h, w.bind(h->d_withdrawals, L, h->stream));

    // ---- the read-only passes
    WithdrawalsColumns C;
    C.credentials = h->d_withdrawal_credentials.as<uint32_t>();
    C.withdrawable = h->d_withdrawable.as<uint64_t>();
    C.eff_balance = h->state_view_set ? h->d_sbalance.as<uint64_t>() : h->d_balance.as<uint64_t>();
    C.balances = h->d_rbalance.as<uint64_t>();
    launch_withdrawals_sweep(h->stream, C, S, w(r_kind), w(r_wg_count), w(r_wg_off), w(r_total), w(r_records));
    HIP_TRY(h, hipGetLastError());
    std::vector<uint32_t> got(r_out.count);
    HIP_TRY(h, w.get(r_out, got.data(), got.size()));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (got[0] > S.bound) return fail(h, PE_ERR_NO_DEVICE, "the withdrawal sweep counted more hits than positions");

    // ---- host step: the expected list, the payload's asserts, the next indices, the list root -- before anything is written
    const uint32_t count = std::min(got[0], S.k);
    uint32_t list[WD_WORDS * WD_MAX_PER_PAYLOAD], pay[WD_WORDS * WD_MAX_PER_PAYLOAD];
    if (have_payload && n_payload) memcpy(pay, payload, 4ull * WD_WORDS * n_payload);  // a packed struct: no alignment to rely on
    WithdrawalsOutcome o;
    withdrawals_outcome(P, n, S.start, next_withdrawal_index, got.data() + 4, count, list, pay, have_payload, n_payload, &o);
    pe_withdrawals_result res;
    memset(&res, 0, sizeof res);
    res.next_withdrawal_index = o.next_withdrawal_index;
    res.next_withdrawal_validator_index = o.next_withdrawal_validator_index;
    res.n_full = o.n_full;
    res.n_partial = o.n_partial;
    res.total_gwei = o.total_gwei;
    res.n_withdrawals = count;
    res.status = (int32_t)o.status;
    res.first_mismatch = o.first_mismatch;
    for (int k = 0; k < 8; ++k) {
        const uint32_t be = __builtin_bswap32(o.root[k]);
        memcpy(res.withdrawals_root + 4 * k, &be, 4);
    }
    if (out_withdrawals && count) memcpy(out_withdrawals, list, 4ull * WD_WORDS * count);

    // ---- the one writing pass
    if (apply && o.status == WD_OK) {
        launch_withdrawals_apply(h->stream, w(r_records), count, n, h->d_rbalance.as<uint64_t>());
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        res.applied = 1;
    }
    *out = res;
    return PE_OK;
}

int pe_process_bls_to_execution_changes(pe_engine* h, const pe_bls_change* changes, uint32_t n_changes, int32_t* status,
                                        pe_bls_changes_stats* out_stats)
{
    if (!h || (n_changes && (!changes || !status))) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));
    static const char who[] = "pe_process_bls_to_execution_changes";
    if (h->dist_ready()) return refuse_dist(h, who);
    if (!h->static_set) return fail(h, PE_ERR_STATE, std::string(who) + ": no resident credentials (pe_registry_set_static first)");
    const uint64_t n = h->n_val;
    if (n >= 0x100000000ull) return fail(h, PE_ERR_CAPACITY, std::string(who) + ": 2^32 or more validators");
    pe_bls_changes_stats stats;
    memset(&stats, 0, sizeof stats);
    if (n_changes == 0) {
        if (out_stats) *out_stats = stats;
        return PE_OK;
    }

    Layout L;
    const auto r_changes = L.take<uint32_t>((size_t)CRED_CHANGE_WORDS * n_changes);
    const auto r_first = L.take<uint32_t>(std::max<uint64_t>(n, 1));
    const auto r_checks = L.take<uint32_t>(n_changes), r_status = L.take<uint32_t>(n_changes);
    Workspace w;
    HIP_TRY(h, w.bind(h->d_withdrawals, L, h->stream));
    HIP_TRY(h, w.put(r_changes, changes, r_changes.count));
    HIP_TRY(h, w.fill(r_first, 0xFF, r_first.count));  // CRED_NONE

    // ---- the read-only passes
    launch_bls_changes_resolve(h->stream, w(r_changes), n_changes, h->d_withdrawal_credentials.as<uint8_t>(), n, w(r_first), w(r_checks),
                               w(r_status));
    HIP_TRY(h, hipGetLastError());
    std::vector<uint32_t> st(n_changes);
    HIP_TRY(h, w.get(r_status, st.data(), n_changes));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (uint32_t i = 0; i < n_changes; ++i) {
        status[i] = (int32_t)st[i];
        stats.n_invalid += st[i] != CRED_OK;
    }

    // ---- the one writing pass: an invalid block leaves nothing
    if (!stats.n_invalid) {
        launch_bls_changes_apply(h->stream, w(r_changes), n_changes, w(r_status), n, h->d_withdrawal_credentials.as<uint8_t>());
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        stats.n_applied = n_changes;
    }
    if (out_stats) *out_stats = stats;
    return PE_OK;
}

int pe_bls_change_signing_roots(pe_engine* h, const pe_bls_change* changes, uint32_t n, const uint8_t domain[32], uint8_t* out_roots32)
{
    if (!h || !domain || (n && (!changes || !out_roots32))) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));
    if (h->dist_ready()) return refuse_dist(h, "pe_bls_change_signing_roots");
    if (n == 0) return PE_OK;
    Layout L;
    const auto r_changes = L.take<uint32_t>((size_t)CRED_CHANGE_WORDS * n), r_roots = L.take<uint32_t>(8ull * n);
    Workspace w;
    HIP_TRY(h, w.bind(h->d_withdrawals, L, h->stream));
    HIP_TRY(h, w.put(r_changes, changes, r_changes.count));
    uint32_t dom[8];
    be32_words(domain, dom);
    launch_bls_change_signing_roots(h->stream, w(r_changes), n, dom, w(r_roots));
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, w.get(r_roots, out_roots32, 8ull * n));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return PE_OK;
}

}  // extern "C"
