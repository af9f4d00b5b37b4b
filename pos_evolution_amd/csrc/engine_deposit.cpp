// engine_deposit.cpp -- process_deposit (pe:139-175) over the resident registry.
//   pe_deposit_signing_roots  compute_signing_root(DepositMessage, domain) of every deposit: what the caller hashes to the curve
//   pe_process_deposits       the whole function for a batch, with the reference's sequential semantics: k_deposit_leaves (the
//                             leaves and the branch walk), k_deposit_probe against the pubkey index the handle keeps over
//                             d_pubkey_leaf (k_deposit_index_build), the signature verdicts of the keys the registry lacks --
//                             every deposit of a new key once, through pe_g1_decompress + pe_g1_key_validate, pe_g2_decompress +
//                             pe_g2_subgroup_check and pairing_run over (pk, H(m)), (-g1, sig): existing code, called --,
//                             k_deposit_resolve (duplicates inside the batch, statuses, new indices), registry_grow and
//                             k_deposit_apply
//   registry_grow             the resident per-validator columns (reg_columns.h) extended with their contents kept
// The rules per deposit are deposit_row.h.  Synchronous, one GPU.
#include "engine_internal.h"
#include "deposit_row.h"

using namespace posevo;

static_assert(sizeof(pe_deposit_data) == 4 * DEPOSIT_ROW_WORDS && offsetof(pe_deposit_data, withdrawal_credentials) == 48 &&
              offsetof(pe_deposit_data, amount) == 80 && offsetof(pe_deposit_data, signature) == 88,
              "deposit_row.h reads pe_deposit_data as 46 words: pubkey 12 | credentials 8 | amount 2 | signature 24");
static_assert(DEPOSIT_APPENDED == PE_DEP_APPENDED && DEPOSIT_TOPUP == PE_DEP_TOPUP &&
              DEPOSIT_IGNORED_BAD_SIGNATURE == PE_DEP_IGNORED_BAD_SIGNATURE && DEPOSIT_BAD_PROOF == PE_DEP_BAD_PROOF,
              "deposit_row.h: DEPOSIT_* are the pe_deposit_status of include/posevo.h");
static_assert(sizeof(DepositParams) == sizeof(pe_deposit_params), "deposit_row.h: DepositParams is pe_deposit_params");
static_assert(DEPOSIT_NONE == NONE32, "deposit_row.h: its empty slot is the engine's NONE32");

namespace posevo {

namespace {

// The pubkey index covers the registry and leaves room for n_more keys: built where there is none, rebuilt larger where a
// call outgrows it, otherwise extended by the validators appended since (none, unless an earlier call failed half-way).
int ensure_pubkey_index(pe_engine* h, uint64_t n_more)
{
    const uint64_t n = h->n_val;
    const uint32_t want = deposit_index_slots(n + n_more);
    if (2 * (n + n_more) > (uint64_t)want) return fail(h, PE_ERR_CAPACITY, "pe_process_deposits: the pubkey index cannot hold the registry");
    if (h->dep_index_slots && h->dep_index_slots >= want && h->dep_index_keys <= n) {
        if (h->dep_index_keys < n) {
            launch_deposit_index_build(h->stream, h->d_pubkey_leaf.as<uint32_t>(), h->dep_index_keys, n, nullptr,
                                       h->d_dep_index.as<uint32_t>(), h->dep_index_slots - 1, nullptr);
            HIP_TRY(h, hipGetLastError());
            h->dep_index_keys = n;
        }
        return PE_OK;
    }
    h->dep_index_slots = 0;
    HIP_TRY(h, h->d_dep_index.ensure(4ull * want));
    hipEvent_t t0 = ProfScope::take(h), t1 = ProfScope::take(h);
    if (t0 && t1) (void)hipEventRecord(t0, h->stream);
    HIP_TRY(h, hipMemsetAsync(h->d_dep_index.p, 0xFF, 4ull * want, h->stream));
    launch_deposit_index_build(h->stream, h->d_pubkey_leaf.as<uint32_t>(), 0, n, nullptr, h->d_dep_index.as<uint32_t>(), want - 1,
                               nullptr);
    HIP_TRY(h, hipGetLastError());
    if (t0 && t1) (void)hipEventRecord(t1, h->stream);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (t0 && t1) (void)hipEventElapsedTime(&h->dep_index_build_ms, t0, t1);
    if (t0) h->event_pool.push_back(t0);
    if (t1) h->event_pool.push_back(t1);
    h->dep_index_slots = want;
    h->dep_index_keys = n;
    return PE_OK;
}

// bls.Verify(pubkey, signing_root, signature) of the deposits `miss` names: sig_ok[i] = 1 where it holds.  pk96: the decoded
// keys, 96 bytes per entry of miss (zero rows where a key does not decode).
int deposit_signature_verdicts(pe_engine* h, const pe_deposit_data* deps, const std::vector<uint32_t>& miss,
                               const uint8_t* message_points192, std::vector<uint32_t>& sig_ok, std::vector<uint8_t>& pk96)
{
    const uint64_t m = miss.size();
    pk96.assign(96 * m, 0);
    if (m == 0) return PE_OK;
    std::vector<uint8_t> pk48(48 * m), sig96(96 * m), sig192(192 * m);
    for (uint64_t j = 0; j < m; ++j) {
        memcpy(&pk48[48 * j], deps[miss[j]].pubkey, 48);
        memcpy(&sig96[96 * j], deps[miss[j]].signature, 96);
    }
    std::vector<int32_t> st_pk(m), st_kv(m), st_sig(m), st_sub(m);
    PE_TRY(pe_g1_decompress(h, pk48.data(), m, pk96.data(), st_pk.data()));
    PE_TRY(pe_g1_key_validate(h, pk96.data(), m, st_kv.data()));        // KeyValidate: in G1 and not the identity
    PE_TRY(pe_g2_decompress(h, sig96.data(), m, sig192.data(), st_sig.data()));
    PE_TRY(pe_g2_subgroup_check(h, sig192.data(), m, st_sub.data()));
    std::vector<uint32_t> good;
    for (uint64_t j = 0; j < m; ++j)
        if (st_pk[j] == 0 && st_kv[j] == 0 && st_sig[j] == 0 && st_sub[j] == 0) good.push_back((uint32_t)j);
    if (good.empty()) return PE_OK;
    std::vector<int32_t> verdict(good.size());
    PE_TRY(verify_pairs_run(
        h, "pe_process_deposits", (uint32_t)good.size(), [&](uint32_t t) { return &pk96[(size_t)96 * good[t]]; },
        [&](uint32_t t) { return message_points192 + (size_t)192 * miss[good[t]]; },
        [&](uint32_t t) { return &sig192[(size_t)192 * good[t]]; }, verdict.data()));
    for (size_t t = 0; t < good.size(); ++t)
        if (verdict[t] == PE_BLS_VALID) sig_ok[miss[good[t]]] = 1;
    return PE_OK;
}

}  // namespace

int registry_grow(pe_engine* h, uint64_t n_new)
{
    const uint64_t n_old = h->n_val;
    if (n_new <= n_old) return PE_OK;
    if (n_new >= 0xFFFFFFFFull) return fail(h, PE_ERR_CAPACITY, "validator index must fit 32 bits");
    committee_sums_drop(h);  // sums over a registry of the old size; a build in flight has read the points before they move
    const uint64_t cap = reg_grown_capacity(h->reg_capacity, n_old, n_new);
    HIP_TRY(h, reg_ensure(h, reg_held(h), cap, /*keep=*/true));
    h->reg_capacity = cap;
    HIP_TRY(h, reg_fill(h, reg_held(h), n_old, n_new));
    if (h->d_totals.p) HIP_TRY(h, hipMemsetAsync(h->d_totals.p, 0, h->d_totals.cap, h->stream));  // k_votes' grid changes with n
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->h_flags.resize(n_new, 0);
    h->active_valid = false;  // get_active_validator_indices of the old registry
    h->n_val = n_new;
    return PE_OK;
}

}  // namespace posevo

extern "C" {

void pe_deposit_params_default(pe_deposit_params* out)
{
    if (!out) return;
    out->effective_balance_increment = 1000000000ull;
    out->max_effective_balance = 32000000000ull;
    out->far_future_epoch = ~0ull;
}

int pe_profile_deposit_index(const pe_engine* h, uint32_t* out_slots, uint64_t* out_keys, float* out_build_ms)
{
    if (!h) return PE_ERR_INVALID_ARG;
    if (out_slots) *out_slots = h->dep_index_slots;
    if (out_keys) *out_keys = h->dep_index_slots ? h->dep_index_keys : 0;
    if (out_build_ms) *out_build_ms = h->dep_index_build_ms;
    return PE_OK;
}

int pe_deposit_signing_roots(pe_engine* h, const pe_deposit_data* deposits, uint32_t n, const uint8_t domain[32],
                             uint8_t* out_roots32)
{
    if (!h || !domain || (n && (!deposits || !out_roots32))) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));
    if (h->dist_ready()) return refuse_dist(h, "pe_deposit_signing_roots");
    if (n == 0) return PE_OK;
    Layout L;
    const auto r_rows = L.take<uint32_t>((size_t)DEPOSIT_ROW_WORDS * n), r_leaf = L.take<uint32_t>(8ull * n);
    const auto r_ok = L.take<uint32_t>(n), r_roots = L.take<uint32_t>(8ull * n);
    Workspace w;
    HIP_TRY(h, w.bind(h->d_deposit, L, h->stream));
    HIP_TRY(h, w.put(r_rows, deposits, (size_t)DEPOSIT_ROW_WORDS * n));
    DepositLeavesArgs a{};
    a.rows = w(r_rows);
    a.n = n;
    be32_words(domain, a.domain);
    a.leaf = w(r_leaf);
    a.proof_ok = w(r_ok);
    a.signing_roots = w(r_roots);
    launch_deposit_leaves(h->stream, a);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, w.get(r_roots, out_roots32, 8ull * n));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return PE_OK;
}

int pe_process_deposits(pe_engine* h, const pe_deposit_data* deposits, uint32_t n, const uint8_t* proofs,
                        uint64_t eth1_deposit_index, const uint8_t deposit_root[32], const uint8_t* message_points192,
                        const pe_deposit_params* params, int32_t* status, uint32_t* out_index, pe_deposit_stats* out)
{
    if (!h || !params || (n && (!deposits || !status)) || (proofs && !deposit_root)) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));
    if (h->dist_ready()) return refuse_dist(h, "pe_process_deposits");
    if (h->slasher.enabled)
        return fail(h, PE_ERR_STATE, "pe_process_deposits: the slasher is enabled and its history is sized for the present registry "
                                     "(pe_slasher_disable first)");
    if (!h->static_set) return fail(h, PE_ERR_STATE, "pe_process_deposits: no static registry part (pe_registry_set_static first)");
    if (!h->balances_set) return fail(h, PE_ERR_STATE, "pe_process_deposits: no resident balances (pe_state_set_balances first)");
    if (!h->epochs_set) return fail(h, PE_ERR_STATE, "pe_process_deposits: no registry epochs (pe_registry_set_epochs first)");
    const DepositParams P{params->effective_balance_increment, params->max_effective_balance, params->far_future_epoch};
    if (P.effective_balance_increment == 0 || P.max_effective_balance / P.effective_balance_increment > 0xFFFF)
        return fail(h, PE_ERR_INVALID_ARG, "pe_process_deposits: increment 0, or max_effective_balance / increment exceeds 65535");
    for (uint32_t i = 0; i < n; ++i)
        if (deposits[i].amount > DEPOSIT_MAX_AMOUNT) return fail(h, PE_ERR_INVALID_ARG, "pe_process_deposits: an amount above 2^63");
    const uint64_t n_val = h->n_val;
    pe_deposit_stats stats{};
    stats.n_validators = n_val;
    if (out) *out = stats;
    if (n == 0) return PE_OK;
    if (n_val >= 0xFFFFFFFEull) return fail(h, PE_ERR_STATE, "pe_process_deposits: the registry is full");

    PE_TRY(ensure_pubkey_index(h, n));
    const uint32_t T2 = deposit_index_slots(n);
    Layout L;
    const auto r_rows = L.take<uint32_t>((size_t)DEPOSIT_ROW_WORDS * n);
    const auto r_proofs = L.take<uint32_t>(proofs ? (size_t)8 * DEPOSIT_PROOF_NODES * n : 0);
    const auto r_leaf = L.take<uint32_t>(8ull * n), r_ok = L.take<uint32_t>(n), r_reg = L.take<uint32_t>(n);
    const auto r_slot = L.take<uint32_t>(n), r_sig = L.take<uint32_t>(n), r_rank = L.take<uint32_t>(n);
    const auto r_tab = L.take<uint32_t>(T2), r_first = L.take<uint32_t>(T2), r_counts = L.take<uint32_t>(4);
    const auto r_status = L.take<int32_t>(n);
    const auto r_index = L.take<uint32_t>(n);
    Workspace w;
    HIP_TRY(h, w.bind(h->d_deposit, L, h->stream));
    HIP_TRY(h, w.put(r_rows, deposits, (size_t)DEPOSIT_ROW_WORDS * n));
    if (proofs) HIP_TRY(h, w.put(r_proofs, proofs, (size_t)8 * DEPOSIT_PROOF_NODES * n));
    HIP_TRY(h, w.fill(r_tab, 0xFF, T2));
    HIP_TRY(h, w.fill(r_first, 0xFF, T2));
    // 1. leaves, proofs, the registry's index, the batch's own table over the keys the registry lacks
    DepositLeavesArgs la{};
    la.rows = w(r_rows);
    la.n = n;
    la.proofs = proofs ? w(r_proofs) : nullptr;
    la.index0 = eth1_deposit_index;
    if (proofs) be32_words(deposit_root, la.root);
    la.leaf = w(r_leaf);
    la.proof_ok = w(r_ok);
    launch_deposit_leaves(h->stream, la);
    launch_deposit_probe(h->stream, w(r_leaf), n, h->d_pubkey_leaf.as<uint32_t>(), h->d_dep_index.as<uint32_t>(),
                         h->dep_index_slots - 1, w(r_reg));
    launch_deposit_index_build(h->stream, w(r_leaf), 0, n, w(r_reg), w(r_tab), T2 - 1, w(r_slot));
    HIP_TRY(h, hipGetLastError());
    std::vector<uint32_t> reg(n), proof_ok(n);
    HIP_TRY(h, w.get(r_reg, reg.data(), n));
    HIP_TRY(h, w.get(r_ok, proof_ok.data(), n));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    // 2. the signature verdicts of every deposit of a key the registry lacks
    std::vector<uint32_t> miss;
    for (uint32_t i = 0; i < n; ++i)
        if (reg[i] == NONE32) miss.push_back(i);
    if (!miss.empty() && !message_points192)
        return fail(h, PE_ERR_INVALID_ARG, "pe_process_deposits: a deposit of a new pubkey and no message points");
    std::vector<uint32_t> sig_ok(n, 0);
    std::vector<uint8_t> pk96;
    PE_TRY(deposit_signature_verdicts(h, deposits, miss, message_points192, sig_ok, pk96));
    // 3. duplicates inside the batch, statuses, new indices
    HIP_TRY(h, w.put(r_sig, sig_ok.data(), n));
    DepositResolveArgs ra{};
    ra.n = n;
    ra.n_val = (uint32_t)n_val;
    ra.reg_index = w(r_reg);
    ra.key_slot = w(r_slot);
    ra.sig_ok = w(r_sig);
    ra.proof_ok = w(r_ok);
    ra.first_valid = w(r_first);
    ra.rank = w(r_rank);
    ra.status = w(r_status);
    ra.out_index = w(r_index);
    ra.counts = w(r_counts);
    launch_deposit_resolve(h->stream, ra);
    HIP_TRY(h, hipGetLastError());
    std::vector<uint32_t> credited(n);
    HIP_TRY(h, w.get(r_status, status, n));
    HIP_TRY(h, w.get(r_index, credited.data(), n));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (uint32_t i = 0; i < n; ++i) {
        stats.n_appended += status[i] == PE_DEP_APPENDED;
        stats.n_topups += status[i] == PE_DEP_TOPUP;
        stats.n_ignored += status[i] == PE_DEP_IGNORED_BAD_SIGNATURE;
        stats.n_bad_proof += status[i] == PE_DEP_BAD_PROOF;
    }
    if (stats.n_bad_proof) {  // the reference's assert: the block is invalid, nothing of it is applied
        stats.n_appended = stats.n_topups = 0;
        if (out_index) std::fill(out_index, out_index + n, NONE32);
        if (out) *out = stats;
        return PE_OK;
    }
    const uint64_t n_new = n_val + stats.n_appended;
    if (n_new > 0xFFFFFFFEull) return fail(h, PE_ERR_STATE, "pe_process_deposits: the registry would grow beyond 2^32 - 2 validators");
    // 4. grow, apply
    if (stats.n_appended) {
        PE_TRY(materialise_state_view(h));  // the new rows' effective balances are the view's alone
        PE_TRY(registry_grow(h, n_new));
    }
    DepositApplyArgs aa{};
    aa.rows = w(r_rows);
    aa.n = n;
    aa.status = w(r_status);
    aa.out_index = w(r_index);
    aa.dep_leaf = w(r_leaf);
    aa.increment = P.effective_balance_increment;
    aa.max_effective_balance = P.max_effective_balance;
    aa.far_future_epoch = P.far_future_epoch;
    aa.balances = h->d_rbalance.as<uint64_t>();
    aa.eff_balance = h->d_sbalance.as<uint64_t>();
    aa.sflags = h->d_sflags.as<uint8_t>();
    aa.increments = h->d_incr.as<uint16_t>();
    aa.activation_eligibility = h->d_activation_eligibility.as<uint64_t>();
    aa.activation_epoch = h->d_activation_epoch.as<uint64_t>();
    aa.exit_epoch = h->d_exit_epoch.as<uint64_t>();
    aa.withdrawable_epoch = h->d_withdrawable.as<uint64_t>();
    aa.pubkey_leaf = h->d_pubkey_leaf.as<uint32_t>();
    aa.withdrawal_credentials = h->d_withdrawal_credentials.as<uint32_t>();
    launch_deposit_apply(h->stream, aa);
    HIP_TRY(h, hipGetLastError());
    if (stats.n_appended) {
        // the appended leaves enter the index (the table has room: ensure_pubkey_index counted every deposit of the call)
        launch_deposit_index_build(h->stream, h->d_pubkey_leaf.as<uint32_t>(), n_val, n_new, nullptr, h->d_dep_index.as<uint32_t>(),
                                   h->dep_index_slots - 1, nullptr);
        HIP_TRY(h, hipGetLastError());
        h->dep_index_keys = n_new;
        if (h->have_points) {  // the creators' decoded keys, in the order of their indices, behind the registry's points
            std::vector<uint8_t> rows96((size_t)96 * stats.n_appended);
            for (size_t j = 0; j < miss.size(); ++j) {
                const uint32_t i = miss[j];
                if (status[i] == PE_DEP_APPENDED) memcpy(&rows96[(size_t)96 * (credited[i] - n_val)], &pk96[96 * j], 96);
            }
            HIP_TRY(h, h->d_tmp_be.ensure(rows96.size()));
            HIP_TRY(h, hipMemcpyAsync(h->d_tmp_be.p, rows96.data(), rows96.size(), hipMemcpyHostToDevice, h->stream));
            launch_g1_convert(h->stream, h->d_tmp_be.as<uint8_t>(), h->d_points.as<uint32_t>() + (uint64_t)G1_ROW_WORDS * n_val,
                              stats.n_appended);
            if (h->points30_valid)
                launch_g1_table_s30(h->stream, h->d_points.as<uint32_t>() + (uint64_t)G1_ROW_WORDS * n_val,
                                    h->d_points30.as<uint32_t>() + (uint64_t)G1_ROW_WORDS * n_val, stats.n_appended);
            HIP_TRY(h, hipGetLastError());
        }
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (out_index) memcpy(out_index, credited.data(), 4ull * n);
    stats.n_validators = h->n_val;
    if (out) *out = stats;
    return PE_OK;
}

}  // extern "C"
