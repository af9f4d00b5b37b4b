// engine_block_ops.cpp -- pe_process_block_operations: proposer slashings, attester slashings and voluntary exits over the
// resident registry (process_proposer_slashing, process_attester_slashing, process_voluntary_exit with slash_validator and
// initiate_validator_exit under them, restated in tests/block_ops_model.py).  The pattern of pe_registry_updates: read-only
// passes (block_ops_kernels.hip and k_registry_census), a host step, one writing pass.  What an operation's own fields
// decide, the scalars and every refusal are block_ops_row.h, the one text the kernels and the host-compiled test share.
// Synchronous, one GPU; the call's inputs and scratch are one Layout in d_block_ops.
#include "block_ops_row.h"
#include "engine_internal.h"

using namespace posevo;

static_assert(sizeof(pe_block_op) == sizeof(BlockOpHost) && sizeof(pe_block_op) == 408 &&
              offsetof(pe_block_op, data_2) == offsetof(BlockOpHost, data_2) &&
              offsetof(pe_block_op, indices_1_offset) == offsetof(BlockOpHost, indices_1_offset) &&
              offsetof(pe_block_op, header_1_root) == offsetof(BlockOpHost, header_1_root) &&
              offsetof(pe_block_op, header_2_slot) == offsetof(BlockOpHost, header_2_slot) &&
              offsetof(pe_block_op, validator_index) == offsetof(BlockOpHost, validator_index) &&
              offsetof(pe_block_op, exit_epoch) == offsetof(BlockOpHost, exit_epoch),
              "block_ops_row.h: BlockOpHost is pe_block_op field for field");
static_assert(sizeof(pe_block_ops_params) == sizeof(BlockOpsParams), "block_ops_row.h: BlockOpsParams is pe_block_ops_params");
static_assert(BLOCK_OP_PROPOSER_SLASHING == PE_OP_PROPOSER_SLASHING && BLOCK_OP_ATTESTER_SLASHING == PE_OP_ATTESTER_SLASHING &&
              BLOCK_OP_VOLUNTARY_EXIT == PE_OP_VOLUNTARY_EXIT && BLOCK_OP_FLAG_SIGNATURE_VALID == PE_OP_FLAG_SIGNATURE_VALID &&
              BLOCK_OP_OK == PE_OP_OK && BLOCK_OP_NOT_SLASHABLE_DATA == PE_OP_NOT_SLASHABLE_DATA &&
              BLOCK_OP_BAD_INDICES == PE_OP_BAD_INDICES && BLOCK_OP_BAD_SIGNATURE == PE_OP_BAD_SIGNATURE &&
              BLOCK_OP_NOBODY_SLASHABLE == PE_OP_NOBODY_SLASHABLE && BLOCK_OP_HEADER_MISMATCH == PE_OP_HEADER_MISMATCH &&
              BLOCK_OP_PROPOSER_NOT_SLASHABLE == PE_OP_PROPOSER_NOT_SLASHABLE && BLOCK_OP_NOT_ACTIVE == PE_OP_NOT_ACTIVE &&
              BLOCK_OP_ALREADY_EXITING == PE_OP_ALREADY_EXITING && BLOCK_OP_EXIT_EPOCH_FUTURE == PE_OP_EXIT_EPOCH_FUTURE &&
              BLOCK_OP_TOO_YOUNG == PE_OP_TOO_YOUNG, "block_ops_row.h: BLOCK_OP_* are the PE_OP_* of include/posevo.h");
static_assert(REWARD_VAL_SLASHED == PE_VAL_SLASHED, "reward_row.h: the view's slashed bit");

extern "C" {

void pe_block_ops_params_default(pe_block_ops_params* out)
{
    if (!out) return;
    pe_registry_params r;
    pe_registry_params_default(&r);
    out->min_slashing_penalty_quotient = 32;  // MIN_SLASHING_PENALTY_QUOTIENT_BELLATRIX; Altair's own is 64
    out->whistleblower_reward_quotient = 512;
    out->epochs_per_slashings_vector = 8192;
    out->shard_committee_period = 256;
    out->min_validator_withdrawability_delay = r.min_validator_withdrawability_delay;
    out->max_seed_lookahead = r.max_seed_lookahead;
    out->min_per_epoch_churn_limit = r.min_per_epoch_churn_limit;
    out->churn_limit_quotient = r.churn_limit_quotient;
}

int pe_process_block_operations(pe_engine* h, uint64_t current_epoch, uint32_t proposer_index, const pe_block_op* ops, uint32_t n_ops,
                                const uint32_t* indices, uint64_t n_indices, const pe_block_ops_params* params, int32_t* status,
                                pe_block_ops_stats* out_stats)
{
    if (!h || !params || (n_ops && (!ops || !status)) || (n_indices && !indices)) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));
    static const char who[] = "pe_process_block_operations";
    if (h->dist_ready()) return refuse_dist(h, who);
    if (!h->epochs_set) return fail(h, PE_ERR_STATE, std::string(who) + ": no registry epochs (pe_registry_set_epochs first)");
    if (!h->balances_set) return fail(h, PE_ERR_STATE, std::string(who) + ": no resident balances (pe_state_set_balances first)");
    const uint64_t n = h->n_val;
    if (h->state_view_set && n && (h->d_sbalance.cap < 8 * n || h->d_sflags.cap < n))
        return fail(h, PE_ERR_STATE, std::string(who) + ": the working-state view does not cover the registry");
    if (proposer_index >= n) return fail(h, PE_ERR_INVALID_ARG, std::string(who) + ": proposer_index lies outside the registry");
    BlockOpsParams P;
    memcpy(&P, params, sizeof P);
    static const char* const refusal[] = {
        "", "a quotient is 0", "current_epoch + epochs_per_slashings_vector reaches FAR_FUTURE_EPOCH",
        "current_epoch + 1 + max_seed_lookahead reaches FAR_FUTURE_EPOCH", "the churn limit is 0 (min_per_epoch_churn_limit)",
        "the last exit epoch + min_validator_withdrawability_delay reaches FAR_FUTURE_EPOCH",
        "the slashed balance and the proposer's rewards can exceed 64 bits"};
    if (const int rc = block_ops_check_params(P, current_epoch)) return fail(h, PE_ERR_INVALID_ARG, std::string(who) + ": " + refusal[rc]);
    if (n_indices >= BLOCK_OPS_MAX_SLOTS) return fail(h, PE_ERR_CAPACITY, std::string(who) + ": 2^31 or more indices");

    // ---- what the operations' own fields decide; the slots
    std::vector<BlockOpDev> dev(std::max<uint32_t>(n_ops, 1));
    std::vector<uint32_t> host_status(n_ops), slot_off((size_t)n_ops + 1, 0);
    uint64_t total_slots = 0;
    for (uint32_t o = 0; o < n_ops; ++o) {
        const int rc = block_ops_prepare(*reinterpret_cast<const BlockOpHost*>(&ops[o]), n, n_indices, current_epoch, &dev[o],
                                         &host_status[o]);
        if (rc)
            return fail(h, PE_ERR_INVALID_ARG, std::string(who) + (rc == 1 ? ": an operation of unknown kind"
                                                                           : ": an index range runs past n_indices"));
        slot_off[o] = (uint32_t)total_slots;
        total_slots += block_ops_slots(dev[o], host_status[o]);
        if (total_slots >= BLOCK_OPS_MAX_SLOTS) return fail(h, PE_ERR_CAPACITY, std::string(who) + ": 2^31 or more candidate slots");
    }
    slot_off[n_ops] = (uint32_t)total_slots;
    const uint32_t n_slots = (uint32_t)total_slots;
    const uint32_t n_wg = block_ops_workgroups(n_slots);

    PE_TRY(materialise_state_view(h));  // the view still mirrors the registry: a view of its own first, flags included

    // ---- the call's inputs and scratch
    Layout L;
    const auto r_ops = L.take<BlockOpDev>(dev.size());
    const auto r_slot_off = L.take<uint32_t>(slot_off.size());
    const auto r_indices = L.take<uint32_t>(std::max<uint64_t>(n_indices, 1));
    const auto r_slot_val = L.take<uint32_t>((size_t)n_slots + 1), r_slot_op = L.take<uint32_t>((size_t)n_slots + 1);
    const auto r_slot_ev = L.take<uint8_t>((size_t)n_slots + 1);
    const auto r_op_words = L.take<uint32_t>(3 * (size_t)std::max<uint32_t>(n_ops, 1));  // bad | hit | status: one fill, one copy out
    const auto r_op_bad = r_op_words.part<uint32_t>(0, n_ops), r_op_hit = r_op_words.part<uint32_t>(4ull * n_ops, n_ops),
               r_op_status = r_op_words.part<uint32_t>(8ull * n_ops, n_ops);
    const auto r_first = L.take<uint32_t>(2 * n);  // first_potent | first_slash
    const auto r_wg_part = L.take<BlockOpsWgPart>(n_wg);
    const auto r_wg_off = L.take<BlockOpsWgOffset>(n_wg);
    const auto r_totals = L.take<BlockOpsTotals>(1);
    const auto r_census = L.take<RegistryTotals>(1);
    const auto r_sums = L.take<uint64_t>(2);
    Workspace w;
    HIP_TRY(h, w.bind(h->d_block_ops, L, h->stream));
    HIP_TRY(h, h->d_registry_wg.ensure(std::max<size_t>(64, registry_scratch_bytes(n))));
    HIP_TRY(h, w.put(r_ops, dev.data(), dev.size()));
    HIP_TRY(h, w.put(r_slot_off, slot_off.data(), slot_off.size()));
    if (n_indices) HIP_TRY(h, w.put(r_indices, indices, n_indices));
    HIP_TRY(h, w.zero(r_op_words, r_op_words.count));
    HIP_TRY(h, w.fill(r_first, 0xFF, 2 * n));  // BLOCK_OPS_NONE
    HIP_TRY(h, w.zero(r_sums, 2));

    // ---- the read-only passes
    uint64_t* const d_act = h->d_activation_epoch.as<uint64_t>();
    uint64_t* const d_exit = h->d_exit_epoch.as<uint64_t>();
    BlockOpsRegistry R;
    R.activation_epoch = d_act;
    R.exit_epoch = d_exit;
    R.withdrawable = h->d_withdrawable.as<uint64_t>();
    R.eff_balance = h->d_sbalance.as<uint64_t>();
    R.balances = h->d_rbalance.as<uint64_t>();
    R.sflags = h->d_sflags.as<uint8_t>();
    uint32_t* const d_first_potent = w(r_first);
    uint32_t* const d_first_slash = w(r_first) + n;
    const U64Div by_reward = u64_div_make(P.whistleblower_reward_quotient);
    launch_block_ops_lists(h->stream, w(r_ops), w(r_slot_off), n_ops, w(r_indices), n, n_slots, w(r_slot_val), w(r_slot_op), w(r_op_bad));
    HIP_TRY(h, hipGetLastError());
    launch_block_ops_resolve(h->stream, w(r_ops), w(r_slot_val), w(r_slot_op), w(r_op_bad), n_slots, R, current_epoch,
                             P.shard_committee_period, by_reward, d_first_potent, d_first_slash, w(r_slot_ev), w(r_op_status),
                             w(r_op_hit), w(r_wg_part), w(r_wg_off), proposer_index, w(r_totals));
    HIP_TRY(h, hipGetLastError());
    // the exit queue's end and the active count: k_registry_census.  Of its four predicates the active one and the (largest
    // exit epoch, holders) pair are read here; its eligibility column is not, so the exit epochs stand in for it.
    launch_registry_census(h->stream, d_exit, d_act, d_exit, h->d_sbalance.as<uint64_t>(), n, current_epoch, 0, 0, 0,
                           h->d_registry_wg.p, w(r_census));
    HIP_TRY(h, hipGetLastError());
    std::vector<uint32_t> op_words(r_op_words.count);
    BlockOpsTotals tot;
    RegistryTotals census;
    HIP_TRY(h, w.get(r_op_words, op_words.data(), op_words.size()));
    HIP_TRY(h, w.get(r_totals, &tot, 1));
    HIP_TRY(h, w.get(r_census, &census, 1));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (census.n_active > n || census.n_at_max > n || tot.n_fresh > n_slots || tot.n_slashed > n_slots)
        return fail(h, PE_ERR_NO_DEVICE, "the block operations' read-only passes counted more validators than there are");

    // ---- host step: the statuses, the limits, the exit queue's closed form, every refusal -- before anything is written
    pe_block_ops_stats stats;
    memset(&stats, 0, sizeof stats);
    std::vector<int32_t> st(n_ops);
    const uint32_t *op_bad = op_words.data(), *op_hit = op_bad + n_ops, *op_status = op_hit + n_ops;
    for (uint32_t o = 0; o < n_ops; ++o) {
        uint32_t s = host_status[o];
        if (s == BLOCK_OP_OK) {
            if (dev[o].kind != BLOCK_OP_ATTESTER_SLASHING) s = op_status[o];
            else if (op_bad[o]) s = BLOCK_OP_BAD_INDICES;
            else if (!(dev[o].pre & BLOCK_OP_PRE_OK)) s = BLOCK_OP_BAD_SIGNATURE;
            else if (!op_hit[o]) s = BLOCK_OP_NOBODY_SLASHABLE;
        }
        st[o] = (int32_t)s;
        stats.n_invalid += s != BLOCK_OP_OK;
    }
    if (stats.n_invalid) memset(&tot, 0, sizeof tot);  // an invalid block: the limits alone, nothing is written
    BlockOpsScalars S;
    uint64_t last_exit = 0;
    if (const int rc = block_ops_scalars_make(P, current_epoch, proposer_index, n_slots, census.n_active, census.max_exit,
                                              census.n_at_max, tot, &S, &stats.churn_limit, &last_exit))
        return fail(h, PE_ERR_INVALID_ARG, std::string(who) + ": " + refusal[rc]);
    stats.n_active = census.n_active;
    if (n_ops) memcpy(status, st.data(), 4ull * n_ops);
    if (stats.n_invalid) {
        if (out_stats) *out_stats = stats;
        return PE_OK;
    }
    stats.n_slashed = tot.n_slashed;
    stats.n_exits_initiated = tot.n_fresh;
    stats.first_exit_epoch = tot.n_fresh ? S.exit_base : 0;
    stats.last_exit_epoch = last_exit;
    stats.slashed_balance = tot.slashed_balance;
    stats.proposer_rewards = tot.rewards;

    // ---- the one writing pass
    if (tot.n_fresh || tot.n_slashed) {
        launch_block_ops_apply(h->stream, S, w(r_slot_val), w(r_slot_ev), w(r_wg_off), d_first_slash, h->d_sbalance.as<uint64_t>(),
                               d_exit, h->d_withdrawable.as<uint64_t>(), h->d_sflags.as<uint8_t>(), h->d_rbalance.as<uint64_t>(),
                               w(r_sums));
        HIP_TRY(h, hipGetLastError());
        uint64_t sums[2] = {0, 0};
        HIP_TRY(h, w.get(r_sums, sums, 2));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        stats.penalties = sums[0];
        stats.n_saturated = sums[1];
        if (tot.n_fresh) h->active_valid = false;  // compacted from the previous exit epochs
    }
    if (out_stats) *out_stats = stats;
    return PE_OK;
}

}  // extern "C"
