// engine_sync.cpp -- Altair's sync committee over the resident registry (the rules restated in
// tests/sync_committee_model.py).
//   pe_sync_committee_compute   get_next_sync_committee: k_sync_sample / k_sync_append in batches of SYNC_SAMPLE_BATCH candidates
//                               with a host step between them (one count word), then the aggregate key through pe_g1_sum
//   pe_sync_committee_set / _get / _rotate   the two resident committees: checkpoint / resume, genesis, the period boundary
//   pe_process_sync_aggregate   process_sync_aggregate for up to PE_SYNC_MAX_BATCH blocks: k_sync_members (participants, signing
//                               roots), the verdicts composed from existing calls as engine_deposit.cpp composes its own --
//                               pe_g1_sum, pe_hash_to_g2, pe_g2_decompress, pe_g2_subgroup_check, verify_pairs_run -- with
//                               eth_fast_aggregate_verify's special case and the identity rules on the host, then k_sync_rewards
// Synchronous, one GPU.  Nothing resident is written before every refusal has been decided.
#include "engine_internal.h"

using namespace posevo;

static_assert(sizeof(pe_sync_aggregate) == 4 * SYNC_AGG_WORDS && offsetof(pe_sync_aggregate, signature) == 64 &&
              offsetof(pe_sync_aggregate, block_root) == 160 && offsetof(pe_sync_aggregate, domain) == 192 &&
              offsetof(pe_sync_aggregate, proposer_index) == 224,
              "sync_kernels.hip reads pe_sync_aggregate as 58 words: bits 16 | signature 24 | block_root 8 | domain 8 | proposer 1 | pad 1");
static_assert(SYNC_COMMITTEE_MAX == PE_SYNC_COMMITTEE_MAX && SYNC_MAX_BATCH == PE_SYNC_MAX_BATCH,
              "kernels.h: SYNC_* are the PE_SYNC_* of include/posevo.h");

namespace posevo {

void sync_committees_drop(pe_engine* h)
{
    for (auto& c : h->sync_committee) c = pe_engine::SyncCommittee{};
}

namespace {

// eth_aggregate_pubkeys of `size` registry members (a validator listed k times counted k times), compressed
int sync_aggregate_key(pe_engine* h, const uint32_t* members, uint32_t size, uint8_t out48[48])
{
    const uint32_t offsets[2] = {0, size};
    uint8_t sum96[96];
    PE_TRY(pe_g1_sum(h, nullptr, 0, members, offsets, 1, sum96));
    return pe_g1_compress(sum96, 1, out48);
}

// committee `which` becomes (members, key): the device copy first, the host's description once it is there
int sync_committee_store(pe_engine* h, int which, const uint32_t* members, uint32_t size, const uint8_t key48[48])
{
    HIP_TRY(h, h->d_sync_members[which].ensure(4ull * SYNC_COMMITTEE_MAX));
    HIP_TRY(h, hipMemcpyAsync(h->d_sync_members[which].p, members, 4ull * size, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    pe_engine::SyncCommittee& c = h->sync_committee[which];
    c.size = size;
    c.members.assign(members, members + size);
    memcpy(c.aggregate_pubkey, key48, 48);
    return PE_OK;
}

bool is_infinity_signature(const uint8_t sig[96])
{
    if (sig[0] != 0xC0) return false;
    for (int k = 1; k < 96; ++k)
        if (sig[k]) return false;
    return true;
}

}  // namespace
}  // namespace posevo

extern "C" {

int pe_sync_committee_compute(pe_engine* h, const uint8_t seed[32], const uint32_t* active_indices, uint32_t n_active,
                              uint32_t shuffle_round_count, uint64_t max_effective_balance, uint32_t size, uint32_t max_tries,
                              uint32_t* out_indices, uint8_t* out_aggregate_pubkey48, uint32_t* out_tries)
{
    if (!h || !seed) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));
    if (h->dist_ready())
        return fail(h, PE_ERR_STATE, "pe_sync_committee_compute: the handle exchanges with other ranks (pe_dist_init); "
                                     "sampling over a sharded registry is not supported");
    if (size == 0 || size > PE_SYNC_COMMITTEE_MAX)
        return fail(h, PE_ERR_INVALID_ARG, "pe_sync_committee_compute: size must lie in 1 .. PE_SYNC_COMMITTEE_MAX");
    if (shuffle_round_count > 255) return fail(h, PE_ERR_INVALID_ARG, "shuffle_round_count is a uint8 in the spec");
    PE_TRY(validate_active_set(h, active_indices, n_active));
    if (n_active == 0) return fail(h, PE_ERR_INVALID_ARG, "pe_sync_committee_compute: the active set is empty");
    if (!h->have_points) return fail(h, PE_ERR_STATE, "pe_sync_committee_compute: no pubkeys loaded");
    const uint64_t tries_cap = max_tries ? max_tries : (1ull << 20);
    const bool staged = active_indices != nullptr && active_indices != PE_ACTIVE_RESIDENT;  // a host list: uploaded

    Layout L;
    const auto r_seed = L.take<uint32_t>(8), r_idx = L.take<uint32_t>(staged ? n_active : 0);
    const auto r_count = L.take<uint32_t>(SYNC_SAMPLE_BATCH / SYNC_SAMPLE_WG), r_entry = L.take<uint32_t>(2ull * SYNC_SAMPLE_BATCH);
    const auto r_state = L.take<SyncSampleState>(1);
    const auto r_members = L.take<uint32_t>(SYNC_COMMITTEE_MAX);
    Workspace w;
    HIP_TRY(h, w.bind(h->d_sync, L, h->stream));
    uint32_t seed_be[8];
    be32_words(seed, seed_be);
    HIP_TRY(h, w.put(r_seed, seed_be, 8));
    if (staged) HIP_TRY(h, w.put(r_idx, active_indices, n_active));
    HIP_TRY(h, w.zero(r_state, 1));
    // batch after batch until `size` members are appended; between two batches the host reads the count
    SyncSampleState state{0, 0};
    for (uint64_t base = 0; base < tries_cap && state.count < size; base += SYNC_SAMPLE_BATCH) {
        if (launch_sync_sample(h->stream, w(r_seed), n_active, shuffle_round_count, active_list_dev(h, active_indices, w(r_idx)),
                               h->d_sbalance.as<uint64_t>(), max_effective_balance, base, tries_cap, size, w(r_count), w(r_entry),
                               w(r_state), w(r_members)))
            return fail(h, PE_ERR_INVALID_ARG, "pe_sync_committee_compute: k_sync_sample refuses these arguments");
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, w.get(r_state, &state, 1));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    if (state.count < size) {
        if (out_tries) *out_tries = (uint32_t)tries_cap;
        return fail(h, PE_ERR_CAPACITY, "pe_sync_committee_compute: fewer than `size` candidates accepted within max_tries");
    }
    std::vector<uint32_t> members(size);
    HIP_TRY(h, w.get(r_members, members.data(), size));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (uint32_t v : members)
        if (v >= h->n_val) return fail(h, PE_ERR_NO_DEVICE, "k_sync_sample returned a validator outside the registry");
    uint8_t key48[48];
    PE_TRY(sync_aggregate_key(h, members.data(), size, key48));
    PE_TRY(sync_committee_store(h, PE_SYNC_NEXT, members.data(), size, key48));
    if (out_indices) memcpy(out_indices, members.data(), 4ull * size);
    if (out_aggregate_pubkey48) memcpy(out_aggregate_pubkey48, key48, 48);
    if (out_tries) *out_tries = state.tries;
    return PE_OK;
}

int pe_sync_committee_set(pe_engine* h, int which, const uint32_t* indices, uint32_t size)
{
    if (!h || !indices || (which != PE_SYNC_CURRENT && which != PE_SYNC_NEXT)) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));
    if (h->dist_ready()) return refuse_dist(h, "pe_sync_committee_set");
    if (size == 0 || size > PE_SYNC_COMMITTEE_MAX)
        return fail(h, PE_ERR_INVALID_ARG, "pe_sync_committee_set: size must lie in 1 .. PE_SYNC_COMMITTEE_MAX");
    for (uint32_t p = 0; p < size; ++p)
        if (indices[p] >= h->n_val) return fail(h, PE_ERR_INVALID_ARG, "pe_sync_committee_set: a member outside the registry");
    if (!h->have_points) return fail(h, PE_ERR_STATE, "pe_sync_committee_set: no pubkeys loaded");
    uint8_t key48[48];
    PE_TRY(sync_aggregate_key(h, indices, size, key48));
    return sync_committee_store(h, which, indices, size, key48);
}

int pe_sync_committee_get(pe_engine* h, int which, uint32_t* out_indices, uint32_t cap, uint32_t* out_size,
                          uint8_t* out_aggregate_pubkey48)
{
    if (!h || !out_size || (which != PE_SYNC_CURRENT && which != PE_SYNC_NEXT)) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));
    const pe_engine::SyncCommittee& c = h->sync_committee[which];
    if (c.size && out_indices && cap < c.size) return fail(h, PE_ERR_CAPACITY, "pe_sync_committee_get: out_indices holds fewer than the committee");
    *out_size = c.size;
    if (c.size == 0) return PE_OK;
    if (out_indices) {  // what the kernels read, not the host's copy of it
        HIP_TRY(h, hipMemcpyAsync(out_indices, h->d_sync_members[which].p, 4ull * c.size, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    if (out_aggregate_pubkey48) memcpy(out_aggregate_pubkey48, c.aggregate_pubkey, 48);
    return PE_OK;
}

int pe_sync_committee_rotate(pe_engine* h)
{
    if (!h) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));
    if (h->sync_committee[PE_SYNC_NEXT].size == 0)
        return fail(h, PE_ERR_STATE, "pe_sync_committee_rotate: no next committee (pe_sync_committee_compute or _set first)");
    std::swap(h->d_sync_members[PE_SYNC_CURRENT], h->d_sync_members[PE_SYNC_NEXT]);
    h->sync_committee[PE_SYNC_CURRENT] = std::move(h->sync_committee[PE_SYNC_NEXT]);
    h->sync_committee[PE_SYNC_NEXT] = pe_engine::SyncCommittee{};
    return PE_OK;
}

void pe_sync_params_default(pe_sync_params* out)
{
    if (!out) return;
    out->total_active_balance = 0;
    out->base_reward_factor = 64;
}

int pe_process_sync_aggregate(pe_engine* h, const pe_sync_aggregate* aggs, uint32_t n, const pe_sync_params* params,
                              uint32_t flags, int32_t* verdict, int32_t* sig_status, pe_sync_stats* out)
{
    if (!h || !params || (n && !aggs)) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));
    if (h->dist_ready()) return refuse_dist(h, "pe_process_sync_aggregate");
    if (flags == 0 || (flags & ~(uint32_t)(PE_SYNC_VERIFY | PE_SYNC_APPLY)))
        return fail(h, PE_ERR_INVALID_ARG, "pe_process_sync_aggregate: flags must be PE_SYNC_VERIFY, PE_SYNC_APPLY or both");
    const bool verify = flags & PE_SYNC_VERIFY, apply = flags & PE_SYNC_APPLY;
    if (verify && n && !verdict) return fail(h, PE_ERR_INVALID_ARG, "pe_process_sync_aggregate: PE_SYNC_VERIFY and no verdict array");
    if (n > PE_SYNC_MAX_BATCH) return fail(h, PE_ERR_INVALID_ARG, "pe_process_sync_aggregate: more than PE_SYNC_MAX_BATCH aggregates");
    const pe_engine::SyncCommittee& com = h->sync_committee[PE_SYNC_CURRENT];
    if (com.size == 0) return fail(h, PE_ERR_STATE, "pe_process_sync_aggregate: no current sync committee");
    if (apply && !h->balances_set)
        return fail(h, PE_ERR_STATE, "pe_process_sync_aggregate: no resident balances (pe_state_set_balances first)");
    if (verify && !h->have_points) return fail(h, PE_ERR_STATE, "pe_process_sync_aggregate: no pubkeys loaded");
    if (verify && h->pipelining)  // pe_hash_to_g2's own refusal, before anything is computed
        return fail(h, PE_ERR_STATE, "pe_process_sync_aggregate: PE_SYNC_VERIFY inside a pipeline (the call is synchronous)");
    for (uint32_t v : com.members)  // (a committee outlives no change of the registry's size but growth)
        if (v >= h->n_val) return fail(h, PE_ERR_STATE, "pe_process_sync_aggregate: the committee names a validator outside the registry");
    for (uint32_t b = 0; b < n; ++b)
        if (aggs[b].proposer_index >= h->n_val) return fail(h, PE_ERR_INVALID_ARG, "pe_process_sync_aggregate: a proposer outside the registry");

    // ---- host step: the scalars, every division of the reference in its order, every product decided in 128 bits
    typedef unsigned __int128 u128;
    const uint64_t inc = h->cfg.effective_balance_increment, total = params->total_active_balance;
    if (inc == 0 || h->cfg.slots_per_epoch == 0 || total < inc)
        return fail(h, PE_ERR_INVALID_ARG, "pe_process_sync_aggregate: total_active_balance lies below the increment");
    pe_sync_stats stats;
    memset(&stats, 0, sizeof stats);
    {
        const u128 factor_wide = (u128)inc * params->base_reward_factor;
        if (factor_wide > (u128)UINT64_MAX)
            return fail(h, PE_ERR_INVALID_ARG, "pe_process_sync_aggregate: increment * base_reward_factor exceeds 64 bits");
        const uint64_t per_increment = (uint64_t)factor_wide / isqrt64(total);
        const u128 base_wide = (u128)per_increment * (total / inc);
        if (base_wide > (u128)UINT64_MAX)
            return fail(h, PE_ERR_INVALID_ARG, "pe_process_sync_aggregate: the total base rewards exceed 64 bits");
        const u128 weighted = base_wide * 2;  // SYNC_REWARD_WEIGHT
        if (weighted > (u128)UINT64_MAX)
            return fail(h, PE_ERR_INVALID_ARG, "pe_process_sync_aggregate: total base rewards * SYNC_REWARD_WEIGHT exceed 64 bits");
        stats.participant_reward = (uint64_t)weighted / 64 / h->cfg.slots_per_epoch / com.size;  // WEIGHT_DENOMINATOR
        const u128 share = (u128)stats.participant_reward * 8;  // PROPOSER_WEIGHT
        if (share > (u128)UINT64_MAX)
            return fail(h, PE_ERR_INVALID_ARG, "pe_process_sync_aggregate: participant_reward * PROPOSER_WEIGHT exceeds 64 bits");
        stats.proposer_reward = (uint64_t)share / (64 - 8);
    }
    if (n == 0) {
        if (out) *out = stats;
        return PE_OK;
    }

    // ---- participants and signing roots
    Layout L;
    const auto r_aggs = L.take<uint32_t>((size_t)SYNC_AGG_WORDS * n);
    const auto r_lists = L.take<uint32_t>((size_t)SYNC_COMMITTEE_MAX * n);
    const auto r_counts = L.take<uint32_t>(n), r_bad = L.take<uint32_t>(n), r_roots = L.take<uint32_t>(8ull * n);
    const auto r_stats = L.take<uint64_t>(3);
    Workspace w;
    HIP_TRY(h, w.bind(h->d_sync, L, h->stream));
    HIP_TRY(h, w.put(r_aggs, aggs, (size_t)SYNC_AGG_WORDS * n));
    const uint32_t* d_committee = h->d_sync_members[PE_SYNC_CURRENT].as<uint32_t>();
    if (launch_sync_members(h->stream, w(r_aggs), n, d_committee, com.size, w(r_lists), w(r_counts), w(r_bad), w(r_roots)))
        return fail(h, PE_ERR_INVALID_ARG, "pe_process_sync_aggregate: k_sync_members refuses these arguments");
    HIP_TRY(h, hipGetLastError());
    std::vector<uint32_t> counts(n), bad(n), lists;
    std::vector<uint8_t> roots(32ull * n);
    HIP_TRY(h, w.get(r_counts, counts.data(), n));
    HIP_TRY(h, w.get(r_bad, bad.data(), n));
    if (verify) {
        // the existing G1 sum takes its index from host memory: the participants' lists cross once, <= 2 KB an aggregate
        lists.resize((size_t)SYNC_COMMITTEE_MAX * n);
        HIP_TRY(h, w.get(r_lists, lists.data(), lists.size()));
        HIP_TRY(h, w.get(r_roots, roots.data(), 8ull * n));
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (uint32_t b = 0; b < n; ++b) {
        if (bad[b]) return fail(h, PE_ERR_INVALID_ARG, "pe_process_sync_aggregate: a set bit at a position beyond the committee's size");
        if (counts[b] > com.size) return fail(h, PE_ERR_NO_DEVICE, "k_sync_members counted more participants than the committee holds");
        stats.n_participants += counts[b];
    }

    // ---- eth_fast_aggregate_verify per aggregate
    std::vector<int32_t> verdicts(n, PE_BLS_INVALID), status(n, 0);
    if (verify) {
        // the aggregate keys of the aggregates with a participant, one group each
        std::vector<uint32_t> index, offsets(1, 0), group_of(n, NONE32);
        for (uint32_t b = 0; b < n; ++b) {
            if (counts[b] == 0) continue;
            group_of[b] = (uint32_t)offsets.size() - 1;
            index.insert(index.end(), &lists[(size_t)SYNC_COMMITTEE_MAX * b], &lists[(size_t)SYNC_COMMITTEE_MAX * b] + counts[b]);
            offsets.push_back((uint32_t)index.size());
        }
        const uint32_t n_keys = (uint32_t)offsets.size() - 1;
        std::vector<uint8_t> keys((size_t)96 * n_keys), sums((size_t)96 * n, 0), msg192((size_t)192 * n), sig96((size_t)96 * n),
            sig192((size_t)192 * n);
        std::vector<int32_t> st_sub(n, 0);
        if (n_keys) PE_TRY(pe_g1_sum(h, nullptr, 0, index.data(), offsets.data(), n_keys, keys.data()));
        for (uint32_t b = 0; b < n; ++b) {
            if (group_of[b] == NONE32) sums[(size_t)96 * b] = 0x40;  // the empty sum: the identity
            else memcpy(&sums[(size_t)96 * b], &keys[(size_t)96 * group_of[b]], 96);
        }
        PE_TRY(pe_hash_to_g2(h, roots.data(), n, 32, reinterpret_cast<const uint8_t*>(PE_ETH2_DST), (uint32_t)strlen(PE_ETH2_DST),
                             msg192.data(), nullptr));
        for (uint32_t b = 0; b < n; ++b) memcpy(&sig96[(size_t)96 * b], aggs[b].signature, 96);
        PE_TRY(pe_g2_decompress(h, sig96.data(), n, sig192.data(), status.data()));
        for (uint32_t b = 0; b < n; ++b)
            if (status[b] != 0) {  // no point came out: the subgroup test reads the identity there
                memset(&sig192[(size_t)192 * b], 0, 192);
                sig192[(size_t)192 * b] = 0x40;
            }
        PE_TRY(pe_g2_subgroup_check(h, sig192.data(), n, st_sub.data()));
        std::vector<uint32_t> good;
        for (uint32_t b = 0; b < n; ++b) {
            if (counts[b] == 0 && is_infinity_signature(aggs[b].signature)) {  // eth_fast_aggregate_verify's own case
                verdicts[b] = PE_BLS_VALID;
                continue;
            }
            if (status[b] == 0) status[b] = st_sub[b];
            if (status[b] != 0) continue;                                        // not a BLSSignature
            if (counts[b] == 0 || (sig192[(size_t)192 * b] & 0x40) || (sums[(size_t)96 * b] & 0x40)) continue;  // FastAggregateVerify refuses
            good.push_back(b);
        }
        if (!good.empty()) {
            std::vector<int32_t> v(good.size());
            PE_TRY(verify_pairs_run(
                h, "pe_process_sync_aggregate", (uint32_t)good.size(), [&](uint32_t t) { return &sums[(size_t)96 * good[t]]; },
                [&](uint32_t t) { return &msg192[(size_t)192 * good[t]]; }, [&](uint32_t t) { return &sig192[(size_t)192 * good[t]]; },
                v.data()));
            for (size_t t = 0; t < good.size(); ++t) verdicts[good[t]] = v[t];
        }
    }
    bool all_valid = true;
    for (uint32_t b = 0; b < n; ++b) all_valid = all_valid && (!verify || verdicts[b] == PE_BLS_VALID);

    // ---- the rewards and penalties, onto the resident balances
    if (apply && all_valid) {
        if (launch_sync_rewards(h->stream, w(r_aggs), n, d_committee, com.size, stats.participant_reward, stats.proposer_reward,
                                h->d_rbalance.as<uint64_t>(), w(r_stats)))
            return fail(h, PE_ERR_INVALID_ARG, "pe_process_sync_aggregate: k_sync_rewards refuses these arguments");
        HIP_TRY(h, hipGetLastError());
        uint64_t s[3] = {0, 0, 0};
        HIP_TRY(h, w.get(r_stats, s, 3));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        stats.credited = s[0];
        stats.debited = s[1];
        stats.n_saturated = s[2];
        stats.applied = 1;
    }
    if (verify) {
        memcpy(verdict, verdicts.data(), 4ull * n);
        if (sig_status) memcpy(sig_status, status.data(), 4ull * n);
    }
    if (out) *out = stats;
    return PE_OK;
}

}  // extern "C"
