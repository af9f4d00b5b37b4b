// pos_evolution_amd/csrc/block_ops_row.h compiled for the HOST by a plain C++ compiler, from the very header
// engine_block_ops.cpp and the gfx950 kernels include: a whole pe_process_block_operations over host arrays in the kernels'
// steps (slots, the two first-occurrence tables, events, ranks and reward prefixes, the host step, one writing pass with one
// writer per column and validator).  tests/test_block_ops_row_host.py holds it against tests/block_ops_model.py.  With
// -DBOH_MAIN the file is a stand-alone program (its own main) that holds the same call to a sequential loop on small random
// blocks, for a run under -fsanitize=address,undefined.
#include <algorithm>
#include <vector>

#include "../../pos_evolution_amd/csrc/block_ops_row.h"

using namespace posevo;

extern "C" {

unsigned boh_sizeof_op() { return (unsigned)sizeof(BlockOpHost); }

// params = the eight words of pe_block_ops_params; out_stats = the eleven words of pe_block_ops_stats.
// -> 0, -1 / -2: block_ops_prepare's refusals, -7: the proposer lies outside the registry, else the codes of
// block_ops_check_params / block_ops_scalars_make (nothing written).  With an invalid operation: 0, statuses written, arrays
// untouched.
int boh_block_operations(uint64_t n, const uint64_t* act, uint64_t* ext, uint64_t* wdr, const uint64_t* eff, uint8_t* sflags,
                         uint64_t* bal, uint64_t cur, uint32_t proposer, const BlockOpHost* ops, uint32_t n_ops,
                         const uint32_t* indices, uint64_t n_indices, const uint64_t params[8], int32_t* status,
                         uint64_t out_stats[11])
{
    BlockOpsParams p;
    memcpy(&p, params, sizeof p);
    if (proposer >= n) return -7;
    if (const int rc = block_ops_check_params(p, cur)) return rc;
    std::vector<BlockOpDev> dev(n_ops);
    std::vector<uint32_t> host_status(n_ops), slot_off(n_ops + 1, 0);
    uint64_t total_slots = 0;
    for (uint32_t o = 0; o < n_ops; ++o) {
        if (const int rc = block_ops_prepare(ops[o], n, n_indices, cur, &dev[o], &host_status[o])) return -rc;
        slot_off[o] = (uint32_t)total_slots;
        total_slots += block_ops_slots(dev[o], host_status[o]);
        if (total_slots >= BLOCK_OPS_MAX_SLOTS) return -2;
    }
    slot_off[n_ops] = (uint32_t)total_slots;
    const uint32_t n_slots = (uint32_t)total_slots;

    // k_block_ops_lists: the validator of every slot, the lists' verdict per operation
    std::vector<uint32_t> slot_val(n_slots), slot_op(n_slots), op_bad(n_ops, 0), op_hit(n_ops, 0);
    for (uint32_t s = 0; s < n_slots; ++s) {
        const uint32_t o = block_ops_op_of_slot(slot_off.data(), n_ops, s);
        const BlockOpsSlot r = block_ops_slot(dev[o], s - slot_off[o], indices, n);
        slot_val[s] = r.validator;
        slot_op[s] = o;
        op_bad[o] |= r.bad;
    }
    // k_block_ops_claim: the two minima per validator (visited backwards here: a minimum does not depend on the order)
    std::vector<uint32_t> first_potent(n, BLOCK_OPS_NONE), first_slash(n, BLOCK_OPS_NONE);
    auto potent = [&](uint32_t s) {
        const uint32_t v = slot_val[s], o = slot_op[s];
        return block_ops_potent(dev[o].kind, dev[o].pre, op_bad[o] != 0, sflags[v], act[v], ext[v], wdr[v], cur, p.shard_committee_period);
    };
    for (uint32_t s = n_slots; s-- > 0;) {
        if (slot_val[s] == BLOCK_OPS_NONE || !potent(s)) continue;
        const uint32_t v = slot_val[s];
        first_potent[v] = std::min(first_potent[v], s);
        if (dev[slot_op[s]].kind != BLOCK_OP_VOLUNTARY_EXIT) first_slash[v] = std::min(first_slash[v], s);
    }
    // k_block_ops_resolve: events, statuses, sums
    std::vector<uint8_t> ev(n_slots, 0);
    std::vector<uint32_t> dev_status(n_ops, BLOCK_OP_OK);
    BlockOpsTotals t;
    memset(&t, 0, sizeof t);
    t.proposer_balance = bal[proposer];
    uint64_t n_active = 0;
    RegistryExitMax pair = {0, 0};
    for (uint64_t v = 0; v < n; ++v) {
        n_active += registry_active(act[v], ext[v], cur);
        const RegistryExitMax one = {ext[v], ext[v] != REGISTRY_FAR_FUTURE_EPOCH ? 1u : 0u};
        pair = registry_exit_max_join(pair, one);
    }
    const U64Div by_reward = u64_div_make(p.whistleblower_reward_quotient);
    for (uint32_t s = 0; s < n_slots; ++s) {
        const uint32_t v = slot_val[s], o = slot_op[s];
        if (v == BLOCK_OPS_NONE) continue;
        const uint32_t kind = dev[o].kind;
        ev[s] = (uint8_t)block_ops_events(kind, potent(s), s, first_potent[v], first_slash[v], ext[v]);
        if (kind == BLOCK_OP_VOLUNTARY_EXIT)
            dev_status[o] = block_ops_exit_status(act[v], ext[v], cur, p.shard_committee_period, first_potent[v] < s, dev[o].pre);
        else if (kind == BLOCK_OP_PROPOSER_SLASHING)
            dev_status[o] = block_ops_proposer_status(block_ops_slashable(sflags[v], act[v], wdr[v], cur), first_slash[v] < s, dev[o].pre);
        if (ev[s] & BLOCK_EV_SLASH) {
            op_hit[o] = 1;
            t.n_slashed += 1;
            t.rewards += u64_div(eff[v], by_reward);
            t.slashed_balance += eff[v];
            t.max_eff_slashed = std::max<unsigned long long>(t.max_eff_slashed, eff[v]);
        }
        if (ev[s] & BLOCK_EV_FRESH_EXIT) t.n_fresh += 1;
    }
    // the host step: statuses, the refusals, the scalars
    uint64_t n_invalid = 0;
    for (uint32_t o = 0; o < n_ops; ++o) {
        uint32_t st = host_status[o];
        if (st == BLOCK_OP_OK) {
            if (dev[o].kind != BLOCK_OP_ATTESTER_SLASHING) st = dev_status[o];
            else if (op_bad[o]) st = BLOCK_OP_BAD_INDICES;
            else if (!(dev[o].pre & BLOCK_OP_PRE_OK)) st = BLOCK_OP_BAD_SIGNATURE;
            else if (!op_hit[o]) st = BLOCK_OP_NOBODY_SLASHABLE;
        }
        status[o] = (int32_t)st;
        n_invalid += st != BLOCK_OP_OK;
    }
    BlockOpsScalars S;
    uint64_t limit = 0, last = 0;
    if (n_invalid) memset(&t, 0, sizeof t);  // the churn limit alone
    if (const int rc = block_ops_scalars_make(p, cur, proposer, n_slots, n_active, pair.epoch, pair.count, t, &S, &limit, &last)) return rc;
    uint64_t stats[11] = {n_active, limit, 0, 0, 0, 0, 0, 0, 0, 0, n_invalid};
    if (n_invalid) {
        for (int i = 0; i < 11; ++i) out_stats[i] = stats[i];
        return 0;
    }
    // k_block_ops_apply: ranks and prefixes in slot order; ext and the fresh withdrawable epoch are the fresh lane's, the flag,
    // the balance and an exiting validator's withdrawable epoch the slash lane's
    uint64_t k = 0, rewards_before = 0, penalties = 0, saturated = 0;
    for (uint32_t s = 0; s < n_slots; ++s) {
        const uint32_t v = slot_val[s];
        if (ev[s] & BLOCK_EV_FRESH_EXIT) {
            const uint64_t q = registry_exit_epoch(S.exit_base, S.exit_fill, k++, S.by_churn_limit);
            ext[v] = q;
            const uint64_t w = q + S.withdrawability_delay;
            wdr[v] = first_slash[v] != BLOCK_OPS_NONE ? block_ops_slashed_withdrawable(w, S.slashed_withdrawable) : w;
        }
        if (ev[s] & BLOCK_EV_SLASH) {
            const uint64_t penalty = u64_div(eff[v], S.by_penalty_quotient), reward = u64_div(eff[v], S.by_reward_quotient);
            const bool is_proposer = v == proposer;
            const BlockOpsDebit d = block_ops_slash_balance(bal[v], penalty, is_proposer ? rewards_before : 0, is_proposer ? S.total_rewards : 0);
            bal[v] = d.balance;
            penalties += d.debited;
            saturated += d.saturated;
            sflags[v] |= REWARD_VAL_SLASHED;
            if (ev[s] & BLOCK_EV_EXIT_WAS_SET) wdr[v] = block_ops_slashed_withdrawable(wdr[v], S.slashed_withdrawable);
            rewards_before += reward;
        }
    }
    if (first_slash[proposer] == BLOCK_OPS_NONE) bal[proposer] += S.total_rewards;  // the proposer's own lane
    stats[2] = t.n_slashed;
    stats[3] = t.n_fresh;
    stats[4] = t.n_fresh ? S.exit_base : 0;
    stats[5] = last;
    stats[6] = t.slashed_balance;
    stats[7] = t.rewards;
    stats[8] = penalties;
    stats[9] = saturated;
    for (int i = 0; i < 11; ++i) out_stats[i] = stats[i];
    return 0;
}

}  // extern "C"

#ifdef BOH_MAIN
#include <stdio.h>
// small registries and blocks of exits and single-validator slashings (the slasher's convention: the same one-element list on
// both sides), the proposer among the slashed: the call above against slash_validator / initiate_validator_exit called one
// after the other
int main()
{
    const uint64_t FAR = REGISTRY_FAR_FUTURE_EPOCH;
    uint64_t state = 0x9E3779B97F4A7C15ull;
    auto next = [&state]() {
        state ^= state << 13;
        state ^= state >> 7;
        state ^= state << 17;
        return state;
    };
    long checked = 0;
    for (int round = 0; round < 600; ++round) {
        const uint64_t n = 2 + next() % 24, cur = 300, limit = 1 + next() % 4, target = cur + 1 + 4;
        const uint32_t proposer = (uint32_t)(next() % n);
        std::vector<uint64_t> act(n, 0), ext(n), wdr(n), eff(n), bal(n);
        std::vector<uint8_t> fl(n);
        for (uint64_t v = 0; v < n; ++v) {
            ext[v] = next() % 4 ? FAR : target - 1 + next() % 3;
            wdr[v] = ext[v] == FAR ? FAR : ext[v] + 256;
            eff[v] = (1 + next() % 32) * 1000000000ull;
            bal[v] = next() % 3 ? eff[v] + next() % 1000 : next() % 100000000ull;
            fl[v] = next() % 6 ? 1 : 3;
        }
        const uint32_t n_ops = 1 + (uint32_t)(next() % 8);
        std::vector<BlockOpHost> ops(n_ops);
        std::vector<uint32_t> indices(n_ops);
        for (uint32_t o = 0; o < n_ops; ++o) {
            BlockOpHost& op = ops[o];
            memset(&op, 0, sizeof op);
            op.flags = next() % 8 ? 1 : 0;
            indices[o] = (uint32_t)(next() % n);
            if (next() % 2) {
                op.kind = BLOCK_OP_ATTESTER_SLASHING;
                op.data_1[16] = 1;  // two different votes for target epoch 0
                op.data_2[16] = 2;
                op.indices_1_offset = op.indices_2_offset = o;
                op.indices_1_length = op.indices_2_length = 1;
            } else {
                op.kind = BLOCK_OP_VOLUNTARY_EXIT;
                op.validator_index = indices[o];
                op.exit_epoch = cur - next() % 2;
            }
        }
        // the sequential loop
        std::vector<uint64_t> e2(ext), w2(wdr), b2(bal);
        std::vector<uint8_t> f2(fl);
        std::vector<int32_t> want(n_ops);
        auto initiate = [&](uint64_t i) {
            if (e2[i] != FAR) return;
            uint64_t q = target, holders = 0;
            for (uint64_t e : e2)
                if (e != FAR && e > q) q = e;
            for (uint64_t e : e2) holders += e == q;
            if (holders >= limit) ++q;
            e2[i] = q;
            w2[i] = q + 256;
        };
        bool all_valid = true;
        for (uint32_t o = 0; o < n_ops; ++o) {
            const uint64_t i = indices[o];
            const bool sig = ops[o].flags & 1;
            int32_t st = 0;
            if (ops[o].kind == BLOCK_OP_ATTESTER_SLASHING) {
                if (!sig) st = BLOCK_OP_BAD_SIGNATURE;
                else if ((f2[i] & 2) || !(act[i] <= cur && cur < w2[i])) st = BLOCK_OP_NOBODY_SLASHABLE;
                else {
                    initiate(i);
                    f2[i] |= 2;
                    w2[i] = std::max(w2[i], cur + 8192);
                    b2[i] -= std::min(b2[i], eff[i] / 32);
                    b2[proposer] += eff[i] / 512;
                }
            } else {
                if (!(act[i] <= cur && cur < e2[i])) st = BLOCK_OP_NOT_ACTIVE;
                else if (e2[i] != FAR) st = BLOCK_OP_ALREADY_EXITING;
                else if (!sig) st = BLOCK_OP_BAD_SIGNATURE;
                else initiate(i);
            }
            want[o] = st;
            all_valid = all_valid && st == 0;
        }
        const uint64_t params[8] = {32, 512, 8192, 256, 256, 4, limit, 1ull << 40};
        uint64_t stats[11];
        std::vector<int32_t> got(n_ops);
        std::vector<uint64_t> e1(ext), w1(wdr), b1(bal);
        std::vector<uint8_t> f1(fl);
        if (boh_block_operations(n, act.data(), e1.data(), w1.data(), eff.data(), f1.data(), b1.data(), cur, proposer, ops.data(), n_ops,
                                 indices.data(), n_ops, params, got.data(), stats))
            return 2;
        if (!all_valid) {
            e2 = ext;
            w2 = wdr;
            b2 = bal;
            f2 = fl;
        }
        if (got != want || e1 != e2 || w1 != w2 || b1 != b2 || f1 != f2) {
            printf("round %d: the call and the sequential loop differ\n", round);
            return 1;
        }
        checked += n_ops;
    }
    printf("block_ops_row_host: %ld operations, closed form exact\n", checked);
    return 0;
}
#endif
