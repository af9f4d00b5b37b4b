// engine_ssz.cpp -- SSZ hash_tree_root of the per-validator fields of BeaconState (pe:354-369) from where the data lies, and
// merkleize for the caller's own chunk vectors.
//   pe_registry_set_static / _get   the parts of Validator (pe:36-45) nothing else in the engine needs: the pubkey's leaf,
//                                   withdrawal_credentials, activation_eligibility_epoch
//   pe_state_roots                  hash_tree_root of balances, inactivity_scores, both participation lists and validators
//   pe_ssz_merkleize                merkleize(chunks, depth) [+ mix_in_length] of chunks in host memory
// The reference names hash_tree_root (pe:142, 423, 1016) and holds no text of it: the conventions are the SSZ specification's
// [UPSTREAM-MEMORY], restated at the top of ssz_kernels.hip and in tests/ssz_model.py.
// The device reduces a list to ONE node (k_ssz_merkle, 2^tile_log2 nodes per workgroup and pass); the host climbs from that
// node's height to the tree's depth against the zero hashes and mixes the length in: at most 65 hashes with sha256.h's text.
#include "engine_internal.h"
#include "sha256.h"

using namespace posevo;

namespace posevo {

void registry_static_drop(pe_engine* h)
{
    h->static_set = false;
    h->dep_index_slots = 0;  // the pubkey index (engine_deposit.cpp) is a table over these leaves
}

namespace {

struct ZeroHashes {
    uint32_t w[SSZ_ZERO_HASHES][8];  // word form
    ZeroHashes()
    {
        memset(w[0], 0, sizeof w[0]);
        for (uint32_t k = 0; k + 1 < SSZ_ZERO_HASHES; ++k) {
            uint32_t msg[16];
            memcpy(msg, w[k], 32);
            memcpy(msg + 8, w[k], 32);
            sha256_64(msg, w[k + 1]);
        }
    }
};
const ZeroHashes& zero_hashes()
{
    static const ZeroHashes z;
    return z;
}

void words_to_bytes(const uint32_t w[8], uint8_t out[32])
{
    for (int k = 0; k < 8; ++k) {
        out[4 * k] = (uint8_t)(w[k] >> 24);
        out[4 * k + 1] = (uint8_t)(w[k] >> 16);
        out[4 * k + 2] = (uint8_t)(w[k] >> 8);
        out[4 * k + 3] = (uint8_t)w[k];
    }
}

// node (word form) of `height` -> the root of the depth-`depth` tree whose other leaves are absent, then mix_in_length
void climb_and_mix(const uint32_t node[8], uint32_t height, uint32_t depth, int64_t mix_length, uint8_t out_root[32])
{
    const ZeroHashes& Z = zero_hashes();
    uint32_t msg[16], cur[8];
    memcpy(cur, node, 32);
    for (uint32_t k = height; k < depth; ++k) {
        memcpy(msg, cur, 32);
        memcpy(msg + 8, Z.w[k], 32);
        sha256_64(msg, cur);
    }
    if (mix_length >= 0) {  // H(root || uint256_le(n))
        memcpy(msg, cur, 32);
        memset(msg + 8, 0, 32);
        const uint64_t n = (uint64_t)mix_length;
        msg[8] = __builtin_bswap32((uint32_t)n);
        msg[9] = __builtin_bswap32((uint32_t)(n >> 32));
        sha256_64(msg, cur);
    }
    words_to_bytes(cur, out_root);
}

int ensure_zero_table(pe_engine* h)
{
    if (h->ssz_zero_ready) return PE_OK;
    HIP_TRY(h, h->d_ssz_zero.ensure(sizeof(ZeroHashes)));
    HIP_TRY(h, hipMemcpyAsync(h->d_ssz_zero.p, zero_hashes().w, sizeof(ZeroHashes), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->ssz_zero_ready = true;
    return PE_OK;
}

// One list's passes on the engine's stream: n_bytes >= 1 of list bytes at src (device) -> the single node left, word form, at
// d_final; *out_height = its height (<= depth).  ceil(n_bytes / 32) <= 2^depth.
int merkle_enqueue(pe_engine* h, const void* src, uint64_t n_bytes, uint32_t depth, uint32_t* d_final, uint32_t* out_height)
{
    const uint32_t TL = h->tune.ssz_tile_log2;
    uint64_t m = (n_bytes + 31) / 32;
    const uint64_t tile = 1ull << TL;
    const uint64_t m1 = (m + tile - 1) / tile, m2 = (m1 + tile - 1) / tile;
    HIP_TRY(h, h->d_ssz_level[0].ensure(std::max<size_t>(64, 32 * m1)));
    HIP_TRY(h, h->d_ssz_level[1].ensure(std::max<size_t>(64, 32 * m2)));
    uint32_t base = 0;
    int raw = 1, pp = 0;
    const void* in = src;
    for (;;) {
        const uint32_t levels = std::min<uint32_t>(TL, depth - base);
        const uint64_t n_out = (m + (1ull << levels) - 1) >> levels;
        if (n_out > 0x7FFFFFFFull) return fail(h, PE_ERR_CAPACITY, "merkleize: more than 2^31 workgroups in one pass");
        uint32_t* dst = n_out == 1 ? d_final : h->d_ssz_level[pp].as<uint32_t>();
        launch_ssz_merkle(h->stream, in, n_bytes, raw, base, levels, h->d_ssz_zero.as<uint32_t>(), dst);
        HIP_TRY(h, hipGetLastError());
        base += levels;
        m = n_out;
        if (m == 1) break;
        in = dst;
        n_bytes = 32 * m;
        raw = 0;
        pp ^= 1;
    }
    *out_height = base;
    return PE_OK;
}

}  // namespace

}  // namespace posevo

extern "C" {

int pe_registry_set_static(pe_engine* h, uint64_t n, const uint8_t* pubkeys48, const uint8_t* withdrawal_credentials32,
                           const uint64_t* activation_eligibility_epoch)
{
    if (!h || (n && (!pubkeys48 || !withdrawal_credentials32 || !activation_eligibility_epoch))) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));
    if (n != h->n_val) return fail(h, PE_ERR_INVALID_ARG, "pe_registry_set_static: n differs from the registry size");
    h->dep_index_slots = 0;  // the leaves are replaced: the pubkey index over the old ones goes with them
    HIP_TRY(h, reg_ensure(h, REG_STATIC, n, /*keep=*/false, &h->static_set));
    if (n) {
        h->static_set = false;
        HIP_TRY(h, hipMemcpyAsync(h->d_withdrawal_credentials.p, withdrawal_credentials32, 32 * n, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(h->d_activation_eligibility.p, activation_eligibility_epoch, 8 * n, hipMemcpyHostToDevice, h->stream));
        const uint64_t chunk = std::min<uint64_t>(n, 1u << 20);  // the keys pass through a bounded staging buffer
        HIP_TRY(h, h->d_tmp_be.ensure(48ull * chunk));
        for (uint64_t base = 0; base < n; base += chunk) {
            const uint64_t m = std::min(chunk, n - base);
            HIP_TRY(h, hipMemcpyAsync(h->d_tmp_be.p, pubkeys48 + 48ull * base, 48ull * m, hipMemcpyHostToDevice, h->stream));
            launch_ssz_pubkey_roots(h->stream, h->d_tmp_be.as<uint8_t>(), m, h->d_pubkey_leaf.as<uint8_t>() + 32ull * base);
            HIP_TRY(h, hipGetLastError());
            HIP_TRY(h, hipStreamSynchronize(h->stream));
        }
    }
    h->static_set = true;
    return PE_OK;
}

int pe_registry_get_static(pe_engine* h, uint64_t n, uint8_t* out_pubkey_leaves32, uint8_t* out_withdrawal_credentials32,
                           uint64_t* out_activation_eligibility_epoch, int* out_is_set)
{
    if (!h || !out_is_set) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));
    if (n != h->n_val) return fail(h, PE_ERR_INVALID_ARG, "pe_registry_get_static: n differs from the registry size");
    *out_is_set = h->static_set ? 1 : 0;
    if (n && h->static_set) {
        if (out_pubkey_leaves32)
            HIP_TRY(h, hipMemcpyAsync(out_pubkey_leaves32, h->d_pubkey_leaf.p, 32 * n, hipMemcpyDeviceToHost, h->stream));
        if (out_withdrawal_credentials32)
            HIP_TRY(h, hipMemcpyAsync(out_withdrawal_credentials32, h->d_withdrawal_credentials.p, 32 * n, hipMemcpyDeviceToHost, h->stream));
        if (out_activation_eligibility_epoch)
            HIP_TRY(h, hipMemcpyAsync(out_activation_eligibility_epoch, h->d_activation_eligibility.p, 8 * n, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    return PE_OK;
}

int pe_state_roots(pe_engine* h, uint32_t which, uint32_t limit_log2, pe_state_root_set* out, uint8_t* out_validator_leaves)
{
    if (!h || !out) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));  // open pipelines complete, and the flag passes on the state stream with them (as pe_ffg_balances)
    if (h->dist_ready())
        return fail(h, PE_ERR_STATE, "pe_state_roots: the handle exchanges with other ranks (pe_dist_init); "
                                     "a sharded registry is not supported");
    const uint32_t all = PE_ROOT_BALANCES | PE_ROOT_INACTIVITY | PE_ROOT_PART_PREV | PE_ROOT_PART_CUR | PE_ROOT_VALIDATORS;
    if (which == 0 || (which & ~all)) return fail(h, PE_ERR_INVALID_ARG, "pe_state_roots: which must be a non-empty set of PE_ROOT_* bits");
    const uint32_t limit = limit_log2 ? limit_log2 : 40;
    const uint64_t n = h->n_val;
    if (limit > 64 || limit < 5 || (limit < 64 && n > (1ull << limit)))
        return fail(h, PE_ERR_INVALID_ARG, "pe_state_roots: limit_log2 must lie in 5 .. 64 and 2^limit_log2 must hold the registry");
    if ((which & (PE_ROOT_BALANCES | PE_ROOT_INACTIVITY)) && !h->balances_set)
        return fail(h, PE_ERR_STATE, "pe_state_roots: no resident balances (pe_state_set_balances first)");
    if (which & PE_ROOT_VALIDATORS) {
        if (!h->epochs_set) return fail(h, PE_ERR_STATE, "pe_state_roots: no registry epochs (pe_registry_set_epochs first)");
        if (!h->balances_set)
            return fail(h, PE_ERR_STATE, "pe_state_roots: no resident withdrawable epochs (pe_state_set_balances first)");
        if (!h->static_set) return fail(h, PE_ERR_STATE, "pe_state_roots: no static registry part (pe_registry_set_static first)");
    }
    PE_TRY(ensure_zero_table(h));
    // the lists in the order of pe_state_root_set's fields
    struct List { uint32_t bit; const void* src; uint64_t n_bytes; uint32_t depth; } lists[5] = {
        {PE_ROOT_BALANCES, h->d_rbalance.p, 8 * n, limit - 2},
        {PE_ROOT_INACTIVITY, h->d_inactivity.p, 8 * n, limit - 2},
        {PE_ROOT_PART_PREV, h->d_part_prev.p, n, limit - 5},
        {PE_ROOT_PART_CUR, h->d_part_cur.p, n, limit - 5},
        {PE_ROOT_VALIDATORS, nullptr, 32 * n, limit},
    };
    OutBlock ob(h);
    const size_t off = ob.alloc(5 * 32);
    PE_TRY(ob.ensure());
    uint32_t height[5] = {0, 0, 0, 0, 0};
    if (n) {
        if (which & PE_ROOT_VALIDATORS) {
            HIP_TRY(h, h->d_ssz_validator_roots.ensure(std::max<size_t>(64, 32 * n)));
            SszValidatorArgs a;
            a.pubkey_leaf32 = h->d_pubkey_leaf.as<uint8_t>();
            a.withdrawal_credentials32 = h->d_withdrawal_credentials.as<uint8_t>();
            a.effective_balance = h->d_sbalance.as<uint64_t>();  // the view, mirrored or its own: pe_set_validators keeps it current
            a.sflags = h->d_sflags.as<uint8_t>();
            a.activation_eligibility_epoch = h->d_activation_eligibility.as<uint64_t>();
            a.activation_epoch = h->d_activation_epoch.as<uint64_t>();
            a.exit_epoch = h->d_exit_epoch.as<uint64_t>();
            a.withdrawable_epoch = h->d_withdrawable.as<uint64_t>();
            a.n_val = n;
            a.out_roots32 = h->d_ssz_validator_roots.as<uint8_t>();
            launch_ssz_validator_roots(h->stream, a);
            HIP_TRY(h, hipGetLastError());
            lists[4].src = h->d_ssz_validator_roots.p;
        }
        for (int i = 0; i < 5; ++i)
            if (which & lists[i].bit)
                PE_TRY(merkle_enqueue(h, lists[i].src, lists[i].n_bytes, lists[i].depth, ob.dev<uint32_t>(off + 32 * i), &height[i]));
        HIP_TRY(h, ob.download());
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if ((which & PE_ROOT_VALIDATORS) && out_validator_leaves)
            HIP_TRY(h, hipMemcpy(out_validator_leaves, h->d_ssz_validator_roots.p, 32 * n, hipMemcpyDeviceToHost));
    }
    pe_state_root_set r = *out;  // the roots not asked for keep what the caller had there
    uint8_t* fields[5] = {r.balances, r.inactivity_scores, r.previous_epoch_participation, r.current_epoch_participation,
                          r.validators};
    for (int i = 0; i < 5; ++i) {
        if (!(which & lists[i].bit)) continue;
        if (n)
            climb_and_mix(ob.host<uint32_t>(off + 32 * i), height[i], lists[i].depth, (int64_t)n, fields[i]);
        else
            climb_and_mix(zero_hashes().w[lists[i].depth], lists[i].depth, lists[i].depth, 0, fields[i]);
    }
    *out = r;
    return PE_OK;
}

int pe_ssz_merkleize(pe_engine* h, const uint8_t* chunks32, uint64_t n_chunks, uint32_t depth, int64_t mix_length,
                     uint8_t out_root[32])
{
    if (!h || !out_root || (n_chunks && !chunks32)) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));
    if (depth > 64 || (depth < 64 && n_chunks > (1ull << depth)))
        return fail(h, PE_ERR_INVALID_ARG, "pe_ssz_merkleize: depth must be at most 64 and 2^depth must hold the chunks");
    if (n_chunks == 0) {
        climb_and_mix(zero_hashes().w[depth], depth, depth, mix_length, out_root);
        return PE_OK;
    }
    PE_TRY(ensure_zero_table(h));
    HIP_TRY(h, h->d_ssz_chunks.ensure(32 * n_chunks));
    OutBlock ob(h);
    const size_t off = ob.alloc(32);
    PE_TRY(ob.ensure());
    HIP_TRY(h, hipMemcpyAsync(h->d_ssz_chunks.p, chunks32, 32 * n_chunks, hipMemcpyHostToDevice, h->stream));
    uint32_t height = 0;
    PE_TRY(merkle_enqueue(h, h->d_ssz_chunks.p, 32 * n_chunks, depth, ob.dev<uint32_t>(off), &height));
    HIP_TRY(h, ob.download());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    climb_and_mix(ob.host<uint32_t>(off), height, depth, mix_length, out_root);
    return PE_OK;
}

}  // extern "C"
