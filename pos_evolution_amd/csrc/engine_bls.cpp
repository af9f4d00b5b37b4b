// engine_bls.cpp -- the pairing-product check and FastAggregateVerify on the device.
//   pe_pairing_check          per group: prod e(P_j, Q_j) == 1
//   pe_fast_aggregate_verify  per group: e(sum of the group's registry pubkeys, H(m)) e(-g1, signature) == 1; the sum goes the
//                             route of pe_g1_sum, H(m) comes in as a point (pe_hash_to_g2 makes it: engine_h2c.cpp)
//   pe_profile_pairing_gt     the value the verdict compares with 1, for the parity tests
// (pe_batch_verify, which decides many aggregates with one final exponentiation and falls back on pairing_run: engine_batch.cpp)
// Both verdict calls are synchronous and complete open pipelines first (enter); one GPU: PE_ERR_STATE under pe_dist_init*.
#include "engine_internal.h"

using namespace posevo;

namespace posevo {

// -g1: the generator of G1 negated, 96-byte uncompressed form (x, p - y of the published generator)
extern const uint8_t NEG_G1_BE96[96] = {
    0x17, 0xf1, 0xd3, 0xa7, 0x31, 0x97, 0xd7, 0x94, 0x26, 0x95, 0x63, 0x8c, 0x4f, 0xa9, 0xac, 0x0f,
    0xc3, 0x68, 0x8c, 0x4f, 0x97, 0x74, 0xb9, 0x05, 0xa1, 0x4e, 0x3a, 0x3f, 0x17, 0x1b, 0xac, 0x58,
    0x6c, 0x55, 0xe8, 0x3f, 0xf9, 0x7a, 0x1a, 0xef, 0xfb, 0x3a, 0xf0, 0x0a, 0xdb, 0x22, 0xc6, 0xbb,
    0x11, 0x4d, 0x1d, 0x68, 0x55, 0xd5, 0x45, 0xa8, 0xaa, 0x7d, 0x76, 0xc8, 0xcf, 0x2e, 0x21, 0xf2,
    0x67, 0x81, 0x6a, 0xef, 0x1d, 0xb5, 0x07, 0xc9, 0x66, 0x55, 0xb9, 0xd5, 0xca, 0xac, 0x42, 0x36,
    0x4e, 0x6f, 0x38, 0xba, 0x0e, 0xcb, 0x75, 0x1b, 0xad, 0x54, 0xdc, 0xd6, 0xb9, 0x39, 0xc2, 0xca
};

int pairing_run(pe_engine* h, const char* who, const uint8_t* g1, const uint8_t* g2, uint64_t n_pairs, const uint32_t* offsets,
                uint32_t n_groups, int32_t* verdict, uint8_t* out576)
{
    if (h->dist_ready()) return refuse_dist(h, who);
    if (n_groups == 0) return PE_OK;
    if (n_pairs >= 0xFFFFFFFFull) return fail(h, PE_ERR_CAPACITY, std::string(who) + ": too many pairs");
    for (uint32_t g = 0; g < n_groups; ++g)
        if (offsets[g + 1] < offsets[g]) return fail(h, PE_ERR_INVALID_ARG, std::string(who) + ": offsets not monotone");
    if (offsets[n_groups] > n_pairs) return fail(h, PE_ERR_INVALID_ARG, std::string(who) + ": offsets exceed the number of pairs");
    const size_t rows = std::max<uint64_t>(1, n_pairs);  // the kernels' idle lanes read row 0
    const size_t ng = n_groups;
    Layout L;
    const auto r_g1 = L.take<uint8_t>(96 * rows), r_g2 = L.take<uint8_t>(192 * rows);
    const auto r_off = L.take<uint32_t>(ng + 1), r_ws = L.take<uint32_t>((size_t)BLS_PAIR_WORDS * rows);
    const auto r_flag = L.take<int32_t>(rows);
    const auto r_gt = L.take<uint32_t>((size_t)BLS_GT_WORDS * ng);
    const auto r_bad = L.take<int32_t>(ng), r_verdict = L.take<int32_t>(ng);
    const auto r_out = L.take<uint8_t>(out576 ? 576 * ng : 0);
    Workspace w;
    HIP_TRY(h, w.bind(h->d_bls, L, h->stream));
    if (n_pairs == 0) HIP_TRY(h, w.zero(r_flag, 1));
    if (n_pairs) {
        HIP_TRY(h, w.put(r_g1, g1, 96 * n_pairs));
        HIP_TRY(h, w.put(r_g2, g2, 192 * n_pairs));
    }
    HIP_TRY(h, w.put(r_off, offsets, ng + 1));
    launch_bls_prepare(h->stream, w(r_g1), w(r_g2), n_pairs, w(r_ws), w(r_flag));
    launch_bls_miller(h->stream, w(r_ws), w(r_flag), w(r_off), n_groups, w(r_gt), w(r_bad));
    launch_bls_final_exp(h->stream, w(r_gt), w(r_bad), n_groups, w(r_verdict), out576 ? w(r_out) : nullptr);
    HIP_TRY(h, hipGetLastError());
    if (verdict) HIP_TRY(h, w.get(r_verdict, verdict, ng));
    if (out576) HIP_TRY(h, w.get(r_out, out576, 576 * ng));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return PE_OK;
}

int verify_pairs_run(pe_engine* h, const char* who, uint32_t n, const WireAt& pk_at, const WireAt& msg_at, const WireAt& sig_at,
                     int32_t* verdict)
{
    std::vector<uint8_t> g1((size_t)192 * n), g2((size_t)384 * n);
    std::vector<uint32_t> pair_off((size_t)n + 1);
    for (uint32_t t = 0; t < n; ++t) {
        memcpy(&g1[(size_t)192 * t], pk_at(t), 96);
        memcpy(&g1[(size_t)192 * t + 96], NEG_G1_BE96, 96);
        memcpy(&g2[(size_t)384 * t], msg_at(t), 192);
        memcpy(&g2[(size_t)384 * t + 192], sig_at(t), 192);
        pair_off[t] = 2 * t;
    }
    pair_off[n] = 2 * n;
    return pairing_run(h, who, g1.data(), g2.data(), 2ull * n, pair_off.data(), n, verdict, nullptr);
}

}  // namespace posevo

extern "C" {

int pe_pairing_check(pe_engine* h, const uint8_t* g1_points96, const uint8_t* g2_points192, uint64_t n_pairs,
                     const uint32_t* offsets, uint32_t n_groups, int32_t* verdict)
{
    if (!h || !offsets || (n_groups && !verdict) || (n_pairs && (!g1_points96 || !g2_points192))) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));  // open pipelines complete
    return pairing_run(h, "pe_pairing_check", g1_points96, g2_points192, n_pairs, offsets, n_groups, verdict, nullptr);
}

int pe_profile_pairing_gt(pe_engine* h, const uint8_t* g1_points96, const uint8_t* g2_points192, uint64_t n_pairs,
                          const uint32_t* offsets, uint32_t n_groups, uint8_t* out576)
{
    if (!h || !offsets || (n_groups && !out576) || (n_pairs && (!g1_points96 || !g2_points192))) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));
    return pairing_run(h, "pe_profile_pairing_gt", g1_points96, g2_points192, n_pairs, offsets, n_groups, nullptr, out576);
}

int pe_fast_aggregate_verify(pe_engine* h, const uint32_t* index, const uint32_t* offsets, uint32_t n_groups,
                             const uint8_t* message_points192, const uint8_t* signatures192, int32_t* verdict)
{
    if (!h || !offsets || (n_groups && (!message_points192 || !signatures192 || !verdict))) return PE_ERR_INVALID_ARG;
    if (n_groups && offsets[n_groups] && !index) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));
    if (h->dist_ready()) return refuse_dist(h, "pe_fast_aggregate_verify");
    if (n_groups == 0) return PE_OK;
    if (!h->have_points) return fail(h, PE_ERR_STATE, "pe_fast_aggregate_verify: no pubkeys loaded");
    // the aggregate pubkeys, summed on the device; the pairs (sum, H(m)), (-g1, signature) of every group
    std::vector<uint8_t> sums((size_t)96 * n_groups);
    PE_TRY(pe_g1_sum(h, nullptr, 0, index, offsets, n_groups, sums.data()));
    PE_TRY(verify_pairs_run(
        h, "pe_fast_aggregate_verify", n_groups, [&](uint32_t g) { return &sums[(size_t)96 * g]; },
        [&](uint32_t g) { return message_points192 + (size_t)192 * g; }, [&](uint32_t g) { return signatures192 + (size_t)192 * g; },
        verdict));
    // FastAggregateVerify refuses n = 0, and an identity signature never verifies (the product is 1 there only with an identity
    // aggregate key, which KeyValidate refuses); a bad point keeps its verdict 2
    for (uint32_t g = 0; g < n_groups; ++g)
        if (verdict[g] == 1 && (offsets[g + 1] == offsets[g] || (signatures192[(size_t)192 * g] & 0x40))) verdict[g] = 0;
    return PE_OK;
}

}  // extern "C"
