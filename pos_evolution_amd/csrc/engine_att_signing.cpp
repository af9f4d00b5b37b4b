// engine_att_signing.cpp -- pe_attestation_signing_roots: the 32-byte messages attestation signatures are over, from rows
// (DESIGN.md 3.12).  The seam of pe_verify_resident_data, as pe_map_to_g2 is pe_hash_to_g2's: the same kernel
// (k_att_signing_roots, the rule of att_signing_row.h) over row i of the caller's array instead of the first row of group g.
// Rows and roots each lie in host or device memory; synchronous on the engine's stream over a workspace in d_bls; one GPU:
// PE_ERR_STATE under pe_dist_init* and inside a pipeline.  No store and no registry is needed.
#include "att_signing_row.h"
#include "engine_internal.h"

using namespace posevo;

static_assert(sizeof(pe_attestation) == 4 * ATT_ROW_WORDS, "att_signing_row.h reads a row as 36 words");
static_assert(offsetof(pe_attestation, source_epoch) == 4 * ATT_W_SOURCE_EPOCH && offsetof(pe_attestation, source_root) == 4 * ATT_W_SOURCE_ROOT &&
                  offsetof(pe_attestation, target_epoch) == 4 * ATT_W_TARGET_EPOCH && offsetof(pe_attestation, target_root) == 4 * ATT_W_TARGET_ROOT &&
                  offsetof(pe_attestation, index) == 4 * ATT_W_INDEX && offsetof(pe_attestation, beacon_block_root) == 4 * ATT_W_BLOCK_ROOT,
              "att_signing_row.h restates the fields' places");
static_assert(sizeof(pe_attester_domains) == 72, "pe_attester_domains");

namespace {
constexpr uint32_t ATT_SIGNING_MAX_N = 1u << 24;  // as pe_hash_to_g2, which takes the roots
}

extern "C" {

int pe_attestation_signing_roots(pe_engine* h, const pe_attestation* rows, uint32_t n, const pe_attester_domains* dom,
                                 uint8_t* out_roots32)
{
    const char* who = "pe_attestation_signing_roots";
    if (!h) return PE_ERR_INVALID_ARG;
    if (!dom) return fail(h, PE_ERR_INVALID_ARG, std::string(who) + ": no domains");
    if (n && (!rows || !out_roots32)) return fail(h, PE_ERR_INVALID_ARG, std::string(who) + ": no rows or no output");
    if (h->pipelining) return fail(h, PE_ERR_STATE, std::string(who) + ": inside a pipeline (the call is synchronous)");
    PE_TRY(enter(h));
    if (h->dist_ready()) return refuse_dist(h, who);
    if (n > ATT_SIGNING_MAX_N) return fail(h, PE_ERR_CAPACITY, std::string(who) + ": more than 2^24 rows in one call");
    if (n == 0) return PE_OK;
    const size_t row_bytes = sizeof(pe_attestation) * (size_t)n, out_bytes = 32 * (size_t)n;
    const MemKind row_kind = mem_kind(rows), out_kind = mem_kind(out_roots32);
    const bool rows_in_place = reads_in_place(row_kind, rows), out_in_place = reads_in_place(out_kind, out_roots32);
    Layout L;
    const auto r_rows = L.take<uint8_t>(rows_in_place ? 0 : row_bytes);
    const auto r_out = L.take<uint8_t>(out_in_place ? 0 : out_bytes);
    hipStream_t s = h->stream;
    Workspace w;
    HIP_TRY(h, w.bind(h->d_bls, L, s));
    const uint8_t* d_rows = nullptr;
    HIP_TRY(h, device_view(w, r_rows, row_kind, reinterpret_cast<const uint8_t*>(rows), row_bytes, &d_rows));
    AttDomains d;
    att_domains_load(dom->fork_epoch, dom->domain_previous, dom->domain_current, d);
    uint8_t* d_out = out_in_place ? out_roots32 : w(r_out);
    launch_att_signing_roots(s, d_rows, n, nullptr, nullptr, n, d, d_out);
    HIP_TRY(h, hipGetLastError());
    if (!out_in_place)
        HIP_TRY(h, hipMemcpyAsync(out_roots32, d_out, out_bytes,
                                  out_kind == MemKind::Device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return PE_OK;
}

}  // extern "C"
