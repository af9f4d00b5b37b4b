// engine_slash.cpp -- slashing detection: the engine finds the double and surround votes (pe:1128; the reference's
// is_slashable_attestation_data, pe:1134-1143) among the attestations it is handed, the one input of the Store (pe:897,
// equivocating_indices) it could not derive itself.  Every validator "eventually recognises equivocations" in its own view
// (pe:1411-1415): the view is a per-validator history of the first vote per target epoch over a window of H epochs, in
// device memory (kernels.h: epoch-major records), scanned by k_slash_scan (slash_kernels.hip).
//
// What runs on the host: the window, committee resolution of the rows and the de-duplication of AttestationData -- a hash
// map per epoch over the batch's rows, so that the device sees (committee, bits, source, target, id) rows only.  That map
// is the thing to move to the device when device-resident rows (PE_ROWS_RESIDENT) follow.
#include "engine_internal.h"

using namespace posevo;

namespace posevo {

int slasher_reset(pe_engine* h)
{
    auto& sl = h->slasher;
    if (!sl.enabled) return PE_OK;
    for (auto& e : sl.epochs) { e.data.clear(); e.id_of.clear(); }
    sl.have_window = false;
    sl.window = 0;
    HIP_TRY(h, hipMemsetAsync(sl.d_rec.p, 0, 8ull * sl.history * sl.n_val, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return PE_OK;
}

void slasher_release(pe_engine* h)
{
    auto& sl = h->slasher;
    sl.d_rec.release();
    sl.d_ids.release();
    sl.d_counter.release();
    sl.d_evidence.release();
    sl.epochs.clear();
    sl.enabled = false;
    sl.have_window = false;
}

}  // namespace posevo

namespace {

// the slots of the epochs that leave the window when it moves from (w0 - H, w0] to (w1 - H, w1]: those of w0 + 1 .. w1
int advance_window(pe_engine* h, uint64_t w1)
{
    auto& sl = h->slasher;
    const uint64_t H = sl.history;
    if (sl.have_window && w1 > sl.window) {
        const uint64_t steps = std::min<uint64_t>(w1 - sl.window, H);
        for (uint64_t k = 0; k < steps; ++k) {
            const uint64_t slot = (w1 - k) % H;
            sl.epochs[slot].data.clear();
            sl.epochs[slot].id_of.clear();
            HIP_TRY(h, hipMemsetAsync(sl.d_rec.as<uint64_t>() + slot * sl.n_val, 0, 8ull * sl.n_val, h->stream));
        }
    }
    sl.have_window = true;
    sl.window = w1;
    return PE_OK;
}

}  // namespace

extern "C" {

int pe_slasher_enable(pe_engine* h, uint32_t history_epochs, uint32_t max_data_per_epoch)
{
    int rc = need_init(h);
    if (rc) return rc;
    if (history_epochs == 0 || max_data_per_epoch == 0)
        return fail(h, PE_ERR_INVALID_ARG, "pe_slasher_enable: history_epochs and max_data_per_epoch must be positive");
    if (h->n_val == 0) return fail(h, PE_ERR_STATE, "pe_slasher_enable: load the registry first (pe_set_validators)");
    slasher_release(h);
    auto& sl = h->slasher;
    const size_t cells = (size_t)history_epochs * h->n_val;
    hipError_t e = sl.d_rec.ensure(8 * cells, false, nullptr, true);
    if (e == hipSuccess) e = sl.d_ids.ensure(4 * cells, false, nullptr, true);
    if (e == hipSuccess) e = sl.d_counter.ensure(256);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        slasher_release(h);
        return fail(h, PE_ERR_OOM, "pe_slasher_enable: 12 bytes per validator and epoch of history do not fit");
    }
    sl.history = history_epochs;
    sl.max_data = max_data_per_epoch;
    sl.n_val = h->n_val;
    sl.epochs.assign(history_epochs, {});
    sl.enabled = true;
    return slasher_reset(h);
}

int pe_slasher_disable(pe_engine* h)
{
    if (!h) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));
    slasher_release(h);
    return PE_OK;
}

int pe_slasher_ingest(pe_engine* h, const pe_attestation* atts, uint32_t n, const uint8_t* bits_arena, uint64_t arena_len,
                      uint64_t current_epoch, uint32_t flags, int32_t* status, pe_slash_evidence* out_evidence, uint32_t cap,
                      uint32_t* out_n_found)
{
    int rc = need_init(h);  // synchronous: completes the outstanding pipeline work first
    if (rc) return rc;
    auto& sl = h->slasher;
    if (!sl.enabled) return fail(h, PE_ERR_STATE, "pe_slasher_ingest: call pe_slasher_enable first");
    if (sl.n_val != h->n_val) return fail(h, PE_ERR_STATE, "pe_slasher_ingest: the registry changed size, enable the slasher again");
    if (!out_n_found || (n && (!atts || !bits_arena || !status)) || (cap && !out_evidence) || (flags & ~PE_SLASH_APPLY))
        return PE_ERR_INVALID_ARG;
    if (sl.have_window && current_epoch < sl.window)
        return fail(h, PE_ERR_INVALID_ARG, "pe_slasher_ingest: current_epoch may not decrease");
    if (current_epoch >= 0xFFFFFFFEull) return fail(h, PE_ERR_INVALID_ARG, "current epoch must fit 32 bits");
    const bool resident = bits_arena == PE_BITS_RESIDENT;
    if (resident && !h->res_valid) return fail(h, PE_ERR_STATE, "PE_BITS_RESIDENT: no pe_aggregate result is resident");
    const bool dev_bits = !resident && n && bits_on_device(bits_arena);
    const uint64_t H = sl.history, W = current_epoch;

    // ---- pass 1, nothing is changed yet: the window, the committee, the bits' bounds
    struct Acc { CommitteeTable* table; uint32_t pos, size, bits_byte; };
    std::vector<Acc> acc(n);
    std::vector<uint32_t> res_group(resident ? n : 0);
    std::vector<CommitteeTable*> tables;
    uint64_t stage_bits = 0;
    uint32_t n_pass = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const pe_attestation& a = atts[i];
        if (a.target_epoch >= 0xFFFFFFFEull) return fail(h, PE_ERR_INVALID_ARG, "target epoch must fit 32 bits");
        if (a.source_epoch >= 0xFFFFFFFFull) return fail(h, PE_ERR_INVALID_ARG, "source epoch must fit 32 bits");
        if (resident) {
            if (!find_resident(h, a, &res_group[i], i))
                return fail(h, PE_ERR_INVALID_ARG, "PE_BITS_RESIDENT: row is not a row of the last pe_aggregate");
        } else if (!att_bits_in_arena(a.bits_offset, a.n_bits, arena_len)) {
            return fail(h, PE_ERR_INVALID_ARG, "attestation bits exceed the arena");
        }
        int32_t s = PE_ATT_OK;
        acc[i].table = nullptr;
        if (a.target_epoch > W) s = PE_SLASH_FUTURE_TARGET;
        else if (a.target_epoch + H <= W) s = PE_SLASH_TOO_OLD;
        else {
            CommitteeTable* t = find_table(h, a.target_epoch);
            Resolved c;
            if (!t || !t->is_partition || t->n_val_at_load != h->n_val || !t->d_inv_comm.p) s = PE_ATT_NO_COMMITTEE_TABLE;
            else if (!resolve_committee(h, t, a, &c).exists) s = PE_ATT_COMMITTEE_INDEX_OUT_OF_RANGE;
            else if (a.n_bits < c.size) s = PE_ATT_BITS_LENGTH_MISMATCH;
            else {
                acc[i] = {t, c.pos, c.size, 0};
                if (std::find(tables.begin(), tables.end(), t) == tables.end()) tables.push_back(t);
                if (!resident && !dev_bits) stage_bits += (c.size + 7) / 8;
                ++n_pass;
            }
        }
        status[i] = s;
    }
    if (stage_bits > 0xFFFFFFFFull) return fail(h, PE_ERR_CAPACITY, "more than 4 GiB of bits in one call");
    size_t csr_bytes = 0;
    for (CommitteeTable* t : tables) csr_bytes += 4ull * (t->n_committees + 1) + 256;
    Stage st(h);
    PE_TRY(st.reserve(sizeof(SlashRow) * (size_t)n_pass + stage_bits + csr_bytes + 4ull * n_pass +
                      sizeof(SlashTable) * tables.size() + 2048));
    if (cap) {
        hipError_t e = sl.d_evidence.ensure(sizeof(pe_slash_evidence) * (size_t)cap);
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(h, PE_ERR_OOM, "pe_slasher_ingest: evidence buffer"); }
    }
    std::vector<uint8_t> flags_back;
    if (flags & PE_SLASH_APPLY) flags_back.resize(h->n_val);

    // ---- from here on the call changes the history: the window first
    PE_TRY(advance_window(h, W));
    *out_n_found = 0;
    const size_t off_rows = st.alloc(sizeof(SlashRow) * (size_t)n_pass);
    const size_t off_bits = st.alloc(stage_bits + 8);
    const size_t off_list = st.alloc(4ull * n_pass);
    const size_t off_tabs = st.alloc(sizeof(SlashTable) * tables.size());
    std::vector<size_t> off_cs(tables.size());
    for (size_t ti = 0; ti < tables.size(); ++ti) off_cs[ti] = st.alloc(4ull * (tables[ti]->n_committees + 1));
    if (st.overflow()) return fail(h, PE_ERR_OOM, "staging block overflow");
    SlashRow* rows = st.host<SlashRow>(off_rows);
    uint8_t* sbits = st.host<uint8_t>(off_bits);
    // data ids (a hash map per epoch; PE_SLASH_TABLE_FULL) and the device rows, in batch order
    std::vector<uint32_t> row_table, row_pos;
    row_table.reserve(n_pass);
    row_pos.reserve(n_pass);
    uint32_t n_rows = 0, bits_at = 0;
    std::string key(128, '\0');
    for (uint32_t i = 0; i < n; ++i) {
        if (status[i] != PE_ATT_OK) continue;
        const pe_attestation& a = atts[i];
        auto& ep = sl.epochs[a.target_epoch % H];
        memcpy(&key[0], &a, 128);
        auto it = ep.id_of.find(key);
        uint32_t id;
        if (it != ep.id_of.end()) id = it->second;
        else if (ep.data.size() >= sl.max_data) { status[i] = PE_SLASH_TABLE_FULL; continue; }
        else {
            id = (uint32_t)ep.data.size();
            std::array<uint8_t, 128> d;
            memcpy(d.data(), &a, 128);
            ep.data.push_back(d);
            ep.id_of.emplace(key, id);
        }
        SlashRow& r = rows[n_rows];
        r.n_bits = acc[i].size;
        r.source = (uint32_t)a.source_epoch;
        r.target = (uint32_t)a.target_epoch;
        r.id = id;
        r.pad[0] = r.pad[1] = r.pad[2] = 0;
        if (resident) r.bits_byte = 4u * h->res_groups[res_group[i]].word;
        else if (dev_bits) r.bits_byte = a.bits_offset;
        else {
            r.bits_byte = bits_at;
            memcpy(sbits + bits_at, bits_arena + a.bits_offset, (acc[i].size + 7) / 8);
            bits_at += (acc[i].size + 7) / 8;
        }
        row_table.push_back((uint32_t)(std::find(tables.begin(), tables.end(), acc[i].table) - tables.begin()));
        row_pos.push_back(acc[i].pos);
        acc[i].table->stamp = ++h->table_stamp;
        ++n_rows;
    }
    if (n_rows == 0) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));  // the window's memsets
        return PE_OK;
    }
    // per table: the CSR of batch rows per committee (rows in batch order), as k_lmd_validator_major reads it
    uint32_t* list = st.host<uint32_t>(off_list);
    SlashTable* tabs = st.host<SlashTable>(off_tabs);
    uint32_t list_at = 0;
    for (size_t ti = 0; ti < tables.size(); ++ti) {
        const uint32_t nc = tables[ti]->n_committees;
        uint32_t* cs = st.host<uint32_t>(off_cs[ti]);
        memset(cs, 0, 4ull * (nc + 1));
        for (uint32_t k = 0; k < n_rows; ++k)
            if (row_table[k] == ti) cs[row_pos[k] + 1] += 1;
        cs[0] = list_at;
        for (uint32_t c = 0; c < nc; ++c) cs[c + 1] += cs[c];
        std::vector<uint32_t> cur(cs, cs + nc);
        for (uint32_t k = 0; k < n_rows; ++k)
            if (row_table[k] == ti) list[cur[row_pos[k]]++] = k;
        list_at = cs[nc];
        tabs[ti].inv_comm = tables[ti]->d_inv_comm.as<uint32_t>();
        tabs[ti].inv_pos = tables[ti]->d_inv_pos.as<uint32_t>();
        tabs[ti].crow_start = st.dev<uint32_t>(off_cs[ti]);
    }
    SlashArgs ka{};
    ka.rows = st.dev<SlashRow>(off_rows);
    ka.tables = st.dev<SlashTable>(off_tabs);
    ka.n_tables = (uint32_t)tables.size();
    ka.crow_list = st.dev<uint32_t>(off_list);
    ka.bits = resident ? h->arena[h->res_arena].d_res_bits.as<uint8_t>() : dev_bits ? bits_arena : st.dev<uint8_t>(off_bits);
    ka.rec = sl.d_rec.as<unsigned long long>();
    ka.ids = sl.d_ids.as<uint32_t>();
    ka.history = sl.history;
    ka.n_val = h->n_val;
    ka.counter = sl.d_counter.as<uint32_t>();
    ka.evidence = sl.d_evidence.as<uint32_t>();
    ka.cap = cap;
    ka.flags = (flags & PE_SLASH_APPLY) ? h->d_flags.as<uint8_t>() : nullptr;
    HIP_TRY(h, st.upload());
    HIP_TRY(h, hipMemsetAsync(ka.counter, 0, 4, h->stream));
    launch_slash_scan(h->stream, ka);
    HIP_TRY(h, hipGetLastError());
    uint32_t found = 0;
    HIP_TRY(h, hipMemcpyAsync(&found, ka.counter, 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *out_n_found = found;
    if (found && cap)
        HIP_TRY(h, hipMemcpy(out_evidence, ka.evidence, sizeof(pe_slash_evidence) * (size_t)std::min(found, cap),
                             hipMemcpyDeviceToHost));
    if (found && (flags & PE_SLASH_APPLY)) {  // the host mirror pe_get_validator_flags and the next flag upload read
        HIP_TRY(h, hipMemcpy(flags_back.data(), h->d_flags.p, h->n_val, hipMemcpyDeviceToHost));
        for (uint64_t v = 0; v < h->n_val; ++v) h->h_flags[v] |= flags_back[v] & PE_VAL_EQUIVOCATING;
    }
    return PE_OK;
}

int pe_slasher_get_data(pe_engine* h, uint64_t target_epoch, uint32_t id, pe_attestation* out)
{
    if (!h || !out) return PE_ERR_INVALID_ARG;
    const auto& sl = h->slasher;
    if (!sl.enabled) return fail(h, PE_ERR_STATE, "pe_slasher_get_data: call pe_slasher_enable first");
    if (!sl.have_window || target_epoch > sl.window || target_epoch + sl.history <= sl.window)
        return fail(h, PE_ERR_INVALID_ARG, "pe_slasher_get_data: target epoch outside the window");
    const auto& ep = sl.epochs[target_epoch % sl.history];
    if (id >= ep.data.size()) return fail(h, PE_ERR_INVALID_ARG, "pe_slasher_get_data: no such data id");
    memset(out, 0, sizeof(*out));
    memcpy(out, ep.data[id].data(), 128);
    return PE_OK;
}

int pe_slasher_get_records(pe_engine* h, uint64_t target_epoch, uint32_t* out_source_epoch, uint32_t* out_id, uint64_t n)
{
    if (!h || (n && (!out_source_epoch || !out_id))) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));
    const auto& sl = h->slasher;
    if (!sl.enabled) return fail(h, PE_ERR_STATE, "pe_slasher_get_records: call pe_slasher_enable first");
    if (n != sl.n_val) return fail(h, PE_ERR_INVALID_ARG, "pe_slasher_get_records: n differs from the registry size");
    for (uint64_t v = 0; v < n; ++v) out_source_epoch[v] = out_id[v] = NONE32;
    if (!sl.have_window || target_epoch > sl.window || target_epoch + sl.history <= sl.window) return PE_OK;
    const uint64_t slot = target_epoch % sl.history;
    std::vector<uint64_t> rec(n);
    std::vector<uint32_t> ids(n);
    HIP_TRY(h, hipMemcpy(rec.data(), sl.d_rec.as<uint64_t>() + slot * n, 8 * n, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(ids.data(), sl.d_ids.as<uint32_t>() + slot * n, 4 * n, hipMemcpyDeviceToHost));
    for (uint64_t v = 0; v < n; ++v) {
        if (rec[v] == 0) continue;
        out_source_epoch[v] = (uint32_t)rec[v];
        out_id[v] = ids[v];
    }
    return PE_OK;
}

}  // extern "C"
