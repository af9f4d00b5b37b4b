// engine_slash.cpp -- slashing detection: the engine finds the double and surround votes (pe:1128; the reference's
// is_slashable_attestation_data, pe:1134-1143) among the attestations it is handed, the one input of the Store (pe:897,
// equivocating_indices) it could not derive itself.  Every validator "eventually recognises equivocations" in its own view
// (pe:1411-1415): the view is a per-validator history of the first vote per target epoch over a window of H epochs, in
// device memory (kernels.h: epoch-major records), scanned by k_slash_scan (slash_kernels.hip).
//
// Two routes lead to that scan.  HOST ROWS: the host keeps the window, resolves the rows' committees and de-duplicates
// AttestationData in a hash map per epoch, so that the device sees (committee, bits, source, target, id) rows only.
// DEVICE ROWS (PE_ROWS_RESIDENT: the groups of the last pe_aggregate over rows in device memory): the host keeps the window
// and reads nothing of the rows; the k_slash_rows_* kernels judge the groups, take the ids from per-slot tables in device
// memory and write the scan's rows and lists (kernels.h, SlashRowsArgs).  Committees are the ones the aggregate resolved:
// only groups of the store's current and previous epoch take part there.
//
// Both routes hand out ONE sequence of ids per epoch slot.  One side of the data tables is current at a time
// (Slasher::on_device); a call of the other route first rebuilds its side from the current one (to_host: a download and
// the maps again; to_device: an upload and k_slash_table_build), so a handle that keeps to one route never pays for the other.
#include "engine_internal.h"

using namespace posevo;

namespace posevo {

int slasher_reset(pe_engine* h)
{
    auto& sl = h->slasher;
    if (!sl.enabled) return PE_OK;
    for (auto& e : sl.epochs) { e.data.clear(); e.id_of.clear(); }
    sl.on_device = false;  // both sides are empty; the device side is cleared when a call turns to it (to_device)
    std::fill(sl.dev_count.begin(), sl.dev_count.end(), 0u);
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
    sl.d_data.release();
    sl.d_count.release();
    sl.d_tab.release();
    sl.d_work.release();
    sl.epochs.clear();
    sl.dev_count.clear();
    sl.on_device = false;
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
            if (sl.on_device) {  // the slot's table goes with its records
                sl.dev_count[slot] = 0;
                HIP_TRY(h, hipMemsetAsync(sl.d_count.as<uint32_t>() + slot, 0, 4, h->stream));
                HIP_TRY(h, hipMemsetAsync(sl.d_tab.as<uint32_t>() + slot * sl.tab_size, 0xFF, 4ull * sl.tab_size, h->stream));
            }
            HIP_TRY(h, hipMemsetAsync(sl.d_rec.as<uint64_t>() + slot * sl.n_val, 0, 8ull * sl.n_val, h->stream));
        }
    }
    sl.have_window = true;
    sl.window = w1;
    return PE_OK;
}

// the device side becomes current: the host's data per slot go up, every slot's table is built from them
int to_device(pe_engine* h)
{
    auto& sl = h->slasher;
    if (sl.on_device) return PE_OK;
    const uint32_t H = sl.history;
    for (uint32_t slot = 0; slot < H; ++slot) {
        const auto& ep = sl.epochs[slot];
        sl.dev_count[slot] = (uint32_t)ep.data.size();
        if (!ep.data.empty())
            HIP_TRY(h, hipMemcpyAsync(sl.d_data.as<uint8_t>() + 128ull * slot * sl.max_data, ep.data.data(), 128ull * ep.data.size(),
                                      hipMemcpyHostToDevice, h->stream));
    }
    HIP_TRY(h, hipMemcpyAsync(sl.d_count.p, sl.dev_count.data(), 4ull * H, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemsetAsync(sl.d_tab.p, 0xFF, 4ull * H * sl.tab_size, h->stream));
    if (std::any_of(sl.dev_count.begin(), sl.dev_count.end(), [](uint32_t c) { return c != 0; })) {
        launch_slash_table_build(h->stream, sl.d_data.as<uint8_t>(), sl.d_count.as<uint32_t>(), sl.d_tab.as<uint32_t>(), sl.max_data,
                                 sl.tab_size - 1, H);
        HIP_TRY(h, hipGetLastError());
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));  // the uploads read the host's vectors
    for (auto& e : sl.epochs) { e.data.clear(); e.id_of.clear(); }
    sl.on_device = true;
    return PE_OK;
}

// ... and back: the data of every slot come down and the maps are built again, ids unchanged
int to_host(pe_engine* h)
{
    auto& sl = h->slasher;
    if (!sl.on_device) return PE_OK;
    std::string key(128, '\0');
    for (uint32_t slot = 0; slot < sl.history; ++slot) {
        auto& ep = sl.epochs[slot];
        ep.data.assign(sl.dev_count[slot], {});
        ep.id_of.clear();
        if (ep.data.empty()) continue;
        HIP_TRY(h, hipMemcpy(ep.data.data(), sl.d_data.as<uint8_t>() + 128ull * slot * sl.max_data, 128ull * ep.data.size(),
                             hipMemcpyDeviceToHost));
        for (uint32_t id = 0; id < ep.data.size(); ++id) {
            memcpy(&key[0], ep.data[id].data(), 128);
            ep.id_of.emplace(key, id);
        }
    }
    sl.on_device = false;
    return PE_OK;
}

// the scan over the rows and lists of `ka`, and what both routes do with its findings
int run_scan(pe_engine* h, const SlashArgs& ka, uint32_t flags, pe_slash_evidence* out_evidence, uint32_t cap,
             uint32_t* out_n_found, std::vector<uint8_t>& flags_back)
{
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

// pe_slasher_ingest(h, PE_ROWS_RESIDENT, cap_rows, PE_BITS_RESIDENT, ...): every group of the resident aggregate, in group order
int ingest_resident_rows(pe_engine* h, uint32_t cap_rows, uint64_t W, uint32_t flags, int32_t* status,
                         pe_slash_evidence* out_evidence, uint32_t cap, uint32_t* out_n_found)
{
    auto& sl = h->slasher;
    if (h->dist_ready()) return fail(h, PE_ERR_STATE, "pe_slasher_ingest: not on a handle that exchanges with other ranks");
    PE_TRY(resident_precheck(h, "pe_slasher_ingest"));
    ResidentParts P;
    PE_TRY(resident_parts(h, &P));
    AttPlan plan;
    HIP_TRY(h, hipMemcpyAsync(&plan, P.plan, sizeof(plan), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (plan.last_error) return plan_error_to_status(h, plan.last_error, "pe_slasher_ingest (PE_ROWS_RESIDENT): the aggregate");
    const uint32_t ng = plan.n_groups;
    if (ng > P.n_in) return fail(h, PE_ERR_NO_DEVICE, "k_att_plan returned more groups than rows");
    if (ng > cap_rows) return fail(h, PE_ERR_CAPACITY, "pe_slasher_ingest: status holds fewer entries than groups were formed");
    // the call's scratch
    uint32_t cand = 64;
    while (cand < 2 * ng) cand <<= 1;
    const TablesDev& T = h->rr.tables;
    uint32_t nc[2];
    for (int t = 0; t < 2; ++t) nc[t] = T.t[t].valid ? T.t[t].n_committees : 0u;
    const size_t n_keys = (size_t)nc[0] + nc[1] + 1;
    Layout L;
    const auto r_err = L.take<uint32_t>(4);
    const auto r_status = L.take<int32_t>(ng);
    const auto r_cslot = L.take<uint32_t>(ng), r_id = L.take<uint32_t>(ng);
    const auto r_rows = L.take<SlashRow>(ng);
    const auto r_cand = L.take<uint32_t>(cand);
    const auto r_cnt = L.take<uint32_t>(n_keys), r_start = L.take<uint32_t>(n_keys), r_cursor = L.take<uint32_t>(n_keys);
    const auto r_list = L.take<uint32_t>(ng);
    const auto r_tabs = L.take<SlashTable>(2);
    Workspace wk;
    hipError_t e = wk.bind(sl.d_work, L, h->stream);
    if (e == hipSuccess && cap) e = sl.d_evidence.ensure(sizeof(pe_slash_evidence) * (size_t)cap);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(h, PE_ERR_OOM, "pe_slasher_ingest: scratch of the call"); }
    std::vector<uint8_t> flags_back;
    if (flags & PE_SLASH_APPLY) flags_back.resize(h->n_val);
    const uint32_t H = sl.history;
    SlashRowsArgs ra{};
    ra.rows = P.rows;
    ra.grp = P.grp;
    ra.n_groups = ng;
    ra.window = W;
    ra.history = H;
    ra.max_data = sl.max_data;
    ra.tab_mask = sl.tab_size - 1;
    ra.slot_of_table[0] = (uint32_t)(T.t[0].epoch % H);
    ra.slot_of_table[1] = T.t[1].valid ? (uint32_t)(T.t[1].epoch % H) : ra.slot_of_table[0];
    ra.data = sl.d_data.as<uint8_t>();
    ra.count = sl.d_count.as<uint32_t>();
    ra.tab = sl.d_tab.as<uint32_t>();
    ra.status = wk(r_status);
    ra.err = wk(r_err);
    ra.cand_tab = wk(r_cand);
    ra.cand_mask = cand - 1;
    ra.cand_slot = wk(r_cslot);
    ra.id = wk(r_id);
    ra.out_rows = wk(r_rows);

    // ---- nothing is changed yet: the check pass (it reads no table) and its error word
    if (ng) {
        uint32_t err = 0;
        HIP_TRY(h, wk.zero(r_err, 4));
        launch_slash_rows_check(h->stream, ra);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, wk.get(r_err, &err, 1));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (err) return fail(h, PE_ERR_INVALID_ARG, "source and target epoch must fit 32 bits");
    }
    PE_TRY(to_device(h));
    // ---- from here on the call changes the history: the window first
    PE_TRY(advance_window(h, W));
    *out_n_found = 0;
    memset(status, 0, 4ull * cap_rows);  // entries past the groups formed read 0
    if (ng == 0) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));  // the window's memsets
        return PE_OK;
    }
    HIP_TRY(h, wk.fill(r_cand, 0xFF, cand));
    launch_slash_rows_lookup(h->stream, ra);
    launch_slash_rows_ids(h->stream, ra);
    launch_slash_rows_emit(h->stream, ra);
    SlashListsArgs la{};
    SlashArgs ka{};
    la.rows = ra.out_rows;
    la.grp = P.grp;
    la.n_groups = ng;
    la.cnt = wk(r_cnt);
    la.start = wk(r_start);
    la.cursor = wk(r_cursor);
    for (int t = 0; t < 2; ++t) {
        la.n_committees[t] = nc[t];
        if (!nc[t]) continue;
        la.table_val[la.n_tables++] = SlashTable{T.t[t].inv_comm, T.t[t].inv_pos, la.start + (t ? nc[0] : 0u)};
        if (CommitteeTable* ct = find_table(h, T.t[t].epoch)) ct->stamp = ++h->table_stamp;
    }
    la.crow_list = wk(r_list);
    la.tables = wk(r_tabs);
    HIP_TRY(h, wk.zero(r_cnt, n_keys));
    launch_slash_rows_lists(h->stream, la);
    HIP_TRY(h, hipGetLastError());
    ka.rows = ra.out_rows;
    ka.tables = la.tables;
    ka.n_tables = la.n_tables;
    ka.crow_list = la.crow_list;
    ka.bits = reinterpret_cast<const uint8_t*>(P.res_bits);
    ka.rec = sl.d_rec.as<unsigned long long>();
    ka.ids = sl.d_ids.as<uint32_t>();
    ka.history = sl.history;
    ka.n_val = h->n_val;
    ka.counter = sl.d_counter.as<uint32_t>();
    ka.evidence = sl.d_evidence.as<uint32_t>();
    ka.cap = cap;
    ka.flags = (flags & PE_SLASH_APPLY) ? h->d_flags.as<uint8_t>() : nullptr;
    HIP_TRY(h, wk.get(r_status, status, ng));
    HIP_TRY(h, hipMemcpyAsync(sl.dev_count.data(), sl.d_count.p, 4ull * H, hipMemcpyDeviceToHost, h->stream));
    if (la.n_tables == 0) {  // no group had a committee: nothing to scan
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        return PE_OK;
    }
    return run_scan(h, ka, flags, out_evidence, cap, out_n_found, flags_back);
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
    // the data tables of the device-row route: per epoch slot D x 128 bytes, a count and T >= 2 D table entries
    uint64_t tab = 2;
    while (tab < 2ull * max_data_per_epoch) tab <<= 1;
    if (e == hipSuccess) e = sl.d_data.ensure(128ull * history_epochs * max_data_per_epoch, false, nullptr, true);
    if (e == hipSuccess) e = sl.d_tab.ensure(4ull * history_epochs * tab, false, nullptr, true);
    if (e == hipSuccess) e = sl.d_count.ensure(4ull * history_epochs + 256);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        slasher_release(h);
        return fail(h, PE_ERR_OOM, "pe_slasher_enable: 12 bytes per validator and epoch of history, and ~136 bytes per "
                                   "AttestationData and epoch, do not fit");
    }
    sl.tab_size = (uint32_t)tab;
    sl.dev_count.assign(history_epochs, 0u);
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
    const bool rows_resident = atts == PE_ROWS_RESIDENT;
    if (rows_resident && bits_arena != PE_BITS_RESIDENT)
        return fail(h, PE_ERR_INVALID_ARG, "pe_slasher_ingest: PE_ROWS_RESIDENT goes with PE_BITS_RESIDENT");
    if (sl.have_window && current_epoch < sl.window)
        return fail(h, PE_ERR_INVALID_ARG, "pe_slasher_ingest: current_epoch may not decrease");
    if (current_epoch >= 0xFFFFFFFEull) return fail(h, PE_ERR_INVALID_ARG, "current epoch must fit 32 bits");
    if (rows_resident) return ingest_resident_rows(h, n, current_epoch, flags, status, out_evidence, cap, out_n_found);
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

    PE_TRY(to_host(h));  // the ids continue where calls over device rows left them
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
    return run_scan(h, ka, flags, out_evidence, cap, out_n_found, flags_back);
}

int pe_slasher_get_data(pe_engine* h, uint64_t target_epoch, uint32_t id, pe_attestation* out)
{
    if (!h || !out) return PE_ERR_INVALID_ARG;
    const auto& sl = h->slasher;
    if (!sl.enabled) return fail(h, PE_ERR_STATE, "pe_slasher_get_data: call pe_slasher_enable first");
    if (!sl.have_window || target_epoch > sl.window || target_epoch + sl.history <= sl.window)
        return fail(h, PE_ERR_INVALID_ARG, "pe_slasher_get_data: target epoch outside the window");
    const uint64_t slot = target_epoch % sl.history;
    const auto& ep = sl.epochs[slot];
    if (id >= (sl.on_device ? sl.dev_count[slot] : ep.data.size()))
        return fail(h, PE_ERR_INVALID_ARG, "pe_slasher_get_data: no such data id");
    memset(out, 0, sizeof(*out));
    if (sl.on_device)  // whichever side is current answers; every call that wrote the tables has completed
        HIP_TRY(h, hipMemcpy(out, sl.d_data.as<uint8_t>() + 128ull * (slot * sl.max_data + id), 128, hipMemcpyDeviceToHost));
    else
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
