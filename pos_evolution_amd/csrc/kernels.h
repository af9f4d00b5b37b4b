// kernels.h -- host-callable launch wrappers around the HIP kernels (internal interface
// between engine_*.cpp and the *.hip translation units; NOT the public ABI -- that is
// include/posevo.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace posevo {

// Function attributes (the opt-in to > 64 KiB of dynamic LDS) are per device: one flag per (kernel tag, device), so that
// a process driving several GPUs through several handles opts every device in.
template <int TAG>
static bool first_use_on_this_device()
{
    static bool done[64] = {false};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64) return true;
    if (done[dev]) return false;
    done[dev] = true;
    return true;
}

constexpr uint32_t NONE32 = 0xFFFFFFFFu;
// Registry / point-table rows: 24 Montgomery words (x | y) padded to 32 = 128 bytes, so that a gathered point is
// exactly one 128-byte memory line (96-byte rows straddle two lines half of the time: PMC showed 2x the
// algorithmic bytes fetched by k_g1_accumulate's random gather).
constexpr int G1_ROW_WORDS = 32;
constexpr int G2_WG_SLOTS = 128;        // point slots per 256-lane workgroup of the G2 kernels (a lane pair per point)
constexpr int G1_WG = 256;             // lanes (task slots) per workgroup of the accumulate kernel
constexpr int G1_LANE_PARTIAL_BYTES = 208;  // a lane's partial on its way to the tree: X | Y | ZZ | ZZZ as 13 limbs of 30 bits each
constexpr int TREE_MAX_BLOCKS = 8192;  // LDS-resident block tree capacity (K_tree)
constexpr int VOTES_MAX_WG = 256;      // workgroups of K_votes = slots of per-workgroup partial totals

// One summation group of the G1 accumulate kernel (device-resident array, built by the host).
//   sum over i in [0, n_members), bit i set (if bits_word != NONE32) of
//   points[ members ? members[member_start + i] : member_start + i ]
struct G1Group {
    uint32_t member_start;  // offset into the members array (or first point index when members == null)
    uint32_t n_members;
    uint32_t bits_word;     // u32-word offset of the group's bitfield in the device bit arena, or NONE32
    uint32_t slot_base;     // first lane slot of this group (aligned to its padded block)
    uint32_t n_tasks;       // ceil(n_members / k)
    uint32_t k;             // members per lane
    uint32_t log2_block;    // padded block = 1 << log2_block slots (<= 8); groups wider than 256 tasks use whole WGs
    uint32_t out_base;      // first slot in the wg-partials buffer; one partial per workgroup the group spans
};

// ---- G1 ----
// 96-byte big-endian uncompressed affine -> 24 u32 Montgomery limbs (x | y); infinity -> all zero.
void launch_g1_convert(hipStream_t s, const uint8_t* be96, uint32_t* mont24, uint64_t n);
// The registry in the accumulation's field form (fp381_s30.h: 13 + 13 balanced limbs of 30 bits per 128-byte row, word 26 =
// the row holds a point), built from the 24-word Montgomery table.
void launch_g1_table_s30(hipStream_t s, const uint32_t* points_mont24, uint32_t* points_s30, uint64_t n);
// Per-lane XYZZ accumulation of k gathered points over that table: one partial per lane slot into lane_partials (limb-major
// per workgroup: ceil(n_slots / 256) * 256 * G1_LANE_PARTIAL_BYTES, the accumulation's own 13 x 30-bit limbs); single-task groups are written
// straight to wg_partials48.  plan_dev (nullable): n_groups / n_slots are read from this device-resident AttPlan instead (the
// arguments are then upper bounds that size the grid); members1: the member array of groups whose G1Group::k has bit 31 set.
struct AttPlan;
void launch_g1_accumulate(hipStream_t s, const uint32_t* points_s30, const uint32_t* members,
                          const uint32_t* bit_arena, const G1Group* groups, uint32_t n_groups, uint32_t n_slots,
                          uint32_t* lane_partials, uint32_t* wg_partials48, const AttPlan* plan_dev = nullptr,
                          const uint32_t* members1 = nullptr, int exclusive = 0, unsigned long long* clock_rec = nullptr,
                          const uint32_t* cmpl = nullptr, const uint32_t* sparse_info = nullptr, uint32_t sparse_max = 0);
// cmpl (nullable): one word per group, written by k_bits_union (UnionArgs::cmpl): NONE32 = the group is summed directly, else
// committee id | candidate table << 31 = the group goes by complement: the accumulation sums the members whose bit is NOT set,
// and k_g1_finish subtracts that from the committee's sum (sums0 / sums1: the candidate tables' per-committee XYZZ sums, 48
// words each, built with the table -- launch_g1_committee_groups + the accumulation + the tree).
void launch_g1_committee_groups(hipStream_t s, const uint32_t* offsets, uint32_t n_committees, uint32_t k, uint32_t log2_block,
                                G1Group* groups);
// The sparse route of the complement: a group that goes by complement, sits inside one block and has at most sparse_max
// absentees (n_members - sparse_info[2 g], the union's popcount as k_bits_union wrote it beside the verdict) is summed by
// k_g1_absentees -- one wave per group: bit scan, compacted index list, a handful of complete adds -- into
// wg_partials48[out_base], the words k_g1_finish reads; k_g1_accumulate and k_g1_tree evaluate the same rule and leave such a
// group alone (sparse_info null or sparse_max 0: no group is sparse, and the three kernels do what they did without the
// route).  The grid covers the upper bound n_groups, like k_g1_finish's.  G1_SPARSE_MAX: the default threshold, a measured
// choice (profiles/NOTES_r17.md); G1_SPARSE_CAP: the most a launch may ask for (the kernel's index list).
constexpr uint32_t G1_SPARSE_MAX = 128;
constexpr uint32_t G1_SPARSE_CAP = 256;
void launch_g1_absentees(hipStream_t s, const uint32_t* points_s30, const uint32_t* members, const uint32_t* members1,
                         const uint32_t* bit_arena, const G1Group* groups, uint32_t n_groups, const AttPlan* plan_dev,
                         const uint32_t* cmpl, const uint32_t* sparse_info, uint32_t sparse_max, uint32_t* wg_partials48);
// exclusive: the launch asks for this much LDS it never touches (more than half a CU's): at most one of its workgroups per CU
constexpr size_t G1_ACC_EXCLUSIVE_LDS = 82 * 1024;
// The compacting LDS tree over each workgroup's 256 lane partials: one 48-u32 XYZZ partial (192 bytes) per
// (group, workgroup) into wg_partials48.
void launch_g1_tree(hipStream_t s, const uint32_t* lane_partials, const G1Group* groups, uint32_t n_groups,
                    uint32_t n_slots, uint32_t* wg_partials48, int one_per_cu = 0, const AttPlan* plan_dev = nullptr,
                    int solo = 0, const uint32_t* cmpl = nullptr, const uint32_t* sparse_info = nullptr,
                    uint32_t sparse_max = 0);
// Per group: add its n_parts partials (stride = part_stride partials apart, starting at first[g] or
// g when first == null), then either write the XYZZ sum (48 u32) or normalise to 96-byte affine.
void launch_g1_finish(hipStream_t s, const uint32_t* partials48, const G1Group* groups, uint32_t n_groups,
                      uint32_t n_parts_fixed, uint32_t part_stride, uint8_t* out_be96, uint32_t* out_xyzz48,
                      const AttPlan* plan_dev = nullptr, const uint32_t* cmpl = nullptr, const uint32_t* sums0 = nullptr,
                      const uint32_t* sums1 = nullptr);

// ---- fork choice ----
struct TreeDev {               // block tree in DFS pre-order (device arrays of n entries)
    const uint32_t* size;      // subtree size of the block at pre-order position i
    const uint32_t* parent;    // pre-order position of the parent (NONE32 for the root of the order)
    const uint32_t* rank;      // rank of the block's root in lexicographic order (tie-break, pe:1114-1116)
    const uint8_t* leaf_ok;    // filter_block_tree's leaf test (Appendix A.3)
    const uint32_t* pos_of_idx;  // insertion index -> pre-order position
    const uint32_t* idx_of_pos;  // pre-order position -> insertion index
    uint32_t n;
};
struct VoteTotals {            // one per K_votes workgroup (VOTES_MAX_WG slots), summed by K_tree
    unsigned long long total_active_balance;
    unsigned long long num_active;
};
// (k_votes and k_tree are launched over VotesArgs / TreeArgs: see "argument blocks" below)

// One resolved attestation (device row).
struct AttRow {
    uint32_t member_base;  // offset of the committee in the device members array
    uint32_t n_bits;
    uint32_t bits_word;    // u32-word offset of its (re-packed, zero-padded) bits in the device arena
    uint32_t block_idx;    // LMD vote: insertion index of beacon_block_root
    uint32_t epoch_p1;     // target.epoch + 1
    uint32_t order;        // position in the batch (first-seen wins among equal epochs, pe:1383/1440)
    uint32_t flag_mask;    // participation flags this attestation earns (process_attestation)
    uint32_t which;        // 0 current / 1 previous epoch participation
    uint32_t slot;         // attestation.data.slot (vote-expiry variant only: recorded with the latest message)
    uint32_t gate;         // index into the gate array (NONE32 = ungated): a non-zero gate word voids the row on the
                           // device (rows handed over resident by pe_aggregate whose members overlapped, A.8)
};
// the row of an accepted attestation: for update_latest_messages (the fork-choice pass) ...
__host__ __device__ inline AttRow att_row_fork_choice(uint32_t member_base, uint32_t n_bits, uint32_t bits_word, uint32_t block_idx,
                                                      uint64_t target_epoch, uint64_t slot, uint32_t order, uint32_t gate)
{
    return AttRow{member_base, n_bits, bits_word, block_idx, (uint32_t)target_epoch + 1, order, 0u, 0u, (uint32_t)slot, gate};
}
// ... and for the flag loop of process_attestation (pe:745-749)
__host__ __device__ inline AttRow att_row_flags(uint32_t member_base, uint32_t n_bits, uint32_t bits_word, uint32_t flag_mask,
                                                uint32_t which, uint32_t order, uint32_t gate)
{
    return AttRow{member_base, n_bits, bits_word, 0u, 0u, order, flag_mask, which, 0u, gate};
}
// update_latest_messages for a batch: phase 1 atomicMax of (epoch+1, ~order), phase 2 winners write.
void launch_lmd_update(hipStream_t s, const AttRow* rows, uint32_t n_rows, const uint32_t* members,
                       const uint32_t* bit_arena, const uint8_t* flags, uint64_t* vote_key, uint32_t* vote_block,
                       uint32_t* vote_slot = nullptr, const uint32_t* gates = nullptr);
// inverse committee map (partition tables only) and the validator-major form of update_latest_messages
void launch_invert_committees(hipStream_t s, const uint32_t* members, const uint32_t* offsets, uint32_t n_committees,
                              uint32_t* inv_comm, uint32_t* inv_pos, uint64_t n_val);
void launch_lmd_validator_major(hipStream_t s, const AttRow* rows, const uint32_t* crow_start,
                                const uint32_t* crow_list, const uint32_t* inv_comm, const uint32_t* inv_pos,
                                const uint32_t* bit_arena, const uint8_t* flags, uint64_t n_val, uint64_t* vote_key,
                                uint32_t* vote_block, uint32_t* vote_slot = nullptr, const uint32_t* gates = nullptr);
// process_attestation flag loop for one round of pairwise-disjoint attestations.
void launch_participation(hipStream_t s, const AttRow* rows, uint32_t n_rows, const uint32_t* members,
                          const uint32_t* bit_arena, const uint16_t* eff_increments,
                          uint64_t base_reward_per_increment, uint32_t* part_cur_words,
                          uint32_t* part_prev_words, uint64_t* numerators, const uint32_t* numerator_slot,
                          const uint32_t* gates = nullptr);
// aggregation_bits = OR over the group's member attestations; count = popcount (wave reduce): k_bits_union, launched
// over UnionArgs (see "argument blocks" below).
struct UnionGroup {
    uint32_t list_start;   // into att_bytes[]: BYTE offsets of the member attestations' bits in the raw arena
    uint32_t n_atts;
    uint32_t n_bits;       // len(aggregation_bits): bits past it in the last word are masked off
    uint32_t out_word;     // word offset of the output bitfield
};

// ---- attestation rows resident in device memory (att_kernels.hip; host side: engine_resident.cpp) ----------------
// pe_aggregate / pe_on_attestation_batch / pe_process_attestation_batch with the rows handed over in device (or
// pinned) memory: grouping by AttestationData (what aggregate_impl does with memcmp on the host), committee
// resolution, validate_on_attestation (A.4) and the asserts of pe:724-730 run on the device; the host enqueues a
// fixed sequence of launches sized by upper bounds and reads nothing of the rows.
constexpr uint32_t ATT_EMPTY = 0xFFFFFFFFu;
struct TableDev {                 // one candidate committee table (the store's current / previous epoch)
    uint64_t epoch;
    const uint32_t* members;
    const uint32_t* offsets;      // n_committees + 1
    const uint32_t* inv_comm;     // validator -> committee id (partition tables)
    const uint32_t* inv_pos;      // validator -> index in its committee
    uint32_t n_committees;
    uint32_t valid;
};
struct TablesDev {
    TableDev t[2];
    uint64_t slots_per_epoch;
};
struct AttPlan {                  // one per resident-rows aggregate: written by k_att_plan's last workgroup (device copy + pinned mirror)
    uint32_t n_groups;
    uint32_t n_slots;             // G1 plan: uniform blocks of 1 << log2_block lane slots, group g at slot g << log2_block
    uint32_t k, log2_block;
    uint32_t out_words, out_bytes;
    uint32_t error;               // 0 or -pe_status of the aggregate (reported when the call completes)
    uint32_t packed_same;         // every union but the last is a whole number of words: word layout == byte layout
    uint32_t n_rows_table[2];     // groups resolved against each candidate table
    uint32_t n_rows_in;
    uint32_t last_error;          // sticky copy of `error` (k_att_members clears `error` for the next call's ingest; the exchange
                                  // kernel of a committee-sharded step runs after it and still has to tell the other ranks)
    unsigned long long total_members;
};
struct AttGroup {                 // one per group, in order of first appearance
    uint32_t rep;                 // first input row of the group
    uint32_t n_atts, list_start, cursor;
    uint32_t n_bits, out_word, out_byte;
    uint32_t table;               // 0 / 1 = candidate table, NONE32 = none
    uint32_t pos, size, member_base;
    uint32_t sig_valid;           // AND of the members' PE_ATT_FLAG_SIGNATURE_VALID
    uint32_t status_agg;          // 0, or the pe_att_status that keeps the group from having a committee
    uint32_t index_over;          // data.index >= committees per slot (pe:727) although the flat committee id exists:
                                  // get_beacon_committee (A.6) does not assert it, process_attestation does
    uint32_t pad[2];
};
struct BlockTableDev {            // the store's blocks for device-side validation (built by refresh_tree)
    const uint32_t* root_tab;     // open addressing: slot -> insertion index (NONE32 = empty), keyed by the root's first 8 bytes
    uint32_t root_mask;
    const uint8_t* roots;         // 32 B per block, by insertion index
    const unsigned long long* slot_pos;  // block slot by pre-order position
    const uint32_t* parent_pos;   // parent's pre-order position
    const uint32_t* pos_of_idx;
    uint32_t n_blocks;
};
struct FcCtx {                    // store scalars validate_on_attestation reads (A.4)
    unsigned long long cur_slot, cur_epoch, prev_epoch, slots_per_epoch;
};
struct StateCtxDev {              // the slice of BeaconState process_attestation reads (pe:722-754), resolved by the host
    unsigned long long slot, cur_epoch, prev_epoch, slots_per_epoch, min_inclusion_delay, sqrt_spe;
    unsigned long long cj_epoch, pj_epoch;
    uint8_t cj_root[32], pj_root[32];
    uint32_t tgt_blk[2];          // get_block_root(state, epoch): [0] current, [1] previous epoch (insertion index)
    uint32_t head_blk[64];        // get_block_root_at_slot(state, slot - spe + j)
    unsigned long long base_reward_per_increment;
};
// k_att_plan runs one lane per input row over as many 256-lane workgroups as the batch needs.  What its workgroups tell each
// other travels through two small records in device memory, both all-zero between launches (the last workgroup to finish
// clears them):
struct PlanSync {                 // sums / maxima over all groups (device-scope atomics) + the arrival ticket
    uint32_t ticket;              // workgroups that have finished their part; the one that draws the last ticket writes the plan
    uint32_t max_size;            // largest committee among the resolved groups
    uint32_t rows_t[2];           // groups resolved against each candidate table
    uint32_t mis_key;             // max of ~g over groups whose union is not a whole number of words (0 = none)
    uint32_t err;                 // max of the groups' error words
    uint32_t pad[2];
    unsigned long long total_members, pad2[3];
};
struct PlanRec {                  // one per workgroup: its own sums (agg) and the sums up to and including it (incl), each value
    unsigned long long agg[3], incl[3], pad[2];  // an 8-byte word with bit 0 = "written" (decoupled look-back, att_kernels.hip)
};
constexpr uint32_t PLAN_WG = 256;
constexpr uint32_t PLAN_MAX_ROWS = 1u << 24;  // rows per resident aggregate (the look-back words hold 24-bit row counts)
struct AttPlanArgs {
    const void* rows; uint32_t n; const uint32_t* n_dev;
    const uint32_t* tab; const uint32_t* cnt_tab; const uint32_t* slot_of;
    uint32_t* rep_of; uint32_t* gid_of_row;
    AttGroup* grp; UnionGroup* ug;
    uint32_t* crow_start[2]; uint32_t* crow_cursor[2]; uint32_t* crow_cnt[2];
    PlanSync* sync; PlanRec* rec;
    AttPlan* plan; AttPlan* plan_host;
    uint64_t out_arena_cap; uint32_t target_slots, slot_cap, min_k, want_pk;
    TablesDev tables;
};
void launch_att_plan(hipStream_t s, const AttPlanArgs& a);
// committee-sharded exchange (pe_aggregate_exchange): the groups of the resident aggregate packed into fixed slots
// ([4 words header | slots x (36 words row, count, reserved, wps words of OR-ed bits)]), and `world` such buffers unpacked
// into one dense batch of rows (36 words each) + bits (wps words per row); *n_dev = rows unpacked
void launch_att_pack(hipStream_t s, const void* rows, const AttGroup* grp, const AttPlan* plan, const uint32_t* res_bits,
                     const uint32_t* res_info, uint32_t slots, uint32_t wps, uint32_t* send);
void launch_att_unpack(hipStream_t s, const uint32_t* recv, uint32_t world, uint32_t slots, uint32_t wps, void* out_rows,
                       uint32_t* out_bits, uint32_t* n_dev, uint32_t* err_host);
// n_bound: upper bound of the groups (sizes the grid); cap: entries of the caller's status / count arrays
void launch_att_validate_state(hipStream_t s, const void* rows, const AttGroup* grp, const AttPlan* plan, uint32_t n_bound,
                               uint32_t cap, BlockTableDev bt, const StateCtxDev& st, const uint32_t* union_info,
                               AttRow* out_rows, int32_t* status_dev, int32_t* status_host, uint32_t* err_host);
// process_attestation's flag loop, one wave per committee: the committee's rows run in batch order inside the wave
// (committees of a partition table touch disjoint validators, so waves are independent).
void launch_participation_tables(hipStream_t s, const AttRow* rows, TablesDev tables, uint32_t* const crow_start[2],
                                 uint32_t* const crow_list[2], const AttPlan* plan, const uint32_t* bit_arena,
                                 const uint16_t* eff_increments, uint64_t base_reward_per_increment,
                                 uint32_t* part_cur_words, uint32_t* part_prev_words, uint64_t* numerators,
                                 const uint32_t* gates, uint32_t cap);  // cap: slots of numerators[]; more groups = no-op

// ---- argument blocks: the launch interface of the row and fork-choice kernels ------------------------------------------
// Each of these kernels takes ONE struct by value, and the struct is what its launcher takes: the engine fills a block
// (votes_args, tree_args, engine_resident.cpp) and either launches it now or holds it back (engine_pair.cpp).
// A streaming caller's engine stream carries two independent chains: the fork-choice chain of step N (validate ->
// LMD -> votes -> tree) and the row chain of step N + 1 (ingest -> plan -> members -> union).  Side by side on two
// streams the command processor's queue interleaving costs more than the overlap gives; launched as ONE
// kernel per pair (pair_kernels.hip) -- block ranges of one grid, each range running the body of its own kernel over its
// own block -- they overlap without a second queue.
struct IngestArgs {
    const void* rows; uint32_t n;
    uint32_t* tab; uint32_t* cnt_tab;  // the grouping table (slot -> first row of the class, ATT_EMPTY when free) and the
    uint32_t tab_mask;                 // class sizes; both are left clean by k_att_members
    uint32_t* slot_of;
    uint64_t arena_len; AttPlan* plan;
    void* arena_pad32;                 // 32 bytes behind the copied bit arena, zeroed here
    const uint32_t* n_dev;             // nullable: the row count lives on the device, n bounds it
    const void* arena_src; void* arena_dst;  // arena_src (nullable; device memory, 16-byte aligned): the launch copies
                                             // arena_len bytes to arena_dst itself
};
struct ValidateFcArgs {
    const void* rows; const AttGroup* grp; const AttPlan* plan;
    uint32_t n_bound, cap;  // upper bound of the groups (sizes the grid); entries of the caller's status / count arrays
    BlockTableDev bt; FcCtx fc;
    const uint32_t* union_info; AttRow* out_rows; int32_t* status_dev; int32_t* status_host; uint32_t* count_host;
    uint32_t* err_host;
};
// validator-major LMD update over both candidate tables in one launch (each lane walks its validator's committee of the
// current-epoch table, then of the previous-epoch one); the per-committee row lists are unordered (built with atomics),
// the batch-order rule is applied by comparing AttRow::order.
struct LmdVmArgs {
    const AttRow* rows; TablesDev tables; const uint32_t* crow_start[2]; const uint32_t* crow_list[2];
    const AttPlan* plan; const uint32_t* bit_arena; const uint8_t* flags; uint64_t n_val; uint64_t* vote_key;
    uint32_t* vote_block; uint32_t* vote_slot; const uint32_t* gates;
};
struct MembersArgs {
    const void* rows; uint32_t n; uint32_t* tab; uint32_t* cnt_tab; const uint32_t* slot_of; const uint32_t* rep_of;
    const uint32_t* gid_of_row; AttGroup* grp; AttPlan* plan; uint32_t* ubytes; uint32_t* member_row;
    uint32_t* host_group_of; void* host_out_rows; const uint32_t* n_dev;
    G1Group* g1; uint32_t* crow_cursor[2]; uint32_t* crow_list[2];  // written per group by the lane of its first row
};
// direct[pos] += effective_balance of every counted validator voting for the block at pos.
struct VotesArgs {
    const uint32_t* vote_block; const uint64_t* eff_balance; const uint8_t* flags; uint64_t n_val;
    uint32_t filter_slashed; const uint32_t* pos_of_idx; uint32_t n_blocks; uint64_t* direct; VoteTotals* totals;
    const uint32_t* vote_slot; uint32_t min_vote_slot;  // vote-expiry variant: nullptr / 0 without it
};
struct UnionArgs {
    const UnionGroup* groups; uint32_t n_groups; const uint32_t* att_bytes;
    const uint8_t* bit_arena;  // the caller's packed bit arena as uploaded (any byte alignment per member; readable 8 bytes
                               // past the last member)
    uint32_t* out_arena;
    uint32_t* out_info;        // [2g] = popcount of the union, [2g + 1] = sum of the members' popcounts minus that: non-zero
                               // <=> members of the group overlap (their signatures would be counted twice, A.8)
    uint32_t* host_arena; uint32_t* host_info;  // nullable: the same two outputs written a second time straight into
                               // host-coherent pinned memory, so that no device-to-host copy command has to follow the kernel
    const AttPlan* plan_dev;   // nullable: the group count lives on the device, n_groups bounds it
    // nullable: the complement verdict of every group, decided here once (the popcount exists here first) and read by
    // k_g1_accumulate and k_g1_finish: cmpl[g] = grp[g].pos | grp[g].table << 31 when the group is a whole committee of a
    // candidate table whose sums are valid (sums_ok) and 2 * popcount(union) > committee size; NONE32 otherwise
    uint32_t* cmpl; uint32_t* host_cmpl; const AttGroup* grp; uint32_t sums_ok[2];
};
// Subtree sums (prefix scan over pre-order), viability, best child, the descent to the head.
struct TreeArgs {
    TreeDev tree; uint64_t* direct; const VoteTotals* totals; uint64_t ov_balance, ov_num; int use_override;
    uint32_t justified_pos, boost_pos; uint64_t slots_per_epoch, boost_percent, balance_increment;
    uint64_t* weights_by_idx; uint32_t* head_idx; int clear_direct;
};
// pe_prune: vote_block[v] = map[vote_block[v]] for every latest message that names a block of the old table.
struct RemapArgs {
    uint32_t* vote_block; uint64_t n_val;  // padded to a multiple of four entries, 16-byte aligned
    const uint32_t* map; uint32_t n_old;   // old insertion index -> new one, VOTE_PRUNED where the block goes; n_old <= TREE_MAX_BLOCKS
    unsigned long long* counts;            // [0] += messages whose index changed (block kept), [1] += messages orphaned
};
constexpr uint32_t VOTE_PRUNED = 0xFFFFFFFEu;  // PE_VOTE_PRUNED (include/posevo.h)
constexpr int REMAP_WG = 256;
constexpr unsigned REMAP_MAX_WG = 256;  // grid cap: one pass covers REMAP_MAX_WG * REMAP_WG * 4 validators, then the grid strides
// the stand-alone launches (lean: the shapes that fit beside a running accumulation)
void launch_votes_remap(hipStream_t s, const RemapArgs& a);
void launch_att_ingest(hipStream_t s, const IngestArgs& a);
void launch_att_validate_fc(hipStream_t s, const ValidateFcArgs& a);
void launch_lmd_vm_tables(hipStream_t s, const LmdVmArgs& a);
void launch_att_members(hipStream_t s, const MembersArgs& a);
void launch_votes(hipStream_t s, const VotesArgs& a, int lean);
// zeroes a caller-owned exchange buffer in front of launch_votes (the engine's own buffers are left zeroed by k_tree)
void votes_clear_exchange(hipStream_t s, uint64_t* direct, uint32_t n_blocks, VoteTotals* totals);
void launch_bits_union(hipStream_t s, const UnionArgs& a);
void launch_tree(hipStream_t s, const TreeArgs& a, int lean);
// ... and pairwise.  Each returns false when the pair has no common shape (the caller then launches the two alone).
bool launch_pair_ingest_validate(hipStream_t s, const IngestArgs& rows_next, const ValidateFcArgs& fc_prev);
bool launch_pair_plan_lmd(hipStream_t s, const AttPlanArgs& rows_next, const LmdVmArgs& fc_prev);
bool launch_pair_members_votes(hipStream_t s, const MembersArgs& rows_next, const VotesArgs& fc_prev);
bool launch_pair_union_tree(hipStream_t s, const UnionArgs& rows_next, const TreeArgs& fc_prev);
void pair_kernels_preload();  // resolve the pair kernels' code object now rather than inside the first streaming step

// ---- slashing detection (slash_kernels.hip; host side: engine_slash.cpp) -----------------------------------------
// is_slashable_attestation_data (pe:1134-1143) of every new vote of a validator against its history of H target epochs.
// History, epoch-major: rec[(e mod H) * n_val + v] = (target_epoch + 1) << 32 | source_epoch, 0 = empty; ids[...] the data id
// of the record, read only on a hit.  Epoch-major: the lanes of a wave (consecutive validators) read consecutive words of
// every slot whatever their committees, and an epoch that leaves the window is one contiguous memset.
struct SlashRow {                 // one accepted row of the batch; the array is in batch order
    uint32_t bits_byte;           // byte offset of its bits (LSB-first) in the bit arena
    uint32_t n_bits;              // committee length: bit i belongs to the validator at position i
    uint32_t source, target;      // source.epoch, target.epoch
    uint32_t id;                  // id of its AttestationData in the table of its target epoch
    uint32_t pad[3];
};
struct SlashTable {               // one committee table the batch's rows resolve against (a partition of the registry)
    const uint32_t* inv_comm;     // validator -> committee id (NONE32: in none)
    const uint32_t* inv_pos;      // validator -> position in that committee
    const uint32_t* crow_start;   // n_committees + 1: the committee's rows are crow_list[crow_start[c] .. crow_start[c + 1])
};
struct SlashArgs {
    const SlashRow* rows;
    const SlashTable* tables; uint32_t n_tables;
    const uint32_t* crow_list;    // indices into rows[], ascending inside a committee (= batch order)
    const uint8_t* bits;
    unsigned long long* rec; uint32_t* ids; uint32_t history; uint64_t n_val;
    uint32_t* counter;            // evidence found (device-scope counter, zeroed by the launcher's caller)
    uint32_t* evidence; uint32_t cap;  // cap x 6 words {validator, kind, target_1, id_1, target_2, id_2}
    uint8_t* flags;               // nullable: validators with evidence get VAL_EQUIVOCATING (PE_SLASH_APPLY)
};
constexpr int SLASH_NV = 4;       // new votes of one validator held in registers per pass over its history
void launch_slash_scan(hipStream_t s, const SlashArgs& a);

// pe_slasher_ingest over the groups of a resident aggregate (PE_ROWS_RESIDENT): the rows, tables and lists k_slash_scan
// reads are formed on the device from AttGroup[] / the caller's device rows, and the AttestationData ids come from tables
// in device memory.  Per epoch slot s of the window: data[s][id] = the 128 bytes behind id (id < count[s] <= D), and
// tab[s][T] (T a power of two >= 2 D) = open addressing over slash_data_hash of the 128 bytes, entry = id, NONE32 = empty;
// a hit is confirmed by comparing all 128 bytes.  A slot's table only ever holds data of ONE target epoch.
struct SlashRowsArgs {
    const void* rows;             // the caller's device rows (144 B each): a group's data = 128 leading bytes of row grp[g].rep
    const AttGroup* grp; uint32_t n_groups;
    uint64_t window; uint32_t history;  // W, H: the window the statuses are judged against
    uint32_t max_data, tab_mask;        // D, T - 1
    uint32_t slot_of_table[2];          // epoch slot of candidate table 0 / 1 (current / previous epoch of the store)
    uint8_t* data; uint32_t* count; uint32_t* tab;
    int32_t* status;              // per group: pe_att_status / PE_SLASH_*
    uint32_t* err;                // check pass: bit 0 = an epoch of some group does not fit 32 bits
    uint32_t* cand_tab; uint32_t cand_mask;  // the call's candidates (data the slot does not hold yet): entry = lowest group
    uint32_t* cand_slot;          // per group: its entry of cand_tab, NONE32 = not a candidate
    uint32_t* id;                 // per group: the id found / handed out, SLASH_ID_FULL = its data did not fit
    SlashRow* out_rows;           // one per group; n_bits = 0 where the group takes no part
};
constexpr uint32_t SLASH_ID_FULL = 0xFFFFFFFEu;
constexpr uint32_t SLASH_ROWS_WG = 256;
// one lane per group: the 32-bit epoch checks into *err, then window status -> status_agg -> bits length into status[]
void launch_slash_rows_check(hipStream_t s, const SlashRowsArgs& a);
// one lane per passing group: look its data up in its slot's table (read only); unknown data joins cand_tab, where the
// lowest group index of each distinct data stays (cand_tab all NONE32 on entry)
void launch_slash_rows_lookup(hipStream_t s, const SlashRowsArgs& a);
// ONE workgroup walks the groups in tiles of 256: the candidates that cand_tab names are the new data, in group order; new
// id = count[slot] + rank among the new data of the slot (wave scan -> LDS -> carry over tiles); ids below D are inserted
// (table, data bytes), the others are SLASH_ID_FULL; count[] is advanced
void launch_slash_rows_ids(hipStream_t s, const SlashRowsArgs& a);
// one lane per group: the id of its data (its own, or the inserting group's), PE_SLASH_TABLE_FULL, and its SlashRow
void launch_slash_rows_emit(hipStream_t s, const SlashRowsArgs& a);
// the committees' group lists as k_slash_scan wants them, by a counting sort over the groups that take part (the plan's own
// lists are unordered and leave out a group whose bits are longer than its committee): ONE start array over the committees
// of table 0, then of table 1 (table t's crow_start begins at its first committee), one list, each committee's groups
// ascending.  count (a lane per group; cnt zeroed by the caller) -> scan (one workgroup, tiles with a carry; writes
// tables[]) -> fill (a lane per group, in arrival order) -> sort (a lane per committee, in place).
struct SlashListsArgs {
    const SlashRow* rows; const AttGroup* grp; uint32_t n_groups;
    uint32_t n_committees[2];     // 0 = the table takes no part
    uint32_t* cnt; uint32_t* start; uint32_t* cursor;  // n_committees[0] + n_committees[1] + 1 entries each
    uint32_t* crow_list;
    SlashTable* tables; SlashTable table_val[2]; uint32_t n_tables;
};
void launch_slash_rows_lists(hipStream_t s, const SlashListsArgs& a);
// (re)build the tables of every slot from data[] / count[] (tab all NONE32 on entry): grid (ceil(D / 256), H)
void launch_slash_table_build(hipStream_t s, const uint8_t* data, const uint32_t* count, uint32_t* tab, uint32_t max_data,
                              uint32_t tab_mask, uint32_t history);

// The working-state view mirrors the registry (pe_store_init): sflags = active/slashed (+ active-in-previous-epoch),
// increments = balance / effective_balance_increment.
void launch_state_view_from_registry(hipStream_t s, const uint8_t* flags, const uint64_t* balance, uint64_t increment,
                                     uint64_t n_val, uint8_t* sflags, uint16_t* increments);

// BLSPubkey decompression: 48-byte compressed -> Montgomery rows (nullable) and/or 96-byte uncompressed (nullable)
void launch_g1_decompress(hipStream_t s, const uint8_t* in48, uint64_t n, uint32_t* out_mont24, uint8_t* out_be96,
                          int32_t* status);

// KeyValidate's subgroup part over Montgomery rows (128-byte rows): status 0 ok, 3 r*P != infinity, 4 identity
void launch_g1_key_validate(hipStream_t s, const uint32_t* points_mont, uint64_t n, int32_t* status);

// G2 (g2_kernels.hip): same group descriptors, points as 48 Montgomery words [x0 x1 y0 y1], partials 96 words
void launch_g2_convert(hipStream_t s, const uint8_t* be192, uint32_t* mont48, uint64_t n);
void launch_g2_accumulate(hipStream_t s, const uint32_t* points_mont48, const uint32_t* members,
                          const G1Group* groups, uint32_t n_groups, uint32_t n_slots, uint32_t* wg_partials96);
void launch_g2_decompress(hipStream_t s, const uint8_t* in96, uint64_t n, uint32_t* out_mont48, uint8_t* out_be192,
                          int32_t* status);
// up to G2_BATCH_MAX arrays of compressed signatures decoded by one launch (first_block is filled by the launcher)
constexpr uint32_t G2_BATCH_MAX = 8;
struct G2DecompressBatch {
    const uint8_t* in96[G2_BATCH_MAX]; uint32_t* out_mont48[G2_BATCH_MAX]; int32_t* status[G2_BATCH_MAX];
    uint32_t n[G2_BATCH_MAX]; uint32_t first_block[G2_BATCH_MAX + 1]; uint32_t count;
};
void launch_g2_decompress_batch(hipStream_t s, G2DecompressBatch& b);
void launch_g2_finish(hipStream_t s, const uint32_t* partials96, const G1Group* groups, uint32_t n_groups,
                      uint8_t* out_be192);
// r * P == infinity per decoded point: status 0 -> 3 where it fails (non-zero entries are left alone)
void launch_g2_subgroup_check(hipStream_t s, const uint32_t* points_mont48, uint64_t n, int32_t* status);
// rows with a non-zero status become the (0, 0) row (infinity): a plain sum then leaves them out
void launch_g2_mask_bad(hipStream_t s, uint32_t* points_mont48, uint64_t n, const int32_t* status);
// the signature leg of pe_aggregate: per group the sum of its members' signature points (rows member_row[list_start ..
// + n_atts) of `ug`), compressed to the 96-byte BLSSignature wire form; out_bad[g] = members that did not decode
// (for the legs of up to G2_BATCH_MAX steps in one launch; n_groups bounds plan_dev's count; first_block is filled by the launcher)
struct UnionGroup;
struct AttPlan;
struct G2AggregateRowsBatch {
    const uint32_t* pts[G2_BATCH_MAX]; const int32_t* status[G2_BATCH_MAX]; const UnionGroup* ug[G2_BATCH_MAX];
    const uint32_t* member_row[G2_BATCH_MAX]; const AttPlan* plan_dev[G2_BATCH_MAX]; uint8_t* out96[G2_BATCH_MAX];
    uint32_t* out_bad[G2_BATCH_MAX]; uint32_t n_groups[G2_BATCH_MAX]; uint32_t first_block[G2_BATCH_MAX + 1]; uint32_t count;
    // nullable, device memory (pe_verify_resident reads them where they lie): the group's sum as an affine Montgomery row
    // [x0 x1 y0 y1] of 48 words (the rows launch_g2_subgroup_check reads; infinity = the zero row) and a second copy of out_bad
    uint32_t* keep_mont48[G2_BATCH_MAX]; uint32_t* keep_bad[G2_BATCH_MAX];
};
void launch_g2_aggregate_rows(hipStream_t s, G2AggregateRowsBatch& b);
// the per-signature statuses of up to G2_BATCH_MAX legs into their pinned output blocks, one launch (a copy command per leg cost
// the stream ~15 us each)
struct G2StatusOutBatch { const int32_t* src[G2_BATCH_MAX]; int32_t* dst_host[G2_BATCH_MAX]; uint32_t n[G2_BATCH_MAX]; uint32_t count; };
void launch_g2_status_out(hipStream_t s, const G2StatusOutBatch& b);
// pe_aggregate_signatures: a device-resident index list copied with entries >= n replaced by 0 (*err |= 1 then); members per
// group whose status is non-zero (groups: member_start / n_members)
void launch_g2_index_check(hipStream_t s, const uint32_t* index, uint32_t total, uint32_t n, uint32_t* out_index, uint32_t* err);
void launch_g2_count_bad(hipStream_t s, const int32_t* status, const uint32_t* index, const G1Group* groups, uint32_t n_groups,
                         uint32_t* out_bad);

// get_indexed_attestation: sorted attesting indices per row, written at out_offsets[row] (committees <= 8192 members)
void launch_indexed_attestations(hipStream_t s, const AttRow* rows, uint32_t n_rows, const uint32_t* members,
                                 const uint32_t* bit_arena, const uint32_t* out_offsets, uint32_t* out_indices);

// FFG balance sums (pe:791-802): per-workgroup partials [blocks][3] = {total active, previous target, current target};
// returns the number of workgroups launched.
uint32_t launch_ffg_balances(hipStream_t s, const uint64_t* balance, const uint8_t* sflags, const uint8_t* part_cur,
                             const uint8_t* part_prev, uint64_t n_val, uint64_t* partials);

// process_effective_balance_updates (pe:122-133) over the working-state view, in place: eff_balance / increments are
// rewritten where the hysteresis rule moves a validator; *n_changed (device, zeroed by the caller) counts those.
// thresholds = increment / HYSTERESIS_QUOTIENT * {downward, upward} multiplier; max_eff / increment <= 65535.
void launch_effective_balance_update(hipStream_t s, const uint64_t* balances, uint64_t* eff_balance, uint16_t* increments,
                                     uint64_t n_val, uint64_t increment, uint64_t downward_threshold,
                                     uint64_t upward_threshold, uint64_t max_eff, uint64_t* n_changed);

// process_inactivity_updates / process_rewards_and_penalties over the resident balances (reward_kernels.hip; the rule per
// validator and its scalar block are reward_row.h).  Both return the number of workgroups launched = rows of `partials`.
//   launch_reward_sums   partials[wg][REWARD_SUMS_Q]: total active balance, the three unslashed participating balances, the
//                        eligible count (sums), the largest effective balance and score among the eligible (maxima)
//   launch_reward_apply  scores and balances in place; partials[wg][REWARD_APPLY_Q]: rewards credited, penalties debited,
//                        validators with a subtraction cut at 0 (sums)
struct RewardScalars;
constexpr int REWARD_SUMS_Q = 7, REWARD_APPLY_Q = 3;
constexpr uint32_t REWARD_SUMS_MAX_WG = 256, REWARD_APPLY_MAX_WG = 2048;
uint32_t launch_reward_sums(hipStream_t s, const uint64_t* eff_balance, const uint8_t* sflags, const uint8_t* part_prev,
                            const uint64_t* scores, const uint64_t* withdrawable, uint64_t n_val, uint64_t previous_plus_1,
                            uint64_t* partials);
uint32_t launch_reward_apply(hipStream_t s, const RewardScalars& S, const uint64_t* eff_balance, const uint8_t* sflags,
                             const uint8_t* part_prev, const uint64_t* withdrawable, uint64_t n_val, uint64_t* balances,
                             uint64_t* scores, uint64_t* partials);

// compute_proposer_index (pe:604-618), one wave per seed (d_seeds_be: 8 big-endian words each): d_out_proposer[s] = the
// first accepted candidate of seed s, d_out_tries[s] = the i it was accepted at; NONE32 / max_tries when none of the first
// max_tries candidates was.  total >= 1 entries of d_indices (null = identity), every one an index into d_eff_balance;
// rounds <= 255.
void launch_proposer_sample(hipStream_t s, const uint32_t* d_seeds_be, uint32_t n_seeds, uint32_t total, uint32_t rounds,
                            const uint32_t* d_indices, const uint64_t* d_eff_balance, uint64_t max_eff, uint32_t max_tries,
                            uint32_t* d_out_proposer, uint32_t* d_out_tries);

// get_active_validator_indices(state, epoch): the ordered compaction of the registry's active validators
// (activation_epoch[v] <= epoch < exit_epoch[v], unsigned 64-bit), its length and its effective-balance sum in three
// launches on one stream: k_active_compact<false> (per-workgroup counts and balance partials), k_active_scan (one workgroup:
// exclusive offsets, the count, the sum), k_active_compact<true> (the indices, in increasing order, no atomics).
constexpr int ACTIVE_WG = 256;          // T: validators per workgroup of k_active_compact, one lane each
constexpr int ACTIVE_SCAN_TILE = 1024;  // S: workgroup counts one pass of k_active_scan's loop takes, one lane each
struct ActiveTotals { unsigned long long balance; uint32_t n_active; uint32_t pad; };
// d_wg: scratch of active_scratch_bytes(n_val) bytes; d_out_indices: capacity n_val; *d_totals: written by the scan
// (balance = the plain 64-bit sum, the caller applies get_total_balance's floor).  n_val >= 1.
size_t active_scratch_bytes(uint64_t n_val);
void launch_active_compact(hipStream_t s, const uint64_t* d_activation_epoch, const uint64_t* d_exit_epoch, uint64_t epoch,
                           const uint64_t* d_eff_balance, uint64_t n_val, void* d_wg, uint32_t* d_out_indices,
                           ActiveTotals* d_totals);

// PE_VAL_ACTIVE / PE_VAL_ACTIVE_PREV of the working-state view from the registry epochs: activity at current_epoch and at
// previous_epoch; every other bit of sflags[v] is kept.
void launch_activity_flags(hipStream_t s, const uint64_t* d_activation_epoch, const uint64_t* d_exit_epoch,
                           uint64_t current_epoch, uint64_t previous_epoch, uint64_t n_val, uint8_t* sflags);

// process_registry_updates over the resident registry (registry_kernels.hip; the predicates, the exit queue's closed form and
// the scalar block are registry_row.h).  One lane per validator, REGISTRY_WG per workgroup; d_wg: scratch of
// registry_scratch_bytes(n_val) bytes that the launches of one call share.  n_val >= 1 launches; 0 launches nothing.
//   launch_registry_census  read-only: per-workgroup counts and the (largest exit epoch set, holders) pair, then one scan
//                           workgroup: the ejected validators' exclusive offsets and *d_totals (n_counted = fresh ejections)
//   launch_registry_select  read-only: d_hist[256] (zeroed by the caller) += the histogram of byte `byte` of the eligibility
//                           epoch over the queued validators with eligibility >> 8 (byte + 1) == prefix (byte 7: no prefix)
//   launch_registry_ties    read-only: the queued validators at `threshold` per workgroup, their exclusive offsets,
//                           d_totals->n_counted = how many there are (the other fields 0)
//   launch_registry_apply   the writes; -> the device array of validators activated per workgroup, *out_n_wg entries
struct RegistryScalars;
constexpr int REGISTRY_WG = 256;  // validators per workgroup, one lane each; the scans take ACTIVE_SCAN_TILE counts per pass
struct RegistryWgCensus {
    uint32_t n_active, n_marked, n_eject, n_queue;
    unsigned long long max_exit;  // the largest exit epoch below FAR_FUTURE_EPOCH among the workgroup's validators ...
    uint32_t n_at_max, pad;       // ... and how many hold it; 0: none has an exit epoch set
};
struct RegistryTotals {
    unsigned long long n_active, n_marked, n_queue;
    unsigned long long n_counted;  // the total of the scanned column
    unsigned long long max_exit, n_at_max;
};
size_t registry_scratch_bytes(uint64_t n_val);
void launch_registry_census(hipStream_t s, const uint64_t* d_eligibility, const uint64_t* d_activation_epoch,
                            const uint64_t* d_exit_epoch, const uint64_t* d_eff_balance, uint64_t n_val, uint64_t current_epoch,
                            uint64_t finalized_epoch, uint64_t max_effective_balance, uint64_t ejection_balance, void* d_wg,
                            RegistryTotals* d_totals);
void launch_registry_select(hipStream_t s, const uint64_t* d_eligibility, const uint64_t* d_activation_epoch, uint64_t n_val,
                            uint64_t finalized_epoch, uint32_t byte, uint64_t prefix, uint32_t* d_hist);
void launch_registry_ties(hipStream_t s, const uint64_t* d_eligibility, const uint64_t* d_activation_epoch, uint64_t n_val,
                          uint64_t finalized_epoch, uint64_t threshold, void* d_wg, RegistryTotals* d_totals);
const uint32_t* launch_registry_apply(hipStream_t s, const RegistryScalars& S, const uint64_t* d_eff_balance, uint64_t n_val,
                                      void* d_wg, uint64_t* d_eligibility, uint64_t* d_activation_epoch, uint64_t* d_exit_epoch,
                                      uint64_t* d_withdrawable, uint32_t* out_n_wg);

// process_slashings over the resident balances (registry_kernels.hip; registry_row.h).  Both return the number of workgroups
// launched = rows of `partials`.
//   launch_slashings_census  partials[wg][SLASHINGS_CENSUS_Q]: validators the penalty falls on (sum), the largest effective
//                            balance among them (maximum)
//   launch_slashings_apply   balances in place; partials[wg][SLASHINGS_APPLY_Q]: validators penalised, Gwei debited,
//                            subtractions cut at 0 (sums)
struct SlashingScalars;
constexpr int SLASHINGS_CENSUS_Q = 2, SLASHINGS_APPLY_Q = 3;
constexpr uint32_t SLASHINGS_CENSUS_MAX_WG = 256, SLASHINGS_APPLY_MAX_WG = 2048;
uint32_t launch_slashings_census(hipStream_t s, const uint64_t* eff_balance, const uint8_t* sflags, const uint64_t* withdrawable,
                                 uint64_t n_val, uint64_t target_epoch, uint64_t* partials);
uint32_t launch_slashings_apply(hipStream_t s, const SlashingScalars& S, const uint64_t* eff_balance, const uint8_t* sflags,
                                const uint64_t* withdrawable, uint64_t n_val, uint64_t* balances, uint64_t* partials);

// Proposer slashings, attester slashings and voluntary exits over the resident registry (block_ops_kernels.hip; the rules, the
// operation as the kernels read it, the scalar block and the totals are block_ops_row.h).  One lane per slot, BLOCK_OPS_WG per
// workgroup; every launch of a call covers n_slots + 1 lanes = block_ops_workgroups(n_slots) workgroups (the last lane holds
// no candidate: it carries the proposer's rewards where nobody slashes the proposer).
//   launch_block_ops_lists    read-only: d_slot_val / d_slot_op[n_slots], d_op_bad[n_ops] (zeroed by the caller) |= a bad list
//   launch_block_ops_resolve  read-only, three kernels: the two tables (u32[n_val] each, 0xFF-filled by the caller) by minima,
//                             then d_slot_ev[n_slots], d_op_status[n_ops] of the single operations, d_op_hit[n_ops] (zeroed by
//                             the caller), the workgroups' partials, their exclusive offsets and *d_totals
//   launch_block_ops_apply    the writes; d_sums[2] (zeroed by the caller) += Gwei debited, subtractions cut at 0
struct BlockOpDev;
struct BlockOpsScalars;
struct BlockOpsTotals;
struct U64Div;
constexpr int BLOCK_OPS_WG = 256;
struct BlockOpsRegistry {  // the resident columns the read-only passes read
    const uint64_t *activation_epoch, *exit_epoch, *withdrawable, *eff_balance, *balances;
    const uint8_t* sflags;
};
struct BlockOpsWgPart {
    uint32_t n_fresh, n_slashed;
    unsigned long long rewards, slashed_balance, max_eff_slashed;
};
struct BlockOpsWgOffset {
    uint32_t fresh, pad;
    unsigned long long rewards;
};
uint32_t block_ops_workgroups(uint32_t n_slots);
void launch_block_ops_lists(hipStream_t s, const BlockOpDev* d_ops, const uint32_t* d_slot_off, uint32_t n_ops,
                            const uint32_t* d_indices, uint64_t n_val, uint32_t n_slots, uint32_t* d_slot_val, uint32_t* d_slot_op,
                            uint32_t* d_op_bad);
void launch_block_ops_resolve(hipStream_t s, const BlockOpDev* d_ops, const uint32_t* d_slot_val, const uint32_t* d_slot_op,
                              const uint32_t* d_op_bad, uint32_t n_slots, const BlockOpsRegistry& R, uint64_t current_epoch,
                              uint64_t shard_committee_period, const U64Div& by_reward_quotient, uint32_t* d_first_potent,
                              uint32_t* d_first_slash, uint8_t* d_slot_ev, uint32_t* d_op_status, uint32_t* d_op_hit,
                              BlockOpsWgPart* d_wg_part, BlockOpsWgOffset* d_wg_offset, uint32_t proposer_index,
                              BlockOpsTotals* d_totals);
void launch_block_ops_apply(hipStream_t s, const BlockOpsScalars& S, const uint32_t* d_slot_val, const uint8_t* d_slot_ev,
                            const BlockOpsWgOffset* d_wg_offset, const uint32_t* d_first_slash, const uint64_t* d_eff_balance,
                            uint64_t* d_exit_epoch, uint64_t* d_withdrawable, uint8_t* d_sflags, uint64_t* d_balances,
                            uint64_t* d_sums);

// Capella's withdrawal sweep and BLS-to-execution changes over the resident registry (withdrawal_kernels.hip; the rules, the
// record and the change as the kernels read them are withdrawals_row.h).  The sweep: one lane per position, WD_WG per
// workgroup, withdrawals_workgroups(bound) workgroups.
//   launch_withdrawals_sweep   read-only, three kernels: d_pos_kind[bound], d_wg_count / d_wg_offset[workgroups], *d_total
//                              (every hit of the sweep) and the first min(total, k) records, WD_RECORD_WORDS words each
//   launch_withdrawals_apply   the write: the balances of `count` records' validators
//   launch_bls_changes_resolve read-only, two kernels: d_first (u32[n_val], 0xFF-filled by the caller) by minima, d_checks and
//                              d_status[n_changes]; a change is CRED_CHANGE_WORDS words
//   launch_bls_changes_apply   the write: the credentials of the valid changes' validators
//   launch_bls_change_signing_roots  d_roots[32 i ..] = compute_signing_root(change i, domain); domain: big-endian words
constexpr int WD_WG = 256;
struct WithdrawalsColumns {  // the resident columns the sweep reads; credentials: 8 words a validator, memory order
    const uint32_t* credentials;
    const uint64_t *withdrawable, *eff_balance, *balances;
};
struct WithdrawalsSweep {
    uint64_t n, start, current_epoch, max_effective_balance, next_index;
    uint32_t bound, k, prefix;  // positions swept | max_withdrawals_per_payload | ETH1_ADDRESS_WITHDRAWAL_PREFIX
};
uint32_t withdrawals_workgroups(uint32_t bound);
void launch_withdrawals_sweep(hipStream_t s, const WithdrawalsColumns& C, const WithdrawalsSweep& S, uint8_t* d_pos_kind,
                              uint32_t* d_wg_count, uint32_t* d_wg_offset, uint32_t* d_total, uint32_t* d_records);
void launch_withdrawals_apply(hipStream_t s, const uint32_t* d_records, uint32_t count, uint64_t n, uint64_t* d_balances);
void launch_bls_changes_resolve(hipStream_t s, const uint32_t* d_changes, uint32_t n_changes, const uint8_t* d_credentials, uint64_t n,
                                uint32_t* d_first, uint32_t* d_checks, uint32_t* d_status);
void launch_bls_changes_apply(hipStream_t s, const uint32_t* d_changes, uint32_t n_changes, const uint32_t* d_status, uint64_t n,
                              uint8_t* d_credentials);
void launch_bls_change_signing_roots(hipStream_t s, const uint32_t* d_changes, uint32_t n_changes, const uint32_t domain[8],
                                     uint32_t* d_roots);

// compute_committee / compute_shuffled_index (pe:495-534) for a whole list: members[i] = indices[shuffled(i)].
// d_source: rounds * ceil(n/256) * 8 words scratch; d_pivots: rounds words; d_indices null = identity.
int launch_shuffle(hipStream_t s, const uint32_t* d_seed_be, uint32_t n, uint32_t rounds, uint32_t* d_source,
                   uint32_t* d_pivots, const uint32_t* d_indices, uint32_t* d_members);

// SSZ merkleisation (ssz_kernels.hip).  A node is 8 words; between passes nodes travel as SHA's big-endian
// words ("word form"), the first pass of a list reads the bytes where they lie.
constexpr uint32_t SSZ_TILE_LOG2 = 10;     // T = 1024 nodes per workgroup and pass, 512 lanes
constexpr uint32_t SSZ_TILE_LOG2_MIN = 6;  // the smallest tile POSEVO_SSZ_TILE_LOG2 may ask for (one wave)
constexpr uint32_t SSZ_ZERO_HASHES = 65;   // Z[0] .. Z[64]
// One pass: the nodes of height `base` in src -> the ceil(m / 2^levels) nodes of height base + levels in out (word form),
// m = ceil(n_bytes / 32), levels <= SSZ_TILE_LOG2.  raw = 1: src is little-endian list bytes (packed basics or Bytes32
// chunks), read in place, every byte at or beyond n_bytes taken as zero (whole 4-byte words of src are read up to the one
// that holds byte n_bytes - 1); raw = 0: src is word-form nodes, n_bytes = 32 m.  A node without a right sibling pairs with
// zero_words[8 * height ..]; a node with no child is not computed.  m >= 1.
void launch_ssz_merkle(hipStream_t s, const void* src, uint64_t n_bytes, int raw, uint32_t base, uint32_t levels,
                       const uint32_t* zero_words, uint32_t* out);
// The 48 -> 32-byte pubkey leaf H(pk[0:32] || pk[32:48] || 0^16) of n keys, written as digest bytes.
void launch_ssz_pubkey_roots(hipStream_t s, const uint8_t* pubkeys48, uint64_t n, uint8_t* out_leaves32);
// hash_tree_root(Validator) (pe:36-45) of every validator, written as digest bytes: out_roots32[32 v ..].
struct SszValidatorArgs {
    const uint8_t* pubkey_leaf32;            // launch_ssz_pubkey_roots' output
    const uint8_t* withdrawal_credentials32;
    const uint64_t* effective_balance;       // the working-state view
    const uint8_t* sflags;                   // ... its flags: VAL_SLASHED is Validator.slashed
    const uint64_t* activation_eligibility_epoch;
    const uint64_t* activation_epoch;
    const uint64_t* exit_epoch;
    const uint64_t* withdrawable_epoch;
    uint64_t n_val;
    uint8_t* out_roots32;
};
void launch_ssz_validator_roots(hipStream_t s, const SszValidatorArgs& a);

// ---- pairing-product check (bls_kernels.hip; host side: engine_bls.cpp) ---------------------------------
// A group is a 16-lane row (six lane pairs = the six Fp2 coefficients of an Fp12 value, fp12.h), a workgroup is one wave.
constexpr uint32_t BLS_GROUPS_PER_WAVE = 4;   // = groups per workgroup
constexpr int BLS_PAIR_WORDS = 144;           // a pair's workspace row: Q.x, Q.y (Fp2), P.x, P.y (Fp), T = X, Y, Z (Fp2), Montgomery
constexpr int BLS_GT_WORDS = 144;             // a group's Fp12 value between the two kernels: c_k component c at 12 (2 k + c)
// the row in fp values (12 words each): Q.x (c0, c1), Q.y (c0, c1), P.x, P.y, then T = (X, Y, Z), two components each
constexpr int BLS_WS_P = 4, BLS_WS_T = 6;
static_assert(BLS_PAIR_WORDS == 12 * (BLS_WS_T + 6), "workspace row");
// pair_flag: the pair contributes | contributes 1 (infinity on a side) | holds a point off its curve
enum { BLS_PAIR_LIVE = 0, BLS_PAIR_SKIP = 1, BLS_PAIR_BAD = 2 };
// wire bytes (96-byte G1, 192-byte G2) -> workspace rows; pair_flag: 0 contributes, 1 infinity on a side, 2 off its curve
void launch_bls_prepare(hipStream_t s, const uint8_t* g1_be96, const uint8_t* g2_be192, uint64_t n_pairs, uint32_t* ws,
                        int32_t* pair_flag);
// the Miller loop of every group over pairs [offsets[g], offsets[g + 1]): gt[g] = the conjugated accumulator, group_bad[g] =
// a pair of the group is flagged 2.  ws / pair_flag hold at least one row even when there is no pair.
void launch_bls_miller(hipStream_t s, uint32_t* ws, const int32_t* pair_flag, const uint32_t* offsets, uint32_t n_groups,
                       uint32_t* gt, int32_t* group_bad);
// verdict[g] = group_bad[g] ? 2 : gt[g]^((p^12 - 1) / r * 3) == 1; out576 (nullable): that power, 12 x 48 bytes big-endian
void launch_bls_final_exp(hipStream_t s, const uint32_t* gt, const int32_t* group_bad, uint32_t n_groups, int32_t* verdict,
                          uint8_t* out576);

// ---- the resident aggregate's verdicts (bls_resident_kernels.hip; host side: engine_resident_verify.cpp) ----
// Group g of the last pe_aggregate_signed over device rows is the two pairs 2g = (aggregate key, H(m)), 2g + 1 = (-g1, aggregate
// signature), built from what that aggregate left in device memory.
struct BlsResidentArgs {
    const uint32_t* pk_xyzz48;     // per group: the aggregate key as k_g1_finish's XYZZ words (ZZ = 0: the identity)
    const uint32_t* sig_mont48;    // per group: the aggregate signature, G2AggregateRowsBatch::keep_mont48
    const uint32_t* sig_bad;       // per group: members left out of it, G2AggregateRowsBatch::keep_bad
    const uint8_t* msg192;         // the message points, wire bytes, 16-byte aligned
    const uint32_t* point_of_row;  // nullable: group g takes point point_of_row[grp[g].rep], else point g
    const uint8_t* neg_g1_be96;    // -g1, wire bytes
    AttGroup* grp;                 // the aggregate's groups (sig_valid is written under PE_VERIFY_APPLY)
    const uint32_t* union_info;    // [2g + 1]: the members of group g overlap
    uint32_t n_groups;
    uint32_t* ws; int32_t* pair_flag; uint32_t* offsets;  // the Miller workspace: 2 n_groups rows and flags, n_groups + 1 offsets
    uint32_t* ident;               // per group: BLS_RES_ID_* of its three points
    const int32_t* sig_status;     // per group: k_g2_subgroup_check's word over sig_mont48 (0 where the pass did not run)
    const int32_t* fe_verdict;     // per group: k_bls_final_exp's word
    int32_t* verdict;              // per group: out
    uint32_t* stats;               // BLS_RES_REASONS counters, zeroed by the caller: groups per deciding row of the table
    uint32_t apply;
};
enum { BLS_RES_ID_KEY = 1, BLS_RES_ID_SIG = 2, BLS_RES_ID_MSG = 4 };
// the row of the rule table that decided a group (include/posevo.h, pe_verify_resident), in precedence order
enum { BLS_RES_NO_COMMITTEE = 0, BLS_RES_BAD_MESSAGE, BLS_RES_OVERLAP, BLS_RES_BAD_MEMBER, BLS_RES_EMPTY_KEY, BLS_RES_IDENTITY_SIG,
       BLS_RES_IDENTITY_MSG, BLS_RES_NOT_G2, BLS_RES_PAIRING, BLS_RES_REASONS };
constexpr int32_t BLS_UNDECIDED = 3;  // PE_BLS_UNDECIDED
// a lane pair per pair: workspace rows, pair flags, offsets and identity words of every group
void launch_bls_resident_prepare(hipStream_t s, const BlsResidentArgs& a);
// a lane per group: the rule table over the final exponentiation's word and everything the aggregate knew already
void launch_bls_resident_settle(hipStream_t s, const BlsResidentArgs& a);

// ---- batch verification by random linear combination (bls_batch_kernels.hip; host side: engine_batch.cpp) ----
constexpr uint32_t BLS_BATCH_FAN = 8;  // F: Fp12 values one row of k_bls_gt_product multiplies per launch
// a group's state after the settle pass; k_g2_subgroup_check turns LIVE into NOT_G2 (its own status 3)
enum { BLS_BATCH_LIVE = 0, BLS_BATCH_IDENTITY = 1, BLS_BATCH_BAD = 2, BLS_BATCH_NOT_G2 = 3 };
// wire bytes -> Montgomery rows (pk: x, y; G2: x0 x1 y0 y1, the layout launch_g2_subgroup_check reads) and status[g]
void launch_bls_batch_settle(hipStream_t s, const uint8_t* pk96, const uint8_t* msg192, const uint8_t* sig192, uint32_t n_groups,
                             uint32_t* pk_mont24, uint32_t* msg_mont48, uint32_t* sig_mont48, int32_t* status);
// live group i = group live[i]: row (i / chunk) (chunk + 1) + i % chunk of ws = (scalars[g] pk_g, H(m_g)); pair_flag set
void launch_bls_scale_g1(hipStream_t s, const uint32_t* live, uint32_t n_live, uint32_t chunk, const uint64_t* scalars,
                         const uint32_t* pk_mont24, const uint32_t* msg_mont48, uint32_t* ws, int32_t* pair_flag);
// scaled96[i] = scalars[g] sig_g as an XYZZ point (G2X_WORDS words)
void launch_bls_scale_g2(hipStream_t s, const uint32_t* live, uint32_t n_live, const uint64_t* scalars, const uint32_t* sig_mont48,
                         uint32_t* scaled96);
// chunk j: row j (chunk + 1) + (its live groups) of ws = (-g1, the sum of its scaled96); pair_flag set
void launch_bls_chunk_sig(hipStream_t s, const uint32_t* scaled96, uint32_t n_live, uint32_t chunk, uint32_t n_chunks,
                          const uint8_t* neg_g1_be96, uint32_t* ws, int32_t* pair_flag);
// out[o] = the product of in[o F .. o F + F) (BLS_GT_WORDS each), n_out = ceil(n_in / F)
void launch_bls_gt_product(hipStream_t s, const uint32_t* in, uint32_t n_in, uint32_t* out, uint32_t n_out);

// ---- per-member signature verification: weighted sums per committee (sigverify_kernels.hip; host side: engine_sigverify.cpp) ----
constexpr uint32_t SV_STRIPE_MAX = 16;  // members per slot at most: a plane's mask of set members is 16 bits
// wg_partials96 = per (group, workgroup) sum of scalars[m] * row (index ? index[m] : m) of points_mont48 over the group's members
// m: k_g2_accumulate's plan and partials (launch_g2_finish takes them), G1Group::k <= SV_STRIPE_MAX
void launch_g2_weighted_accumulate(hipStream_t s, const uint32_t* points_mont48, const uint32_t* index, const uint64_t* scalars,
                                   const G1Group* groups, uint32_t n_groups, uint32_t n_slots, uint32_t* wg_partials96);
// the same over registry rows (G1_ROW_WORDS words each) signer[m]: a plan of G1_WG slots per workgroup, partials of G1X_WORDS
// words as launch_g1_finish takes them
void launch_g1_weighted_accumulate(hipStream_t s, const uint32_t* points_mont, const uint32_t* signer, const uint64_t* scalars,
                                   const G1Group* groups, uint32_t n_groups, uint32_t n_slots, uint32_t* wg_partials48);
// status[i] = code where it is 0 and row i of points_mont48 is the (0, 0) row
void launch_sv_mark_identity(hipStream_t s, const uint32_t* points_mont48, uint64_t n, int32_t* status, int32_t code);
// rows of the registry / of the decoded signatures back to wire bytes (96 / 192 each), for the locate pass
void launch_sv_rows_g1(hipStream_t s, const uint32_t* points_mont, const uint32_t* rows, uint32_t n, uint8_t* out_be96);
void launch_sv_rows_g2(hipStream_t s, const uint32_t* points_mont48, const uint32_t* rows, uint32_t n, uint8_t* out_be192);

// ---- process_deposit (deposit_kernels.hip; host side: engine_deposit.cpp; the rules per deposit: deposit_row.h) ----
// The pubkey index: tab[T] (T a power of two, mask = T - 1) = open addressing over 32-byte leaves (8 words each, memory order),
// entry = the LOWEST key index that holds the slot's leaf, NONE32 = empty.  Keys [first, end) of `leaves` are inserted; where
// only_if_none is not null key v takes part only if only_if_none[v] == NONE32.  out_slot (nullable): the slot key v's leaf
// lives in (NONE32 where it took no part).  The table must keep at least as many empty slots as keys.
void launch_deposit_index_build(hipStream_t s, const uint32_t* leaves, uint64_t first, uint64_t end, const uint32_t* only_if_none,
                                uint32_t* tab, uint32_t mask, uint32_t* out_slot);
// One lane per deposit: the pubkey's leaf (digest bytes, as d_pubkey_leaf holds them), hash_tree_root(DepositData) walked up
// the 33 nodes of its branch (proofs null: not walked, proof_ok = 1) and compare with deposit_root, and (signing_roots not
// null) compute_signing_root(DepositMessage, domain) as digest bytes.
struct DepositLeavesArgs {
    const uint32_t* rows;        // n x DEPOSIT_ROW_WORDS: pe_deposit_data
    uint32_t n;
    const uint32_t* proofs;      // nullable: n x 33 x 8 words
    uint64_t index0;             // eth1_deposit_index of deposit 0
    uint32_t root[8];            // deposit_root, SHA word form
    uint32_t domain[8];          // the domain, SHA word form (read where signing_roots is not null)
    uint32_t* leaf;              // n x 8 words
    uint32_t* proof_ok;          // n
    uint32_t* signing_roots;     // nullable: n x 8 words
};
void launch_deposit_leaves(hipStream_t s, const DepositLeavesArgs& a);
// reg_index[i] = the registry's lowest index whose leaf equals deposit i's in all 32 bytes, or NONE32
void launch_deposit_probe(hipStream_t s, const uint32_t* dep_leaf, uint32_t n, const uint32_t* reg_leaves, const uint32_t* tab,
                          uint32_t mask, uint32_t* reg_index);
// ONE workgroup.  For the deposits that missed the registry (reg_index NONE32; key_slot = their slot of the batch's own table,
// launch_deposit_index_build over dep_leaf): first_valid[slot] (NONE32 on entry) = the key's first position whose sig_ok is
// set; then deposit_status per deposit, the creators' new indices n_val + (creators before them, in batch order), and the
// index every deposit credits (NONE32: none).  counts[0] = creators.
struct DepositResolveArgs {
    uint32_t n;
    uint32_t n_val;
    const uint32_t* reg_index;
    const uint32_t* key_slot;
    const uint32_t* sig_ok;
    const uint32_t* proof_ok;
    uint32_t* first_valid;
    uint32_t* rank;              // n: scratch
    int32_t* status;
    uint32_t* out_index;
    uint32_t* counts;
};
void launch_deposit_resolve(hipStream_t s, const DepositResolveArgs& a);
// One lane per deposit: a credited deposit adds its amount to balances[out_index] (64-bit atomic: several deposits may credit
// one validator; a new validator's balance starts at 0), a creator also writes its validator's rows.
struct DepositApplyArgs {
    const uint32_t* rows;
    uint32_t n;
    const int32_t* status;
    const uint32_t* out_index;
    const uint32_t* dep_leaf;
    uint64_t increment, max_effective_balance, far_future_epoch;  // DepositParams
    uint64_t* balances;
    uint64_t* eff_balance;       // the working-state view ...
    uint8_t* sflags;
    uint16_t* increments;
    uint64_t *activation_eligibility, *activation_epoch, *exit_epoch, *withdrawable_epoch;
    uint32_t* pubkey_leaf;       // 8 words per validator
    uint32_t* withdrawal_credentials;
};
void launch_deposit_apply(hipStream_t s, const DepositApplyArgs& a);

// ---- hash_to_curve for G2 (h2c_kernels.hip; RFC 9380, BLS12381G2_XMD:SHA-256_SSWU_RO_)
constexpr int H2C_POINT_WORDS = 96;  // an XYZZ point over Fp2 between k_h2c_map and k_h2c_finish (g2.h: G2X_WORDS)
// n messages of msg_len bytes back to back -> (u0, u1): 48 Montgomery words a message (u0.c0 | u0.c1 | u1.c0 | u1.c1)
void launch_h2c_expand(hipStream_t s, const uint8_t* msgs, uint32_t n, uint32_t msg_len, const uint8_t* dst, uint32_t dst_len,
                       uint32_t* u_mont);
// n_words canonical 48-byte big-endian values -> Montgomery words (the same rows, from pe_map_to_g2's bytes)
void launch_h2c_load_u(hipStream_t s, const uint8_t* be48, uint32_t n_words, uint32_t* u_mont);
// n_u values of Fp2 (24 words) -> n_u points of E2 as XYZZ (H2C_POINT_WORDS words): simplified SWU, then the 3-isogeny
void launch_h2c_map(hipStream_t s, const uint32_t* u_mont, uint32_t n_u, uint32_t* out_xyzz);
// message i: points 2 i and 2 i + 1 added, the cofactor cleared, 192 wire bytes; status (nullable): 1 where H is the identity
void launch_h2c_finish(hipStream_t s, const uint32_t* pts_xyzz, uint32_t n, uint8_t* out_be192, int32_t* status);

// ---- attestation signing roots (att_signing_kernels.hip; the rule: att_signing_row.h)
struct AttDomains;
// out_roots32[i] = compute_signing_root(AttestationData of a row, get_domain(target.epoch)), 32 bytes each, back to back as
// launch_h2c_expand reads its messages.  grp == nullptr: n roots, of rows 0 .. n - 1.  Else: one root per group of the
// resident aggregate, of row grp[g].rep, for g < min(plan->n_groups, n) -- n is the host's upper bound and sizes the grid.
// rows: n_rows rows of 144 bytes, 4-byte aligned; a rep beyond n_rows gives a zero root.
void launch_att_signing_roots(hipStream_t s, const void* rows, uint32_t n_rows, const AttGroup* grp, const AttPlan* plan,
                              uint32_t n, const AttDomains& dom, uint8_t* out_roots32);

// ---- sync committees (sync_kernels.hip; host side: engine_sync.cpp)
constexpr int SYNC_COMMITTEE_MAX = 512;  // PE_SYNC_COMMITTEE_MAX: positions of a committee, lanes of k_sync_members' workgroup
constexpr int SYNC_MAX_BATCH = 64;       // PE_SYNC_MAX_BATCH: aggregates of one call
constexpr int SYNC_AGG_WORDS = 58;       // sizeof(pe_sync_aggregate) / 4
constexpr int SYNC_SAMPLE_WG = 256;      // candidates per workgroup of k_sync_sample, one lane each
// Candidates one launch examines: 64 workgroups, whose counts one wave scans.  A launch costs a candidate's 91 dependent
// compressions whatever its width until the lanes fill the chip, so the width only has to cover the common cases in one or two
// launches: 512 acceptances at 1 ETH against 32 need 16 384 +- 700 candidates, at full balances 512.
constexpr uint32_t SYNC_SAMPLE_BATCH = 16384;
struct SyncSampleState { uint32_t count, tries; };  // members appended so far | the i of the size-th acceptance + 1
// One batch of get_next_sync_committee_indices: the candidates i in [base, base + SYNC_SAMPLE_BATCH) below max_tries, those
// accepted appended to d_members in the order of i behind the d_state->count already there, up to `size` in all; zero *d_state
// before the first batch.  Arguments as launch_proposer_sample's; d_wg_count: SYNC_SAMPLE_BATCH / SYNC_SAMPLE_WG words,
// d_wg_entry: 2 * SYNC_SAMPLE_BATCH words (8-byte aligned).  1 <= size <= SYNC_COMMITTEE_MAX.  The three launchers of this
// section return 0, or -1 where an argument lies outside what the kernel's arrays are sized for: nothing is launched then.
int launch_sync_sample(hipStream_t s, const uint32_t* d_seed_be, uint32_t total, uint32_t rounds, const uint32_t* d_indices,
                        const uint64_t* d_eff_balance, uint64_t max_eff, uint64_t base, uint64_t max_tries, uint32_t size,
                        uint32_t* d_wg_count, uint32_t* d_wg_entry, SyncSampleState* d_state, uint32_t* d_members);
// d_aggs: n aggregates of SYNC_AGG_WORDS words; d_committee: `size` validator indices.  Per aggregate b: d_lists[b][0 .. d_counts[b])
// = the participants in committee order, d_bad[b] != 0 where a bit at a position >= size is set, d_roots[b] = its signing root
// (32 bytes).  1 <= n <= SYNC_MAX_BATCH.
int launch_sync_members(hipStream_t s, const uint32_t* d_aggs, uint32_t n, const uint32_t* d_committee, uint32_t size,
                         uint32_t* d_lists, uint32_t* d_counts, uint32_t* d_bad, uint32_t* d_roots);
// The aggregates' rewards and penalties onto d_balances, aggregate by aggregate, position by position (one workgroup).  Every
// member and proposer index must lie inside d_balances.  d_stats[3]: Gwei credited | Gwei debited | decreases cut at 0.
int launch_sync_rewards(hipStream_t s, const uint32_t* d_aggs, uint32_t n, const uint32_t* d_committee, uint32_t size,
                         uint64_t participant_reward, uint64_t proposer_reward, uint64_t* d_balances, uint64_t* d_stats);

}  // namespace posevo
