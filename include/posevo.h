/*
 * posevo.h -- C ABI of the MI355X attestation-aggregation + LMD-GHOST engine.
 *
 * The reference (ethereum/pos-evolution, one file: pos-evolution.md, cited as
 * pe:N) has no FFI; its "API" for this path is three pyspec signatures over
 * Python objects:
 *     get_head(store) -> Root                                   pe:1102
 *     on_attestation(store, attestation, is_from_block=False)   pe:963 / pe:1423
 *     process_attestation(state, attestation)                   pe:722
 * plus the handlers that feed them (get_forkchoice_store pe:1077, on_tick
 * pe:934, on_block pe:986, on_attester_slashing pe:1447).  Every entry point
 * below names the reference lines it replaces.  INTEGRATION.md shows the
 * ctypes / cgo stubs a client maintainer would add.
 *
 * Conventions
 *  - plain C: pointers + sizes, no C++ / torch types.  The caller owns every
 *    buffer it passes; the engine owns its handle and all device memory.
 *  - every function returns PE_OK (0) or a negative pe_status; nothing throws.
 *    A failing call leaves the store unmodified ("Invalid calls to handlers
 *    must not modify store", pe:1041).
 *  - one thread per handle at a time (the spec is sequential, pe:929-1039).
 *    Calls are synchronous: they return once their results are complete in the
 *    caller's buffers (pe_get_head polls the head word its kernel releases to host
 *    memory instead of waiting for the stream to drain; later calls are ordered
 *    behind it on the engine's stream).  The exception is opt-in: between pe_pipeline_begin
 *    and pe_pipeline_end the batch calls return once their work is enqueued (see there).
 *  - roots are 32 opaque bytes; the all-zero root is "unset" (Root(), pe:943).
 *  - G1 points cross the boundary in the 96-byte uncompressed form: big-endian
 *    x (48 B) || big-endian y (48 B); bit 6 of byte 0 set = point at infinity.
 *    Outputs are canonical (x, y fully reduced mod p), so equality with the
 *    oracle is integer equality (tolerance 0).
 *  - bitfields are packed LSB-first (bit i = byte i/8, bit i%8), the SSZ
 *    Bitlist order without the length delimiter; n_bits travels beside it.
 */
#ifndef POSEVO_H
#define POSEVO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PE_ABI_VERSION 15

typedef struct pe_engine pe_engine;

typedef enum pe_status {
    PE_OK = 0,
    PE_ERR_INVALID_ARG = -1,
    PE_ERR_NO_DEVICE = -2,      /* no HIP device / HIP runtime failure (message via pe_last_error) */
    PE_ERR_OOM = -3,
    PE_ERR_UNKNOWN_PARENT = -4, /* on_block: assert block.parent_root in store.block_states (pe:990) */
    PE_ERR_FUTURE_BLOCK = -5,   /* on_block: assert get_current_slot(store) >= block.slot (pe:994) */
    PE_ERR_NOT_AFTER_FINALIZED = -6, /* on_block: assert block.slot > finalized_slot (pe:998) */
    PE_ERR_NOT_FINALIZED_DESCENDANT = -7, /* on_block: ancestor-at-finalized-slot check (pe:1000) */
    PE_ERR_DUPLICATE_BLOCK = -8,
    PE_ERR_UNKNOWN_ROOT = -9,
    PE_ERR_CAPACITY = -10,
    PE_ERR_NO_COMMITTEES = -11, /* no committee table loaded for the attestation's target epoch */
    PE_ERR_NOT_SLASHABLE = -12, /* on_attester_slashing: is_slashable_attestation_data false (pe:1453) */
    PE_ERR_INVALID_INDEXED = -13, /* is_valid_indexed_attestation false (pe:1455-1456) */
    PE_ERR_STATE = -14,         /* call sequence error (e.g. store not initialised) */
    PE_ERR_TIMEOUT = -15        /* multi-GPU: a collective did not complete within the engine's bounded wait */
} pe_status;

/* Per-attestation result codes written by the *_batch calls (0 = applied).  Each
 * value names the assert that failed; a rejected attestation changes nothing. */
typedef enum pe_att_status {
    PE_ATT_OK = 0,
    PE_ATT_TARGET_EPOCH_NOT_CURRENT_OR_PREVIOUS = 1, /* validate_target_epoch_against_current_time / pe:724 */
    PE_ATT_TARGET_EPOCH_SLOT_MISMATCH = 2,           /* target.epoch == compute_epoch_at_slot(data.slot), pe:725 */
    PE_ATT_UNKNOWN_TARGET_ROOT = 3,
    PE_ATT_UNKNOWN_BEACON_BLOCK_ROOT = 4,
    PE_ATT_BLOCK_AFTER_ATTESTATION_SLOT = 5,
    PE_ATT_TARGET_NOT_ANCESTOR = 6,                  /* LMD vote must be consistent with FFG vote target */
    PE_ATT_SLOT_NOT_IN_PAST = 7,                     /* get_current_slot(store) >= data.slot + 1 */
    PE_ATT_NO_COMMITTEE_TABLE = 8,
    PE_ATT_COMMITTEE_INDEX_OUT_OF_RANGE = 9,         /* pe:727 */
    PE_ATT_BITS_LENGTH_MISMATCH = 10,                /* len(aggregation_bits) == len(committee), pe:730 */
    PE_ATT_EMPTY_OR_INVALID_INDICES = 11,            /* is_valid_indexed_attestation structural part, pe:736/976 */
    PE_ATT_BAD_SIGNATURE = 12,                       /* injected pairing result false, pe:736/976 */
    PE_ATT_INCLUSION_WINDOW = 13,                    /* pe:726 */
    PE_ATT_SOURCE_MISMATCH = 14,                     /* assert is_matching_source (Appendix A.9) */
    /* pe_slasher_ingest only (values >= 32): the row takes no part in the detection */
    PE_SLASH_FUTURE_TARGET = 32,                     /* target.epoch > current_epoch */
    PE_SLASH_TOO_OLD = 33,                           /* target.epoch + history_epochs <= current_epoch */
    PE_SLASH_TABLE_FULL = 34                         /* new AttestationData for an epoch that already holds max_data_per_epoch */
} pe_att_status;

/* Constants the reference cites by name only (pe:467, 1021-1022, 1054, ...);
 * defaults = mainnet preset. */
typedef struct pe_config {
    uint64_t slots_per_epoch;                 /* 32, pe:472 */
    uint64_t seconds_per_slot;                /* 12, pe:1536 */
    uint64_t intervals_per_slot;              /* 3,  pe:1536 */
    uint64_t safe_slots_to_update_justified;  /* 8,  pe:1054 */
    uint64_t proposer_score_boost;            /* 40 (percent of one slot's committee weight), pe:1355 */
    uint64_t effective_balance_increment;     /* 1e9 Gwei, pe:126 */
    uint64_t min_attestation_inclusion_delay; /* 1, pe:726 */
    uint64_t max_validators_per_committee;    /* 2048, pe:715 */
    uint32_t filter_slashed;                  /* 0: this era's get_latest_attesting_balance ignores `slashed` */
    int32_t  device;                          /* HIP device ordinal; -1 = current device */
    uint64_t reserve_validators;              /* capacity hints (0 = grow on demand) */
    uint32_t reserve_blocks;
    uint32_t max_committee_tables;            /* epochs of committee tables kept resident (0 = 4) */
    uint64_t vote_expiry_slots;               /* 0 = LMD-GHOST (no expiry).  eta > 0: RLMD-GHOST's vote expiry period
                                                 (pe:1585-1596; eta = 1 is Goldfish's GHOST-Eph, pe:1549): get_head
                                                 counts a latest message only if message.slot + eta >= current slot */
} pe_config;

/* Validator flag bits (T1: the per-validator byte the vote kernel streams). */
#define PE_VAL_ACTIVE       0x01u  /* activation_epoch <= current_epoch(justified state) < exit_epoch */
#define PE_VAL_SLASHED      0x02u  /* Validator.slashed (pe:40) */
#define PE_VAL_EQUIVOCATING 0x04u  /* in store.equivocating_indices (pe:897); set by the engine */

/* Attestation row: AttestationData (pe:689-697) + where its Bitlist (pe:715) lives
 * in the caller's bit arena + the injected signature verdict (pe:717). */
#define PE_ATT_FLAG_SIGNATURE_VALID 0x1u  /* result of the out-of-scope pairing check */
#define PE_ATT_FLAG_FROM_BLOCK      0x2u  /* is_from_block (pe:1423) */
#define PE_ATT_FLAG_OVERLAPPING_BITS 0x4u /* set by pe_aggregate on an output row whose members share a bit: the summed
                                             signature counts that validator twice while bits and aggregate pubkey count
                                             it once, so the aggregate can never verify (validator guide, Appendix A.8:
                                             "aggregates with overlapping bits are not merged").  PE_ATT_FLAG_SIGNATURE_VALID
                                             is cleared on such a row; re-aggregate without the duplicate members. */
typedef struct pe_attestation {
    uint64_t slot;                  /* data.slot */
    uint64_t index;                 /* data.index: committee index within the slot */
    uint8_t  beacon_block_root[32]; /* data.beacon_block_root: the LMD GHOST vote */
    uint64_t source_epoch;          /* data.source */
    uint8_t  source_root[32];
    uint64_t target_epoch;          /* data.target */
    uint8_t  target_root[32];
    uint32_t bits_offset;           /* byte offset of aggregation_bits in the arena */
    uint32_t n_bits;                /* len(aggregation_bits) */
    uint32_t flags;                 /* PE_ATT_FLAG_* */
    uint32_t reserved0;
} pe_attestation;                   /* 144 bytes */

/* The slice of BeaconState that process_attestation (pe:722-754) reads. */
typedef struct pe_state_ctx {
    uint64_t slot;                        /* state.slot */
    uint8_t  chain_tip_root[32];          /* latest block of the state's chain: get_block_root* resolve against it */
    uint64_t current_justified_epoch;     /* state.current_justified_checkpoint */
    uint8_t  current_justified_root[32];
    uint64_t previous_justified_epoch;    /* state.previous_justified_checkpoint */
    uint8_t  previous_justified_root[32];
    uint64_t base_reward_per_increment;   /* get_base_reward_per_increment(state) (Appendix A.9) */
} pe_state_ctx;

/* ---- lifecycle --------------------------------------------------------- */
uint32_t    pe_abi_version(void);
void        pe_config_default(pe_config* cfg);
int         pe_engine_create(const pe_config* cfg, pe_engine** out);
void        pe_engine_destroy(pe_engine* h);
const char* pe_strerror(int status);
const char* pe_last_error(const pe_engine* h);  /* detail of the last failing call on this handle */
/* Run the engine's kernels on a caller-owned HIP stream (hipStream_t as void*).
 * NULL = the engine's own stream.  Lets a host framework order its collectives
 * (RCCL) with the engine's kernels without host synchronisation. */
int         pe_set_stream(pe_engine* h, void* hip_stream);

/* ---- store: get_forkchoice_store (pe:1077-1095) ------------------------- */
/* Anchor block + state: justified = finalized = best_justified = (anchor_epoch,
 * anchor_root); time = genesis_time + SECONDS_PER_SLOT * anchor_slot; no latest
 * messages; no equivocators; no boost.  Resets any previous store contents. */
int pe_store_init(pe_engine* h, uint64_t genesis_time, uint64_t anchor_slot,
                  const uint8_t anchor_root[32]);

/* checkpoint_states[justified_checkpoint].validators (Appendix A.1): balances and
 * activity of the JUSTIFIED-checkpoint state.  pubkeys96 may be NULL (no G1 work).
 * Copies the caller's buffers.  Keeps existing votes when n is unchanged/grows. */
int pe_set_validators(pe_engine* h, uint64_t n, const uint8_t* pubkeys96,
                      const uint64_t* effective_balance, const uint8_t* flags);
/* Cheap refresh when the justified checkpoint changes: balances + flags only. */
int pe_set_balances(pe_engine* h, uint64_t n, const uint64_t* effective_balance, const uint8_t* flags);

/* on_tick (pe:934-955): time, boost reset on a new slot, best_justified promotion. */
int pe_on_tick(pe_engine* h, uint64_t time);

/* on_block (pe:986-1036) minus state_transition: the caller supplies the block's
 * root and the post-state's current_justified / finalized checkpoints. */
int pe_on_block(pe_engine* h, const uint8_t root[32], const uint8_t parent_root[32], uint64_t slot,
                uint64_t post_justified_epoch, const uint8_t post_justified_root[32],
                uint64_t post_finalized_epoch, const uint8_t post_finalized_root[32]);
/* Raw insertion (store.blocks[root] = block, pe:1016) with only the structural
 * checks (known parent, slot > parent.slot); no time/finality/boost handling.
 * For bulk loading a tree (checkpoint sync, benchmarks). */
int pe_add_block(pe_engine* h, const uint8_t root[32], const uint8_t parent_root[32], uint64_t slot,
                 uint64_t post_justified_epoch, const uint8_t post_justified_root[32],
                 uint64_t post_finalized_epoch, const uint8_t post_finalized_root[32]);

/* Direct setters for store scalars (pe:891-896); root may be the zero root. */
int pe_set_checkpoints(pe_engine* h, uint64_t justified_epoch, const uint8_t justified_root[32],
                       uint64_t finalized_epoch, const uint8_t finalized_root[32]);
int pe_set_proposer_boost(pe_engine* h, const uint8_t root[32]);
/* on_attester_slashing's effect (pe:1459-1461): equivocating_indices.add(index). */
int pe_mark_equivocating(pe_engine* h, const uint64_t* indices, uint64_t n);
/* on_attester_slashing (pe:1447-1461) on two IndexedAttestations: checks
 * is_slashable_attestation_data (pe:1134-1143) and the structural part of
 * is_valid_indexed_attestation, then marks the intersection. */
int pe_on_attester_slashing(pe_engine* h,
                            const pe_attestation* data_1, const uint64_t* indices_1, uint64_t n_1,
                            const pe_attestation* data_2, const uint64_t* indices_2, uint64_t n_2);

/* Committee table of one epoch = get_beacon_committee(state, slot, index) for every
 * (slot, index) of that epoch (Appendix A.6 / compute_committee pe:495-504), as CSR:
 * committee id = (slot % SLOTS_PER_EPOCH) * committees_per_slot + index,
 * members[offsets[id] .. offsets[id+1]).  n_committees must be a multiple of
 * SLOTS_PER_EPOCH.  The engine keeps the cfg.max_committee_tables most recently used epochs.
 * A table that partitions the registry also gets the sum of every committee's pubkeys, enqueued behind the call on the
 * stream all tables' sums share (not the shuffles') (aggregates in which a majority attests are then summed as that sum minus the absentees; POSEVO_COMMITTEE_SUMS=0: never). */
int pe_set_committees(pe_engine* h, uint64_t epoch, uint32_t n_committees,
                      const uint32_t* offsets, const uint32_t* members);

/* The same table computed ON THE GPU from the epoch's seed: compute_committee (pe:495-504) over
 * compute_shuffled_index (pe:513-534, swap-or-not, shuffle_round_count rounds of SHA-256) for every committee
 * of the epoch: committee c = [active_indices[shuffled(i)] for i in [n*c/count, n*(c+1)/count)], count =
 * n_committees.  seed = get_seed(state, epoch, DOMAIN_BEACON_ATTESTER) (pe:481-486) is the caller's (a state
 * accessor); the active set is the caller's list, or PE_ACTIVE_RESIDENT = the list pe_active_set left on the device
 * (below); active_indices NULL = validators 0 .. n_active - 1 (every validator active).  Registers
 * the table for `epoch` like pe_set_committees and KEEPS IT ON THE DEVICE; out_offsets (n_committees + 1) and
 * out_members (n_active) are optional copies of the result (NULL: nothing is read back).
 * The per-committee pubkey sums of the table (see pe_set_committees) are enqueued behind it; the call does not wait for them. */
int pe_compute_committees(pe_engine* h, uint64_t epoch, const uint8_t seed[32], const uint32_t* active_indices,
                          uint32_t n_active, uint32_t n_committees, uint32_t shuffle_round_count,
                          uint32_t* out_offsets, uint32_t* out_members);

/* The same shuffle without a wait and without a read-back, for a caller that streams epochs: the kernels go to a
 * stream of their own (beside the steps' G1 sums and fork-choice kernels; a shuffling is known one epoch ahead --
 * MIN_SEED_LOOKAHEAD, get_seed pe:481-486 -- so it is enqueued an epoch before the calls that read it), the table is
 * registered at once, and the first call that reads it makes the engine's stream wait for the shuffle.  A caller that streams with lag depth L keeps
 * max_committee_tables >= L + 3: the least recently used table is rewritten in place, and if work in flight may still
 * read it the call first completes everything in flight.
 * The table's per-committee pubkey sums are NOT enqueued with the shuffle: the first pe_aggregate over rows in device memory that
 * has the table as a candidate and finds the table complete and no shuffle in flight builds them (a caller that shuffles inside
 * every step keeps the direct sums and pays nothing).  The call sizes their buffers; the first call per table shape may wait
 * for an earlier build once while it grows them. */
int pe_compute_committees_async(pe_engine* h, uint64_t epoch, const uint8_t seed[32], const uint32_t* active_indices,
                                uint32_t n_active, uint32_t n_committees, uint32_t shuffle_round_count);

/* ---- pipelined calls: one wait per step --------------------------------- */
/* Between pe_pipeline_begin and pe_pipeline_end the batch calls (pe_aggregate, pe_on_attestation_batch,
 * pe_process_attestation_batch) validate on the host, enqueue their device work and RETURN WITHOUT WAITING:
 *   - what is host-derived is complete at return: out_atts rows, out_n_groups, group_of, every status[] entry that
 *     names a failed host-side assert;
 *   - device results (OR-ed bits, counts, aggregate pubkeys, numerators, and the status of rows whose verdict needs the
 *     bits: PE_ATT_EMPTY_OR_INVALID_INDICES / PE_ATT_BAD_SIGNATURE for overlapping members) are written into the
 *     caller's buffers when pe_pipeline_end returns -- the buffers must stay alive until then;
 *   - pe_get_head stays synchronous (it returns a root) and is ordered behind everything enqueued before it; the G1
 *     sums of a pipelined pe_aggregate run on a second stream beside the fork-choice kernels;
 *   - any other entry point first completes the pipeline's outstanding work.
 * Results are the same as with synchronous calls.  pe_pipeline_end returns the first deferred error, if any. */
int pe_pipeline_begin(pe_engine* h);
int pe_pipeline_end(pe_engine* h);
/* Lagged end, for a caller that streams step after step: returns once the pipeline L before this one is complete
 * (its buffers filled, its deferred error returned), L = the lag depth (default 2); this one completes at the L-th next
 * pe_pipeline_end_lagged, at pe_pipeline_end or at any other synchronous call.  The G1 sums of step N then run while
 * the host prepares and enqueues steps N+1 .. N+L-1.  Buffers handed to the calls of a lagged pipeline must stay alive
 * until that later completion. */
int pe_pipeline_end_lagged(pe_engine* h);
/* Lag depth of the lagged pipelines, 1 .. 7 (L + 1 sets of staging / output blocks rotate; they allocate on first use).
 * Depth 2 keeps a step's outputs two steps behind; depth 3 lets the host run far enough ahead that the device queue never
 * drains while a step's latency-bound tail (tree, normalisation) is still in flight -- what bench.py's throughput leg
 * uses.  Completes everything in flight first; not inside a pipeline (PE_ERR_STATE). */
int pe_pipeline_set_lag(pe_engine* h, uint32_t depth);
uint32_t pe_pipeline_get_lag(const pe_engine* h);
/* Which buffers may be touched: pipelines are numbered from 1 in the order of their pe_pipeline_begin(_streaming);
 * pe_pipeline_generation = the number of the one begun last, pe_pipeline_completed = the highest number whose outputs
 * are complete (they complete in order: after a pe_pipeline_end_lagged that is generation - lag or later, after
 * pe_pipeline_end or any synchronous call it is generation).  A caller that rotates its output buffers reads set g
 * when pe_pipeline_completed(h) >= g and hands it out again after that -- no need to count lagged ends itself. */
uint64_t pe_pipeline_generation(const pe_engine* h);
uint64_t pe_pipeline_completed(const pe_engine* h);
/* pe_pipeline_begin for a pipeline that will end lagged: the G1 sums of its pe_aggregate are not launched by that call
 * but by pe_pipeline_end_lagged, BEHIND the step's fork-choice kernels.  k_g1_accumulate fills every CU for its whole
 * run, so launched first it would hold pe_get_head (and with it the host's preparation of the next step) back until it
 * ends; launched last it overlaps exactly that preparation.  Results are unchanged. */
int pe_pipeline_begin_streaming(pe_engine* h);
/* Device-resident hand-over: pass PE_BITS_RESIDENT as bits_arena (arena_len ignored) to pe_on_attestation_batch /
 * pe_process_attestation_batch when `atts` are rows of out_atts of the LAST pe_aggregate on this handle (any subset,
 * any order, fields other than flags unchanged): their OR-ed bits are used where pe_aggregate left them in HBM --
 * nothing is re-packed or re-uploaded, and it works inside a pipeline where out_bits_arena is not filled yet.  Rows
 * whose members overlapped (PE_ATT_FLAG_OVERLAPPING_BITS) are rejected with PE_ATT_BAD_SIGNATURE; len(aggregation_bits)
 * must equal the committee length.  A row that is not a row of the last pe_aggregate -- e.g. one of an earlier
 * aggregate of the same pipeline, which a later one replaced -- fails the call with PE_ERR_INVALID_ARG (rows are
 * recognised by bits_offset, n_bits and a fold of their AttestationData), nothing applied. */
#define PE_BITS_RESIDENT ((const uint8_t*)(uintptr_t)1)
/* Rows resident on the device: the host off the step's critical path.
 * pe_aggregate accepts `atts` in DEVICE memory (hipMalloc of the engine's device, 16-byte aligned; the bits as above).
 * The host then reads nothing of the rows: grouping by AttestationData (pe:689-697), committee resolution
 * (get_beacon_committee's index arithmetic, Appendix A.6), validate_on_attestation (Appendix A.4, called at pe:970) and
 * the asserts of process_attestation (pe:724-730) all run on the device, and EVERY output of the call -- out_atts,
 * *out_n_groups, group_of, bits, counts, aggregate pubkeys -- is complete when a synchronous call returns / when the
 * pipeline's outputs are (nothing is host-derived any more).  Capacities are the caller's bounds: out_atts, group_of,
 * out_count, out_aggpk96 hold n entries (groups <= rows).  The handlers then take
 *     pe_on_attestation_batch(h, PE_ROWS_RESIDENT, cap, PE_BITS_RESIDENT, 0, status, NULL, out_count)
 *     pe_process_attestation_batch(h, state, PE_ROWS_RESIDENT, cap, PE_BITS_RESIDENT, 0, status, out_numerators)
 * = on_attestation / process_attestation over every group of that aggregate, in group order; cap = entries of the
 * status / count / numerator arrays (entries past the groups formed read 0; fewer entries than groups: PE_ERR_CAPACITY
 * at completion, nothing applied).  Statuses and results equal those of the host-row path.  Restrictions of this mode:
 *   - committees are resolved against the tables of the store's CURRENT and PREVIOUS epoch (the only targets
 *     validate_on_attestation admits for gossip attestations; a from-block row with an older target reads
 *     PE_ATT_NO_COMMITTEE_TABLE -- hand such rows over from host memory), and both tables must partition the registry
 *     (a real shuffling does; pe_compute_committees tables always do);
 *   - the store's clock and tables stay unchanged between pe_aggregate and its handlers (else PE_ERR_STATE);
 *   - a failing aggregate (bits outside the arena, no committee table / index out of range / len(aggregation_bits) !=
 *     len(committee) when aggregate pubkeys are asked for, output arena too small) forms NO groups: its error is returned
 *     where its outputs complete, and the handlers behind it apply nothing;
 *   - signature points (sig_points96) and the partial / sharded forms take host rows. */
#define PE_ROWS_RESIDENT ((const pe_attestation*)(uintptr_t)1)

/* ---- the hot path ------------------------------------------------------ */
/* get_head (pe:1102-1116): full recomputation from the V-entry vote table:
 * get_filtered_block_tree (Appendix A.3), get_latest_attesting_balance
 * (Appendix A.1, incl. proposer boost and equivocation mask), heaviest-child
 * descent with ties to the lexicographically higher root (pe:1114-1116). */
int pe_get_head(pe_engine* h, uint8_t out_root[32]);
/* The same computation with the root delivered like every other output of a pipeline: inside pe_pipeline_begin ...
 * _end(_lagged) the call enqueues its kernels and returns; out_root is written where the pipeline's outputs complete
 * (it must stay alive until then).  For a caller that streams steps and consumes results behind -- chain sync, replay,
 * the throughput leg of bench.py -- so that its loop never blocks on the device inside a step.  Outside a pipeline it is
 * pe_get_head. */
int pe_get_head_async(pe_engine* h, uint8_t out_root[32]);
/* get_latest_attesting_balance(store, root) for every block, in insertion order
 * (index 0 = anchor).  out must hold pe_num_blocks(h) entries. */
int pe_get_weights(pe_engine* h, uint64_t* out_weights, uint32_t n);
/* The per-block weights the LAST head computation left behind (pe_get_head, or pe_head_from_weights on a reduced
 * multi-GPU buffer), without recomputing them.  pe_prune drops them: PE_ERR_STATE until the next head computation. */
int pe_get_last_weights(pe_engine* h, uint64_t* out_weights, uint32_t n);

/* on_attestation (pe:963-979, pe:1423-1428) x n, applied AS IF sequentially in
 * array order: validate_on_attestation (Appendix A.4), committee lookup
 * (get_indexed_attestation), is_valid_indexed_attestation (structural +
 * injected signature verdict), update_latest_messages (pe:1435-1441).
 * status[i] receives a pe_att_status.  out_aggpk96 (nullable, 96*n bytes)
 * receives sum of the attesters' pubkeys = the G1 sum FastAggregateVerify
 * consumes (Appendix A.7); out_count (nullable) the number of attesters. */
int pe_on_attestation_batch(pe_engine* h, const pe_attestation* atts, uint32_t n,
                            const uint8_t* bits_arena, uint64_t arena_len,
                            int32_t* status, uint8_t* out_aggpk96, uint32_t* out_count);

/* get_indexed_attestation (Appendix A.6; call sites pe:736, pe:975) x n: attesting_indices =
 * sorted(committee[i] for i with aggregation_bits[i]), resolved against the committee table of each row's target
 * epoch exactly as pe_on_attestation_batch resolves it (no store time/root validation: this is the state-only
 * helper).  out_offsets has n + 1 entries; indices of row i are out_indices[out_offsets[i] .. out_offsets[i+1]).
 * status[i] = PE_ATT_NO_COMMITTEE_TABLE / _COMMITTEE_INDEX_OUT_OF_RANGE / _BITS_LENGTH_MISMATCH or 0.
 * out_indices must have room for the total number of set bits (<= sum of n_bits). */
int pe_get_indexed_attestations(pe_engine* h, const pe_attestation* atts, uint32_t n,
                                const uint8_t* bits_arena, uint64_t arena_len, int32_t* status,
                                uint32_t* out_offsets, uint32_t* out_indices, uint64_t out_indices_cap);

/* Aggregation (validator guide, Appendix A.8; reference prose pe:474/659/715/1536):
 * attestations with identical AttestationData and n_bits form one group (groups
 * ordered by first appearance).  Per group: aggregation_bits = OR of the members'
 * bits; signature = sum of the members' signature points (sig_points96, 96 B per
 * input attestation, nullable); aggregate pubkey = sum of pubkey[committee[i]]
 * over the OR-ed bits (needs the committee table of every target epoch in the batch;
 * NULL out to skip).  A batch may span target epochs (an epoch boundary); only the
 * partial / sharded forms below want one target epoch per call.
 *   out_atts[g]   : the group's data, bits_offset into out_bits_arena
 *   group_of[i]   : group index of input attestation i (nullable)
 * Capacities: out_atts has room for n rows, out_bits_arena for out_arena_cap bytes.
 * bits_arena may lie in pageable host memory (copied during the call), in pinned host memory or in device memory
 * (hipMalloc of the engine's device): the latter two are picked up by the copy engine without a pass on the host, and
 * must stay unchanged until the call's outputs are complete (inside a pipeline: until the pipeline's are).  The same
 * holds for pe_aggregate_partial and pe_aggregate_sharded.  The attestation rows are host memory, or -- pe_aggregate
 * only -- device memory: see PE_ROWS_RESIDENT above. */
int pe_aggregate(pe_engine* h, const pe_attestation* atts, uint32_t n,
                 const uint8_t* bits_arena, uint64_t arena_len, const uint8_t* sig_points96,
                 pe_attestation* out_atts, uint32_t* out_n_groups, uint32_t* group_of,
                 uint8_t* out_bits_arena, uint64_t out_arena_cap,
                 uint8_t* out_sig96, uint8_t* out_aggpk96, uint32_t* out_count);

/* process_attestation (pe:722-754) x n, as if sequentially in array order, on the
 * engine's working participation arrays: asserts pe:724-730, participation flag
 * indices (Appendix A.9), flag RMW pe:745-749, and per attestation the
 * proposer_reward_numerator (pe:744-749).  The caller finishes pe:752-754
 * (numerator // denominator, increase_balance). */
int pe_process_attestation_batch(pe_engine* h, const pe_state_ctx* state,
                                 const pe_attestation* atts, uint32_t n,
                                 const uint8_t* bits_arena, uint64_t arena_len,
                                 int32_t* status, uint64_t* out_numerators);
/* state.{current,previous}_epoch_participation of the working state (pe:739-742).
 * which: 0 = current, 1 = previous. */
int pe_participation_set(pe_engine* h, int which, const uint8_t* flags, uint64_t n);
int pe_participation_get(pe_engine* h, int which, uint8_t* out_flags, uint64_t n);
/* process_participation_flag_updates at an epoch boundary: previous = current, current = 0. */
int pe_participation_rotate(pe_engine* h);

/* The working BeaconState's registry view (the state process_attestation / FFG run on), when it differs from the
 * justified-checkpoint state given to pe_set_validators: effective balances (get_base_reward, pe:749; FFG sums)
 * and flags PE_VAL_ACTIVE (active in get_current_epoch(state)), PE_VAL_SLASHED, PE_VAL_ACTIVE_PREV (active in
 * get_previous_epoch(state)).  Until this is called the engine uses the pe_set_validators data for both. */
#define PE_VAL_ACTIVE_PREV 0x08u
int pe_state_set_validators(pe_engine* h, uint64_t n, const uint64_t* effective_balance, const uint8_t* flags);
/* Read-backs for checkpoint / resume (pe_store_init drops committee tables, the working-state view and participation
 * with the store; a restart hands them back).  *out_is_set = 0: the view still mirrors pe_set_validators. */
int pe_state_get_validators(pe_engine* h, uint64_t n, uint64_t* out_effective_balance, uint8_t* out_flags, int* out_is_set);
/* Epochs of the committee tables held (out_epochs NULL: count only), and one table: out_offsets u32[n_committees + 1],
 * out_members u32[offsets[n_committees]] (either may be NULL; *out_n_committees is always written). */
int pe_get_committee_epochs(pe_engine* h, uint64_t* out_epochs, uint32_t cap, uint32_t* out_n);
int pe_get_committees(pe_engine* h, uint64_t epoch, uint32_t* out_n_committees, uint32_t* out_offsets,
                      uint32_t offsets_cap, uint32_t* out_members, uint64_t members_cap);
/* The balance sums of process_justification_and_finalization (pe:791-802) over the working state and the engine's
 * participation arrays: out[0] = get_total_active_balance(state), out[1] = previous_target_balance,
 * out[2] = current_target_balance (each max(EFFECTIVE_BALANCE_INCREMENT, sum), Appendix A.1).  The caller feeds
 * them to weigh_justification_and_finalization (pe:815-853), which is scalar logic on the state. */
int pe_ffg_balances(pe_engine* h, uint64_t out[3]);

/* ---- the epoch boundary over the resident registry ----------------------- */
/* compute_proposer_index (pe:604-618), once per seed: for i = 0, 1, ... the candidate
 * indices[compute_shuffled_index(i % total, total, seed)] is accepted iff
 * effective_balance * 255 >= max_effective_balance * hash(seed + uint64_le(i / 32))[i % 32].
 * effective balances = the working-state view (pe_state_set_validators; the pe_set_validators data until then).
 * seeds: n_seeds x 32 bytes (the caller's state accessor, e.g. one per slot of an epoch).
 * active_indices / n_active / shuffle_round_count: exactly as pe_compute_committees (NULL = validators 0..n_active-1;
 * same validation, same bound on the round count, PE_ACTIVE_RESIDENT accepted); an empty active set is
 * PE_ERR_INVALID_ARG (pe:608).
 * max_tries: candidates examined per seed before giving up (0 = 4096).
 * out_proposers u32[n_seeds]: the validator index, or 0xFFFFFFFF where no candidate within max_tries was accepted
 *   (the reference loops forever there).
 * out_tries u32[n_seeds] (may be NULL): the i at which the candidate was accepted; max_tries when none was.
 * Synchronous; one GPU: PE_ERR_STATE on a handle with pe_dist_init* active. */
int pe_compute_proposers(pe_engine* h, const uint8_t* seeds32, uint32_t n_seeds,
                         const uint32_t* active_indices, uint32_t n_active, uint32_t shuffle_round_count,
                         uint64_t max_effective_balance, uint32_t max_tries,
                         uint32_t* out_proposers, uint32_t* out_tries);

/* process_effective_balance_updates (pe:122-133) on the working-state view, in place:
 * balances u64[n] = state.balances (host memory, or PE_BALANCES_RESIDENT); increment = cfg.effective_balance_increment;
 * thresholds = increment / hysteresis_quotient * {downward, upward}_multiplier.
 * If the view still mirrors pe_set_validators, it is first materialised from it, flags included.
 * The justified-checkpoint data that get_head weighs is NOT changed.
 * Updates d_sbalance and the u16 increments the flag passes read.
 * *out_n_changed = validators whose effective balance changed.
 * out_effective_balance (may be NULL): the new values.
 * n != registry size, or max_effective_balance / increment > 65535: PE_ERR_INVALID_ARG, nothing changed.
 * Synchronous; one GPU: PE_ERR_STATE on a handle with pe_dist_init* active. */
int pe_effective_balance_updates(pe_engine* h, uint64_t n, const uint64_t* balances,
                                 uint64_t max_effective_balance, uint64_t hysteresis_quotient,
                                 uint64_t downward_multiplier, uint64_t upward_multiplier,
                                 uint64_t* out_n_changed, uint64_t* out_effective_balance);

/* ---- the active validator set over the resident registry ------------------ */
/* Validator.activation_epoch / exit_epoch (pe:43-44) of the whole registry, copied into device memory (16 B per
 * validator).  n must equal pe_num_validators(h): else PE_ERR_INVALID_ARG and nothing changes.  FAR_FUTURE_EPOCH is
 * 2^64 - 1; every comparison the engine makes on these values is unsigned 64-bit.  The arrays are dropped where the
 * working-state view is: pe_store_init, and a pe_set_validators that changes n.  Setting them drops the resident
 * active list (it was compacted from the previous values).  *out_is_set = 0: none held, the outputs are not written.
 * Checkpoint / resume: read them with _get, hand them back with _set. */
int pe_registry_set_epochs(pe_engine* h, uint64_t n, const uint64_t* activation_epoch, const uint64_t* exit_epoch);
int pe_registry_get_epochs(pe_engine* h, uint64_t n, uint64_t* out_activation_epoch, uint64_t* out_exit_epoch,
                           int* out_is_set);

/* get_active_validator_indices(state, epoch): every v with activation_epoch[v] <= epoch < exit_epoch[v]
 * (is_active_validator), in increasing order of v -- the order the shuffle reads (pe:495-504).  One ordered compaction
 * over the resident epochs; the list STAYS ON THE DEVICE as the handle's resident active list, with its epoch and length.
 * *out_n_active = len(list): what get_committee_count_per_slot (pe:461-468), compute_weak_subjectivity_period
 *   (pe:1267) and get_latest_weak_subjectivity_checkpoint_epoch (pe:1234) ask for.
 * *out_total_balance = max(EFFECTIVE_BALANCE_INCREMENT, sum of effective_balance over the list): get_total_active_balance
 *   (pe:1268) for `epoch`; effective balances = the working-state view (pe_state_set_validators; the pe_set_validators
 *   data until then).  The same quantity and rule as pe_ffg_balances out[0]; slashed validators count, as there.
 * out_indices (may be NULL; capacity pe_num_validators(h)): a copy of the list, *out_n_active entries.
 * Without epochs (pe_registry_set_epochs): PE_ERR_STATE.  One resident list per handle: the next call replaces it.
 * Synchronous (completes open pipelines first); one GPU: PE_ERR_STATE on a handle with pe_dist_init* active. */
int pe_active_set(pe_engine* h, uint64_t epoch, uint32_t* out_n_active, uint64_t* out_total_balance,
                  uint32_t* out_indices);

/* As `active_indices` of pe_compute_committees, pe_compute_committees_async and pe_compute_proposers: the resident
 * list, read by the kernels where pe_active_set left it -- no host validation (increasing and in range by
 * construction), no copy, no upload.  n_active must equal the resident length (else PE_ERR_INVALID_ARG); without a
 * resident list the calls return PE_ERR_STATE.  The list is dropped with the epochs, and by pe_registry_set_epochs.
 * pe_compute_committees_async reads the list on the shuffle's own stream, behind the call's return: it records an
 * event there, and the next pe_active_set makes the engine's stream wait for that event before its kernels rewrite
 * the list (ordered on the device, no host wait; one buffer, not two). */
#define PE_ACTIVE_RESIDENT ((const uint32_t*)(uintptr_t)1)

/* PE_VAL_ACTIVE / PE_VAL_ACTIVE_PREV of the working-state view from the resident epochs: PE_VAL_ACTIVE = activity at
 * current_epoch, PE_VAL_ACTIVE_PREV = activity at max(current_epoch, 1) - 1 (get_previous_epoch's clamp at
 * GENESIS_EPOCH).  PE_VAL_SLASHED and every other bit are kept.  If the view still mirrors pe_set_validators, it is
 * first materialised from it exactly as pe_effective_balance_updates does.  The justified-checkpoint flags get_head
 * weighs (pe_get_validator_flags) are NOT changed.  Without epochs: PE_ERR_STATE.  Synchronous; one GPU. */
int pe_state_refresh_activity(pe_engine* h, uint64_t current_epoch);

/* ---- rewards and penalties over resident balances -------------------------- */
/* state.balances, state.inactivity_scores and Validator.withdrawable_epoch of the whole registry, copied into device
 * memory (three u64[n] arrays, 24 B per validator).  inactivity_scores NULL = zeros; withdrawable_epoch NULL =
 * FAR_FUTURE_EPOCH (2^64 - 1) everywhere.  n must equal pe_num_validators(h): else PE_ERR_INVALID_ARG and nothing
 * changes.  The arrays are dropped where the working-state view is: pe_store_init, and a pe_set_validators that changes n.
 * _get: any output may be NULL; *out_is_set = 0: none held, the arrays are not written.  Checkpoint / resume goes through
 * this pair (read with _get, hand back with _set), as with pe_registry_get_epochs. */
int pe_state_set_balances(pe_engine* h, uint64_t n, const uint64_t* balances, const uint64_t* inactivity_scores,
                          const uint64_t* withdrawable_epoch);
int pe_state_get_balances(pe_engine* h, uint64_t n, uint64_t* out_balances, uint64_t* out_inactivity_scores,
                          uint64_t* out_withdrawable_epoch, int* out_is_set);

/* The constants process_inactivity_updates and process_rewards_and_penalties read beside cfg.effective_balance_increment.
 * The participation flag weights (14, 26, 14) and WEIGHT_DENOMINATOR (64) are the ones process_attestation's flag passes
 * use (Appendix A.9) and are not parameters. */
typedef struct pe_rewards_params {
    uint64_t base_reward_factor;                /* BASE_REWARD_FACTOR */
    uint64_t inactivity_score_bias;             /* INACTIVITY_SCORE_BIAS */
    uint64_t inactivity_score_recovery_rate;    /* INACTIVITY_SCORE_RECOVERY_RATE */
    uint64_t inactivity_penalty_quotient;       /* INACTIVITY_PENALTY_QUOTIENT_* of the fork in force */
    uint64_t min_epochs_to_inactivity_penalty;  /* MIN_EPOCHS_TO_INACTIVITY_PENALTY */
} pe_rewards_params;
/* 64, 4, 16, 2^24, 4.  The quotient is INACTIVITY_PENALTY_QUOTIENT_BELLATRIX (2^24), the value every fork since
 * Bellatrix keeps; Altair's own was 3 * 2^24 -- set it for an Altair state. */
void pe_rewards_params_default(pe_rewards_params* out);

#define PE_REWARDS_INACTIVITY 1u  /* process_inactivity_updates: the scores */
#define PE_REWARDS_DELTAS     2u  /* process_rewards_and_penalties: the four (rewards, penalties) pairs onto the balances */
typedef struct pe_rewards_stats {
    uint64_t total_active_balance;    /* get_total_active_balance: the quantity and rule of pe_ffg_balances out[0] */
    uint64_t unslashed_balance[3];    /* get_total_balance(get_unslashed_participating_indices(f, previous_epoch)), f = 0, 1, 2 */
    uint64_t n_eligible;              /* len(get_eligible_validator_indices) */
    uint64_t in_leak;                 /* is_in_inactivity_leak: 0 or 1 */
    uint64_t rewards;                 /* Gwei credited, all pairs */
    uint64_t penalties;               /* Gwei actually debited, all pairs (after decrease_balance's cut at 0) */
    uint64_t n_saturated;             /* validators where at least one subtraction was cut at 0 */
} pe_rewards_stats;

/* process_inactivity_updates (which & PE_REWARDS_INACTIVITY) and process_rewards_and_penalties (which &
 * PE_REWARDS_DELTAS) of Altair over the resident arrays, in place; given both, the scores move first, as in
 * process_epoch.  The rule set is restated in tests/rewards_model.py (the reference holds the fields and the callers of
 * these functions, not their text).  Reads the working-state view (effective balances; PE_VAL_ACTIVE for the total,
 * PE_VAL_ACTIVE_PREV and PE_VAL_SLASHED for eligibility and the unslashed sets: set them, or pe_state_refresh_activity
 * does) and previous_epoch_participation; previous_epoch = max(current_epoch, 1) - 1.  If the view still mirrors
 * pe_set_validators it is first materialised, as pe_effective_balance_updates does.
 * in_leak = previous_epoch - finalized_epoch > min_epochs_to_inactivity_penalty.
 * current_epoch == 0 (GENESIS_EPOCH): nothing is launched, *out_stats = 0.
 * Two streaming kernels with a host step between them (k_reward_sums, k_reward_apply).  Synchronous (completes open
 * pipelines first; ordered against the flag passes as pe_ffg_balances is); one GPU.  out_stats may be NULL.
 * A failing call changes nothing:
 *   PE_ERR_STATE        no resident balances (pe_state_set_balances), or pe_dist_init* active
 *   PE_ERR_INVALID_ARG  which is 0 or has other bits; bias * quotient is 0 or exceeds 64 bits; finalized_epoch >
 *                       previous_epoch; or the reference's uint64 would overflow -- decided on the host in 128 bits from
 *                       what the first kernel reads back, before the second is launched: INCREMENT * base_reward_factor;
 *                       total_active_balance / INCREMENT * 64; (largest effective balance among eligible validators /
 *                       INCREMENT) * per_increment * 26 * (largest of the three unslashed balances / INCREMENT; 1 in a
 *                       leak); largest effective balance * (largest score among eligible validators + bias, the bias
 *                       only with PE_REWARDS_INACTIVITY).  The bounds are conservative: they pair maxima that need not
 *                       meet in one validator.  balance + reward itself is not checked (it needs a balance above
 *                       2^63 Gwei) and wraps. */
int pe_rewards_and_penalties(pe_engine* h, uint64_t current_epoch, uint64_t finalized_epoch,
                             const pe_rewards_params* params, uint32_t which, pe_rewards_stats* out_stats);

/* As `balances` of pe_effective_balance_updates: the resident vector, read by the kernel where pe_state_set_balances /
 * pe_rewards_and_penalties left it -- no staging, no upload.  n must equal the registry size; without resident balances
 * the call returns PE_ERR_STATE.  Every other argument and result of that call is as without it. */
#define PE_BALANCES_RESIDENT ((const uint64_t*)(uintptr_t)1)

/* ---- registry updates and slashings over the resident registry -------------- */
/* The constants process_registry_updates reads. */
typedef struct pe_registry_params {
    uint64_t max_effective_balance;                 /* MAX_EFFECTIVE_BALANCE */
    uint64_t ejection_balance;                      /* EJECTION_BALANCE */
    uint64_t max_seed_lookahead;                    /* MAX_SEED_LOOKAHEAD */
    uint64_t min_validator_withdrawability_delay;   /* MIN_VALIDATOR_WITHDRAWABILITY_DELAY */
    uint64_t min_per_epoch_churn_limit;             /* MIN_PER_EPOCH_CHURN_LIMIT */
    uint64_t churn_limit_quotient;                  /* CHURN_LIMIT_QUOTIENT */
    uint64_t max_per_epoch_activation_churn_limit;  /* MAX_PER_EPOCH_ACTIVATION_CHURN_LIMIT; 0 = none (pre-Deneb); Deneb: 8 */
} pe_registry_params;
/* 32e9, 16e9, 4, 256, 4, 65536, 0 */
void pe_registry_params_default(pe_registry_params* out);

typedef struct pe_registry_stats {
    uint64_t n_active;                /* len(get_active_validator_indices(state, current_epoch)) */
    uint64_t churn_limit;             /* get_validator_churn_limit: max(min_per_epoch_churn_limit, n_active / quotient) */
    uint64_t activation_churn_limit;  /* min(max_per_epoch_activation_churn_limit, churn_limit); the cap 0 = none */
    uint64_t n_marked_eligible;       /* validators whose activation_eligibility_epoch became current_epoch + 1 */
    uint64_t n_ejected;               /* validators whose exit was initiated (it was FAR_FUTURE_EPOCH before) */
    uint64_t first_exit_epoch;        /* the exit epoch of the first of them in index order; 0 when n_ejected == 0 */
    uint64_t last_exit_epoch;         /* ... of the last; 0 when n_ejected == 0 */
    uint64_t queue_len;               /* the activation queue */
    uint64_t n_activated;             /* min(activation_churn_limit, queue_len) */
    uint64_t activation_epoch;        /* current_epoch + 1 + max_seed_lookahead: what they were given */
} pe_registry_stats;

/* process_registry_updates over the resident arrays, in place (the rule set is restated in
 * tests/registry_updates_model.py: the reference holds the fields, pe:36-45, and names get_validator_churn_limit,
 * pe:1261/1270, not the function's text).  For every validator, comparisons unsigned 64-bit, FAR = 2^64 - 1:
 *   mark    activation_eligibility_epoch == FAR and effective_balance == max_effective_balance:
 *           activation_eligibility_epoch = current_epoch + 1
 *   eject   active at current_epoch, effective_balance <= ejection_balance and exit_epoch == FAR: initiate_validator_exit.
 *           With E0 = max(largest exit epoch set, current_epoch + 1 + max_seed_lookahead), c0 = validators whose exit
 *           epoch is E0 and (base, fill) = (E0 + 1, 0) if c0 >= churn_limit else (E0, c0), the k-th such validator in
 *           index order gets exit_epoch = base + (fill + k) / churn_limit -- the sequential loop's closed form -- and
 *           withdrawable_epoch = exit_epoch + min_validator_withdrawability_delay
 *   queue   activation_eligibility_epoch <= finalized_epoch and activation_epoch == FAR, as read before the marks of this
 *           call (a validator marked now has current_epoch + 1 > finalized_epoch): the first activation_churn_limit by
 *           (activation_eligibility_epoch, index) get activation_epoch = current_epoch + 1 + max_seed_lookahead
 * Reads the working-state view's effective balances as they are (the view is not materialised), the resident epochs
 * (pe_registry_set_epochs), withdrawable epochs (pe_state_set_balances) and eligibility epochs (pe_registry_set_static).
 * PE_VAL_ACTIVE / PE_VAL_ACTIVE_PREV are not touched: pe_state_refresh_activity stays the caller's step.  If an
 * activation or exit epoch was written the resident active list is dropped, as pe_registry_set_epochs drops it; else it
 * is kept.  pe_registry_get_epochs, pe_state_get_balances and pe_registry_get_static read the new values back and
 * pe_state_roots hashes them with no further call.
 * Read-only passes (k_registry_census, k_registry_select, k_registry_ties), a host step, one writing pass
 * (k_registry_apply).  Synchronous (completes open pipelines first); one GPU.  out may be NULL.
 * A failing call changes nothing:
 *   PE_ERR_STATE        the epochs, the balances or the static part are not resident, or pe_dist_init* active
 *   PE_ERR_INVALID_ARG  churn_limit_quotient == 0; current_epoch + 1 + max_seed_lookahead wraps or reaches FAR; the last
 *                       exit epoch + min_validator_withdrawability_delay wraps or reaches FAR (decided on the host in 128
 *                       bits before anything is written) */
int pe_registry_updates(pe_engine* h, uint64_t current_epoch, uint64_t finalized_epoch, const pe_registry_params* params,
                        pe_registry_stats* out);

typedef struct pe_slashings_stats {
    uint64_t total_active_balance;             /* get_total_active_balance: the quantity and rule of pe_ffg_balances out[0] */
    uint64_t adjusted_total_slashing_balance;  /* min(sum_slashings * multiplier, total_active_balance) */
    uint64_t n_penalised;                      /* slashed validators whose withdrawable epoch is the target */
    uint64_t penalties;                        /* Gwei actually debited (after decrease_balance's cut at 0) */
    uint64_t n_saturated;                      /* validators whose penalty exceeded the balance */
} pe_slashings_stats;

/* process_slashings over the resident balances, in place: every validator with PE_VAL_SLASHED in the working-state view
 * and withdrawable_epoch == current_epoch + epochs_per_slashings_vector / 2 loses
 * effective_balance / INCREMENT * adjusted / total * INCREMENT, cut at its balance.  total = get_total_active_balance over
 * the view's PE_VAL_ACTIVE (k_ffg_balances' sum); sum_slashings = sum(state.slashings), the caller's scalar -- the vector
 * and its reset stay with the caller.  Writes the resident balances alone; the view is read as it is.
 * Synchronous (completes open pipelines first); one GPU.  out may be NULL.  A failing call changes nothing:
 *   PE_ERR_STATE        no resident balances (pe_state_set_balances), or pe_dist_init* active
 *   PE_ERR_INVALID_ARG  sum_slashings * multiplier exceeds 64 bits; current_epoch + epochs_per_slashings_vector / 2 wraps;
 *                       (the largest effective balance of a penalised validator / INCREMENT) * adjusted exceeds 64 bits */
int pe_process_slashings(pe_engine* h, uint64_t current_epoch, uint64_t sum_slashings,
                         uint64_t proportional_slashing_multiplier, uint64_t epochs_per_slashings_vector,
                         pe_slashings_stats* out);

/* ---- block operations over the resident registry: slashings and exits -------- */
/* process_proposer_slashing, process_attester_slashing and process_voluntary_exit, with slash_validator and
 * initiate_validator_exit under them (Altair / Bellatrix; the rule set is restated in tests/block_ops_model.py: the reference
 * holds the Validator fields, pe:36-45, `slashings`, pe:359/397, and is_slashable_attestation_data, pe:1134-1143, not these
 * functions' text).  With process_attestation (pe_process_attestation_batch) and process_deposit (pe_process_deposits) this
 * completes Altair's process_operations over resident state. */
#define PE_OP_PROPOSER_SLASHING 1u
#define PE_OP_ATTESTER_SLASHING 2u
#define PE_OP_VOLUNTARY_EXIT    3u
#define PE_OP_FLAG_SIGNATURE_VALID 0x1u /* the injected verdict over every signature of the operation (both headers, both
                                           IndexedAttestations, the SignedVoluntaryExit): the caller computes it with the BLS
                                           calls, as PE_ATT_FLAG_SIGNATURE_VALID */
typedef struct pe_block_op {
    uint32_t kind;                  /* PE_OP_* */
    uint32_t flags;                 /* PE_OP_FLAG_* */
    /* PE_OP_ATTESTER_SLASHING: the two AttestationData = the leading 128 bytes of a pe_attestation (as
     * pe_on_attester_slashing and pe_slasher_get_data use them) and attesting_indices of both sides as ranges of `indices` */
    uint8_t  data_1[128], data_2[128];
    uint64_t indices_1_offset, indices_1_length, indices_2_offset, indices_2_length;
    /* PE_OP_PROPOSER_SLASHING: of the two BeaconBlockHeaders the slot, the proposer index and hash_tree_root(header) */
    uint64_t header_1_slot, header_1_proposer_index;
    uint8_t  header_1_root[32];
    uint64_t header_2_slot, header_2_proposer_index;
    uint8_t  header_2_root[32];
    /* PE_OP_VOLUNTARY_EXIT */
    uint64_t validator_index, exit_epoch;
} pe_block_op;                      /* 408 bytes */

/* status[i] of pe_process_block_operations: 0 = valid, else the first assert of the operation that fails, in its order */
typedef enum pe_op_status {
    PE_OP_OK = 0,
    PE_OP_NOT_SLASHABLE_DATA = 64,      /* attester: is_slashable_attestation_data false */
    PE_OP_BAD_INDICES = 65,             /* attester: a list empty, not strictly ascending or with an index >= n; proposer /
                                           exit: the validator index >= n */
    PE_OP_BAD_SIGNATURE = 66,           /* the injected verdict is false */
    PE_OP_NOBODY_SLASHABLE = 67,        /* attester: no validator of the intersection was slashable when visited */
    PE_OP_HEADER_MISMATCH = 68,         /* proposer: slots or proposer indices differ, or the two roots are equal */
    PE_OP_PROPOSER_NOT_SLASHABLE = 69,  /* proposer: is_slashable_validator false */
    PE_OP_NOT_ACTIVE = 70,              /* exit: not active at current_epoch */
    PE_OP_ALREADY_EXITING = 71,         /* exit: exit_epoch != FAR (before the call, or by an earlier operation of it) */
    PE_OP_EXIT_EPOCH_FUTURE = 72,       /* exit: current_epoch < exit.epoch */
    PE_OP_TOO_YOUNG = 73                /* exit: current_epoch < activation_epoch + shard_committee_period */
} pe_op_status;

typedef struct pe_block_ops_params {
    uint64_t min_slashing_penalty_quotient;       /* 32: MIN_SLASHING_PENALTY_QUOTIENT_BELLATRIX (Altair's own is 64) */
    uint64_t whistleblower_reward_quotient;       /* 512 */
    uint64_t epochs_per_slashings_vector;         /* 8192 */
    uint64_t shard_committee_period;              /* 256 */
    uint64_t min_validator_withdrawability_delay; /* 256  -- these four as pe_registry_params */
    uint64_t max_seed_lookahead;                  /* 4 */
    uint64_t min_per_epoch_churn_limit;           /* 4 */
    uint64_t churn_limit_quotient;                /* 65536 */
} pe_block_ops_params;
void pe_block_ops_params_default(pe_block_ops_params* out);

typedef struct pe_block_ops_stats {
    uint64_t n_active;           /* active at current_epoch, before the call */
    uint64_t churn_limit;        /* get_validator_churn_limit: constant during the call, every exit it writes lies after
                                    current_epoch */
    uint64_t n_slashed;
    uint64_t n_exits_initiated;  /* exit epochs written: voluntary exits and slashed validators without one */
    uint64_t first_exit_epoch, last_exit_epoch;  /* 0 if none was written */
    uint64_t slashed_balance;    /* the effective balances slashed: the caller adds it to
                                    state.slashings[current_epoch % EPOCHS_PER_SLASHINGS_VECTOR] (the vector stays the
                                    caller's scalar state, as for pe_process_slashings) */
    uint64_t proposer_rewards;   /* Gwei credited to proposer_index */
    uint64_t penalties;          /* Gwei actually debited (after decrease_balance's cut at 0) */
    uint64_t n_saturated;        /* slashed validators whose penalty exceeded the balance */
    uint64_t n_invalid;          /* operations with a status != 0 */
} pe_block_ops_stats;

/* An ordered list of block operations applied to the resident registry with the semantics of the sequential pyspec loop:
 * operations take effect in array order and each sees the effects of the earlier ones (a validator slashed by one is not
 * slashable in the next; a validator already exiting is slashed without a new exit epoch; an exit after a slashing of the
 * same validator is invalid).  Comparisons unsigned 64-bit, FAR = 2^64 - 1 an ordinary value:
 *   initiate_validator_exit(i)   nothing if exit_epoch[i] != FAR; else with E0, c0, (base, fill) as for pe_registry_updates the
 *                                k-th such validator IN OPERATION ORDER gets exit_epoch = base + (fill + k) / churn_limit and
 *                                withdrawable_epoch = exit_epoch + min_validator_withdrawability_delay
 *   slash_validator(i)           whistleblower = the proposer: initiate_validator_exit(i); PE_VAL_SLASHED in the working-state
 *                                view; withdrawable_epoch = max(withdrawable_epoch, current_epoch + epochs_per_slashings_vector);
 *                                balance[i] -= min(balance[i], effective_balance[i] / min_slashing_penalty_quotient);
 *                                balance[proposer_index] += effective_balance[i] / whistleblower_reward_quotient
 *   is_slashable_validator(i)    not slashed, activation_epoch <= current_epoch < withdrawable_epoch
 *   attester slashing            valid iff the data are slashable, both lists are non-empty, strictly ascending and < n, the
 *                                verdict is true and at least one validator of the intersection, visited in ascending order, is
 *                                slashable when visited; every such validator is slashed
 *   proposer slashing            valid iff slots and proposer indices are equal, the roots differ, the proposer is slashable
 *                                and the verdict is true
 *   voluntary exit               valid iff active at current_epoch, exit_epoch == FAR, current_epoch >= exit.epoch,
 *                                current_epoch >= activation_epoch + shard_committee_period and the verdict is true
 * A BLOCK WITH AN INVALID OPERATION IS AN INVALID BLOCK: the call writes every operation's status and, if any is not 0,
 * CHANGES NOTHING (it still returns PE_OK; out->n_invalid counts them, out->n_active and churn_limit are filled, the rest is
 * 0).  The statuses behind the first invalid operation are those the operations get on the state the earlier VALID
 * operations leave; an invalid operation itself leaves nothing.
 * indices: the attester slashings' attesting_indices, flat; the ranges may overlap or coincide.  The proposer's balance is
 * the only one several slashings touch: it takes the closed form of the loop -- where the proposer is itself the j-th
 * slashing of the call its penalty is cut against balance + the rewards of the slashings before it, and the other rewards,
 * its own slashing's included, arrive afterwards.
 * Reads and writes the resident epochs (pe_registry_set_epochs), balances and withdrawable epochs (pe_state_set_balances)
 * and the working-state view (materialised first if it still mirrors pe_set_validators).  PE_VAL_ACTIVE / _PREV are not
 * touched.  If an exit epoch was written the resident active list is dropped, as pe_registry_updates drops it.
 * pe_registry_get_epochs, pe_state_get_balances and pe_state_get_validators read the new values back and pe_state_roots
 * hashes them with no further call.  Read-only passes (k_block_ops_lists, _claim, _resolve, _scan, k_registry_census), a host
 * step, one writing pass (k_block_ops_apply: one writer per validator and column, no atomic on a balance).
 * Synchronous (completes open pipelines first); one GPU.  status: n_ops entries; out may be NULL.  A block's operations
 * run slashings, attestations, deposits, exits: two calls around the other two.  A failing call changes
 * nothing:
 *   PE_ERR_STATE        the epochs or the balances are not resident, the view does not cover the registry, or pe_dist_init*
 *   PE_ERR_INVALID_ARG  an unknown kind; an offset or length past n_indices; proposer_index >= n; a quotient is 0;
 *                       current_epoch + epochs_per_slashings_vector or current_epoch + 1 + max_seed_lookahead wraps or reaches
 *                       FAR; the churn limit is 0; the last exit epoch + min_validator_withdrawability_delay wraps or reaches
 *                       FAR; n_slashed * (the largest slashed effective balance) + balance[proposer_index] exceeds 64 bits
 *                       (the bound under which no sum of the call can wrap) -- the last three decided on the host, in 128
 *                       bits, before anything is written
 *   PE_ERR_CAPACITY     2^31 or more indices, or candidate slots (list elements + single operations) */
int pe_process_block_operations(pe_engine* h, uint64_t current_epoch, uint32_t proposer_index,
                                const pe_block_op* ops, uint32_t n_ops,
                                const uint32_t* indices, uint64_t n_indices,
                                const pe_block_ops_params* params,
                                int32_t* status, pe_block_ops_stats* out);

/* ---- Capella: withdrawals and BLS-to-execution changes over the resident registry -------- */
/* process_withdrawals (with get_expected_withdrawals, is_fully_withdrawable_validator, is_partially_withdrawable_validator and
 * has_eth1_withdrawal_credential under it) and process_bls_to_execution_change (Capella; the rule set is restated in
 * tests/withdrawals_model.py: the reference holds the Validator fields, pe:36-45, and `balances`, pe:112, not these
 * functions' text). */
#pragma pack(push, 1)
typedef struct pe_withdrawal {      /* Withdrawal as it travels: 44 bytes, no padding */
    uint64_t index;
    uint64_t validator_index;
    uint8_t  address[20];
    uint64_t amount;
} pe_withdrawal;
#pragma pack(pop)

typedef struct pe_withdrawals_params {
    uint64_t max_effective_balance;        /* 32 * 10^9 */
    uint64_t max_withdrawals_per_payload;  /* 16 (minimal preset: 4); at most 64 */
    uint64_t max_validators_per_sweep;     /* 16384 (minimal preset: 16); may exceed the registry */
    uint64_t eth1_prefix;                  /* 0x01: ETH1_ADDRESS_WITHDRAWAL_PREFIX, one byte */
} pe_withdrawals_params;
void pe_withdrawals_params_default(pe_withdrawals_params* out);

#define PE_WD_APPLY   0x1u  /* debit the balances: process_withdrawals.  Needs PE_WD_PAYLOAD.  Without it the call only computes:
                               get_expected_withdrawals, what a proposer building a payload needs */
#define PE_WD_PAYLOAD 0x2u  /* payload / n_payload are the execution payload's withdrawals (n_payload may be 0) */

/* pe_withdrawals_result.status: 0, or process_withdrawals' first failing assert over the payload */
typedef enum pe_wd_status {
    PE_WD_OK = 0,
    PE_WD_COUNT_MISMATCH = 80,      /* len(payload.withdrawals) != len(expected_withdrawals) */
    PE_WD_INDEX_MISMATCH = 81,      /* the first differing entry differs in its index, ... */
    PE_WD_VALIDATOR_MISMATCH = 82,  /* ... else in its validator_index, ... */
    PE_WD_ADDRESS_MISMATCH = 83,    /* ... else in its address, ... */
    PE_WD_AMOUNT_MISMATCH = 84      /* ... else in its amount */
} pe_wd_status;

typedef struct pe_withdrawals_result {
    uint64_t next_withdrawal_index;            /* behind the last expected withdrawal; unchanged if there is none */
    uint64_t next_withdrawal_validator_index;  /* (the last withdrawal's validator + 1) mod n where the list is full, else
                                                  (start + max_validators_per_sweep) mod n -- the parameter, not the bound */
    uint64_t n_full, n_partial;                /* expected withdrawals of either kind */
    uint64_t total_gwei;                       /* their amounts, cut at 2^64 - 1 */
    uint32_t n_withdrawals;                    /* entries written to out_withdrawals */
    int32_t  status;                           /* pe_wd_status */
    uint32_t first_mismatch;                   /* status != 0: the first differing entry (the shorter length where the
                                                  lengths differ) */
    uint32_t applied;                          /* 1: the balances were debited */
    uint8_t  withdrawals_root[32];             /* hash_tree_root(List[Withdrawal, max_withdrawals_per_payload]) of the
                                                  expected list */
} pe_withdrawals_result;

/* The withdrawal sweep over the resident registry, exactly the sequential loop: bound = min(n, max_validators_per_sweep)
 * positions, position j visits validator (next_withdrawal_validator_index + j) mod n.  A visited validator yields
 *   a full withdrawal of balance                           if credentials[0] == eth1_prefix, withdrawable_epoch <=
 *                                                          current_epoch and balance > 0;
 *   else a partial one of balance - max_effective_balance  if credentials[0] == eth1_prefix, effective_balance ==
 *                                                          max_effective_balance and balance > max_effective_balance,
 * to the address credentials[12:32], with consecutive indices from next_withdrawal_index; the loop stops at the
 * max_withdrawals_per_payload-th hit.  bound <= n: no validator is visited twice, the positions behind the last hit taken are
 * not touched.  Comparisons unsigned 64-bit.
 * out_withdrawals (room for max_withdrawals_per_payload entries; may be NULL) takes the expected list, *out the rest.
 * With PE_WD_PAYLOAD the payload must equal the expected list in length and in every field; else THE BLOCK IS INVALID: the
 * call returns PE_OK, out->status and out->first_mismatch say where, and NOTHING CHANGES (out still describes the expected
 * list).  With PE_WD_APPLY and a matching payload the balances of the expected withdrawals' validators are debited.
 * Reads the credentials (pe_registry_set_static), the withdrawable epochs and balances (pe_state_set_balances) and the
 * working-state view's effective balances (the pe_set_validators data while the view mirrors it; the view is not
 * materialised); writes the balances alone.  pe_state_get_balances reads them back, pe_state_roots hashes them with no
 * further call.  Read-only passes (k_withdrawals_flag, _scan, _select: the first hits in position order by wave ballots and
 * an ordered scan of per-workgroup counts), a host step (the comparison, the next indices, the list root), one writing pass
 * (k_withdrawals_apply: one writer per balance, no atomic).  Synchronous (completes open pipelines first); one GPU.  A
 * block runs this call before pe_process_block_operations.  A failing call changes nothing:
 *   PE_ERR_STATE        the epochs, the balances or the static part are not resident, the view does not cover the registry,
 *                       or pe_dist_init* active
 *   PE_ERR_INVALID_ARG  the registry is empty; next_withdrawal_validator_index >= n; a parameter is 0; eth1_prefix above
 *                       0xFF; max_withdrawals_per_payload above 64; n_payload above it; next_withdrawal_index +
 *                       max_withdrawals_per_payload wraps; PE_WD_APPLY without PE_WD_PAYLOAD; unknown flag bits */
int pe_process_withdrawals(pe_engine* h, uint64_t current_epoch, uint64_t next_withdrawal_index,
                           uint64_t next_withdrawal_validator_index, const pe_withdrawals_params* params,
                           const pe_withdrawal* payload, uint32_t n_payload, uint32_t flags,
                           pe_withdrawal* out_withdrawals, pe_withdrawals_result* out);

#define PE_CRED_FLAG_SIGNATURE_VALID 0x1u /* the injected verdict over the SignedBLSToExecutionChange's signature: the caller
                                             computes it with the BLS calls from pe_bls_change_signing_roots, as
                                             PE_OP_FLAG_SIGNATURE_VALID */
typedef struct pe_bls_change {      /* BLSToExecutionChange and its verdict: 80 bytes */
    uint64_t validator_index;
    uint8_t  from_bls_pubkey[48];
    uint8_t  to_execution_address[20];
    uint32_t flags;                 /* PE_CRED_FLAG_* */
} pe_bls_change;

/* status[i] of pe_process_bls_to_execution_changes: 0 = valid, else the first assert of the change that fails, in its order */
typedef enum pe_cred_status {
    PE_CRED_OK = 0,
    PE_CRED_BAD_INDEX = 96,         /* validator_index >= n */
    PE_CRED_NOT_BLS = 97,           /* credentials[0] != 0x00 (before the call, or by an earlier change of it) */
    PE_CRED_PUBKEY_MISMATCH = 98,   /* credentials[1:] != SHA-256(from_bls_pubkey)[1:] */
    PE_CRED_BAD_SIGNATURE = 99      /* the injected verdict is false */
} pe_cred_status;

typedef struct pe_bls_changes_stats {
    uint64_t n_applied;             /* credentials written */
    uint64_t n_invalid;             /* changes with a status != 0 */
} pe_bls_changes_stats;

/* An ordered list of address changes applied to the resident withdrawal credentials with the semantics of the sequential
 * loop: a valid change writes 0x01 || 0^11 || to_execution_address; of two changes that name one validator the first that
 * passes every check takes effect and the second then fails the prefix check.  The hash is the plain SHA-256 of the 48 key
 * bytes, computed on the device from the change (not the SSZ leaf the static part keeps).
 * A BLOCK WITH AN INVALID CHANGE IS AN INVALID BLOCK: the call writes every status and, if any is not 0, CHANGES NOTHING (it
 * still returns PE_OK; out->n_invalid counts them).  Writes the credentials (pe_registry_set_static) alone;
 * pe_registry_get_static reads them back, pe_state_roots hashes them.  Read-only passes (k_bls_changes_claim, _resolve: the
 * first potent change per validator by a minimum over positions), one writing pass (k_bls_changes_apply: one writer per
 * validator).  Synchronous (completes open pipelines first); one GPU.  status: n_changes entries; out may be NULL.  A block
 * runs this call after its voluntary exits.  A failing call changes nothing:
 *   PE_ERR_STATE        the static part is not resident, or pe_dist_init* active
 *   PE_ERR_CAPACITY     the registry holds 2^32 or more validators */
int pe_process_bls_to_execution_changes(pe_engine* h, const pe_bls_change* changes, uint32_t n_changes, int32_t* status,
                                        pe_bls_changes_stats* out);
/* out_roots32[32 i ..] = compute_signing_root(BLSToExecutionChange(change i), domain), hashed on the device; the flags are not
 * read.  pe_hash_to_g2 of these and pe_pairing_check / pe_batch_verify against from_bls_pubkey give the verdicts.
 * Synchronous; needs no registry. */
int pe_bls_change_signing_roots(pe_engine* h, const pe_bls_change* changes, uint32_t n, const uint8_t domain[32],
                                uint8_t* out_roots32);

/* ---- SSZ roots of the resident per-validator lists -------------------------- */
/* hash_tree_root (named at pe:142, 423, 1016; the reference holds no text of it) by the SSZ specification's rules: chunks of
 * 32 bytes; basic values packed little-endian, the last chunk zero-padded; Z[0] = 32 zero bytes, Z[k+1] = H(Z[k] || Z[k]);
 * merkleize(chunks, depth) = the root of the binary tree of 2^depth leaves whose absent leaves are Z[0];
 * mix_in_length(root, n) = H(root || uint256_le(n)); H = SHA-256.  Restated in tests/ssz_model.py.
 *
 * The parts of Validator (pe:36-45) nothing else in the engine reads: pubkey (48 B compressed), withdrawal_credentials
 * (32 B) and activation_eligibility_epoch of the whole registry.  Kept in device memory as the pubkey's 32-byte leaf
 * H(pubkey[0:32] || pubkey[32:48] || 0^16) + 32 B + 8 B per validator.  n must equal pe_num_validators(h): else
 * PE_ERR_INVALID_ARG and nothing changes.  Dropped where the working-state view is: pe_store_init, and a
 * pe_set_validators that changes n.  _get: any output may be NULL; *out_is_set = 0: none held, nothing is written.
 * Checkpoint / resume: _get for the credentials and epochs, the caller's own pubkeys, _set -- as with the epochs. */
int pe_registry_set_static(pe_engine* h, uint64_t n, const uint8_t* pubkeys48, const uint8_t* withdrawal_credentials32,
                           const uint64_t* activation_eligibility_epoch);
int pe_registry_get_static(pe_engine* h, uint64_t n, uint8_t* out_pubkey_leaves32, uint8_t* out_withdrawal_credentials32,
                           uint64_t* out_activation_eligibility_epoch, int* out_is_set);

#define PE_ROOT_BALANCES   1u   /* List[Gwei, 2^limit_log2] over the resident balances (pe_state_set_balances) */
#define PE_ROOT_INACTIVITY 2u   /* List[uint64, 2^limit_log2] over the resident inactivity scores */
#define PE_ROOT_PART_PREV  4u   /* List[ParticipationFlags, 2^limit_log2] over previous_epoch_participation */
#define PE_ROOT_PART_CUR   8u   /* ... over current_epoch_participation */
#define PE_ROOT_VALIDATORS 16u  /* List[Validator, 2^limit_log2] */
typedef struct pe_state_root_set {
    uint8_t balances[32];
    uint8_t inactivity_scores[32];
    uint8_t previous_epoch_participation[32];
    uint8_t current_epoch_participation[32];
    uint8_t validators[32];
} pe_state_root_set;
/* The hash_tree_root of the BeaconState fields (pe:354-369) named by `which`, from the arrays where they lie in device
 * memory; the fields of *out not asked for are left as they were.  Combining them with the state's other field roots into
 * hash_tree_root(state) is a handful of hashes and stays with the caller.
 * limit_log2: log2 of VALIDATOR_REGISTRY_LIMIT (0 = 40).  Tree depths: limit_log2 - 2 for the uint64 lists, limit_log2 - 5
 * for the uint8 lists, limit_log2 for validators; each root is mixed with n = pe_num_validators(h).
 * Validator: effective_balance and slashed (PE_VAL_SLASHED) are the working-state view's (pe_state_set_validators; the
 * pe_set_validators data while the view mirrors it), activation / exit epochs the resident ones (pe_registry_set_epochs),
 * withdrawable_epoch the one of pe_state_set_balances, the rest pe_registry_set_static's.
 * out_validator_leaves (may be NULL; V x 32 B): hash_tree_root(Validator) of every validator, with PE_ROOT_VALIDATORS.
 * Read-only: no resident array changes, the view is not materialised.  Synchronous (completes open pipelines first;
 * ordered against the flag passes as pe_ffg_balances is); one GPU.  A failing call writes nothing to *out:
 *   PE_ERR_INVALID_ARG  which is 0 or has other bits; limit_log2 above 64, below 5, or 2^limit_log2 < n
 *   PE_ERR_STATE        an array `which` asks for is not resident (PE_ROOT_VALIDATORS needs the epochs, the balances and
 *                       the static part), or pe_dist_init* active */
int pe_state_roots(pe_engine* h, uint32_t which, uint32_t limit_log2, pe_state_root_set* out, uint8_t* out_validator_leaves);

/* merkleize(chunks, depth) of n_chunks 32-byte chunks in host memory -- block_roots, state_roots, randao_mixes, any Vector
 * or List of Bytes32 or of packed basic values -- through the same kernel.  mix_length >= 0: the root is mixed with that
 * length; < 0: no mix-in.  n_chunks = 0 gives Z[depth].  n_chunks > 2^depth or depth > 64: PE_ERR_INVALID_ARG, out_root
 * is not written.  Synchronous. */
int pe_ssz_merkleize(pe_engine* h, const uint8_t* chunks32, uint64_t n_chunks, uint32_t depth, int64_t mix_length,
                     uint8_t out_root[32]);

/* ---- deposits: process_deposit over the resident registry (pe:139-175) ------- */
/* DepositData (pe:91-95) as it travels: 184 bytes, no padding. */
typedef struct pe_deposit_data {
    uint8_t pubkey[48];
    uint8_t withdrawal_credentials[32];
    uint64_t amount;
    uint8_t signature[96];
} pe_deposit_data;
typedef struct pe_deposit_params {
    uint64_t effective_balance_increment;  /* 10^9 */
    uint64_t max_effective_balance;        /* 32 * 10^9; at most 65535 increments */
    uint64_t far_future_epoch;             /* 2^64 - 1: the four epochs of a new validator */
} pe_deposit_params;
void pe_deposit_params_default(pe_deposit_params* out);
typedef enum pe_deposit_status {
    PE_DEP_APPENDED = 0,               /* a new pubkey with a valid signature: state.validators.append (pe:166-170) */
    PE_DEP_TOPUP = 1,                  /* the pubkey is in the registry (or was created earlier in this batch): increase_balance */
    PE_DEP_IGNORED_BAD_SIGNATURE = 2,  /* a new pubkey whose bls.Verify is false (pe:165): the key does not decode or fails
                                          KeyValidate, the signature does not decode or lies outside G2, or the pairing
                                          product is not 1.  The reference skips such a deposit silently */
    PE_DEP_BAD_PROOF = 3               /* is_valid_merkle_branch false (pe:141): the reference's assert */
} pe_deposit_status;
typedef struct pe_deposit_stats {
    uint32_t n_appended, n_topups, n_ignored, n_bad_proof;
    uint64_t n_validators;             /* pe_num_validators(h) after the call */
} pe_deposit_stats;
/* out_roots32[32 i ..] = compute_signing_root(DepositMessage(deposit i), domain) (pe:157-163), hashed on the device:
 * H(hash_tree_root(DepositMessage) || domain).  pe_hash_to_g2 of these (tag: Ethereum's signature DST) gives
 * pe_process_deposits' message_points192.  Synchronous; needs no registry. */
int pe_deposit_signing_roots(pe_engine* h, const pe_deposit_data* deposits, uint32_t n, const uint8_t domain[32],
                             uint8_t* out_roots32);
/* process_deposit for n deposits, with the reference's semantics applied sequentially in batch order: a deposit's pubkey is
 * looked up in the registry as the deposits before it left it (where the registry holds a pubkey twice the lowest index is
 * the match, as .index() returns it); the first deposit of a new pubkey with a valid signature creates validator
 * pe_num_validators + (validators created before it in this batch); later deposits of that pubkey are top-ups whose
 * signature is not looked at; earlier ones with a bad signature are ignored.
 * proofs: n x 33 x 32 bytes, the branch of deposit i against deposit_root at index eth1_deposit_index + i (depth 33: the
 * length mix-in is the last node; the leaf is hash_tree_root(DepositData)); NULL = proofs are not checked (genesis).  If ANY
 * deposit fails its proof nothing is applied: the failing ones read PE_DEP_BAD_PROOF, the others the status they would have
 * had, every out_index is 0xFFFFFFFF, out->n_appended = n_topups = 0 and the call returns PE_OK.
 * message_points192: H(signing_root_i) in the 192-byte form of pe_pairing_check, one per deposit (read for new pubkeys
 * only; may be NULL when the caller knows there are none -- a new pubkey then fails with PE_ERR_INVALID_ARG).
 * status[i]: pe_deposit_status.  out_index[i] (may be NULL): the validator credited, or 0xFFFFFFFF.  out may be NULL.
 * What grows: every resident per-validator array, by capacity doubling, contents kept -- the working-state view (effective
 * balance min(amount - amount % increment, max), not active, not slashed; a view that still mirrored the pe_set_validators
 * data becomes one of its own), activation / exit / eligibility / withdrawable epochs (far_future_epoch), balances
 * (amount), inactivity scores and both participation lists (0), pubkey leaves and withdrawal credentials, the G1 pubkey
 * table (where keys are loaded) and the pubkey index itself.  The justified-state arrays of pe_set_validators take
 * effective balance 0, inactive, no latest message until the caller's next pe_set_validators(new n, ...): get_head does not
 * see the new validators.  Dropped, as derived from n: the resident active list (pe_active_set) and the committee sums.
 * Committee tables of past epochs name old indices only and stay.
 * Synchronous (completes open pipelines first); one GPU.
 *   PE_ERR_STATE        pe_dist_init* active; the slasher is enabled (its history is sized for n: pe_slasher_disable first);
 *                       pe_registry_set_static, pe_state_set_balances or pe_registry_set_epochs missing; the registry
 *                       would grow beyond 2^32 - 2 validators.  Nothing changes.
 *   PE_ERR_INVALID_ARG  an amount above 2^63 (increase_balance does not saturate: the sums of a call then cannot wrap);
 *                       increment 0 or max_effective_balance above 65535 increments.  Nothing changes. */
int pe_process_deposits(pe_engine* h, const pe_deposit_data* deposits, uint32_t n, const uint8_t* proofs,
                        uint64_t eth1_deposit_index, const uint8_t deposit_root[32], const uint8_t* message_points192,
                        const pe_deposit_params* params, int32_t* status, uint32_t* out_index, pe_deposit_stats* out);

/* Plain G1 sum over caller-chosen groups: out[g] = sum_{j in [offsets[g], offsets[g+1])}
 * points[index[j]] (index NULL = identity).  points96 NULL = the validators' pubkeys.
 * The input points are NOT validated, here or in pe_g2_sum, pe_g1_key_validate, pe_g2_subgroup_check and pe_set_validators
 * (one converter each for G1 and G2 feeds them all): no test for coordinates < p, none for the curve equation.  Bit 6 of
 * byte 0 set is the identity whatever else the encoding holds; bits 7 and 5 of byte 0 are masked and ignored (the pairing
 * calls below REFUSE bit 7); a coordinate >= p is reduced.  A caller that needs the checks has the pairing calls, or the
 * decompress calls, which build y themselves. */
int pe_g1_sum(pe_engine* h, const uint8_t* points96, uint64_t n_points,
              const uint32_t* index, const uint32_t* offsets, uint32_t n_groups, uint8_t* out96);

/* BLSPubkey wire format (Validator.pubkey: BLSPubkey, pe:37): 48 bytes, big-endian x, flag bits in the leading byte
 * (bit 7 compressed, bit 6 infinity, bit 5 y > (p-1)/2).  Decompression runs on the GPU (one square root per key);
 * status[i]: 0 ok, 1 malformed encoding (flag bits, x >= p), 2 x is not on the curve.  Subgroup: pe_g1_key_validate.
 *   pe_g1_decompress          48-byte keys -> 96-byte uncompressed affine (the format pe_set_validators takes)
 *   pe_set_pubkeys_compressed decompress straight into the registry of the n validators already loaded;
 *                             any status != 0 fails the call (PE_ERR_INVALID_ARG) and leaves no pubkeys loaded
 *   pe_g1_compress            96-byte affine -> 48-byte compressed (serialisation only: host, no handle) */
/* KeyValidate (FastAggregateVerify validates every pubkey before summing them, Appendix A.7; call sites pe:736, pe:976):
 * beyond "decodes to a curve point" (pe_g1_decompress / pe_set_pubkeys_compressed) a key must not be the identity and
 * must lie in the prime-order subgroup, r * P == infinity -- one 255-bit scalar multiplication per key on the GPU.
 * points96: n uncompressed points, or NULL = the n pubkeys of the registry as loaded.
 * status[i]: 0 valid, 3 not in the subgroup, 4 identity.  An optional once-per-registry-load pass (~65 ms per 1 M keys). */
int pe_g1_key_validate(pe_engine* h, const uint8_t* points96, uint64_t n, int32_t* status);
int pe_g1_decompress(pe_engine* h, const uint8_t* in48, uint64_t n, uint8_t* out96, int32_t* status);
int pe_set_pubkeys_compressed(pe_engine* h, uint64_t n, const uint8_t* pubkeys48, int32_t* status);
int pe_g1_compress(const uint8_t* in96, uint64_t n, uint8_t* out48);

/* bls.Aggregate over real BLSSignature points (type pe:37, Attestation.signature pe:717; aggregation prose pe:659,
 * pe:1536): plain G2 sum over caller-chosen groups, out[g] = sum_{j in [offsets[g], offsets[g+1])} points[index[j]]
 * (index NULL = identity).  Points are 192-byte uncompressed affine, ZCash order x.c1 | x.c0 | y.c1 | y.c0, each 48
 * bytes big-endian; bit 6 of byte 0 flags infinity.  Outputs are canonical affine in the same format (exact).
 * Like pe_g1_sum, pe_g2_sum and pe_g2_subgroup_check validate nothing: bits 7 and 5 of byte 0 are ignored, no coordinate is
 * tested against p or the curve (see pe_g1_sum). */
#define PE_G2_POINT_BYTES 192
/* BLSSignature wire format (pe:37, pe:717): 96 bytes x.c1 | x.c0, flag bits as for BLSPubkey with the sign taken on
 * (y.c1, y.c0).  pe_g2_decompress runs on the GPU (an Fp2 square root per point: two Fp exponentiations, ~0.95 ms
 * per 8192 points); status[i]: 0 ok, 1 malformed, 2 not on the curve; no subgroup check.  pe_g2_compress is host-side
 * serialisation. */
int pe_g2_decompress(pe_engine* h, const uint8_t* in96, uint64_t n, uint8_t* out192, int32_t* status);
int pe_g2_compress(const uint8_t* in192, uint64_t n, uint8_t* out96);
int pe_g2_sum(pe_engine* h, const uint8_t* points192, uint64_t n_points,
              const uint32_t* index, const uint32_t* offsets, uint32_t n_groups, uint8_t* out192);
/* bls.Aggregate per committee over the UNAGGREGATED signatures of an epoch (pe:717: one BLSSignature per attester; pe:474,
 * pe:659, pe:1536: aggregated per committee): signatures96 = n compressed signatures (host or DEVICE memory; device memory
 * at a 16-byte boundary is read in place), aggregate g = sum of signatures96[index[j]] for j in [offsets[g], offsets[g+1])
 * (index: host or device memory, NULL = identity; offsets: host), decompressed on the whole chip (k_g2_decompress: an Fp2
 * square root each, curve membership checked; PE_SIG_CHECK_SUBGROUP adds the endomorphism test), summed (k_g2_accumulate /
 * k_g2_finish) and handed back compressed in out_signatures96 (n_groups x 96 bytes, host).  sig_status (nullable, n entries,
 * host): 0 ok, 1 malformed, 2 not on the curve, 3 outside G2; a signature that does not decode is left out of its sum and
 * counted in out_bad[g] (nullable, n_groups entries).  Synchronous.  1 048 576 signatures in 2048 committees: ~1 k
 * Fp products per signature against ~10 per addition -- the decompression is the cost of the call. */
int pe_aggregate_signatures(pe_engine* h, const uint8_t* signatures96, uint64_t n, const uint32_t* index,
                            const uint32_t* offsets, uint32_t n_groups, uint32_t sig_flags, uint8_t* out_signatures96,
                            int32_t* sig_status, uint32_t* out_bad);

/* ---- inspection (parity checks) ---------------------------------------- */
uint32_t pe_num_blocks(const pe_engine* h);
uint64_t pe_num_validators(const pe_engine* h);
int pe_block_root_at(const pe_engine* h, uint32_t block_index, uint8_t out_root[32]);
int pe_block_index_of(const pe_engine* h, const uint8_t root[32], uint32_t* out_index);
/* store.latest_messages: epoch and block index per validator; block index
 * 0xFFFFFFFF = no message (epoch 0), PE_VOTE_PRUNED = a message whose block pe_prune removed (its epoch is kept). */
int pe_get_latest_messages(pe_engine* h, uint64_t* out_epoch, uint32_t* out_block_index, uint64_t n);

/* ---- pruning at finalization ------------------------------------------------------------------------------------
 * The block table holds at most 8192 LIVE blocks (the tree kernel keeps it in LDS); pe_prune re-roots it at
 * store.finalized_checkpoint.root.  Kept: exactly the finalized root and its descendants, in their relative insertion
 * order (still parent-first), so the root becomes block 0 with parent 0xFFFFFFFF; its proper ancestors and every side
 * branch go.  on_block refuses a block that does not descend from the finalized root (pe:998-1005), get_head starts at
 * the justified root (pe:1106), which descends from it, and a block's weight is the sum over its own subtree (pe:322):
 * no removed block can be a head, a child in the descent or a parent of a new block, nor add to the weight of one that
 * can, so the call is unobservable to pe_get_head.
 *   Latest messages stay on the device and follow the re-indexing there (k_votes_remap).  A message on a removed block
 * keeps its epoch -- update_latest_messages compares against it (pe:1440): a later vote of an equal or lower epoch is
 * still refused -- and its block index becomes PE_VOTE_PRUNED: it weighs on nothing, which is what it weighs on among
 * the kept blocks in the reference.  pe_get_latest_messages reports (epoch, PE_VOTE_PRUNED); pe_set_latest_messages
 * accepts that pair, so export / import round-trip a pruned store.
 *   Synchronous, like pe_active_set: it first issues held-back launches and completes every open pipeline.  Everything
 * that can fail is checked before anything changes: store not initialised -> PE_ERR_STATE; finalized root not in the
 * table -> PE_ERR_UNKNOWN_ROOT; justified root (or a non-zero best_justified root that is in the table) outside the kept
 * subtree -> PE_ERR_STATE; a handle with pe_dist_init* active -> PE_ERR_STATE.  With the finalized root already at block 0
 * the call changes nothing and launches nothing (blocks_before == blocks_after, zero vote counts).  proposer_boost_root
 * stays as it is (a boost root that is not in the table boosts nothing); the weights of pe_get_last_weights are dropped;
 * the slasher's history holds no block indices and is not touched.  The caller decides when: typically after a
 * pe_on_block that raised finalized_checkpoint.
 *   DEVIATION (the reference's Store never forgets a block): the pruned store equals the reference store with those
 * blocks deleted from store.blocks, and equals the unpruned reference on every call sequence in which no later call names
 * a deleted block.  An attestation that names one fails the reference's own assert "beacon_block_root / target.root in
 * store.blocks" (A.4) with PE_ATT_UNKNOWN_BEACON_BLOCK_ROOT / PE_ATT_UNKNOWN_TARGET_ROOT; a block whose parent was
 * removed fails pe:990 (PE_ERR_UNKNOWN_PARENT) where the unpruned reference would fail at pe:1000.  Both are rejections
 * that leave the store untouched. */
#define PE_VOTE_PRUNED 0xFFFFFFFEu   /* latest message whose block was pruned */
typedef struct pe_prune_stats {
    uint32_t blocks_before, blocks_after;
    uint64_t votes_remapped;   /* latest messages whose block was kept under another index */
    uint64_t votes_orphaned;   /* latest messages whose block was removed by this call */
} pe_prune_stats;
int pe_prune(pe_engine* h, pe_prune_stats* out /* may be NULL */);
/* ---- checkpoint / resume: the store is a handful of flat arrays -------------------------------
 * Export: pe_get_store_scalars, pe_get_block x pe_num_blocks (insertion order: parents first), pe_get_validator_flags
 * (incl. PE_VAL_EQUIVOCATING), pe_get_latest_messages (+ _slots under the vote-expiry variant), pe_participation_get.
 * Import into a fresh handle: pe_store_init(genesis_time, block 0) -> pe_set_block_checkpoints(0, ...) (after a pe_prune
 * block 0 is an ordinary block whose post-state checkpoints decide filter_block_tree's leaf test) -> pe_add_block in order -> pe_set_validators
 * (balances, flags without the equivocating bit, pubkeys) -> pe_mark_equivocating -> pe_set_latest_messages ->
 * pe_on_tick(time) -> pe_set_checkpoints / pe_set_best_justified / pe_set_proposer_boost -> pe_participation_set.
 * pos_evolution_amd.Engine.export_state / import_state do exactly this. */
int pe_get_block(const pe_engine* h, uint32_t block_index, uint8_t root[32], uint32_t* parent_index, uint64_t* slot,
                 uint64_t* post_justified_epoch, uint8_t post_justified_root[32],
                 uint64_t* post_finalized_epoch, uint8_t post_finalized_root[32]);
int pe_get_validator_flags(const pe_engine* h, uint8_t* out_flags, uint64_t n);
int pe_get_latest_message_slots(pe_engine* h, uint32_t* out_slot, uint64_t n);
/* The post-state checkpoints of a block already in the table (block_states[root].current_justified_checkpoint /
 * .finalized_checkpoint), as pe_get_block reports them: pe_store_init gives block 0 the anchor checkpoint for both. */
int pe_set_block_checkpoints(pe_engine* h, uint32_t block_index, uint64_t post_justified_epoch,
                             const uint8_t post_justified_root[32], uint64_t post_finalized_epoch,
                             const uint8_t post_finalized_root[32]);
/* block_index 0xFFFFFFFF = no message (the epoch is ignored); PE_VOTE_PRUNED = a message of that epoch on a pruned block;
 * slot may be NULL (only read under the vote-expiry variant). */
int pe_set_latest_messages(pe_engine* h, uint64_t n, const uint64_t* epoch, const uint32_t* block_index,
                           const uint32_t* slot);
int pe_set_best_justified(pe_engine* h, uint64_t epoch, const uint8_t root[32]);
int pe_get_store_scalars(const pe_engine* h, uint64_t* time, uint64_t* genesis_time,
                         uint64_t* justified_epoch, uint8_t justified_root[32],
                         uint64_t* finalized_epoch, uint8_t finalized_root[32],
                         uint64_t* best_justified_epoch, uint8_t best_justified_root[32],
                         uint8_t proposer_boost_root[32]);

/* ---- pe_aggregate with its signature leg (bls.Aggregate, pe:659, pe:714-717) -------------------------------------- */
/* Everything pe_aggregate does, plus Attestation.signature of every aggregate it forms: the sum in G2 of the member
 * attestations' BLSSignatures, returned in the 96-byte compressed wire form (pe:37, pe:717) -- what a validator client
 * publishes as "a well-packed aggregate attestation" (pe:659).
 *   signatures        n signatures, one per input row, in host or device memory (host memory is read before the call
 *                     returns -- a buffer refilled per step is fine; device memory is read where the leg runs, which in a
 *                     pipeline may be after the call: it stays unchanged until the pipeline has completed, like device rows):
 *                     PE_SIG_G2_COMPRESSED    96 bytes each (x.c1 | x.c0 big-endian, flag bits in the leading byte): decoded
 *                                             on the device (square root in Fp2, sign and canonicity checks, curve membership);
 *                     PE_SIG_G2_UNCOMPRESSED  192 bytes each (x.c1 | x.c0 | y.c1 | y.c0): converted, trusted to lie on the curve;
 *   | PE_SIG_CHECK_SUBGROUP  additionally r * P = infinity for every decoded point (a curve point outside G2 is not a
 *                     BLSSignature; is_valid_indexed_attestation, pe:736 / pe:976, presumes members of G2);
 *   out_signatures96  96 bytes per group formed, group order as out_atts (capacity: n entries);
 *   sig_status        n entries, one per input row: PE_SIG_OK, PE_SIG_MALFORMED (encoding), PE_SIG_NOT_ON_CURVE,
 *                     PE_SIG_NOT_IN_SUBGROUP.
 * A member whose signature does not decode is left out of its group's sum and the group's row loses
 * PE_ATT_FLAG_SIGNATURE_VALID (the handlers then reject it with PE_ATT_BAD_SIGNATURE): an aggregate over an invalid
 * signature can never verify.  Members with overlapping bits: the row carries PE_ATT_FLAG_OVERLAPPING_BITS as with
 * pe_aggregate, and its signature is the plain sum (which counts a validator twice -- such an aggregate does not verify
 * either, Appendix A.8).  Rows in host or device memory, synchronous or inside a pipeline, exactly as pe_aggregate.
 * The signature leg (decode, per-group sums, compression, statuses) runs on a stream of its own that is joined into no
 * other: whoever completes the pipeline waits for it.  In a streaming pipeline (pe_pipeline_begin_streaming) over
 * compressed signatures the leg is not launched by the call but COLLECTED: the legs of POSEVO_SIG_BATCH steps (default
 * 8) share one decompression launch, which goes out with the call that fills the batch -- or when one of the collected
 * pipelines completes (a drain, a synchronous call, a lag depth shorter than the batch).  That launch and the sums behind
 * it last 4-5 steps: with a lag depth (pe_pipeline_set_lag) of at least the batch plus those steps the host never waits
 * for a leg (bench.py's signed steps run at depth 15); a shallower lag gives the same outputs, its lagged end launches
 * what its arena still holds collected and waits for it.  Uncompressed signatures are never collected.
 * Several signed aggregates inside ONE pipeline: the leg's device scratch is one set of buffers per pipeline, so every
 * further signed call first launches the leg the pipeline still holds collected and orders its own signature copy and leg
 * behind that leg's end.  The legs of one pipeline therefore run one after the other, each with a decompression launch
 * of its own (~1 ms for up to 64 Ki signatures), and the engine's stream waits for the earlier leg: correct, but without
 * the batching a streaming caller gets from one signed call per pipeline. */
#define PE_SIG_G2_COMPRESSED   1u
#define PE_SIG_G2_UNCOMPRESSED 2u
#define PE_SIG_CHECK_SUBGROUP  0x100u
#define PE_SIG_OK 0
#define PE_SIG_MALFORMED 1
#define PE_SIG_NOT_ON_CURVE 2
#define PE_SIG_NOT_IN_SUBGROUP 3
int pe_aggregate_signed(pe_engine* h, const pe_attestation* atts, uint32_t n,
                        const uint8_t* bits_arena, uint64_t arena_len,
                        const uint8_t* signatures, uint32_t sig_format_flags,
                        pe_attestation* out_atts, uint32_t* out_n_groups, uint32_t* group_of,
                        uint8_t* out_bits_arena, uint64_t out_arena_cap,
                        uint8_t* out_signatures96, int32_t* sig_status,
                        uint8_t* out_aggpk96, uint32_t* out_count);
/* The subgroup check on its own: n points in the 192-byte uncompressed form (host memory); status[i] = PE_SIG_OK or
 * PE_SIG_NOT_IN_SUBGROUP (infinity passes). */
int pe_g2_subgroup_check(pe_engine* h, const uint8_t* points192, uint64_t n, int32_t* status);

/* ---- the pairing check (is_valid_indexed_attestation's last step, pe:736, 976, 1456) ------------------------------
 * Batched optimal-ate pairing products on the device.  Points in the formats above: 96-byte uncompressed G1 (x | y),
 * 192-byte uncompressed G2 in ZCash order (x.c1 | x.c0 | y.c1 | y.c0), infinity = bit 6 of byte 0.  All arrays in host
 * memory.  Every point is checked against its curve equation (and for canonical coordinates) on the device:
 *   bit 6 of byte 0 set            infinity, whatever else the encoding holds (0xC0.., 0x60.., 0x40 over non-zero bytes)
 *   otherwise bit 7 of byte 0 set  PE_BLS_BAD_POINT: the compressed form is refused (pe_g1_sum / pe_g2_sum ignore the bit)
 *   bit 5 of byte 0                no part of the leading coordinate: ignored
 *   any coordinate >= p            PE_BLS_BAD_POINT (x + p is no second spelling of x); the elements after the first are
 *                                  plain 384-bit integers, so any of their top three bits set is >= p
 *   off the curve                  PE_BLS_BAD_POINT
 * verdict[g]: 1  the product of e(P_j, Q_j) over j in [offsets[g], offsets[g+1]) is 1
 *             0  it is not
 *             2  a point of the group is not on its curve (PE_BLS_BAD_POINT)
 * an empty group gives 1 (the empty product); infinity on either side contributes 1.
 * Subgroup membership is the caller's: pe_g1_key_validate / pe_g2_subgroup_check.
 * Synchronous (completes open pipelines first); one GPU: PE_ERR_STATE on a handle with pe_dist_init* active.
 * offsets not monotone or past n_pairs: PE_ERR_INVALID_ARG.  Not computed here: hash_to_curve (pe_hash_to_g2 makes the
 * message point H(m) in G2; these calls take it).  One final exponentiation per group; pe_batch_verify below pays one per call. */
#define PE_BLS_VALID 1
#define PE_BLS_INVALID 0
#define PE_BLS_BAD_POINT 2
int pe_pairing_check(pe_engine* h, const uint8_t* g1_points96, const uint8_t* g2_points192, uint64_t n_pairs,
                     const uint32_t* offsets, uint32_t n_groups, int32_t* verdict);
/* FastAggregateVerify per group: the pubkeys registry[index[j]], j in [offsets[g], offsets[g+1]), are summed on the device
 * (the route of pe_g1_sum), and the pairs (sum, message_points192[g]), (-G1, signatures192[g]) are checked.
 * verdict[g] as above; an empty group gives 0 (FastAggregateVerify refuses n = 0), an identity signature gives 0.
 * The verdict may be passed on as PE_ATT_FLAG_SIGNATURE_VALID where the caller injects it today.  No pubkeys loaded:
 * PE_ERR_STATE; an index outside the registry: PE_ERR_INVALID_ARG. */
int pe_fast_aggregate_verify(pe_engine* h, const uint32_t* index, const uint32_t* offsets, uint32_t n_groups,
                             const uint8_t* message_points192, const uint8_t* signatures192, int32_t* verdict);
/* Many aggregates at once, by random linear combination:
 *     prod_g e(r_g pk_g, H(m_g)) * e(-G1, sum_g r_g sig_g) == 1
 * Only the message pairs pay a Miller loop each, and when every group is valid the whole call pays ONE final exponentiation;
 * otherwise the engine finds the invalid groups itself (per chunk of groups, then one by one).  Formats, host-memory arrays,
 * synchronous completion and PE_ERR_STATE under pe_dist_init* are those of the calls above.
 * pe_batch_verify takes one aggregate pubkey per group (96-byte G1, e.g. out_aggpk96 of pe_aggregate_signed, decompressed);
 * pe_batch_fast_aggregate_verify sums registry[index[j]], j in [offsets[g], offsets[g+1]), as pe_fast_aggregate_verify does.
 * verdict[g] is what pe_fast_aggregate_verify gives the group, for every input whose signatures lie in G2:
 *     1  valid     0  invalid (also: an empty group, an identity aggregate key, an identity signature)     2  a point off its curve
 * and a signature on the curve but outside G2 -- not a BLSSignature -- gives 0: it is decided by the subgroup check before
 * batching, because the combination is sound over G2 only.  Message points are taken to be hash outputs (in G2) and pubkeys to
 * be KeyValidated, as in the calls above.
 * scalars: n_groups non-zero 64-bit values, or NULL: the engine draws them from the operating system's generator (getrandom).
 * NULL is the production mode.  Caller-supplied scalars MUST BE UNPREDICTABLE to whoever made the signatures: knowing r_1, r_2,
 * a forger submits sig_1 + r_2 D and sig_2 - r_1 D, whose combination is that of the honest pair, and both groups pass.  With
 * secret scalars a wrong 1 has probability about 2^-64 per call.  A zero scalar: PE_ERR_INVALID_ARG. */
int pe_batch_verify(pe_engine* h, const uint8_t* pubkeys96, const uint8_t* message_points192,
                    const uint8_t* signatures192, uint32_t n_groups, const uint64_t* scalars, int32_t* verdict);
int pe_batch_fast_aggregate_verify(pe_engine* h, const uint32_t* index, const uint32_t* offsets, uint32_t n_groups,
                                   const uint8_t* message_points192, const uint8_t* signatures192,
                                   const uint64_t* scalars, int32_t* verdict);
/* An epoch's UNAGGREGATED signatures, each decided: an aggregate can be valid while two of its members are forged (sig_a + D and
 * sig_b - D sum to the honest aggregate), so pe_aggregate_signatures' output says nothing about its members.  All members of a
 * group signed the same message (one committee's votes for one AttestationData), and with secret weights r_j
 *     e(sum_j r_j pk_j, H(m_g)) * e(-G1, sum_j r_j sig_j) == 1
 * decides them all with ONE two-pair check per group; the two weighted sums are the device's work (k_g1_weighted_accumulate,
 * k_g2_weighted_accumulate).  Only a group that fails pays one pairing check per member, all such groups in one further run.
 *   signatures96   n compressed BLSSignatures, host or device memory, as pe_aggregate_signatures takes them
 *   index          host; member j's signature is signatures96[index[j]]; NULL: member j's is signatures96[j]
 *   signer         host; member j's validator index: its pubkey is the registry's (taken as KeyValidated)
 *   offsets        host; group g = members [offsets[g], offsets[g+1])
 *   message_points192   H(m_g), one 192-byte G2 point per group (pe_hash_to_g2 makes them)
 *   scalars        host; one non-zero 64-bit r_j per member, or NULL: drawn from getrandom.  NULL is the production mode.
 *                  Caller-supplied scalars MUST BE UNPREDICTABLE to the signers, exactly as for pe_batch_verify: with r_a = r_b
 *                  known, sig_a + D and sig_b - D both pass.  With secret scalars a wrong 1 has probability <= 2^-64 per group.
 *   member_verdict per member: 1 valid, 0 not
 *   sig_status     nullable, per member: 0 ok, 1 malformed, 2 off the curve, 3 on the curve outside G2 (the subgroup test is
 *                  always on: the combination is sound over G2 only), PE_SIG_STATUS_IDENTITY the point at infinity.  A member
 *                  whose status is not 0 has verdict 0 and is left out of both sums: it cannot spoil its group.
 *   group_verdict  1 iff every member's verdict is 1 (an empty group: 1); 2: H(m_g) is not on its curve (its members: 0);
 *                  a group whose message point is the identity has 0, and so has every member
 *   out_signatures96   nullable: per group the compressed aggregate of the members with verdict 1 (none: infinity) -- for a
 *                  group without a bad member byte for byte pe_aggregate_signatures(..., PE_SIG_CHECK_SUBGROUP)'s
 * Synchronous; completes open pipelines first.  PE_ERR_STATE without pubkeys or under pe_dist_init*; PE_ERR_INVALID_ARG for a
 * zero scalar, a signer outside the registry, an index outside n, non-monotone offsets: nothing is written then. */
#define PE_SIG_STATUS_IDENTITY 4
int pe_verify_signatures(pe_engine* h, const uint8_t* signatures96, uint64_t n, const uint32_t* index, const uint32_t* signer,
                         const uint32_t* offsets, uint32_t n_groups, const uint8_t* message_points192, const uint64_t* scalars,
                         int32_t* member_verdict, int32_t* sig_status, int32_t* group_verdict, uint8_t* out_signatures96);

/* The RESIDENT aggregate decided where it lies: every group of the handle's last pe_aggregate_signed over rows in device memory
 * (with out_aggpk96 requested) gets the verdict of e(aggregate key, H(m)) e(-G1, aggregate signature) == 1, computed from the
 * key and the signature that aggregate left in device memory -- no wait for out_aggpk96 / out_signatures96, no second
 * decompression, no upload of points the device already holds.
 *   message_points192   n_points message points H(m), 192-byte G2 wire form; host memory, or device memory (read in place when
 *                       16-byte aligned, copied otherwise).  pe_hash_to_g2 writes them there.
 *   point_of_row        host memory, one entry per INPUT row of that aggregate: the group a row went into takes the point of
 *                       its first row (pe_attestation order of appearance).  NULL: group g takes message_points192[g].
 *   flags               PE_VERIFY_APPLY: on the device, sig_valid of every group decided by rows 2-4 below becomes
 *                       sig_valid AND (verdict == 1) -- pe_on_attestation_batch / pe_process_attestation_batch with
 *                       PE_ROWS_RESIDENT then answer PE_ATT_BAD_SIGNATURE for the groups that did not verify.  Idempotent.
 *   verdict             cap entries in group order; entries past the groups formed read 0.
 * verdict[g], first matching row:
 *   1. the group has no committee (its row status says why)                                  PE_BLS_UNDECIDED, sig_valid untouched
 *   2. its message point is not canonical or not on its curve                                PE_BLS_BAD_POINT
 *   3. its members overlap | a member's signature did not decode or failed the leg's subgroup check | its union is empty
 *      (identity aggregate key) | identity aggregate signature | identity message point | aggregate signature outside G2
 *                                                                                            PE_BLS_INVALID
 *   4. the pairing product is 1: PE_BLS_VALID, otherwise PE_BLS_INVALID
 * The G2 test of row 3 is the call's own pass over the aggregate signatures; it is skipped when the aggregate ran with
 * PE_SIG_CHECK_SUBGROUP (sums of members of G2 lie in G2).
 * Synchronous: completes open pipelines first.  PE_ERR_STATE unless the handle's last aggregate is such a pe_aggregate_signed,
 * the store's clock and committee tables are what it resolved against (the rule of PE_ROWS_RESIDENT), and no pe_dist_init* is
 * active; PE_ERR_INVALID_ARG for a point_of_row entry >= n_points, or n_points below the group count without point_of_row;
 * PE_ERR_CAPACITY for cap below the group count.  An error writes nothing and applies nothing. */
#define PE_BLS_UNDECIDED 3
#define PE_VERIFY_APPLY  0x1u
int pe_verify_resident(pe_engine* h, const uint8_t* message_points192, uint32_t n_points, const uint32_t* point_of_row,
                       uint32_t flags, uint32_t cap, int32_t* verdict);

/* ---- hash_to_curve: the message points H(m) from messages (RFC 9380) -------- */
/* Suite BLS12381G2_XMD:SHA-256_SSWU_RO_: hash_to_field by expand_message_xmd over SHA-256, the simplified SWU map onto the
 * isogenous curve, the 3-isogeny to the twist, the sum of the two mapped points, clear_cofactor.  What comes out is the 192-byte
 * G2 wire form (x.c1 | x.c0 | y.c1 | y.c0) that pe_fast_aggregate_verify, pe_batch_verify, pe_verify_signatures,
 * pe_verify_resident and pe_process_deposits take as message points.
 *   msgs      n messages of msg_len bytes each, back to back; 0 <= msg_len <= 255.  Host memory, or device memory (read in
 *             place when 16-byte aligned, copied otherwise).  NULL is allowed for msg_len == 0.
 *   dst       the domain separation tag, host memory, 1 <= dst_len <= 255 (Ethereum's signatures:
 *             "BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_")
 *   out192    n x 192 bytes.  Host memory, or device memory as pe_verify_resident accepts its message points (written in
 *             place when 16-byte aligned, through a copy otherwise): signing roots -> H(m) -> verdict then never cross to
 *             the host.
 *   status    nullable, host memory, one per message: 0, or 1 where H(m) is the identity (out192: 0x40 and zeros) -- no known
 *             message gives it; the verification calls refuse an identity message point.
 * Synchronous, one GPU.  PE_ERR_STATE under pe_dist_init* and inside a pipeline (between pe_pipeline_begin* and its end);
 * PE_ERR_INVALID_ARG for dst_len outside 1 .. 255, msg_len above 255 or a missing array; PE_ERR_CAPACITY above 2^24 messages.
 * n == 0 returns PE_OK.  An error writes nothing. */
int pe_hash_to_g2(pe_engine* h, const uint8_t* msgs, uint32_t n, uint32_t msg_len, const uint8_t* dst, uint32_t dst_len,
                  uint8_t* out192, int32_t* status);
/* The same from field elements -- the RFC's own seam behind hash_to_field: out192[i] = clear_cofactor(map_to_curve(u0_i) +
 * map_to_curve(u1_i)).
 *   u_be      host memory, n x 192 bytes: u0.c0 | u0.c1 | u1.c0 | u1.c1 (c0 + c1 i), each a 48-byte big-endian integer below p
 *   out192    as pe_hash_to_g2's
 * u = 0 takes the map's exceptional case, u1 = u0 the doubling, u1 = -u0 gives the identity.  Errors as pe_hash_to_g2;
 * PE_ERR_INVALID_ARG also for a word that is not below p. */
int pe_map_to_g2(pe_engine* h, const uint8_t* u_be, uint32_t n, uint8_t* out192);

/* ---- the message of an attestation's signature, from the attestation itself -------- */
/* is_valid_indexed_attestation verifies over compute_signing_root(data, get_domain(state, DOMAIN_BEACON_ATTESTER,
 * data.target.epoch)) = H(hash_tree_root(AttestationData) || domain).  The state's part of that is three values: */
#define PE_ETH2_DST "BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_"   /* Ethereum's signature tag, 43 bytes */
typedef struct pe_attester_domains {      /* get_domain(state, DOMAIN_BEACON_ATTESTER, data.target.epoch) */
    uint64_t fork_epoch;                  /* state.fork.epoch */
    uint8_t  domain_previous[32];         /* compute_domain(type, fork.previous_version, genesis_validators_root) */
    uint8_t  domain_current[32];          /* ... fork.current_version ...: taken where target.epoch >= fork_epoch */
} pe_attester_domains;                    /* 72 bytes */

/* out_roots32[i] = the signing root of rows[i], 32 bytes each, back to back as pe_hash_to_g2 takes its messages.  Of a row only
 * the seven fields of AttestationData enter (slot, index, beacon_block_root, source, target): bits_offset, n_bits, flags and
 * reserved0 do not.  Nine SHA-256 of 64 bytes per row, on the device.
 *   rows, out_roots32   each host memory, or device memory (used in place when 16-byte aligned, through a copy otherwise)
 * Needs no store and no registry.  Synchronous, one GPU.  PE_ERR_STATE under pe_dist_init* and inside a pipeline;
 * PE_ERR_INVALID_ARG for a missing dom or array; PE_ERR_CAPACITY above 2^24 rows.  n == 0 returns PE_OK.  An error writes
 * nothing. */
int pe_attestation_signing_roots(pe_engine* h, const pe_attestation* rows, uint32_t n, const pe_attester_domains* dom,
                                 uint8_t* out_roots32);

/* pe_verify_resident with the messages taken from the groups themselves: group g is verified over the signing root of ITS
 * OWN AttestationData (its first input row's; a group is formed by AttestationData equality) under dom, hashed to G2 with
 * PE_ETH2_DST -- signing roots, (u0, u1), message points and pairings all on the call's stream in one workspace, nothing of
 * the messages crossing to the host in between.  The caller names no message, so it cannot name the wrong one.
 *   out_roots32   nullable, host memory, 32 x cap: the groups' signing roots in group order (entries past the groups read 0);
 *                 also written for a group without a committee
 * Preconditions, flags, cap, the verdict table (row 2 cannot occur: the points are the engine's own), the counters of the profile
 * hook, the completion of open pipelines and the errors are pe_verify_resident's;
 * PE_ERR_INVALID_ARG also for a NULL dom. */
int pe_verify_resident_data(pe_engine* h, const pe_attester_domains* dom, uint32_t flags, uint32_t cap, int32_t* verdict,
                            uint8_t* out_roots32);

/* ---- sync committees (Altair): sampling, verification, rewards ------------- */
/* The handle keeps two committees in device memory, the CURRENT one (whose members sign and are paid) and the NEXT one, each a
 * list of `size` validator indices -- duplicates allowed -- with its aggregate pubkey: the compressed G1 sum of the members'
 * registry pubkeys, a validator listed k times counted k times (eth_aggregate_pubkeys).
 * Lifetime: both are dropped by pe_store_init, by a pe_set_validators that changes the registry's size or brings pubkeys, and
 * by pe_set_pubkeys_compressed; they survive pe_process_deposits (indices stay valid as the registry grows). */
#define PE_SYNC_COMMITTEE_MAX 512   /* SYNC_COMMITTEE_SIZE of mainnet; the minimal preset has 32 */
#define PE_SYNC_MAX_BATCH 64        /* aggregates of one pe_process_sync_aggregate */
#define PE_SYNC_CURRENT 0
#define PE_SYNC_NEXT 1
/* get_next_sync_committee: with total = n_active and i = 0, 1, ... the candidate
 * active[compute_shuffled_index(i % total, total, seed)] is appended iff
 * effective_balance * 255 >= max_effective_balance * hash(seed + uint64_le(i / 32))[i % 32] -- pe_compute_proposers' rule
 * (pe:604-618), so member 0 and its i are what that call returns for the seed -- until `size` members are appended; a
 * validator may be appended more than once, and is when n_active < size.  Sampled on the device (k_sync_sample, in batches
 * of 16 384 candidates); the indices and the aggregate key STAY ON THE DEVICE as the handle's NEXT committee.
 *   seed, active_indices / n_active / shuffle_round_count   as pe_compute_proposers: NULL = validators 0..n_active-1,
 *       PE_ACTIVE_RESIDENT accepted, same validation; an empty active set is PE_ERR_INVALID_ARG
 *   max_effective_balance   effective balances = the working-state view, as for the proposers
 *   size            1 .. PE_SYNC_COMMITTEE_MAX (else PE_ERR_INVALID_ARG)
 *   max_tries       candidates examined before giving up (0 = 2^20)
 *   out_indices u32[size] (may be NULL), out_aggregate_pubkey48 (may be NULL): copies of what stays resident
 *   out_tries (may be NULL): the i of the last accepted candidate + 1
 * Fewer than `size` acceptances within max_tries: PE_ERR_CAPACITY and *out_tries = max_tries; both resident committees and the
 * other outputs stay as they were.  Needs pubkeys loaded (PE_ERR_STATE).  Synchronous; one GPU: PE_ERR_STATE on a handle with
 * pe_dist_init* active. */
int pe_sync_committee_compute(pe_engine* h, const uint8_t seed[32], const uint32_t* active_indices, uint32_t n_active,
                              uint32_t shuffle_round_count, uint64_t max_effective_balance, uint32_t size, uint32_t max_tries,
                              uint32_t* out_indices, uint8_t* out_aggregate_pubkey48, uint32_t* out_tries);
/* Checkpoint / resume and genesis: `which` = PE_SYNC_CURRENT or PE_SYNC_NEXT.
 * _set: indices u32[size], 1 <= size <= PE_SYNC_COMMITTEE_MAX, every index below pe_num_validators(h) (else
 *   PE_ERR_INVALID_ARG, nothing changed); the aggregate key is computed from the registry (PE_ERR_STATE without pubkeys).
 * _get: *out_size = the committee's size, 0 where none is held (nothing else is written then); out_indices (may be NULL) has
 *   room for `cap` entries, PE_ERR_CAPACITY where that is fewer than the size; out_aggregate_pubkey48 may be NULL. */
int pe_sync_committee_set(pe_engine* h, int which, const uint32_t* indices, uint32_t size);
int pe_sync_committee_get(pe_engine* h, int which, uint32_t* out_indices, uint32_t cap, uint32_t* out_size,
                          uint8_t* out_aggregate_pubkey48);
/* process_sync_committee_updates' move at a period boundary: current = next, and there is no next until the caller computes
 * or sets one.  PE_ERR_STATE without a next committee. */
int pe_sync_committee_rotate(pe_engine* h);

/* SyncAggregate of one block with what process_sync_aggregate reads beside it.  The engine reads neither state.block_roots nor
 * the forks (as with pe_attester_domains): the caller supplies get_block_root_at_slot(state, previous_slot) and
 * get_domain(state, DOMAIN_SYNC_COMMITTEE, compute_epoch_at_slot(previous_slot)). */
typedef struct pe_sync_aggregate {
    uint8_t  bits[64];         /* sync_committee_bits: bit p is (bits[p / 8] >> (p % 8)) & 1 */
    uint8_t  signature[96];    /* sync_committee_signature, compressed */
    uint8_t  block_root[32];
    uint8_t  domain[32];
    uint32_t proposer_index;   /* get_beacon_proposer_index(state) of the block */
    uint32_t reserved0;
} pe_sync_aggregate;           /* 232 bytes */
typedef struct pe_sync_params {
    uint64_t total_active_balance;   /* get_total_active_balance(state), as pe_active_set returns it */
    uint64_t base_reward_factor;     /* BASE_REWARD_FACTOR */
} pe_sync_params;
void pe_sync_params_default(pe_sync_params* out);   /* base_reward_factor 64; total_active_balance 0: the caller's */
typedef struct pe_sync_stats {
    uint64_t participant_reward;   /* per set bit; also the penalty per clear bit */
    uint64_t proposer_reward;      /* per set bit, to the aggregate's proposer */
    uint64_t n_participants;       /* set bits over all aggregates */
    uint64_t credited;             /* Gwei added to balances */
    uint64_t debited;              /* Gwei actually taken off balances (decrease_balance stops at 0) */
    uint64_t n_saturated;          /* decreases that stopped at 0 */
    uint64_t applied;              /* 1: the balances were changed */
} pe_sync_stats;
#define PE_SYNC_VERIFY 0x1u
#define PE_SYNC_APPLY  0x2u
/* process_sync_aggregate for the aggregates of n consecutive blocks, n <= PE_SYNC_MAX_BATCH, all over the resident CURRENT
 * committee (size S).  Per aggregate: the participants' indices in committee order and the signing root
 * sha256(block_root || domain) = hash_tree_root(SigningData) on the device (k_sync_members), then
 * PE_SYNC_VERIFY   verdict[b] = eth_fast_aggregate_verify(participants' pubkeys, signing root, signature): 1 valid, 0 invalid,
 *                  2 a point off its curve.  No participant AND the compressed infinity signature (0xC0, 95 zero bytes): 1.
 *                  Otherwise FastAggregateVerify: no participant, an identity signature or an identity aggregate key: 0.  A
 *                  signature that does not decode or lies outside G2: 0, and sig_status[b] (nullable; else 0) says why: 1
 *                  malformed, 2 not on the curve, 3 not in the subgroup.  The keys are summed by pe_g1_sum's route (a member
 *                  listed twice and participating twice counts twice), the root hashed by pe_hash_to_g2 under PE_ETH2_DST.
 *                  Without this flag verdict and sig_status are not touched and may be NULL.
 * PE_SYNC_APPLY    with participant_reward and proposer_reward from
 *                      per_increment = increment * base_reward_factor / isqrt(total_active_balance)
 *                      total_base = per_increment * (total_active_balance / increment)
 *                      participant_reward = total_base * 2 / 64 / slots_per_epoch / S;  proposer_reward = participant_reward * 8 / 56
 *                  (increment and slots_per_epoch are the handle's cfg), aggregate by aggregate and in committee order p = 0 .. S-1:
 *                  bit set: balance[member[p]] += participant_reward, balance[proposer] += proposer_reward; bit clear:
 *                  balance[member[p]] -= min(balance, participant_reward) -- onto the resident balances (pe_state_set_balances),
 *                  exactly as the sequential loop leaves them (k_sync_rewards).  Additions wrap, as in pe_rewards_and_penalties.
 *                  With both flags the balances change only when every verdict is 1 (out->applied says which).
 * out (may be NULL): the scalars and what was done; credited .. n_saturated are 0 where nothing was applied.
 * PE_ERR_STATE: no current committee; PE_SYNC_APPLY without resident balances; PE_SYNC_VERIFY without pubkeys; pe_dist_init*.
 * PE_ERR_INVALID_ARG: flags 0 or with other bits; n > PE_SYNC_MAX_BATCH; a set bit at a position >= S; a proposer_index
 *   outside the registry; total_active_balance below the increment; a step of the scalar chain above that exceeds 64 bits
 *   (decided on the host in 128 bits).  A failing call changes nothing.  n == 0 returns PE_OK.
 * Synchronous (completes open pipelines first); one GPU. */
int pe_process_sync_aggregate(pe_engine* h, const pe_sync_aggregate* aggs, uint32_t n, const pe_sync_params* params,
                              uint32_t flags, int32_t* verdict, int32_t* sig_status, pe_sync_stats* out);

/* ---- multi-GPU exchange (validator-range shards) ----------- */
/* Each rank owns a contiguous validator range and the whole (small) block table.
 * get_head splits at the one exchange point:
 *   pe_votes_partial  : this shard's direct vote weight per block (tree order) into a
 *                       caller-owned DEVICE buffer of n_blocks + PE_EXCHANGE_EXTRA u64;
 *                       the extra entries carry the shard's active balance / active
 *                       validator count as per-workgroup partials (the proposer boost
 *                       needs the global values, Appendix A.1).  Asynchronous on the
 *                       engine's stream.
 *   <host framework: ONE all-reduce(sum, u64) of the buffer -- RCCL via torch.distributed>
 *   pe_head_from_weights : subtree sums + descent from the reduced DEVICE buffer.
 * Integer sums: bit-exact for any reduction order. */
#define PE_EXCHANGE_EXTRA 512
int pe_votes_partial(pe_engine* h, void* dev_buf_u64, uint32_t n_blocks);
int pe_head_from_weights(pe_engine* h, const void* dev_buf_u64, uint32_t n_blocks, uint8_t out_root[32]);
/* G1: per-group partial sums in XYZZ coordinates (X|Y|ZZ|ZZZ, 4 x 48 B, Montgomery form) of this shard's
 * points into a caller-owned DEVICE buffer; after an all-gather over ranks,
 * pe_g1_finish adds the n_ranks partials per group and normalises to affine. */
#define PE_G1_PARTIAL_BYTES 192
/* dev_partials_capacity: how many partials (groups) the caller's device buffer holds; a batch that forms more groups
 * fails with PE_ERR_CAPACITY before anything is written. */
int pe_g1_partial(pe_engine* h, const uint32_t* index, const uint32_t* offsets, uint32_t n_groups,
                  void* dev_partials, uint32_t dev_partials_capacity);
int pe_g1_finish(pe_engine* h, const void* dev_gathered, uint32_t n_ranks, uint32_t n_groups,
                 uint8_t* out96);
/* pe_aggregate whose aggregate pubkeys stay projective (XYZZ) partials of THIS shard's committee
 * members, written to a caller-owned DEVICE buffer (PE_G1_PARTIAL_BYTES per group, group
 * order as in out_atts); all-gather them and call pe_g1_finish.  Asynchronous w.r.t. the
 * partials; everything else as pe_aggregate. */
int pe_aggregate_partial(pe_engine* h, const pe_attestation* atts, uint32_t n,
                         const uint8_t* bits_arena, uint64_t arena_len,
                         pe_attestation* out_atts, uint32_t* out_n_groups, uint32_t* group_of,
                         uint8_t* out_bits_arena, uint64_t out_arena_cap, uint32_t* out_count,
                         void* dev_partials, uint32_t dev_partials_capacity);

/* ---- RCCL inside the engine: the exchange steps behind the C ABI ---------- */
/* For clients without a collective library of their own (the cgo / bindgen / Panama bindings of INTEGRATION.md): the
 * engine owns its RCCL communicators and issues the two collectives on its own streams, between its own kernels.
 *   rank 0: pe_dist_unique_id(id); ship the PE_DIST_ID_BYTES to the other ranks (any side channel)
 *   every rank: pe_dist_init(h, id, rank, world)      -- one process per GPU, one handle per process
 *   pe_get_head_sharded   = pe_votes_partial -> ncclAllReduce(u64, sum, B + PE_EXCHANGE_EXTRA) -> pe_head_from_weights
 *   pe_aggregate_sharded  = pe_aggregate_partial -> ncclAllGather(192 B x groups) -> pe_g1_finish
 * The id holds two ncclUniqueIds: the all-reduce and the all-gather have a communicator each, because inside a
 * pipeline the G1 chain of a step (partials -> all-gather -> finish) runs on the engine's finishing stream beside the
 * next step's fork-choice kernels and their all-reduce, and one communicator must not be driven from two streams.
 * pe_aggregate_sharded takes its rows from host memory or -- like pe_aggregate -- from DEVICE memory (grouping and
 * committee resolution on the device, handlers with PE_ROWS_RESIDENT; every rank passes the same rows in the same order,
 * each with the bits of ITS members).
 * Both calls may be made inside pe_pipeline_begin(_streaming) ... _end(_lagged): nothing then waits except the poll
 * for the head; pe_aggregate_sharded's unions are handed on with PE_BITS_RESIDENT like pe_aggregate's, its outputs are
 * complete where the pipeline's are.  Every rank must make the same sequence of calls (collectives pair up by order).
 * librccl is loaded with dlopen at the first pe_dist_* call (the copy already in the process, e.g. torch's, else the
 * ROCm installation's); single-GPU use never touches it. */
#define PE_DIST_ID_BYTES 256
int pe_dist_unique_id(uint8_t out_id[PE_DIST_ID_BYTES]);
int pe_dist_init(pe_engine* h, const uint8_t id[PE_DIST_ID_BYTES], int rank, int world);
/* Flags for pe_dist_init_ex (pe_dist_init = flags 0, or PE_DIST_SINGLE_COMM when POSEVO_DIST_SINGLE_COMM=1 is set):
 *   PE_DIST_SINGLE_COMM  both collectives on ONE communicator and ONE stream (the engine's): every rank then issues them
 *                        in program order on one queue, so two collective kernels can never become resident in different
 *                        orders on different ranks.  Costs overlap: a step's all-gather (behind its G1 partials) holds
 *                        the next step's fork-choice kernels back.  The form to fall back to when the two-communicator
 *                        form times out (PE_ERR_TIMEOUT). */
#define PE_DIST_SINGLE_COMM 1u
int pe_dist_init_ex(pe_engine* h, const uint8_t id[PE_DIST_ID_BYTES], int rank, int world, uint32_t flags);
/* The same exchange through the CALLER's collectives (MPI, a host-staged shim, a test double): two function pointers
 * replace RCCL.  Both operate on DEVICE memory and are ordered on the given HIP stream: an implementation either enqueues
 * on that stream or synchronises it, exchanges and returns -- work the engine enqueues on the stream afterwards must see
 * the result.  Return 0 on success; anything else fails the engine call with PE_ERR_NO_DEVICE.  The engine-owned
 * streaming sharded step runs unchanged on top (tests/test_gpu_dist_custom.py drives it with two ranks that share one
 * GPU). */
typedef struct pe_collectives {
    void* user;
    /* in-place sum over ranks of count uint64 at dev_buf */
    int (*all_reduce_u64)(void* user, void* dev_buf, uint64_t count, void* hip_stream);
    /* rank r's bytes_per_rank bytes at dev_send land at dev_recv + r * bytes_per_rank on every rank */
    int (*all_gather)(void* user, const void* dev_send, void* dev_recv, uint64_t bytes_per_rank, void* hip_stream);
} pe_collectives;
int pe_dist_init_custom(pe_engine* h, int rank, int world, const pe_collectives* fn);
/* Bounded waits (default 30 000 ms; 0 = wait for ever; POSEVO_DIST_TIMEOUT_MS presets it): once a handle has
 * pe_dist_init'ed, the waits for enqueued work poll with this limit; past it the call aborts the communicators
 * (ncclCommAbort), returns PE_ERR_TIMEOUT and the handle refuses further sharded calls until pe_dist_destroy +
 * pe_dist_init(_ex).  A hung exchange thus surfaces as an error on every rank instead of a stuck job.  The outputs of
 * the calls and pipelines in flight at that moment are lost (pe_pipeline_completed stays where it was); the store
 * keeps what the device had applied -- votes and flags are idempotent, the caller replays the lost steps. */
int pe_dist_set_timeout_ms(pe_engine* h, uint32_t ms);
/* Upper bound of the groups one pe_aggregate_sharded over rows in DEVICE memory may form (default: its row count n).  The
 * all-gather of such a call is sized before the device has formed the groups; a caller that knows its epoch has C
 * committees sets C and ships C x 192 B per rank instead of n x 192 B.  More groups than the bound: PE_ERR_CAPACITY where
 * the outputs complete. */
int pe_dist_set_max_groups(pe_engine* h, uint32_t max_groups);
int pe_dist_destroy(pe_engine* h);
int pe_get_head_sharded(pe_engine* h, uint8_t out_root[32]);
/* pe_get_head_async's counterpart: inside a pipeline nothing waits, out_root is written where the pipeline's outputs
 * complete (a streaming caller's loop then never waits for the all-reduce inside a step). */
int pe_get_head_sharded_async(pe_engine* h, uint8_t out_root[32]);
int pe_aggregate_sharded(pe_engine* h, const pe_attestation* atts, uint32_t n,
                         const uint8_t* bits_arena, uint64_t arena_len,
                         pe_attestation* out_atts, uint32_t* out_n_groups, uint32_t* group_of,
                         uint8_t* out_bits_arena, uint64_t out_arena_cap, uint8_t* out_aggpk96, uint32_t* out_count);

/* ---- committee-sharded steps (Option B; pe:474 "parallelising the aggregation of attestations") ---- */
/* The other way to split an epoch over N GPUs: by COMMITTEE instead of by validator range.  Every rank holds the whole
 * registry and the whole store; rank g is handed only the rows of the committees it serves (its attestation subnets) and
 * runs pe_aggregate over them as on one GPU -- its unions and its aggregate pubkeys are complete, there is no G1
 * collective, and a rank's grouping / union / G1 work is 1/N of the epoch's.  pe_aggregate_exchange then makes the
 * epoch whole again: the aggregates of the LAST pe_aggregate over rows in device memory (AttestationData + OR-ed bits +
 * attester count + verdict flags: the aggregate attestation a validator client publishes, pe:659, pe:714-717) are packed
 * into fixed slots, all-gathered over the handle's communicator (pe_dist_init / pe_dist_init_custom), and ingested as ONE
 * batch that becomes the handle's resident aggregate: the handlers that follow
 *     pe_on_attestation_batch(h, PE_ROWS_RESIDENT, cap, PE_BITS_RESIDENT, 0, status, NULL, out_count)
 *     pe_process_attestation_batch(h, state, PE_ROWS_RESIDENT, cap, PE_BITS_RESIDENT, 0, status, out_numerators)
 * apply the whole epoch's votes and flags to this rank's copy of the store, and pe_get_head (the plain one: no weight
 * exchange) returns the same head on every rank.  Outputs: the gathered aggregates, rank after rank (out_atts rows with
 * bits_offset into out_bits_arena, out_count), cap_groups entries each -- cap_groups >= world x the bound of
 * pe_dist_set_max_groups (required, and the same on every rank: PE_ERR_STATE without one -- the exchange is sized by it).  Every rank calls it once per step; inside a
 * pipeline nothing waits (with RCCL) and the local aggregate's G1 sums keep running beside the exchange.  A union may be
 * at most max_validators_per_committee bits (pe_config). */
int pe_aggregate_exchange(pe_engine* h, pe_attestation* out_atts, uint32_t* out_n_groups, uint8_t* out_bits_arena,
                          uint64_t out_arena_cap, uint32_t* out_count, uint32_t cap_groups);

/* ---- slashing detection: double and surround votes (pe:1128, pe:1134-1143, pe:1411-1415) -------------------------- */
/* The engine consumes slashings (pe_on_attester_slashing, pe_mark_equivocating); the slasher FINDS them in the
 * attestations the node already hands over.  Per validator and per target epoch of a window of history_epochs epochs
 * (W - H, W] it keeps the FIRST AttestationData the validator attested (in hand-over order), and per epoch the table of the
 * distinct AttestationData recorded for it (128 bytes each, compared exactly; at most max_data_per_epoch).  A record names
 * its data as (target_epoch, id); ids count the data of an epoch in order of first appearance.  Device memory: 12 *
 * history_epochs bytes per validator, and ~136-140 * history_epochs * max_data_per_epoch bytes for the data tables of the
 * device-row form.
 *
 * pe_slasher_enable   (pe:1411-1415: every validator "eventually recognises equivocations" in its own view) allocates the
 *                     history for the registry as loaded (pe_set_validators first; a registry of another size afterwards:
 *                     enable again).  Enabling again, pe_slasher_disable and pe_store_init drop every record and table.
 * pe_slasher_ingest   (pe:1128 the two Casper conditions, pe:1134-1143 is_slashable_attestation_data, pe:1447-1461
 *                     on_attester_slashing).  current_epoch may not decrease (PE_ERR_INVALID_ARG, nothing changes); it
 *                     becomes W, and epochs that left the window are cleared.  status[i], first match wins:
 *                       PE_SLASH_FUTURE_TARGET, PE_SLASH_TOO_OLD                     the window;
 *                       PE_ATT_NO_COMMITTEE_TABLE, _COMMITTEE_INDEX_OUT_OF_RANGE, _BITS_LENGTH_MISMATCH
 *                                                     the committee, resolved against the table of the row's target epoch as
 *                                                     pe_on_attestation_batch resolves it; the table must partition the registry;
 *                       PE_SLASH_TABLE_FULL           new data for an epoch whose table is full.
 *                     Then, for every validator v and every accepted row a with v's bit set, in array order: if v's record
 *                     for a's target epoch holds a's data nothing happens; otherwise a is compared with every record b of v
 *                     in the window and every slashable pair is one pe_slash_evidence:
 *                       PE_SLASH_DOUBLE    same target epoch, different data: (d1, d2) = (the recorded one, a);
 *                       PE_SLASH_SURROUND  d1.source < d2.source and d2.target < d1.target: d1 is the surrounding vote --
 *                                          the argument order on_attester_slashing (pe:1454) accepts;
 *                     and a is recorded if v's slot for its target epoch is empty (a rejected double vote is not recorded).
 *                     *out_n_found = pieces of evidence found; the first `cap` that arrive are written to out_evidence in no
 *                     particular order, THE REST IS DROPPED -- the history is updated all the same, so a caller that
 *                     wants every pair sizes cap generously (out_n_found tells when it did not).
 *                     flags & PE_SLASH_APPLY: every validator with evidence joins store.equivocating_indices on the device =
 *                     on_attester_slashing with attesting_indices = [v] on both sides (pe:1459-1461), exact whatever cap is.
 *                     Rows are host memory; bits host, pinned or device memory, or PE_BITS_RESIDENT with rows of the last
 *                     pe_aggregate's out_atts.  Synchronous; inside a pipeline it first completes the outstanding work.
 *                     ROWS IN DEVICE MEMORY:
 *                       pe_slasher_ingest(h, PE_ROWS_RESIDENT, cap_rows, PE_BITS_RESIDENT, 0, current_epoch, flags, status, ...)
 *                     ingests every group of the last pe_aggregate over rows in device memory, in group order, as the host-row
 *                     call over that aggregate's out_atts would: same statuses, evidence, records and data ids (the two forms
 *                     mix on one handle and continue one sequence of ids).  The host reads nothing of the rows.  status holds
 *                     cap_rows entries; those past the groups formed read 0; fewer than groups: PE_ERR_CAPACITY.  Any other
 *                     bits_arena: PE_ERR_INVALID_ARG.  No valid resident aggregate, or the store's clock / committee tables
 *                     changed since it: PE_ERR_STATE, as for the handlers; so is a handle with pe_dist_init* active.  An
 *                     aggregate that failed ingests nothing and returns its error.  A group whose target epoch is >= 2^32 - 2
 *                     or whose source epoch is >= 2^32 - 1 fails the whole call (PE_ERR_INVALID_ARG).  A failing call changes
 *                     nothing.  RESTRICTION of this form: committees are the ones the aggregate resolved, against the tables
 *                     of the store's current and previous epoch only -- after the window statuses, a group with an older
 *                     target epoch reads PE_ATT_NO_COMMITTEE_TABLE even where a table for it is loaded.
 * pe_slasher_get_data     the AttestationData behind (target_epoch, id): the leading 128 bytes of *out, the rest zero.
 * pe_slasher_get_records  the records of one target epoch: source epoch and data id per validator, 0xFFFFFFFF = none
 *                         (parity tests, checkpoint).  An epoch outside the window reads as empty. */
#define PE_SLASH_APPLY    0x1u
#define PE_SLASH_DOUBLE   1u
#define PE_SLASH_SURROUND 2u
typedef struct pe_slash_evidence {
    uint32_t validator, kind;           /* PE_SLASH_DOUBLE / PE_SLASH_SURROUND */
    uint32_t target_epoch_1, id_1;      /* d1 */
    uint32_t target_epoch_2, id_2;      /* d2 */
} pe_slash_evidence;
int pe_slasher_enable(pe_engine* h, uint32_t history_epochs, uint32_t max_data_per_epoch);
int pe_slasher_disable(pe_engine* h);
int pe_slasher_ingest(pe_engine* h, const pe_attestation* atts, uint32_t n, const uint8_t* bits_arena, uint64_t arena_len,
                      uint64_t current_epoch, uint32_t flags, int32_t* status, pe_slash_evidence* out_evidence, uint32_t cap,
                      uint32_t* out_n_found);
int pe_slasher_get_data(pe_engine* h, uint64_t target_epoch, uint32_t id, pe_attestation* out);
int pe_slasher_get_records(pe_engine* h, uint64_t target_epoch, uint32_t* out_source_epoch, uint32_t* out_id, uint64_t n);

/* Measurement hooks (per-kernel event brackets, the in-situ timeline) are not part of the boundary: include/posevo_profile.h. */

#ifdef __cplusplus
}
#endif
#endif /* POSEVO_H */
