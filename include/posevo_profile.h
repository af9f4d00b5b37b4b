/* posevo_profile.h -- measurement hooks of libposevo.so: per-kernel launch counts / durations from HIP events the engine
 * records around its own launches, and an in-situ timeline of a streaming step.  NOT part of the drop-in boundary
 * (include/posevo.h): nothing a client of the reference's functions needs; bench.py's `roofline` leg and
 * tools/engine_timeline.py use them. */
#ifndef POSEVO_PROFILE_H
#define POSEVO_PROFILE_H
#include "posevo.h"
#ifdef __cplusplus
extern "C" {
#endif

/* When enabled, the engine brackets each launch of its kernels with HIP events on
 * the launch stream and accumulates per-kernel launch counts and durations. */
#define PE_KERNEL_G1_ACCUMULATE 0
#define PE_KERNEL_G1_NORMALISE  1
#define PE_KERNEL_VOTES         2
#define PE_KERNEL_TREE          3
#define PE_KERNEL_LMD           4
#define PE_KERNEL_PARTICIPATION 5
#define PE_KERNEL_BITS_UNION    6
#define PE_KERNEL_G2_ACCUMULATE 7
#define PE_KERNEL_G2_NORMALISE  8
#define PE_KERNEL_G1_TREE       9   /* the LDS tree over the lane partials: its own kernel since round 2 */
#define PE_KERNEL_ATT_GROUP     10  /* rows in device memory: ingest + plan + members (bracketed in timeline mode only) */
#define PE_KERNEL_ATT_VALIDATE  11  /* rows in device memory: the validate_on_attestation / process_attestation kernels (ditto) */
/* paired launches of a streaming caller (round 5): the fork-choice kernel of step N and the row kernel of step N + 1 as block
 * ranges of one grid (pair_kernels.hip); the stand-alone ids above count only the launches that ran alone */
#define PE_KERNEL_PAIR_INGEST_VALIDATE 12
#define PE_KERNEL_PAIR_PLAN_LMD        13
#define PE_KERNEL_PAIR_MEMBERS_VOTES   14
#define PE_KERNEL_PAIR_UNION_TREE      15
#define PE_KERNEL_G2_DECOMPRESS 16  /* the signature legs' decompression: one launch per POSEVO_SIG_BATCH streaming steps (round 6) */
#define PE_KERNEL_COUNT         17
/* on = 0 off, 1 per-kernel totals, 3 totals of PE_KERNEL_G1_ACCUMULATE only (what a timed region can afford: every bracket is
 * two event packets on its stream), 2 totals + a timeline: every bracketed launch's start (relative to the last
 * pe_profile_reset, which marks time zero on the engine's stream) and duration, read with pe_profile_timeline.  The
 * events are the engine's own, on the streams the kernels run on: an in-situ picture of a streaming step without a
 * profiler's serialisation (rocprofv3 stretches the 0.28 ms step to 0.4). */
int pe_profile_enable(pe_engine* h, int on);
int pe_profile_reset(pe_engine* h);
int pe_profile_get(pe_engine* h, int kernel, uint64_t* launches, double* total_ms);
/* The launches bracketed since the last pe_profile_reset, in the order they were drained (per kernel kind, launch order
 * inside a kind): kernel id, start and duration in ms.  At most cap entries are written; *out_n = how many exist. */
int pe_profile_timeline(pe_engine* h, int32_t* kernel, double* start_ms, double* duration_ms, uint32_t cap, uint32_t* out_n);

/* Which of the handle's four hot streams (engine, accumulation, tree, finish) share a hardware queue, asked of the device
 * again (a spin kernel on one stream, clock stamps on the others; everything enqueued completes first):
 * out_class[i] = the lowest i' whose stream shares stream i's queue -- {0, 1, 2, 3} when every stream has a queue of its own,
 * which is what pe_engine_create arranges whatever the process created before the handle (POSEVO_QUEUE_PROBE=0 skips it). */
int pe_profile_queue_classes(pe_engine* h, int32_t out_class[4]);
/* How often the handle has (re)allocated a buffer of its arenas (staging / output blocks, resident words, G1 and signature scratch)
 * since it was created.  Every such growth inside a stream of steps is milliseconds of allocation or a drained pipeline; after the
 * first step of a stream of like steps the count must stand still, whatever the lag depth. */
int pe_profile_arena_growths(const pe_engine* h, uint64_t* out);
/* Which route the aggregate pubkeys take (POSEVO_COMMITTEE_SUMS): how many of the handle's committee tables hold valid
 * per-committee pubkey sums, and how many groups of the last COMPLETED pe_aggregate over rows in device memory were summed by
 * complement (committee sum minus the absentees) instead of directly. */
int pe_profile_committee_sums(const pe_engine* h, uint32_t* out_tables_with_sums, uint32_t* out_groups_by_complement);
/* The shader clock each k_g1_accumulate launch ran at, in MHz, for the launches since pe_profile_reset made while profiling was
 * on (the last 4096 of them), in launch order: workgroup 0 of every launch counts shader cycles against the fixed 100 MHz counter.
 * out_n = how many there are; at most cap are written.  The clock is the power management's and a multiplier-bound kernel follows
 * it one to one: ~2.05 GHz for the first milliseconds of heavy load after an idle moment, ~2.4 GHz after ~35 ms of it
 * (tools/clockramp.hip, profiles/r06_clockramp.txt) -- which is most of the distance between a 20-step and a 200-step run. */
int pe_profile_accumulate_mhz(pe_engine* h, double* out_mhz, uint32_t cap, uint32_t* out_n);
/* For the parity tests of pe_pairing_check (same arguments): the value each group's verdict compares with 1, i.e. the Miller
 * loop's product raised to (p^12 - 1) / r * 3 -- the reduced pairing product cubed.  576 bytes per group: the 12 Fp
 * coefficients as plain (not Montgomery) residues, 48 bytes big-endian each, in the order c_0.c0, c_0.c1, c_1.c0, ... c_5.c1,
 * where c_k = c_k.c0 + c_k.c1 u is the Fp2 coefficient of w^k in Fp12 = Fp2[w] / (w^6 - (1 + u)); in the tower
 * Fp6 = Fp2[v] / (v^3 - (1 + u)), Fp12 = Fp6[w] / (w^2 - v), c_(2i+j) is the coefficient of v^i w^j. */
int pe_profile_pairing_gt(pe_engine* h, const uint8_t* g1_points96, const uint8_t* g2_points192, uint64_t n_pairs,
                          const uint32_t* offsets, uint32_t n_groups, uint8_t* out576);
/* pe_batch_verify / pe_batch_fast_aggregate_verify.  A chunk is c live groups and the one signature pair they share: c + 1 pairs
 * on one Miller accumulator.  c is the handle's knob, 1 .. PE_BATCH_CHUNK_MAX; the tests walk it. */
#define PE_BATCH_CHUNK_MAX 64
int pe_profile_batch_set_chunk(pe_engine* h, uint32_t chunk);
/* What the handle's last batch call did: out[0] live groups (what the settle pass left), [1] chunks, [2] launches of the
 * product tree, [3] values put through the final exponentiation at the top level (1, or 0 without a live group), [4] chunk
 * values exponentiated in the fallback, [5] groups rechecked one by one, [6] c, [7] F (the product tree's fan-in).
 * An honest batch shows [3] == 1 and [4] == [5] == 0. */
int pe_profile_batch_stats(const pe_engine* h, uint32_t out[8]);
/* The 576 bytes (layout of pe_profile_pairing_gt) the last batch call's top-level verdict compared with 1: the product of the
 * chunk values raised to (p^12 - 1) / r * 3.  Without a live group: the bytes of 1. */
int pe_profile_batch_gt(const pe_engine* h, uint8_t* out576);

/* pe_verify_signatures.  A slot of the weighted sums is a stripe of k members of one group (one Horner pass over the 64 bit
 * planes per stripe: 64 / k doublings per point); k is the handle's knob, 1 .. PE_VERIFY_STRIPE_MAX; the tests walk it to reach
 * the layout's edges with a few hundred points. */
#define PE_VERIFY_STRIPE_MAX 16
int pe_profile_verify_set_stripe(pe_engine* h, uint32_t k);
/* What the handle's last pe_verify_signatures did: out[0] members the settle pass decided (status != 0), [1] groups whose
 * combined check failed, [2] members rechecked one by one, [3] pairing runs (1, or 2 with the locate pass), [4] k. */
int pe_profile_verify_stats(const pe_engine* h, uint32_t out[5]);
/* The last call's weighted sums per group, canonical affine wire bytes: sum_j r_j pk_j (96 each) and sum_j r_j sig_j (192 each)
 * over the members the settle pass left.  n_groups must be the last call's. */
int pe_profile_verify_sums(const pe_engine* h, uint32_t n_groups, uint8_t* out_pk96, uint8_t* out_sig192);

/* pe_verify_resident.  What the handle's last call did: out[r] for r < 9 = groups decided by row r of the rule table, in its
 * precedence order: [0] no committee (PE_BLS_UNDECIDED), [1] message point not canonical or off its curve, [2] overlapping
 * members, [3] a member's signature did not decode or failed its subgroup check, [4] empty union (identity aggregate key),
 * [5] identity aggregate signature, [6] identity message point, [7] aggregate signature outside G2, [8] the pairing value;
 * out[9] = 1 when the call ran its own subgroup pass over the aggregate signatures (0: the leg ran with PE_SIG_CHECK_SUBGROUP),
 * out[10] = groups.  A call that failed leaves the previous call's numbers. */
#define PE_VERIFY_RESIDENT_STATS 11
int pe_profile_verify_resident_stats(const pe_engine* h, uint32_t out[PE_VERIFY_RESIDENT_STATS]);

/* pe_process_deposits.  The pubkey index the handle keeps: *out_slots = its u32 slots (0 = none: never built, or dropped with
 * the static part), a power of two: at a build the smallest one >= max(64, 2 (validators + the call's deposits)), doubled until
 * that holds again when a later call outgrows it; a pubkey's first slot is the first four bytes of its leaf, little-endian,
 * masked; *out_keys = validators in it; *out_build_ms = device time of the last full build (paid once per handle and static
 * part, not per call).  Any output may be NULL. */
int pe_profile_deposit_index(const pe_engine* h, uint32_t* out_slots, uint64_t* out_keys, float* out_build_ms);

#ifdef __cplusplus
}
#endif
#endif /* POSEVO_PROFILE_H */
