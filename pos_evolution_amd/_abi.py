"""ctypes declarations of include/posevo.h -- the only way Python reaches the engine.

The library is built in-tree (``pos_evolution_amd/libposevo.so``, see
``__graft_entry__.build``).  There is no fallback: a missing library raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# POSEVO_LIB_PATH: another build of the same sources (kernel-variant experiments, tools/); the default is the in-tree library
LIB_PATH = os.environ.get("POSEVO_LIB_PATH") or os.path.join(_HERE, "libposevo.so")

PE_OK = 0
PE_ERR_INVALID_ARG = -1
PE_ERR_NO_DEVICE = -2
PE_ERR_UNKNOWN_PARENT = -4
PE_ERR_UNKNOWN_ROOT = -9
PE_ERR_CAPACITY = -10
PE_ERR_STATE = -14
PE_ERR_TIMEOUT = -15
PE_DIST_SINGLE_COMM = 1
PE_SIG_G2_COMPRESSED, PE_SIG_G2_UNCOMPRESSED, PE_SIG_CHECK_SUBGROUP = 1, 2, 0x100
PE_SIG_STATUS_IDENTITY = 4  # pe_verify_signatures: the signature is the point at infinity
PE_BLS_INVALID, PE_BLS_VALID, PE_BLS_BAD_POINT, PE_BLS_UNDECIDED = 0, 1, 2, 3
PE_VERIFY_APPLY = 0x1  # pe_verify_resident: AND the verdict into the group's sig_valid on the device
PE_VERIFY_RESIDENT_STATS = 11
ETH2_DST = b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_"  # pe_hash_to_g2: the domain separation tag of Ethereum's signatures
NONE32 = 0xFFFFFFFF

PE_VAL_ACTIVE, PE_VAL_SLASHED, PE_VAL_EQUIVOCATING, PE_VAL_ACTIVE_PREV = 0x01, 0x02, 0x04, 0x08
PE_ATT_FLAG_SIGNATURE_VALID, PE_ATT_FLAG_FROM_BLOCK = 0x1, 0x2
PE_G1_PARTIAL_BYTES = 192
PE_EXCHANGE_EXTRA = 512
PE_DIST_ID_BYTES = 256
(PE_KERNEL_G1_ACCUMULATE, PE_KERNEL_G1_NORMALISE, PE_KERNEL_VOTES, PE_KERNEL_TREE, PE_KERNEL_LMD,
 PE_KERNEL_PARTICIPATION, PE_KERNEL_BITS_UNION, PE_KERNEL_G2_ACCUMULATE, PE_KERNEL_G2_NORMALISE,
 PE_KERNEL_G1_TREE, PE_KERNEL_ATT_GROUP, PE_KERNEL_ATT_VALIDATE, PE_KERNEL_PAIR_INGEST_VALIDATE,
 PE_KERNEL_PAIR_PLAN_LMD, PE_KERNEL_PAIR_MEMBERS_VOTES, PE_KERNEL_PAIR_UNION_TREE, PE_KERNEL_G2_DECOMPRESS,
 PE_KERNEL_COUNT) = range(18)
KERNEL_NAMES = ["g1_accumulate", "g1_normalise", "votes", "tree", "lmd", "participation", "bits_union",
                "g2_accumulate", "g2_normalise", "g1_tree", "att_group", "att_validate", "pair_ingest_validate",
                "pair_plan_lmd", "pair_members_votes", "pair_union_tree", "g2_decompress"]

ATT_STATUS_NAMES = {
    0: "ok", 1: "target epoch not current or previous", 2: "target epoch != epoch(slot)",
    3: "unknown target root", 4: "unknown beacon block root", 5: "block after attestation slot",
    6: "target not ancestor of beacon block", 7: "attestation slot not in the past", 8: "no committee table",
    9: "committee index out of range", 10: "bits length mismatch", 11: "empty or invalid indices",
    12: "bad signature", 13: "outside inclusion window", 14: "source mismatch",
    32: "slasher: target epoch in the future", 33: "slasher: target epoch left the window",
    34: "slasher: data table of the epoch is full",
}
PE_ATT_UNKNOWN_TARGET_ROOT, PE_ATT_UNKNOWN_BEACON_BLOCK_ROOT = 3, 4
PE_SLASH_FUTURE_TARGET, PE_SLASH_TOO_OLD, PE_SLASH_TABLE_FULL = 32, 33, 34
PE_SLASH_APPLY = 1
PE_SLASH_DOUBLE, PE_SLASH_SURROUND = 1, 2


class pe_config(C.Structure):
    _fields_ = [
        ("slots_per_epoch", C.c_uint64), ("seconds_per_slot", C.c_uint64), ("intervals_per_slot", C.c_uint64),
        ("safe_slots_to_update_justified", C.c_uint64), ("proposer_score_boost", C.c_uint64),
        ("effective_balance_increment", C.c_uint64), ("min_attestation_inclusion_delay", C.c_uint64),
        ("max_validators_per_committee", C.c_uint64), ("filter_slashed", C.c_uint32), ("device", C.c_int32),
        ("reserve_validators", C.c_uint64), ("reserve_blocks", C.c_uint32), ("max_committee_tables", C.c_uint32),
        ("vote_expiry_slots", C.c_uint64),
    ]


class pe_attestation(C.Structure):
    _fields_ = [
        ("slot", C.c_uint64), ("index", C.c_uint64), ("beacon_block_root", C.c_uint8 * 32),
        ("source_epoch", C.c_uint64), ("source_root", C.c_uint8 * 32),
        ("target_epoch", C.c_uint64), ("target_root", C.c_uint8 * 32),
        ("bits_offset", C.c_uint32), ("n_bits", C.c_uint32), ("flags", C.c_uint32), ("reserved0", C.c_uint32),
    ]


assert C.sizeof(pe_attestation) == 144


class pe_state_ctx(C.Structure):
    _fields_ = [
        ("slot", C.c_uint64), ("chain_tip_root", C.c_uint8 * 32),
        ("current_justified_epoch", C.c_uint64), ("current_justified_root", C.c_uint8 * 32),
        ("previous_justified_epoch", C.c_uint64), ("previous_justified_root", C.c_uint8 * 32),
        ("base_reward_per_increment", C.c_uint64),
    ]


class pe_prune_stats(C.Structure):
    """struct pe_prune_stats (include/posevo.h): what one pe_prune did."""
    _fields_ = [("blocks_before", C.c_uint32), ("blocks_after", C.c_uint32), ("votes_remapped", C.c_uint64),
                ("votes_orphaned", C.c_uint64)]


class pe_rewards_params(C.Structure):
    """struct pe_rewards_params (include/posevo.h): the constants of pe_rewards_and_penalties."""
    _fields_ = [("base_reward_factor", C.c_uint64), ("inactivity_score_bias", C.c_uint64),
                ("inactivity_score_recovery_rate", C.c_uint64), ("inactivity_penalty_quotient", C.c_uint64),
                ("min_epochs_to_inactivity_penalty", C.c_uint64)]


class pe_state_root_set(C.Structure):
    """struct pe_state_root_set (include/posevo.h): the five per-validator field roots of BeaconState."""
    _fields_ = [("balances", C.c_uint8 * 32), ("inactivity_scores", C.c_uint8 * 32),
                ("previous_epoch_participation", C.c_uint8 * 32), ("current_epoch_participation", C.c_uint8 * 32),
                ("validators", C.c_uint8 * 32)]


class pe_rewards_stats(C.Structure):
    """struct pe_rewards_stats (include/posevo.h): what one pe_rewards_and_penalties read and did."""
    _fields_ = [("total_active_balance", C.c_uint64), ("unslashed_balance", C.c_uint64 * 3), ("n_eligible", C.c_uint64),
                ("in_leak", C.c_uint64), ("rewards", C.c_uint64), ("penalties", C.c_uint64), ("n_saturated", C.c_uint64)]


class pe_registry_params(C.Structure):
    """struct pe_registry_params (include/posevo.h): the constants of pe_registry_updates."""
    _fields_ = [("max_effective_balance", C.c_uint64), ("ejection_balance", C.c_uint64), ("max_seed_lookahead", C.c_uint64),
                ("min_validator_withdrawability_delay", C.c_uint64), ("min_per_epoch_churn_limit", C.c_uint64),
                ("churn_limit_quotient", C.c_uint64), ("max_per_epoch_activation_churn_limit", C.c_uint64)]


class pe_registry_stats(C.Structure):
    """struct pe_registry_stats (include/posevo.h): what one pe_registry_updates read and did."""
    _fields_ = [("n_active", C.c_uint64), ("churn_limit", C.c_uint64), ("activation_churn_limit", C.c_uint64),
                ("n_marked_eligible", C.c_uint64), ("n_ejected", C.c_uint64), ("first_exit_epoch", C.c_uint64),
                ("last_exit_epoch", C.c_uint64), ("queue_len", C.c_uint64), ("n_activated", C.c_uint64),
                ("activation_epoch", C.c_uint64)]


class pe_slashings_stats(C.Structure):
    """struct pe_slashings_stats (include/posevo.h): what one pe_process_slashings read and did."""
    _fields_ = [("total_active_balance", C.c_uint64), ("adjusted_total_slashing_balance", C.c_uint64),
                ("n_penalised", C.c_uint64), ("penalties", C.c_uint64), ("n_saturated", C.c_uint64)]


class pe_block_op(C.Structure):
    """struct pe_block_op (include/posevo.h): one proposer slashing, attester slashing or voluntary exit, 408 bytes."""
    _fields_ = [("kind", C.c_uint32), ("flags", C.c_uint32), ("data_1", C.c_uint8 * 128), ("data_2", C.c_uint8 * 128),
                ("indices_1_offset", C.c_uint64), ("indices_1_length", C.c_uint64), ("indices_2_offset", C.c_uint64),
                ("indices_2_length", C.c_uint64), ("header_1_slot", C.c_uint64), ("header_1_proposer_index", C.c_uint64),
                ("header_1_root", C.c_uint8 * 32), ("header_2_slot", C.c_uint64), ("header_2_proposer_index", C.c_uint64),
                ("header_2_root", C.c_uint8 * 32), ("validator_index", C.c_uint64), ("exit_epoch", C.c_uint64)]


assert C.sizeof(pe_block_op) == 408


class pe_block_ops_params(C.Structure):
    """struct pe_block_ops_params (include/posevo.h): the constants of pe_process_block_operations."""
    _fields_ = [("min_slashing_penalty_quotient", C.c_uint64), ("whistleblower_reward_quotient", C.c_uint64),
                ("epochs_per_slashings_vector", C.c_uint64), ("shard_committee_period", C.c_uint64),
                ("min_validator_withdrawability_delay", C.c_uint64), ("max_seed_lookahead", C.c_uint64),
                ("min_per_epoch_churn_limit", C.c_uint64), ("churn_limit_quotient", C.c_uint64)]


class pe_block_ops_stats(C.Structure):
    """struct pe_block_ops_stats (include/posevo.h): what one pe_process_block_operations read and did."""
    _fields_ = [("n_active", C.c_uint64), ("churn_limit", C.c_uint64), ("n_slashed", C.c_uint64),
                ("n_exits_initiated", C.c_uint64), ("first_exit_epoch", C.c_uint64), ("last_exit_epoch", C.c_uint64),
                ("slashed_balance", C.c_uint64), ("proposer_rewards", C.c_uint64), ("penalties", C.c_uint64),
                ("n_saturated", C.c_uint64), ("n_invalid", C.c_uint64)]


PE_OP_PROPOSER_SLASHING, PE_OP_ATTESTER_SLASHING, PE_OP_VOLUNTARY_EXIT = 1, 2, 3
PE_OP_FLAG_SIGNATURE_VALID = 1
OP_STATUS_NAMES = {
    0: "ok", 64: "attestation data not slashable", 65: "bad indices", 66: "bad signature", 67: "nobody slashable",
    68: "header mismatch", 69: "proposer not slashable", 70: "not active", 71: "already exiting",
    72: "exit epoch in the future", 73: "too young to exit",
}


class pe_withdrawal(C.Structure):
    """struct pe_withdrawal (include/posevo.h): Withdrawal as it travels, 44 bytes packed."""
    _pack_ = 1
    _fields_ = [("index", C.c_uint64), ("validator_index", C.c_uint64), ("address", C.c_uint8 * 20), ("amount", C.c_uint64)]


assert C.sizeof(pe_withdrawal) == 44


class pe_withdrawals_params(C.Structure):
    """struct pe_withdrawals_params (include/posevo.h): the constants of pe_process_withdrawals."""
    _fields_ = [("max_effective_balance", C.c_uint64), ("max_withdrawals_per_payload", C.c_uint64),
                ("max_validators_per_sweep", C.c_uint64), ("eth1_prefix", C.c_uint64)]


class pe_withdrawals_result(C.Structure):
    """struct pe_withdrawals_result (include/posevo.h): what one pe_process_withdrawals found and did."""
    _fields_ = [("next_withdrawal_index", C.c_uint64), ("next_withdrawal_validator_index", C.c_uint64), ("n_full", C.c_uint64),
                ("n_partial", C.c_uint64), ("total_gwei", C.c_uint64), ("n_withdrawals", C.c_uint32), ("status", C.c_int32),
                ("first_mismatch", C.c_uint32), ("applied", C.c_uint32), ("withdrawals_root", C.c_uint8 * 32)]


class pe_bls_change(C.Structure):
    """struct pe_bls_change (include/posevo.h): BLSToExecutionChange and its verdict, 80 bytes."""
    _fields_ = [("validator_index", C.c_uint64), ("from_bls_pubkey", C.c_uint8 * 48), ("to_execution_address", C.c_uint8 * 20),
                ("flags", C.c_uint32)]


assert C.sizeof(pe_bls_change) == 80


class pe_bls_changes_stats(C.Structure):
    """struct pe_bls_changes_stats (include/posevo.h): what one pe_process_bls_to_execution_changes did."""
    _fields_ = [("n_applied", C.c_uint64), ("n_invalid", C.c_uint64)]


PE_WD_APPLY, PE_WD_PAYLOAD = 1, 2
PE_WD_OK, PE_WD_COUNT_MISMATCH, PE_WD_INDEX_MISMATCH, PE_WD_VALIDATOR_MISMATCH = 0, 80, 81, 82
PE_WD_ADDRESS_MISMATCH, PE_WD_AMOUNT_MISMATCH = 83, 84
WD_STATUS_NAMES = {0: "ok", 80: "count mismatch", 81: "index mismatch", 82: "validator mismatch", 83: "address mismatch",
                   84: "amount mismatch"}
PE_CRED_FLAG_SIGNATURE_VALID = 1
PE_CRED_OK, PE_CRED_BAD_INDEX, PE_CRED_NOT_BLS, PE_CRED_PUBKEY_MISMATCH, PE_CRED_BAD_SIGNATURE = 0, 96, 97, 98, 99
CRED_STATUS_NAMES = {0: "ok", 96: "bad index", 97: "not BLS credentials", 98: "pubkey mismatch", 99: "bad signature"}


class pe_deposit_data(C.Structure):
    """struct pe_deposit_data (include/posevo.h): DepositData as it travels, 184 bytes."""
    _fields_ = [("pubkey", C.c_uint8 * 48), ("withdrawal_credentials", C.c_uint8 * 32), ("amount", C.c_uint64),
                ("signature", C.c_uint8 * 96)]


class pe_deposit_params(C.Structure):
    """struct pe_deposit_params (include/posevo.h): the constants of get_validator_from_deposit."""
    _fields_ = [("effective_balance_increment", C.c_uint64), ("max_effective_balance", C.c_uint64),
                ("far_future_epoch", C.c_uint64)]


class pe_deposit_stats(C.Structure):
    """struct pe_deposit_stats (include/posevo.h): what one pe_process_deposits did."""
    _fields_ = [("n_appended", C.c_uint32), ("n_topups", C.c_uint32), ("n_ignored", C.c_uint32), ("n_bad_proof", C.c_uint32),
                ("n_validators", C.c_uint64)]


class pe_attester_domains(C.Structure):
    """struct pe_attester_domains (include/posevo.h): what get_domain(state, DOMAIN_BEACON_ATTESTER, epoch) reads, 72 bytes."""
    _fields_ = [("fork_epoch", C.c_uint64), ("domain_previous", C.c_uint8 * 32), ("domain_current", C.c_uint8 * 32)]


assert C.sizeof(pe_attester_domains) == 72

class pe_sync_aggregate(C.Structure):
    """struct pe_sync_aggregate (include/posevo.h): a block's SyncAggregate with its block root, domain and proposer, 232 bytes."""
    _fields_ = [("bits", C.c_uint8 * 64), ("signature", C.c_uint8 * 96), ("block_root", C.c_uint8 * 32), ("domain", C.c_uint8 * 32),
                ("proposer_index", C.c_uint32), ("reserved0", C.c_uint32)]


assert C.sizeof(pe_sync_aggregate) == 232


class pe_sync_params(C.Structure):
    """struct pe_sync_params (include/posevo.h): what process_sync_aggregate's scalars are made of."""
    _fields_ = [("total_active_balance", C.c_uint64), ("base_reward_factor", C.c_uint64)]


class pe_sync_stats(C.Structure):
    """struct pe_sync_stats (include/posevo.h): the scalars of one pe_process_sync_aggregate and what it did."""
    _fields_ = [("participant_reward", C.c_uint64), ("proposer_reward", C.c_uint64), ("n_participants", C.c_uint64),
                ("credited", C.c_uint64), ("debited", C.c_uint64), ("n_saturated", C.c_uint64), ("applied", C.c_uint64)]


PE_SYNC_COMMITTEE_MAX, PE_SYNC_MAX_BATCH = 512, 64
PE_SYNC_CURRENT, PE_SYNC_NEXT = 0, 1
PE_SYNC_VERIFY, PE_SYNC_APPLY = 1, 2
PE_DEP_APPENDED, PE_DEP_TOPUP, PE_DEP_IGNORED_BAD_SIGNATURE, PE_DEP_BAD_PROOF = 0, 1, 2, 3
PE_REWARDS_INACTIVITY, PE_REWARDS_DELTAS = 1, 2
PE_ROOT_BALANCES, PE_ROOT_INACTIVITY, PE_ROOT_PART_PREV, PE_ROOT_PART_CUR, PE_ROOT_VALIDATORS = 1, 2, 4, 8, 16

_P = C.POINTER
# Buffer arguments are declared void*: the wrappers pass raw addresses (engine._ptr), which costs 0.5 us per argument
# against 2.8 us for ndarray.ctypes.data_as -- some twenty pointers cross the boundary per step.
_u8p = _u32p = _u64p = _i32p = _attp = C.c_void_p
_H = C.c_void_p

# name -> (restype, argtypes); every symbol include/posevo.h declares
ALL_REDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p)
ALL_GATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p)


class pe_collectives(C.Structure):
    """struct pe_collectives (include/posevo.h): the caller's collectives for pe_dist_init_custom."""
    _fields_ = [("user", C.c_void_p), ("all_reduce_u64", ALL_REDUCE_FN), ("all_gather", ALL_GATHER_FN)]


SIGNATURES = {
    "pe_abi_version": (C.c_uint32, []),
    "pe_config_default": (None, [_P(pe_config)]),
    "pe_engine_create": (C.c_int, [_P(pe_config), _P(_H)]),
    "pe_engine_destroy": (None, [_H]),
    "pe_strerror": (C.c_char_p, [C.c_int]),
    "pe_last_error": (C.c_char_p, [_H]),
    "pe_set_stream": (C.c_int, [_H, C.c_void_p]),
    "pe_store_init": (C.c_int, [_H, C.c_uint64, C.c_uint64, _u8p]),
    "pe_set_validators": (C.c_int, [_H, C.c_uint64, _u8p, _u64p, _u8p]),
    "pe_set_balances": (C.c_int, [_H, C.c_uint64, _u64p, _u8p]),
    "pe_on_tick": (C.c_int, [_H, C.c_uint64]),
    "pe_on_block": (C.c_int, [_H, _u8p, _u8p, C.c_uint64, C.c_uint64, _u8p, C.c_uint64, _u8p]),
    "pe_add_block": (C.c_int, [_H, _u8p, _u8p, C.c_uint64, C.c_uint64, _u8p, C.c_uint64, _u8p]),
    "pe_set_checkpoints": (C.c_int, [_H, C.c_uint64, _u8p, C.c_uint64, _u8p]),
    "pe_set_proposer_boost": (C.c_int, [_H, _u8p]),
    "pe_mark_equivocating": (C.c_int, [_H, _u64p, C.c_uint64]),
    "pe_on_attester_slashing": (C.c_int, [_H, _attp, _u64p, C.c_uint64, _attp, _u64p,
                                          C.c_uint64]),
    "pe_set_committees": (C.c_int, [_H, C.c_uint64, C.c_uint32, _u32p, _u32p]),
    "pe_compute_committees": (C.c_int, [_H, C.c_uint64, _u8p, _u32p, C.c_uint32, C.c_uint32, C.c_uint32, _u32p, _u32p]),
    "pe_compute_committees_async": (C.c_int, [_H, C.c_uint64, _u8p, _u32p, C.c_uint32, C.c_uint32, C.c_uint32]),
    "pe_get_head": (C.c_int, [_H, _u8p]),
    "pe_get_head_async": (C.c_int, [_H, _u8p]),
    "pe_aggregate_signed": (C.c_int, [_H, _attp, C.c_uint32, _u8p, C.c_uint64, _u8p, C.c_uint32, _attp, _u32p, _u32p, _u8p,
                                      C.c_uint64, _u8p, _i32p, _u8p, _u32p]),
    "pe_g2_subgroup_check": (C.c_int, [_H, _u8p, C.c_uint64, _i32p]),
    "pe_pairing_check": (C.c_int, [_H, _u8p, _u8p, C.c_uint64, _u32p, C.c_uint32, _i32p]),
    "pe_fast_aggregate_verify": (C.c_int, [_H, _u32p, _u32p, C.c_uint32, _u8p, _u8p, _i32p]),
    "pe_batch_verify": (C.c_int, [_H, _u8p, _u8p, _u8p, C.c_uint32, _u64p, _i32p]),
    "pe_batch_fast_aggregate_verify": (C.c_int, [_H, _u32p, _u32p, C.c_uint32, _u8p, _u8p, _u64p, _i32p]),
    "pe_verify_signatures": (C.c_int, [_H, C.c_void_p, C.c_uint64, _u32p, _u32p, _u32p, C.c_uint32, _u8p, _u64p, _i32p, _i32p, _i32p,
                                       _u8p]),
    "pe_verify_resident": (C.c_int, [_H, C.c_void_p, C.c_uint32, _u32p, C.c_uint32, C.c_uint32, _i32p]),
    "pe_pipeline_set_lag": (C.c_int, [_H, C.c_uint32]),
    "pe_pipeline_get_lag": (C.c_uint32, [_H]),
    "pe_pipeline_generation": (C.c_uint64, [_H]),
    "pe_pipeline_completed": (C.c_uint64, [_H]),
    "pe_get_weights": (C.c_int, [_H, _u64p, C.c_uint32]),
    "pe_on_attestation_batch": (C.c_int, [_H, _attp, C.c_uint32, _u8p, C.c_uint64, _i32p, _u8p, _u32p]),
    "pe_get_indexed_attestations": (C.c_int, [_H, _attp, C.c_uint32, _u8p, C.c_uint64, _i32p, _u32p, _u32p,
                                              C.c_uint64]),
    "pe_aggregate": (C.c_int, [_H, _attp, C.c_uint32, _u8p, C.c_uint64, _u8p, _attp,
                               _u32p, _u32p, _u8p, C.c_uint64, _u8p, _u8p, _u32p]),
    "pe_process_attestation_batch": (C.c_int, [_H, _P(pe_state_ctx), _attp, C.c_uint32, _u8p,
                                               C.c_uint64, _i32p, _u64p]),
    "pe_participation_set": (C.c_int, [_H, C.c_int, _u8p, C.c_uint64]),
    "pe_participation_get": (C.c_int, [_H, C.c_int, _u8p, C.c_uint64]),
    "pe_participation_rotate": (C.c_int, [_H]),
    "pe_state_set_validators": (C.c_int, [_H, C.c_uint64, _u64p, _u8p]),
    "pe_state_get_validators": (C.c_int, [_H, C.c_uint64, _u64p, _u8p, C.c_void_p]),
    "pe_get_committee_epochs": (C.c_int, [_H, _u64p, C.c_uint32, _u32p]),
    "pe_get_committees": (C.c_int, [_H, C.c_uint64, _u32p, _u32p, C.c_uint32, _u32p, C.c_uint64]),
    "pe_ffg_balances": (C.c_int, [_H, _u64p]),
    "pe_compute_proposers": (C.c_int, [_H, _u8p, C.c_uint32, _u32p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, _u32p,
                                       _u32p]),
    "pe_effective_balance_updates": (C.c_int, [_H, C.c_uint64, _u64p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, _u64p,
                                               _u64p]),
    "pe_registry_set_epochs": (C.c_int, [_H, C.c_uint64, _u64p, _u64p]),
    "pe_registry_get_epochs": (C.c_int, [_H, C.c_uint64, _u64p, _u64p, C.c_void_p]),
    "pe_active_set": (C.c_int, [_H, C.c_uint64, C.c_void_p, C.c_void_p, _u32p]),
    "pe_state_refresh_activity": (C.c_int, [_H, C.c_uint64]),
    "pe_state_set_balances": (C.c_int, [_H, C.c_uint64, _u64p, _u64p, _u64p]),
    "pe_state_get_balances": (C.c_int, [_H, C.c_uint64, _u64p, _u64p, _u64p, C.c_void_p]),
    "pe_rewards_params_default": (None, [_P(pe_rewards_params)]),
    "pe_rewards_and_penalties": (C.c_int, [_H, C.c_uint64, C.c_uint64, _P(pe_rewards_params), C.c_uint32,
                                           _P(pe_rewards_stats)]),
    "pe_registry_params_default": (None, [_P(pe_registry_params)]),
    "pe_registry_updates": (C.c_int, [_H, C.c_uint64, C.c_uint64, _P(pe_registry_params), _P(pe_registry_stats)]),
    "pe_process_slashings": (C.c_int, [_H, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, _P(pe_slashings_stats)]),
    "pe_block_ops_params_default": (None, [_P(pe_block_ops_params)]),
    "pe_process_block_operations": (C.c_int, [_H, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32, _u32p, C.c_uint64,
                                              _P(pe_block_ops_params), _i32p, _P(pe_block_ops_stats)]),
    "pe_withdrawals_params_default": (None, [_P(pe_withdrawals_params)]),
    "pe_process_withdrawals": (C.c_int, [_H, C.c_uint64, C.c_uint64, C.c_uint64, _P(pe_withdrawals_params), C.c_void_p,
                                         C.c_uint32, C.c_uint32, C.c_void_p, _P(pe_withdrawals_result)]),
    "pe_process_bls_to_execution_changes": (C.c_int, [_H, C.c_void_p, C.c_uint32, _i32p, _P(pe_bls_changes_stats)]),
    "pe_bls_change_signing_roots": (C.c_int, [_H, C.c_void_p, C.c_uint32, _u8p, _u8p]),
    "pe_registry_set_static": (C.c_int, [_H, C.c_uint64, _u8p, _u8p, _u64p]),
    "pe_registry_get_static": (C.c_int, [_H, C.c_uint64, _u8p, _u8p, _u64p, C.c_void_p]),
    "pe_state_roots": (C.c_int, [_H, C.c_uint32, C.c_uint32, _P(pe_state_root_set), _u8p]),
    "pe_ssz_merkleize": (C.c_int, [_H, _u8p, C.c_uint64, C.c_uint32, C.c_int64, _u8p]),
    "pe_deposit_params_default": (None, [_P(pe_deposit_params)]),
    "pe_deposit_signing_roots": (C.c_int, [_H, _u8p, C.c_uint32, _u8p, _u8p]),
    "pe_process_deposits": (C.c_int, [_H, _u8p, C.c_uint32, _u8p, C.c_uint64, _u8p, _u8p, _P(pe_deposit_params), _i32p, _u32p,
                                      _P(pe_deposit_stats)]),
    "pe_hash_to_g2": (C.c_int, [_H, _u8p, C.c_uint32, C.c_uint32, _u8p, C.c_uint32, _u8p, _i32p]),
    "pe_map_to_g2": (C.c_int, [_H, _u8p, C.c_uint32, _u8p]),
    "pe_attestation_signing_roots": (C.c_int, [_H, _attp, C.c_uint32, _P(pe_attester_domains), _u8p]),
    "pe_verify_resident_data": (C.c_int, [_H, _P(pe_attester_domains), C.c_uint32, C.c_uint32, _i32p, _u8p]),
    "pe_sync_committee_compute": (C.c_int, [_H, _u8p, _u32p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, _u32p, _u8p,
                                            C.c_void_p]),
    "pe_sync_committee_set": (C.c_int, [_H, C.c_int, _u32p, C.c_uint32]),
    "pe_sync_committee_get": (C.c_int, [_H, C.c_int, _u32p, C.c_uint32, C.c_void_p, _u8p]),
    "pe_sync_committee_rotate": (C.c_int, [_H]),
    "pe_sync_params_default": (None, [_P(pe_sync_params)]),
    "pe_process_sync_aggregate": (C.c_int, [_H, _u8p, C.c_uint32, _P(pe_sync_params), C.c_uint32, _i32p, _i32p, _P(pe_sync_stats)]),
    "pe_g1_sum": (C.c_int, [_H, _u8p, C.c_uint64, _u32p, _u32p, C.c_uint32, _u8p]),
    "pe_prune": (C.c_int, [_H, C.c_void_p]),
    "pe_set_block_checkpoints": (C.c_int, [_H, C.c_uint32, C.c_uint64, _u8p, C.c_uint64, _u8p]),
    "pe_get_block": (C.c_int, [_H, C.c_uint32, _u8p, _u32p, _u64p, _u64p, _u8p, _u64p, _u8p]),
    "pe_get_validator_flags": (C.c_int, [_H, _u8p, C.c_uint64]),
    "pe_get_latest_message_slots": (C.c_int, [_H, _u32p, C.c_uint64]),
    "pe_set_latest_messages": (C.c_int, [_H, C.c_uint64, _u64p, _u32p, _u32p]),
    "pe_set_best_justified": (C.c_int, [_H, C.c_uint64, _u8p]),
    "pe_g1_key_validate": (C.c_int, [_H, _u8p, C.c_uint64, _i32p]),
    "pe_g1_decompress": (C.c_int, [_H, _u8p, C.c_uint64, _u8p, _i32p]),
    "pe_set_pubkeys_compressed": (C.c_int, [_H, C.c_uint64, _u8p, _i32p]),
    "pe_g1_compress": (C.c_int, [_u8p, C.c_uint64, _u8p]),
    "pe_g2_decompress": (C.c_int, [_H, _u8p, C.c_uint64, _u8p, _i32p]),
    "pe_g2_compress": (C.c_int, [_u8p, C.c_uint64, _u8p]),
    "pe_g2_sum": (C.c_int, [_H, _u8p, C.c_uint64, _u32p, _u32p, C.c_uint32, _u8p]),
    "pe_aggregate_signatures": (C.c_int, [_H, C.c_void_p, C.c_uint64, C.c_void_p, _u32p, C.c_uint32, C.c_uint32, _u8p, _i32p,
                                         _u32p]),
    "pe_num_blocks": (C.c_uint32, [_H]),
    "pe_num_validators": (C.c_uint64, [_H]),
    "pe_block_root_at": (C.c_int, [_H, C.c_uint32, _u8p]),
    "pe_block_index_of": (C.c_int, [_H, _u8p, _u32p]),
    "pe_get_latest_messages": (C.c_int, [_H, _u64p, _u32p, C.c_uint64]),
    "pe_get_store_scalars": (C.c_int, [_H, _u64p, _u64p, _u64p, _u8p, _u64p, _u8p, _u64p, _u8p, _u8p]),
    "pe_votes_partial": (C.c_int, [_H, C.c_void_p, C.c_uint32]),
    "pe_head_from_weights": (C.c_int, [_H, C.c_void_p, C.c_uint32, _u8p]),
    "pe_aggregate_partial": (C.c_int, [_H, _attp, C.c_uint32, _u8p, C.c_uint64, _attp,
                                       _u32p, _u32p, _u8p, C.c_uint64, _u32p, C.c_void_p, C.c_uint32]),
    "pe_g1_partial": (C.c_int, [_H, _u32p, _u32p, C.c_uint32, C.c_void_p, C.c_uint32]),
    "pe_get_last_weights": (C.c_int, [_H, _u64p, C.c_uint32]),
    "pe_g1_finish": (C.c_int, [_H, C.c_void_p, C.c_uint32, C.c_uint32, _u8p]),
    "pe_dist_unique_id": (C.c_int, [_u8p]),
    "pe_dist_init": (C.c_int, [_H, _u8p, C.c_int, C.c_int]),
    "pe_dist_destroy": (C.c_int, [_H]),
    "pe_dist_init_ex": (C.c_int, [_H, _u8p, C.c_int, C.c_int, C.c_uint32]),
    "pe_dist_init_custom": (C.c_int, [_H, C.c_int, C.c_int, C.c_void_p]),
    "pe_dist_set_timeout_ms": (C.c_int, [_H, C.c_uint32]),
    "pe_dist_set_max_groups": (C.c_int, [_H, C.c_uint32]),
    "pe_aggregate_exchange": (C.c_int, [_H, _attp, _u32p, _u8p, C.c_uint64, _u32p, C.c_uint32]),
    "pe_get_head_sharded": (C.c_int, [_H, _u8p]),
    "pe_get_head_sharded_async": (C.c_int, [_H, _u8p]),
    "pe_aggregate_sharded": (C.c_int, [_H, _attp, C.c_uint32, _u8p, C.c_uint64, _attp, _u32p, _u32p, _u8p,
                                       C.c_uint64, _u8p, _u32p]),
    "pe_slasher_enable": (C.c_int, [_H, C.c_uint32, C.c_uint32]),
    "pe_slasher_disable": (C.c_int, [_H]),
    "pe_slasher_ingest": (C.c_int, [_H, _attp, C.c_uint32, _u8p, C.c_uint64, C.c_uint64, C.c_uint32, _i32p, C.c_void_p,
                                    C.c_uint32, _u32p]),
    "pe_slasher_get_data": (C.c_int, [_H, C.c_uint64, C.c_uint32, _attp]),
    "pe_slasher_get_records": (C.c_int, [_H, C.c_uint64, _u32p, _u32p, C.c_uint64]),
    "pe_pipeline_begin": (C.c_int, [_H]),
    "pe_pipeline_end": (C.c_int, [_H]),
    "pe_pipeline_end_lagged": (C.c_int, [_H]),
    "pe_pipeline_begin_streaming": (C.c_int, [_H]),
    "pe_profile_enable": (C.c_int, [_H, C.c_int]),
    "pe_profile_reset": (C.c_int, [_H]),
    "pe_profile_get": (C.c_int, [_H, C.c_int, _u64p, _P(C.c_double)]),
    "pe_profile_timeline": (C.c_int, [_H, _i32p, C.c_void_p, C.c_void_p, C.c_uint32, _P(C.c_uint32)]),
    "pe_profile_queue_classes": (C.c_int, [_H, _i32p]),
    "pe_profile_arena_growths": (C.c_int, [_H, _P(C.c_uint64)]),
    "pe_profile_committee_sums": (C.c_int, [_H, _P(C.c_uint32), _P(C.c_uint32)]),
    "pe_profile_accumulate_mhz": (C.c_int, [_H, C.c_void_p, C.c_uint32, _P(C.c_uint32)]),
    "pe_profile_pairing_gt": (C.c_int, [_H, _u8p, _u8p, C.c_uint64, _u32p, C.c_uint32, _u8p]),
    "pe_profile_batch_set_chunk": (C.c_int, [_H, C.c_uint32]),
    "pe_profile_batch_stats": (C.c_int, [_H, _u32p]),
    "pe_profile_batch_gt": (C.c_int, [_H, _u8p]),
    "pe_profile_verify_set_stripe": (C.c_int, [_H, C.c_uint32]),
    "pe_profile_verify_stats": (C.c_int, [_H, _u32p]),
    "pe_profile_deposit_index": (C.c_int, [_H, _u32p, _u64p, C.c_void_p]),
    "pe_profile_verify_sums": (C.c_int, [_H, C.c_uint32, _u8p, _u8p]),
    "pe_profile_verify_resident_stats": (C.c_int, [_H, _u32p]),
}

PE_ROWS_RESIDENT = 1  # include/posevo.h: "every group of the last pe_aggregate over rows in device memory"
PE_BITS_RESIDENT = 1  # the address include/posevo.h defines as "bits are where the last pe_aggregate left them"
PE_ACTIVE_RESIDENT = 1  # ... and as "the active list is where the last pe_active_set left it"
PE_BALANCES_RESIDENT = 1  # ... and as "the balances are where pe_state_set_balances / pe_rewards_and_penalties left them"
PE_ATT_FLAG_OVERLAPPING_BITS = 0x4
PE_VOTE_PRUNED = 0xFFFFFFFE  # block index of a latest message whose block pe_prune removed (its epoch is kept)

_lib = None


def load():
    """dlopen libposevo.so and attach the signatures.  Raises if the library is absent:
    the product path has no CPU fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback."
        )
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the header and the library disagree
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
