"""Host-side mirror of the reference's fork-choice / attestation interface, backed by the
MI355X engine through the C ABI.

Same names, argument meaning and error behaviour as the pyspec excerpts in
pos-evolution.md (``pe:N``):

    get_forkchoice_store(anchor_state, anchor_block)        pe:1077-1095
    on_tick(store, time)                                    pe:934-955
    on_block(store, signed_block, post_state)               pe:986-1036   (state_transition is the caller's)
    on_attestation(store, attestation, is_from_block=False) pe:963-979, pe:1423-1428
    on_attester_slashing(store, attester_slashing)          pe:1447-1461
    find_attester_slashings(store, attestations)            pe:1128, pe:1134-1143 (the detection the handlers presume)
    get_head(store) -> Root                                 pe:1102-1116
    prune(store)                                            -- (not in the reference: its Store never forgets a block)
    process_attestation(state, attestation)                 pe:722-754    (state bound with bind_state)
    compute_proposer_index(state, indices, seed)            pe:604-618    (state bound with bind_state)
    process_effective_balance_updates(state)                pe:122-133    (state bound with bind_state)
    process_inactivity_updates(state)                       Altair; fields pe:368-369 (state bound with bind_state)
    process_rewards_and_penalties(state)                    Altair; fields pe:112, pe:45 (state bound with bind_state)
    process_registry_updates(state)                         fields pe:36-45; churn limit pe:1261 (state bound with bind_state)
    process_slashings(state)                                fields pe:359/397 (state bound with bind_state)
    process_proposer_slashing(state, proposer_slashing)     fields pe:36-45, pe:359/397 (state bound with bind_state)
    process_attester_slashing(state, attester_slashing)     pe:1134-1143 and the same fields (state bound with bind_state)
    process_voluntary_exit(state, signed_voluntary_exit)    fields pe:43-45 (state bound with bind_state)
    attester_slashing_ops_from_evidence(evidence)           find_attester_slashings' output as operations of the three above
    get_active_validator_indices(state, epoch)              named at pe:467 (state bound with bind_state)
    get_committee_count_per_slot(state, epoch)              pe:461-468
    compute_weak_subjectivity_period(state)                 pe:1257-1287
    get_latest_weak_subjectivity_checkpoint_epoch(state)    pe:1225-1241
    is_within_weak_subjectivity_period(...)                 pe:1298-1301  (the final comparison)

Objects are duck-typed: anything exposing the pyspec's field names works
(``attestation.data.beacon_block_root``, ``attestation.aggregation_bits``,
``state.validators[i].effective_balance`` ...).  A failed handler raises
``AssertionError`` (``EngineError``) and leaves the store unmodified (pe:1041).

Out of scope and therefore supplied by the caller: SSZ
``hash_tree_root`` (pass the function), ``state_transition`` (pass the post-state),
committee shuffling (pass the committees), the pairing check (its boolean rides on
``attestation.signature_valid``, default True).

This module performs no arithmetic of the hot path itself and never imports the
oracle: without libposevo.so + a HIP device it raises.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, Iterable, List, Optional, Sequence

import numpy as np

from . import _abi
from .engine import (ROWS_RESIDENT, AttRow, Engine, EngineError, ZERO_ROOT, attester_slashing_op, proposer_slashing_op,
                     voluntary_exit_op)
from ._abi import pe_state_ctx

GENESIS_EPOCH = 0
PARTICIPATION_FLAG_WEIGHTS = [14, 26, 14]
PROPOSER_WEIGHT = 8
WEIGHT_DENOMINATOR = 64


@dataclass(eq=True, frozen=True)
class Checkpoint:
    """pe:219-221"""
    epoch: int = 0
    root: bytes = ZERO_ROOT


@dataclass(eq=True, frozen=True)
class LatestMessage:
    """pe:286-289"""
    epoch: int
    root: bytes


def _att_row(attestation, is_from_block: bool = False) -> AttRow:
    d = attestation.data
    return AttRow(
        slot=int(d.slot), index=int(d.index), beacon_block_root=bytes(d.beacon_block_root),
        source_epoch=int(d.source.epoch), source_root=bytes(d.source.root),
        target_epoch=int(d.target.epoch), target_root=bytes(d.target.root),
        bits=np.asarray(attestation.aggregation_bits, dtype=np.uint8),
        signature_valid=bool(getattr(attestation, "signature_valid", True)),
        is_from_block=is_from_block,
    )


class Store:
    """Engine-backed ``Store`` (pe:889-901).  Scalars live in the engine; this object exposes them
    under the pyspec's attribute names."""

    def __init__(self, engine: Engine, hash_tree_root: Optional[Callable] = None):
        self.engine = engine
        self.hash_tree_root = hash_tree_root
        self.equivocating_indices = set()   # host mirror of pe:897 (the engine holds the per-validator bit)
        self.blocks: Dict[bytes, object] = {}  # root -> the caller's block object (pe:898)
        # get_latest_attesting_balance reads checkpoint_states[store.justified_checkpoint] on EVERY call (Appendix A.1);
        # the engine holds ONE registry view.  Which checkpoint it belongs to is tracked here, and get_head refuses
        # to weigh votes with another checkpoint's balances (on_block / on_tick / set_checkpoints can move
        # justified_checkpoint).  checkpoint_state_provider(checkpoint) -> state, when set, is asked for the missing
        # state instead (a client has it materialised by the time the checkpoint is justified).
        self.balances_checkpoint: Optional[Checkpoint] = None
        self.checkpoint_state_provider: Optional[Callable] = None

    # -- the spec's fields ---------------------------------------------------
    @property
    def time(self) -> int:
        return self.engine.store_scalars()["time"]

    @property
    def genesis_time(self) -> int:
        return self.engine.store_scalars()["genesis_time"]

    @property
    def justified_checkpoint(self) -> Checkpoint:
        return Checkpoint(*self.engine.store_scalars()["justified"])

    @property
    def finalized_checkpoint(self) -> Checkpoint:
        return Checkpoint(*self.engine.store_scalars()["finalized"])

    @property
    def best_justified_checkpoint(self) -> Checkpoint:
        return Checkpoint(*self.engine.store_scalars()["best_justified"])

    @property
    def proposer_boost_root(self) -> bytes:
        return self.engine.store_scalars()["proposer_boost_root"]

    @proposer_boost_root.setter
    def proposer_boost_root(self, root: bytes):
        self.engine.set_proposer_boost(bytes(root))

    @property
    def latest_messages(self) -> Dict[int, LatestMessage]:
        epoch, block = self.engine.latest_messages()
        roots = [self.engine.block_root_at(i) for i in range(self.engine.num_blocks)]
        # a message whose block ``prune`` removed keeps its epoch; its root is gone and reads as the unset root
        return {int(i): LatestMessage(int(epoch[i]), roots[int(block[i])] if block[i] != _abi.PE_VOTE_PRUNED else ZERO_ROOT)
                for i in np.nonzero(block != _abi.NONE32)[0]}

    # -- inputs the pyspec derives from states the engine does not hold -----------
    def ensure_justified_state(self):
        """The engine's balances must be those of checkpoint_states[justified_checkpoint] (A.1)."""
        jc = self.justified_checkpoint
        if self.balances_checkpoint == jc:
            return
        if self.checkpoint_state_provider is not None:
            self.set_justified_state(self.checkpoint_state_provider(jc))
            return
        raise EngineError(_abi.PE_ERR_STATE,
                          f"justified checkpoint moved to epoch {jc.epoch} but the engine still holds the balances of "
                          f"{self.balances_checkpoint}: call store.set_justified_state(checkpoint_states[justified_checkpoint]) "
                          "or set store.checkpoint_state_provider")

    def set_justified_state(self, state, slots_per_epoch: Optional[int] = None):
        """checkpoint_states[justified_checkpoint] (Appendix A.1): balances/activity feeding the weights,
        and the pubkeys feeding the G1 sums.  Records that the engine's view now belongs to the store's current
        justified checkpoint."""
        spe = slots_per_epoch or int(self.engine.cfg.slots_per_epoch)
        epoch = int(state.slot) // spe
        n = len(state.validators)
        bal = np.fromiter((int(v.effective_balance) for v in state.validators), dtype=np.uint64, count=n)
        flags = np.fromiter(
            ((_abi.PE_VAL_ACTIVE if int(v.activation_epoch) <= epoch < int(v.exit_epoch) else 0)
             | (_abi.PE_VAL_SLASHED if v.slashed else 0) for v in state.validators), dtype=np.uint8, count=n)
        pk = pk48 = None
        if n and all(getattr(v, "pubkey", None) is not None for v in state.validators):
            if all(isinstance(v.pubkey, (bytes, bytearray)) and len(v.pubkey) == 48 for v in state.validators):
                # the pyspec's own type: BLSPubkey = 48-byte compressed (pe:37); decompressed on the GPU
                pk48 = np.frombuffer(b"".join(bytes(v.pubkey) for v in state.validators), dtype=np.uint8)
            else:
                pk = np.frombuffer(b"".join(_point96(v.pubkey) for v in state.validators), dtype=np.uint8)
        if self.engine.num_validators == n and pk is None and pk48 is None:
            self.engine.set_balances(bal, flags)
        else:
            self.engine.set_validators(bal, flags, pk)
            if pk48 is not None:
                self.engine.set_pubkeys_compressed(pk48)
        self.balances_checkpoint = self.justified_checkpoint

    def set_committees(self, epoch: int, committees: Sequence[Sequence[int]]):
        """get_beacon_committee(state, slot, index) for every (slot, index) of ``epoch``, in committee-id
        order (slot-major): the L2 feeder's output (compute_committee, pe:495-504)."""
        sizes = np.fromiter((len(c) for c in committees), dtype=np.uint32, count=len(committees))
        offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
        members = (np.concatenate([np.asarray(c, dtype=np.uint32) for c in committees])
                   if len(committees) else np.zeros(0, dtype=np.uint32))
        self.engine.set_committees(epoch, offsets, members)


    def compute_committees(self, epoch: int, seed: bytes, active_indices: Sequence[int], committees_per_slot: int,
                           shuffle_round_count: int = 90):
        """The same table computed on the GPU from get_seed(state, epoch, DOMAIN_BEACON_ATTESTER) (pe:481-486)
        and get_active_validator_indices(state, epoch): compute_committee over compute_shuffled_index
        (pe:495-534).  Store method so that the client no longer runs the shuffle itself."""
        n = int(self.engine.cfg.slots_per_epoch) * committees_per_slot
        return self.engine.compute_committees(epoch, bytes(seed), active_indices, n, shuffle_round_count)


def _point96(pt) -> bytes:
    """Affine (x, y) int tuple / None / 96 raw bytes -> 96-byte uncompressed encoding."""
    if isinstance(pt, (bytes, bytearray)):
        assert len(pt) == 96
        return bytes(pt)
    if pt is None:
        return bytes([0x40]) + bytes(95)
    x, y = pt
    return int(x).to_bytes(48, "big") + int(y).to_bytes(48, "big")


# ----------------------------------------------------------------------------- handlers
def get_forkchoice_store(anchor_state, anchor_block, *, hash_tree_root: Callable, engine: Optional[Engine] = None,
                         **engine_config) -> Store:
    """pe:1077-1095"""
    assert bytes(anchor_block.state_root) == bytes(hash_tree_root(anchor_state))
    anchor_root = bytes(hash_tree_root(anchor_block))
    eng = engine or Engine(**engine_config)
    eng.store_init(int(anchor_state.genesis_time), int(anchor_state.slot), anchor_root)
    store = Store(eng, hash_tree_root)
    store.blocks[anchor_root] = anchor_block
    store.set_justified_state(anchor_state)  # checkpoint_states = {justified_checkpoint: anchor_state}
    return store


def on_tick(store: Store, time: int) -> None:
    """pe:934-955"""
    store.engine.on_tick(int(time))


def on_block(store: Store, signed_block, post_state) -> None:
    """pe:986-1036.  ``post_state`` = the block's post-state as computed by the caller's
    ``state_transition`` (pe:1009); only its two checkpoints are read."""
    block = signed_block.message
    root = bytes(store.hash_tree_root(block))
    j, f = post_state.current_justified_checkpoint, post_state.finalized_checkpoint
    store.engine.on_block(root, bytes(block.parent_root), int(block.slot), (int(j.epoch), bytes(j.root)),
                          (int(f.epoch), bytes(f.root)))
    store.blocks[root] = block


def on_attestation(store: Store, attestation, is_from_block: bool = False) -> None:
    """pe:963-979 with the ``is_from_block`` form of pe:1423-1428."""
    status, _, _ = store.engine.on_attestation_batch([_att_row(attestation, is_from_block)])
    if status[0] != 0:
        raise EngineError(int(status[0]), "on_attestation: " + _abi.ATT_STATUS_NAMES.get(int(status[0]), "?"))


def on_attestations(store: Store, attestations: Iterable, is_from_block: bool = False) -> np.ndarray:
    """Batch form: ``on_attestation`` x n applied as if sequentially; returns the per-attestation status
    (0 = applied) instead of raising on the first invalid one."""
    rows = [_att_row(a, is_from_block) for a in attestations]
    status, _, _ = store.engine.on_attestation_batch(rows)
    return status


def on_attester_slashing(store: Store, attester_slashing) -> None:
    """pe:1447-1461"""
    a1, a2 = attester_slashing.attestation_1, attester_slashing.attestation_2

    def row(ia):
        d = ia.data
        return AttRow(int(d.slot), int(d.index), bytes(d.beacon_block_root), int(d.source.epoch), bytes(d.source.root),
                      int(d.target.epoch), bytes(d.target.root), np.zeros(0, dtype=np.uint8),
                      bool(getattr(ia, "signature_valid", True)))

    store.engine.on_attester_slashing(row(a1), list(a1.attesting_indices), row(a2), list(a2.attesting_indices))
    store.equivocating_indices |= set(a1.attesting_indices).intersection(a2.attesting_indices)


@dataclass(eq=True, frozen=True)
class AttestationData:
    """pe:689-697"""
    slot: int
    index: int
    beacon_block_root: bytes
    source: Checkpoint
    target: Checkpoint


@dataclass
class IndexedAttestation:
    """Appendix A.6; ``signature_valid`` is the injected verdict of the pairing check, as on every attestation here."""
    attesting_indices: List[int]
    data: AttestationData
    signature: object = None
    signature_valid: bool = True


@dataclass
class AttesterSlashing:
    """pe:1159-1162"""
    attestation_1: IndexedAttestation
    attestation_2: IndexedAttestation


def find_attester_slashings(store: Store, attestations: Iterable, *, apply: bool = False,
                            cap: Optional[int] = None, cap_rows: int = 0) -> List[AttesterSlashing]:
    """The double and surround votes (pe:1128) that ``attestations`` hold against what their validators attested before,
    found on the GPU (Engine.slasher_enable first): one AttesterSlashing per slashable pair of AttestationData
    (is_slashable_attestation_data(d1, d2), pe:1134-1143, in the argument order on_attester_slashing accepts), the sorted
    validators that signed both as ``attesting_indices`` of both sides.  The history is that of the engine's window as of
    get_current_slot(store); the attestations join it.  ``cap`` bounds the pieces of evidence read back (default: four
    per set bit); more than that raises -- the history has moved on by then, so size it generously.
    ``attestations=(ROWS_RESIDENT, RESIDENT), cap_rows=c``: every group of the engine's last aggregate over DeviceRows
    (c >= the groups formed; ``cap`` then defaults to 65536)."""
    eng = store.engine
    resident = isinstance(attestations, tuple) and len(attestations) == 2 and attestations[0] is ROWS_RESIDENT
    rows = [] if resident else [_att_row(a) for a in attestations]
    sc = eng.store_scalars()
    spe, sps = int(eng.cfg.slots_per_epoch), int(eng.cfg.seconds_per_slot)
    current_epoch = (sc["time"] - sc["genesis_time"]) // sps // spe
    if cap is None:
        cap = 1 << 16 if resident else 4 * sum(int(np.count_nonzero(r.bits)) for r in rows) + 1024
    if resident:
        _, evidence = eng.slasher_ingest(packed=attestations, cap_rows=cap_rows, current_epoch=current_epoch, apply=apply, cap=cap)
    else:
        _, evidence = eng.slasher_ingest(rows, current_epoch=current_epoch, apply=apply, cap=cap)
    if eng.slasher_found > len(evidence):
        raise EngineError(_abi.PE_ERR_CAPACITY, f"find_attester_slashings: {eng.slasher_found} pieces of evidence, cap {cap}")
    pairs: Dict[tuple, List[int]] = {}
    for ev in evidence:
        key = (int(ev["target_epoch_1"]), int(ev["id_1"]), int(ev["target_epoch_2"]), int(ev["id_2"]))
        pairs.setdefault(key, []).append(int(ev["validator"]))

    def data(epoch, data_id):
        r = eng.slasher_data(epoch, data_id)
        return AttestationData(int(r["slot"]), int(r["index"]), r["beacon_block_root"].tobytes(),
                               Checkpoint(int(r["source_epoch"]), r["source_root"].tobytes()),
                               Checkpoint(int(r["target_epoch"]), r["target_root"].tobytes()))

    out = []
    for (e1, i1, e2, i2), validators in sorted(pairs.items()):
        idx = sorted(set(validators))
        out.append(AttesterSlashing(IndexedAttestation(list(idx), data(e1, i1)), IndexedAttestation(list(idx), data(e2, i2))))
    if apply:
        store.equivocating_indices |= {v for s_ in out for v in s_.attestation_1.attesting_indices}
    return out


def get_indexed_attestation(store: Store, attestation):
    """get_indexed_attestation(state, attestation) (Appendix A.6): the sorted attesting indices, resolved against the
    committee table of the attestation's target epoch on the GPU.  Returns (attesting_indices, data, signature)."""
    status, offsets, indices = store.engine.get_indexed_attestations([_att_row(attestation)])
    if status[0] != 0:
        raise EngineError(int(status[0]), "get_indexed_attestation: " + _abi.ATT_STATUS_NAMES.get(int(status[0]), "?"))
    return [int(i) for i in indices], attestation.data, getattr(attestation, "signature", None)


ETH2_DST = b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_"


def hash_to_curve_g2(engine: Engine, signing_roots: Sequence[bytes], dst: bytes = ETH2_DST) -> np.ndarray:
    """hash_to_curve(signing_root, DST) of every root, on the GPU (pe_hash_to_g2): (n, 192) uint8 message points, what
    fast_aggregate_verify, batch_fast_aggregate_verify, verify_attestation_signatures, verify_resident_attestations and
    process_deposits take as ``message_point(s)``."""
    return engine.hash_to_g2([bytes(r) for r in signing_roots], dst)


def fast_aggregate_verify(store: Store, indices: Sequence[int], message_point, signature) -> bool:
    """bls.FastAggregateVerify(pubkeys of ``indices``, message, signature) -- the check is_valid_indexed_attestation ends with
    (pe:1456) -- computed on the GPU: the registry pubkeys are summed and e(sum, H(m)) == e(g1, signature) is decided by the
    pairing-product kernels.  ``message_point`` is H(m) as a 192-byte uncompressed G2 point (hash_to_curve_g2 makes them),
    ``signature`` the 192-byte uncompressed aggregate signature.  Returns the computed boolean; it may be passed as
    ``signature_valid`` wherever the verdict is injected today (attestations, IndexedAttestation).  An empty index list, an
    identity signature and a point off its curve give False.  Subgroup membership is checked by Engine.g2_subgroup_check /
    key validation, not here."""
    idx = np.asarray(list(indices), dtype=np.uint32)
    verdict = store.engine.fast_aggregate_verify(idx, np.array([0, idx.size], dtype=np.uint32),
                                                 np.frombuffer(bytes(message_point), dtype=np.uint8),
                                                 np.frombuffer(bytes(signature), dtype=np.uint8))
    return int(verdict[0]) == 1


def batch_fast_aggregate_verify(store: Store, index_lists: Sequence[Sequence[int]], message_points, signatures) -> list:
    """bls.FastAggregateVerify for many aggregates at once -- one list of indices, one H(m) and one signature (192-byte
    uncompressed G2 points) per aggregate -- by random linear combination with scalars the engine draws itself
    (Engine.batch_fast_aggregate_verify): one final exponentiation for the whole call when every aggregate is valid.  Returns one
    boolean per aggregate, each what fast_aggregate_verify returns for it; a signature outside G2 gives False."""
    lists = [np.asarray(list(ix), dtype=np.uint32) for ix in index_lists]
    off = np.cumsum([0] + [ix.size for ix in lists]).astype(np.uint32)
    idx = np.concatenate(lists) if lists else np.zeros(0, dtype=np.uint32)
    verdict = store.engine.batch_fast_aggregate_verify(
        idx, off, np.frombuffer(b"".join(bytes(m) for m in message_points), dtype=np.uint8),
        np.frombuffer(b"".join(bytes(s) for s in signatures), dtype=np.uint8))
    return [int(v) == 1 for v in verdict]


def verify_attestation_signatures(store: Store, signers: Sequence[Sequence[int]], message_points, signatures) -> list:
    """One boolean per UNAGGREGATED attestation: ``signers[g]`` are the validators whose single-signer attestations carry the
    same AttestationData (one committee's votes), ``message_points[g]`` is H(m) of that data as a 192-byte uncompressed G2 point
    (hash_to_curve_g2 makes them) and ``signatures[g]`` their 96-byte compressed BLSSignatures, in the order of ``signers[g]``.
    Engine.verify_signatures decides each group with one pairing check over sums weighted by scalars the engine draws itself,
    and finds the invalid members of a group that fails.  Returns a list of lists of booleans, shaped like ``signers``; each may
    be passed as ``signature_valid`` wherever the verdict is injected today.  A valid aggregate says nothing about its members
    (sig_a + D and sig_b - D sum to the honest aggregate): this call is what does."""
    lists = [np.asarray(list(ix), dtype=np.uint32) for ix in signers]
    off = np.cumsum([0] + [ix.size for ix in lists]).astype(np.uint32)
    who = np.concatenate(lists) if lists else np.zeros(0, dtype=np.uint32)
    sig = np.frombuffer(b"".join(bytes(s) for group in signatures for s in group), dtype=np.uint8)
    msg = np.frombuffer(b"".join(bytes(m) for m in message_points), dtype=np.uint8)
    verdict, _, _, _ = store.engine.verify_signatures(sig, who, off, msg, aggregates=False)
    return [[int(v) == 1 for v in verdict[off[g]:off[g + 1]]] for g in range(len(lists))]


def verify_resident_attestations(store: Store, message_points, point_of_row=None) -> list:
    """The pairing check of is_valid_indexed_attestation (pe:736, 976, 1456) for every aggregate the engine's last
    ``aggregate_signed`` over DeviceRows formed (with ``want_aggregate_pubkeys=True``), computed where the aggregate keys and
    signatures lie; the verdicts take the place of the injected ``signature_valid``: ``on_attestation_batch`` /
    ``process_attestation_batch`` with ``(ROWS_RESIDENT, RESIDENT)`` afterwards reject every group that did not verify with
    PE_ATT_BAD_SIGNATURE.  ``message_points``: H(m) as 192-byte uncompressed G2 points (hash_to_curve_g2 makes them), one per
    group in group order, or -- with ``point_of_row`` (one index per input row) -- in any order, named by row.  Returns one
    entry per group: True / False, or None for a group without a committee (the handlers reject it for that reason)."""
    msg = np.frombuffer(b"".join(bytes(m) for m in message_points), dtype=np.uint8)
    verdict = store.engine.verify_resident(msg, point_of_row=point_of_row, apply=True)
    return [None if int(v) == _abi.PE_BLS_UNDECIDED else int(v) == _abi.PE_BLS_VALID for v in verdict]


# The message of an attestation's signature, as scalar logic: what the engine's k_att_signing_roots computes per row
# (Engine.attestation_signing_roots) and what a caller needs once per fork to fill pe_attester_domains.  The reference names
# compute_signing_root and get_domain and holds no text of them; these are the consensus specification's.
DOMAIN_BEACON_ATTESTER = bytes([1, 0, 0, 0])
GENESIS_FORK_VERSION = bytes(4)


def _sha256(data: bytes) -> bytes:
    import hashlib
    return hashlib.sha256(data).digest()


def _u64_chunk(v: int) -> bytes:
    return int(v).to_bytes(8, "little") + bytes(24)


def compute_fork_data_root(current_version: bytes, genesis_validators_root: bytes) -> bytes:
    """hash_tree_root(ForkData(current_version, genesis_validators_root)): two chunks, one hash."""
    assert len(current_version) == 4 and len(genesis_validators_root) == 32
    return _sha256(bytes(current_version) + bytes(28) + bytes(genesis_validators_root))


def compute_domain(domain_type: bytes, fork_version: Optional[bytes] = None, genesis_validators_root: Optional[bytes] = None) -> bytes:
    """domain_type + compute_fork_data_root(fork_version, genesis_validators_root)[:28]"""
    assert len(domain_type) == 4
    fork_version = GENESIS_FORK_VERSION if fork_version is None else bytes(fork_version)
    genesis_validators_root = ZERO_ROOT if genesis_validators_root is None else bytes(genesis_validators_root)
    return bytes(domain_type) + compute_fork_data_root(fork_version, genesis_validators_root)[:28]


def get_domain(state, domain_type: bytes, epoch: int) -> bytes:
    """get_domain(state, domain_type, epoch): over ``state.fork.previous_version`` before ``state.fork.epoch``, over
    ``state.fork.current_version`` from it on.  (The specification's default epoch, the state's current one, is the caller's
    to pass: the signature of an attestation takes ``data.target.epoch``.)"""
    fork = state.fork
    version = fork.previous_version if int(epoch) < int(fork.epoch) else fork.current_version
    return compute_domain(domain_type, bytes(version), bytes(state.genesis_validators_root))


def _attestation_data_root(data) -> bytes:
    cp = lambda c: _sha256(_u64_chunk(c.epoch) + bytes(c.root))
    h01 = _sha256(_u64_chunk(data.slot) + _u64_chunk(data.index))
    h23 = _sha256(bytes(data.beacon_block_root) + cp(data.source))
    h45 = _sha256(cp(data.target) + ZERO_ROOT)
    h67 = _sha256(bytes(64))
    return _sha256(_sha256(h01 + h23) + _sha256(h45 + h67))


def compute_signing_root(data, domain: bytes) -> bytes:
    """compute_signing_root(AttestationData, domain) = hash_tree_root(SigningData(hash_tree_root(data), domain)): the 32 bytes
    an attestation's signature is over.  ``data``: anything with AttestationData's fields."""
    assert len(domain) == 32
    return _sha256(_attestation_data_root(data) + bytes(domain))


def verify_resident_attestation_data(store: Store, fork_epoch: int, domain_previous: bytes, domain_current: bytes) -> list:
    """verify_resident_attestations with the messages taken from the aggregates themselves (pe_verify_resident_data): every
    group of the engine's last ``aggregate_signed`` over DeviceRows is verified over compute_signing_root of ITS OWN
    AttestationData under get_domain(state, DOMAIN_BEACON_ATTESTER, data.target.epoch) -- ``domain_previous`` before
    ``fork_epoch``, ``domain_current`` from it on -- hashed to the curve and paired on the GPU, and the verdicts take the place of
    the injected ``signature_valid`` as there.  Returns one entry per group: True / False, or None for a group without a
    committee."""
    verdict, _ = store.engine.verify_resident_data(fork_epoch, domain_previous, domain_current, apply=True)
    return [None if int(v) == _abi.PE_BLS_UNDECIDED else int(v) == _abi.PE_BLS_VALID for v in verdict]


def get_head(store: Store) -> bytes:
    """pe:1102-1116.  Raises (AssertionError) when the justified checkpoint has moved and the balances of its state
    have not been handed over (Store.ensure_justified_state)."""
    store.ensure_justified_state()
    return store.engine.get_head()


def prune(store: Store) -> dict:
    """Re-root the store at ``store.finalized_checkpoint.root`` (Engine.prune): the finalized root and its descendants
    stay, every other block leaves the engine's table and ``store.blocks``.  Not a reference function -- its Store never
    forgets a block -- but unobservable to ``get_head``: on_block refuses blocks outside that subtree (pe:998-1005),
    get_head starts inside it (pe:1106) and a block's weight sums its own subtree (pe:322).  Call it after an ``on_block``
    that raised the finalized checkpoint.  -> the engine's counts (blocks_before, blocks_after, votes_remapped,
    votes_orphaned)."""
    eng = store.engine
    stats = eng.prune()
    if stats["blocks_after"] != stats["blocks_before"]:
        kept = {eng.block_root_at(i) for i in range(eng.num_blocks)}
        for root in [r for r in store.blocks if r not in kept]:
            del store.blocks[root]
    return stats


# ----------------------------------------------------------------------------- process_attestation
class StateBinding:
    """Binds a BeaconState-like object to the engine's working participation arrays so that
    ``process_attestation(state, attestation)`` can mutate it as the pyspec does."""

    def __init__(self, engine: Engine, state, chain_tip_root: bytes, base_reward_per_increment: int):
        self.engine = engine
        self.state = state
        self.chain_tip_root = bytes(chain_tip_root)
        self.base_reward_per_increment = int(base_reward_per_increment)
        engine.participation_set(0, np.asarray(state.current_epoch_participation, dtype=np.uint8))
        engine.participation_set(1, np.asarray(state.previous_epoch_participation, dtype=np.uint8))
        # the working state's own registry view (effective balances, activity in current/previous epoch, slashed)
        spe = int(engine.cfg.slots_per_epoch)
        cur = int(state.slot) // spe
        prev = max(cur - 1, GENESIS_EPOCH)
        n = len(state.validators)
        bal = np.fromiter((int(v.effective_balance) for v in state.validators), dtype=np.uint64, count=n)
        fl = np.fromiter(
            ((_abi.PE_VAL_ACTIVE if int(v.activation_epoch) <= cur < int(v.exit_epoch) else 0)
             | (_abi.PE_VAL_SLASHED if v.slashed else 0)
             | (_abi.PE_VAL_ACTIVE_PREV if int(v.activation_epoch) <= prev < int(v.exit_epoch) else 0)
             for v in state.validators), dtype=np.uint8, count=n)
        engine.state_set_validators(bal, fl)

    def ctx(self) -> pe_state_ctx:
        s = self.state
        c = pe_state_ctx()
        c.slot = int(s.slot)
        c.chain_tip_root[:] = self.chain_tip_root
        c.current_justified_epoch = int(s.current_justified_checkpoint.epoch)
        c.current_justified_root[:] = bytes(s.current_justified_checkpoint.root)
        c.previous_justified_epoch = int(s.previous_justified_checkpoint.epoch)
        c.previous_justified_root[:] = bytes(s.previous_justified_checkpoint.root)
        c.base_reward_per_increment = self.base_reward_per_increment
        return c

    def sync_back(self):
        self.state.current_epoch_participation[:] = [int(x) for x in self.engine.participation_get(0)]
        self.state.previous_epoch_participation[:] = [int(x) for x in self.engine.participation_get(1)]


_BINDING_ATTR = "_posevo_state_binding"


def bind_state(engine: Engine, state, chain_tip_root: bytes, base_reward_per_increment: int) -> StateBinding:
    """The binding lives ON the state object (not in a table keyed by id(state), which would leak and could hand a
    recycled id a stale binding); ``unbind_state`` drops it."""
    b = StateBinding(engine, state, chain_tip_root, base_reward_per_increment)
    object.__setattr__(state, _BINDING_ATTR, b)
    return b


def unbind_state(state) -> None:
    if getattr(state, _BINDING_ATTR, None) is not None:
        object.__setattr__(state, _BINDING_ATTR, None)


def _binding(state) -> Optional[StateBinding]:
    b = getattr(state, _BINDING_ATTR, None)
    return b if b is not None and b.state is state else None   # a copy of a bound state is not bound


def process_attestation(state, attestation, *, get_beacon_proposer_index: Optional[Callable] = None,
                        proposer_index: Optional[int] = None) -> None:
    """pe:722-754.  ``state`` must have been bound with ``bind_state``.  The proposer that earns the reward
    (pe:754) is ``get_beacon_proposer_index(state)`` or the explicit ``proposer_index``: one of them is required --
    crediting a default validator would silently corrupt ``state.balances``."""
    b = _binding(state)
    assert b is not None, "process_attestation: bind_state(engine, state, ...) first"
    assert get_beacon_proposer_index is not None or proposer_index is not None, \
        "process_attestation: pass get_beacon_proposer_index or proposer_index (pe:754)"
    status, numerators = b.engine.process_attestation_batch(b.ctx(), [_att_row(attestation)])
    if status[0] != 0:
        raise EngineError(int(status[0]), "process_attestation: " + _abi.ATT_STATUS_NAMES.get(int(status[0]), "?"))
    b.sync_back()
    # Reward proposer (pe:752-754)
    denominator = WEIGHT_DENOMINATOR * (WEIGHT_DENOMINATOR - PROPOSER_WEIGHT) // PROPOSER_WEIGHT
    proposer_reward = int(numerators[0]) // denominator
    proposer = int(proposer_index) if proposer_index is not None else int(get_beacon_proposer_index(state))
    state.balances[proposer] += proposer_reward
    state._last_proposer_reward_numerator = int(numerators[0])


# ----------------------------------------------------------------------------- FFG
JUSTIFICATION_BITS_LENGTH = 4


# The finalization rules of pe:841-852 as data: (justified bits that must all be set, which of the two checkpoints held BEFORE
# this epoch's update is the source, how many epochs back that source must lie).  Rules apply in this order; a later
# match overrides an earlier one, as the reference's four consecutive `if`s do.
_FINALITY_RULES = (
    (range(1, 4), "previous", 3),   # epochs 2-4 back justified, the 2nd finalizes its source, the 4th
    (range(1, 3), "previous", 2),   # epochs 2-3 back justified, source = the 3rd
    (range(0, 3), "current", 2),    # epochs 1-3 back justified, source = the 3rd
    (range(0, 2), "current", 1),    # epochs 1-2 back justified, source = the 2nd
)


def weigh_justification_and_finalization(state, total_active_balance: int, previous_epoch_target_balance: int,
                                         current_epoch_target_balance: int, *, get_block_root: Callable,
                                         slots_per_epoch: int) -> None:
    """The FFG verdict of pe:815-853 on the three Gwei sums `pe_ffg_balances` delivers.  Same state transition as the
    reference's function (tests/test_gpu_forkchoice.py runs both on the same states), written as two tables: which epoch
    a 2/3 supermajority justifies (bit position = epochs back), and `_FINALITY_RULES`."""
    epoch_now = int(state.slot) // slots_per_epoch
    epoch_before = max(epoch_now - 1, GENESIS_EPOCH)
    held = {"previous": state.previous_justified_checkpoint, "current": state.current_justified_checkpoint}
    make_checkpoint = type(held["current"])

    # justification: the bit vector ages by one epoch, then a supermajority of the target balance sets its epoch's bit
    aged = [False] + [bool(x) for x in state.justification_bits[:JUSTIFICATION_BITS_LENGTH - 1]]
    state.previous_justified_checkpoint = held["current"]
    for bit, epoch, target_balance in ((1, epoch_before, previous_epoch_target_balance),
                                       (0, epoch_now, current_epoch_target_balance)):
        if 3 * target_balance >= 2 * total_active_balance:
            aged[bit] = True
            state.current_justified_checkpoint = make_checkpoint(epoch=epoch, root=get_block_root(state, epoch))
    for i, v in enumerate(aged):
        state.justification_bits[i] = v

    # finalization
    for needed, source, distance in _FINALITY_RULES:
        if all(aged[i] for i in needed) and held[source].epoch + distance == epoch_now:
            state.finalized_checkpoint = held[source]


def process_justification_and_finalization(state, *, get_block_root: Callable) -> None:
    """pe:791-802.  ``state`` must have been bound with ``bind_state`` (its participation arrays live on the GPU);
    the three balance sums come from one streaming kernel over the working-state registry view."""
    b = _binding(state)
    assert b is not None, "process_justification_and_finalization: bind_state(engine, state, ...) first"
    spe = int(b.engine.cfg.slots_per_epoch)
    if int(state.slot) // spe <= GENESIS_EPOCH + 1:
        return
    total_active_balance, previous_target_balance, current_target_balance = b.engine.ffg_balances()
    state._last_ffg_balances = (total_active_balance, previous_target_balance, current_target_balance)
    weigh_justification_and_finalization(state, total_active_balance, previous_target_balance,
                                         current_target_balance, get_block_root=get_block_root, slots_per_epoch=spe)


# ----------------------------------------------------------------------------- epoch boundary
SHUFFLE_ROUND_COUNT = 90
MAX_EFFECTIVE_BALANCE = 32 * 10**9
HYSTERESIS_QUOTIENT = 4
HYSTERESIS_DOWNWARD_MULTIPLIER = 1
HYSTERESIS_UPWARD_MULTIPLIER = 5


def compute_proposer_index(state, indices: Sequence[int], seed: bytes, *, shuffle_round_count: int = SHUFFLE_ROUND_COUNT,
                           max_effective_balance: int = MAX_EFFECTIVE_BALANCE, max_tries: int = 0) -> int:
    """pe:604-618.  ``state`` must have been bound with ``bind_state``: the effective balances sampled are the
    working-state view the binding uploaded.  Where the reference would loop forever (no candidate among the first
    ``max_tries``, 0 = 4096, is accepted) this raises."""
    b = _binding(state)
    assert b is not None, "compute_proposer_index: bind_state(engine, state, ...) first"
    assert len(indices) > 0
    proposers, _ = b.engine.compute_proposers([bytes(seed)], np.asarray(indices, dtype=np.uint32), shuffle_round_count,
                                              max_effective_balance, max_tries)
    assert int(proposers[0]) != _abi.NONE32, "compute_proposer_index: no candidate was accepted within max_tries"
    return int(proposers[0])


def process_effective_balance_updates(state, *, max_effective_balance: int = MAX_EFFECTIVE_BALANCE,
                                      hysteresis_quotient: int = HYSTERESIS_QUOTIENT,
                                      downward_multiplier: int = HYSTERESIS_DOWNWARD_MULTIPLIER,
                                      upward_multiplier: int = HYSTERESIS_UPWARD_MULTIPLIER) -> None:
    """pe:122-133.  ``state`` must have been bound with ``bind_state``; the hysteresis rule runs over the engine's
    working-state view against ``state.balances`` and the new effective balances are written back to
    ``state.validators``."""
    b = _binding(state)
    assert b is not None, "process_effective_balance_updates: bind_state(engine, state, ...) first"
    n = len(state.validators)
    balances = np.fromiter((int(x) for x in state.balances), dtype=np.uint64, count=n)
    n_changed, new = b.engine.effective_balance_updates(balances, max_effective_balance, hysteresis_quotient,
                                                        downward_multiplier, upward_multiplier)
    if n_changed:
        for validator, value in zip(state.validators, new):
            validator.effective_balance = int(value)


# ----------------------------------------------------------------------------- rewards and penalties
def _rewards_call(state, which: int, params: dict, who: str) -> dict:
    """Hand state.balances, state.inactivity_scores and the validators' withdrawable epochs to the engine, run the
    part(s) of pe_rewards_and_penalties `which` names over the binding's working-state view and write balances and scores
    back.  (A caller that keeps them on the device between epochs uses Engine.rewards_and_penalties itself.)"""
    b = _binding(state)
    assert b is not None, who + ": bind_state(engine, state, ...) first"
    n = len(state.validators)
    balances = np.fromiter((int(x) for x in state.balances), dtype=np.uint64, count=n)
    scores = np.fromiter((int(x) for x in state.inactivity_scores), dtype=np.uint64, count=n)
    withdrawable = np.fromiter((int(v.withdrawable_epoch) for v in state.validators), dtype=np.uint64, count=n)
    b.engine.state_set_balances(balances, scores, withdrawable)
    current_epoch = int(state.slot) // int(b.engine.cfg.slots_per_epoch)
    stats = b.engine.rewards_and_penalties(current_epoch, int(state.finalized_checkpoint.epoch), params, which)
    new_balances, new_scores, _, _ = b.engine.state_get_balances()
    if which & _abi.PE_REWARDS_DELTAS:
        state.balances[:] = [int(x) for x in new_balances]
    if which & _abi.PE_REWARDS_INACTIVITY:
        state.inactivity_scores[:] = [int(x) for x in new_scores]
    return stats


def process_inactivity_updates(state, **params) -> None:
    """Altair's process_inactivity_updates over ``state.inactivity_scores`` (pe:368-369), on the GPU.  ``state`` must
    have been bound with ``bind_state`` (activity and slashed flags, effective balances and previous_epoch_participation
    are the binding's).  Keywords replace fields of pe_rewards_params (inactivity_score_bias, ...)."""
    state._last_rewards_stats = _rewards_call(state, _abi.PE_REWARDS_INACTIVITY, params, "process_inactivity_updates")


def process_rewards_and_penalties(state, **params) -> None:
    """Altair's process_rewards_and_penalties over ``state.balances`` (pe:112): the three flag-index delta pairs and the
    inactivity penalties, applied pair by pair.  Call it after ``process_inactivity_updates``, as process_epoch does.
    ``state`` must have been bound with ``bind_state``.  Keywords replace fields of pe_rewards_params."""
    state._last_rewards_stats = _rewards_call(state, _abi.PE_REWARDS_DELTAS, params, "process_rewards_and_penalties")


# ----------------------------------------------------------------------------- registry updates and slashings
def _u64_of(items, count: int) -> np.ndarray:
    return np.fromiter((int(x) for x in items), dtype=np.uint64, count=count)


def process_registry_updates(state, **params) -> None:
    """process_registry_updates over ``state.validators``, on the GPU: eligibility marks, ejections through the exit queue
    and the head of the activation queue (pe_registry_updates).  ``state`` must have been bound with ``bind_state``
    (effective balances are the binding's).  The validators' epochs, pubkeys and credentials are handed to the engine, the
    four epochs that can change are written back.  Keywords replace fields of pe_registry_params (ejection_balance,
    churn_limit_quotient, max_per_epoch_activation_churn_limit, ...).
    Every call moves the whole registry both ways: the epochs, balances, pubkeys and credentials go up (112 B per validator
    and the pubkeys' hashing), the four epochs come back.  There is no host route.  The path without any transfer is
    ``Engine.registry_updates`` over arrays that stay resident between epochs."""
    b = _binding(state)
    assert b is not None, "process_registry_updates: bind_state(engine, state, ...) first"
    vals, n, e = state.validators, len(state.validators), b.engine
    e.registry_set_epochs(_u64_of((v.activation_epoch for v in vals), n), _u64_of((v.exit_epoch for v in vals), n))
    b.epochs_resident = True
    scores = getattr(state, "inactivity_scores", None)
    e.state_set_balances(_u64_of(state.balances, n), None if scores is None else _u64_of(scores, n),
                         _u64_of((v.withdrawable_epoch for v in vals), n))
    e.registry_set_static(np.frombuffer(b"".join(bytes(v.pubkey) for v in vals), dtype=np.uint8).reshape(n, 48),
                          np.frombuffer(b"".join(bytes(v.withdrawal_credentials) for v in vals), dtype=np.uint8).reshape(n, 32),
                          _u64_of((v.activation_eligibility_epoch for v in vals), n))
    current_epoch = int(state.slot) // int(e.cfg.slots_per_epoch)
    state._last_registry_stats = e.registry_updates(current_epoch, int(state.finalized_checkpoint.epoch), params)
    act, ext, _ = e.registry_get_epochs()
    wdr = e.state_get_balances()[2]
    elig = e.registry_static()[2]
    for v, a, x, w, g in zip(vals, act, ext, wdr, elig):
        v.activation_epoch, v.exit_epoch, v.withdrawable_epoch, v.activation_eligibility_epoch = int(a), int(x), int(w), int(g)


def process_slashings(state, *, proportional_slashing_multiplier: int = 3, epochs_per_slashings_vector: int = 8192) -> None:
    """process_slashings over ``state.balances``, on the GPU (pe_process_slashings): the correlated penalty of every slashed
    validator half a slashings vector before its withdrawable epoch.  ``state`` must have been bound with ``bind_state``
    (activity and slashed flags and effective balances are the binding's); ``sum(state.slashings)`` is taken here, the
    vector itself is left alone.  Every call uploads the balances and withdrawable epochs and downloads the balances; the
    path without any transfer is ``Engine.process_slashings`` over resident balances."""
    b = _binding(state)
    assert b is not None, "process_slashings: bind_state(engine, state, ...) first"
    n, e = len(state.validators), b.engine
    scores = getattr(state, "inactivity_scores", None)
    e.state_set_balances(_u64_of(state.balances, n), None if scores is None else _u64_of(scores, n),
                         _u64_of((v.withdrawable_epoch for v in state.validators), n))
    current_epoch = int(state.slot) // int(e.cfg.slots_per_epoch)
    state._last_slashings_stats = e.process_slashings(current_epoch, sum(int(x) for x in state.slashings),
                                                      proportional_slashing_multiplier, epochs_per_slashings_vector)
    state.balances[:] = [int(x) for x in e.state_get_balances()[0]]


# ----------------------------------------------------------------------------- block operations: slashings and exits
def _block_operations(state, ops, proposer_index: int, params: dict, who: str) -> dict:
    """One pe_process_block_operations over a bound state: the epochs, balances and withdrawable epochs go up, and -- only
    if every operation is valid -- the exit and withdrawable epochs, the balances and the slashed flags come back and
    ``slashed_balance`` joins ``state.slashings`` where the state has one.  An invalid operation raises AssertionError, as the
    pyspec's assert would, and the state is untouched.  The path without any transfer is ``Engine.process_block_operations``
    over arrays that stay resident."""
    b = _binding(state)
    assert b is not None, who + ": bind_state(engine, state, ...) first"
    vals, n, e = state.validators, len(state.validators), b.engine
    e.registry_set_epochs(_u64_of((v.activation_epoch for v in vals), n), _u64_of((v.exit_epoch for v in vals), n))
    scores = getattr(state, "inactivity_scores", None)
    e.state_set_balances(_u64_of(state.balances, n), None if scores is None else _u64_of(scores, n),
                         _u64_of((v.withdrawable_epoch for v in vals), n))
    current_epoch = int(state.slot) // int(e.cfg.slots_per_epoch)
    status, stats = e.process_block_operations(current_epoch, int(proposer_index), ops, params)
    state._last_block_ops_stats = stats
    bad = [(i, int(s)) for i, s in enumerate(status) if s != 0]
    assert not bad, who + ": " + ", ".join(f"operation {i}: {_abi.OP_STATUS_NAMES.get(s, s)}" for i, s in bad)
    _, ext, _ = e.registry_get_epochs()
    bal, _, wdr, _ = e.state_get_balances()
    _, flags, _ = e.state_validators()
    for v, x, w, f in zip(vals, ext, wdr, flags):
        v.exit_epoch, v.withdrawable_epoch, v.slashed = int(x), int(w), bool(f & _abi.PE_VAL_SLASHED)
    state.balances[:] = [int(x) for x in bal]
    slashings = getattr(state, "slashings", None)
    if slashings is not None and len(slashings) and stats["slashed_balance"]:
        k = current_epoch % int((params or {}).get("epochs_per_slashings_vector", 8192)) % len(slashings)
        slashings[k] = int(slashings[k]) + stats["slashed_balance"]
    return stats


def _proposer_of(state, proposer_index, get_beacon_proposer_index, who: str) -> int:
    if proposer_index is None:
        assert get_beacon_proposer_index is not None, who + ": pass proposer_index or get_beacon_proposer_index"
        proposer_index = get_beacon_proposer_index(state)
    return int(proposer_index)


def _data_row(d) -> AttRow:
    return AttRow(int(d.slot), int(d.index), bytes(d.beacon_block_root), int(d.source.epoch), bytes(d.source.root),
                  int(d.target.epoch), bytes(d.target.root), np.zeros(0, dtype=np.uint8))


def _attester_slashing_op(attester_slashing, signature_valid: bool) -> dict:
    a1, a2 = attester_slashing.attestation_1, attester_slashing.attestation_2
    valid = bool(signature_valid) and bool(getattr(a1, "signature_valid", True)) and bool(getattr(a2, "signature_valid", True))
    return attester_slashing_op(_data_row(a1.data), list(a1.attesting_indices), _data_row(a2.data), list(a2.attesting_indices), valid)


def process_attester_slashing(state, attester_slashing, *, signature_valid: bool = True, proposer_index: Optional[int] = None,
                              get_beacon_proposer_index: Optional[Callable] = None, **params) -> None:
    """process_attester_slashing over a state bound with ``bind_state`` (pe_process_block_operations): every slashable
    validator of the two lists' intersection is slashed.  ``signature_valid``: the verdict over both aggregate signatures
    (AND-ed with the attestations' own ``signature_valid`` where they carry one).  Keywords replace fields of
    pe_block_ops_params.  Raises AssertionError on an invalid operation; the state is then untouched."""
    who = "process_attester_slashing"
    _block_operations(state, [_attester_slashing_op(attester_slashing, signature_valid)],
                      _proposer_of(state, proposer_index, get_beacon_proposer_index, who), params, who)


def process_proposer_slashing(state, proposer_slashing, *, hash_tree_root: Callable, signature_valid: bool = True,
                              proposer_index: Optional[int] = None, get_beacon_proposer_index: Optional[Callable] = None,
                              **params) -> None:
    """process_proposer_slashing over a bound state: ``proposer_slashing.signed_header_1 / _2 .message`` are the two
    BeaconBlockHeaders, compared by slot, proposer index and ``hash_tree_root``.  ``proposer_index``: the proposer of the
    block that carries the operation (it earns the whistleblower reward)."""
    who = "process_proposer_slashing"
    h1, h2 = proposer_slashing.signed_header_1.message, proposer_slashing.signed_header_2.message
    op = proposer_slashing_op(int(h1.slot), int(h1.proposer_index), bytes(hash_tree_root(h1)), int(h2.slot), int(h2.proposer_index),
                              bytes(hash_tree_root(h2)), signature_valid)
    _block_operations(state, [op], _proposer_of(state, proposer_index, get_beacon_proposer_index, who), params, who)


def process_voluntary_exit(state, signed_voluntary_exit, *, signature_valid: bool = True, **params) -> None:
    """process_voluntary_exit over a bound state: ``signed_voluntary_exit.message`` names validator_index and epoch."""
    m = signed_voluntary_exit.message
    # no slashing, no reward: the proposer is not read, any validator stands in
    _block_operations(state, [voluntary_exit_op(int(m.validator_index), int(m.epoch), signature_valid)], 0, params,
                      "process_voluntary_exit")


# ----------------------------------------------------------------------------- Capella: withdrawals and address changes
def _upload_for_withdrawals(state, who: str):
    """The columns the two Capella calls read, from a bound state: epochs, balances and withdrawable epochs, and the static
    part (the credentials).  The effective balances are the binding's view."""
    b = _binding(state)
    assert b is not None, who + ": bind_state(engine, state, ...) first"
    vals, n, e = state.validators, len(state.validators), b.engine
    e.registry_set_epochs(_u64_of((v.activation_epoch for v in vals), n), _u64_of((v.exit_epoch for v in vals), n))
    scores = getattr(state, "inactivity_scores", None)
    e.state_set_balances(_u64_of(state.balances, n), None if scores is None else _u64_of(scores, n),
                         _u64_of((v.withdrawable_epoch for v in vals), n))
    e.registry_set_static(np.frombuffer(b"".join(bytes(v.pubkey) for v in vals), dtype=np.uint8).reshape(n, 48),
                          np.frombuffer(b"".join(bytes(v.withdrawal_credentials) for v in vals), dtype=np.uint8).reshape(n, 32),
                          _u64_of((v.activation_eligibility_epoch for v in vals), n))
    return e


def _withdrawal_rows(withdrawals):
    return [(int(w.index), int(w.validator_index), bytes(w.address), int(w.amount)) for w in withdrawals]


def get_expected_withdrawals(state, **params):
    """get_expected_withdrawals over a state bound with ``bind_state`` (pe_process_withdrawals without PE_WD_APPLY): reads
    ``state.next_withdrawal_index`` and ``state.next_withdrawal_validator_index``.  Keywords replace fields of
    pe_withdrawals_params.  -> the expected withdrawals as WITHDRAWAL_DTYPE rows."""
    e = _upload_for_withdrawals(state, "get_expected_withdrawals")
    rows, _ = e.process_withdrawals(int(state.slot) // int(e.cfg.slots_per_epoch), int(state.next_withdrawal_index),
                                    int(state.next_withdrawal_validator_index), None, False, params)
    return rows


def process_withdrawals(state, payload, **params) -> None:
    """process_withdrawals over a bound state: ``payload.withdrawals`` must be the expected withdrawals; their balances are
    debited and the state's two next-indices move.  Raises AssertionError where the payload differs, as the pyspec's assert
    would; the state is then untouched.  The path without any transfer is ``Engine.process_withdrawals`` over arrays that stay
    resident."""
    who = "process_withdrawals"
    e = _upload_for_withdrawals(state, who)
    _, res = e.process_withdrawals(int(state.slot) // int(e.cfg.slots_per_epoch), int(state.next_withdrawal_index),
                                   int(state.next_withdrawal_validator_index), _withdrawal_rows(payload.withdrawals), True, params)
    state._last_withdrawals_result = res
    assert res["status"] == 0, f"{who}: withdrawal {res['first_mismatch']}: {_abi.WD_STATUS_NAMES.get(res['status'], res['status'])}"
    bal, _, _, _ = e.state_get_balances()
    state.balances[:] = [int(x) for x in bal]
    state.next_withdrawal_index = res["next_withdrawal_index"]
    state.next_withdrawal_validator_index = res["next_withdrawal_validator_index"]


def process_bls_to_execution_change(state, signed_address_change, *, signature_valid: bool = True) -> None:
    """process_bls_to_execution_change over a bound state: ``signed_address_change.message`` names validator_index,
    from_bls_pubkey and to_execution_address; ``signature_valid`` is the verdict over its signature
    (``Engine.bls_change_signing_roots`` gives the root to verify).  Raises AssertionError on an invalid change; the state is
    then untouched."""
    who = "process_bls_to_execution_change"
    e = _upload_for_withdrawals(state, who)
    m = signed_address_change.message
    status, _ = e.process_bls_to_execution_changes([(int(m.validator_index), bytes(m.from_bls_pubkey), bytes(m.to_execution_address),
                                                     bool(signature_valid))])
    assert status[0] == 0, f"{who}: {_abi.CRED_STATUS_NAMES.get(int(status[0]), int(status[0]))}"
    _, cred, _, _ = e.registry_static()
    v = state.validators[int(m.validator_index)]
    v.withdrawal_credentials = cred[int(m.validator_index)].tobytes()


def attester_slashing_ops_from_evidence(evidence: Iterable, signature_valid: bool = True) -> List[dict]:
    """``find_attester_slashings`` output -> single-validator operations for ``Engine.process_block_operations``, by the
    slasher's own convention (include/posevo.h: on_attester_slashing with attesting_indices = [v] on both sides): one
    operation per (pair of AttestationData, validator), in the evidence's order and ascending validators."""
    ops = []
    for s in evidence:
        both = sorted(set(s.attestation_1.attesting_indices) & set(s.attestation_2.attesting_indices))
        ops += [attester_slashing_op(_data_row(s.attestation_1.data), [v], _data_row(s.attestation_2.data), [v], signature_valid)
                for v in both]
    return ops


# ----------------------------------------------------------------------------- deposits
def process_deposits(state, deposits, message_points, *, check_proofs: bool = True, make_validator: Optional[Callable] = None,
                     **params) -> np.ndarray:
    """process_deposit (pe:139-175) for ``deposits`` in order, on the GPU (pe_process_deposits): Merkle proofs against
    ``state.eth1_data.deposit_root`` at ``state.eth1_deposit_index`` (check_proofs False: genesis), the pubkey lookup in a
    device-side index, proofs of possession for new pubkeys, top-ups and appended validators.  ``state`` must have been bound
    with ``bind_state``.  message_points[i]: hash_to_curve(compute_signing_root(DepositMessage_i, domain)) as a 192-byte uncompressed
    G2 point -- ``Engine.deposit_signing_roots`` gives the roots, hash_to_curve_g2 the points.
    make_validator(**fields): how a Validator of the caller's state type is made (default: a SimpleNamespace).
    A failing proof raises AssertionError, as the reference does, with the state untouched.  -> the statuses (DEP_*).
    Every call moves the registry up (as process_registry_updates does); the path without any transfer is
    ``Engine.process_deposits`` over arrays that stay resident.  Keywords replace fields of pe_deposit_params."""
    from types import SimpleNamespace

    b = _binding(state)
    assert b is not None, "process_deposits: bind_state(engine, state, ...) first"
    deposits = list(deposits)
    vals, n, e = state.validators, len(state.validators), b.engine
    e.registry_set_epochs(_u64_of((v.activation_epoch for v in vals), n), _u64_of((v.exit_epoch for v in vals), n))
    b.epochs_resident = True
    scores = getattr(state, "inactivity_scores", None)
    e.state_set_balances(_u64_of(state.balances, n), None if scores is None else _u64_of(scores, n),
                         _u64_of((v.withdrawable_epoch for v in vals), n))
    e.registry_set_static(np.frombuffer(b"".join(bytes(v.pubkey) for v in vals), dtype=np.uint8).reshape(n, 48),
                          np.frombuffer(b"".join(bytes(v.withdrawal_credentials) for v in vals), dtype=np.uint8).reshape(n, 32),
                          _u64_of((v.activation_eligibility_epoch for v in vals), n))
    rows = [(d.data.pubkey, d.data.withdrawal_credentials, d.data.amount, d.data.signature) for d in deposits]
    mp = np.frombuffer(b"".join(bytes(m) for m in message_points), dtype=np.uint8)
    proofs = None
    if check_proofs:
        proofs = np.frombuffer(b"".join(b"".join(bytes(x) for x in d.proof) for d in deposits), dtype=np.uint8)
    res = e.process_deposits(rows, mp, proofs, int(state.eth1_deposit_index),
                             bytes(state.eth1_data.deposit_root) if check_proofs else None, params)
    assert res["n_bad_proof"] == 0, "process_deposit: is_valid_merkle_branch failed (pe:141)"
    state.eth1_deposit_index += len(deposits)
    p = e.deposit_params(**params)
    make = make_validator or (lambda **kw: SimpleNamespace(**kw))
    for d, st, idx in zip(deposits, res["status"], res["index"]):
        amount = int(d.data.amount)
        if st == _abi.PE_DEP_APPENDED:
            far = int(p.far_future_epoch)
            eff = min(amount - amount % int(p.effective_balance_increment), int(p.max_effective_balance))
            state.validators.append(make(pubkey=d.data.pubkey, withdrawal_credentials=d.data.withdrawal_credentials,
                                         effective_balance=eff, slashed=False, activation_eligibility_epoch=far,
                                         activation_epoch=far, exit_epoch=far, withdrawable_epoch=far))
            state.balances.append(amount)
            state.previous_epoch_participation.append(0)
            state.current_epoch_participation.append(0)
            if scores is not None:
                scores.append(0)
        elif st == _abi.PE_DEP_TOPUP:
            state.balances[int(idx)] += amount
    state._last_deposit_stats = {k: v for k, v in res.items() if k not in ("status", "index")}
    return res["status"]


# ----------------------------------------------------------------------------- the active set and what is counted from it
FAR_FUTURE_EPOCH = 2**64 - 1
# the constants pe:461-468 and pe:1225-1287 name, mainnet values; pass `preset=` to replace any of them
MAINNET_PRESET = {
    "SLOTS_PER_EPOCH": 32, "MAX_COMMITTEES_PER_SLOT": 64, "TARGET_COMMITTEE_SIZE": 128,
    "MIN_VALIDATOR_WITHDRAWABILITY_DELAY": 256, "MIN_PER_EPOCH_CHURN_LIMIT": 4, "CHURN_LIMIT_QUOTIENT": 65536,
    "MAX_DEPOSITS": 16, "SAFETY_DECAY": 10, "ETH_TO_GWEI": 10**9, "MAX_EFFECTIVE_BALANCE": MAX_EFFECTIVE_BALANCE,
    "EPOCHS_PER_SYNC_COMMITTEE_PERIOD": 256,
}


def _preset(preset: Optional[dict]) -> dict:
    return MAINNET_PRESET if preset is None else {**MAINNET_PRESET, **preset}


def is_active_validator(validator, epoch: int) -> bool:
    """Named by the reference, not given: the standard activation_epoch <= epoch < exit_epoch."""
    return int(validator.activation_epoch) <= int(epoch) < int(validator.exit_epoch)


def _active_set(state, epoch: int, want_indices: bool = False):
    """(n_active, total_active_balance, indices | None) of a bound state from the engine; the registry's epochs are
    handed to it once per binding."""
    b = _binding(state)
    assert b is not None, "the active set: bind_state(engine, state, ...) first"
    if not getattr(b, "epochs_resident", False):
        n = len(state.validators)
        b.engine.registry_set_epochs(
            np.fromiter((int(v.activation_epoch) for v in state.validators), dtype=np.uint64, count=n),
            np.fromiter((int(v.exit_epoch) for v in state.validators), dtype=np.uint64, count=n))
        b.epochs_resident = True
    return b.engine.active_set(int(epoch), want_indices)


def _current_epoch(state, p: dict) -> int:
    return int(state.slot) // p["SLOTS_PER_EPOCH"]


def get_active_validator_indices(state, epoch: int) -> List[int]:
    """Named at pe:467 / pe:1234 / pe:1267.  ``state`` must have been bound with ``bind_state``; the list is compacted on
    the GPU and stays there as the engine's resident active list (``ACTIVE_RESIDENT``)."""
    return [int(i) for i in _active_set(state, epoch, True)[2]]


def get_committee_count_per_slot(state, epoch: int, *, n_active: Optional[int] = None, preset: Optional[dict] = None) -> int:
    """pe:461-468.  ``n_active`` = len(get_active_validator_indices(state, epoch)) where the caller already holds it
    (``state`` is then not read); else it is counted on the GPU for the bound ``state``."""
    p = _preset(preset)
    if n_active is None:
        n_active = _active_set(state, epoch)[0]
    return max(1, min(p["MAX_COMMITTEES_PER_SLOT"], int(n_active) // p["SLOTS_PER_EPOCH"] // p["TARGET_COMMITTEE_SIZE"]))


def get_validator_churn_limit(state, *, n_active: Optional[int] = None, preset: Optional[dict] = None) -> int:
    """Named at pe:1270, not given: the standard max(MIN_PER_EPOCH_CHURN_LIMIT, active validators // CHURN_LIMIT_QUOTIENT)."""
    p = _preset(preset)
    if n_active is None:
        n_active = _active_set(state, _current_epoch(state, p))[0]
    return max(p["MIN_PER_EPOCH_CHURN_LIMIT"], int(n_active) // p["CHURN_LIMIT_QUOTIENT"])


def compute_weak_subjectivity_period(state, *, n_active: Optional[int] = None, total_active_balance: Optional[int] = None,
                                     preset: Optional[dict] = None) -> int:
    """pe:1257-1287.  The two registry-wide quantities -- the active validators of the current epoch and their total
    balance -- come from one ``Engine.active_set`` call for the bound ``state``, or from the caller (both together;
    ``state`` is then not read)."""
    p = _preset(preset)
    if n_active is None or total_active_balance is None:
        assert n_active is None and total_active_balance is None, "pass both n_active and total_active_balance, or neither"
        n_active, total_active_balance, _ = _active_set(state, _current_epoch(state, p))
    count = int(n_active)
    mean = int(total_active_balance) // count // p["ETH_TO_GWEI"]           # t: average active balance, ETH
    cap = p["MAX_EFFECTIVE_BALANCE"] // p["ETH_TO_GWEI"]                    # T
    churn = get_validator_churn_limit(state, n_active=count, preset=p)      # delta
    top_ups = p["MAX_DEPOSITS"] * p["SLOTS_PER_EPOCH"]                      # Delta
    decay = p["SAFETY_DECAY"]                                               # D
    light, heavy = 200 + 3 * decay, 200 + 12 * decay
    if cap * light < mean * heavy:
        by_churn = count * (mean * heavy - cap * light) // (600 * churn * (2 * mean + cap))
        by_top_ups = count * light // (600 * top_ups)
        return p["MIN_VALIDATOR_WITHDRAWABILITY_DELAY"] + max(by_churn, by_top_ups)
    return p["MIN_VALIDATOR_WITHDRAWABILITY_DELAY"] + 3 * count * decay * mean // (200 * top_ups * (cap - mean))


def get_latest_weak_subjectivity_checkpoint_epoch(state, safety_decay: float = 0.1, *, n_active: Optional[int] = None,
                                                  finalized_epoch: Optional[int] = None, preset: Optional[dict] = None):
    """pe:1225-1241, its float arithmetic as written (the result is a float whenever the modulus is).  ``n_active`` and
    ``finalized_epoch`` from the caller, or from the bound ``state``."""
    p = _preset(preset)
    if n_active is None:
        n_active = _active_set(state, _current_epoch(state, p))[0]
    if finalized_epoch is None:
        finalized_epoch = int(state.finalized_checkpoint.epoch)
    count = int(n_active)
    churn_floor, quotient = p["MIN_PER_EPOCH_CHURN_LIMIT"], p["CHURN_LIMIT_QUOTIENT"]
    # whole multiples of 256 epochs; true division, then floor division of a float: a float modulus, as in the reference
    if count >= churn_floor * quotient:
        extra = 256 * ((safety_decay * quotient / 2) // 256)
    else:
        extra = 256 * ((safety_decay * count / (2 * churn_floor)) // 256)
    modulus = p["MIN_VALIDATOR_WITHDRAWABILITY_DELAY"] + extra
    return finalized_epoch - (finalized_epoch % modulus)


def is_within_weak_subjectivity_period(current_epoch: int, ws_state_epoch: int, ws_period: int) -> bool:
    """The comparison pe:1298-1301 ends in: ws_period = compute_weak_subjectivity_period(ws_state), ws_state_epoch and
    current_epoch = the epochs of ws_state.slot and of the store's current slot.  The two asserts before it (pe:1295-1296)
    compare roots and are the caller's."""
    return int(current_epoch) <= int(ws_state_epoch) + int(ws_period)


def compute_sync_committee_period(epoch: int, *, preset: Optional[dict] = None) -> int:
    """pe:586-587."""
    return int(epoch) // _preset(preset)["EPOCHS_PER_SYNC_COMMITTEE_PERIOD"]


def is_assigned_to_sync_committee(current_epoch: int, epoch: int, validator_index: int, current_indices, next_indices, *,
                                  preset: Optional[dict] = None) -> bool:
    """pe:564-577 as scalar logic over the two index lists ``Engine.sync_committee_get`` returns (SYNC_CURRENT, SYNC_NEXT).
    The reference asks whether the validator's PUBKEY is among the committee's pubkeys; that equals membership by index while
    the registry's pubkeys are distinct, which process_deposit guarantees (a deposit of a known pubkey tops its validator up
    and appends none).  ``epoch`` must lie in the current or the next period: AssertionError otherwise, as in the reference."""
    period = compute_sync_committee_period(epoch, preset=preset)
    current_period = compute_sync_committee_period(current_epoch, preset=preset)
    assert period in (current_period, current_period + 1)
    members = current_indices if period == current_period else next_indices
    return any(int(m) == int(validator_index) for m in members)
