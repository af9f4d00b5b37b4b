"""numpy-level wrapper over the C ABI (include/posevo.h).  Thin: no arithmetic here.

Every method maps to exactly one ``pe_*`` entry point and raises ``EngineError``
(an ``AssertionError`` subclass, so spec-style ``assert``-driven tests behave as
with the pyspec) on a non-zero status.
"""
from __future__ import annotations

import ctypes as C
import sys
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _abi
from ._abi import pe_attestation, pe_config, pe_state_ctx

ZERO_ROOT = bytes(32)


class EngineError(AssertionError):
    def __init__(self, status: int, message: str):
        super().__init__(f"posevo status {status}: {message}")
        self.status = status


_c_char = C.c_char


class DeviceArena:
    """A bit arena that already lies in device memory (or pinned host memory): ``ptr`` = its address, ``size`` = bytes.
    pe_aggregate copies it with the copy engine instead of passing over it on the host; keep it unchanged (and ``keep``,
    the owning object, alive) until the call's outputs are complete."""
    __slots__ = ("ptr", "size", "keep")

    def __init__(self, ptr: int, size: int, keep=None):
        self.ptr, self.size, self.keep = int(ptr), int(size), keep


class DeviceRows:
    """Attestation rows (``n`` x struct pe_attestation, 144 bytes each, 16-byte aligned) that lie in DEVICE memory:
    ``Engine.aggregate(packed=(DeviceRows(...), arena))`` groups, resolves and validates them on the device
    (include/posevo.h, PE_ROWS_RESIDENT) -- the host reads nothing of them.  Keep them unchanged (and ``keep`` alive)
    until the call's outputs are complete."""
    __slots__ = ("ptr", "n", "keep")

    def __init__(self, ptr: int, n: int, keep=None):
        self.ptr, self.n, self.keep = int(ptr), int(n), keep

    def __len__(self):
        return self.n


def _ptr(a, ctype=None):
    """Address of a C-contiguous numpy buffer (None stays NULL).  c_char.from_buffer + addressof is the cheapest route
    ctypes offers; read-only or empty arrays take the slower ndarray.ctypes path."""
    if a is None:
        return None
    if a.__class__ is DeviceArena:
        return a.ptr
    try:
        return C.addressof(_c_char.from_buffer(a))
    except (TypeError, ValueError, BufferError):
        return a.ctypes.data


_ACTIVE_RESIDENT_ARG = DeviceArena(_abi.PE_ACTIVE_RESIDENT, 0)   # the sentinel address, as _ptr passes it on


def _att_ptr(arr):
    """ctypes array of pe_attestation or numpy structured array (synth.ATT_DTYPE) -> address."""
    if isinstance(arr, np.ndarray):
        assert arr.dtype.itemsize == 144 and arr.flags["C_CONTIGUOUS"]
        return _ptr(arr)
    return arr


def _root(b: bytes):
    assert len(b) == 32, "roots are 32 bytes"
    return (C.c_uint8 * 32).from_buffer_copy(bytes(b))


@dataclass
class AttRow:
    """AttestationData (pe:689-697) + aggregation bits + the injected signature verdict."""
    slot: int
    index: int
    beacon_block_root: bytes
    source_epoch: int
    source_root: bytes
    target_epoch: int
    target_root: bytes
    bits: np.ndarray  # bool or 0/1, one entry per committee position
    signature_valid: bool = True
    is_from_block: bool = False


def pack_attestations(rows: Sequence[AttRow]):
    """-> (ctypes array of pe_attestation, uint8 arena).  Bits are packed LSB-first (SSZ order)."""
    n = len(rows)
    arr = (pe_attestation * max(n, 1))()
    chunks = []
    off = 0
    for i, r in enumerate(rows):
        a = arr[i]
        a.slot, a.index = int(r.slot), int(r.index)
        C.memmove(a.beacon_block_root, bytes(r.beacon_block_root), 32)
        a.source_epoch = int(r.source_epoch)
        C.memmove(a.source_root, bytes(r.source_root), 32)
        a.target_epoch = int(r.target_epoch)
        C.memmove(a.target_root, bytes(r.target_root), 32)
        bits = np.asarray(r.bits).astype(np.uint8)
        packed = np.packbits(bits, bitorder="little") if bits.size else np.zeros(0, dtype=np.uint8)
        a.bits_offset, a.n_bits = off, int(bits.size)
        a.flags = (_abi.PE_ATT_FLAG_SIGNATURE_VALID if r.signature_valid else 0) | (
            _abi.PE_ATT_FLAG_FROM_BLOCK if r.is_from_block else 0)
        chunks.append(packed)
        off += packed.size
    arena = np.concatenate(chunks) if chunks else np.zeros(0, dtype=np.uint8)
    if arena.size == 0:
        arena = np.zeros(1, dtype=np.uint8)
    return arr, np.ascontiguousarray(arena)


# -- block operations (pe_block_op): plain dicts, one constructor per kind ----
def attestation_data_bytes(row) -> bytes:
    """AttestationData as a pe_block_op carries it: the leading 128 bytes of the row's pe_attestation.  row: an AttRow, a
    pe_attestation, a row of a structured array (144 bytes) or 128+ bytes."""
    if isinstance(row, AttRow):
        row = pack_attestations([row])[0][0]
    if isinstance(row, pe_attestation):
        return bytes(C.string_at(C.addressof(row), 128))
    b = row.tobytes() if hasattr(row, "tobytes") else bytes(row)
    assert len(b) >= 128, "AttestationData is the leading 128 bytes of a pe_attestation"
    return b[:128]


def attester_slashing_op(data_1, indices_1, data_2, indices_2, signature_valid: bool = True) -> dict:
    """AttesterSlashing: two IndexedAttestations as (AttestationData, attesting_indices); signature_valid: the verdict over
    both aggregate signatures."""
    return dict(kind=_abi.PE_OP_ATTESTER_SLASHING, d1=attestation_data_bytes(data_1), d2=attestation_data_bytes(data_2),
                i1=[int(x) for x in indices_1], i2=[int(x) for x in indices_2], sig=bool(signature_valid))


def proposer_slashing_op(slot_1: int, proposer_index_1: int, root_1: bytes, slot_2: int, proposer_index_2: int, root_2: bytes,
                         signature_valid: bool = True) -> dict:
    """ProposerSlashing: of each signed header its slot, proposer index and hash_tree_root; signature_valid: both verdicts."""
    return dict(kind=_abi.PE_OP_PROPOSER_SLASHING, slot1=int(slot_1), prop1=int(proposer_index_1), root1=bytes(root_1),
                slot2=int(slot_2), prop2=int(proposer_index_2), root2=bytes(root_2), sig=bool(signature_valid))


def voluntary_exit_op(validator_index: int, epoch: int, signature_valid: bool = True) -> dict:
    """SignedVoluntaryExit: message.validator_index, message.epoch and the verdict over its signature."""
    return dict(kind=_abi.PE_OP_VOLUNTARY_EXIT, index=int(validator_index), epoch=int(epoch), sig=bool(signature_valid))


def pack_block_ops(ops):
    """-> (ctypes array of pe_block_op, the attester slashings' lists as one flat uint32 array)."""
    arr = (_abi.pe_block_op * max(len(ops), 1))()
    lists, off = [], 0
    for i, op in enumerate(ops):
        a = arr[i]
        a.kind = int(op["kind"])
        a.flags = _abi.PE_OP_FLAG_SIGNATURE_VALID if op["sig"] else 0
        if a.kind == _abi.PE_OP_ATTESTER_SLASHING:
            C.memmove(a.data_1, op["d1"], 128)
            C.memmove(a.data_2, op["d2"], 128)
            for name, idx in (("indices_1", op["i1"]), ("indices_2", op["i2"])):
                idx = np.asarray(idx, dtype=np.uint64)
                assert idx.size == 0 or int(idx.max()) < 2**32, "a validator index beyond 32 bits"
                setattr(a, name + "_offset", off)
                setattr(a, name + "_length", idx.size)
                lists.append(idx.astype(np.uint32))
                off += idx.size
        elif a.kind == _abi.PE_OP_PROPOSER_SLASHING:
            a.header_1_slot, a.header_1_proposer_index = op["slot1"], op["prop1"]
            a.header_2_slot, a.header_2_proposer_index = op["slot2"], op["prop2"]
            assert len(op["root1"]) == 32 and len(op["root2"]) == 32, "roots are 32 bytes"
            C.memmove(a.header_1_root, op["root1"], 32)
            C.memmove(a.header_2_root, op["root2"], 32)
        else:
            a.validator_index, a.exit_epoch = op["index"], op["epoch"]
    flat = np.ascontiguousarray(np.concatenate(lists)) if lists else np.zeros(0, dtype=np.uint32)
    return arr, flat


# -- Capella: withdrawals (pe_withdrawal) and address changes (pe_bls_change) ----
WITHDRAWAL_DTYPE = np.dtype([("index", "<u8"), ("validator_index", "<u8"), ("address", "u1", (20,)),
                             ("amount", "<u8")])  # == struct pe_withdrawal (44 bytes, packed)
BLS_CHANGE_DTYPE = np.dtype([("validator_index", "<u8"), ("from_bls_pubkey", "u1", (48,)), ("to_execution_address", "u1", (20,)),
                             ("flags", "<u4")])  # == struct pe_bls_change (80 bytes)
assert WITHDRAWAL_DTYPE.itemsize == 44 and BLS_CHANGE_DTYPE.itemsize == 80


def pack_withdrawals(withdrawals) -> np.ndarray:
    """WITHDRAWAL_DTYPE rows, or an iterable of (index, validator_index, address20, amount)."""
    if isinstance(withdrawals, np.ndarray) and withdrawals.dtype == WITHDRAWAL_DTYPE:
        return np.ascontiguousarray(withdrawals)
    items = list(withdrawals)
    rows = np.zeros(len(items), dtype=WITHDRAWAL_DTYPE)
    for i, (index, validator, address, amount) in enumerate(items):
        assert len(address) == 20, "an execution address is 20 bytes"
        rows[i] = (int(index), int(validator), np.frombuffer(bytes(address), dtype=np.uint8), int(amount))
    return rows


def pack_bls_changes(changes) -> np.ndarray:
    """BLS_CHANGE_DTYPE rows, or an iterable of (validator_index, from_bls_pubkey48, to_execution_address20, signature_valid)."""
    if isinstance(changes, np.ndarray) and changes.dtype == BLS_CHANGE_DTYPE:
        return np.ascontiguousarray(changes)
    items = list(changes)
    rows = np.zeros(len(items), dtype=BLS_CHANGE_DTYPE)
    for i, (validator, pubkey, address, valid) in enumerate(items):
        assert len(pubkey) == 48 and len(address) == 20, "a BLS pubkey is 48 bytes, an execution address 20"
        rows[i] = (int(validator), np.frombuffer(bytes(pubkey), dtype=np.uint8), np.frombuffer(bytes(address), dtype=np.uint8),
                   _abi.PE_CRED_FLAG_SIGNATURE_VALID if valid else 0)
    return rows


_ATT_DTYPE = np.dtype([
    ("slot", "<u8"), ("index", "<u8"), ("beacon_block_root", "u1", (32,)),
    ("source_epoch", "<u8"), ("source_root", "u1", (32,)),
    ("target_epoch", "<u8"), ("target_root", "u1", (32,)),
    ("bits_offset", "<u4"), ("n_bits", "<u4"), ("flags", "<u4"), ("reserved0", "<u4"),
])  # == synth.ATT_DTYPE == struct pe_attestation (144 bytes)


SLASH_EVIDENCE_DTYPE = np.dtype([("validator", "<u4"), ("kind", "<u4"), ("target_epoch_1", "<u4"), ("id_1", "<u4"),
                                 ("target_epoch_2", "<u4"), ("id_2", "<u4")])  # == struct pe_slash_evidence

_I32, _U32, _U64, _U8 = np.dtype(np.int32), np.dtype(np.uint32), np.dtype(np.uint64), np.dtype(np.uint8)


class _Resident:
    """Sentinel for ``packed=(rows, RESIDENT)``: the rows are rows of the last ``aggregate`` result and their OR-ed
    bits are used where pe_aggregate left them on the device (PE_BITS_RESIDENT, include/posevo.h)."""
    size = 0

    def __repr__(self):
        return "RESIDENT"


RESIDENT = _Resident()


class _RowsResident:
    """Sentinel for ``packed=(ROWS_RESIDENT, RESIDENT)``: every group of the last ``aggregate`` over DeviceRows, in
    group order, validated on the device (PE_ROWS_RESIDENT)."""

    def __repr__(self):
        return "ROWS_RESIDENT"


ROWS_RESIDENT = _RowsResident()


class _ActiveResident:
    """Sentinel for ``active_indices`` of ``compute_committees``, ``compute_committees_async`` and ``compute_proposers``:
    the list the last ``active_set`` left on the device (PE_ACTIVE_RESIDENT, include/posevo.h)."""

    def __repr__(self):
        return "ACTIVE_RESIDENT"


ACTIVE_RESIDENT = _ActiveResident()


class _BalancesResident:
    """Sentinel for ``balances`` of ``effective_balance_updates``: the vector ``state_set_balances`` /
    ``rewards_and_penalties`` left on the device (PE_BALANCES_RESIDENT, include/posevo.h)."""

    def __repr__(self):
        return "BALANCES_RESIDENT"


BALANCES_RESIDENT = _BalancesResident()
_BALANCES_RESIDENT_ARG = DeviceArena(_abi.PE_BALANCES_RESIDENT, 0)   # the sentinel address, as _ptr passes it on
REWARDS_INACTIVITY, REWARDS_DELTAS = _abi.PE_REWARDS_INACTIVITY, _abi.PE_REWARDS_DELTAS
SYNC_CURRENT, SYNC_NEXT = _abi.PE_SYNC_CURRENT, _abi.PE_SYNC_NEXT
SYNC_VERIFY, SYNC_APPLY = _abi.PE_SYNC_VERIFY, _abi.PE_SYNC_APPLY
ROOT_BALANCES, ROOT_INACTIVITY, ROOT_PART_PREV, ROOT_PART_CUR, ROOT_VALIDATORS = (
    _abi.PE_ROOT_BALANCES, _abi.PE_ROOT_INACTIVITY, _abi.PE_ROOT_PART_PREV, _abi.PE_ROOT_PART_CUR, _abi.PE_ROOT_VALIDATORS)
ROOT_ALL = ROOT_BALANCES | ROOT_INACTIVITY | ROOT_PART_PREV | ROOT_PART_CUR | ROOT_VALIDATORS
DEP_APPENDED, DEP_TOPUP, DEP_IGNORED_BAD_SIGNATURE, DEP_BAD_PROOF = (
    _abi.PE_DEP_APPENDED, _abi.PE_DEP_TOPUP, _abi.PE_DEP_IGNORED_BAD_SIGNATURE, _abi.PE_DEP_BAD_PROOF)
# struct pe_deposit_data as a numpy row: 184 bytes, no padding
DEPOSIT_DTYPE = np.dtype([("pubkey", np.uint8, 48), ("withdrawal_credentials", np.uint8, 32), ("amount", "<u8"),
                          ("signature", np.uint8, 96)])
assert DEPOSIT_DTYPE.itemsize == C.sizeof(_abi.pe_deposit_data) == 184
_ROOT_FIELDS = ((ROOT_BALANCES, "balances"), (ROOT_INACTIVITY, "inactivity_scores"),
                (ROOT_PART_PREV, "previous_epoch_participation"), (ROOT_PART_CUR, "current_epoch_participation"),
                (ROOT_VALIDATORS, "validators"))


class AggregateResult(dict):
    """Result of Engine.aggregate; ``res["bits"]`` decodes the OR-ed bitfields on demand."""

    def __getitem__(self, key):
        if key == "bits" and "bits" not in self:
            out, arena = [], dict.__getitem__(self, "out_arena")
            for a in dict.__getitem__(self, "atts"):
                off, nbits = int(a["bits_offset"]), int(a["n_bits"])
                nb = (nbits + 7) // 8
                out.append(np.unpackbits(arena[off:off + nb], bitorder="little")[:nbits].astype(bool))
            self["bits"] = out
        return dict.__getitem__(self, key)


class ResidentAggregateResult(dict):
    """Result of Engine.aggregate over DeviceRows: nothing is host-derived, so every field -- the number of groups
    included -- is valid once the call's outputs are complete (at return for a synchronous call, at the pipeline's
    completion otherwise).  Fields are sliced to the groups formed when they are read."""

    def __getitem__(self, key):
        raw = dict.__getitem__(self, "_raw")
        g = int(raw["n_groups"][0])
        if key == "n_groups":
            return g
        if key == "group_of":
            return raw["group_of"]
        if key == "out_arena":
            if g == 0:
                return raw["out_arena"][:0]
            last = raw["atts"][g - 1]
            return raw["out_arena"][: int(last["bits_offset"]) + (int(last["n_bits"]) + 7) // 8]
        if key == "bits":
            arena, out = raw["out_arena"], []
            for a in raw["atts"][:g]:
                off, nbits = int(a["bits_offset"]), int(a["n_bits"])
                out.append(np.unpackbits(arena[off:off + (nbits + 7) // 8], bitorder="little")[:nbits].astype(bool))
            return out
        if key in ("atts", "aggpk96", "count", "sig96c"):
            v = raw.get(key)
            return None if v is None else v[:g]
        if key == "sig_status":
            return raw.get(key)
        return dict.__getitem__(self, key)


class _Pipeline:
    def __init__(self, engine, lagged=False):
        self.e = engine
        self.lagged = lagged

    def __enter__(self):
        e = self.e
        # a lagged pipeline still in flight stays in flight
        if self.lagged and e._ring is not None and len(e._ring) < e._lag + 2:
            # outputs of lagged pipeline k are written at the exit of k + lag: a set handed out again before k + lag + 1
            # would never be stable to read
            raise ValueError(f"reuse_outputs(depth) must be >= {e._lag + 2} with lagged pipelines of lag depth {e._lag}")
        e._check((e._lib.pe_pipeline_begin_streaming if self.lagged else e._lib.pe_pipeline_begin)(e._h))
        e._pipe_keep = []
        e._ring_ord = {}
        return e

    def __exit__(self, exc_type, exc, tb):
        e = self.e
        if self.lagged and exc_type is None:
            rc = e._lib.pe_pipeline_end_lagged(e._h)
            # lag depth L: the generation L back is complete now, keep this one and the L - 1 before it alive
            e._lagged_keep = [e._pipe_keep] + (e._lagged_keep or [])[:e._lag - 1]
        else:
            rc = e._lib.pe_pipeline_end(e._h)
            e._lagged_keep = None
        e._pipe_keep = None
        if e._ring is not None:
            e._ring_i = (e._ring_i + 1) % len(e._ring)
        if exc_type is None:
            e._check(rc)
        return False


class Engine:
    """One engine handle = one fork-choice store + validator registry on one GPU."""

    def __init__(self, device: int = -1, **config):
        self._lib = _abi.load()
        cfg = pe_config()
        self._lib.pe_config_default(C.byref(cfg))
        cfg.device = device
        for k, v in config.items():
            if not hasattr(cfg, k):
                raise TypeError(f"unknown config field {k}")
            setattr(cfg, k, v)
        self.cfg = cfg
        h = C.c_void_p()
        rc = self._lib.pe_engine_create(C.byref(cfg), C.byref(h))
        if rc != _abi.PE_OK:
            raise EngineError(rc, self._lib.pe_strerror(rc).decode() +
                              " (the engine needs a HIP device; there is no CPU fallback)")
        self._h = h
        self._pipe_keep = None
        self._lagged_keep = None
        self._ring = None
        self._ring_i = 0
        self._ring_ord = {}
        self._lag = int(self._lib.pe_pipeline_get_lag(self._h)) or 2
        self._resident_active = 0   # length of the list the last active_set left on the device
        self._signed_device_rows = 0   # input rows of the last successful aggregate_signed over DeviceRows (verify_resident)

    def set_pipeline_lag(self, depth: int):
        """Lag depth of ``pipeline(lagged=True)`` blocks (pe_pipeline_set_lag): a block's outputs are complete when the
        depth-th next lagged block exits.  Completes everything in flight first."""
        self._check(self._lib.pe_pipeline_set_lag(self._h, int(depth)))
        self._lag = int(depth)
        self._lagged_keep = None

    # -- plumbing ---------------------------------------------------------
    def reuse_outputs(self, depth: int = 4):
        """Opt in to output-buffer reuse: the arrays the batch calls return come from a ring of `depth` buffer sets that
        advances at every pipeline exit (and after every batch call made outside a pipeline), instead of fresh
        ``np.empty`` allocations (whose first touch page-faults: 50+ us per step for the 1 MB of rows and bits an epoch
        returns).  An array stays valid for depth - 1 further pipelines / synchronous calls; copy what must live longer.
        Two calls of the same kind inside ONE pipeline get distinct sets (keyed by their ordinal in the pipeline).
        depth >= lag + 2 with lagged pipelines (4 at the default lag depth 2: entering one with a shallower ring raises)."""
        self._ring = [dict() for _ in range(max(depth, 1))]
        self._ring_i = 0
        self._ring_ord = {}

    def fill_ring(self):
        """Allocate (and touch) in every ring slot the output sets seen so far in any slot: a caller that wants to keep
        the outputs of a whole run -- ring depth = number of pipelines -- pays the allocations before its timed region."""
        if self._ring is None:
            return
        seen = {}
        for d in self._ring:
            for k, (arrs, _) in d.items():
                seen.setdefault(k, tuple(None if a is None else (a.shape, a.dtype) for a in arrs))
        for d in self._ring:
            for k, specs in seen.items():
                if k not in d:
                    arrs = tuple(None if sp is None else np.zeros(sp[0], dtype=sp[1]) for sp in specs)
                    for a in arrs:
                        if a is not None:
                            a.fill(0)  # np.zeros maps pages lazily: touch them now
                    d[k] = (arrs, tuple(_ptr(a) for a in arrs))

    def _outs(self, key, specs):
        """The output arrays of one call and their addresses: ``specs`` = ((shape, dtype) or None, ...).  With
        reuse_outputs() the set comes from the ring slot of the current pipeline -- one dict lookup instead of one
        allocation and one address computation per array (a step makes ~20 pointer arguments)."""
        if self._ring is None:
            arrs = tuple(None if sp is None else np.empty(sp[0], dtype=sp[1]) for sp in specs)
            return arrs, tuple(_ptr(a) for a in arrs)
        d = self._ring[self._ring_i]
        if self._pipe_keep is None:
            # a synchronous call: its results are complete at return, the next call gets the next set
            k = (key, specs, 0)
            self._ring_i = (self._ring_i + 1) % len(self._ring)
        else:
            # inside a pipeline every call's buffers are written at the pipeline's end: the n-th call of a kind gets
            # the n-th set of this ring slot (two aggregates of one pipeline must not share their outputs)
            o = self._ring_ord.get((key, specs), 0)
            self._ring_ord[(key, specs)] = o + 1
            k = (key, specs, o)
        hit = d.get(k)
        if hit is None:
            arrs = tuple(None if sp is None else np.zeros(sp[0], dtype=sp[1]) for sp in specs)  # zeros: touch the pages here
            hit = d[k] = (arrs, tuple(_ptr(a) for a in arrs))
        return hit

    def _keep(self, *buffers):
        """Inside a pipeline the engine writes into these buffers at pe_pipeline_end: keep them alive until then."""
        if self._pipe_keep is not None:
            self._pipe_keep.extend(b for b in buffers if b is not None)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pe_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != _abi.PE_OK:
            detail = self._lib.pe_last_error(self._h).decode()
            raise EngineError(rc, f"{self._lib.pe_strerror(rc).decode()}: {detail}")

    def pipeline(self, lagged: bool = False):
        """``with engine.pipeline(): ...`` -- the batch calls inside return once their device work is enqueued
        (pe_pipeline_begin); their output arrays are complete when the block exits (pe_pipeline_end): one wait per
        step instead of one per call.  get_head() inside the block is still synchronous.
        lagged=True (pe_pipeline_end_lagged): the block's outputs are complete when the L-th next lagged block exits
        (L = lag depth, default 2; or at drain() / any other synchronous call) -- step N's G1 sums run while the steps
        behind it are being prepared."""
        return _Pipeline(self, lagged)

    def drain(self):
        """Complete every pipelined call still in flight (pe_pipeline_end outside a pipeline does exactly that)."""
        self._check(self._lib.pe_pipeline_end(self._h))
        self._lagged_keep = None

    def set_stream(self, hip_stream: int):
        self._check(self._lib.pe_set_stream(self._h, C.c_void_p(hip_stream)))

    # -- store ------------------------------------------------------------
    def store_init(self, genesis_time: int, anchor_slot: int, anchor_root: bytes):
        self._check(self._lib.pe_store_init(self._h, genesis_time, anchor_slot, _root(anchor_root)))

    def set_validators(self, effective_balance, flags, pubkeys96=None):
        bal = np.ascontiguousarray(effective_balance, dtype=np.uint64)
        fl = np.ascontiguousarray(flags, dtype=np.uint8)
        assert bal.shape == fl.shape
        pk = None
        if pubkeys96 is not None:
            pk = np.ascontiguousarray(pubkeys96, dtype=np.uint8)
            assert pk.size == 96 * bal.size
        self._check(self._lib.pe_set_validators(self._h, bal.size, _ptr(pk, C.c_uint8), _ptr(bal, C.c_uint64),
                                                _ptr(fl, C.c_uint8)))

    def set_balances(self, effective_balance, flags):
        bal = np.ascontiguousarray(effective_balance, dtype=np.uint64)
        fl = np.ascontiguousarray(flags, dtype=np.uint8)
        self._check(self._lib.pe_set_balances(self._h, bal.size, _ptr(bal, C.c_uint64), _ptr(fl, C.c_uint8)))

    def on_tick(self, time: int):
        self._check(self._lib.pe_on_tick(self._h, time))

    def on_block(self, root, parent_root, slot, post_justified=(0, ZERO_ROOT), post_finalized=(0, ZERO_ROOT)):
        self._check(self._lib.pe_on_block(self._h, _root(root), _root(parent_root), slot, post_justified[0],
                                          _root(post_justified[1]), post_finalized[0], _root(post_finalized[1])))

    def add_block(self, root, parent_root, slot, post_justified=(0, ZERO_ROOT), post_finalized=(0, ZERO_ROOT)):
        self._check(self._lib.pe_add_block(self._h, _root(root), _root(parent_root), slot, post_justified[0],
                                           _root(post_justified[1]), post_finalized[0], _root(post_finalized[1])))

    def set_checkpoints(self, justified: Tuple[int, bytes], finalized: Tuple[int, bytes]):
        self._check(self._lib.pe_set_checkpoints(self._h, justified[0], _root(justified[1]), finalized[0],
                                                 _root(finalized[1])))

    def prune(self) -> dict:
        """pe_prune: re-root the block table at store.finalized_checkpoint.root (the root and its descendants stay, in
        their insertion order; the root becomes block 0) and remap the latest messages on the device.  The caller decides
        when -- typically after an ``on_block`` that raised the finalized checkpoint.  -> dict(blocks_before, blocks_after,
        votes_remapped, votes_orphaned); unobservable to ``get_head`` (include/posevo.h has the argument and the stated
        deviation for later calls that name a removed block)."""
        st = _abi.pe_prune_stats()
        self._check(self._lib.pe_prune(self._h, C.addressof(st)))
        return dict(blocks_before=int(st.blocks_before), blocks_after=int(st.blocks_after),
                    votes_remapped=int(st.votes_remapped), votes_orphaned=int(st.votes_orphaned))

    def set_proposer_boost(self, root: bytes):
        self._check(self._lib.pe_set_proposer_boost(self._h, _root(root)))

    def mark_equivocating(self, indices):
        idx = np.ascontiguousarray(indices, dtype=np.uint64)
        self._check(self._lib.pe_mark_equivocating(self._h, _ptr(idx, C.c_uint64), idx.size))

    def on_attester_slashing(self, row1: AttRow, indices1, row2: AttRow, indices2):
        a1, _ = pack_attestations([row1])
        a2, _ = pack_attestations([row2])
        i1 = np.ascontiguousarray(indices1, dtype=np.uint64)
        i2 = np.ascontiguousarray(indices2, dtype=np.uint64)
        self._check(self._lib.pe_on_attester_slashing(self._h, a1, _ptr(i1, C.c_uint64), i1.size, a2,
                                                      _ptr(i2, C.c_uint64), i2.size))

    def set_committees(self, epoch: int, offsets, members):
        off = np.ascontiguousarray(offsets, dtype=np.uint32)
        mem = np.ascontiguousarray(members, dtype=np.uint32)
        assert off[-1] == mem.size
        if mem.size == 0:
            mem = np.zeros(1, dtype=np.uint32)
        self._check(self._lib.pe_set_committees(self._h, epoch, off.size - 1, _ptr(off, C.c_uint32),
                                                _ptr(mem, C.c_uint32)))

    def compute_committees(self, epoch: int, seed: bytes, active_indices, n_committees: int,
                           shuffle_round_count: int = 90, want_result: bool = True):
        """compute_committee / compute_shuffled_index (pe:495-534) for the whole epoch on the GPU; registers the
        table for `epoch` (it stays on the device).  active_indices: the index array, or an int n meaning validators
        0 .. n - 1, or ACTIVE_RESIDENT (the list of the last ``active_set``).  -> (offsets uint32[C+1], members
        uint32[n_active]) when want_result, else nothing is read back."""
        act, n_act = self._active_arg(active_indices)
        off = np.empty(n_committees + 1, dtype=np.uint32) if want_result else None
        mem = np.empty(max(n_act, 1), dtype=np.uint32) if want_result else None
        self._check(self._lib.pe_compute_committees(self._h, epoch, _root(seed), _ptr(act, C.c_uint32), n_act,
                                                    n_committees, shuffle_round_count, _ptr(off, C.c_uint32),
                                                    _ptr(mem, C.c_uint32)))
        return (off, mem[:n_act]) if want_result else None

    def compute_committees_async(self, epoch: int, seed: bytes, n_active: int, n_committees: int,
                                 shuffle_round_count: int = 90):
        """pe_compute_committees_async over validators 0 .. n_active - 1, or over the list of the last ``active_set``
        (n_active = ACTIVE_RESIDENT): enqueued on the state-transition stream, nothing waited for or read back; the table
        is usable by the calls that follow."""
        act, n_act = self._active_arg(n_active)
        rc = self._lib.pe_compute_committees_async(self._h, epoch, _root(seed), _ptr(act, C.c_uint32), n_act, n_committees,
                                                   shuffle_round_count)
        if rc:
            self._check(rc)

    # -- hot path ---------------------------------------------------------
    def get_head(self) -> bytes:
        out = (C.c_uint8 * 32)()
        self._check(self._lib.pe_get_head(self._h, out))
        return bytes(out)

    def get_head_async(self) -> np.ndarray:
        """pe_get_head_async: -> a 32-byte array that holds the root once the pipeline's outputs are complete (inside a
        pipeline nothing waits; outside one the call is synchronous)."""
        (out,), (p_out,) = self._outs("head", ((32, _U8),))
        if self._pipe_keep is not None:
            self._pipe_keep.append(out)
        rc = self._lib.pe_get_head_async(self._h, p_out)
        if rc:
            self._check(rc)
        return out

    def get_weights(self) -> np.ndarray:
        n = self.num_blocks
        out = np.zeros(n, dtype=np.uint64)
        self._check(self._lib.pe_get_weights(self._h, _ptr(out, C.c_uint64), n))
        return out

    def last_weights(self) -> np.ndarray:
        """Per-block weights left behind by the last head computation (get_head / head_from_weights), not recomputed."""
        n = self.num_blocks
        out = np.zeros(n, dtype=np.uint64)
        self._check(self._lib.pe_get_last_weights(self._h, _ptr(out, C.c_uint64), n))
        return out

    def on_attestation_batch(self, rows=None, packed=None, want_aggregate_pubkeys=False, cap: int = 0):
        """-> (status int32[n], aggpk (n,96) u8 or None, count uint32[n]).
        ``packed=(ROWS_RESIDENT, RESIDENT), cap=c``: every group of the last aggregate over DeviceRows; the arrays hold c
        entries (c >= the groups formed; entries past them read 0)."""
        arr, arena = packed if packed is not None else pack_attestations(rows)
        if arr is ROWS_RESIDENT:
            assert arena is RESIDENT and cap > 0 and not want_aggregate_pubkeys
            (status, count), (p_status, p_count) = self._outs("ratt", ((cap, _I32), (cap, _U32)))
            if self._pipe_keep is not None:
                self._pipe_keep.append((status, count))
            rc = self._lib.pe_on_attestation_batch(self._h, _abi.PE_ROWS_RESIDENT, cap, _abi.PE_BITS_RESIDENT, 0, p_status,
                                                   None, p_count)
            if rc:
                self._check(rc)
            return status, None, count
        n = len(rows) if rows is not None else len(arr)
        m = max(n, 1)
        (status, count, agg), (p_status, p_count, p_agg) = self._outs(
            "att", ((m, _I32), (m, _U32), ((m, 96), _U8) if want_aggregate_pubkeys else None))
        arena_p = _abi.PE_BITS_RESIDENT if arena is RESIDENT else _ptr(arena, C.c_uint8)
        if self._pipe_keep is not None:
            self._pipe_keep.append((arr, status, count, agg))
        rc = self._lib.pe_on_attestation_batch(self._h, _att_ptr(arr), n, arena_p, arena.size, p_status, p_agg, p_count)
        if rc:
            self._check(rc)
        return status[:n], (agg[:n] if agg is not None else None), count[:n]

    # -- slashing detection (pe:1128, pe:1134-1143) -------------------------
    def validator_flags(self) -> np.ndarray:
        """pe_get_validator_flags: the flag byte of every validator, PE_VAL_EQUIVOCATING included."""
        n = self.num_validators
        out = np.zeros(max(n, 1), dtype=np.uint8)
        self._check(self._lib.pe_get_validator_flags(self._h, _ptr(out), n))
        return out[:n]

    def slasher_enable(self, history_epochs: int, max_data_per_epoch: int = 4096):
        """pe_slasher_enable: a history of the first vote per validator and target epoch over ``history_epochs`` epochs
        (12 bytes per validator and epoch in device memory), at most ``max_data_per_epoch`` distinct AttestationData per
        epoch.  After set_validators; drops an earlier history."""
        self._check(self._lib.pe_slasher_enable(self._h, int(history_epochs), int(max_data_per_epoch)))

    def slasher_disable(self):
        self._check(self._lib.pe_slasher_disable(self._h))

    def slasher_ingest(self, rows=None, packed=None, current_epoch: int = 0, apply: bool = False, cap: int = 4096,
                       cap_rows: int = 0):
        """pe_slasher_ingest -> (status int32[n], evidence): ``evidence`` = the first min(cap, found) pieces as a structured
        array (SLASH_EVIDENCE_DTYPE: validator, kind, target_epoch_1, id_1, target_epoch_2, id_2; ids resolve through
        slasher_data); ``self.slasher_found`` = the number found, which may exceed cap.  ``apply``: every validator with
        evidence joins store.equivocating_indices on the device (PE_SLASH_APPLY).  ``packed=(rows, RESIDENT)``: rows of
        the last aggregate's result, their OR-ed bits used where they lie.  ``packed=(ROWS_RESIDENT, RESIDENT),
        cap_rows=c``: every group of the last aggregate over DeviceRows, in group order; status holds c entries (c >= the
        groups formed; entries past them read 0)."""
        arr, arena = packed if packed is not None else pack_attestations(rows)
        evidence = np.zeros(max(int(cap), 1), dtype=SLASH_EVIDENCE_DTYPE)
        found = C.c_uint32(0)
        if arr is ROWS_RESIDENT:
            status = np.zeros(max(int(cap_rows), 1), dtype=np.int32)
            self._check(self._lib.pe_slasher_ingest(
                self._h, _abi.PE_ROWS_RESIDENT, int(cap_rows), _abi.PE_BITS_RESIDENT if arena is RESIDENT else _ptr(arena, C.c_uint8),
                0, int(current_epoch), _abi.PE_SLASH_APPLY if apply else 0, _ptr(status), _ptr(evidence), int(cap),
                C.addressof(found)))
            self.slasher_found = int(found.value)
            return status[:int(cap_rows)], evidence[:min(int(cap), self.slasher_found)]
        n = len(rows) if rows is not None else len(arr)
        status = np.zeros(max(n, 1), dtype=np.int32)
        arena_p = _abi.PE_BITS_RESIDENT if arena is RESIDENT else _ptr(arena, C.c_uint8)
        self._check(self._lib.pe_slasher_ingest(self._h, _att_ptr(arr), n, arena_p, arena.size, int(current_epoch),
                                                _abi.PE_SLASH_APPLY if apply else 0, _ptr(status), _ptr(evidence), int(cap),
                                                C.addressof(found)))
        self.slasher_found = int(found.value)
        return status[:n], evidence[:min(int(cap), self.slasher_found)]

    def slasher_data(self, target_epoch: int, data_id: int) -> np.ndarray:
        """pe_slasher_get_data -> one ATT_DTYPE row whose leading 128 bytes are the AttestationData behind the id."""
        out = np.zeros(1, dtype=_ATT_DTYPE)
        self._check(self._lib.pe_slasher_get_data(self._h, int(target_epoch), int(data_id), _ptr(out)))
        return out[0]

    def slasher_records(self, target_epoch: int):
        """pe_slasher_get_records -> (source_epoch uint32[n_val], data id uint32[n_val]); 0xFFFFFFFF = no record."""
        n = self.num_validators
        src = np.empty(max(n, 1), dtype=np.uint32)
        ids = np.empty(max(n, 1), dtype=np.uint32)
        self._check(self._lib.pe_slasher_get_records(self._h, int(target_epoch), _ptr(src), _ptr(ids), n))
        return src[:n], ids[:n]

    def get_indexed_attestations(self, rows=None, packed=None):
        """get_indexed_attestation x n (A.6): -> (status int32[n], offsets uint32[n+1], sorted attesting indices)."""
        arr, arena = packed if packed is not None else pack_attestations(rows)
        n = len(rows) if rows is not None else len(arr)
        status = np.empty(max(n, 1), dtype=np.int32)
        offsets = np.empty(n + 1, dtype=np.uint32)
        cap = int(sum(int(r.bits.size) for r in rows)) if rows is not None else int(arr["n_bits"].sum())
        indices = np.empty(max(cap, 1), dtype=np.uint32)
        self._check(self._lib.pe_get_indexed_attestations(self._h, _att_ptr(arr), n, _ptr(arena, C.c_uint8), arena.size,
                                                          _ptr(status, C.c_int32), _ptr(offsets, C.c_uint32),
                                                          _ptr(indices, C.c_uint32), indices.size))
        return status[:n], offsets, indices[:int(offsets[-1])]

    def aggregate(self, rows=None, packed=None, sig_points96=None, want_aggregate_pubkeys=False, sig_points192=None):
        """-> AggregateResult(n_groups, atts (ATT_DTYPE rows of the groups), group_of, out_arena, sig96, aggpk96,
        count; ``["bits"]`` decodes the OR-ed bitfields on demand).  sig_points192: the members' signatures as G2
        points (192-byte uncompressed BLSSignature, pe:717); their per-group sums come back as ``sig192``
        (pe_g2_sum over pe_aggregate's grouping)."""
        arr, arena = packed if packed is not None else pack_attestations(rows)
        n = len(rows) if rows is not None else len(arr)
        m = max(n, 1)
        self._signed_device_rows = 0   # verify_resident follows an aggregate_signed, not this
        if arr.__class__ is DeviceRows:  # rows in device memory: grouped / resolved / validated there
            assert sig_points96 is None and sig_points192 is None, "signature points take host rows"
            (out_atts, group_of, out_arena, out_pk, count, ng), (p_atts, p_gof, p_arena, p_pk, p_count, p_ng) = self._outs(
                "ragg", ((m, _ATT_DTYPE), (m, _U32), (max(arena.size, 1), _U8),
                         ((m, 96), _U8) if want_aggregate_pubkeys else None, (m, _U32), (1, _U32)))
            ng[0] = 0
            if self._pipe_keep is not None:
                self._pipe_keep.append((arr, arena, out_atts, group_of, out_arena, out_pk, count, ng))
            rc = self._lib.pe_aggregate(self._h, arr.ptr, n, _ptr(arena, C.c_uint8), arena.size, None, p_atts, p_ng, p_gof,
                                        p_arena, out_arena.size, None, p_pk, p_count)
            if rc:
                self._check(rc)
            return ResidentAggregateResult(_raw=dict(n_groups=ng, atts=out_atts, group_of=group_of, out_arena=out_arena,
                                                     aggpk96=out_pk, count=count), sig96=None, sig192=None)
        sig = None
        if sig_points96 is not None:
            sig = np.ascontiguousarray(sig_points96, dtype=np.uint8)
            assert sig.size == 96 * n
        # output buffers: written by the engine, never read before that.  "tail" receives (offset, n_bits) of the last
        # group's bits through two of the row fields the C side fills in, read back as plain u32s below
        (out_atts, group_of, out_arena, out_sig, out_pk, count), (p_atts, p_gof, p_arena, p_sig, p_pk, p_count) = self._outs(
            "agg", ((m, _ATT_DTYPE), (m, _U32), (max(arena.size, 1), _U8), ((m, 96), _U8) if sig is not None else None,
                    ((m, 96), _U8) if want_aggregate_pubkeys else None, (m, _U32)))
        n_groups = C.c_uint32(0)
        if self._pipe_keep is not None:
            self._pipe_keep.append((arr, arena, sig, out_atts, group_of, out_arena, out_sig, out_pk, count))
        rc = self._lib.pe_aggregate(self._h, _att_ptr(arr), n, _ptr(arena, C.c_uint8), arena.size, _ptr(sig, C.c_uint8),
                                    p_atts, C.byref(n_groups), p_gof, p_arena, out_arena.size, p_sig, p_pk, p_count)
        if rc:
            self._check(rc)
        g = n_groups.value
        if g:  # the groups' unions are laid out back to back: hand back only the written part of the arena
            tail = out_atts.view(np.uint32).reshape(-1, 36)[g - 1]   # u32 words 32 / 33 of a row: bits_offset, n_bits
            out_arena = out_arena[: int(tail[32]) + (int(tail[33]) + 7) // 8]
        sig192 = None
        if sig_points192 is not None:
            s2 = np.ascontiguousarray(sig_points192, dtype=np.uint8)
            assert s2.size == 192 * n
            order = np.argsort(group_of[:n], kind="stable").astype(np.uint32)   # members of a group in input order
            offs = np.concatenate([[0], np.cumsum(np.bincount(group_of[:n], minlength=g))]).astype(np.uint32)
            sig192 = self.g2_sum(s2, offs, index=order)
        return AggregateResult(n_groups=g, atts=out_atts[:g], group_of=group_of[:n], out_arena=out_arena,
                               sig96=None if out_sig is None else out_sig[:g], sig192=sig192,
                               aggpk96=None if out_pk is None else out_pk[:g], count=count[:g])

    def aggregate_signed(self, signatures, rows=None, packed=None, compressed: bool = True, check_subgroup: bool = False,
                         want_aggregate_pubkeys: bool = False):
        """pe_aggregate_signed: pe_aggregate plus bls.Aggregate over the members' BLSSignatures (pe:659, pe:714-717).
        signatures: (n, 96) compressed or (n, 192) uncompressed uint8 (or a DeviceArena holding them).  -> the aggregate
        result with ``sig96c`` ((groups, 96) uint8: the compressed aggregate signature of every group) and ``sig_status``
        (int32[n]: PE_SIG_* per input row).  Host rows or DeviceRows, synchronous or inside a pipeline, as aggregate()."""
        arr, arena = packed if packed is not None else pack_attestations(rows)
        n = len(rows) if rows is not None else len(arr)
        m = max(n, 1)
        fmt = (_abi.PE_SIG_G2_COMPRESSED if compressed else _abi.PE_SIG_G2_UNCOMPRESSED) | (
            _abi.PE_SIG_CHECK_SUBGROUP if check_subgroup else 0)
        sig = signatures if signatures.__class__ is DeviceArena else np.ascontiguousarray(signatures, dtype=np.uint8)
        assert sig.size == (96 if compressed else 192) * n, "one signature per input row"
        dev = arr.__class__ is DeviceRows
        (out_atts, group_of, out_arena, out_pk, count, ng, osig, sst), (p_atts, p_gof, p_arena, p_pk, p_count, p_ng, p_osig,
                                                                       p_sst) = self._outs(
            "saggd" if dev else "sagg", ((m, _ATT_DTYPE), (m, _U32), (max(arena.size, 1), _U8),
                                         ((m, 96), _U8) if want_aggregate_pubkeys else None, (m, _U32), (1, _U32),
                                         ((m, 96), _U8), (m, _I32)))
        ng[0] = 0
        self._signed_device_rows = 0
        if self._pipe_keep is not None:
            self._pipe_keep.append((arr, arena, sig, out_atts, group_of, out_arena, out_pk, count, ng, osig, sst))
        rc = self._lib.pe_aggregate_signed(self._h, arr.ptr if dev else _att_ptr(arr), n, _ptr(arena, C.c_uint8), arena.size,
                                           _ptr(sig, C.c_uint8), fmt, p_atts, p_ng, p_gof, p_arena, out_arena.size, p_osig,
                                           p_sst, p_pk, p_count)
        if rc:
            self._check(rc)
        self._signed_device_rows = n if dev else 0
        return ResidentAggregateResult(_raw=dict(n_groups=ng, atts=out_atts, group_of=group_of, out_arena=out_arena,
                                                 aggpk96=out_pk, count=count, sig96c=osig, sig_status=sst[:n]),
                                       sig96=None, sig192=None)

    def g2_subgroup_check(self, points192) -> np.ndarray:
        """pe_g2_subgroup_check: int32[n], 0 = in G2 (r * P = infinity), 3 = not."""
        pts = np.ascontiguousarray(points192, dtype=np.uint8).reshape(-1, 192)
        st = np.zeros(max(len(pts), 1), dtype=np.int32)
        self._check(self._lib.pe_g2_subgroup_check(self._h, _ptr(pts, C.c_uint8), len(pts), _ptr(st, C.c_int32)))
        return st[:len(pts)]

    @staticmethod
    def _pair_args(g1_points96, g2_points192, offsets):
        g1 = np.ascontiguousarray(g1_points96, dtype=np.uint8).reshape(-1, 96)
        g2 = np.ascontiguousarray(g2_points192, dtype=np.uint8).reshape(-1, 192)
        off = np.ascontiguousarray(offsets, dtype=np.uint32)
        if len(g1) != len(g2) or off.size < 1:
            raise ValueError("one G2 point per G1 point, and n_groups + 1 offsets")
        return g1, g2, off

    def pairing_check(self, g1_points96, g2_points192, offsets) -> np.ndarray:
        """pe_pairing_check: int32[n_groups]; 1 = the product of e(P_j, Q_j) over the group's pairs is 1, 0 = it is not,
        2 = a point of the group is off its curve.  An empty group gives 1; infinity on either side contributes 1."""
        g1, g2, off = self._pair_args(g1_points96, g2_points192, offsets)
        verdict = np.zeros(max(off.size - 1, 1), dtype=np.int32)
        self._check(self._lib.pe_pairing_check(self._h, _ptr(g1, C.c_uint8), _ptr(g2, C.c_uint8), len(g1), _ptr(off, C.c_uint32),
                                               off.size - 1, _ptr(verdict, C.c_int32)))
        return verdict[:off.size - 1]

    def fast_aggregate_verify(self, index, offsets, message_points192, signatures192) -> np.ndarray:
        """pe_fast_aggregate_verify: int32[n_groups]; per group the registry pubkeys index[offsets[g]:offsets[g+1]] are summed
        on the device and e(sum, message_points192[g]) == e(g1, signatures192[g]) is checked.  1 valid, 0 not (also: empty
        group, identity signature), 2 = a point off its curve.  The message point H(m) is the caller's."""
        idx = np.ascontiguousarray(index, dtype=np.uint32)
        off = np.ascontiguousarray(offsets, dtype=np.uint32)
        msg = np.ascontiguousarray(message_points192, dtype=np.uint8).reshape(-1, 192)
        sig = np.ascontiguousarray(signatures192, dtype=np.uint8).reshape(-1, 192)
        n_groups = off.size - 1
        if n_groups < 0 or len(msg) != n_groups or len(sig) != n_groups or (n_groups and idx.size < int(off[-1])):
            raise ValueError("n_groups + 1 offsets, one message point and one signature per group, offsets[-1] indices")
        verdict = np.zeros(max(n_groups, 1), dtype=np.int32)
        self._check(self._lib.pe_fast_aggregate_verify(self._h, _ptr(idx, C.c_uint32) if idx.size else None, _ptr(off, C.c_uint32),
                                                       n_groups, _ptr(msg, C.c_uint8), _ptr(sig, C.c_uint8),
                                                       _ptr(verdict, C.c_int32)))
        return verdict[:n_groups]

    @staticmethod
    def _batch_scalars(scalars, n_groups):
        if scalars is None:
            return None, None
        r = np.ascontiguousarray(scalars, dtype=np.uint64)
        if r.size != n_groups:
            raise ValueError("one scalar per group (verify_signatures: per member)")
        return r, (_ptr(r, C.c_uint64) if r.size else None)

    def batch_verify(self, pubkeys96, message_points192, signatures192, scalars=None) -> np.ndarray:
        """pe_batch_verify: int32[n_groups], the verdicts of fast_aggregate_verify for groups given by their aggregate pubkey,
        reached by random linear combination: one final exponentiation for the whole call when every group is valid.
        ``scalars=None`` (production): the engine draws secret 64-bit scalars.  Scalars the signers can predict let a pair of
        forged signatures pass; a signature outside G2 gives 0."""
        pk = np.ascontiguousarray(pubkeys96, dtype=np.uint8).reshape(-1, 96)
        msg = np.ascontiguousarray(message_points192, dtype=np.uint8).reshape(-1, 192)
        sig = np.ascontiguousarray(signatures192, dtype=np.uint8).reshape(-1, 192)
        n_groups = len(pk)
        if len(msg) != n_groups or len(sig) != n_groups:
            raise ValueError("one pubkey, one message point and one signature per group")
        r, r_ptr = self._batch_scalars(scalars, n_groups)
        verdict = np.zeros(max(n_groups, 1), dtype=np.int32)
        self._check(self._lib.pe_batch_verify(self._h, _ptr(pk, C.c_uint8), _ptr(msg, C.c_uint8), _ptr(sig, C.c_uint8), n_groups,
                                              r_ptr, _ptr(verdict, C.c_int32)))
        return verdict[:n_groups]

    def batch_fast_aggregate_verify(self, index, offsets, message_points192, signatures192, scalars=None) -> np.ndarray:
        """pe_batch_fast_aggregate_verify: fast_aggregate_verify's arguments and verdicts, decided as batch_verify decides."""
        idx = np.ascontiguousarray(index, dtype=np.uint32)
        off = np.ascontiguousarray(offsets, dtype=np.uint32)
        msg = np.ascontiguousarray(message_points192, dtype=np.uint8).reshape(-1, 192)
        sig = np.ascontiguousarray(signatures192, dtype=np.uint8).reshape(-1, 192)
        n_groups = off.size - 1
        if n_groups < 0 or len(msg) != n_groups or len(sig) != n_groups or (n_groups and idx.size < int(off[-1])):
            raise ValueError("n_groups + 1 offsets, one message point and one signature per group, offsets[-1] indices")
        r, r_ptr = self._batch_scalars(scalars, n_groups)
        verdict = np.zeros(max(n_groups, 1), dtype=np.int32)
        self._check(self._lib.pe_batch_fast_aggregate_verify(self._h, _ptr(idx, C.c_uint32) if idx.size else None,
                                                             _ptr(off, C.c_uint32), n_groups, _ptr(msg, C.c_uint8),
                                                             _ptr(sig, C.c_uint8), r_ptr, _ptr(verdict, C.c_int32)))
        return verdict[:n_groups]

    def verify_signatures(self, signatures, signer, offsets, message_points192, index=None, scalars=None, aggregates=True):
        """pe_verify_signatures: every unaggregated signature of an epoch decided, one pairing check per group.  Group g is the
        members [offsets[g], offsets[g+1]) -- one committee's votes for one AttestationData, so one message point
        message_points192[g] --, member j is signed by validator signer[j] with signatures[index[j]] (index=None: signatures[j]).
        signatures: (n, 96) uint8 array or a DeviceArena of n * 96 bytes.  ``scalars=None`` (production): the engine draws one
        secret 64-bit weight per member; weights the signers can predict let a cancelling pair of forged signatures pass.
        -> (member_verdict int32 (members,): 1 valid, 0 not;  sig_status int32 (members,): 0 ok, 1 malformed, 2 off the curve,
        3 outside G2, 4 the identity;  group_verdict int32 (n_groups,): 1 iff every member is valid, 2 = H(m) off its curve;
        aggregates (n_groups, 96) uint8: per group the compressed sum of the valid members' signatures, or None)."""
        off = np.ascontiguousarray(offsets, dtype=np.uint32)
        n_groups = off.size - 1
        who = np.ascontiguousarray(signer, dtype=np.uint32)
        msg = np.ascontiguousarray(message_points192, dtype=np.uint8).reshape(-1, 192)
        members = int(off[-1]) if n_groups > 0 else 0
        if n_groups < 0 or len(msg) != n_groups or who.size != members:
            raise ValueError("n_groups + 1 offsets, one message point per group, one signer per member")
        if isinstance(signatures, DeviceArena):
            sig_ptr, n = signatures.ptr, signatures.size // 96
        else:
            sig = np.ascontiguousarray(signatures, dtype=np.uint8)
            sig_ptr, n = sig.ctypes.data, sig.size // 96
        idx = None if index is None else np.ascontiguousarray(index, dtype=np.uint32)
        if idx is not None and idx.size != members:
            raise ValueError("one index per member")
        r, r_ptr = self._batch_scalars(scalars, members)
        verdict = np.zeros(max(members, 1), dtype=np.int32)
        status = np.zeros(max(members, 1), dtype=np.int32)
        group = np.zeros(max(n_groups, 1), dtype=np.int32)
        out = np.zeros((max(n_groups, 1), 96), dtype=np.uint8) if aggregates else None
        self._check(self._lib.pe_verify_signatures(
            self._h, C.c_void_p(sig_ptr), n, _ptr(idx, C.c_uint32) if idx is not None and idx.size else None,
            _ptr(who, C.c_uint32) if who.size else None, _ptr(off, C.c_uint32), n_groups, _ptr(msg, C.c_uint8) if n_groups else None,
            r_ptr, _ptr(verdict, C.c_int32), _ptr(status, C.c_int32), _ptr(group, C.c_int32),
            _ptr(out, C.c_uint8) if aggregates else None))
        return verdict[:members], status[:members], group[:n_groups], (out[:n_groups] if aggregates else None)

    def hash_to_g2(self, messages, dst: bytes = _abi.ETH2_DST, out: Optional[DeviceArena] = None, want_status: bool = False):
        """pe_hash_to_g2: the message points H(m) of ``messages`` under the tag ``dst`` -- hash_to_curve of RFC 9380, suite
        BLS12381G2_XMD:SHA-256_SSWU_RO_ -- as every BLS call of the engine takes them: (n, 192) uint8, G2 wire form.
        messages: n byte strings of ONE length (0 .. 255), an (n, msg_len) uint8 array, or ``(DeviceArena, msg_len)`` for
        messages that lie in device memory.  ``out``: a DeviceArena of n * 192 bytes -- the points are written there and never
        cross to the host (``verify_resident`` reads them in place); the arena is returned.  ``want_status``: also int32 (n,),
        1 where H(m) is the identity (no message anybody has seen)."""
        if isinstance(messages, tuple) and messages[0].__class__ is DeviceArena:
            arena, msg_len = messages[0], int(messages[1])
            n = arena.size // msg_len if msg_len else 0
            msg_ptr = arena.ptr
        else:
            if isinstance(messages, np.ndarray):
                m = np.ascontiguousarray(messages, dtype=np.uint8)
                m = m.reshape(len(m), -1) if m.ndim != 2 else m
            else:
                rows = [bytes(x) for x in messages]
                if len({len(x) for x in rows}) > 1:
                    raise ValueError("hash_to_g2: the messages of one call have one length")
                m = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), len(rows[0]) if rows else 0)
            n, msg_len = m.shape
            msg_ptr = m.ctypes.data if m.size else None
        dst_arr = np.frombuffer(bytes(dst), dtype=np.uint8)
        if out is not None and out.size < 192 * n:
            raise ValueError("hash_to_g2: the output arena is smaller than n * 192 bytes")
        pts = None if out is not None else np.zeros((max(n, 1), 192), dtype=np.uint8)
        status = np.zeros(max(n, 1), dtype=np.int32) if want_status else None
        self._check(self._lib.pe_hash_to_g2(self._h, C.c_void_p(msg_ptr), n, msg_len, _ptr(dst_arr) if dst_arr.size else None,
                                            dst_arr.size, C.c_void_p(out.ptr) if out is not None else _ptr(pts),
                                            _ptr(status) if want_status else None))
        res = out if out is not None else pts[:n]
        return (res, status[:n]) if want_status else res

    def map_to_g2(self, u) -> np.ndarray:
        """pe_map_to_g2: n x (u0, u1) -> (n, 192) uint8 points of G2: map_to_curve of both, their sum, clear_cofactor (RFC 9380's
        steps behind hash_to_field).  u: (n, 192) uint8 -- u0.c0 | u0.c1 | u1.c0 | u1.c1, 48-byte big-endian words below p."""
        ub = np.ascontiguousarray(u, dtype=np.uint8).reshape(-1, 192)
        n = len(ub)
        pts = np.zeros((max(n, 1), 192), dtype=np.uint8)
        self._check(self._lib.pe_map_to_g2(self._h, _ptr(ub) if n else None, n, _ptr(pts)))
        return pts[:n]

    def verify_resident(self, message_points192, point_of_row=None, apply: bool = True, cap: Optional[int] = None) -> np.ndarray:
        """pe_verify_resident: int32[n_groups], one verdict per group of the last ``aggregate_signed`` over DeviceRows with
        ``want_aggregate_pubkeys=True``, from the aggregate keys and signatures that call left in device memory: 1 valid,
        0 not (also: overlapping members, a member that did not decode, an empty union, an identity signature or message
        point, an aggregate signature outside G2), 2 = the message point is off its curve, 3 = the group has no committee.
        message_points192: (n_points, 192) uint8 H(m), or a DeviceArena holding them; point_of_row: one point index per input
        row of that aggregate (its group takes the point of its first row), None: group g takes point g.  ``apply``: the
        verdict is ANDed into the groups' signature flag on the device, so that on_attestation_batch /
        process_attestation_batch with (ROWS_RESIDENT, RESIDENT) answer PE_ATT_BAD_SIGNATURE for what did not verify.
        ``cap``: entries of the verdict array handed to the library (default: that aggregate's input rows, which bound its groups)."""
        if message_points192.__class__ is DeviceArena:
            msg_ptr, n_points = message_points192.ptr, message_points192.size // 192
        else:
            msg = np.ascontiguousarray(message_points192, dtype=np.uint8).reshape(-1, 192)
            msg_ptr, n_points = msg.ctypes.data, len(msg)
        por = None if point_of_row is None else np.ascontiguousarray(point_of_row, dtype=np.uint32)
        rows = self._signed_device_rows  # input rows of the last aggregate_signed over DeviceRows: bounds its groups
        if por is not None and por.size != rows:
            raise ValueError("one point index per input row of the resident aggregate")
        cap = rows if cap is None else int(cap)
        verdict = np.zeros(max(cap, 1), dtype=np.int32)
        self._check(self._lib.pe_verify_resident(self._h, C.c_void_p(msg_ptr), n_points, _ptr(por, C.c_uint32) if por is not None else None,
                                                 _abi.PE_VERIFY_APPLY if apply else 0, cap, _ptr(verdict, C.c_int32)))
        return verdict[:self._profile_verify_resident_stats()["groups"]]

    @staticmethod
    def _attester_domains(fork_epoch: int, domain_previous: bytes, domain_current: bytes) -> "_abi.pe_attester_domains":
        if len(domain_previous) != 32 or len(domain_current) != 32:
            raise ValueError("a domain is 32 bytes")
        dom = _abi.pe_attester_domains()
        dom.fork_epoch = int(fork_epoch)
        dom.domain_previous[:] = bytes(domain_previous)
        dom.domain_current[:] = bytes(domain_current)
        return dom

    def attestation_signing_roots(self, rows, fork_epoch: int, domain_previous: bytes, domain_current: bytes,
                                  out: Optional[DeviceArena] = None):
        """pe_attestation_signing_roots: (n, 32) uint8, compute_signing_root(AttestationData of row i, domain) -- the messages
        attestation signatures are over, as ``hash_to_g2`` takes them -- with ``domain_current`` where the row's target epoch
        is at or past ``fork_epoch`` and ``domain_previous`` before it (get_domain).  rows: a structured array of
        pe_attestation (synth.ATT_DTYPE), a ctypes array of them, a list of AttRow, or DeviceRows.  ``out``: a DeviceArena of
        n * 32 bytes -- the roots are written there and never cross to the host; the arena is returned."""
        if rows.__class__ is DeviceRows:
            n, row_ptr = rows.n, rows.ptr
        else:
            if not isinstance(rows, np.ndarray) and len(rows) and isinstance(rows[0], AttRow):
                rows = pack_attestations(rows)[0]
            n = len(rows)
            row_ptr = (_att_ptr(rows) if isinstance(rows, np.ndarray) else C.addressof(rows)) if n else None
        if out is not None and out.size < 32 * n:
            raise ValueError("attestation_signing_roots: the output arena is smaller than n * 32 bytes")
        dom = self._attester_domains(fork_epoch, domain_previous, domain_current)
        roots = None if out is not None else np.zeros((max(n, 1), 32), dtype=np.uint8)
        self._check(self._lib.pe_attestation_signing_roots(self._h, C.c_void_p(row_ptr), n, C.byref(dom),
                                                           C.c_void_p(out.ptr) if out is not None else _ptr(roots)))
        return out if out is not None else roots[:n]

    def verify_resident_data(self, fork_epoch: int, domain_previous: bytes, domain_current: bytes, apply: bool = True,
                             cap: Optional[int] = None, want_roots: bool = True):
        """pe_verify_resident_data: ``verify_resident`` with every group's message taken from the group's own
        AttestationData -- its signing root under get_domain(DOMAIN_BEACON_ATTESTER, target epoch), hashed to G2 under
        Ethereum's tag -- all on the device.  Returns (int32[n_groups] verdicts as verify_resident's, (n_groups, 32) uint8
        signing roots in group order, or None without ``want_roots``)."""
        dom = self._attester_domains(fork_epoch, domain_previous, domain_current)
        cap = self._signed_device_rows if cap is None else int(cap)
        verdict = np.zeros(max(cap, 1), dtype=np.int32)
        roots = np.zeros((max(cap, 1), 32), dtype=np.uint8) if want_roots else None
        self._check(self._lib.pe_verify_resident_data(self._h, C.byref(dom), _abi.PE_VERIFY_APPLY if apply else 0, cap,
                                                      _ptr(verdict, C.c_int32), _ptr(roots) if want_roots else None))
        ng = self._profile_verify_resident_stats()["groups"]
        return verdict[:ng], (roots[:ng] if want_roots else None)

    def _profile_verify_resident_stats(self) -> dict:
        """pe_profile_verify_resident_stats: how the last verify_resident decided its groups, by row of the rule table."""
        out = np.zeros(_abi.PE_VERIFY_RESIDENT_STATS, dtype=np.uint32)
        self._check(self._lib.pe_profile_verify_resident_stats(self._h, _ptr(out, C.c_uint32)))
        names = ("no_committee", "bad_message", "overlap", "bad_member", "empty_key", "identity_signature", "identity_message",
                 "not_g2", "pairing", "subgroup_pass", "groups")
        return dict(zip(names, (int(v) for v in out)))

    def _profile_verify_set_stripe(self, k: int) -> None:
        """pe_profile_verify_set_stripe: k, the members of one slot of verify_signatures' weighted sums."""
        self._check(self._lib.pe_profile_verify_set_stripe(self._h, int(k)))

    def _profile_verify_stats(self) -> dict:
        """pe_profile_verify_stats: what the last verify_signatures did."""
        out = np.zeros(5, dtype=np.uint32)
        self._check(self._lib.pe_profile_verify_stats(self._h, _ptr(out, C.c_uint32)))
        return dict(zip(("settled", "failed_groups", "rechecked", "pairing_runs", "k"), (int(v) for v in out)))

    def _profile_verify_sums(self, n_groups: int):
        """pe_profile_verify_sums: the last verify_signatures' weighted sums per group, (n_groups, 96) and (n_groups, 192)."""
        pk = np.zeros((max(n_groups, 1), 96), dtype=np.uint8)
        sig = np.zeros((max(n_groups, 1), 192), dtype=np.uint8)
        self._check(self._lib.pe_profile_verify_sums(self._h, int(n_groups), _ptr(pk, C.c_uint8), _ptr(sig, C.c_uint8)))
        return pk[:n_groups], sig[:n_groups]

    def _profile_batch_set_chunk(self, chunk: int) -> None:
        """pe_profile_batch_set_chunk: c, the live groups of one chunk of the batch calls."""
        self._check(self._lib.pe_profile_batch_set_chunk(self._h, int(chunk)))

    def _profile_batch_stats(self) -> dict:
        """pe_profile_batch_stats: what the last batch call did."""
        out = np.zeros(8, dtype=np.uint32)
        self._check(self._lib.pe_profile_batch_stats(self._h, _ptr(out, C.c_uint32)))
        names = ("live", "chunks", "product_launches", "top_exps", "fallback_exps", "rechecked", "c", "F")
        return dict(zip(names, (int(v) for v in out)))

    def _profile_batch_gt(self) -> bytes:
        """pe_profile_batch_gt: the 576 bytes the last batch call's top-level verdict compared with 1."""
        out = np.zeros(576, dtype=np.uint8)
        self._check(self._lib.pe_profile_batch_gt(self._h, _ptr(out, C.c_uint8)))
        return out.tobytes()

    def _profile_pairing_gt(self, g1_points96, g2_points192, offsets) -> np.ndarray:
        """pe_profile_pairing_gt (parity tests only): uint8[n_groups, 576], the value each verdict compares with 1."""
        g1, g2, off = self._pair_args(g1_points96, g2_points192, offsets)
        out = np.zeros((max(off.size - 1, 1), 576), dtype=np.uint8)
        self._check(self._lib.pe_profile_pairing_gt(self._h, _ptr(g1, C.c_uint8), _ptr(g2, C.c_uint8), len(g1),
                                                    _ptr(off, C.c_uint32), off.size - 1, _ptr(out, C.c_uint8)))
        return out[:off.size - 1]

    def process_attestation_batch(self, state_ctx: pe_state_ctx, rows=None, packed=None, cap: int = 0):
        """-> (status int32[n], proposer_reward_numerator uint64[n]).  ``packed=(ROWS_RESIDENT, RESIDENT), cap=c`` as for
        on_attestation_batch."""
        arr, arena = packed if packed is not None else pack_attestations(rows)
        if arr is ROWS_RESIDENT:
            assert arena is RESIDENT and cap > 0
            (status, num), (p_status, p_num) = self._outs("rproc", ((cap, _I32), (cap, _U64)))
            if self._pipe_keep is not None:
                self._pipe_keep.append((status, num))
            rc = self._lib.pe_process_attestation_batch(self._h, C.byref(state_ctx), _abi.PE_ROWS_RESIDENT, cap,
                                                        _abi.PE_BITS_RESIDENT, 0, p_status, p_num)
            if rc:
                self._check(rc)
            return status, num
        n = len(rows) if rows is not None else len(arr)
        m = max(n, 1)
        (status, num), (p_status, p_num) = self._outs("proc", ((m, _I32), (m, _U64)))
        arena_p = _abi.PE_BITS_RESIDENT if arena is RESIDENT else _ptr(arena, C.c_uint8)
        if self._pipe_keep is not None:
            self._pipe_keep.append((arr, status, num))
        rc = self._lib.pe_process_attestation_batch(self._h, C.byref(state_ctx), _att_ptr(arr), n, arena_p, arena.size,
                                                    p_status, p_num)
        if rc:
            self._check(rc)
        return status[:n], num[:n]

    def participation_set(self, which: int, flags):
        f = np.ascontiguousarray(flags, dtype=np.uint8)
        self._check(self._lib.pe_participation_set(self._h, which, _ptr(f, C.c_uint8), f.size))

    def participation_get(self, which: int) -> np.ndarray:
        out = np.zeros(self.num_validators, dtype=np.uint8)
        self._check(self._lib.pe_participation_get(self._h, which, _ptr(out, C.c_uint8), out.size))
        return out

    def participation_rotate(self):
        self._check(self._lib.pe_participation_rotate(self._h))

    def state_set_validators(self, effective_balance, flags):
        bal = np.ascontiguousarray(effective_balance, dtype=np.uint64)
        fl = np.ascontiguousarray(flags, dtype=np.uint8)
        self._check(self._lib.pe_state_set_validators(self._h, bal.size, _ptr(bal, C.c_uint64), _ptr(fl, C.c_uint8)))

    def ffg_balances(self):
        """-> (total_active_balance, previous_target_balance, current_target_balance) of pe:791-802."""
        out = np.zeros(3, dtype=np.uint64)
        self._check(self._lib.pe_ffg_balances(self._h, _ptr(out, C.c_uint64)))
        return int(out[0]), int(out[1]), int(out[2])

    # -- epoch boundary ----------------------------------------------------
    def _active_arg(self, active_indices):
        """-> (what ``_ptr`` turns into the C argument, n_active) of an ``active_indices`` argument: ACTIVE_RESIDENT (with
        the length ``active_set`` reported), an int n (validators 0 .. n - 1: nothing to upload) or an index array."""
        if active_indices is ACTIVE_RESIDENT:
            return _ACTIVE_RESIDENT_ARG, self._resident_active
        if isinstance(active_indices, (int, np.integer)):
            return None, int(active_indices)
        act = np.ascontiguousarray(active_indices, dtype=np.uint32)
        return act, act.size

    def registry_set_epochs(self, activation_epoch, exit_epoch):
        """Validator.activation_epoch / exit_epoch (pe:43-44) of the whole registry -> device memory."""
        act = np.ascontiguousarray(activation_epoch, dtype=np.uint64)
        ext = np.ascontiguousarray(exit_epoch, dtype=np.uint64)
        assert act.size == ext.size, "one activation and one exit epoch per validator"
        self._check(self._lib.pe_registry_set_epochs(self._h, act.size, _ptr(act if act.size else None, C.c_uint64),
                                                     _ptr(ext if ext.size else None, C.c_uint64)))

    def registry_get_epochs(self):
        """-> (activation_epoch u64[n], exit_epoch u64[n], is_set); is_set False: the handle holds none."""
        n = self.num_validators
        act, ext, is_set = np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint64), C.c_int(0)
        self._check(self._lib.pe_registry_get_epochs(self._h, n, _ptr(act), _ptr(ext), C.addressof(is_set)))
        return act[:n], ext[:n], bool(is_set.value)

    def active_set(self, epoch: int, want_indices: bool = False):
        """get_active_validator_indices(state, epoch) over the resident epochs -> (n_active, total_balance, indices
        uint32[n_active] | None); the list stays on the device for ACTIVE_RESIDENT.  total_balance is
        get_total_active_balance's value for `epoch` over the working-state view."""
        idx = np.empty(max(self.num_validators, 1), dtype=np.uint32) if want_indices else None
        n_active, total = C.c_uint32(0), C.c_uint64(0)
        self._check(self._lib.pe_active_set(self._h, int(epoch), C.addressof(n_active), C.addressof(total),
                                            _ptr(idx, C.c_uint32)))
        self._resident_active = int(n_active.value)
        return int(n_active.value), int(total.value), (idx[:n_active.value] if want_indices else None)

    def state_refresh_activity(self, current_epoch: int):
        """PE_VAL_ACTIVE / PE_VAL_ACTIVE_PREV of the working-state view from the resident epochs."""
        self._check(self._lib.pe_state_refresh_activity(self._h, int(current_epoch)))

    def compute_proposers(self, seeds, active_indices, rounds: int = 90,
                          max_effective_balance: int = 32 * 10**9, max_tries: int = 0):
        """compute_proposer_index (pe:604-618) on the GPU, once per seed, over the working-state view's effective
        balances.  seeds: a sequence of 32-byte seeds (or a uint8 array of n x 32); active_indices: the index array, an
        int n meaning validators 0 .. n - 1, or ACTIVE_RESIDENT.  -> (proposers uint32[n_seeds], tries uint32[n_seeds]); a proposer of
        0xFFFFFFFF (tries == max_tries) means none of the first max_tries candidates (0 = 4096) was accepted."""
        if isinstance(seeds, np.ndarray):
            sd = np.ascontiguousarray(seeds, dtype=np.uint8).reshape(-1)
        else:
            sd = np.frombuffer(b"".join(bytes(s) for s in seeds), dtype=np.uint8)
        assert sd.size % 32 == 0, "seeds are 32 bytes each"
        n_seeds = sd.size // 32
        act, n_act = self._active_arg(active_indices)
        prop = np.empty(max(n_seeds, 1), dtype=np.uint32)
        tries = np.empty(max(n_seeds, 1), dtype=np.uint32)
        self._check(self._lib.pe_compute_proposers(self._h, _ptr(sd if n_seeds else None, C.c_uint8), n_seeds,
                                                   _ptr(act, C.c_uint32), n_act, int(rounds),
                                                   int(max_effective_balance), int(max_tries), _ptr(prop, C.c_uint32),
                                                   _ptr(tries, C.c_uint32)))
        return prop[:n_seeds], tries[:n_seeds]

    # -- sync committees ----------------------------------------------------
    def sync_committee_compute(self, seed: bytes, active_indices, rounds: int = 90, max_effective_balance: int = 32 * 10**9,
                               size: int = _abi.PE_SYNC_COMMITTEE_MAX, max_tries: int = 0):
        """get_next_sync_committee on the GPU (pe_sync_committee_compute): sampled over the working-state view's effective
        balances with compute_proposers' acceptance rule, left resident as the handle's NEXT committee.  active_indices as
        ``compute_proposers`` takes them.  -> (indices uint32[size], aggregate_pubkey bytes[48], tries: the i of the last accepted
        candidate + 1).  EngineError PE_ERR_CAPACITY where max_tries candidates (0 = 2^20) did not yield `size` members."""
        sd = np.frombuffer(bytes(seed), dtype=np.uint8).copy()
        assert sd.size == 32, "a seed is 32 bytes"
        act, n_act = self._active_arg(active_indices)
        idx = np.zeros(_abi.PE_SYNC_COMMITTEE_MAX, dtype=np.uint32)
        key = np.zeros(48, dtype=np.uint8)
        tries = C.c_uint32(0)
        self._check(self._lib.pe_sync_committee_compute(self._h, _ptr(sd, C.c_uint8), _ptr(act, C.c_uint32), n_act, int(rounds),
                                                        int(max_effective_balance), int(size), int(max_tries),
                                                        _ptr(idx, C.c_uint32), _ptr(key, C.c_uint8), C.addressof(tries)))
        return idx[:int(size)], key.tobytes(), int(tries.value)

    def sync_committee_set(self, which: int, indices):
        """Committee `which` (SYNC_CURRENT / SYNC_NEXT) from a list of validator indices, duplicates allowed; its aggregate
        pubkey is computed from the registry (pe_sync_committee_set): genesis, checkpoint / resume."""
        idx = np.ascontiguousarray(indices, dtype=np.uint32)
        self._check(self._lib.pe_sync_committee_set(self._h, int(which), _ptr(idx if idx.size else None, C.c_uint32), idx.size))

    def sync_committee_get(self, which: int):
        """-> (indices uint32[size], aggregate_pubkey bytes[48]) of committee `which`, or None where the handle holds none."""
        idx = np.zeros(_abi.PE_SYNC_COMMITTEE_MAX, dtype=np.uint32)
        key = np.zeros(48, dtype=np.uint8)
        size = C.c_uint32(0)
        self._check(self._lib.pe_sync_committee_get(self._h, int(which), _ptr(idx, C.c_uint32), idx.size, C.addressof(size),
                                                    _ptr(key, C.c_uint8)))
        return (idx[:size.value], key.tobytes()) if size.value else None

    def sync_committee_rotate(self):
        """process_sync_committee_updates' move: current = next, no next (pe_sync_committee_rotate)."""
        self._check(self._lib.pe_sync_committee_rotate(self._h))

    def process_sync_aggregate(self, aggregates, total_active_balance: int, flags: int = SYNC_VERIFY | SYNC_APPLY,
                               base_reward_factor: int = 64) -> dict:
        """process_sync_aggregate for the blocks' aggregates in order, over the resident CURRENT committee
        (pe_process_sync_aggregate).  aggregates: a sequence of dicts / tuples (bits: 64 bytes, signature: 96 bytes,
        block_root, domain: 32 bytes each, proposer_index), or an array of _abi.pe_sync_aggregate.
        -> pe_sync_stats as a dict, with "verdict" int32[n] and "sig_status" int32[n] under SYNC_VERIFY."""
        if isinstance(aggregates, C.Array):
            rows = aggregates
        else:
            rows = (_abi.pe_sync_aggregate * max(len(aggregates), 1))()
            for r, a in zip(rows, aggregates):
                bits, sig, root, dom, prop = (a[k] for k in ("bits", "signature", "block_root", "domain", "proposer_index")) \
                    if isinstance(a, dict) else a
                for name, val, size in (("bits", bits, 64), ("signature", sig, 96), ("block_root", root, 32), ("domain", dom, 32)):
                    val = bytes(val)
                    assert len(val) == size, (name, len(val))
                    C.memmove(getattr(r, name), val, size)
                r.proposer_index = int(prop)
        n = len(aggregates)
        p = _abi.pe_sync_params()
        self._lib.pe_sync_params_default(C.byref(p))
        p.total_active_balance, p.base_reward_factor = int(total_active_balance), int(base_reward_factor)
        verdict = np.zeros(max(n, 1), dtype=np.int32)
        status = np.zeros(max(n, 1), dtype=np.int32)
        st = _abi.pe_sync_stats()
        self._check(self._lib.pe_process_sync_aggregate(self._h, C.addressof(rows), n, C.byref(p), int(flags),
                                                        _ptr(verdict, C.c_int32), _ptr(status, C.c_int32), C.byref(st)))
        res = {name: int(getattr(st, name)) for name, _ in _abi.pe_sync_stats._fields_}
        if flags & SYNC_VERIFY:
            res["verdict"], res["sig_status"] = verdict[:n], status[:n]
        return res

    def effective_balance_updates(self, balances, max_effective_balance: int = 32 * 10**9, hysteresis_quotient: int = 4,
                                  downward_multiplier: int = 1, upward_multiplier: int = 5, want_result: bool = True):
        """process_effective_balance_updates (pe:122-133) on the working-state view, in place.  balances: state.balances
        (one per validator), or BALANCES_RESIDENT: the vector on the device, read where it lies.
        -> (n_changed, new effective balances uint64[n] | None when not want_result)."""
        if balances is BALANCES_RESIDENT:
            bal, n = _BALANCES_RESIDENT_ARG, self.num_validators
        else:
            bal = np.ascontiguousarray(balances, dtype=np.uint64)
            n = bal.size
            if not n:
                bal = None
        out = np.empty(max(n, 1), dtype=np.uint64) if want_result else None
        n_changed = C.c_uint64(0)
        self._check(self._lib.pe_effective_balance_updates(self._h, n, _ptr(bal, C.c_uint64),
                                                           int(max_effective_balance), int(hysteresis_quotient),
                                                           int(downward_multiplier), int(upward_multiplier),
                                                           C.addressof(n_changed), _ptr(out, C.c_uint64)))
        return int(n_changed.value), (out[:n] if want_result else None)

    # -- rewards and penalties over resident balances ----------------------
    def state_set_balances(self, balances, inactivity_scores=None, withdrawable_epoch=None):
        """state.balances, state.inactivity_scores (None = zeros) and Validator.withdrawable_epoch (None =
        FAR_FUTURE_EPOCH everywhere) of the whole registry -> device memory (pe_state_set_balances).  (``set_balances``
        is pe_set_balances: the justified state's effective balances.)"""
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.uint64)
                for a in (balances, inactivity_scores, withdrawable_epoch)]
        n = arrs[0].size
        assert all(a is None or a.size == n for a in arrs), "one balance, score and withdrawable epoch per validator"
        self._check(self._lib.pe_state_set_balances(self._h, n, *(_ptr(a if n else None, C.c_uint64) for a in arrs)))

    def state_get_balances(self):
        """-> (balances, inactivity_scores, withdrawable_epoch: uint64[n] each, is_set); is_set False: the handle holds none."""
        n = self.num_validators
        bal, sc, wd = (np.zeros(max(n, 1), dtype=np.uint64) for _ in range(3))
        is_set = C.c_int(0)
        self._check(self._lib.pe_state_get_balances(self._h, n, _ptr(bal), _ptr(sc), _ptr(wd), C.addressof(is_set)))
        return bal[:n], sc[:n], wd[:n], bool(is_set.value)

    def rewards_params(self, **overrides):
        """pe_rewards_params_default with fields replaced by keyword (base_reward_factor, inactivity_score_bias,
        inactivity_score_recovery_rate, inactivity_penalty_quotient, min_epochs_to_inactivity_penalty)."""
        p = _abi.pe_rewards_params()
        self._lib.pe_rewards_params_default(C.byref(p))
        for k, v in overrides.items():
            assert hasattr(p, k), k
            setattr(p, k, int(v))
        return p

    def rewards_and_penalties(self, current_epoch: int, finalized_epoch: int, params=None,
                              which: int = REWARDS_INACTIVITY | REWARDS_DELTAS) -> dict:
        """process_inactivity_updates (REWARDS_INACTIVITY) and process_rewards_and_penalties (REWARDS_DELTAS) over the
        resident balances and scores, in place (pe_rewards_and_penalties).  params: ``rewards_params(...)``, a dict of its
        overrides, or None for the defaults.  -> pe_rewards_stats as a dict."""
        if params is None or isinstance(params, dict):
            params = self.rewards_params(**(params or {}))
        st = _abi.pe_rewards_stats()
        self._check(self._lib.pe_rewards_and_penalties(self._h, int(current_epoch), int(finalized_epoch), C.byref(params),
                                                       int(which), C.byref(st)))
        return {"total_active_balance": int(st.total_active_balance),
                "unslashed_balance": [int(x) for x in st.unslashed_balance], "n_eligible": int(st.n_eligible),
                "in_leak": int(st.in_leak), "rewards": int(st.rewards), "penalties": int(st.penalties),
                "n_saturated": int(st.n_saturated)}

    # -- registry updates and slashings over the resident registry ----------
    def registry_params(self, **overrides):
        """pe_registry_params_default with fields replaced by keyword (max_effective_balance, ejection_balance,
        max_seed_lookahead, min_validator_withdrawability_delay, min_per_epoch_churn_limit, churn_limit_quotient,
        max_per_epoch_activation_churn_limit)."""
        p = _abi.pe_registry_params()
        self._lib.pe_registry_params_default(C.byref(p))
        for k, v in overrides.items():
            assert hasattr(p, k), k
            setattr(p, k, int(v))
        return p

    def registry_updates(self, current_epoch: int, finalized_epoch: int, params=None) -> dict:
        """process_registry_updates over the resident epochs, in place (pe_registry_updates): eligibility marks, ejections
        through the exit queue, the head of the activation queue.  params: ``registry_params(...)``, a dict of its
        overrides, or None for the defaults.  -> pe_registry_stats as a dict.  The resident active list is dropped when an
        activation or exit epoch was written."""
        if params is None or isinstance(params, dict):
            params = self.registry_params(**(params or {}))
        st = _abi.pe_registry_stats()
        self._check(self._lib.pe_registry_updates(self._h, int(current_epoch), int(finalized_epoch), C.byref(params),
                                                  C.byref(st)))
        return {name: int(getattr(st, name)) for name, _ in _abi.pe_registry_stats._fields_}

    def process_slashings(self, current_epoch: int, sum_slashings: int, proportional_slashing_multiplier: int = 3,
                          epochs_per_slashings_vector: int = 8192) -> dict:
        """process_slashings over the resident balances, in place (pe_process_slashings).  sum_slashings =
        sum(state.slashings); the multiplier is PROPORTIONAL_SLASHING_MULTIPLIER of the fork in force (Bellatrix: 3).
        -> pe_slashings_stats as a dict."""
        st = _abi.pe_slashings_stats()
        self._check(self._lib.pe_process_slashings(self._h, int(current_epoch), int(sum_slashings),
                                                   int(proportional_slashing_multiplier), int(epochs_per_slashings_vector),
                                                   C.byref(st)))
        return {name: int(getattr(st, name)) for name, _ in _abi.pe_slashings_stats._fields_}

    # -- block operations over the resident registry: slashings and exits ----
    def block_ops_params(self, **overrides):
        """pe_block_ops_params_default with fields replaced by keyword (min_slashing_penalty_quotient,
        whistleblower_reward_quotient, epochs_per_slashings_vector, shard_committee_period,
        min_validator_withdrawability_delay, max_seed_lookahead, min_per_epoch_churn_limit, churn_limit_quotient)."""
        p = _abi.pe_block_ops_params()
        self._lib.pe_block_ops_params_default(C.byref(p))
        for k, v in overrides.items():
            assert hasattr(p, k), k
            setattr(p, k, int(v))
        return p

    def process_block_operations(self, current_epoch: int, proposer_index: int, ops, params=None):
        """process_proposer_slashing / process_attester_slashing / process_voluntary_exit over the resident registry, in
        array order, each on what the earlier ones left (pe_process_block_operations).  ops: ``attester_slashing_op``,
        ``proposer_slashing_op`` and ``voluntary_exit_op`` dicts.  params: ``block_ops_params(...)``, a dict of its
        overrides, or None for the defaults.  -> (status int32[n_ops], pe_block_ops_stats as a dict).  If any status is
        not 0 the block is invalid and NOTHING was changed (stats["n_invalid"] counts them); the caller adds
        stats["slashed_balance"] to state.slashings[current_epoch % EPOCHS_PER_SLASHINGS_VECTOR]."""
        if params is None or isinstance(params, dict):
            params = self.block_ops_params(**(params or {}))
        arr, flat = pack_block_ops(ops)
        status = np.zeros(max(len(ops), 1), dtype=np.int32)
        st = _abi.pe_block_ops_stats()
        self._check(self._lib.pe_process_block_operations(self._h, int(current_epoch), int(proposer_index), C.addressof(arr),
                                                          len(ops), _ptr(flat if flat.size else None, C.c_uint32), flat.size,
                                                          C.byref(params), _ptr(status), C.byref(st)))
        return status[:len(ops)], {name: int(getattr(st, name)) for name, _ in _abi.pe_block_ops_stats._fields_}

    # -- Capella: withdrawals and address changes over the resident registry ----
    def withdrawals_params(self, **overrides):
        """pe_withdrawals_params_default with fields replaced by keyword (max_effective_balance, max_withdrawals_per_payload,
        max_validators_per_sweep, eth1_prefix)."""
        p = _abi.pe_withdrawals_params()
        self._lib.pe_withdrawals_params_default(C.byref(p))
        for k, v in overrides.items():
            assert hasattr(p, k), k
            setattr(p, k, int(v))
        return p

    def process_withdrawals(self, current_epoch: int, next_withdrawal_index: int, next_withdrawal_validator_index: int,
                            payload=None, apply: bool = False, params=None):
        """get_expected_withdrawals / process_withdrawals over the resident registry (pe_process_withdrawals).  payload: the
        execution payload's withdrawals (``pack_withdrawals`` rows or (index, validator_index, address, amount) tuples; None =
        no payload: the call only computes); apply: debit the balances where the payload matches.  params:
        ``withdrawals_params(...)``, a dict of its overrides, or None for the defaults.  -> (the expected withdrawals as
        WITHDRAWAL_DTYPE rows, pe_withdrawals_result as a dict; "status" != 0: the block is invalid and NOTHING was changed)."""
        if params is None or isinstance(params, dict):
            params = self.withdrawals_params(**(params or {}))
        flags = (_abi.PE_WD_APPLY if apply else 0) | (0 if payload is None else _abi.PE_WD_PAYLOAD)
        rows = None if payload is None else pack_withdrawals(payload)
        out = np.zeros(64, dtype=WITHDRAWAL_DTYPE)
        res = _abi.pe_withdrawals_result()
        self._check(self._lib.pe_process_withdrawals(
            self._h, int(current_epoch), int(next_withdrawal_index), int(next_withdrawal_validator_index), C.byref(params),
            _ptr(rows if rows is not None and rows.size else None), 0 if rows is None else rows.size, flags, _ptr(out), C.byref(res)))
        d = {name: int(getattr(res, name)) for name, _ in _abi.pe_withdrawals_result._fields_ if name != "withdrawals_root"}
        d["withdrawals_root"] = bytes(res.withdrawals_root)
        return out[:res.n_withdrawals].copy(), d

    def process_bls_to_execution_changes(self, changes):
        """process_bls_to_execution_change over the resident withdrawal credentials, in array order, each on what the earlier
        ones left (pe_process_bls_to_execution_changes).  changes: ``pack_bls_changes`` rows or (validator_index,
        from_bls_pubkey, to_execution_address, signature_valid) tuples.  -> (status int32[n], pe_bls_changes_stats as a dict).
        If any status is not 0 the block is invalid and NOTHING was changed."""
        rows = pack_bls_changes(changes)
        status = np.zeros(max(rows.size, 1), dtype=np.int32)
        st = _abi.pe_bls_changes_stats()
        self._check(self._lib.pe_process_bls_to_execution_changes(self._h, _ptr(rows if rows.size else None), rows.size,
                                                                  _ptr(status), C.byref(st)))
        return status[:rows.size], {name: int(getattr(st, name)) for name, _ in _abi.pe_bls_changes_stats._fields_}

    def bls_change_signing_roots(self, changes, domain: bytes) -> np.ndarray:
        """compute_signing_root(BLSToExecutionChange, domain) of every change, hashed on the GPU
        (pe_bls_change_signing_roots): uint8[n, 32].  The caller hashes these to the curve and checks them against
        from_bls_pubkey: the verdicts are ``process_bls_to_execution_changes``' signature_valid."""
        rows = pack_bls_changes(changes)
        dom = np.frombuffer(bytes(domain), dtype=np.uint8).copy()
        assert dom.size == 32
        out = np.zeros((max(rows.size, 1), 32), dtype=np.uint8)
        self._check(self._lib.pe_bls_change_signing_roots(self._h, _ptr(rows if rows.size else None), rows.size, _ptr(dom), _ptr(out)))
        return out[:rows.size]

    # -- SSZ roots of the resident lists ------------------------------------
    def registry_set_static(self, pubkeys48, withdrawal_credentials, activation_eligibility_epoch):
        """Validator.pubkey (n x 48 B compressed), withdrawal_credentials (n x 32 B) and activation_eligibility_epoch of
        the whole registry -> device memory (pe_registry_set_static); the pubkeys are kept as their 32-byte leaves."""
        pk = np.ascontiguousarray(pubkeys48, dtype=np.uint8).reshape(-1, 48)
        wc = np.ascontiguousarray(withdrawal_credentials, dtype=np.uint8).reshape(-1, 32)
        el = np.ascontiguousarray(activation_eligibility_epoch, dtype=np.uint64)
        n = el.size
        assert pk.shape[0] == n and wc.shape[0] == n, "one pubkey, one credential and one epoch per validator"
        self._check(self._lib.pe_registry_set_static(self._h, n, _ptr(pk if n else None, C.c_uint8),
                                                     _ptr(wc if n else None, C.c_uint8), _ptr(el if n else None, C.c_uint64)))

    def registry_static(self):
        """-> (pubkey leaves uint8[n, 32], withdrawal_credentials uint8[n, 32], activation_eligibility_epoch uint64[n],
        is_set); is_set False: the handle holds none."""
        n = self.num_validators
        leaf, wc = np.zeros((max(n, 1), 32), dtype=np.uint8), np.zeros((max(n, 1), 32), dtype=np.uint8)
        el, is_set = np.zeros(max(n, 1), dtype=np.uint64), C.c_int(0)
        self._check(self._lib.pe_registry_get_static(self._h, n, _ptr(leaf), _ptr(wc), _ptr(el), C.addressof(is_set)))
        return leaf[:n], wc[:n], el[:n], bool(is_set.value)

    def state_roots(self, which: int = ROOT_ALL, limit_log2: int = 40, want_leaves: bool = False) -> dict:
        """hash_tree_root of the BeaconState fields named by ``which`` (ROOT_* bits) from the resident arrays
        (pe_state_roots).  -> {field name: 32 bytes} for the fields asked for; with want_leaves and ROOT_VALIDATORS also
        "validator_leaves": uint8[n, 32], hash_tree_root(Validator) of every validator."""
        out = _abi.pe_state_root_set()
        leaves = None
        if want_leaves and (which & ROOT_VALIDATORS):
            leaves = np.zeros((max(self.num_validators, 1), 32), dtype=np.uint8)
        self._check(self._lib.pe_state_roots(self._h, int(which), int(limit_log2), C.byref(out), _ptr(leaves, C.c_uint8)))
        res = {name: bytes(getattr(out, name)) for bit, name in _ROOT_FIELDS if which & bit}
        if leaves is not None:
            res["validator_leaves"] = leaves[:self.num_validators]
        return res

    def ssz_merkleize(self, chunks, depth: int, mix_length: Optional[int] = None) -> bytes:
        """merkleize(chunks, depth) of 32-byte chunks in host memory (bytes, or a uint8 array of n x 32) on the GPU;
        mix_length: mix_in_length with it (None = no mix-in).  -> the 32-byte root."""
        if isinstance(chunks, (bytes, bytearray, memoryview)):
            ch = np.frombuffer(bytes(chunks), dtype=np.uint8)
        else:
            ch = np.ascontiguousarray(chunks, dtype=np.uint8).reshape(-1)
        assert ch.size % 32 == 0, "chunks are 32 bytes each"
        out = np.zeros(32, dtype=np.uint8)
        self._check(self._lib.pe_ssz_merkleize(self._h, _ptr(ch if ch.size else None, C.c_uint8), ch.size // 32, int(depth),
                                               -1 if mix_length is None else int(mix_length), _ptr(out, C.c_uint8)))
        return out.tobytes()

    # -- deposits -----------------------------------------------------------
    @staticmethod
    def _deposit_rows(deposits) -> np.ndarray:
        """DEPOSIT_DTYPE rows, or an iterable of (pubkey48, withdrawal_credentials32, amount, signature96)."""
        if isinstance(deposits, np.ndarray) and deposits.dtype == DEPOSIT_DTYPE:
            return np.ascontiguousarray(deposits)
        items = list(deposits)
        rows = np.zeros(len(items), dtype=DEPOSIT_DTYPE)
        for i, (pk, wc, amount, sig) in enumerate(items):
            rows[i] = (np.frombuffer(bytes(pk), dtype=np.uint8), np.frombuffer(bytes(wc), dtype=np.uint8), int(amount),
                       np.frombuffer(bytes(sig), dtype=np.uint8))
        return rows

    def deposit_params(self, **overrides):
        """pe_deposit_params with the mainnet defaults, fields replaced by keyword."""
        p = _abi.pe_deposit_params()
        self._lib.pe_deposit_params_default(C.byref(p))
        for k, v in overrides.items():
            assert hasattr(p, k), k
            setattr(p, k, int(v))
        return p

    def deposit_signing_roots(self, deposits, domain: bytes) -> np.ndarray:
        """compute_signing_root(DepositMessage, domain) of every deposit, hashed on the GPU (pe_deposit_signing_roots):
        uint8[n, 32].  The caller hashes these to the curve: the results are ``process_deposits``' message points."""
        rows = self._deposit_rows(deposits)
        dom = np.frombuffer(bytes(domain), dtype=np.uint8).copy()
        assert dom.size == 32
        out = np.zeros((max(rows.size, 1), 32), dtype=np.uint8)
        self._check(self._lib.pe_deposit_signing_roots(self._h, _ptr(rows if rows.size else None), rows.size, _ptr(dom), _ptr(out)))
        return out[:rows.size]

    def process_deposits(self, deposits, message_points192=None, proofs=None, eth1_deposit_index: int = 0,
                         deposit_root: Optional[bytes] = None, params=None) -> dict:
        """process_deposit for a batch, sequential semantics, over the resident registry (pe_process_deposits).
        proofs: uint8[n, 33, 32] or None (not checked: genesis); message_points192: uint8[n, 192], H(signing_root_i), needed
        where a deposit's pubkey is new.  params: ``deposit_params(...)``, a dict of its overrides, or None.
        -> {"status": int32[n] (DEP_*), "index": uint32[n] (validator credited, 0xFFFFFFFF = none), and pe_deposit_stats}."""
        rows = self._deposit_rows(deposits)
        n = rows.size
        if params is None or isinstance(params, dict):
            params = self.deposit_params(**(params or {}))
        pr = None if proofs is None else np.ascontiguousarray(proofs, dtype=np.uint8).reshape(-1)
        assert pr is None or pr.size == n * 33 * 32, "a proof is 33 nodes of 32 bytes"
        mp = None if message_points192 is None else np.ascontiguousarray(message_points192, dtype=np.uint8).reshape(-1)
        assert mp is None or mp.size == n * 192, "one 192-byte message point per deposit"
        root = None if deposit_root is None else np.frombuffer(bytes(deposit_root), dtype=np.uint8).copy()
        assert root is None or root.size == 32
        status = np.zeros(max(n, 1), dtype=np.int32)
        index = np.full(max(n, 1), 0xFFFFFFFF, dtype=np.uint32)
        st = _abi.pe_deposit_stats()
        self._check(self._lib.pe_process_deposits(self._h, _ptr(rows if n else None), n, _ptr(pr if n else None),
                                                  int(eth1_deposit_index), _ptr(root), _ptr(mp if n else None),
                                                  C.byref(params), _ptr(status), _ptr(index), C.byref(st)))
        res = {name: int(getattr(st, name)) for name, _ in _abi.pe_deposit_stats._fields_}
        res["status"], res["index"] = status[:n], index[:n]
        return res

    def deposit_index_info(self) -> dict:
        """The pubkey index ``process_deposits`` keeps (pe_profile_deposit_index): slots (0 = none), keys, build_ms."""
        slots, keys, ms = C.c_uint32(0), C.c_uint64(0), C.c_float(0)
        self._check(self._lib.pe_profile_deposit_index(self._h, C.addressof(slots), C.addressof(keys), C.addressof(ms)))
        return {"slots": int(slots.value), "keys": int(keys.value), "build_ms": float(ms.value)}

    def g1_sum(self, offsets, index=None, points96=None) -> np.ndarray:
        off = np.ascontiguousarray(offsets, dtype=np.uint32)
        idx = None if index is None else np.ascontiguousarray(index, dtype=np.uint32)
        pts = None if points96 is None else np.ascontiguousarray(points96, dtype=np.uint8)
        n_points = 0 if pts is None else pts.size // 96
        n_groups = off.size - 1
        out = np.zeros((max(n_groups, 1), 96), dtype=np.uint8)
        self._check(self._lib.pe_g1_sum(self._h, _ptr(pts, C.c_uint8), n_points, _ptr(idx, C.c_uint32),
                                        _ptr(off, C.c_uint32), n_groups, _ptr(out, C.c_uint8)))
        return out[:n_groups]

    def g1_key_validate(self, points96=None) -> np.ndarray:
        """KeyValidate (A.7): status per key -- 0 valid, 3 not in the prime-order subgroup, 4 identity.  points96 None =
        the registry's pubkeys as loaded."""
        if points96 is None:
            n, p = self.num_validators, None
        else:
            p = np.ascontiguousarray(points96, dtype=np.uint8).reshape(-1, 96)
            n = p.shape[0]
        status = np.empty(max(n, 1), dtype=np.int32)
        self._check(self._lib.pe_g1_key_validate(self._h, _ptr(p, C.c_uint8), n, _ptr(status, C.c_int32)))
        return status[:n]

    def g1_decompress(self, keys48):
        """48-byte compressed BLSPubkeys (pe:37) -> (96-byte uncompressed (n, 96), status int32[n])."""
        k = np.ascontiguousarray(keys48, dtype=np.uint8).reshape(-1, 48)
        n = k.shape[0]
        out = np.empty((max(n, 1), 96), dtype=np.uint8)
        status = np.empty(max(n, 1), dtype=np.int32)
        self._check(self._lib.pe_g1_decompress(self._h, _ptr(k, C.c_uint8), n, _ptr(out, C.c_uint8), _ptr(status, C.c_int32)))
        return out[:n], status[:n]

    def set_pubkeys_compressed(self, keys48):
        """Load the registry's pubkeys from their 48-byte wire form; raises if any key does not decode."""
        k = np.ascontiguousarray(keys48, dtype=np.uint8).reshape(-1, 48)
        status = np.empty(max(k.shape[0], 1), dtype=np.int32)
        self._check(self._lib.pe_set_pubkeys_compressed(self._h, k.shape[0], _ptr(k, C.c_uint8), _ptr(status, C.c_int32)))

    def g1_compress(self, points96) -> np.ndarray:
        p = np.ascontiguousarray(points96, dtype=np.uint8).reshape(-1, 96)
        out = np.empty((max(p.shape[0], 1), 48), dtype=np.uint8)
        self._check(self._lib.pe_g1_compress(_ptr(p, C.c_uint8), p.shape[0], _ptr(out, C.c_uint8)))
        return out[:p.shape[0]]

    def g2_decompress(self, sigs96):
        """96-byte compressed BLSSignatures (pe:37) -> (192-byte uncompressed (n, 192), status int32[n])."""
        k = np.ascontiguousarray(sigs96, dtype=np.uint8).reshape(-1, 96)
        n = k.shape[0]
        out = np.empty((max(n, 1), 192), dtype=np.uint8)
        status = np.empty(max(n, 1), dtype=np.int32)
        self._check(self._lib.pe_g2_decompress(self._h, _ptr(k, C.c_uint8), n, _ptr(out, C.c_uint8), _ptr(status, C.c_int32)))
        return out[:n], status[:n]

    def g2_compress(self, points192) -> np.ndarray:
        p = np.ascontiguousarray(points192, dtype=np.uint8).reshape(-1, 192)
        out = np.empty((max(p.shape[0], 1), 96), dtype=np.uint8)
        self._check(self._lib.pe_g2_compress(_ptr(p, C.c_uint8), p.shape[0], _ptr(out, C.c_uint8)))
        return out[:p.shape[0]]

    def g2_sum(self, points192, offsets, index=None) -> np.ndarray:
        """bls.Aggregate over G2 signature points (pe:659, pe:1536): 192-byte uncompressed in, 192-byte affine out."""
        off = np.ascontiguousarray(offsets, dtype=np.uint32)
        idx = None if index is None else np.ascontiguousarray(index, dtype=np.uint32)
        pts = np.ascontiguousarray(points192, dtype=np.uint8)
        n_groups = off.size - 1
        out = np.empty((max(n_groups, 1), 192), dtype=np.uint8)
        self._check(self._lib.pe_g2_sum(self._h, _ptr(pts, C.c_uint8), pts.size // 192, _ptr(idx, C.c_uint32),
                                        _ptr(off, C.c_uint32), n_groups, _ptr(out, C.c_uint8)))
        return out[:n_groups]

    def aggregate_signatures(self, signatures, offsets, index=None, check_subgroup: bool = False):
        """pe_aggregate_signatures: bls.Aggregate per committee over an epoch's unaggregated compressed signatures
        (pe:717, pe:659, pe:1536).  signatures: (n, 96) uint8 array or a DeviceArena of n * 96 bytes; index: uint32 array
        or a DeviceArena of 4-byte entries (None = contiguous groups).
        -> (aggregates (n_groups, 96) uint8, per-signature status int32 (n,), undecodable members per group uint32)."""
        off = np.ascontiguousarray(offsets, dtype=np.uint32)
        n_groups = off.size - 1
        if isinstance(signatures, DeviceArena):
            sig_ptr, n = signatures.ptr, signatures.size // 96
        else:
            sig = np.ascontiguousarray(signatures, dtype=np.uint8)
            sig_ptr, n = sig.ctypes.data, sig.size // 96
        if index is None:
            idx_ptr = None
        elif isinstance(index, DeviceArena):
            idx_ptr = index.ptr
        else:
            idx = np.ascontiguousarray(index, dtype=np.uint32)
            idx_ptr = idx.ctypes.data
        out = np.empty((max(n_groups, 1), 96), dtype=np.uint8)
        status = np.zeros(max(n, 1), dtype=np.int32)
        bad = np.zeros(max(n_groups, 1), dtype=np.uint32)
        flags = _abi.PE_SIG_CHECK_SUBGROUP if check_subgroup else 0
        self._check(self._lib.pe_aggregate_signatures(self._h, C.c_void_p(sig_ptr), n, C.c_void_p(idx_ptr) if idx_ptr else None,
                                                      _ptr(off, C.c_uint32), n_groups, flags, _ptr(out, C.c_uint8),
                                                      _ptr(status, C.c_int32), _ptr(bad, C.c_uint32)))
        return out[:n_groups], status[:n], bad[:n_groups]

    # -- multi-GPU exchange inside the C ABI (RCCL owned by the engine) -------
    def dist_unique_id(self) -> bytes:
        """rank 0: the PE_DIST_ID_BYTES (two RCCL unique ids) to ship to the other ranks (pe_dist_unique_id)."""
        out = (C.c_uint8 * _abi.PE_DIST_ID_BYTES)()
        rc = self._lib.pe_dist_unique_id(out)
        if rc != _abi.PE_OK:
            raise EngineError(rc, "pe_dist_unique_id: librccl not available")
        return bytes(out)

    def dist_init(self, unique_id: bytes, rank: int, world: int):
        assert len(unique_id) == _abi.PE_DIST_ID_BYTES
        buf = (C.c_uint8 * _abi.PE_DIST_ID_BYTES).from_buffer_copy(unique_id)
        self._check(self._lib.pe_dist_init(self._h, buf, rank, world))

    def dist_init_ex(self, unique_id: bytes, rank: int, world: int, single_comm: bool = False):
        assert len(unique_id) == _abi.PE_DIST_ID_BYTES
        buf = (C.c_uint8 * _abi.PE_DIST_ID_BYTES).from_buffer_copy(unique_id)
        self._check(self._lib.pe_dist_init_ex(self._h, buf, rank, world, _abi.PE_DIST_SINGLE_COMM if single_comm else 0))

    def dist_init_custom(self, rank: int, world: int, all_reduce_u64, all_gather):
        """pe_dist_init_custom: the two exchange steps through Python callables
        ``all_reduce_u64(dev_ptr, count, hip_stream) -> int`` (in-place sum over ranks) and
        ``all_gather(dev_send, dev_recv, bytes_per_rank, hip_stream) -> int``, both on device memory, ordered on the stream
        (pos_evolution_amd.sharded.HostStagedCollectives is one such pair over any torch.distributed backend)."""
        def _ar(_user, buf, count, stream):
            try:
                return int(all_reduce_u64(buf or 0, int(count), stream or 0) or 0)
            except Exception as err:  # never unwind through the C frames
                print(f"[posevo] all_reduce_u64 callback failed: {err!r}", file=sys.stderr)
                return 1

        def _ag(_user, send, recv, nbytes, stream):
            try:
                return int(all_gather(send or 0, recv or 0, int(nbytes), stream or 0) or 0)
            except Exception as err:
                print(f"[posevo] all_gather callback failed: {err!r}", file=sys.stderr)
                return 1

        fn = _abi.pe_collectives(None, _abi.ALL_REDUCE_FN(_ar), _abi.ALL_GATHER_FN(_ag))
        self._coll_keep = fn  # the engine calls through these pointers until dist_destroy
        self._check(self._lib.pe_dist_init_custom(self._h, rank, world, C.addressof(fn)))

    def dist_set_timeout_ms(self, ms: int):
        self._check(self._lib.pe_dist_set_timeout_ms(self._h, int(ms)))

    def dist_set_max_groups(self, n: int):
        self._check(self._lib.pe_dist_set_max_groups(self._h, int(n)))

    def aggregate_exchange(self, cap_groups: int, max_bits: int = 2048):
        """pe_aggregate_exchange (committee-sharded steps): the aggregates of the last aggregate() over DeviceRows are
        all-gathered and become the resident aggregate for the handlers.  -> the gathered aggregates (atts, out_arena,
        count; fields valid when the call's outputs are complete).  cap_groups >= world x the local bound."""
        m = max(int(cap_groups), 1)
        (out_atts, out_arena, count, ng), (p_atts, p_arena, p_count, p_ng) = self._outs(
            "xagg", ((m, _ATT_DTYPE), (m * ((max_bits + 31) // 32) * 4, _U8), (m, _U32), (1, _U32)))
        ng[0] = 0
        if self._pipe_keep is not None:
            self._pipe_keep.append((out_atts, out_arena, count, ng))
        rc = self._lib.pe_aggregate_exchange(self._h, p_atts, p_ng, p_arena, out_arena.size, p_count, m)
        if rc:
            self._check(rc)
        return ResidentAggregateResult(_raw=dict(n_groups=ng, atts=out_atts, group_of=None, out_arena=out_arena, aggpk96=None,
                                                 count=count), sig96=None, sig192=None)

    def dist_destroy(self):
        self._check(self._lib.pe_dist_destroy(self._h))
        self._coll_keep = None

    def get_head_sharded(self) -> bytes:
        """get_head over all shards through the engine's own RCCL communicator (one all-reduce on its stream)."""
        out = (C.c_uint8 * 32)()
        self._check(self._lib.pe_get_head_sharded(self._h, out))
        return bytes(out)

    def get_head_sharded_async(self) -> np.ndarray:
        """pe_get_head_sharded_async: -> a 32-byte array that holds the root once the pipeline's outputs are complete."""
        (out,), (p_out,) = self._outs("headsh", ((32, _U8),))
        if self._pipe_keep is not None:
            self._pipe_keep.append(out)
        rc = self._lib.pe_get_head_sharded_async(self._h, p_out)
        if rc:
            self._check(rc)
        return out

    def aggregate_sharded(self, rows=None, packed=None):
        """pe_aggregate over all shards (one all-gather of the XYZZ partials inside): rank-local unions, global
        aggregate pubkeys.  Inside a pipeline() block nothing waits; the unions can be handed on as RESIDENT."""
        arr, arena = packed if packed is not None else pack_attestations(rows)
        n = len(rows) if rows is not None else len(arr)
        m = max(n, 1)
        if arr.__class__ is DeviceRows:  # rows in device memory: grouped / resolved there; the handlers take ROWS_RESIDENT
            (out_atts, group_of, out_arena, out_pk, count, ng), (p_atts, p_gof, p_arena, p_pk, p_count, p_ng) = self._outs(
                "raggsh", ((m, _ATT_DTYPE), (m, _U32), (max(arena.size, 1), _U8), ((m, 96), _U8), (m, _U32), (1, _U32)))
            ng[0] = 0
            if self._pipe_keep is not None:
                self._pipe_keep.append((arr, arena, out_atts, group_of, out_arena, out_pk, count, ng))
            rc = self._lib.pe_aggregate_sharded(self._h, arr.ptr, n, _ptr(arena, C.c_uint8), arena.size, p_atts, p_ng,
                                                p_gof, p_arena, out_arena.size, p_pk, p_count)
            if rc:
                self._check(rc)
            return ResidentAggregateResult(_raw=dict(n_groups=ng, atts=out_atts, group_of=group_of, out_arena=out_arena,
                                                     aggpk96=out_pk, count=count), sig96=None, sig192=None)
        (out_atts, group_of, out_arena, out_pk, count), (p_atts, p_gof, p_arena, p_pk, p_count) = self._outs(
            "aggsh", ((m, _ATT_DTYPE), (m, _U32), (max(arena.size, 1), _U8), ((m, 96), _U8), (m, _U32)))
        n_groups = C.c_uint32(0)
        if self._pipe_keep is not None:
            self._pipe_keep.append((arr, arena, out_atts, group_of, out_arena, out_pk, count))
        rc = self._lib.pe_aggregate_sharded(self._h, _att_ptr(arr), n, _ptr(arena, C.c_uint8), arena.size, p_atts,
                                            C.byref(n_groups), p_gof, p_arena, out_arena.size, p_pk, p_count)
        if rc:
            self._check(rc)
        g = n_groups.value
        if g:
            tail = out_atts.view(np.uint32).reshape(-1, 36)[g - 1]   # u32 words 32 / 33 of a row: bits_offset, n_bits
            out_arena = out_arena[: int(tail[32]) + (int(tail[33]) + 7) // 8]
        return AggregateResult(n_groups=g, atts=out_atts[:g], group_of=group_of[:n], out_arena=out_arena, sig96=None,
                               sig192=None, aggpk96=out_pk[:g], count=count[:g])

    # -- multi-GPU exchange -------------------------------------------------
    def votes_partial(self, dev_ptr: int):
        """dev_ptr: device buffer of num_blocks + PE_EXCHANGE_EXTRA u64 (weights | per-workgroup active totals)."""
        self._check(self._lib.pe_votes_partial(self._h, C.c_void_p(dev_ptr), self.num_blocks))

    def head_from_weights(self, dev_ptr: int) -> bytes:
        out = (C.c_uint8 * 32)()
        self._check(self._lib.pe_head_from_weights(self._h, C.c_void_p(dev_ptr), self.num_blocks, out))
        return bytes(out)

    def aggregate_partial(self, dev_ptr: int, rows=None, packed=None, capacity_groups: int = 0):
        """pe_aggregate with the aggregate pubkeys left as this shard's XYZZ partials (192 B each) at dev_ptr, a device
        buffer of capacity_groups partials (a batch forming more groups fails with PE_ERR_CAPACITY, nothing written)."""
        arr, arena = packed if packed is not None else pack_attestations(rows)
        n = len(rows) if rows is not None else len(arr)
        out_atts = np.empty(max(n, 1), dtype=_ATT_DTYPE)
        n_groups = C.c_uint32(0)
        group_of = np.empty(max(n, 1), dtype=np.uint32)
        out_arena = np.empty(max(arena.size, 1), dtype=np.uint8)
        count = np.empty(max(n, 1), dtype=np.uint32)
        self._check(self._lib.pe_aggregate_partial(self._h, _att_ptr(arr), n, _ptr(arena, C.c_uint8), arena.size,
                                                   _att_ptr(out_atts), C.byref(n_groups), _ptr(group_of, C.c_uint32),
                                                   _ptr(out_arena, C.c_uint8), out_arena.size,
                                                   _ptr(count, C.c_uint32), C.c_void_p(dev_ptr), capacity_groups))
        g = n_groups.value
        if g:
            last = out_atts[g - 1]
            out_arena = out_arena[: int(last["bits_offset"]) + (int(last["n_bits"]) + 7) // 8]
        return dict(n_groups=g, atts=out_atts[:g], group_of=group_of[:n], out_arena=out_arena, count=count[:g])

    def g1_partial(self, offsets, index, dev_ptr: int, capacity_groups: int):
        off = np.ascontiguousarray(offsets, dtype=np.uint32)
        idx = None if index is None else np.ascontiguousarray(index, dtype=np.uint32)
        self._check(self._lib.pe_g1_partial(self._h, _ptr(idx, C.c_uint32), _ptr(off, C.c_uint32), off.size - 1,
                                            C.c_void_p(dev_ptr), capacity_groups))

    def g1_finish(self, dev_ptr: int, n_ranks: int, n_groups: int) -> np.ndarray:
        out = np.zeros((max(n_groups, 1), 96), dtype=np.uint8)
        self._check(self._lib.pe_g1_finish(self._h, C.c_void_p(dev_ptr), n_ranks, n_groups, _ptr(out, C.c_uint8)))
        return out[:n_groups]

    # -- inspection -------------------------------------------------------
    @property
    def num_blocks(self) -> int:
        return int(self._lib.pe_num_blocks(self._h))

    @property
    def num_validators(self) -> int:
        return int(self._lib.pe_num_validators(self._h))

    def block_root_at(self, i: int) -> bytes:
        out = (C.c_uint8 * 32)()
        self._check(self._lib.pe_block_root_at(self._h, i, out))
        return bytes(out)

    def block_index_of(self, root: bytes) -> int:
        out = C.c_uint32(0)
        self._check(self._lib.pe_block_index_of(self._h, _root(root), C.byref(out)))
        return out.value

    def latest_messages(self):
        """-> (epoch uint64[V], block_index uint32[V]); block_index 0xFFFFFFFF = no message (epoch 0), PE_VOTE_PRUNED
        (0xFFFFFFFE) = a message whose block ``prune`` removed: it keeps its epoch, so a later vote of an equal or lower
        epoch is still refused, and weighs on nothing."""
        n = self.num_validators
        ep = np.zeros(max(n, 1), dtype=np.uint64)
        bi = np.zeros(max(n, 1), dtype=np.uint32)
        self._check(self._lib.pe_get_latest_messages(self._h, _ptr(ep, C.c_uint64), _ptr(bi, C.c_uint32), n))
        return ep[:n], bi[:n]

    # -- checkpoint / resume ------------------------------------------------
    def state_validators(self):
        """-> (effective_balance u64[n], flags u8[n], is_set): the working-state view process_attestation and the FFG
        sums read (pe_state_set_validators); is_set False while it still mirrors the registry."""
        n = self.num_validators
        bal, flags, is_set = np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint8), C.c_int(0)
        self._check(self._lib.pe_state_get_validators(self._h, n, _ptr(bal), _ptr(flags), C.byref(is_set)))
        return bal[:n], flags[:n], bool(is_set.value)

    def committee_epochs(self):
        n = C.c_uint32(0)
        self._check(self._lib.pe_get_committee_epochs(self._h, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=np.uint64)
        self._check(self._lib.pe_get_committee_epochs(self._h, _ptr(out), n.value, C.byref(n)))
        return [int(x) for x in out[: n.value]]

    def committees(self, epoch: int):
        """-> (offsets u32[C + 1], members u32[total]) of the table held for `epoch` (set or computed on the GPU)."""
        nc = C.c_uint32(0)
        self._check(self._lib.pe_get_committees(self._h, epoch, C.byref(nc), None, 0, None, 0))
        offsets = np.zeros(nc.value + 1, dtype=np.uint32)
        self._check(self._lib.pe_get_committees(self._h, epoch, C.byref(nc), _ptr(offsets), offsets.size, None, 0))
        members = np.zeros(max(int(offsets[-1]), 1), dtype=np.uint32)
        self._check(self._lib.pe_get_committees(self._h, epoch, C.byref(nc), None, 0, _ptr(members), int(offsets[-1])))
        return offsets, members[: int(offsets[-1])]

    def export_state(self) -> dict:
        """The store's dynamic state as flat arrays (SURVEY.md 5 "checkpoint / resume"): scalars, the block table in
        insertion order, validator flags (incl. the equivocating bit), latest messages, participation flags, the
        committee tables and the working-state view.  The registry itself (balances, pubkeys) is the caller's input and
        is passed again to import_state."""
        nb, nv = self.num_blocks, self.num_validators
        roots = np.zeros((nb, 32), dtype=np.uint8)
        parent = np.zeros(nb, dtype=np.uint32)
        slot = np.zeros(nb, dtype=np.uint64)
        pj_e, pf_e = np.zeros(nb, dtype=np.uint64), np.zeros(nb, dtype=np.uint64)
        pj_r, pf_r = np.zeros((nb, 32), dtype=np.uint8), np.zeros((nb, 32), dtype=np.uint8)
        r, jr, fr = ((C.c_uint8 * 32)() for _ in range(3))
        pi, sl, je, fe = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        for i in range(nb):
            self._check(self._lib.pe_get_block(self._h, i, r, C.byref(pi), C.byref(sl), C.byref(je), jr, C.byref(fe), fr))
            roots[i], parent[i], slot[i] = np.frombuffer(r, dtype=np.uint8), pi.value, sl.value
            pj_e[i], pf_e[i] = je.value, fe.value
            pj_r[i], pf_r[i] = np.frombuffer(jr, dtype=np.uint8), np.frombuffer(fr, dtype=np.uint8)
        flags = np.zeros(max(nv, 1), dtype=np.uint8)
        lm_slot = np.zeros(max(nv, 1), dtype=np.uint32)
        if nv:
            self._check(self._lib.pe_get_validator_flags(self._h, _ptr(flags), nv))
            self._check(self._lib.pe_get_latest_message_slots(self._h, _ptr(lm_slot), nv))
        ep, bi = self.latest_messages()
        sbal, sflags, s_set = self.state_validators()
        return dict(committees={e: self.committees(e) for e in self.committee_epochs()},
                    state_view=(sbal.copy(), sflags.copy()) if s_set else None,
                    scalars=self.store_scalars(), roots=roots, parent=parent, slot=slot, post_justified_epoch=pj_e,
                    post_justified_root=pj_r, post_finalized_epoch=pf_e, post_finalized_root=pf_r, flags=flags[:nv],
                    lm_epoch=ep.copy(), lm_block=bi.copy(), lm_slot=lm_slot[:nv],
                    participation=(self.participation_get(0), self.participation_get(1)))

    def import_state(self, st: dict, effective_balance, pubkeys96=None):
        """Rebuild the store exported by export_state on this (fresh) handle."""
        sc = st["scalars"]
        roots = st["roots"]
        self.store_init(sc["genesis_time"], int(st["slot"][0]), roots[0].tobytes())
        # block 0 of a pruned store is an ordinary block: its own post-state checkpoints, not the anchor's
        self._check(self._lib.pe_set_block_checkpoints(
            self._h, 0, int(st["post_justified_epoch"][0]), _root(st["post_justified_root"][0].tobytes()),
            int(st["post_finalized_epoch"][0]), _root(st["post_finalized_root"][0].tobytes())))
        for i in range(1, roots.shape[0]):
            self.add_block(roots[i].tobytes(), roots[int(st["parent"][i])].tobytes(), int(st["slot"][i]),
                           (int(st["post_justified_epoch"][i]), st["post_justified_root"][i].tobytes()),
                           (int(st["post_finalized_epoch"][i]), st["post_finalized_root"][i].tobytes()))
        flags = np.ascontiguousarray(st["flags"], dtype=np.uint8)
        self.set_validators(effective_balance, flags & np.uint8(0xFF ^ _abi.PE_VAL_EQUIVOCATING), pubkeys96)
        equiv = np.nonzero(flags & _abi.PE_VAL_EQUIVOCATING)[0]
        if equiv.size:
            self.mark_equivocating(equiv)
        ep = np.ascontiguousarray(st["lm_epoch"], dtype=np.uint64)
        bi = np.ascontiguousarray(st["lm_block"], dtype=np.uint32)
        sl = np.ascontiguousarray(st["lm_slot"], dtype=np.uint32)
        self._check(self._lib.pe_set_latest_messages(self._h, ep.size, _ptr(ep), _ptr(bi), _ptr(sl)))
        self.on_tick(sc["time"])
        self.set_checkpoints(sc["justified"], sc["finalized"])
        self._check(self._lib.pe_set_best_justified(self._h, sc["best_justified"][0], _root(sc["best_justified"][1])))
        self.set_proposer_boost(sc["proposer_boost_root"])
        self.participation_set(0, st["participation"][0])
        self.participation_set(1, st["participation"][1])
        for epoch, (offsets, members) in sorted(st.get("committees", {}).items()):
            self.set_committees(epoch, offsets, members)
        if st.get("state_view") is not None:
            self.state_set_validators(*st["state_view"])

    def store_scalars(self) -> dict:
        t, g, je, fe, be = (C.c_uint64(0) for _ in range(5))
        jr, fr, br, boost = ((C.c_uint8 * 32)() for _ in range(4))
        self._check(self._lib.pe_get_store_scalars(self._h, C.byref(t), C.byref(g), C.byref(je), jr, C.byref(fe), fr,
                                                   C.byref(be), br, boost))
        return dict(time=t.value, genesis_time=g.value, justified=(je.value, bytes(jr)),
                    finalized=(fe.value, bytes(fr)), best_justified=(be.value, bytes(br)),
                    proposer_boost_root=bytes(boost))

    # -- profiling --------------------------------------------------------
    def profile_enable(self, on=True):
        """0 / False off, 1 / True per-kernel totals, 3 totals of the accumulation only, 2 totals + the timeline of
        profile_timeline()."""
        self._check(self._lib.pe_profile_enable(self._h, int(on)))

    def profile_timeline(self):
        """-> list of (kernel name, start_ms, duration_ms) of the launches bracketed since profile_reset(), by start time
        (pe_profile_timeline; profile_enable(2))."""
        n = C.c_uint32(0)
        self._check(self._lib.pe_profile_timeline(self._h, None, None, None, 0, C.byref(n)))
        k = np.zeros(max(n.value, 1), dtype=np.int32)
        t0 = np.zeros(max(n.value, 1), dtype=np.float64)
        dt = np.zeros(max(n.value, 1), dtype=np.float64)
        self._check(self._lib.pe_profile_timeline(self._h, _ptr(k, C.c_int32), _ptr(t0, C.c_double), _ptr(dt, C.c_double),
                                                  n.value, C.byref(n)))
        rows = [(_abi.KERNEL_NAMES[int(k[i])], float(t0[i]), float(dt[i])) for i in range(min(n.value, k.size))]
        return sorted(rows, key=lambda r: r[1])

    def profile_queue_classes(self):
        """pe_profile_queue_classes: for the engine / accumulation / tree / finish streams, the lowest of them that shares
        its hardware queue -- [0, 1, 2, 3] when each has a queue of its own."""
        out = np.zeros(4, dtype=np.int32)
        self._check(self._lib.pe_profile_queue_classes(self._h, _ptr(out, C.c_int32)))
        return [int(x) for x in out]

    def profile_arena_growths(self) -> int:
        """pe_profile_arena_growths: (re)allocations of arena buffers since the handle was created."""
        n = C.c_uint64(0)
        self._check(self._lib.pe_profile_arena_growths(self._h, C.byref(n)))
        return int(n.value)

    def profile_committee_sums(self):
        """pe_profile_committee_sums: (committee tables that hold valid pubkey sums, groups of the last completed aggregate
        over device rows that were summed by complement)."""
        a, b = C.c_uint32(0), C.c_uint32(0)
        self._check(self._lib.pe_profile_committee_sums(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def profile_accumulate_mhz(self):
        """pe_profile_accumulate_mhz: the shader clock (MHz) of each k_g1_accumulate launch since profile_reset(), in launch
        order (launches made while profiling was on; the last 4096)."""
        out = np.zeros(4096, dtype=np.float64)
        n = C.c_uint32(0)
        self._check(self._lib.pe_profile_accumulate_mhz(self._h, out.ctypes.data_as(C.c_void_p), 4096, C.byref(n)))
        return out[:min(int(n.value), 4096)].copy()

    def profile_reset(self):
        self._check(self._lib.pe_profile_reset(self._h))

    def profile(self) -> dict:
        out = {}
        for k, name in enumerate(_abi.KERNEL_NAMES):
            n, ms = C.c_uint64(0), C.c_double(0)
            self._check(self._lib.pe_profile_get(self._h, k, C.byref(n), C.byref(ms)))
            out[name] = dict(launches=n.value, total_ms=ms.value)
        return out
