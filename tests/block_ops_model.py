"""An own-words model of the block operations the engine applies to its resident registry (pe_process_block_operations):
process_proposer_slashing, process_attester_slashing and process_voluntary_exit with slash_validator and
initiate_validator_exit under them.  The reference holds the Validator fields (pe:36-45), `slashings` (pe:359/397) and
is_slashable_attestation_data (pe:1134-1143, executed here from the reference's own text through oracle.spec, as
tests/slasher_model.py does); the rest is restated from the consensus specification's Altair/Bellatrix text
[UPSTREAM-MEMORY], the whistleblower always the proposer.

Two forms:
  block_operations_sequential   the specification's loop: one operation after the other, each on the state the earlier ones
                                left, Python integers.  THE specification of the call.
  block_operations_closed_form  what the kernels compute: candidates in (operation, index) order, per validator the first
                                potent candidate and the first potent slashing candidate, exit epochs by rank in the queue's
                                closed form, the proposer's balance in one expression.
tests/test_block_ops_model.py holds one to the other; the GPU tests compare the engine with the sequential form.

A registry is registry_updates_model's dict of arrays (act, ext, wdr, eff, slashed, bal are read).  An operation is a dict:
  attester_slashing(d1, d2, i1, i2, sig)   d1, d2: 128 bytes of AttestationData as a pe_attestation begins
  proposer_slashing(slot1, prop1, root1, slot2, prop2, root2, sig)
  voluntary_exit(index, epoch, sig)
A block with an invalid operation is an invalid block: every status is returned and the registry is unchanged; the statuses
behind the first invalid operation are those the operations get on the state the earlier VALID ones leave.
ValueError = the call the engine refuses with PE_ERR_INVALID_ARG."""
import struct
from dataclasses import dataclass

import numpy as np

from tests.registry_updates_model import ETH, FAR, U64, Params, activation_exit_epoch, churn_limits, copy_registry

PROPOSER_SLASHING, ATTESTER_SLASHING, VOLUNTARY_EXIT = 1, 2, 3
OK = 0
(NOT_SLASHABLE_DATA, BAD_INDICES, BAD_SIGNATURE, NOBODY_SLASHABLE, HEADER_MISMATCH, PROPOSER_NOT_SLASHABLE, NOT_ACTIVE,
 ALREADY_EXITING, EXIT_EPOCH_FUTURE, TOO_YOUNG) = range(64, 74)
STATS = ("n_active", "churn_limit", "n_slashed", "n_exits_initiated", "first_exit_epoch", "last_exit_epoch", "slashed_balance",
         "proposer_rewards", "penalties", "n_saturated", "n_invalid")


@dataclass
class BlockParams(Params):
    """pe_block_ops_params: Bellatrix's quotient by default (Altair: 64); the exit queue's constants are Params'."""
    min_slashing_penalty_quotient: int = 32
    whistleblower_reward_quotient: int = 512
    epochs_per_slashings_vector: int = 8192
    shard_committee_period: int = 256


def attester_slashing(d1: bytes, d2: bytes, i1, i2, sig: bool = True) -> dict:
    assert len(d1) == 128 and len(d2) == 128
    return dict(kind=ATTESTER_SLASHING, d1=bytes(d1), d2=bytes(d2), i1=[int(x) for x in i1], i2=[int(x) for x in i2], sig=bool(sig))


def proposer_slashing(slot1, prop1, root1, slot2, prop2, root2, sig: bool = True) -> dict:
    return dict(kind=PROPOSER_SLASHING, slot1=int(slot1), prop1=int(prop1), root1=bytes(root1), slot2=int(slot2), prop2=int(prop2),
                root2=bytes(root2), sig=bool(sig))


def voluntary_exit(index, epoch, sig: bool = True) -> dict:
    return dict(kind=VOLUNTARY_EXIT, index=int(index), epoch=int(epoch), sig=bool(sig))


def att_data(slot=0, index=0, block_root=bytes(32), source_epoch=0, source_root=bytes(32), target_epoch=0, target_root=bytes(32)) -> bytes:
    """AttestationData as the leading 128 bytes of a pe_attestation."""
    return struct.pack("<QQ32sQ32sQ32s", slot, index, block_root, source_epoch, source_root, target_epoch, target_root)


def double_vote(target_epoch: int, tag: int = 0):
    """Two different AttestationData with one target epoch."""
    return (att_data(target_epoch=target_epoch, source_epoch=max(target_epoch, 1) - 1, block_root=bytes([1 + tag % 250]) * 32),
            att_data(target_epoch=target_epoch, source_epoch=max(target_epoch, 1) - 1, block_root=bytes([2 + tag % 250]) * 32))


def slashable_data(d1: bytes, d2: bytes) -> bool:
    """is_slashable_attestation_data: the reference's text over the two AttestationData."""
    from oracle import spec

    def data(b):
        slot, index, bbr, se, sr, te, tr = struct.unpack("<QQ32sQ32sQ32s", b)
        return spec.AttestationData(slot=slot, index=index, beacon_block_root=spec.Root(bbr),
                                    source=spec.Checkpoint(se, spec.Root(sr)), target=spec.Checkpoint(te, spec.Root(tr)))
    return bool(spec.is_slashable_attestation_data(data(d1), data(d2)))


def valid_index_list(idx, n: int) -> bool:
    """the structural part of is_valid_indexed_attestation, and every index in the registry"""
    return len(idx) > 0 and all(0 <= x < n for x in idx) and all(idx[k] < idx[k + 1] for k in range(len(idx) - 1))


def check_call(n: int, cur: int, proposer: int, p: BlockParams):
    if not 0 <= proposer < n:
        raise ValueError("the proposer lies outside the registry")
    if p.min_slashing_penalty_quotient == 0 or p.whistleblower_reward_quotient == 0:
        raise ValueError("a quotient is 0")
    if cur + p.epochs_per_slashings_vector >= FAR:
        raise ValueError("current_epoch + epochs_per_slashings_vector reaches FAR_FUTURE_EPOCH")


def check_sums(st: dict, max_eff_slashed: int, proposer_balance: int, p: BlockParams):
    """What the engine refuses before it writes: an exit epoch whose withdrawable epoch reaches FAR, and sums that could
    leave 64 bits (bounded by the slashed validators' count times their largest effective balance, over the proposer's
    balance: every reward, every sum of rewards and the slashed balance lie below that)."""
    if st["n_exits_initiated"] and st["last_exit_epoch"] + p.min_validator_withdrawability_delay >= FAR:
        raise ValueError("the last exit epoch + min_validator_withdrawability_delay reaches FAR_FUTURE_EPOCH")
    if st["n_slashed"] * max_eff_slashed + proposer_balance >= U64:
        raise ValueError("the slashed balance and the proposer's rewards can exceed 64 bits")


# ------------------------------------------------------------------ the specification's loop
def initiate_validator_exit(ext, wdr, i: int, target: int, limit: int, delay: int, st: dict):
    """ext, wdr: lists of Python integers, written in place.  target = compute_activation_exit_epoch(current_epoch)."""
    if ext[i] != FAR:
        return
    q = max([e for e in ext if e != FAR] + [target])
    if sum(1 for e in ext if e == q) >= limit:
        q += 1
    ext[i] = q
    wdr[i] = q + delay
    if st["n_exits_initiated"] == 0:
        st["first_exit_epoch"] = q
    st["last_exit_epoch"] = q
    st["n_exits_initiated"] += 1


def block_operations_sequential(a: dict, cur: int, proposer: int, ops, p: BlockParams = BlockParams()):
    """-> (the registry after the call, one status per operation, stats by the names of pe_block_ops_stats).  `a` is not
    written.  With an invalid operation the registry returned is `a`'s copy and the stats hold n_active, churn_limit and
    n_invalid alone."""
    act, ext, wdr, eff, bal = ([int(x) for x in a[k]] for k in ("act", "ext", "wdr", "eff", "bal"))
    slashed = [int(x) for x in a["slashed"]]
    n = len(eff)
    check_call(n, cur, proposer, p)
    n_active = sum(1 for v in range(n) if act[v] <= cur < ext[v])
    limit, _ = churn_limits(n_active, p)
    target = activation_exit_epoch(cur, p)
    st = dict.fromkeys(STATS, 0)
    st.update(n_active=n_active, churn_limit=limit)
    max_eff_slashed, proposer_balance = 0, bal[proposer]

    def slashable(i):
        return not slashed[i] and act[i] <= cur < wdr[i]

    def slash_validator(i):
        nonlocal max_eff_slashed
        initiate_validator_exit(ext, wdr, i, target, limit, p.min_validator_withdrawability_delay, st)
        slashed[i] = 1
        wdr[i] = max(wdr[i], cur + p.epochs_per_slashings_vector)
        st["slashed_balance"] += eff[i]
        penalty = eff[i] // p.min_slashing_penalty_quotient
        if penalty > bal[i]:
            st["n_saturated"] += 1
            penalty = bal[i]
        bal[i] -= penalty
        st["penalties"] += penalty
        reward = eff[i] // p.whistleblower_reward_quotient     # proposer_reward + (whistleblower_reward - proposer_reward)
        bal[proposer] += reward
        st["proposer_rewards"] += reward
        st["n_slashed"] += 1
        max_eff_slashed = max(max_eff_slashed, eff[i])

    def apply(op) -> int:
        if op["kind"] == ATTESTER_SLASHING:
            if not slashable_data(op["d1"], op["d2"]):
                return NOT_SLASHABLE_DATA
            if not valid_index_list(op["i1"], n) or not valid_index_list(op["i2"], n):
                return BAD_INDICES
            if not op["sig"]:
                return BAD_SIGNATURE
            slashed_any = False
            for i in sorted(set(op["i1"]) & set(op["i2"])):
                if slashable(i):
                    slash_validator(i)
                    slashed_any = True
            return OK if slashed_any else NOBODY_SLASHABLE
        if op["kind"] == PROPOSER_SLASHING:
            if op["slot1"] != op["slot2"] or op["prop1"] != op["prop2"] or op["root1"] == op["root2"]:
                return HEADER_MISMATCH
            i = op["prop1"]
            if i >= n:
                return BAD_INDICES
            if not slashable(i):
                return PROPOSER_NOT_SLASHABLE
            if not op["sig"]:
                return BAD_SIGNATURE
            slash_validator(i)
            return OK
        assert op["kind"] == VOLUNTARY_EXIT
        i = op["index"]
        if i >= n:
            return BAD_INDICES
        if not act[i] <= cur < ext[i]:
            return NOT_ACTIVE
        if ext[i] != FAR:
            return ALREADY_EXITING
        if not cur >= op["epoch"]:
            return EXIT_EPOCH_FUTURE
        if not cur >= act[i] + p.shard_committee_period:
            return TOO_YOUNG
        if not op["sig"]:
            return BAD_SIGNATURE
        initiate_validator_exit(ext, wdr, i, target, limit, p.min_validator_withdrawability_delay, st)
        return OK

    status = [apply(op) for op in ops]
    n_invalid = sum(1 for s in status if s != OK)
    if n_invalid:
        st = dict.fromkeys(STATS, 0)
        st.update(n_active=n_active, churn_limit=limit, n_invalid=n_invalid)
        return copy_registry(a), status, st
    check_sums(st, max_eff_slashed, proposer_balance, p)
    out = copy_registry(a)
    for k, x in (("ext", ext), ("wdr", wdr), ("bal", bal)):
        out[k] = np.array(x, dtype=np.uint64)
    out["slashed"] = np.array(slashed, dtype=np.uint8)
    return out, status, st


# ------------------------------------------------------------------ ... and what the kernels compute
def block_operations_closed_form(a: dict, cur: int, proposer: int, ops, p: BlockParams = BlockParams()):
    """The same call without a loop-carried registry: every decision from the registry as it was and two minima per validator."""
    from tests.registry_updates_model import exit_queue_start
    out = copy_registry(a)
    act, ext, wdr, eff, bal, sl = (a[k] for k in ("act", "ext", "wdr", "eff", "bal", "slashed"))
    n = eff.size
    check_call(n, cur, proposer, p)
    c = np.uint64(cur)
    active0 = (act <= c) & (c < ext)
    slashable0 = (sl == 0) & (act <= c) & (c < wdr)
    n_active = int(active0.sum())
    limit, _ = churn_limits(n_active, p)
    target = activation_exit_epoch(cur, p)
    # candidates in (operation, index) order: (op, kind, validator, potent); the host-decided statuses
    status = [OK] * len(ops)
    cand = []
    for o, op in enumerate(ops):
        if op["kind"] == ATTESTER_SLASHING:
            if not slashable_data(op["d1"], op["d2"]):
                status[o] = NOT_SLASHABLE_DATA
            elif not valid_index_list(op["i1"], n) or not valid_index_list(op["i2"], n):
                status[o] = BAD_INDICES
            elif not op["sig"]:
                status[o] = BAD_SIGNATURE
            else:
                second = set(op["i2"])
                cand += [(o, ATTESTER_SLASHING, v, bool(slashable0[v])) for v in op["i1"] if v in second]
        elif op["kind"] == PROPOSER_SLASHING:
            if op["slot1"] != op["slot2"] or op["prop1"] != op["prop2"] or op["root1"] == op["root2"]:
                status[o] = HEADER_MISMATCH
            elif op["prop1"] >= n:
                status[o] = BAD_INDICES
            else:
                v = op["prop1"]
                cand.append((o, PROPOSER_SLASHING, v, bool(slashable0[v]) and op["sig"]))
        else:
            v = op["index"]
            if v >= n:
                status[o] = BAD_INDICES
            else:
                static = (bool(active0[v]) and int(ext[v]) == FAR and cur >= op["epoch"]
                          and cur - int(act[v]) >= p.shard_committee_period and op["sig"])
                cand.append((o, VOLUNTARY_EXIT, v, static))
    first_potent, first_slash = {}, {}
    for s, (o, kind, v, potent) in enumerate(cand):
        if potent:
            first_potent.setdefault(v, s)
            if kind != VOLUNTARY_EXIT:
                first_slash.setdefault(v, s)
    fresh = np.zeros(len(cand), dtype=bool)
    slash = np.zeros(len(cand), dtype=bool)
    hit = [False] * len(ops)
    for s, (o, kind, v, potent) in enumerate(cand):
        op = ops[o]
        slash[s] = potent and kind != VOLUNTARY_EXIT and first_slash[v] == s
        fresh[s] = potent and first_potent[v] == s and int(ext[v]) == FAR
        hit[o] = hit[o] or bool(slash[s])
        if kind == PROPOSER_SLASHING:
            if not slashable0[v] or first_slash.get(v, s) < s:
                status[o] = PROPOSER_NOT_SLASHABLE
            elif not op["sig"]:
                status[o] = BAD_SIGNATURE
        elif kind == VOLUNTARY_EXIT:
            if not active0[v]:
                status[o] = NOT_ACTIVE
            elif int(ext[v]) != FAR or first_potent.get(v, s) < s:
                status[o] = ALREADY_EXITING
            elif not cur >= op["epoch"]:
                status[o] = EXIT_EPOCH_FUTURE
            elif not cur - int(act[v]) >= p.shard_committee_period:
                status[o] = TOO_YOUNG
            elif not op["sig"]:
                status[o] = BAD_SIGNATURE
    for o, op in enumerate(ops):
        if op["kind"] == ATTESTER_SLASHING and status[o] == OK and not hit[o]:
            status[o] = NOBODY_SLASHABLE
    st = dict.fromkeys(STATS, 0)
    st.update(n_active=n_active, churn_limit=limit, n_invalid=sum(1 for x in status if x != OK))
    if st["n_invalid"]:
        return out, status, st
    who = np.array([v for _, _, v, _ in cand], dtype=np.int64)
    v_slash, v_fresh = who[slash], who[fresh]
    reward = eff[v_slash] // np.uint64(p.whistleblower_reward_quotient)
    before = np.concatenate([[0], np.cumsum(reward.astype(object))])[:-1] if reward.size else np.zeros(0, dtype=object)
    total = int(reward.astype(object).sum()) if reward.size else 0
    base, fill = exit_queue_start(ext, target, limit)
    st.update(n_slashed=int(v_slash.size), n_exits_initiated=int(v_fresh.size), proposer_rewards=total,
              slashed_balance=int(eff[v_slash].astype(object).sum()) if v_slash.size else 0)
    if v_fresh.size:
        q = [base + (fill + k) // limit for k in range(v_fresh.size)]
        st["first_exit_epoch"], st["last_exit_epoch"] = q[0], q[-1]
    check_sums(st, int(eff[v_slash].max()) if v_slash.size else 0, int(bal[proposer]), p)
    if v_fresh.size:
        out["ext"][v_fresh] = np.array(q, dtype=np.uint64)
        out["wdr"][v_fresh] = np.array(q, dtype=np.uint64) + np.uint64(p.min_validator_withdrawability_delay)
    out["slashed"][v_slash] = 1
    out["wdr"][v_slash] = np.maximum(out["wdr"][v_slash], np.uint64(cur + p.epochs_per_slashings_vector))
    proposer_done = False
    for j, v in enumerate(v_slash):
        penalty = int(eff[v]) // p.min_slashing_penalty_quotient
        b = int(bal[v]) + (int(before[j]) if v == proposer else 0)
        cut = min(penalty, b)
        st["n_saturated"] += penalty > b
        st["penalties"] += cut
        b -= cut
        if v == proposer:
            b += total - int(before[j])
            proposer_done = True
        out["bal"][v] = np.uint64(b)
    if not proposer_done:
        out["bal"][proposer] = np.uint64(int(bal[proposer]) + total)
    return out, status, st


def view_slashed_flags(flags: np.ndarray, slashed: np.ndarray) -> np.ndarray:
    """the working-state view's flag bytes with PE_VAL_SLASHED as `slashed` says"""
    return ((np.asarray(flags, dtype=np.uint8) & np.uint8(0xFD)) | (np.asarray(slashed, dtype=np.uint8) << 1)).astype(np.uint8)
