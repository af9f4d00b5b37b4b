"""Registries and blocks of operations for the block-operations tests (tests/block_ops_model.py is the model): a seeded
generator whose classes the CPU test counts, and the small fixed shapes the GPU test runs."""
import numpy as np

from tests import block_ops_model as B
from tests.registry_updates_model import ETH, FAR, blank_registry

CUR = 1000
CLASSES = ("two_ops", "slash_already_exiting", "exit_after_slash_invalid", "proposer_first", "proposer_middle", "proposer_last",
           "saturated", "taken_invalid", "queue_beyond_lookahead", "full_epoch_skipped", "two_boundaries")


def params(limit: int = 4, **kw) -> B.BlockParams:
    return B.BlockParams(min_per_epoch_churn_limit=limit, churn_limit_quotient=1 << 40, **kw)


def registry(n: int, seed: int, c0: int, e0_beyond: bool, p: B.BlockParams, cur: int = CUR) -> dict:
    """n validators, most of them active, old enough and untouched; the last c0 leave at E0 (the look-ahead epoch or three
    beyond it); the rest draws from: leaving earlier, left and still slashable, withdrawn, slashed, not yet active, too young
    to exit, a balance too small for the penalty."""
    rng = np.random.default_rng(seed)
    a = blank_registry(n, p)
    a["bal"] = (a["eff"] + rng.integers(0, ETH, size=n, dtype=np.uint64)).astype(np.uint64)
    target = cur + 1 + p.max_seed_lookahead
    e0 = target + (3 if e0_beyond else 0)
    kind = rng.integers(0, 24, size=n)
    for v in range(n - c0):
        k = kind[v]
        if k == 0:
            a["ext"][v], a["wdr"][v] = target - 1, target - 1 + 256       # leaving before E0: still active, must not count
        elif k == 1:
            a["ext"][v], a["wdr"][v] = cur - 3, cur + 200                 # left, not withdrawable: slashable, not active
        elif k == 2:
            a["ext"][v], a["wdr"][v] = cur - 300, cur                     # withdrawable now: not slashable
        elif k == 3:
            a["slashed"][v], a["ext"][v], a["wdr"][v] = 1, target - 2, cur + 4000
        elif k == 4:
            a["act"][v] = cur + 1
        elif k == 5:
            a["act"][v] = cur - p.shard_committee_period + 1             # one epoch too young
        elif k == 6:
            a["act"][v] = cur - p.shard_committee_period
        elif k in (7, 8):
            a["bal"][v] = rng.integers(0, ETH // 2)
            a["eff"][v] = 17 * ETH
    a["ext"][n - c0:] = e0
    a["wdr"][n - c0:] = e0 + p.min_validator_withdrawability_delay
    return a


def slash_order(a, cur, ops, p):
    """the validators the block slashes, in the loop's order (the proposer's identity does not change it)"""
    out, status, _ = B.block_operations_sequential(a, cur, 0, ops, p)
    if any(status):
        return []
    newly = (out["slashed"] != 0) & (a["slashed"] == 0)
    order, seen = [], set()
    for op in ops:
        who = sorted(set(op["i1"]) & set(op["i2"])) if op["kind"] == B.ATTESTER_SLASHING else \
            [op["prop1"]] if op["kind"] == B.PROPOSER_SLASHING else []
        for v in who:
            if newly[v] and v not in seen:
                seen.add(v)
                order.append(v)
    return order


def random_block(n: int, seed: int, *, c0: int = 0, e0_beyond: bool = False, valid: bool = True, proposer_at: str = "none",
                 limit: int = 4, cur: int = CUR):
    """-> (registry, proposer, ops, params).  valid: operations the loop rejects are taken out until none is left; else the
    block also gets an exit of a validator it slashed and an attester slashing of validators it has already slashed.
    proposer_at: "first" / "middle" / "last" -- the proposer is that one of the slashed, with a balance the earlier rewards
    decide the saturation of -- or "none"."""
    p = params(limit)
    rng = np.random.default_rng(1000 + seed)
    a = registry(n, seed, c0, e0_beyond, p, cur)
    ops = []
    for t in range(int(rng.integers(3, 7))):
        kind = int(rng.integers(0, 4))
        if kind <= 1:
            pool = rng.choice(n, size=min(n, int(rng.integers(2, 40))), replace=False)
            i1 = sorted(int(x) for x in pool[: max(1, int(pool.size * 0.8))])
            i2 = sorted(int(x) for x in pool[int(pool.size * 0.3):])
            d1, d2 = B.double_vote(cur - 1 - t % 2, t)
            ops.append(B.attester_slashing(d1, d2, i1, i2))
        elif kind == 2:
            v = int(rng.integers(0, n))
            ops.append(B.proposer_slashing(5, v, bytes([t + 1]) * 32, 5, v, bytes([t + 101]) * 32))
        else:
            ops += [B.voluntary_exit(int(v), cur - int(rng.integers(0, 2))) for v in rng.choice(n, size=min(n, 5), replace=False)]
    if valid:
        while True:
            _, status, _ = B.block_operations_sequential(a, cur, 0, ops, p)
            if not any(status):
                break
            ops = [op for op, s in zip(ops, status) if s == B.OK]
    else:
        order = slash_order(a, cur, [op for op, s in zip(ops, B.block_operations_sequential(a, cur, 0, ops, p)[1]) if s == B.OK], p)
        fresh = [v for v in order if int(a["ext"][v]) == FAR and int(a["act"][v]) + p.shard_committee_period <= cur]
        if fresh:
            ops.append(B.voluntary_exit(fresh[0], cur))
        if len(order) >= 2:
            d1, d2 = B.double_vote(cur - 2, 77)
            ops.append(B.attester_slashing(d1, d2, sorted(order[:3]), sorted(order[:3])))
    order = slash_order(a, cur, ops, p) if valid else []
    proposer = int(rng.integers(0, n))
    if proposer_at != "none" and len(order) >= 3:
        proposer = order[{"first": 0, "middle": len(order) // 2, "last": -1}[proposer_at]]
        a["bal"][proposer] = int(a["eff"][proposer]) // p.min_slashing_penalty_quotient - \
            (int(a["eff"][proposer]) // p.whistleblower_reward_quotient) * (len(order) // 4) - 7
    return a, proposer, ops, p


def classes_of(a, cur, proposer, ops, p) -> dict:
    """which of CLASSES this block shows, from its inputs and what the loop makes of them"""
    out, status, st = B.block_operations_sequential(a, cur, proposer, ops, p)
    c = dict.fromkeys(CLASSES, False)
    seen, slashing_seen = {}, set()
    slashable0 = (a["slashed"] == 0) & (a["act"] <= np.uint64(cur)) & (np.uint64(cur) < a["wdr"])
    for o, op in enumerate(ops):
        if op["kind"] == B.ATTESTER_SLASHING:
            who = sorted(set(op["i1"]) & set(op["i2"]))
        else:
            who = [op["prop1"] if op["kind"] == B.PROPOSER_SLASHING else op["index"]]
        who = [v for v in who if v < a["eff"].size]
        if any(v in seen for v in who):
            c["two_ops"] = True
        if op["kind"] == B.VOLUNTARY_EXIT and status[o] == B.ALREADY_EXITING and who and who[0] in slashing_seen \
                and int(a["ext"][who[0]]) == FAR:
            c["exit_after_slash_invalid"] = True
        if op["kind"] == B.ATTESTER_SLASHING and status[o] == B.NOBODY_SLASHABLE and who and all(slashable0[v] for v in who) \
                and all(v in slashing_seen for v in who):
            c["taken_invalid"] = True
        for v in who:
            seen[v] = o
            if op["kind"] != B.VOLUNTARY_EXIT and status[o] == B.OK:
                slashing_seen.add(v)
    if st["n_invalid"]:
        return c
    newly = (out["slashed"] != 0) & (a["slashed"] == 0)
    c["slash_already_exiting"] = bool((newly & (a["ext"] != np.uint64(FAR))).any())
    order = slash_order(a, cur, ops, p)
    if len(order) >= 3 and proposer in order:
        j = order.index(proposer)
        c["proposer_first"], c["proposer_last"] = j == 0, j == len(order) - 1
        c["proposer_middle"] = 0 < j < len(order) - 1
    c["saturated"] = st["n_saturated"] > 0
    target = cur + 1 + p.max_seed_lookahead
    set_ = a["ext"][a["ext"] != np.uint64(FAR)]
    if st["n_exits_initiated"] and set_.size:
        e0 = int(set_.max())
        c["queue_beyond_lookahead"] = e0 > target
        c["full_epoch_skipped"] = e0 >= target and int((set_ == np.uint64(e0)).sum()) >= st["churn_limit"]
    c["two_boundaries"] = st["n_exits_initiated"] > 0 and st["last_exit_epoch"] - st["first_exit_epoch"] >= 2
    return c


# the knobs the CPU test walks: every class occurs among them (test_every_class_occurred)
GRID = [dict(n=n, seed=seed, c0=c0, e0_beyond=beyond, valid=valid, proposer_at=at)
        for seed, (n, c0, beyond, valid, at) in enumerate(
            [(97, 0, False, True, "first"), (97, 3, False, True, "middle"), (97, 4, False, True, "last"),
             (130, 5, True, True, "none"), (130, 2, True, True, "middle"), (64, 0, False, False, "none"),
             (64, 3, True, False, "none"), (257, 1, False, True, "first"), (257, 4, True, True, "last"),
             (300, 0, False, False, "none"), (33, 2, False, True, "none"), (33, 0, True, False, "none")] * 2)]
