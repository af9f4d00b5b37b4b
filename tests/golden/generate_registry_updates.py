"""Writes tests/golden/registry_updates_vectors.json from the SEQUENTIAL form of tests/registry_updates_model.py: small
registries, the specification's loop, the arrays and statistics it leaves.  Run from the repository root:
    python tests/golden/generate_registry_updates.py"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import registry_updates_model as M  # noqa: E402


def to_json(a: dict) -> dict:
    return {k: [int(x) for x in a[k]] for k in M.FIELDS}


def from_json(d: dict) -> dict:
    return M.copy_registry(d)


def record(name, a, cur, fin, p, vector=64, sums=(0, 5 * M.ETH, 10**12)):
    after, st = M.registry_updates_sequential(a, cur, fin, p)
    flags = M.view_flags(a, cur)
    sl = []
    for sum_slashings in sums:
        bal, sst = M.slashings_sequential(a, flags, cur, sum_slashings, 3, vector)
        sl.append(dict(sum_slashings=sum_slashings, balances=[int(x) for x in bal], stats=sst))
    return dict(name=name, current_epoch=cur, finalized_epoch=fin, params=p.abi(), vector=vector, registry=to_json(a),
                after={k: [int(x) for x in after[k]] for k in ("elig", "act", "ext", "wdr")}, stats=st, slashings=sl)


def cases():
    out = []
    # every class of random_registry (256 validators is the smallest registry that holds them all): ejections that spill
    # over epochs, a queue longer than the cap, marks, penalties on both sides of the min, saturating ones
    p = M.Params(min_per_epoch_churn_limit=2, max_per_epoch_activation_churn_limit=3)
    a, counters = M.random_registry(256, 1, 20, 18, p, vector=64)
    assert M.every_class_occurred(counters)
    out.append(record("every class, churn limit 2, activation cap 3", a, 20, 18, p, sums=(0, 5 * M.ETH, 10**15)))
    # the exit queue: an exit beyond the look-ahead epoch half full, seven ejections over four epochs, no-ops between them
    a, p = M.exit_queue_case(60, 20, 2, 1, True, 7, True)
    out.append(record("exit queue: churn limit 2, E0 beyond the look-ahead, c0 = 1, 7 ejections", a, 20, 18, p))
    a, p = M.exit_queue_case(40, 20, 1, 2, False, 4, True)
    out.append(record("exit queue: churn limit 1, E0 the look-ahead epoch over full, 4 ejections", a, 20, 18, p))
    # the quotient decides the churn limit: 64 active validators / 8 = 8 > 4; ten ejections, a queue of twelve, and
    # slashed validators at the target epoch, two of them with less balance than the penalty
    p = M.Params(churn_limit_quotient=8)
    a = M.blank_registry(72, p)
    a["act"][64:] = M.FAR                       # eight not yet active: n_active = 64
    a["elig"][64:] = [18, 17, 19, 18, 16, 18, M.FAR, 18]
    a["act"][[3, 9, 30, 31]] = M.FAR
    a["elig"][[3, 9, 30, 31]] = [18, 18, 17, 18]
    a["eff"][[1, 5, 6, 7, 20, 21, 40, 41, 42, 63]] = p.ejection_balance
    for v, bal in ((10, 40 * M.ETH), (11, 3), (12, 0), (13, 32 * M.ETH)):
        a["slashed"][v], a["wdr"][v], a["bal"][v], a["ext"][v] = 1, 20 + 32, bal, 25
    a["wdr"][13] = 20 + 33                      # slashed, one epoch off: untouched
    a["wdr"][14] = 20 + 32                      # at the epoch, not slashed: untouched
    out.append(record("the quotient decides: churn limit 8", a, 20, 18, p, sums=(0, 100 * M.ETH, 10**13)))
    a, _ = M.random_registry(1, 5, 2, 1, M.Params(), vector=64)
    out.append(record("one validator", a, 2, 1, M.Params()))
    return out


if __name__ == "__main__":
    with open(M.GOLDEN_PATH, "w") as f:
        json.dump(cases(), f, indent=None, separators=(",", ":"))
        f.write("\n")
    print(M.GOLDEN_PATH, os.path.getsize(M.GOLDEN_PATH), "bytes")
