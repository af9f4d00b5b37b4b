#!/usr/bin/env python
"""Regenerates tests/golden/epoch_vectors.json by RUNNING THE REFERENCE'S OWN pyspec text for the two epoch-boundary
functions: compute_proposer_index (pe:604-618) and process_effective_balance_updates (pe:122-133).

Their fences are taken from the reference's Markdown at run time (oracle/ref_extract.py) and executed in a copy of
``oracle.spec``'s namespace plus the three hysteresis constants ``spec`` lacks.  The file holds data
only: inputs and the outputs those fences gave.  compute_proposer_index never returns for a registry that accepts nobody;
the runner below bounds it from outside (its callee compute_shuffled_index is counted and the run is abandoned at call
max_tries + 1), the function's text is not touched.

    python tests/golden/generate_epoch.py          # rewrites epoch_vectors.json (needs the reference's Markdown)
"""
import __future__
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

from oracle import ref_extract, spec  # noqa: E402

OUT = os.path.join(HERE, "epoch_vectors.json")
ETH = 10**9
MAX_EFF = 32 * ETH
HYSTERESIS = dict(HYSTERESIS_QUOTIENT=4, HYSTERESIS_DOWNWARD_MULTIPLIER=1, HYSTERESIS_UPWARD_MULTIPLIER=5)
LATE_CLASSES = [0, 31, 32, 63, 64, 128]   # accepting i; the last one stands for "i >= 128"
N_ACTIVE = [1, 2, 3, 255, 256, 257, 1000]


class _Exhausted(Exception):
    pass


def reference_namespace() -> dict:
    """A copy of oracle.spec's namespace with the two fences executed in it."""
    by_name = ref_extract.index_fences(ref_extract.fences())
    ns = dict(vars(spec))
    ns.update(HYSTERESIS)
    for name in ("compute_proposer_index", "process_effective_balance_updates"):
        fence = by_name[name]
        # postponed evaluation of annotations: BeaconState / Bytes32 / Sequence[ValidatorIndex] stay strings
        exec(compile(fence.code, f"<pe:{fence.first}-{fence.last}>", "exec", flags=__future__.annotations.compiler_flag,
                     dont_inherit=True), ns)
    return ns


def ref_proposer(ns, indices, effective_balance, seed, rounds, max_eff, max_tries):
    """The fence's compute_proposer_index -> (validator | None, tries)."""
    state = spec.BeaconState(validators=[spec.Validator(effective_balance=int(b)) for b in effective_balance])
    calls = [0]
    shuffled = spec.compute_shuffled_index

    def counted(index, index_count, seed_):
        if calls[0] == max_tries:
            raise _Exhausted()
        calls[0] += 1
        return shuffled(index, index_count, seed_)

    saved_rounds = spec.SHUFFLE_ROUND_COUNT
    spec.SHUFFLE_ROUND_COUNT = rounds
    ns["MAX_EFFECTIVE_BALANCE"] = max_eff
    ns["compute_shuffled_index"] = counted
    try:
        return int(ns["compute_proposer_index"](state, [int(i) for i in indices], bytes(seed))), calls[0] - 1
    except _Exhausted:
        return None, max_tries
    finally:
        spec.SHUFFLE_ROUND_COUNT = saved_rounds
        ns["compute_shuffled_index"] = shuffled


def ref_balance_updates(ns, balances, eff, increment, quotient, down, up, max_eff):
    """The fence's process_effective_balance_updates -> the new effective balances."""
    ns.update(EFFECTIVE_BALANCE_INCREMENT=increment, HYSTERESIS_QUOTIENT=quotient, HYSTERESIS_DOWNWARD_MULTIPLIER=down,
              HYSTERESIS_UPWARD_MULTIPLIER=up, MAX_EFFECTIVE_BALANCE=max_eff)
    state = spec.BeaconState(validators=[spec.Validator(effective_balance=int(e)) for e in eff],
                             balances=[int(b) for b in balances])
    ns["process_effective_balance_updates"](state)
    return [int(v.effective_balance) for v in state.validators]


def expand_eff(row):
    """effective balances (Gwei) of a proposer row: eff_eth is one number for the whole registry, or a list."""
    e = row["eff_eth"]
    return [e * ETH] * row["n_val"] if isinstance(e, int) else [x * ETH for x in e]


def expand_indices(row):
    return list(range(row["n_active"])) if row["indices"] is None else row["indices"]


def _first_accepting_i(seed, threshold_byte, limit):
    """With equal balances the accepting i depends on the random bytes alone: a cheap search for seeds of a wanted class
    (the expected outputs still come from the fence)."""
    for q in range((limit + 31) // 32):
        d = hashlib.sha256(seed + q.to_bytes(8, "little")).digest()
        for j in range(32):
            if d[j] <= threshold_byte and 32 * q + j < limit:
                return 32 * q + j
    return None


def proposer_rows(ns):
    rows = []

    def add(tag, seed, rounds, n_val, eff_eth, indices, max_tries):
        row = {"tag": tag, "seed": seed.hex(), "rounds": rounds, "n_val": n_val, "eff_eth": eff_eth,
               "n_active": n_val if indices is None else len(indices), "indices": indices, "max_eff": MAX_EFF,
               "max_tries": max_tries}
        got, tries = ref_proposer(ns, expand_indices(row), expand_eff(row), seed, rounds, MAX_EFF, max_tries or 4096)
        row["proposer"], row["tries"] = got, tries
        rows.append(row)

    # late acceptance: 3 validators of 1 ETH accept a try with probability 1/32 (random byte <= 7)
    want, k = dict.fromkeys(LATE_CLASSES), 0
    while any(v is None for v in want.values()):
        seed = hashlib.sha256(b"s%d" % k).digest()
        i = _first_accepting_i(seed, 7, 4096)
        cls = 128 if i is not None and i >= 128 else i
        if cls in want and want[cls] is None:
            want[cls] = seed
        k += 1
    for cls in LATE_CLASSES:
        add("late", want[cls], 90, 3, 1, None, 0)
    # a registry without balance accepts only through a random byte of 0: both outcomes within 128 tries
    found, k = {True: [], False: []}, 0
    while len(found[True]) < 2 or len(found[False]) < 2:
        seed = hashlib.sha256(b"z%d" % k).digest()
        hit = _first_accepting_i(seed, 0, 128) is not None
        if len(found[hit]) < 2:
            found[hit].append(seed)
        k += 1
    for seed in found[True] + found[False]:
        add("zero", seed, 10, 5, 0, None, 128)
    # the kernel's shape edges: position // 256 and i % total
    rng = np.random.default_rng(604)
    for n_active in N_ACTIVE:
        for kind in ("full", "one", "mixed"):
            rounds = 10 if kind == "one" else 90
            subset = n_active in (3, 257) or (n_active == 1000 and kind == "mixed")
            n_val = n_active + 37 if subset else n_active
            indices = sorted(int(x) for x in rng.choice(n_val, size=n_active, replace=False)) if subset else None
            if kind == "mixed":
                eff_eth = [int(x) for x in rng.choice([0, 0, 1, 7, 16, 31, 32], size=n_val)]
                eff_eth[(indices or [0])[0]] = 32   # never a registry of zeros: the fence would not return
            else:
                eff_eth = 32 if kind == "full" else 1
            seed = hashlib.sha256(b"e%d-%s" % (n_active, kind.encode())).digest()
            add("edge", seed, rounds, n_val, eff_eth, indices, 0)
    return rows


def hysteresis_rows(ns):
    """One row = one registry: parallel lists of effective balance, balance and the fence's answer."""
    quarter = ETH // 4
    eff, bal = [], []
    for n in (1, 2, 16, 31, 32):
        e = n * ETH
        for centre in (e - quarter, e + 5 * quarter):       # the two thresholds and one Gwei either side
            for d in (-1, 0, 1):
                eff.append(e)
                bal.append(centre + d)
        eff += [e, e, e, e]
        bal += [40 * ETH, 33 * ETH + quarter + 1, ETH - 1, 0]   # above the cap (twice), below one increment, nothing
    eff += [0, 0, 0, 0, 32 * ETH]
    bal += [0, 5 * quarter, 5 * quarter + 1, ETH - 1, 32 * ETH]
    rows = [{"tag": "thresholds", "eff": eff, "balances": bal}]
    rng = np.random.default_rng(122)
    e = rng.integers(0, 33, size=64) * ETH
    b = np.clip(e + rng.integers(-3 * ETH, 3 * ETH, size=64), 0, None)
    rows.append({"tag": "random", "eff": [int(x) for x in e], "balances": [int(x) for x in b]})
    # other constants: a coarser increment and a lower cap
    rows.append({"tag": "constants", "eff": [int(x) for x in e], "balances": [int(x) for x in b], "increment": 2 * ETH,
                 "quotient": 8, "down": 3, "up": 7, "max_eff": 20 * ETH})
    for row in rows:
        row.setdefault("increment", ETH)
        row.setdefault("quotient", 4)
        row.setdefault("down", 1)
        row.setdefault("up", 5)
        row.setdefault("max_eff", MAX_EFF)
        row["new"] = ref_balance_updates(ns, row["balances"], row["eff"], row["increment"], row["quotient"], row["down"],
                                         row["up"], row["max_eff"])
        row["n_changed"] = sum(1 for a, c in zip(row["eff"], row["new"]) if a != c)
    return rows


def render() -> str:
    """The file's text: one JSON object per line, so that a diff shows the row that changed."""
    ns = reference_namespace()
    lines = ['{"proposer": ' + json.dumps(r, sort_keys=True) + "}" for r in proposer_rows(ns)]
    lines += ['{"hysteresis": ' + json.dumps(r, sort_keys=True) + "}" for r in hysteresis_rows(ns)]
    return "[\n" + ",\n".join(lines) + "\n]\n"


def load(path: str = OUT):
    rows = json.load(open(path))
    return [r["proposer"] for r in rows if "proposer" in r], [r["hysteresis"] for r in rows if "hysteresis" in r]


if __name__ == "__main__":
    if not ref_extract.reference_available():
        sys.exit("the reference's Markdown is not on this machine: epoch_vectors.json is written from its text only")
    open(OUT, "w").write(render())
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
