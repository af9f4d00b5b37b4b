#!/usr/bin/env python
"""Regenerates tests/golden/registry_vectors.json by RUNNING THE REFERENCE'S OWN pyspec text for the three functions that
count the active set: get_committee_count_per_slot (pe:461-468), compute_weak_subjectivity_period (pe:1257-1287) and
get_latest_weak_subjectivity_checkpoint_epoch (pe:1225-1241).

Their fences are taken from the reference's Markdown at run time (oracle/ref_extract.py) and executed as they stand in a
namespace that holds the constants they name (mainnet values) and, for the callees whose text the reference does not give
(get_active_validator_indices, get_current_epoch, get_total_active_balance, get_validator_churn_limit), the model of
tests/registry_model.py.  The file holds data only: a registry described by four numbers, and what the fences answered.

    python tests/golden/generate_registry.py       # rewrites registry_vectors.json (needs the reference's Markdown)
"""
import __future__
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

from oracle import ref_extract  # noqa: E402
from tests import registry_model as M  # noqa: E402

OUT = os.path.join(HERE, "registry_vectors.json")
ETH = 10**9
FENCES = ("get_committee_count_per_slot", "compute_weak_subjectivity_period", "get_latest_weak_subjectivity_checkpoint_epoch")
CONSTANTS = dict(SLOTS_PER_EPOCH=32, MAX_COMMITTEES_PER_SLOT=64, TARGET_COMMITTEE_SIZE=128,
                 MIN_VALIDATOR_WITHDRAWABILITY_DELAY=256, MIN_PER_EPOCH_CHURN_LIMIT=4, CHURN_LIMIT_QUOTIENT=65536,
                 MAX_DEPOSITS=16, SAFETY_DECAY=10, ETH_TO_GWEI=ETH, MAX_EFFECTIVE_BALANCE=32 * ETH)


def reference_namespace() -> dict:
    """The constants, the model's callees and the three fences executed on top of them."""
    by_name = ref_extract.index_fences(ref_extract.fences())
    ns = dict(CONSTANTS, uint64=int, **M.callees(CONSTANTS["SLOTS_PER_EPOCH"], ETH, CONSTANTS["MIN_PER_EPOCH_CHURN_LIMIT"],
                                                 CONSTANTS["CHURN_LIMIT_QUOTIENT"]))
    for name in FENCES:
        fence = by_name[name]
        # postponed evaluation of annotations: BeaconState / Epoch stay strings
        exec(compile(fence.code, f"<pe:{fence.first}-{fence.last}>", "exec", flags=__future__.annotations.compiler_flag,
                     dont_inherit=True), ns)
    return ns


def registry(row):
    """The row's registry -> (activation_epoch, exit_epoch, effective_balance): the first n_active validators are active
    in the epoch of row["slot"], the others alternate between exited in that very epoch and activated in the next one."""
    n_val, n_active = row["n_val"], row["n_active"]
    epoch = row["slot"] // CONSTANTS["SLOTS_PER_EPOCH"]
    activation = np.zeros(n_val, dtype=np.uint64)
    exit_ = np.full(n_val, M.FAR_FUTURE_EPOCH, dtype=np.uint64)
    rest = np.arange(n_active, n_val)
    exit_[rest[0::2]] = epoch
    activation[rest[1::2]] = epoch + 1
    return activation, exit_, np.full(n_val, row["eff_eth"] * ETH, dtype=np.uint64)


def state_of(row):
    return M.make_state(row["slot"], *registry(row), finalized_epoch=row["finalized_epoch"])


def _plain(x):
    """ints stay ints, floats stay floats (pe:1236 / pe:1239 divide truly): what json writes back unchanged."""
    return float(x) if isinstance(x, float) else int(x)


def answer(ns, row):
    state = state_of(row)
    epoch = row["slot"] // CONSTANTS["SLOTS_PER_EPOCH"]
    active = M.active_mask(state.activation_epoch, state.exit_epoch, epoch)
    out = {"total_active_balance": M.total_balance(state.effective_balance, active, ETH),
           "churn_limit": M.churn_limit(int(active.sum())),
           "count_per_slot": _plain(ns["get_committee_count_per_slot"](state, epoch)),
           "ws_checkpoint_epoch": _plain(ns["get_latest_weak_subjectivity_checkpoint_epoch"](state, row["safety_decay"]))}
    if row["n_active"]:   # pe:1268 divides by the count
        out["ws_period"] = _plain(ns["compute_weak_subjectivity_period"](state))
    else:
        out["ws_period"] = None
    return out


def rows(ns):
    out = []

    def add(tag, n_active, eff_eth=32, slot=32 * 1000, finalized_epoch=998, safety_decay=0.1, extra=3):
        row = {"tag": tag, "n_val": n_active + extra, "n_active": n_active, "eff_eth": eff_eth, "slot": slot,
               "finalized_epoch": finalized_epoch, "safety_decay": safety_decay}
        row.update(answer(ns, row))
        out.append(row)

    # pe:465: max(1, ...) below one committee of the target size per slot, min(MAX_COMMITTEES_PER_SLOT, ...) above 64 of them,
    # and the worked example of pe:472 (262 144 active validators -> 64 committees per slot)
    for n in (0, 1, 4095, 4096, 4097, 8191, 8192, 100000, 262143, 262144, 262145, 1048576):
        add("count", n)
    # pe:1274: T (200 + 3 D) < t (200 + 12 D), with D = 10 and T = 32: true from t = 24 ETH of average balance upwards
    for n in (1000, 32768, 262144, 1048576):
        for eff in (32, 24, 23, 16, 1):
            add("period", n, eff_eth=eff)
    add("period", 4194304, eff_eth=32)
    # pe:1235: val_count >= MIN_PER_EPOCH_CHURN_LIMIT * CHURN_LIMIT_QUOTIENT = 262 144, either side, and other arguments
    for n in (262143, 262144, 40000, 600000):
        for finalized, decay in ((0, 0.1), (998, 0.1), (100000, 0.1), (100000, 0.5), (3327, 0.1)):
            add("checkpoint", n, finalized_epoch=finalized, safety_decay=decay, slot=32 * (finalized + 2))
    return out


def render() -> str:
    """The file's text: one JSON object per line, so that a diff shows the row that changed."""
    ns = reference_namespace()
    return "[\n" + ",\n".join(json.dumps(r, sort_keys=True) for r in rows(ns)) + "\n]\n"


def load(path: str = OUT):
    return json.load(open(path))


if __name__ == "__main__":
    if not ref_extract.reference_available():
        sys.exit("the reference's Markdown is not on this machine: registry_vectors.json is written from its text only")
    open(OUT, "w").write(render())
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
