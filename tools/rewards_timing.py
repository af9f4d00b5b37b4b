#!/usr/bin/env python
"""Wall time of the epoch boundary's balance step at 1 M and 4 M validators, next to the route a caller had before the
balances were resident, in one process on one GPU:

    resident     pe_rewards_and_penalties (both functions), then pe_effective_balance_updates(PE_BALANCES_RESIDENT):
                 nothing per validator crosses the bus
    host_route   pe_participation_get of both arrays, the numpy model of the two functions on the host
                 (tests/rewards_model.run_numpy), then pe_effective_balance_updates from the host vector (8 B per
                 validator staged and uploaded)

Every figure is a host clock around synchronous calls (each ends in a stream synchronise): the median of 20 after 5
warm-ups, with the minimum beside it.  The state is put back before every repetition (outside the clock), so each one
does the same work.  Prints the device and its clock as the runtime reports it while idle, then one JSON object; writes it
to the path given.

    python tools/rewards_timing.py [out.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pos_evolution_amd as pea  # noqa: E402
from tests import rewards_model as M  # noqa: E402

CURRENT, FINALIZED = 12, 10
WARMUP, REPS = 5, 20


def box():
    import torch
    name = torch.cuda.get_device_name(0)
    try:
        clock = f"{torch.cuda.clock_rate(0)} MHz"
    except Exception as err:  # the query needs the management library
        clock = f"unavailable ({type(err).__name__})"
    return {"device": name, "idle_clock": clock}


def timed(setup, call):
    ts = []
    for i in range(WARMUP + REPS):
        setup()
        t0 = time.perf_counter()
        call()
        dt = (time.perf_counter() - t0) * 1e3
        if i >= WARMUP:
            ts.append(dt)
    ts.sort()
    return {"ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4)}


def measure(n):
    a = M.random_registry(n, n, CURRENT)
    e = pea.Engine(device=0)
    e.set_validators(a["eff"], (a["sflags"] & 3).astype(np.uint8))
    e.participation_set(1, a["participation"])

    def setup():
        e.state_set_validators(a["eff"], a["sflags"])
        e.state_set_balances(a["balances"], a["scores"], a["withdrawable"])

    def resident():
        e.rewards_and_penalties(CURRENT, FINALIZED)
        e.effective_balance_updates(pea.BALANCES_RESIDENT, want_result=False)

    state = {}

    def host_route():
        e.participation_get(0)
        part = e.participation_get(1)
        bal, sc, _ = M.run_numpy(a["eff"], a["sflags"], part, a["withdrawable"], a["balances"], a["scores"], CURRENT, FINALIZED)
        e.effective_balance_updates(bal, want_result=False)
        state["bal"], state["sc"] = bal, sc

    out = {"resident": timed(setup, resident)}
    got_bal, got_sc, _, _ = e.state_get_balances()
    got_eff = e.state_validators()[0]
    out["host_route"] = timed(setup, host_route)
    assert np.array_equal(got_bal, state["bal"]) and np.array_equal(got_sc, state["sc"])
    assert np.array_equal(got_eff, e.state_validators()[0])
    e.close()
    return out


if __name__ == "__main__":
    result = {"box": box(), "current_epoch": CURRENT, "finalized_epoch": FINALIZED, "warmup": WARMUP, "reps": REPS}
    print(json.dumps(result["box"]))
    for n in (1 << 20, 1 << 22):
        result[str(n)] = measure(n)
    text = json.dumps(result, indent=1)
    print(text)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(text + "\n")
