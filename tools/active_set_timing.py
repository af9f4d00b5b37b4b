#!/usr/bin/env python
"""Wall time of pe_active_set at 1 M and 4 M validators next to the route it replaces, in one process on one GPU:

    active_set              pe_active_set(epoch), count and total balance only (three launches, one 16-byte read-back, one wait)
    active_set_with_list    ... plus the copy of the list to the host
    numpy_flatnonzero       the host's get_active_validator_indices: flatnonzero over the two epoch arrays, as uint32
    committees_host_list    pe_compute_committees over that host list (validated, copied, uploaded, shuffled)
    committees_resident     pe_compute_committees over PE_ACTIVE_RESIDENT (shuffled where the list lies)

Every figure is a host clock around a synchronous call (each ends in a stream synchronise); five rounds alternate the five
variants, the median of the rounds' medians is reported with every round's median beside it.  99.5 % of the registry is
active, 64 committees per slot, 90 rounds.  Writes one JSON object to the path given (default: standard output only).

    python tools/active_set_timing.py [out.json]
"""
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pos_evolution_amd as pea  # noqa: E402

ETH = 10**9
FAR = np.uint64(2**64 - 1)
EPOCH = 1000
VARIANTS = ("active_set", "active_set_with_list", "numpy_flatnonzero", "committees_host_list", "committees_resident")


def median_ms(call, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return round(ts[len(ts) // 2], 4), round(ts[0], 4)


def measure(n):
    rng = np.random.default_rng(n)
    e = pea.Engine(device=0)
    e.set_validators(np.full(n, 32 * ETH, dtype=np.uint64), np.ones(n, dtype=np.uint8))
    mask = rng.random(n) < 0.995
    activation = np.zeros(n, dtype=np.uint64)
    activation[~mask] = FAR
    exit_ = np.full(n, FAR, dtype=np.uint64)
    e.registry_set_epochs(activation, exit_)
    epoch = np.uint64(EPOCH)
    seed = hashlib.sha256(b"active-set-timing").digest()
    n_committees = 64 * 32

    def host_list():
        return np.flatnonzero((activation <= epoch) & (epoch < exit_)).astype(np.uint32)

    calls = {}
    for _ in range(3):   # warm-up of every shape: code objects, staging blocks, tables
        n_active, _, idx = e.active_set(EPOCH, want_indices=True)
        calls = {
            "active_set": lambda: e.active_set(EPOCH),
            "active_set_with_list": lambda: e.active_set(EPOCH, want_indices=True),
            "numpy_flatnonzero": host_list,
            "committees_host_list": lambda: e.compute_committees(7, seed, idx, n_committees, 90, want_result=False),
            "committees_resident": lambda: e.compute_committees(8, seed, pea.ACTIVE_RESIDENT, n_committees, 90, want_result=False),
        }
        for name in VARIANTS:
            calls[name]()
    assert np.array_equal(host_list(), idx)
    for a, b in zip(e.committees(7), e.committees(8)):
        assert np.array_equal(a, b)
    rounds = {name: [] for name in VARIANTS}
    for _ in range(5):
        for name in VARIANTS:
            rounds[name].append(median_ms(calls[name], 40 if name == "active_set" else 20))
    out = {"n_active": int(n_active)}
    for name, rs in rounds.items():
        meds = [m for m, _ in rs]
        out[name] = {"ms": sorted(meds)[len(meds) // 2], "round_medians_ms": meds, "min_ms": min(lo for _, lo in rs)}
    e.close()
    return out


if __name__ == "__main__":
    result = {str(n): measure(n) for n in (1 << 20, 1 << 22)}
    text = json.dumps(result, indent=1)
    print(text)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(text + "\n")
