#!/usr/bin/env python
"""Times pe_registry_updates and pe_process_slashings on one GPU at V validators (default 1 048 576) for a realistic epoch
-- a few ejections, an activation queue of a few thousand -- as the host wall clock around the synchronous calls, the median
of at least 20 after a warm-up.  In the same run, the route a caller had before these calls existed, for the same epoch:
download the activation, exit and withdrawable epochs and the balances (32 B per validator; the eligibility epochs, pubkeys
and credentials are the caller's own host copies), run the numpy model of tests/registry_updates_model.py on the host, then
pe_registry_set_epochs + pe_state_set_balances + pe_registry_set_static (112 B per validator and the pubkeys' hashing).
Both routes' arrays are compared before anything is printed.

    python examples/registry_updates_timing.py [--validators V] [--calls N] [--json PATH]

Every timed call starts from the same registry: it is restored (untimed) between calls."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pos_evolution_amd as pea  # noqa: E402
from tests import registry_updates_model as M  # noqa: E402

CUR, FIN, VECTOR = 1000, 998, 8192


def realistic_registry(n: int, seed: int = 8):
    """Everybody active with a full balance, except: 12 validators at the ejection balance, 3000 waiting in the activation
    queue (eligibility epochs over the last 200 epochs), 500 not yet marked, 40 slashed ones at the penalty's epoch."""
    rng = np.random.default_rng(seed)
    p = M.Params(max_per_epoch_activation_churn_limit=8)
    a = M.blank_registry(n, p)
    pick = rng.choice(n, size=min(n, 12 + 3000 + 500 + 40), replace=False)
    eject, queue, fresh, slashed = np.split(pick, [12, 3012, 3512])
    a["eff"][eject] = p.ejection_balance
    a["act"][queue] = M.FAR
    a["elig"][queue] = rng.integers(FIN - 200, FIN + 1, size=queue.size, dtype=np.uint64)
    a["act"][fresh] = M.FAR
    a["elig"][fresh] = M.FAR
    a["slashed"][slashed] = 1
    a["ext"][slashed] = CUR - 10
    a["wdr"][slashed] = CUR + VECTOR // 2
    return a, p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--validators", type=int, default=1 << 20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None, help="write the figures to this file")
    args = ap.parse_args()
    n, calls = args.validators, max(20, args.calls)
    a, p = realistic_registry(n)
    rng = np.random.default_rng(9)
    pk = rng.integers(0, 256, size=(n, 48), dtype=np.uint8)
    wc = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    flags = M.view_flags(a, CUR)
    e = pea.Engine(device=0)
    e.set_validators(a["eff"], (flags & 3).astype(np.uint8))
    e.state_set_validators(a["eff"], flags)
    e.registry_set_static(pk, wc, a["elig"])

    def restore():
        e.registry_set_epochs(a["act"], a["ext"])
        e.state_set_balances(a["bal"], None, a["wdr"])
        e.registry_set_static(pk, wc, a["elig"])

    def device_route():
        st = e.registry_updates(CUR, FIN, p.abi())
        return st, e.process_slashings(CUR, 10**15, 3, VECTOR)

    def host_route():
        act, ext, _ = e.registry_get_epochs()
        bal, _, wdr, _ = e.state_get_balances()
        b = dict(elig=a["elig"], act=act, ext=ext, wdr=wdr, eff=a["eff"], slashed=a["slashed"], bal=bal)
        out, st = M.registry_updates_numpy(b, CUR, FIN, p)
        out["bal"], sst = M.slashings_numpy(out, flags, CUR, 10**15, 3, VECTOR)
        e.registry_set_epochs(out["act"], out["ext"])
        e.state_set_balances(out["bal"], None, out["wdr"])
        e.registry_set_static(pk, wc, out["elig"])
        return st, sst

    def read():
        act, ext, _ = e.registry_get_epochs()
        bal, _, wdr, _ = e.state_get_balances()
        return [e.registry_static()[2], act, ext, wdr, bal]

    results, arrays, stats = {}, {}, {}
    for name, route in (("device", device_route), ("host", host_route)):
        times = []
        for i in range(args.warmup + calls):
            restore()
            t0 = time.perf_counter()
            stats[name] = route()
            dt = time.perf_counter() - t0
            if i >= args.warmup:
                times.append(dt)
        arrays[name] = read()
        results[name] = dict(median_ms=float(np.median(times)) * 1e3, min_ms=min(times) * 1e3, calls=calls)
    assert stats["device"] == stats["host"], (stats["device"], stats["host"])
    assert all(np.array_equal(x, y) for x, y in zip(arrays["device"], arrays["host"])), "the two routes' arrays differ"
    st, sst = stats["device"]
    print(f"validators {n}  ejected {st['n_ejected']}  queue {st['queue_len']}  activated {st['n_activated']}  "
          f"marked {st['n_marked_eligible']}  penalised {sst['n_penalised']}")
    for name, label in (("device", "pe_registry_updates + pe_process_slashings"),
                        ("host", "download, numpy model, three re-uploads")):
        r = results[name]
        print(f"  {label:45s} median of {calls}: {r['median_ms']:9.3f} ms   min {r['min_ms']:9.3f} ms")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(validators=n, method="host wall clock around the synchronous calls, median after warm-up",
                           warmup=args.warmup, registry_stats=st, slashings_stats=sst, **results), f, indent=1)
            f.write("\n")
    e.close()


if __name__ == "__main__":
    main()
