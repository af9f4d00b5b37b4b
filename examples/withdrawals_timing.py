#!/usr/bin/env python
"""Times pe_process_withdrawals on one GPU at V validators (default 1 048 576) for the mainnet sweep (16 384 positions, 16
withdrawals) and for a whole-registry sweep (V positions, the shape the kernels are sized for), as the host wall clock around
the synchronous call with PE_WD_APPLY and a matching payload.  In the same session, alternating with it, the route the call
replaces: download the credentials, withdrawable epochs, effective balances and balances, a numpy sweep on the host (the closed
form of tests/withdrawals_model.py over the swept range), upload the balances.  The engine has no getter for a range of a
column, so that route moves WHOLE columns at either sweep size (pe_registry_get_static with the credentials alone,
pe_state_get_balances without the scores, pe_state_get_validators, pe_state_set_balances).  Medians after a warm-up; every
timed call starts from the same registry, restored untimed; both routes' withdrawals and balances are compared before anything
is printed.

    python examples/withdrawals_timing.py [--validators V] [--calls N] [--out PATH]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pos_evolution_amd as pea  # noqa: E402
from pos_evolution_amd.engine import WITHDRAWAL_DTYPE  # noqa: E402

EPOCH, MAXEB = 1000, 32 * 10**9


def registry(n: int, seed: int = 7):
    """one validator in 200 partially withdrawable, one in 1000 fully; the rest keep BLS credentials"""
    rng = np.random.default_rng(seed)
    cred = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    cred[:, 0] = 0
    r = rng.integers(0, 1000, size=n)
    cred[r < 6, 0] = 1
    wdr = np.full(n, 2**64 - 1, dtype=np.uint64)
    wdr[r == 0] = EPOCH - 3
    bal = np.full(n, MAXEB, dtype=np.uint64) + rng.integers(0, 10**8, size=n).astype(np.uint64)
    return cred, wdr, np.full(n, MAXEB, dtype=np.uint64), bal


def host_sweep(cred, wdr, eff, bal, n, start, sweep, k, next_index):
    bound = min(n, sweep)
    v = (start + np.arange(bound, dtype=np.int64)) % n
    prefix = cred[v, 0] == 1
    b = bal[v]
    full = prefix & (wdr[v] <= np.uint64(EPOCH)) & (b > 0)
    hit = full | (prefix & (eff[v] == np.uint64(MAXEB)) & (b > np.uint64(MAXEB)))
    take = np.flatnonzero(hit)[:k]
    out = np.zeros(take.size, dtype=WITHDRAWAL_DTYPE)
    out["index"] = next_index + np.arange(take.size)
    out["validator_index"] = v[take]
    out["address"] = cred[v[take], 12:]
    out["amount"] = np.where(full[take], b[take], b[take] - np.uint64(MAXEB))
    bal[v[take]] -= out["amount"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--validators", type=int, default=1 << 20)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    n = args.validators
    cred, wdr, eff, bal = registry(n)
    e = pea.Engine(device=0)
    flags = np.full(n, 9, dtype=np.uint8)
    e.set_validators(eff, (flags & 1).astype(np.uint8))
    e.state_set_validators(eff, flags)
    e.registry_set_epochs(np.zeros(n, dtype=np.uint64), np.full(n, 2**64 - 1, dtype=np.uint64))
    e.registry_set_static(np.zeros((n, 48), dtype=np.uint8), cred, np.zeros(n, dtype=np.uint64))
    lib, h = e._lib, e._h
    start, next_index = n - 5000, 12345
    lines = [f"validators {n}  start {start}  epoch {EPOCH}",
             "host wall clock around synchronous calls, both routes alternating in one session; medians after "
             f"{args.warmup} warm-up rounds of {args.calls} timed"]
    for name, sweep in (("mainnet sweep", 16384), ("whole-registry sweep", n)):
        params = dict(max_validators_per_sweep=sweep)
        device_ms, dry_ms, transfer_ms, numpy_ms = [], [], [], []
        for i in range(args.warmup + args.calls):
            e.state_set_balances(bal, None, wdr)
            t0 = time.perf_counter()
            expected, dry = e.process_withdrawals(EPOCH, next_index, start, None, False, params)
            t1 = time.perf_counter()
            _, res = e.process_withdrawals(EPOCH, next_index, start, expected, True, params)
            t2 = time.perf_counter()
            assert res["applied"] == 1 and res["n_withdrawals"] == 16
            device_bal = e.state_get_balances()[0].copy()
            e.state_set_balances(bal, None, wdr)
            g_cred, g_bal, g_wdr = np.zeros((n, 32), dtype=np.uint8), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
            is_set = C.c_int(0)
            t3 = time.perf_counter()
            assert lib.pe_registry_get_static(h, n, None, g_cred.ctypes.data, None, C.addressof(is_set)) == 0
            assert lib.pe_state_get_balances(h, n, g_bal.ctypes.data, None, g_wdr.ctypes.data, C.addressof(is_set)) == 0
            g_eff, _, _ = e.state_validators()
            t4 = time.perf_counter()
            host = host_sweep(g_cred, g_wdr, g_eff, g_bal, n, start, sweep, 16, next_index)
            t5 = time.perf_counter()
            e.state_set_balances(g_bal, None, g_wdr)
            t6 = time.perf_counter()
            assert host.tobytes() == expected.tobytes() and np.array_equal(g_bal, device_bal), "the two routes differ"
            if i >= args.warmup:
                dry_ms.append((t1 - t0) * 1e3)
                device_ms.append((t2 - t1) * 1e3)
                transfer_ms.append((t4 - t3 + t6 - t5) * 1e3)
                numpy_ms.append((t5 - t4) * 1e3)
        med = lambda x: float(np.median(x))  # noqa: E731
        lines += [f"{name}: {min(n, sweep)} positions, 16 withdrawals ({res['n_full']} full, {res['n_partial']} partial), "
                  f"next validator index {res['next_withdrawal_validator_index']}",
                  f"  pe_process_withdrawals, compute only                 median {med(dry_ms):8.3f} ms   min {min(dry_ms):8.3f} ms",
                  f"  pe_process_withdrawals, payload + PE_WD_APPLY        median {med(device_ms):8.3f} ms   min {min(device_ms):8.3f} ms",
                  f"  three _get calls + pe_state_set_balances (columns)   median {med(transfer_ms):8.3f} ms   min {min(transfer_ms):8.3f} ms",
                  f"  the numpy sweep over the range                       median {med(numpy_ms):8.3f} ms   min {min(numpy_ms):8.3f} ms",
                  f"  the route the call replaces (transfers + sweep)      {med(transfer_ms) + med(numpy_ms):8.3f} ms"]
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    e.close()


if __name__ == "__main__":
    main()
