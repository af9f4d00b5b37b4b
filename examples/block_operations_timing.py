#!/usr/bin/env python
"""Times pe_process_block_operations on one GPU at V validators (default 1 048 576) for a block of 2 attester slashings
(2048 indices on either side, all of them in the intersection) and 16 voluntary exits, as the host wall clock around the
synchronous call.  In the same session, alternating with it, the route the call replaces: pe_registry_get_epochs,
pe_state_get_balances and pe_state_get_validators (download), the sequential loop of tests/block_ops_model.py on the host
restricted to the rows the block touches (and the rows that hold the exit queue's end), then pe_registry_set_epochs,
pe_state_set_balances and pe_state_set_validators (upload).  Medians after a warm-up; every timed call starts from the same
registry, restored untimed; both routes' arrays are compared before anything is printed.

    python examples/block_operations_timing.py [--validators V] [--calls N] [--host-calls M] [--out PATH]

The host loop costs seconds per call at this block size (initiate_validator_exit walks the rows once per exit), so it is timed
M times (default 5) and reported apart from the transfers around it, which are timed with it every time."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pos_evolution_amd as pea  # noqa: E402
from tests import block_ops_model as B  # noqa: E402
from tests import registry_updates_model as M  # noqa: E402

CUR = 1000


def block(n: int, per_list: int, n_exits: int, seed: int = 5):
    rng = np.random.default_rng(seed)
    pick = rng.choice(n, size=2 * per_list + n_exits + 1, replace=False)
    ops = []
    for t in range(2):
        idx = sorted(int(x) for x in pick[t * per_list:(t + 1) * per_list])
        ops.append(B.attester_slashing(*B.double_vote(CUR - 1, t), idx, idx))
    ops += [B.voluntary_exit(int(v), CUR) for v in pick[2 * per_list:2 * per_list + n_exits]]
    return ops, int(pick[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--validators", type=int, default=1 << 20)
    ap.add_argument("--per-list", type=int, default=2048)
    ap.add_argument("--exits", type=int, default=16)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    n = args.validators
    p = B.BlockParams()
    a = M.blank_registry(n, p)
    a["bal"] += np.arange(n, dtype=np.uint64) % np.uint64(1000)
    ops, proposer = block(n, args.per_list, args.exits)
    flags = M.view_flags(a, CUR)
    params = {k: getattr(p, k) for k, _ in pea._abi.pe_block_ops_params._fields_}
    e = pea.Engine(device=0)
    e.set_validators(a["eff"], (flags & 3).astype(np.uint8))

    def restore():
        e.state_set_validators(a["eff"], flags)
        e.registry_set_epochs(a["act"], a["ext"])
        e.state_set_balances(a["bal"], None, a["wdr"])

    def read():
        act, ext, _ = e.registry_get_epochs()
        bal, _, wdr, _ = e.state_get_balances()
        return [act.copy(), ext.copy(), wdr.copy(), bal.copy(), e.state_validators()[1].copy()]

    touched = sorted({v for op in ops for v in (op.get("i1", []) + [op.get("index", proposer)])} | {proposer})

    def host_route(run_loop: bool):
        t0 = time.perf_counter()
        act, ext, _ = e.registry_get_epochs()
        bal, _, wdr, _ = e.state_get_balances()
        eff, fl, _ = e.state_validators()
        t1 = time.perf_counter()
        out = None
        if run_loop:
            c = np.uint64(CUR)
            limit, _ = M.churn_limits(int(((act <= c) & (c < ext)).sum()), p)
            queue_end = np.flatnonzero((ext != np.uint64(M.FAR)) & (ext >= np.uint64(CUR + 1 + p.max_seed_lookahead)))
            rows = np.union1d(np.array(touched, dtype=np.int64), queue_end)
            local = {int(v): i for i, v in enumerate(rows)}
            sub = dict(elig=a["elig"][rows], act=act[rows], ext=ext[rows], wdr=wdr[rows], eff=eff[rows], slashed=(fl[rows] >> 1) & 1,
                       bal=bal[rows])
            sub_ops = [dict(op, i1=[local[v] for v in op["i1"]], i2=[local[v] for v in op["i2"]]) if op["kind"] == B.ATTESTER_SLASHING
                       else dict(op, index=local[op["index"]]) for op in ops]
            q = B.BlockParams(min_per_epoch_churn_limit=limit, churn_limit_quotient=1 << 62)
            res, status, st = B.block_operations_sequential(sub, CUR, local[proposer], sub_ops, q)
            assert not any(status)
            ext, wdr, bal, fl = ext.copy(), wdr.copy(), bal.copy(), fl.copy()
            ext[rows], wdr[rows], bal[rows] = res["ext"], res["wdr"], res["bal"]
            fl[rows] = B.view_slashed_flags(fl[rows], res["slashed"])
            out = st
        t2 = time.perf_counter()
        e.registry_set_epochs(act, ext)
        e.state_set_balances(bal, None, wdr)
        e.state_set_validators(eff, fl)
        t3 = time.perf_counter()
        return (t1 - t0) + (t3 - t2), t2 - t1, out

    device_ms, transfer_ms, loop_ms = [], [], []
    stats, arrays = {}, {}
    for i in range(args.warmup + max(20, args.calls)):
        restore()
        t0 = time.perf_counter()
        status, stats["device"] = e.process_block_operations(CUR, proposer, ops, params)
        dt = time.perf_counter() - t0
        assert not status.any()
        if i == 0:
            arrays["device"] = read()
        restore()
        run_loop = i < args.host_calls
        transfers, loop, st = host_route(run_loop)
        if run_loop:
            stats["host"], arrays["host"] = st, read()
        if i >= args.warmup:
            device_ms.append(dt * 1e3)
            transfer_ms.append(transfers * 1e3)
        if run_loop:
            loop_ms.append(loop * 1e3)
    for k in ("n_slashed", "n_exits_initiated", "first_exit_epoch", "last_exit_epoch", "slashed_balance", "proposer_rewards",
              "penalties", "n_saturated"):
        assert stats["device"][k] == stats["host"][k], k
    assert all(np.array_equal(x, y) for x, y in zip(arrays["device"], arrays["host"])), "the two routes' arrays differ"
    st = stats["device"]
    lines = [f"validators {n}  operations {len(ops)}  indices {4 * args.per_list}  slashed {st['n_slashed']}  "
             f"exits initiated {st['n_exits_initiated']}  exit epochs {st['first_exit_epoch']}..{st['last_exit_epoch']}",
             "host wall clock around synchronous calls, both routes alternating in one session; medians after "
             f"{args.warmup} warm-up rounds",
             f"  pe_process_block_operations                      median of {len(device_ms)}: {np.median(device_ms):9.3f} ms   "
             f"min {min(device_ms):9.3f} ms",
             f"  three _get calls + three _set calls (no host work) median of {len(transfer_ms)}: {np.median(transfer_ms):9.3f} ms   "
             f"min {min(transfer_ms):9.3f} ms",
             f"  the model's loop over the {len(touched)} touched rows      median of {len(loop_ms)}: {np.median(loop_ms):9.3f} ms   "
             f"min {min(loop_ms):9.3f} ms",
             f"  the route the call replaces (transfers + loop)   {np.median(transfer_ms) + np.median(loop_ms):9.3f} ms"]
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    e.close()


if __name__ == "__main__":
    main()
