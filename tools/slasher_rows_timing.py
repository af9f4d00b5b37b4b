#!/usr/bin/env python
"""Wall time of the synchronous pe_slasher_ingest at the configs[3] shape (1 048 576 validators, 2048 committees of 512, 8192
rows in four partial aggregates per committee -> 2048 groups, H = 64, D = 4096) over its two routes, in one process on one GPU:

    device_rows   rows handed over as DeviceRows -> pe_aggregate -> pe_slasher_ingest(PE_ROWS_RESIDENT, PE_BITS_RESIDENT)
    host_rows     pe_aggregate over host rows   -> pe_slasher_ingest(out_atts, PE_BITS_RESIDENT)

Each route has a handle of its own (a handle that changes route rebuilds the other side's data tables: not what is timed).  The
aggregate runs once; the figure is a host clock around the ingest alone, the median of 20 calls after 5 warm-ups.  From the
second call on every group's data is known and every vote meets its own record: the steady state of both routes, the scan's
work the same on both.  The first call (every data new, every record written) is reported beside it.  Writes one JSON object
with the device's name and clock to the path given (default: standard output only).

    python tools/slasher_rows_timing.py [out.json]
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pos_evolution_amd as pea  # noqa: E402
from pos_evolution_amd import synth  # noqa: E402

N_VAL, N_COMM, SPE, PARTS, H, D, EPOCH = 1 << 20, 2048, 32, 4, 64, 4096, 1


def handle(comm):
    e = pea.Engine(device=0, slots_per_epoch=SPE)
    e.store_init(0, 0, bytes([7]) * 32)
    e.set_validators(np.full(N_VAL, 32 * 10**9, dtype=np.uint64), np.ones(N_VAL, dtype=np.uint8))
    e.set_committees(EPOCH, comm.offsets, comm.members)
    e.on_tick((EPOCH * SPE + SPE - 1) * int(e.cfg.seconds_per_slot))
    e.slasher_enable(H, D)
    return e


def timed(call, reps=20, warm=5):
    t0 = time.perf_counter()
    call()
    first = (time.perf_counter() - t0) * 1e3
    for _ in range(warm - 1):
        call()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4), "first_call_ms": round(first, 4)}


def main():
    import torch

    comm = synth.random_committees(N_VAL, N_COMM, 40)
    tree = synth.random_tree(8, 1, "branchy")
    tree.slot[:] = np.minimum(tree.slot, EPOCH * SPE)
    atts, arena, _ = synth.epoch_attestations(comm, tree, EPOCH, SPE, seed=5, density=0.9, parts=PARTS, source=(0, None))
    try:   # the current shader clock, where the runtime's management library is at hand
        clock = int(torch.cuda.clock_rate(0))
    except Exception:
        clock = None
    out = {"device": torch.cuda.get_device_name(0), "shader_clock_mhz": clock, "rows": int(len(atts))}
    dev, host = handle(comm), handle(comm)
    t = torch.from_numpy(np.ascontiguousarray(atts).view(np.uint8).reshape(-1).copy()).cuda()
    agg = dev.aggregate(packed=(pea.DeviceRows(t.data_ptr(), len(atts), keep=t), arena))
    rows = np.ascontiguousarray(host.aggregate(packed=(atts, arena))["atts"])
    out["groups"] = int(agg["n_groups"])
    assert out["groups"] == len(rows) == N_COMM
    out["device_rows"] = timed(lambda: dev.slasher_ingest(packed=(pea.ROWS_RESIDENT, pea.RESIDENT), cap_rows=len(atts), current_epoch=EPOCH))
    out["host_rows"] = timed(lambda: host.slasher_ingest(packed=(rows, pea.RESIDENT), current_epoch=EPOCH))
    a, b = dev.slasher_records(EPOCH), host.slasher_records(EPOCH)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])   # the two handles hold the same records
    dev.close()
    host.close()
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(text + "\n")


if __name__ == "__main__":
    main()
