"""-m gpu: MORE THAN ONE pe_aggregate_signed inside one pipeline (a slot's aggregates fed in two or three parts).

The signature leg's device scratch is one set of buffers per pipeline arena (PipeArena::d_sig_in / d_sig_pts / d_sig_status),
and a streaming caller's legs are collected and launched later (engine_g1.cpp: sig_batch_flush): a second signed aggregate of
the same pipeline must be ordered behind the first one's leg, or the first call returns sums and statuses of the second
call's signatures.  Every other test makes one signed call per pipeline.

Expectations come from oracle/g2.py: row i of call c signs with (a_c + i * b_c) * G2 (built on the host with
g2.synthetic_points / g2.compress), every call has its own (a_c, b_c), so a group's aggregate is the closed form
(|S| a_c + b_c sum(S)) * G2 over the rows S of the call that pe_aggregate grouped together -- a sum formed from another call's
signatures cannot match.  Everything else a call returns (groups, rows and their flags, OR-ed bits, aggregate pubkeys,
counts) is held against the same call made synchronously on a twin engine.  Every group of every call is compared.

The parameter sets of test_repeated_signed_aggregates_equal_the_oracle cover every value of every axis -- pipeline (plain /
streaming), rows (host / device), signatures (one host buffer refilled between the calls / device memory read in place /
device memory at an address that is not a multiple of 16, copied by the leg), wire form per call, sizes (a smaller second
call; a call larger than every earlier one of the engine, whose scratch grows in the middle of the pipeline; three calls with
both), POSEVO_SIG_BATCH (1 / default) -- and every pair (pipeline x signatures) and (pipeline x wire form): these two pairs
pick the code path (collected or launched at once; which of the three buffers two calls share; whether the host copy is
there to race).  The full product (2 x 2 x 3 x 4 x 3 x 2 = 288) is left out: rows, sizes and the batch size change what the
path is handed, not which path runs, so each of their values appears with both pipelines but not with every signature /
wire combination.  A plain pipeline's second call over host signatures is a race against the first leg on the parent of this
file (no event between the copy and a ~1 ms decompression): those sets run five pipelines; the others, which are deterministic
once the handle's blocks have their size, run three (the first one grows them, see ROUNDS)."""
import functools

import numpy as np
import pytest

import bench
import pos_evolution_amd as pea
from oracle import g2
from pos_evolution_amd import RESIDENT, ROWS_RESIDENT, DeviceArena, _abi
from tests.test_gpu_g2 import R_ORDER, _off_curve_x, _off_subgroup_point
from tests.test_gpu_pairing import _args, _same_step, _same_store, _twin
from tests.test_gpu_pipeline import _world
from tests.test_gpu_resident_rows import _dev_arena, _dev_rows

pytestmark = pytest.mark.gpu

SPE, LAG = 32, 2
# A handle's first pipeline of a shape is not its steady state: the staging and output blocks grow call by call, and a block
# that grows completes what is enqueued -- which orders two calls by accident.  Every case therefore runs ROUNDS pipelines, each
# one checked in full: the first with the growths, the later ones with every arena sized and nothing but the engine's own
# ordering between the calls.  The cases that are a race on the parent of this file run RACE_ROUNDS.
ROUNDS, RACE_ROUNDS = 3, 5
WORLD = dict(n_val=8192, n_comm=128, seed=83, density=0.8, parts=6)    # 768 rows: 4 committees a slot, 6 rows a committee
# the epoch's rows by slot: [0, cut), [cut, next cut), ..., [last cut, 32)
SPLITS = {"smaller": (20,),       # 480 rows, then 288: a stale tail of the first call must not leak into the second
          "larger": (8,),         # 192 rows, then 576: the arena's scratch grows with the first call enqueued
          "three": (12, 18),      # 288, 144, 336: a smaller one, then one larger than both
          "even": (16,)}          # 384 and 384: every row index of one call exists in the other
SCALARS = [(0xABCDEF12345, 0x1357), (0x5151F00D77, 0x2F3B), (0x77AA55CC33, 0x0B0D)]   # (a_c, b_c) of call c
BAD = {5: "malformed", 9: "off_curve", 11: "off_subgroup", 40: "infinity"}
BAD_STATUS = {"malformed": 1, "off_curve": 2, "off_subgroup": 3, "infinity": 0}   # PE_SIG_* of include/posevo.h


def _parts(atts, split):
    cuts = (0,) + SPLITS[split] + (SPE,)
    slot = atts["slot"] % SPE
    return [np.ascontiguousarray(atts[(slot >= lo) & (slot < hi)]) for lo, hi in zip(cuts, cuts[1:])]


@functools.lru_cache(maxsize=None)
def _points(n, a, b):
    return g2.synthetic_points(n, a, b)


@functools.lru_cache(maxsize=None)
def _off_subgroup():
    return _off_subgroup_point()


def _wire(n, a, b, compressed, bad=None):
    """(n, 96 | 192) uint8: signature i = (a + i * b) * G2 in its wire form; bad = {row: kind} replaces some."""
    out = []
    for i, p in enumerate(_points(n, a, b)):
        kind = (bad or {}).get(i)
        if kind == "off_subgroup":
            p = _off_subgroup()
        elif kind == "infinity":
            p = None
        enc = bytearray(g2.compress(p) if compressed else g2.to_bytes192(p))
        if kind == "malformed":
            enc[0] &= 0x7F                       # the compression bit cleared
        elif kind == "off_curve":
            enc = bytearray(_off_curve_x())
        out.append(bytes(enc))
    return np.frombuffer(b"".join(out), dtype=np.uint8).reshape(n, -1).copy()


@functools.lru_cache(maxsize=None)
def _closed_forms(group_of_bytes, n_groups, a, b, left_out):
    """The compressed aggregate of every group: (|S| a + b sum(S)) * G2 over its member rows S without those left out."""
    gof = np.frombuffer(group_of_bytes, dtype=np.uint32)
    out = []
    for k in range(n_groups):
        good = [int(i) for i in np.nonzero(gof == k)[0] if int(i) not in left_out]
        out.append(g2.compress(g2.mul((a * len(good) + b * sum(good)) % R_ORDER, g2.G2) if good else None))
    return out


class _Feed:
    """Hands a call its signatures: 'host' -- ONE buffer, refilled for every call (pe_aggregate_signed reads host memory before
    it returns); 'dev16' -- a device buffer of the call's own at a 16-byte boundary (read in place by the leg); 'dev_odd' -- the
    same 8 bytes further on (the leg copies it into the arena's scratch first)."""

    def __init__(self, mode, max_bytes):
        self.mode, self.keep = mode, []
        self.host = np.empty(max_bytes, dtype=np.uint8) if mode == "host" else None

    def __call__(self, wire):
        flat = wire.reshape(-1)
        if self.mode == "host":
            view = self.host[:flat.size]
            view[:] = flat
            return view.reshape(wire.shape)
        import torch

        pad = 8 if self.mode == "dev_odd" else 0
        t = torch.zeros(flat.size + 16, dtype=torch.uint8, device="cuda")
        t[pad:pad + flat.size].copy_(torch.from_numpy(flat.copy()))
        torch.cuda.synchronize()
        self.keep.append(t)
        assert t.data_ptr() % 16 == 0
        return DeviceArena(t.data_ptr() + pad, flat.size, keep=t)

    def scribble(self):
        if self.host is not None:
            self.host[:] = 0xA5                  # the last call has returned: nothing may read the buffer any more


def _same_as_twin(got, want, n, tag):
    g = int(want["n_groups"])
    assert int(got["n_groups"]) == g, tag
    assert np.array_equal(np.asarray(got["group_of"])[:n], np.asarray(want["group_of"])[:n]), (tag, "group_of")
    for key in ("atts", "aggpk96", "count"):
        assert np.array_equal(np.asarray(got[key])[:g], np.asarray(want[key])[:g]), (tag, key)
    assert np.array_equal(got["out_arena"], want["out_arena"]), (tag, "out_arena")


def _check_signed(got, want, n, a, b, bad, tag):
    """One signed call: the twin's synchronous call for everything pe_aggregate returns, oracle/g2.py for the signatures."""
    _same_as_twin(got, want, n, tag)
    g = int(got["n_groups"])
    gof = np.ascontiguousarray(np.asarray(got["group_of"])[:n], dtype=np.uint32)
    assert g >= 2 and np.bincount(gof, minlength=g).max() > 1, (tag, "the grouping is degenerate")
    want_st = np.zeros(n, dtype=np.int32)
    for i, kind in (bad or {}).items():
        want_st[i] = BAD_STATUS[kind]
    assert np.array_equal(np.asarray(got["sig_status"])[:n], want_st), (tag, "sig_status")
    exp = _closed_forms(gof.tobytes(), g, a, b, frozenset(bad or ()))
    sig = np.asarray(got["sig96c"])
    for k in range(g):
        assert sig[k].tobytes() == exp[k], (tag, f"aggregate signature of group {k}")
    return gof, want_st


_twins = {}


def _twin_world(engine_factory):
    """The same world on a second engine, for synchronous host-row calls (aggregates do not change the store: one twin serves
    every test of the module that does not run the handlers)."""
    if "w" not in _twins:
        _twins["w"] = _world(engine_factory, **WORLD)
    return _twins["w"]


def _fresh_world(engine_factory, monkeypatch, batch=None):
    if batch is not None:
        monkeypatch.setenv("POSEVO_SIG_BATCH", str(batch))     # read once per handle, when it is created
    w = _world(engine_factory, **WORLD)
    if batch is not None:
        monkeypatch.delenv("POSEVO_SIG_BATCH")
    w["e"].set_pipeline_lag(LAG)
    return w


CASES = [
    # pipeline, rows,    signatures, wire,  sizes,     POSEVO_SIG_BATCH
    ("plain",  "host",   "host",    "cc",  "smaller", None),   # the host copy of call 2 against call 1's leg (a race: x 5)
    ("plain",  "device", "dev16",   "uu",  "larger",  None),
    ("plain",  "host",   "dev_odd", "cu",  "smaller", 1),
    ("plain",  "device", "host",    "uc",  "larger",  None),   # device rows: the guard of the row path came after the copy (x 5)
    ("plain",  "device", "dev_odd", "ccc", "three",   None),
    ("lagged", "host",   "host",    "cc",  "smaller", None),   # both legs collected: one launch over the same buffers
    ("lagged", "device", "host",    "ccc", "three",   None),   # ... with device rows, three calls, a growth in the middle
    ("lagged", "host",   "dev16",   "cc",  "smaller", None),   # read in place: the decoded points and statuses are still shared
    ("lagged", "host",   "dev16",   "cu",  "even",    None),   # the uncompressed call flushes the collected compressed one
    ("lagged", "device", "dev_odd", "uc",  "larger",  None),
    ("lagged", "host",   "dev_odd", "uu",  "smaller", 1),
    ("lagged", "device", "dev16",   "cc",  "larger",  1),      # a launch per call: the plain pipeline's race on the legs' stream
    ("lagged", "host",   "host",    "cuc", "three",   None),
]


@pytest.mark.parametrize("pipe,rows,sigs,wire,sizes,batch", CASES,
                         ids=["-".join(str(x) for x in c[:5]) + ("-batch%d" % c[5] if c[5] else "") for c in CASES])
def test_repeated_signed_aggregates_equal_the_oracle(engine_factory, monkeypatch, pipe, rows, sigs, wire, sizes, batch):
    w = _fresh_world(engine_factory, monkeypatch, batch)
    tw = _twin_world(engine_factory)
    e, arena = w["e"], w["arena"]
    parts = _parts(w["atts"], sizes)
    assert len(parts) == len(wire)
    wires = [_wire(len(p), *SCALARS[c], wire[c] == "c") for c, p in enumerate(parts)]
    want = [tw["e"].aggregate_signed(wires[c], packed=(p, tw["arena"]), compressed=wire[c] == "c", want_aggregate_pubkeys=True)
            for c, p in enumerate(parts)]
    packed = [(_dev_rows(p), _dev_arena(arena)) if rows == "device" else (p, arena) for p in parts]
    feed = _Feed(sigs, max(x.size for x in wires))
    grows = sizes in ("larger", "three")
    for rep in range(RACE_ROUNDS if pipe == "plain" and sigs == "host" else ROUNDS):
        got = []
        with e.pipeline(lagged=pipe == "lagged"):
            for c, p in enumerate(parts):
                growths = e.profile_arena_growths()
                got.append(e.aggregate_signed(feed(wires[c]), packed=packed[c], compressed=wire[c] == "c",
                                              want_aggregate_pubkeys=True))
                if grows and rep == 0 and c == len(parts) - 1:   # the case is the one it claims to be
                    assert e.profile_arena_growths() > growths, "the last call did not grow the arena's scratch"
            feed.scribble()
        e.drain()
        for c, p in enumerate(parts):
            _check_signed(got[c], want[c], len(p), *SCALARS[c], None, (rep, c))


@pytest.mark.parametrize("bad_call", [0, 1])
@pytest.mark.parametrize("rows", ["host", "device"])
@pytest.mark.parametrize("pipe", ["plain", "lagged"])
def test_statuses_and_the_valid_flag_stay_with_their_call(engine_factory, monkeypatch, pipe, rows, bad_call):
    """One call carries a malformed, an off-curve, an off-subgroup and an infinity signature at rows 5, 9, 11 and 40, the
    other call of the pipeline is all good at the same row indices (and the other way round): sig_status of each call is
    exactly its own, a group loses PE_ATT_FLAG_SIGNATURE_VALID through its own members only, and a bad member is left out of
    its own group's sum."""
    w = _fresh_world(engine_factory, monkeypatch)
    tw = _twin_world(engine_factory)
    e, arena = w["e"], w["arena"]
    parts = _parts(w["atts"], "even")
    bad = [BAD if c == bad_call else None for c in range(2)]
    wires = [_wire(len(p), *SCALARS[c], True, bad[c]) for c, p in enumerate(parts)]
    plain = [tw["e"].aggregate(packed=(p, tw["arena"]), want_aggregate_pubkeys=True) for p in parts]
    want = [tw["e"].aggregate_signed(wires[c], packed=(p, tw["arena"]), check_subgroup=True, want_aggregate_pubkeys=True)
            for c, p in enumerate(parts)]
    packed = [(_dev_rows(p), _dev_arena(arena)) if rows == "device" else (p, arena) for p in parts]
    feed = _Feed("host", max(x.size for x in wires))
    for rep in range(ROUNDS):
        got = []
        with e.pipeline(lagged=pipe == "lagged"):
            for c in range(2):
                got.append(e.aggregate_signed(feed(wires[c]), packed=packed[c], check_subgroup=True,
                                              want_aggregate_pubkeys=True))
            feed.scribble()
        e.drain()
        for c, p in enumerate(parts):
            gof, st = _check_signed(got[c], want[c], len(p), *SCALARS[c], bad[c], (rep, c))
            lost = 0
            for k in range(int(got[c]["n_groups"])):
                valid = bool(got[c]["atts"][k]["flags"] & _abi.PE_ATT_FLAG_SIGNATURE_VALID)
                was_valid = bool(plain[c]["atts"][k]["flags"] & _abi.PE_ATT_FLAG_SIGNATURE_VALID)
                own = not st[gof == k].any()
                assert valid == (was_valid and own), (rep, c, f"group {k}: signature-valid flag")
                lost += was_valid and not valid
            assert (lost >= 1) if c == bad_call else (lost == 0), (rep, c, "groups that lost their signature-valid flag", lost)


@pytest.mark.parametrize("rows", ["host", "device"])
@pytest.mark.parametrize("pipe", ["plain", "lagged"])
def test_signed_unsigned_signed_in_one_pipeline(engine_factory, monkeypatch, pipe, rows):
    """aggregate_signed, aggregate, aggregate_signed over the three parts of an epoch inside one pipeline: the unsigned call in
    the middle (which, over device rows, launches what the first leg still holds) returns what the twin's does, and both
    signed calls return the oracle's sums."""
    w = _fresh_world(engine_factory, monkeypatch)
    tw = _twin_world(engine_factory)
    e, arena = w["e"], w["arena"]
    parts = _parts(w["atts"], "three")
    wires = [_wire(len(p), *SCALARS[c], True) for c, p in enumerate(parts)]
    want = [tw["e"].aggregate(packed=(p, tw["arena"]), want_aggregate_pubkeys=True) if c == 1 else
            tw["e"].aggregate_signed(wires[c], packed=(p, tw["arena"]), want_aggregate_pubkeys=True) for c, p in enumerate(parts)]
    packed = [(_dev_rows(p), _dev_arena(arena)) if rows == "device" else (p, arena) for p in parts]
    feed = _Feed("host", max(x.size for x in wires))
    for rep in range(ROUNDS):
        got = []
        with e.pipeline(lagged=pipe == "lagged"):
            for c in range(3):
                if c == 1:
                    got.append(e.aggregate(packed=packed[c], want_aggregate_pubkeys=True))
                else:
                    got.append(e.aggregate_signed(feed(wires[c]), packed=packed[c], want_aggregate_pubkeys=True))
            feed.scribble()
        e.drain()
        for c, p in enumerate(parts):
            if c == 1:
                _same_as_twin(got[c], want[c], len(p), (rep, c))
                assert int(got[c]["n_groups"]) >= 2
            else:
                _check_signed(got[c], want[c], len(p), *SCALARS[c], None, (rep, c))


@pytest.mark.parametrize("where", ["host", "device"])
def test_two_signed_steps_in_every_streaming_pipeline(where):
    """aggregate_signed -> on_attestation_batch -> get_head_async -> process_attestation_batch TWICE per streaming pipeline (the
    two halves of an epoch), five pipelines at lag 3 with signatures that change from call to call: legs of several arenas are
    in flight and collected at once.  Head, statuses, numerators, aggregate signatures and the store equal the twin's
    synchronous host-row calls; the aggregate signatures equal the oracle's closed form as well."""
    n, lag = 5, 3
    e = pea.Engine(max_committee_tables=n + 3)
    w = bench.build_workload(e, _args(32768, 128, 300, n), 0, n)
    spe = w["spe"]
    halves = []
    for st in w["steps"]:
        first = st["atts"]["slot"] % spe < spe // 2
        halves.append([np.ascontiguousarray(st["atts"][m]) for m in (first, ~first)])
    n_max = max(len(h) for hs in halves for h in hs)
    a, b = SCALARS[0]
    base = np.frombuffer(b"".join(g2.compress(p) for p in _points(n_max + 2 * n, a, b)), dtype=np.uint8).reshape(-1, 96)
    # call j of pipeline k signs its row i with (a + (i + 2 k + j) b) G2
    wires = [[np.ascontiguousarray(base[2 * k + j:2 * k + j + len(h)]) for j, h in enumerate(hs)] for k, hs in enumerate(halves)]
    feed = _Feed("host" if where == "host" else "dev16", 96 * n_max)
    e.set_pipeline_lag(lag)
    e.reuse_outputs(n + lag + 2)
    got, keep = [], []
    for k, st in enumerate(w["steps"]):
        e.on_tick((st["epoch"] + 1) * spe * 12)
        e.participation_rotate()
        cap = st["comm"].offsets.size - 1
        rows_in = [_dev_rows(h) for h in halves[k]]
        keep.append(rows_in)
        with e.pipeline(lagged=True):
            for j in range(2):
                agg = e.aggregate_signed(feed(wires[k][j]), packed=(rows_in[j], st["arena_in"]), want_aggregate_pubkeys=True)
                status, _, count = e.on_attestation_batch(packed=(ROWS_RESIDENT, RESIDENT), cap=cap)
                head = e.get_head_async()
                pst, num = e.process_attestation_batch(st["ctx"], packed=(ROWS_RESIDENT, RESIDENT), cap=cap)
                got.append(dict(agg=agg, status=status, count=count, head=head, pstatus=pst, numerators=num))
            feed.scribble()
    e.drain()
    e2 = _twin(w, n)
    for k, st in enumerate(w["steps"]):
        e2.on_tick((st["epoch"] + 1) * spe * 12)
        e2.participation_rotate()
        for j, half in enumerate(halves[k]):
            agg = e2.aggregate_signed(wires[k][j], packed=(half, st["arena"]), want_aggregate_pubkeys=True)
            rows = agg["atts"]
            status, _, count = e2.on_attestation_batch(packed=(rows, agg["out_arena"]))
            head = e2.get_head()
            pst, num = e2.process_attestation_batch(st["ctx"], packed=(rows, agg["out_arena"]))
            want = dict(agg=agg, status=status, count=count, head=head, pstatus=pst, numerators=num)
            g_ = got[2 * k + j]
            _same_step(g_, want, (k, j))
            g = int(want["agg"]["n_groups"])
            gof = np.ascontiguousarray(np.asarray(g_["agg"]["group_of"])[:len(half)], dtype=np.uint32)
            assert g >= 2 and np.bincount(gof, minlength=g).max() > 1, (k, j)
            assert np.array_equal(np.asarray(g_["agg"]["sig96c"])[:g], np.asarray(agg["sig96c"])[:g]), (k, j, "signatures")
            assert not np.asarray(g_["agg"]["sig_status"])[:len(half)].any() and not agg["sig_status"].any(), (k, j)
            exp = _closed_forms(gof.tobytes(), g, a + (2 * k + j) * b, b, frozenset())
            for q in range(g):
                assert np.asarray(g_["agg"]["sig96c"])[q].tobytes() == exp[q], (k, j, f"aggregate signature of group {q}")
    _same_store(e, e2)
    e.close()
    e2.close()
