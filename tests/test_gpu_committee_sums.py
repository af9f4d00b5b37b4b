"""-m gpu: aggregate pubkeys by complement -- committee sums built with every committee table, and groups in
which a majority attests summed as S_c minus the absentees.

Keys are s_v * G with known scalars: every expected output is (sum of the attesting members' scalars) * G, the closed form of
tests/committee_sums_model.py over oracle/g1.py, compared byte for byte.  Every case goes through pe_compute_committees and a
pe_aggregate over rows in device memory inside a streaming pipeline; which route ran is read from pe_profile_committee_sums.
All cases run once more in ONE fresh child process with POSEVO_COMMITTEE_SUMS=0 (the direct route throughout): identical bytes.

A device-row aggregate forms no ungated group (those exist for pe_g1_sum only), so the mixed step mixes complement and direct
groups over both candidate tables."""
import functools
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import pos_evolution_amd as pea
import pos_evolution_amd.synth as synth
from oracle import g1
from tests import committee_sums_model as M
from tests import helpers as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF96 = bytes([0x40]) + bytes(95)
PROG_A, PROG_B = 0x1234567, 0x89ABCDE


@functools.lru_cache(maxsize=None)
def _tree():
    return synth.random_tree(8, 2, "chain")


def _epoch(spe):
    return int(_tree().slot.max()) // spe + 1


def _seed(tag):
    return hashlib.sha256(b"committee sums " + tag.encode()).digest()


def _dev(arr):
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).cuda()


@functools.lru_cache(maxsize=None)
def _prog_points(n):
    return H.oracle_points(n, PROG_A, PROG_B)[0]


def _prog_scalars(n):
    return [(PROG_A + v * PROG_B) % g1.R_ORDER for v in range(n)]


def _points_of(scalars):
    return np.frombuffer(b"".join(g1.to_bytes96(g1.mul(int(s) % g1.R_ORDER, g1.G)) for s in scalars),
                         dtype=np.uint8).reshape(len(scalars), 96).copy()


def _engine(make, n_val, pts, spe, tables=4):
    e = make(slots_per_epoch=spe, max_committee_tables=tables)
    H.load_tree(e, _tree())
    e.set_validators(synth.balances(n_val, 2), np.ones(n_val, dtype=np.uint8), pts)
    e.on_tick((_epoch(spe) + 1) * spe * 12)
    return e


def _committees(e, epoch, tag, n_val, n_comm):
    off, mem = e.compute_committees(epoch, _seed(tag), n_val, n_comm, 10)
    return synth.Committees(np.asarray(off, dtype=np.uint32), np.asarray(mem, dtype=np.uint32))


def _members(comm, c):
    return comm.members[comm.offsets[c]:comm.offsets[c + 1]]


def _aggregate(e, comm_of_row, epoch_of_row, committees, bit_rows, spe):
    """One streaming pipeline with one pe_aggregate over device rows -> (aggpk96 of the groups formed, route counters)."""
    parts = []
    for ep in sorted(set(epoch_of_row)):
        sel = [i for i, x in enumerate(epoch_of_row) if x == ep]
        parts.append((sel, H.committee_attestations(comm_of_row[sel[0]], _tree(), ep, [committees[i] for i in sel],
                                                    [bit_rows[i] for i in sel], spe)))
    atts = np.zeros(len(committees), dtype=synth.ATT_DTYPE)
    arena, base = [], 0
    for sel, (a, ar) in parts:
        a = a.copy()
        a["bits_offset"] += base
        atts[sel] = a
        arena.append(ar)
        base += ar.size
    arena = np.concatenate(arena)
    t_rows, t_bits = _dev(atts), _dev(arena)
    rows = pea.DeviceRows(t_rows.data_ptr(), len(atts), keep=t_rows)
    bits = pea.DeviceArena(t_bits.data_ptr(), t_bits.numel(), keep=t_bits)
    with e.pipeline(lagged=True):
        agg = e.aggregate(packed=(rows, bits), want_aggregate_pubkeys=True)
    e.drain()
    return np.array(agg["aggpk96"][:agg["n_groups"]]), e.profile_committee_sums()


def _expect(scalars, comm, c, union):
    mem = _members(comm, c)
    return M.expected96([scalars[int(v)] for v in mem], union)


def _one_table(make, tag, n_val, n_comm, spe, bits_of, scalars=None, parts=1):
    """Committees of one table, one group each (split into `parts` disjoint rows); bits_of(c, size) -> the union's bits."""
    pts = _prog_points(n_val) if scalars is None else _points_of(scalars)
    scalars = _prog_scalars(n_val) if scalars is None else scalars
    e = _engine(make, n_val, pts, spe)
    ep = _epoch(spe)
    comm = _committees(e, ep, tag, n_val, n_comm)
    unions = [np.asarray(bits_of(c, int(comm.offsets[c + 1] - comm.offsets[c])), dtype=bool) for c in range(n_comm)]
    rng = np.random.Generator(np.random.PCG64(len(tag)))
    part_of = [rng.integers(0, parts, size=u.size) for u in unions]
    rows = [u & (p == q) for q in range(parts) for u, p in zip(unions, part_of)]
    pk, route = _aggregate(e, [comm] * len(rows), [ep] * len(rows), list(range(n_comm)) * parts, rows, spe)
    want = [_expect(scalars, comm, c, unions[c]) for c in range(n_comm)]
    n_cmpl = sum(M.by_complement(u.size, int(u.sum())) for u in unions)
    return dict(pk=pk, want=want, route=route, n_cmpl=n_cmpl, tables=1)


def _first(n_set):
    return lambda c, size: [i < n_set(c, size) for i in range(size)]


# ---------------------------------------------------------------- the cases (each runs here and, knob off, in the child)
def case_threshold_even(make):  # n = 8: 4 bits direct, 5 bits by complement, all, all but one
    return _one_table(make, "thr8", 32, 4, 4, _first(lambda c, n: (4, 5, n, n - 1)[c]))


def case_threshold_odd(make):   # n = 9: 4 direct, 5 by complement, one bit, no bit (infinity)
    return _one_table(make, "thr9", 36, 4, 4, _first(lambda c, n: (4, 5, 1, 0)[c]))


def case_single_member(make):   # committees of one member: bit set (by complement, N at infinity) and not set
    return _one_table(make, "one", 4, 4, 4, lambda c, n: [c % 2 == 0])


def case_within_k(make):        # committees of 3 <= k members: the accumulation's own hand-over writes the absentees' sum
    return _one_table(make, "k3", 12, 4, 4, lambda c, n: ([1, 1, 1], [1, 1, 0], [0, 1, 0], [0, 1, 1])[c])


def case_one_block(make):       # 16 members = 4 lanes of k = 4: exactly one padded block
    return _one_table(make, "blk", 64, 4, 4, lambda c, n: [(i * 7 + c) % 16 >= (0, 1, 3, 9)[c] for i in range(n)], parts=4)


def case_wide(make):            # 1025 members: more than 256 lanes of k = 4; 3 absentees, and a direct twin
    return _one_table(make, "wide", 2050, 2, 2, lambda c, n: [(i % 400 != 1) if c == 0 else (i % 2 == 1) for i in range(n)], parts=4)


def _group_law(make, name):
    """The committee of tests/committee_sums_model.GROUP_LAW[name] as committee 0 of a real shuffle: the shuffle is taken
    first, the scalars are dealt to its members, the keys are loaded (which drops the sums) and the table is built again."""
    scal_c, bits_c = M.GROUP_LAW[name]
    size, spe, n_comm = len(scal_c), 2, 2
    n_val = size * n_comm
    e = _engine(make, n_val, _prog_points(n_val), spe)
    ep = _epoch(spe)
    comm = _committees(e, ep, "law" + name, n_val, n_comm)
    scalars = [0] * n_val
    for j, v in enumerate(_members(comm, 0)):
        scalars[int(v)] = scal_c[j]
    for j, v in enumerate(_members(comm, 1)):
        scalars[int(v)] = 77 + 1000 * j
    e.set_validators(synth.balances(n_val, 2), np.ones(n_val, dtype=np.uint8), _points_of(scalars))
    dropped = e.profile_committee_sums()[0]
    comm2 = _committees(e, ep, "law" + name, n_val, n_comm)
    assert np.array_equal(comm2.members, comm.members)
    unions = [np.asarray(bits_c, dtype=bool), np.ones(size, dtype=bool)]
    pk, route = _aggregate(e, [comm] * 2, [ep] * 2, [0, 1], unions, spe)
    want = [_expect(scalars, comm, c, unions[c]) for c in range(2)]
    return dict(pk=pk, want=want, route=route, n_cmpl=2, tables=1, dropped=dropped)


def case_law_cancels(make):
    return _group_law(make, "cancels")


def case_law_doubling(make):
    return _group_law(make, "doubling")


def case_law_all(make):
    return _group_law(make, "all")


def case_law_same_x(make):
    return _group_law(make, "same_x")


def case_mixed_two_tables(make):
    """Current- and previous-epoch tables in one aggregate, 4 disjoint partial rows per committee, densities on both sides of
    the threshold."""
    n_val, n_comm, spe = 2048, 8, 4
    e = _engine(make, n_val, _prog_points(n_val), spe)   # the clock stands in epoch E + 1: tables E (previous), E + 1 (current)
    scalars = _prog_scalars(n_val)
    eps = [_epoch(spe), _epoch(spe) + 1]
    comms = [_committees(e, ep, "mix%d" % ep, n_val, n_comm) for ep in eps]
    rng = np.random.Generator(np.random.PCG64(99))
    dens = [0.99, 0.3, 1.0, 0.6, 0.45, 0.99, 0.0, 0.9]
    rows, comm_of, ep_of, committees, unions = [], [], [], [], []
    for t in (1, 0):
        for c in range(n_comm):
            size = int(comms[t].offsets[c + 1] - comms[t].offsets[c])
            u = rng.random(size) < dens[(c + 3 * t) % 8]
            unions.append((t, c, u))
    part = [rng.integers(0, 4, size=u.size) for _, _, u in unions]
    for q in range(4):
        for (t, c, u), p in zip(unions, part):
            rows.append(u & (p == q))
            comm_of.append(comms[t])
            ep_of.append(eps[t])
            committees.append(c)
    order = range(len(unions))   # groups come out in order of first appearance: the first of the four parts names them all
    pk, route = _aggregate(e, comm_of, ep_of, committees, rows, spe)
    want = [_expect(scalars, comms[unions[i][0]], unions[i][1], unions[i][2]) for i in order]
    n_cmpl = sum(M.by_complement(u.size, int(u.sum())) for _, _, u in unions)
    return dict(pk=pk, want=want, route=route, n_cmpl=n_cmpl, tables=2)


def case_invalidation(make):
    """pe_set_validators with other keys under an existing table: the sums are dropped and the next aggregate is the closed
    form over the NEW keys by the direct route; a fresh pe_compute_committees brings the complement route back."""
    n_val, n_comm, spe = 256, 4, 4
    e = _engine(make, n_val, _prog_points(n_val), spe)
    ep = _epoch(spe)
    comm = _committees(e, ep, "inval", n_val, n_comm)
    unions = [np.arange(int(comm.offsets[c + 1] - comm.offsets[c])) % 11 != c for c in range(n_comm)]
    args = ([comm] * n_comm, [ep] * n_comm, list(range(n_comm)), unions, spe)
    pk0, route0 = _aggregate(e, *args)
    new_pts, (a2, b2) = H.oracle_points(n_val, 0x777, 0x31337)
    new_scalars = [(a2 + v * b2) % g1.R_ORDER for v in range(n_val)]
    e.set_validators(synth.balances(n_val, 2), np.ones(n_val, dtype=np.uint8), new_pts)
    pk1, route1 = _aggregate(e, *args)
    comm2 = _committees(e, ep, "inval", n_val, n_comm)
    assert np.array_equal(comm2.members, comm.members)
    pk2, route2 = _aggregate(e, *args)
    old = [_expect(_prog_scalars(n_val), comm, c, unions[c]) for c in range(n_comm)]
    new = [_expect(new_scalars, comm, c, unions[c]) for c in range(n_comm)]
    return dict(pk=np.concatenate([pk0, pk1, pk2]), want=old + new + new, route=route2, n_cmpl=n_comm, tables=1,
                routes=[route0, route1, route2])


def case_lru(make):
    """More pe_compute_committees_async calls than table slots inside lagged steps: each step's table is shuffled during the
    step before it, into the slot of the least recently used table.  Whether an aggregate finds its table's shuffle still in
    flight (direct) or done (the deferred build, then by complement) is a matter of timing: the bytes are held, not the route."""
    n_val, n_comm, spe, steps, slots = 512, 4, 4, 6, 3
    twin = _engine(make, n_val, None, spe, tables=steps + 2)
    e = _engine(make, n_val, _prog_points(n_val), spe, tables=slots)
    scalars = _prog_scalars(n_val)
    ep0 = _epoch(spe)
    comms = [_committees(twin, ep0 + s, "lru%d" % s, n_val, n_comm) for s in range(steps)]
    first = _committees(e, ep0, "lru0", n_val, n_comm)
    assert np.array_equal(first.members, comms[0].members)
    pks, want, keep = [], [], []
    for s in range(steps):
        e.on_tick((ep0 + s + 1) * spe * 12)
        unions = [np.arange(int(comms[s].offsets[c + 1] - comms[s].offsets[c])) % (5 + s) != c for c in range(n_comm)]
        atts, arena = H.committee_attestations(comms[s], _tree(), ep0 + s, list(range(n_comm)), unions, spe)
        t_rows, t_bits = _dev(atts), _dev(arena)
        keep.append((t_rows, t_bits))
        with e.pipeline(lagged=True):
            agg = e.aggregate(packed=(pea.DeviceRows(t_rows.data_ptr(), n_comm, keep=t_rows),
                                      pea.DeviceArena(t_bits.data_ptr(), t_bits.numel(), keep=t_bits)),
                              want_aggregate_pubkeys=True)
            if s + 1 < steps:
                e.compute_committees_async(ep0 + s + 1, _seed("lru%d" % (s + 1)), n_val, n_comm, 10)
        pks.append(agg)
        want += [_expect(scalars, comms[s], c, unions[c]) for c in range(n_comm)]
    e.drain()
    pk = np.concatenate([np.array(a["aggpk96"][:a["n_groups"]]) for a in pks])
    return dict(pk=pk, want=want, route=e.profile_committee_sums(), n_cmpl=None, tables=None)


def case_async_table_builds_at_first_aggregate(make):
    """pe_compute_committees_async enqueues no sums; the first aggregate that finds the table complete and no shuffle in flight
    builds them and already goes by complement."""
    n_val, n_comm, spe = 256, 4, 4
    twin = _engine(make, n_val, None, spe)
    e = _engine(make, n_val, _prog_points(n_val), spe)
    ep = _epoch(spe)
    comm = _committees(twin, ep, "lazy", n_val, n_comm)
    e.compute_committees_async(ep, _seed("lazy"), n_val, n_comm, 10)
    before = e.profile_committee_sums()[0]
    off, mem = e.committees(ep)                      # a synchronous read of the table: the shuffle has ended
    assert np.array_equal(mem, comm.members)
    unions = [np.arange(int(comm.offsets[c + 1] - comm.offsets[c])) % 9 != c for c in range(n_comm)]
    pk, route = _aggregate(e, [comm] * n_comm, [ep] * n_comm, list(range(n_comm)), unions, spe)
    want = [_expect(_prog_scalars(n_val), comm, c, unions[c]) for c in range(n_comm)]
    return dict(pk=pk, want=want, route=route, n_cmpl=n_comm, tables=1, before=before)


def case_dist_custom_handle(make):
    """A handle after pe_dist_init_custom builds no sums and keeps the direct route."""
    n_val, n_comm, spe = 128, 4, 4
    e = _engine(make, n_val, _prog_points(n_val), spe)
    e.dist_init_custom(0, 1, lambda *a: 0, lambda *a: 0)
    ep = _epoch(spe)
    comm = _committees(e, ep, "dist", n_val, n_comm)
    unions = [np.ones(int(comm.offsets[c + 1] - comm.offsets[c]), dtype=bool) for c in range(n_comm)]
    pk, route = _aggregate(e, [comm] * n_comm, [ep] * n_comm, list(range(n_comm)), unions, spe)
    want = [_expect(_prog_scalars(n_val), comm, c, unions[c]) for c in range(n_comm)]
    return dict(pk=pk, want=want, route=route, n_cmpl=0, tables=0)


CASES = {k[5:]: v for k, v in sorted(globals().items()) if k.startswith("case_")}
_results = {}


def _result(name, engine_factory):
    if name not in _results:
        _results[name] = CASES[name](engine_factory)
    return _results[name]


@functools.lru_cache(maxsize=None)
def _knob_off_outputs():
    """Every case once more, in one fresh child process with POSEVO_COMMITTEE_SUMS=0 -> {case: aggpk96 bytes}."""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "off.npz")
        env = dict(os.environ, POSEVO_COMMITTEE_SUMS="0")
        out = subprocess.run([sys.executable, "-m", "tests.test_gpu_committee_sums", path], cwd=ROOT, env=env,
                             capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-3000:] + "\n" + out.stderr[-3000:]
        with np.load(path) as z:
            return {k: z[k].copy() for k in z.files}


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_is_the_closed_form_by_the_expected_route(engine_factory, name):
    r = _result(name, engine_factory)
    assert r["pk"].shape == (len(r["want"]), 96)
    bad = [g for g, w in enumerate(r["want"]) if r["pk"][g].tobytes() != w]
    assert not bad, (name, "groups whose aggregate pubkey is not the closed form", bad[:8])
    tables, n_cmpl = r["route"]
    if r["tables"] is not None:
        assert tables == r["tables"], (name, "committee tables with valid sums")
        assert n_cmpl == r["n_cmpl"], (name, "groups of the last aggregate that went by complement")


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_gives_the_same_bytes_with_the_knob_off(engine_factory, name):
    r = _result(name, engine_factory)
    off = _knob_off_outputs()
    assert np.array_equal(off[name], r["pk"])
    assert int(off[name + ".n_cmpl"]) == 0 and int(off[name + ".tables"]) == 0


def test_named_outputs(engine_factory):
    """The outputs the cases are named after: infinity where everything cancels or nobody attests, the routes of the
    invalidation in order."""
    assert _result("law_cancels", engine_factory)["pk"][0].tobytes() == INF96
    assert _result("threshold_odd", engine_factory)["pk"][3].tobytes() == INF96
    assert _result("law_cancels", engine_factory)["dropped"] == 0     # pe_set_validators dropped the sums
    assert _result("async_table_builds_at_first_aggregate", engine_factory)["before"] == 0
    inval = _result("invalidation", engine_factory)["routes"]
    assert [r[0] for r in inval] == [1, 0, 1] and inval[1][1] == 0 and inval[0][1] == inval[2][1] == 4


def test_a_table_that_is_no_partition_builds_no_sums(engine_factory):
    """pe_set_committees with a validator in two committees: no sums, the host-row aggregate is the closed form as before; a
    partition set the same way builds them."""
    n_val, spe = 64, 4
    e = _engine(engine_factory, n_val, _prog_points(n_val), spe)
    ep = _epoch(spe)
    offsets = np.array([0, 16, 32, 48, 64], dtype=np.uint32)
    members = np.arange(64, dtype=np.uint32)
    e.set_committees(ep, offsets, members)
    assert e.profile_committee_sums()[0] == 1
    members[16] = 0                                    # validator 0 sits in committees 0 and 1
    comm = synth.Committees(offsets, members)
    e.set_committees(ep, offsets, members)
    assert e.profile_committee_sums()[0] == 0
    unions = [np.ones(16, dtype=bool) for _ in range(4)]
    atts, arena = H.committee_attestations(comm, _tree(), ep, [0, 1, 2, 3], unions, spe)
    agg = e.aggregate(packed=(atts, arena), want_aggregate_pubkeys=True)
    scalars = _prog_scalars(n_val)
    assert [x.tobytes() for x in agg["aggpk96"][:4]] == [_expect(scalars, comm, c, unions[c]) for c in range(4)]


if __name__ == "__main__":
    import torch

    torch.cuda.init()
    made = []

    def make(**cfg):
        made.append(pea.Engine(**cfg))
        return made[-1]

    out = {}
    for name, fn in CASES.items():
        r = fn(make)
        assert [x.tobytes() for x in r["pk"]] == r["want"], name
        out[name] = r["pk"]
        out[name + ".n_cmpl"] = np.array(r["route"][1])
        out[name + ".tables"] = np.array(r["route"][0])
    np.savez(sys.argv[1], **out)
    for e in made:
        e.close()
