"""-m gpu: the sparse route of the aggregate pubkeys by complement -- a complement group with at most
G1_SPARSE_MAX absentees is summed by k_g1_absentees (one wave: bit scan, compacted index list, complete adds) while the
accumulation and the tree leave it alone.

Keys are s_v * G with known scalars, so every expected output is the closed form of tests/committee_sums_model.py over
oracle/g1.py, compared byte for byte (tolerance 0).  Every case runs once more in ONE fresh child process with
POSEVO_G1_SPARSE=0 (the dense complement route, the parent's launches): identical aggregate pubkeys, OR-ed bits, counts and
the same number of complement verdicts (pe_profile_committee_sums counts the `cmpl` words that are set; the words themselves
have no reader on the host besides that count).

Shapes: committees of 3, 31, 32, 33, 63, 64, 65, 96 and 512 members (tail-word mask, one and several bit words, fewer members
than lanes); 0, 1, 2 (one word / two words) absentees, absentees at member 0 and member n - 1, exactly G1_SPARSE_MAX (more than 64: lanes
with two list entries) and one more (dense complement), the largest count that still goes by complement; with the threshold
raised to G1_SPARSE_CAP, up to 255 absentees in one wave (lanes with four entries).  Registries with duplicate keys, a key and its negation, and (i + 1) G."""
import functools
import os
import re
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
from tests import test_gpu_committee_sums as CS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HDR = open(os.path.join(ROOT, "pos_evolution_amd", "csrc", "kernels.h")).read()
SPARSE_MAX = int(re.search(r"G1_SPARSE_MAX = (\d+);", _HDR).group(1))
SPARSE_CAP = int(re.search(r"G1_SPARSE_CAP = (\d+);", _HDR).group(1))
SIZES = (3, 31, 32, 33, 63, 64, 65, 96, 512)
KNOB = "POSEVO_G1_SPARSE"


def _aggregate(e, comm_of_row, epoch_of_row, committees, bit_rows, spe):
    """CS._aggregate, with the unions' bits and counts beside the pubkeys."""
    parts = []
    for ep in sorted(set(epoch_of_row)):
        sel = [i for i, x in enumerate(epoch_of_row) if x == ep]
        parts.append((sel, H.committee_attestations(comm_of_row[sel[0]], CS._tree(), ep, [committees[i] for i in sel],
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
    t_rows, t_bits = CS._dev(atts), CS._dev(arena)
    with e.pipeline(lagged=True):
        agg = e.aggregate(packed=(pea.DeviceRows(t_rows.data_ptr(), len(atts), keep=t_rows),
                                  pea.DeviceArena(t_bits.data_ptr(), t_bits.numel(), keep=t_bits)),
                          want_aggregate_pubkeys=True)
    e.drain()
    return _outputs(agg), e.profile_committee_sums()


def _outputs(agg):
    g = agg["n_groups"]
    bits = np.concatenate([np.packbits(b, bitorder="little") for b in agg["bits"]]) if g else np.zeros(0, np.uint8)
    return dict(pk=np.array(agg["aggpk96"][:g]), bits=bits, count=np.array(agg["count"][:g]))


def _absent(n, idx):
    u = np.ones(n, dtype=bool)
    u[list(idx)] = False
    return u


def _spread(n, a, salt):
    """a absentees of n members at seeded positions."""
    return np.random.Generator(np.random.PCG64(1000 * n + 7 * a + salt)).permutation(n)[:a]


def _patterns(n, limit):
    """Eight unions of an n-member committee around the threshold `limit`; every one goes by complement (a < n / 2)."""
    amax = (n - 1) // 2
    pats = [[], [0], [n - 1], [0, 1], [0, n - 1],
            list(range(1, 2 * amax, 2)),                 # the largest count that still goes by complement
            _spread(n, min(limit, amax), 1),             # exactly the threshold (where the committee allows it)
            _spread(n, min(limit + 1, amax), 2)]         # one more: the dense complement route
    return [_absent(n, [i for i in p][:amax]) for p in pats]


def _table(make, tag, size, unions_of, scalars=None, n_comm=8, spe=4):
    n_val = size * n_comm
    pts = CS._prog_points(n_val) if scalars is None else CS._points_of(scalars)
    scalars = CS._prog_scalars(n_val) if scalars is None else scalars
    e = CS._engine(make, n_val, pts, spe)
    ep = CS._epoch(spe)
    comm = CS._committees(e, ep, tag, n_val, n_comm)
    assert all(int(comm.offsets[c + 1] - comm.offsets[c]) == size for c in range(n_comm))
    unions = unions_of(size)
    assert len(unions) == n_comm
    out, route = _aggregate(e, [comm] * n_comm, [ep] * n_comm, list(range(n_comm)), unions, spe)
    want = [CS._expect(scalars, comm, c, unions[c]) for c in range(n_comm)]
    return dict(out, want=want, route=route, unions=unions, n_cmpl=sum(M.by_complement(u.size, int(u.sum())) for u in unions))


def _dealt(make, tag, committees):
    """Committees given as (scalars, bits) lists of one size, dealt to the members of a real shuffle (CS._group_law)."""
    size, n_comm, spe = len(committees[0][0]), len(committees), 4
    n_val = size * n_comm
    e = CS._engine(make, n_val, CS._prog_points(n_val), spe)
    ep = CS._epoch(spe)
    comm = CS._committees(e, ep, tag, n_val, n_comm)
    scalars = [0] * n_val
    for c, (scal_c, _) in enumerate(committees):
        for j, v in enumerate(CS._members(comm, c)):
            scalars[int(v)] = scal_c[j]
    e.set_validators(synth.balances(n_val, 2), np.ones(n_val, dtype=np.uint8), CS._points_of(scalars))
    comm2 = CS._committees(e, ep, tag, n_val, n_comm)
    assert np.array_equal(comm2.members, comm.members)
    unions = [np.asarray(b, dtype=bool) for _, b in committees]
    out, route = _aggregate(e, [comm] * n_comm, [ep] * n_comm, list(range(n_comm)), unions, spe)
    want = [CS._expect(scalars, comm, c, unions[c]) for c in range(n_comm)]
    return dict(out, want=want, route=route, unions=unions, n_cmpl=sum(M.by_complement(u.size, int(u.sum())) for u in unions))


# ---------------------------------------------------------------- the cases (each runs here and, knob off, in the child)
def _size_case(size):
    def case(make):
        return _table(make, "sparse%d" % size, size, lambda n: _patterns(n, SPARSE_MAX))
    return case


for _s in SIZES:
    globals()["case_size_%03d" % _s] = _size_case(_s)


def case_raised_threshold(make):
    """POSEVO_G1_SPARSE = G1_SPARSE_CAP: every count a 512-member committee can send by complement goes to the wave -- lanes
    with two, three and four list entries (the affine + affine add, then the general one)."""
    counts = (65, SPARSE_MAX - 1, SPARSE_MAX + 1, 192, 193, 254, 255, 2)
    old = os.environ.get(KNOB)
    if old != "0":                       # (the child's knob-off run keeps its 0)
        os.environ[KNOB] = str(SPARSE_CAP)
    try:
        return _table(make, "raised", 512, lambda n: [_absent(n, _spread(n, a, 3)) for a in counts])
    finally:
        if old is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = old


def case_structured_keys(make):
    """synth's structured keys (i + 1) G: neighbours' sums meet third keys (same x) all the time."""
    size, n_comm = 16, 8
    pats = ([], [0], [0, 1], [0, 1, 2], [1, 2, 3, 15], [0, 15], [3, 4, 5, 6, 7, 8, 9], [15])
    return _table(make, "structured", size, lambda n: [_absent(n, p) for p in pats],
                  scalars=[v + 1 for v in range(size * n_comm)])


P_, Q_, C_ = M.P_, M.Q_, M.C_
R = g1.R_ORDER


def case_special_registries(make):
    """Committees of 9: duplicate keys among the absentees (P + P: a doubling inside the wave's tree, at its last and at an
    earlier level), a key and its negation both absent (the absentees' sum at infinity), with a third absentee, and P + P + (-2P)."""
    rest = [1000 + 37 * j for j in range(9)]

    def comm(head, n_absent):
        return (list(head) + rest[len(head):], [0] * n_absent + [1] * (9 - n_absent))
    return _dealt(make, "special", [
        comm([P_, P_], 2),                          # lanes 0 and 1 hold the same point
        comm([P_, Q_, P_, Q_], 4),                  # level 2: P + P and Q + Q, level 1: 2P + 2Q
        comm([P_, R - P_], 2),                      # P + (-P): infinity out of the wave
        comm([P_, R - P_, Q_], 3),                  # ... and a third absentee beside the pair
        comm([P_, P_, (R - 2 * P_) % R], 3),        # 2P meets -2P one level up
        comm([P_, Q_, (P_ + Q_) % R], 3),           # P + Q meets P + Q: a doubling of a sum
        comm([C_, C_, C_, C_], 4),                  # four times the same key
        comm([], 0)])                               # nobody absent


def case_mixed_aggregate(make):
    """Sparse, dense-complement and direct groups over BOTH candidate tables in one call, four disjoint partial rows per
    committee; the first and the last group of the plan are sparse."""
    n_val, n_comm, spe = 4096, 8, 4                      # committees of 512
    e = CS._engine(make, n_val, CS._prog_points(n_val), spe)
    scalars = CS._prog_scalars(n_val)
    eps = [CS._epoch(spe), CS._epoch(spe) + 1]
    comms = [CS._committees(e, ep, "smix%d" % ep, n_val, n_comm) for ep in eps]
    absent = {1: (2, 100, 300, 0, SPARSE_MAX, SPARSE_MAX + 1, 255, 1), 0: (5, 400, SPARSE_MAX, 200, 30, 256, 512, 3)}
    rng = np.random.Generator(np.random.PCG64(17))
    unions = []
    for t in (1, 0):
        for c in range(n_comm):
            size = int(comms[t].offsets[c + 1] - comms[t].offsets[c])
            unions.append((t, c, _absent(size, _spread(size, absent[t][c], t))))
    part = [rng.integers(0, 4, size=u.size) for _, _, u in unions]
    rows, comm_of, ep_of, committees = [], [], [], []
    for q in range(4):
        for (t, c, u), p in zip(unions, part):
            rows.append(u & (p == q))
            comm_of.append(comms[t])
            ep_of.append(eps[t])
            committees.append(c)
    out, route = _aggregate(e, comm_of, ep_of, committees, rows, spe)
    want = [CS._expect(scalars, comms[t], c, u) for t, c, u in unions]
    return dict(out, want=want, route=route, unions=[u for _, _, u in unions],
                n_cmpl=sum(M.by_complement(u.size, int(u.sum())) for _, _, u in unions))


def case_streaming(make):
    """Five streaming steps at lag 2, every group sparse, each step's unions its own; outputs per step (the synchronous
    replay is test_streaming_steps_match_the_synchronous_replay)."""
    n_val, n_comm, spe, steps = 8 * 96, 8, 4, 5
    e = CS._engine(make, n_val, CS._prog_points(n_val), spe)
    e.set_pipeline_lag(2)
    scalars = CS._prog_scalars(n_val)
    ep = CS._epoch(spe)
    comm = CS._committees(e, ep, "sstream", n_val, n_comm)
    aggs, want, keep, unions_all = [], [], [], []
    for s in range(steps):
        unions = [_absent(96, _spread(96, (s + c) % 6, s)) for c in range(n_comm)]
        atts, arena = H.committee_attestations(comm, CS._tree(), ep, list(range(n_comm)), unions, spe)
        t_rows, t_bits = CS._dev(atts), CS._dev(arena)
        keep.append((t_rows, t_bits))
        with e.pipeline(lagged=True):
            aggs.append(e.aggregate(packed=(pea.DeviceRows(t_rows.data_ptr(), n_comm, keep=t_rows),
                                            pea.DeviceArena(t_bits.data_ptr(), t_bits.numel(), keep=t_bits)),
                                    want_aggregate_pubkeys=True))
        want += [CS._expect(scalars, comm, c, unions[c]) for c in range(n_comm)]
        unions_all += unions
    e.drain()
    outs = [_outputs(a) for a in aggs]
    out = {k: np.concatenate([o[k] for o in outs]) for k in ("pk", "bits", "count")}
    return dict(out, want=want, route=e.profile_committee_sums(), unions=unions_all, n_cmpl=n_comm, comm=comm, ep=ep)


CASES = {k[5:]: v for k, v in sorted(globals().items()) if k.startswith("case_")}
_results = {}


def _result(name, engine_factory):
    if name not in _results:
        _results[name] = CASES[name](engine_factory)
    return _results[name]


@functools.lru_cache(maxsize=None)
def _knob_off_outputs():
    """Every case once more, in one fresh child process with POSEVO_G1_SPARSE=0."""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "off.npz")
        env = dict(os.environ)
        env[KNOB] = "0"
        out = subprocess.run([sys.executable, "-m", "tests.test_gpu_g1_sparse", path], cwd=ROOT, env=env,
                             capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-3000:] + "\n" + out.stderr[-3000:]
        with np.load(path) as z:
            return {k: z[k].copy() for k in z.files}


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_is_the_closed_form(engine_factory, name):
    r = _result(name, engine_factory)
    assert r["pk"].shape == (len(r["want"]), 96)
    bad = [g for g, w in enumerate(r["want"]) if r["pk"][g].tobytes() != w]
    assert not bad, (name, "groups whose aggregate pubkey is not the closed form", bad[:8])
    assert r["route"][1] == r["n_cmpl"], (name, "groups of the last aggregate with a complement verdict")
    assert np.array_equal(r["count"], [int(u.sum()) for u in r["unions"]])
    assert np.array_equal(r["bits"], np.concatenate([np.packbits(u, bitorder="little") for u in r["unions"]]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_gives_the_same_outputs_by_the_dense_route(engine_factory, name):
    r = _result(name, engine_factory)
    off = _knob_off_outputs()
    assert np.array_equal(off[name + ".pk"], r["pk"])
    assert np.array_equal(off[name + ".bits"], r["bits"])
    assert np.array_equal(off[name + ".count"], r["count"])
    assert int(off[name + ".n_cmpl"]) == r["route"][1]


def test_the_cases_straddle_the_threshold():
    """What the shapes above are for: the patterns of a 512-member committee hold exactly G1_SPARSE_MAX absentees and one
    more, the small committees their largest complement count; infinity comes out where the special registries say so."""
    counts = [512 - int(u.sum()) for u in _patterns(512, SPARSE_MAX)]
    assert counts == [0, 1, 1, 2, 2, 255, SPARSE_MAX, SPARSE_MAX + 1]
    assert [3 - int(u.sum()) for u in _patterns(3, SPARSE_MAX)] == [0, 1, 1, 1, 1, 1, 1, 1]
    assert [65 - int(u.sum()) for u in _patterns(65, SPARSE_MAX)][5:] == [32, 32, 32]
    assert 64 < SPARSE_MAX < 255 and SPARSE_MAX < SPARSE_CAP      # a lane with two entries and a dense 512-member group both exist


def test_streaming_steps_match_the_synchronous_replay(engine_factory):
    """The streaming case's steps once more, one synchronous aggregate each on a second handle: the same bytes per step."""
    r = _result("streaming", engine_factory)
    n_comm, spe = 8, 4
    e = CS._engine(engine_factory, 8 * 96, CS._prog_points(8 * 96), spe)
    comm = CS._committees(e, r["ep"], "sstream", 8 * 96, n_comm)
    assert np.array_equal(comm.members, r["comm"].members)
    for s in range(len(r["unions"]) // n_comm):
        unions = r["unions"][s * n_comm:(s + 1) * n_comm]
        atts, arena = H.committee_attestations(comm, CS._tree(), r["ep"], list(range(n_comm)), unions, spe)
        t_rows, t_bits = CS._dev(atts), CS._dev(arena)
        agg = e.aggregate(packed=(pea.DeviceRows(t_rows.data_ptr(), n_comm, keep=t_rows),
                                  pea.DeviceArena(t_bits.data_ptr(), t_bits.numel(), keep=t_bits)),
                          want_aggregate_pubkeys=True)
        o = _outputs(agg)
        assert np.array_equal(o["pk"], r["pk"][s * n_comm:(s + 1) * n_comm]), s
        assert np.array_equal(o["count"], r["count"][s * n_comm:(s + 1) * n_comm]), s


def test_named_outputs(engine_factory):
    r = _result("special_registries", engine_factory)
    assert r["pk"][2].tobytes() != CS.INF96            # S_c minus an absentees' sum at infinity: S_c itself
    mixed = _result("mixed_aggregate", engine_factory)
    assert mixed["pk"][14].tobytes() == CS.INF96       # nobody attests (direct route): infinity


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
        for k in ("pk", "bits", "count"):
            out[name + "." + k] = r[k]
        out[name + ".n_cmpl"] = np.array(r["route"][1])
    np.savez(sys.argv[1], **out)
    for e in made:
        e.close()
