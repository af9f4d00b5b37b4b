"""GPU: pe_verify_signatures.  Every case is held to tests/verify_signatures_model.py byte for byte: verdicts, statuses, the
stats of pe_profile_verify_stats and both weighted sums of pe_profile_verify_sums (the new kernels against closed forms, with no
pairing in between), and the aggregates to the closed form of the survivors' sum.

Points are made BY CONSTRUCTION, no pairing in Python: registry key v = (a + v b) G1 (synth.registry_points), H(m_g) = h_g G2,
and a group's signatures are the progression (a + v b) h_g G2, one addition per member.  s + 1 is an invalid signature.

Layout edges: a slot is a stripe of k members; S = 128 slots make a workgroup of k_g2_weighted_accumulate, 256 one of
k_g1_weighted_accumulate: group sizes 1, k, k + 1, S k, S k + 1 (and 257 at k = 1 for the G1 kernel's second workgroup)."""
import numpy as np
import pytest

from oracle import g2
from oracle.g1 import R_ORDER
from tests import verify_signatures_model as vm

pytestmark = pytest.mark.gpu
A, B = 0x1234567, 0x89ABCDE                # synth.registry_points' progression
N_VAL = 512
SCALAR_EDGES = (1, 2, 1 << 63, (1 << 64) - 1, 0xAAAAAAAAAAAAAAAA, 0x5555555555555555, 0xFFFFFFFF00000000, 0x8000000000000001)
H = [0x9E3779B97F4A7C15 + 0x1000003 * g for g in range(8)]
IDENTITY = bytes([0xC0]) + bytes(95)
INVALID_ARG = -1                           # PE_ERR_INVALID_ARG of include/posevo.h


def sk(v):
    return (A + v * B) % R_ORDER


@pytest.fixture(scope="module")
def engine(engine_factory):
    import pos_evolution_amd.synth as synth
    e = engine_factory(device=0)
    e.set_validators(np.full(N_VAL, 32 * 10 ** 9, dtype=np.uint64), np.ones(N_VAL, dtype=np.uint8), synth.registry_points(e, N_VAL))
    return e


class Case:
    """Groups of consecutive signers v0, v0 + 1, ...: members (signer, s, status, wire bytes), built with one addition each."""

    def __init__(self, sizes, first_signer=lambda g: 7 * g):
        self.offsets = [0]
        self.members, self.msgs = [], []
        for g, size in enumerate(sizes):
            h, v0 = H[g % len(H)], first_signer(g)
            pt, step = g2.mul(sk(v0) * h % R_ORDER, g2.G2), g2.mul(B * h % R_ORDER, g2.G2)
            for i in range(size):
                self.members.append([v0 + i, sk(v0 + i) * h % R_ORDER, 0, g2.compress(pt)])
                pt = g2.add(pt, step)
            self.offsets.append(len(self.members))
            self.msgs.append(h)

    def spoil(self, j):
        """member j's signature becomes (s + 1) G2"""
        m = self.members[j]
        m[1] = (m[1] + 1) % R_ORDER
        m[3] = g2.compress(g2.mul(m[1], g2.G2))

    def settle(self, j, status, enc):
        self.members[j][1:] = [None, status, enc]

    def run(self, e, r, k=None, index=None, device=False):
        """One call against the model; -> (verdicts, statuses, group verdicts, stats)."""
        if k is not None:
            e._profile_verify_set_stripe(k)
        n, n_groups = len(self.members), len(self.msgs)
        rows = list(range(n)) if index is None else index
        sig = np.zeros((max(rows) + 1 if rows else 0, 96), dtype=np.uint8)
        for j, row in enumerate(rows):
            sig[row] = np.frombuffer(self.members[j][3], dtype=np.uint8)
        arg = sig
        if device:
            import torch
            import pos_evolution_amd as pea
            st = torch.from_numpy(sig.reshape(-1).copy()).to("cuda:0")
            arg = pea.DeviceArena(st.data_ptr(), st.numel(), keep=st)
        msg = np.frombuffer(b"".join(g2.to_bytes192(g2.mul(h, g2.G2)) for h in self.msgs), dtype=np.uint8).reshape(-1, 192)
        signer = np.array([m[0] for m in self.members], dtype=np.uint32)
        got = e.verify_signatures(arg, signer, np.array(self.offsets, dtype=np.uint32), msg,
                                  index=None if index is None else np.array(index, dtype=np.uint32),
                                  scalars=None if r is None else np.array(r, dtype=np.uint64))
        stats = e._profile_verify_stats()
        verdict, status, group, agg = (x.tolist() if i < 3 else x for i, x in enumerate(got))
        print("verdicts", verdict, "status", status, "groups", group, "stats", stats)
        if r is not None:
            model = [(sk(m[0]), m[1], m[2]) for m in self.members]
            want = vm.verify(model, self.offsets, self.msgs, r, k=stats["k"])
            assert (verdict, status, group) == want[:3]
            assert tuple(stats[name] for name in vm.STAT_NAMES) == want[4]
            pk, sg = e._profile_verify_sums(n_groups)
            want_pk, want_sg = vm.sum_bytes(want[3])
            assert pk.tobytes() == want_pk and sg.tobytes() == want_sg
            assert agg.tobytes() == vm.aggregate_bytes(model, self.offsets, verdict)
        self.last, self.agg = (sig, signer, msg), agg
        return verdict, status, group, stats


def _scalars(n, seed=1):
    rng = np.random.default_rng(seed)
    return [int(v) | 1 for v in rng.integers(1, 1 << 63, size=n, dtype=np.uint64)]


@pytest.mark.parametrize("k,sizes", [(1, (1, 2, 129, 257)), (1, (128, 256, 1)), (2, (1, 2, 3, 256, 257)), (3, (1, 3, 4, 384)),
                                     (3, (385, 1, 3))])
def test_layout_edges_all_valid(engine, k, sizes):
    case = Case(sizes)
    n = len(case.members)
    verdict, status, group, stats = case.run(engine, _scalars(n, seed=n + k), k=k)
    assert verdict == [1] * n and status == [0] * n and group == [1] * len(sizes)
    assert stats["rechecked"] == 0 and stats["pairing_runs"] == 1 and stats["k"] == k
    sig, _, _ = case.last
    plain, _, bad = engine.aggregate_signatures(sig, np.array(case.offsets, dtype=np.uint32), check_subgroup=True)
    assert case.agg.tobytes() == plain.tobytes() and not bad.any()


def test_scalar_edges_mixed_within_a_wave(engine):
    """Neighbouring slots disagree on every plane: the scalars cycle through 1, 2, 2^63, 2^64 - 1 and the alternating patterns."""
    case = Case((70, 9, 33))
    n = len(case.members)
    r = [SCALAR_EDGES[i % len(SCALAR_EDGES)] for i in range(n)]
    for k in (2, 3, 16):
        verdict, _, group, _ = case.run(engine, r, k=k)
        assert verdict == [1] * n and group == [1, 1, 1]


@pytest.mark.parametrize("scalar", SCALAR_EDGES)
def test_one_scalar_for_a_whole_stripe_of_equal_keys(engine, scalar):
    """Every member of a stripe carries the same scalar AND the same key (a signer may appear any number of times): each plane
    adds P to an accumulator that is a multiple of P -- acc = 2 acc, then + P meets acc = P on the lowest plane of scalar 2 ...
    -- so the complete forms' doubling branch runs inside the Horner pass, in both kernels."""
    case = Case((6, 5), first_signer=lambda g: 40 + g)
    for j, m in enumerate(case.members):           # all members of a group: that group's first signer, the same signature
        first = case.members[case.offsets[0 if j < 6 else 1]]
        m[0], m[1], m[3] = first[0], first[1], first[3]
    verdict, _, group, _ = case.run(engine, [scalar] * 11, k=3)
    assert verdict == [1] * 11 and group == [1, 1]


@pytest.mark.parametrize("where", ("first_of_stripe", "last_of_stripe", "tail_stripe", "last_member"))
def test_one_invalid_member(engine, where):
    k, sizes = 3, (7, 10, 5)                       # group 1: stripes [7..9], [10..12], [13..15] and the one-member tail [16]
    j = {"first_of_stripe": 10, "last_of_stripe": 12, "tail_stripe": 16, "last_member": 16}[where]
    if where == "last_member":
        sizes, j = (7, 9, 5), 15                   # ... full stripes only: the group's last member ends one
    case = Case(sizes)
    case.spoil(j)
    n = len(case.members)
    verdict, status, group, stats = case.run(engine, _scalars(n, seed=j), k=k)
    assert verdict == [0 if i == j else 1 for i in range(n)] and group == [1, 0, 1] and status == [0] * n
    assert stats["failed_groups"] == 1 and stats["rechecked"] == sizes[1] and stats["pairing_runs"] == 2    # the neighbours pay nothing


def test_the_cancelling_pair(engine):
    """sig_a + D and sig_b - D: the plain aggregate verifies, the two members are forged.  What the feature exists for."""
    case = Case((4, 2))
    d = 0x1234567
    for j, sign in ((1, 1), (3, -1)):
        m = case.members[j]
        m[1] = (m[1] + sign * d) % R_ORDER
        m[3] = g2.compress(g2.mul(m[1], g2.G2))
    off = np.array(case.offsets, dtype=np.uint32)
    r = _scalars(6, seed=3)
    r[3] = r[1]                                                     # the documented hazard: weights the signers knew
    verdict, _, group, stats = case.run(engine, r)
    assert verdict == [1] * 6 and group == [1, 1] and stats["rechecked"] == 0
    sig, signer, msg = case.last
    plain = engine.aggregate_signatures(sig, off, check_subgroup=True)[0]
    assert engine.fast_aggregate_verify(signer, off, msg, engine.g2_decompress(plain)[0]).tolist() == [1, 1]
    r[3] = r[1] + 2
    verdict, _, group, _ = case.run(engine, r)
    assert verdict == [1, 0, 1, 0, 1, 1] and group == [0, 1]
    verdict, _, group, stats = case.run(engine, None)               # the engine's own weights
    assert verdict == [1, 0, 1, 0, 1, 1] and group == [0, 1] and stats["rechecked"] == 4


def _off_curve():
    from tests.g2_special import oracle_status
    for x0 in range(1, 64):
        enc = bytes([0x80]) + bytes(47) + x0.to_bytes(48, "big")
        if oracle_status(g2.decompress, enc) == 2:
            return enc
    raise AssertionError("no abscissa off the curve among 63")


def _outside_g2():
    for x0 in range(1, 64):
        enc = bytes([0x80]) + bytes(47) + x0.to_bytes(48, "big")
        try:
            pt = g2.decompress(enc)
        except ValueError:
            continue
        if g2.mul(R_ORDER, pt) is not None:
            return enc
    raise AssertionError("no curve point outside G2 among 63")


@pytest.mark.parametrize("invalid_neighbour", (False, True))
def test_settled_members_of_every_kind(engine, invalid_neighbour):
    case = Case((5, 6, 4, 3))
    malformed = bytearray(case.members[0][3])
    malformed[0] &= 0x7F                                            # no compression flag
    case.settle(1, 1, bytes(malformed))
    case.settle(3, 2, _off_curve())
    case.settle(6, 3, _outside_g2())
    case.settle(10, vm.STATUS_IDENTITY, IDENTITY)
    if invalid_neighbour:
        case.spoil(12)
    verdict, status, group, stats = case.run(engine, _scalars(18, seed=9), k=2)
    want = [1] * 18
    for j in (1, 3, 6, 10) + ((12,) if invalid_neighbour else ()):
        want[j] = 0
    assert verdict == want and group == [0, 0, 0 if invalid_neighbour else 1, 1]
    assert [status[j] for j in (1, 3, 6, 10)] == [1, 2, 3, 4] and sum(status) == 10
    assert stats["settled"] == 4 and stats["rechecked"] == (4 if invalid_neighbour else 0)    # settled members cost no recheck


def test_message_point_rules(engine):
    case = Case((2, 0, 3, 2))
    case.msgs[2] = 0                                                # the identity: every member 0
    verdict, _, group, stats = case.run(engine, _scalars(7, seed=4), k=2)
    assert verdict == [1, 1, 0, 0, 0, 1, 1] and group == [1, 1, 0, 1] and stats["rechecked"] == 0
    sig, signer, msg = case.last
    msg = msg.copy()
    msg[3, 191] ^= 1                                                # off its curve
    got = engine.verify_signatures(sig, signer, np.array(case.offsets, dtype=np.uint32), msg)
    assert got[0].tolist() == [1, 1, 0, 0, 0, 0, 0] and got[2].tolist() == [1, 1, 0, 2]


def test_index_indirection_and_device_input(engine):
    case = Case((5, 7, 130))
    n = len(case.members)
    index = [(37 * j + 11) % 151 for j in range(n)]                 # a permutation into a longer array (151 is prime)
    case.spoil(8)
    want = [0 if j == 8 else 1 for j in range(n)]
    for device in (False, True):
        verdict, _, group, _ = case.run(engine, _scalars(n, seed=12), k=3, index=index, device=device)
        assert verdict == want and group == [1, 0, 1]
    verdict, _, _, _ = case.run(engine, _scalars(n, seed=13), k=16, device=True)
    assert verdict == want


def test_error_returns_leave_the_outputs_untouched(engine_factory, engine):
    import ctypes as C
    import pos_evolution_amd as pea
    from pos_evolution_amd import _abi

    case = Case((3, 2))
    case.run(engine, _scalars(5))
    sig, signer, msg = case.last
    off = np.array(case.offsets, dtype=np.uint32)

    def call(e, sig=sig, signer=signer, off=off, index=None, scalars=None):
        verdict, status, group = np.full(5, 7, np.int32), np.full(5, 7, np.int32), np.full(2, 7, np.int32)
        out = np.full((2, 96), 7, np.uint8)
        p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        rc = e._lib.pe_verify_signatures(e._h, C.c_void_p(sig.ctypes.data), len(sig), None if index is None else p(index, C.c_uint32),
                                         p(signer, C.c_uint32), p(off, C.c_uint32), 2, p(msg, C.c_uint8),
                                         None if scalars is None else p(scalars, C.c_uint64), p(verdict, C.c_int32),
                                         p(status, C.c_int32), p(group, C.c_int32), p(out, C.c_uint8))
        untouched = (verdict == 7).all() and (status == 7).all() and (group == 7).all() and (out == 7).all()
        return rc, untouched

    assert call(engine) == (_abi.PE_OK, False)
    assert call(engine, scalars=np.array([1, 2, 0, 4, 5], np.uint64)) == (INVALID_ARG, True)
    assert call(engine, signer=np.array([0, 1, N_VAL, 3, 4], np.uint32)) == (INVALID_ARG, True)
    assert call(engine, index=np.array([0, 1, 2, 3, 5], np.uint32)) == (INVALID_ARG, True)
    assert call(engine, off=np.array([0, 4, 3], np.uint32)) == (INVALID_ARG, True)
    assert call(engine_factory(device=0)) == (_abi.PE_ERR_STATE, True)                  # no pubkeys
    d = engine_factory(device=0)
    d.dist_init_custom(0, 1, lambda *x: 0, lambda *x: 0)
    assert call(d) == (_abi.PE_ERR_STATE, True)
    with pytest.raises(pea.EngineError):
        engine._profile_verify_set_stripe(17)
    with pytest.raises(pea.EngineError):
        engine._profile_verify_set_stripe(0)


def test_forkchoice_surface(engine):
    from pos_evolution_amd import forkchoice
    case = Case((3, 2))
    case.spoil(4)

    class _Store:
        pass
    _Store.engine = engine
    sigs = [[m[3] for m in case.members[:3]], [m[3] for m in case.members[3:]]]
    msgs = [g2.to_bytes192(g2.mul(h, g2.G2)) for h in case.msgs]
    got = forkchoice.verify_attestation_signatures(_Store, [[m[0] for m in case.members[:3]], [m[0] for m in case.members[3:]]], msgs, sigs)
    assert got == [[True, True, True], [True, False]]
