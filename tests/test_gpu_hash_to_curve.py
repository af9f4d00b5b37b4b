"""-m gpu: pe_hash_to_g2 / pe_map_to_g2 -- hash_to_curve for G2 (RFC 9380, BLS12381G2_XMD:SHA-256_SSWU_RO_) on the device, byte
for byte against tests/hash_to_curve_model.py.

Edges: k_h2c_expand runs a lane per message (a wave: 64 | 65), k_h2c_map and k_h2c_finish a lane pair (32 | 33 pairs fill a
wave; the map has two pairs a message: 16 | 17 lie inside 31 | 32 | 33's calls too).  SHA-256's padding: b0 hashes 64 + msg_len
+ 3 + dst_len + 1 bytes, with the 43-byte Ethereum tag 111 + msg_len + ... the lengths 0, 8, 9, 16, 17, 32 put the end of the
text on both sides of the 55 | 56 byte edge (where the length no longer fits the block) and of the 63 | 64 edge; b_i hashes
34 + dst_len bytes, dst_len 21 | 22 is its 55 | 56 edge; 1 and 255 are the tag's bounds."""
import random

import numpy as np
import pytest

import pos_evolution_amd as pea
import pos_evolution_amd.synth as synth
from oracle import g1, g2
from oracle.g1 import P, R_ORDER
from pos_evolution_amd import _abi, forkchoice
from tests import hash_to_curve_model as hm
from tests import helpers as H

pytestmark = pytest.mark.gpu
ETH = hm.ETH2_DST


@pytest.fixture(scope="module")
def engine(engine_factory):
    return engine_factory(device=0)


def _roots(n, seed=1):
    rng = random.Random(seed)
    return [bytes(rng.randrange(256) for _ in range(32)) for _ in range(n)]


@pytest.fixture(scope="module")
def roots65():
    """65 roots and their model points, computed once."""
    roots = _roots(65)
    return roots, [g2.to_bytes192(hm.hash_to_g2(r, ETH)) for r in roots]


def _want(msgs, dst):
    return [g2.to_bytes192(hm.hash_to_g2(m, dst)) for m in msgs]


def _rows(a):
    return [bytes(r) for r in np.asarray(a)]


@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 64, 65])
def test_counts_at_the_wave_edges(engine, roots65, n):
    roots, want = roots65
    got, status = engine.hash_to_g2(roots[:n], want_status=True)
    assert got.shape == (n, 192) and _rows(got) == want[:n]
    assert status.tolist() == [0] * n
    if n == 33:
        assert _rows(forkchoice.hash_to_curve_g2(engine, roots[:n])) == want[:n]
        assert _rows(engine.hash_to_g2(np.frombuffer(b"".join(roots[:n]), dtype=np.uint8).reshape(n, 32))) == want[:n]


@pytest.mark.parametrize("msg_len", [0, 8, 9, 16, 17, 32])
def test_padding_edges_of_the_message(engine, msg_len):
    rng = random.Random(100 + msg_len)
    msgs = [bytes(rng.randrange(256) for _ in range(msg_len)) for _ in range(3)]
    assert _rows(engine.hash_to_g2(msgs, ETH)) == _want(msgs, ETH)


@pytest.mark.parametrize("dst_len", [1, 21, 22, 255])
def test_tag_edges(engine, dst_len):
    dst = bytes((37 * i + dst_len) % 251 + 1 for i in range(dst_len))
    msgs = _roots(2, seed=dst_len)
    assert _rows(engine.hash_to_g2(msgs, dst)) == _want(msgs, dst)


def test_the_rfc_messages(engine):
    v = hm.load_vectors()
    dst = v["dst"].encode()
    for case in v["points"]:       # two lengths: two calls
        want = (tuple(int(t, 16) for t in case["x"]), tuple(int(t, 16) for t in case["y"]))
        got = engine.hash_to_g2([case["msg"].encode()], dst)
        assert bytes(got[0]) == g2.to_bytes192(want)
    # the longest message the call takes
    msg = bytes(range(255))
    assert _rows(engine.hash_to_g2([msg], dst)) == _want([msg], dst)


def _map(engine, us):
    ub = np.frombuffer(b"".join(hm.u_to_bytes(u0, u1) for u0, u1 in us), dtype=np.uint8).reshape(-1, 192)
    return _rows(engine.map_to_g2(ub))


def test_map_to_g2_special_inputs(engine):
    u = (0x1234567 % P, 0x89ABCDEF01 % P)
    cases = [
        ((0, 0), (0, 0)),                       # the exceptional case tv1 == 0, twice: a doubling as well
        ((0, 0), u),
        (u, u),                                 # equal points: the add is a doubling
        (u, g2.f2_neg(u)),                      # opposite points: the identity
        ((0, 7), (0, 8)),                       # sgn0's second branch: c0 == 0, c1 odd | c1 even
        ((0, P - 1), (P - 1, 0)),               # the largest canonical words
    ]
    want = [g2.to_bytes192(hm.map_to_g2(u0, u1)) for u0, u1 in cases]
    assert want[3] == bytes([0x40]) + bytes(191)
    assert hm.sgn0((0, 7)) == 1 and hm.sgn0((0, 8)) == 0
    assert _map(engine, cases) == want
    assert _map(engine, cases[3:4]) == want[3:4]     # the identity alone in its call


def test_map_to_g2_random_inputs_take_both_branches(engine):
    rng = random.Random(64)
    us = [((rng.randrange(P), rng.randrange(P)), (rng.randrange(P), rng.randrange(P))) for _ in range(64)]
    took = [hm.swu_takes_x1(u) for pair in us for u in pair]
    assert True in took and False in took       # g(x1) a square, and not
    assert _map(engine, us) == [g2.to_bytes192(hm.map_to_g2(u0, u1)) for u0, u1 in us]


def test_map_to_g2_refuses_a_word_that_is_not_below_p(engine):
    good = hm.u_to_bytes((1, 2), (3, 4))
    for k in range(4):
        for v in (P, (1 << 384) - 1):
            bad = bytearray(good)
            bad[48 * k:48 * k + 48] = v.to_bytes(48, "big")
            with pytest.raises(pea.EngineError) as err:
                engine.map_to_g2(np.frombuffer(bytes(good) + bytes(bad), dtype=np.uint8).reshape(2, 192))
            assert err.value.status == _abi.PE_ERR_INVALID_ARG
    assert _map(engine, [((1, 2), (3, 4))]) == [g2.to_bytes192(hm.map_to_g2((1, 2), (3, 4)))]
    assert engine.map_to_g2(np.zeros((0, 192), np.uint8)).shape == (0, 192)
    assert engine.hash_to_g2([]).shape == (0, 192)


# ------------------------------------------------------------------ end to end: real signatures decided from roots
N_KEYS = 33


@pytest.fixture(scope="module")
def signed(roots65):
    """33 keys, 33 roots: key j signs root j; sig = sk H(m), H from the model."""
    roots, want = roots65
    sk = [(0x1F2E3D4C5B6A7988 * (i + 1) + 0xABCDEF) % R_ORDER for i in range(N_KEYS)]
    pk = np.frombuffer(b"".join(g1.to_bytes96(g1.mul(k, g1.G)) for k in sk), dtype=np.uint8).reshape(N_KEYS, 96).copy()
    sig = np.frombuffer(b"".join(g2.to_bytes192(g2.mul(k, g2.from_bytes192(w))) for k, w in zip(sk, want)),
                        dtype=np.uint8).reshape(N_KEYS, 192).copy()
    return roots[:N_KEYS], pk, sig


def test_verification_fed_by_hash_to_g2(engine_factory, signed):
    roots, pk, sig = signed
    e = engine_factory(device=0)
    e.set_validators(np.full(N_KEYS, 32 * 10 ** 9, dtype=np.uint64), np.ones(N_KEYS, dtype=np.uint8), pk)
    index = np.arange(N_KEYS, dtype=np.uint32)
    off = np.arange(N_KEYS + 1, dtype=np.uint32)
    msgs = e.hash_to_g2(roots)
    assert e.fast_aggregate_verify(index, off, msgs, sig).tolist() == [1] * N_KEYS
    assert e.batch_verify(pk, msgs, sig).tolist() == [1] * N_KEYS
    # one flipped bit of one message
    flipped = list(roots)
    flipped[17] = bytes([roots[17][0] ^ 1]) + roots[17][1:]
    bad = e.hash_to_g2(flipped)
    want = [1] * N_KEYS
    want[17] = 0
    assert _rows(bad[:17]) == _rows(msgs[:17]) and bytes(bad[17]) != bytes(msgs[17])
    assert e.fast_aggregate_verify(index, off, bad, sig).tolist() == want
    assert e.batch_verify(pk, bad, sig).tolist() == want
    # one aggregate of all 33 keys over one root
    h0 = g2.from_bytes192(bytes(msgs[0]))
    sk_sum = sum((0x1F2E3D4C5B6A7988 * (i + 1) + 0xABCDEF) % R_ORDER for i in range(N_KEYS)) % R_ORDER
    agg = np.frombuffer(g2.to_bytes192(g2.mul(sk_sum, h0)), dtype=np.uint8).reshape(1, 192)
    whole = np.array([0, N_KEYS], dtype=np.uint32)
    assert e.fast_aggregate_verify(index, whole, msgs[:1], agg).tolist() == [1]
    assert e.fast_aggregate_verify(index, whole, bad[17:18], agg).tolist() == [0]


def test_device_resident_points_into_verify_resident(engine_factory, roots65):
    """roots -> H(m) -> verdict with the points in device memory throughout: 33 groups, one committee each."""
    import torch
    from tests.test_gpu_resident_rows import _dev_rows

    roots, want_pts = roots65
    n_val, n_comm, spe, size, a, b = 512, 64, 32, 8, 0x1234567, 0x89ABCDE
    e = engine_factory(device=0)
    tree = synth.random_tree(96, 7, "branchy")
    H.load_tree(e, tree)
    e.set_validators(synth.balances(n_val, 7, mixed=True), synth.validator_flags(n_val, 7), synth.registry_points(e, n_val, a, b))
    epoch = int(tree.slot.max()) // spe + 1
    comm = synth.random_committees(n_val, n_comm, 7)
    e.set_committees(epoch, comm.offsets, comm.members)
    e.on_tick((epoch + 1) * spe * 12)
    n_groups = N_KEYS
    bits = [np.ones(size, dtype=bool) for _ in range(n_groups)]
    atts, arena = H.committee_attestations(comm, tree, epoch, list(range(n_groups)), bits)
    sigs = []
    for g in range(n_groups):
        mem = comm.members[comm.offsets[g]:comm.offsets[g + 1]]
        sk = (len(mem) * a + int(mem.astype(np.int64).sum()) * b) % R_ORDER
        sigs.append(g2.compress(g2.mul(sk, g2.from_bytes192(want_pts[g]))))
    sigs = np.frombuffer(b"".join(sigs), dtype=np.uint8).reshape(n_groups, 96).copy()

    def decide(msgs):
        agg = e.aggregate_signed(sigs, packed=(_dev_rows(atts), arena), compressed=True, want_aggregate_pubkeys=True)
        assert agg["n_groups"] == n_groups
        gof = np.asarray(agg["group_of"][:n_groups])
        t_roots = torch.from_numpy(np.frombuffer(b"".join(msgs), dtype=np.uint8).copy()).cuda()
        t_out = torch.zeros(192 * n_groups + 16, dtype=torch.uint8, device="cuda")
        assert t_roots.data_ptr() % 16 == 0 and t_out.data_ptr() % 16 == 0
        out = pea.DeviceArena(t_out.data_ptr(), 192 * n_groups, keep=t_out)
        res = e.hash_to_g2((pea.DeviceArena(t_roots.data_ptr(), 32 * n_groups, keep=t_roots), 32), out=out)
        assert res is out
        verdict = e.verify_resident(out, point_of_row=np.arange(n_groups, dtype=np.uint32), apply=False)
        # the same through an output that is not 16-byte aligned (written through a copy)
        off8 = pea.DeviceArena(t_out.data_ptr() + 8, 192 * n_groups, keep=t_out)
        first = t_out[:192 * n_groups].cpu().numpy().copy()
        e.hash_to_g2(msgs, out=off8)
        assert np.array_equal(t_out[8:8 + 192 * n_groups].cpu().numpy(), first)
        return [int(verdict[gof[r]]) for r in range(n_groups)], first

    verdicts, pts = decide(roots[:n_groups])
    assert pts.tobytes() == b"".join(want_pts[:n_groups])
    assert verdicts == [1] * n_groups
    flipped = list(roots[:n_groups])
    flipped[5] = flipped[5][:31] + bytes([flipped[5][31] ^ 0x80])
    want = [1] * n_groups
    want[5] = 0
    assert decide(flipped)[0] == want


def test_argument_errors(engine_factory, engine):
    roots = _roots(2)
    d = engine_factory(device=0)
    d.dist_init_custom(0, 1, lambda *x: 0, lambda *x: 0)
    for call in (lambda: d.hash_to_g2(roots), lambda: d.map_to_g2(np.zeros((1, 192), np.uint8))):
        with pytest.raises(pea.EngineError) as err:
            call()
        assert err.value.status == _abi.PE_ERR_STATE
    for call in (lambda: engine.hash_to_g2(roots), lambda: engine.map_to_g2(np.zeros((1, 192), np.uint8))):
        with engine.pipeline():
            with pytest.raises(pea.EngineError) as err:
                call()
            assert err.value.status == _abi.PE_ERR_STATE
    for dst in (b"", bytes(256)):
        with pytest.raises(pea.EngineError) as err:
            engine.hash_to_g2(roots, dst)
        assert err.value.status == _abi.PE_ERR_INVALID_ARG
    with pytest.raises(pea.EngineError) as err:
        engine.hash_to_g2([bytes(256)])
    assert err.value.status == _abi.PE_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        engine.hash_to_g2([b"a", b"bc"])
    # and a valid call follows
    assert _rows(engine.hash_to_g2(roots)) == _want(roots, ETH)
