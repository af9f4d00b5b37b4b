"""-m gpu: pe_process_deposits / pe_deposit_signing_roots (engine_deposit.cpp, deposit_kernels.hip) against
tests/deposits_model.py, bit for bit: statuses, credited indices, every resident array read back through the _get calls and
pe_state_roots against tests/ssz_model.py over the model's grown registry.

Shapes: registries of 1, 63, 64, 65 and 1000 validators and batches of 1, 16, 65 and 300 deposits cross a wave (64), a
workgroup (256: the tile of k_deposit_resolve's ordered count) and, at 1000 + 300, the index's growth.  Signatures are real:
secret keys, keys sk G1, one message point M = m G2 and signatures sk M, as tests/test_gpu_bls_verify.py forms them; the
model takes the verdicts the construction fixes."""
import numpy as np
import pytest

from oracle import g1, g2
from oracle.g1 import R_ORDER
from tests import deposits_model as M
from tests import ssz_model as S

pytestmark = pytest.mark.gpu
ETH = 10**9
MSG_SCALAR = 0x5A3C19E0F1D2B4A6978877665544332211FFEEDDCCBBAA990011223344556677 % R_ORDER
N_KEYS = 24


@pytest.fixture(scope="module")
def pool():
    """N_KEYS real key pairs: (pubkey48, signature96 over the message point), and the message point itself."""
    msg = g2.mul(MSG_SCALAR, g2.G2)
    keys = []
    for i in range(N_KEYS):
        sk = (0x1F2E3D4C5B6A7988 * (i + 1) + 0xABCDEF) % R_ORDER
        keys.append((g1.compress(g1.mul(sk, g1.G)), g2.compress(g2.mul(sk * MSG_SCALAR % R_ORDER, g2.G2))))
    return {"keys": keys, "msg": g2.to_bytes192(msg), "wrong_msg": g2.to_bytes192(g2.mul(MSG_SCALAR + 1, g2.G2))}


class Rig:
    """An engine with every resident part loaded from a model registry."""

    def __init__(self, engine_factory, reg: S.Registry, prepare=None, active=False, points=None):
        self.e = e = engine_factory(device=0)
        self.reg = reg
        if prepare:
            prepare(e)                                   # a store: pe_store_init drops the resident parts, so it comes first
        n = len(reg)
        eff = np.array(reg.effective_balance, dtype=np.uint64)
        flags = np.array([2 * s + (1 if active else 0) for s in reg.slashed], dtype=np.uint8)
        e.set_validators(eff, flags, points(e) if points else None)
        e.state_set_validators(eff, flags | np.uint8(8 if active else 0))
        e.registry_set_epochs(np.array(reg.activation_epoch, dtype=np.uint64), np.array(reg.exit_epoch, dtype=np.uint64))
        e.state_set_balances(np.array(reg.balances, dtype=np.uint64), np.array(reg.inactivity_scores, dtype=np.uint64),
                             np.array(reg.withdrawable_epoch, dtype=np.uint64))
        e.registry_set_static(np.frombuffer(b"".join(reg.pubkeys), dtype=np.uint8).reshape(n, 48),
                              np.frombuffer(b"".join(reg.withdrawal_credentials), dtype=np.uint8).reshape(n, 32),
                              np.array(reg.activation_eligibility_epoch, dtype=np.uint64))
        e.participation_set(0, np.array(reg.current_epoch_participation, dtype=np.uint8))
        e.participation_set(1, np.array(reg.previous_epoch_participation, dtype=np.uint8))

    def snapshot(self):
        e = self.e
        eff, flags, _ = e.state_validators()
        act, ext, _ = e.registry_get_epochs()
        bal, score, wdr, _ = e.state_get_balances()
        leaf, wc, elig, _ = e.registry_static()
        return {"n": e.num_validators, "eff": eff.copy(), "flags": flags.copy(), "act": act.copy(), "ext": ext.copy(),
                "bal": bal.copy(), "score": score.copy(), "wdr": wdr.copy(), "leaf": leaf.copy(), "wc": wc.copy(),
                "elig": elig.copy(), "cur": e.participation_get(0).copy(), "prev": e.participation_get(1).copy()}

    def check_against_model(self):
        reg, s = self.reg, self.snapshot()
        assert s["n"] == len(reg)
        u64 = lambda x: np.array(x, dtype=np.uint64)  # noqa: E731
        assert np.array_equal(s["eff"], u64(reg.effective_balance)) and np.array_equal(s["bal"], u64(reg.balances))
        assert np.array_equal(s["flags"] & 2, np.array([2 * x for x in reg.slashed], dtype=np.uint8))
        assert np.array_equal(s["act"], u64(reg.activation_epoch)) and np.array_equal(s["ext"], u64(reg.exit_epoch))
        assert np.array_equal(s["wdr"], u64(reg.withdrawable_epoch)) and np.array_equal(s["elig"], u64(reg.activation_eligibility_epoch))
        assert np.array_equal(s["score"], u64(reg.inactivity_scores))
        assert s["leaf"].tobytes() == b"".join(S.pubkey_leaf(p) for p in reg.pubkeys)
        assert s["wc"].tobytes() == b"".join(reg.withdrawal_credentials)
        assert s["cur"].tolist() == reg.current_epoch_participation and s["prev"].tolist() == reg.previous_epoch_participation
        assert self.e.state_roots() == S.state_roots(reg)

    def run(self, deposits, sig_ok, msgs, proofs=None, index=0, root=None, **kw):
        """One call on the engine and on the model; statuses and indices compared, then every array."""
        rows = [(d.pubkey, d.withdrawal_credentials, d.amount, d.signature) for d in deposits]
        pr = None if proofs is None else np.frombuffer(b"".join(b"".join(p) for p in proofs), dtype=np.uint8)
        mp = None if msgs is None else np.frombuffer(b"".join(msgs), dtype=np.uint8)
        n_before = len(self.reg)
        res = self.e.process_deposits(rows, mp, pr, index, root, kw or None)
        status, idx = M.process_deposits(self.reg, deposits, sig_ok, proofs, index, root or b"", **kw)
        assert res["status"].tolist() == status, (res["status"].tolist(), status)
        assert res["index"].tolist() == idx
        bad = status.count(M.BAD_PROOF)
        assert res["n_bad_proof"] == bad and res["n_validators"] == len(self.reg) == self.e.num_validators
        assert res["n_appended"] == (0 if bad else status.count(M.APPENDED)) == len(self.reg) - n_before
        assert res["n_topups"] == (0 if bad else status.count(M.TOPUP)) and res["n_ignored"] == status.count(M.IGNORED_BAD_SIGNATURE)
        self.check_against_model()
        return res


def registry(n, seed):
    return S.random_registry(n, seed, S.ENGINE_MAX_EFFECTIVE_BALANCE)


def dep(pubkey, signature=bytes(96), amount=32 * ETH, wc=None):
    return M.DepositData(bytes(pubkey), wc if wc is not None else bytes([len(pubkey), amount % 251]) * 16, int(amount), bytes(signature))


def mixed_batch(reg, n_batch, seed, pool, first_key=0):
    """Top-ups of registry keys, new real keys with their own signature (valid) or another key's (invalid), keys that are no
    curve points, and repeats of keys met earlier in the batch -- with the verdict bls.Verify gives each."""
    rng = np.random.default_rng(seed)
    deposits, sig_ok, used = [], [], []
    next_key = first_key
    for i in range(n_batch):
        kind = int(rng.integers(0, 6)) if i else 1
        amount = int(rng.integers(1, 40 * ETH))
        if kind == 0 or (kind == 1 and next_key >= N_KEYS):
            deposits.append(dep(reg.pubkeys[int(rng.integers(0, len(reg.pubkeys)))], rng.bytes(96), amount))
            sig_ok.append(False)
        elif kind == 1:
            pk, sig = pool["keys"][next_key]
            valid = bool(rng.integers(0, 4)) or i == 0
            deposits.append(dep(pk, sig if valid else pool["keys"][(next_key + 1) % N_KEYS][1], amount))
            sig_ok.append(valid)
            used.append(next_key)
            if valid or rng.integers(0, 2):      # an invalid first deposit: the key may come again, valid or not
                next_key += 1
        elif kind == 2:
            deposits.append(dep(rng.bytes(48), rng.bytes(96), amount))
            sig_ok.append(False)
        elif used:
            k = used[int(rng.integers(0, len(used)))]
            pk, sig = pool["keys"][k]
            valid = bool(rng.integers(0, 2))
            deposits.append(dep(pk, sig if valid else rng.bytes(96), amount))
            sig_ok.append(valid)
        else:
            deposits.append(dep(rng.bytes(48), rng.bytes(96), amount))
            sig_ok.append(False)
    return deposits, sig_ok


@pytest.mark.parametrize("n_reg,n_batch", [(1, 1), (63, 16), (64, 65), (65, 300), (1000, 16), (1000, 300)])
def test_mixed_batches_against_the_model(engine_factory, pool, n_reg, n_batch):
    rig = Rig(engine_factory, registry(n_reg, n_reg))
    deposits, sig_ok = mixed_batch(rig.reg, n_batch, 7 * n_reg + n_batch, pool)
    res = rig.run(deposits, sig_ok, [pool["msg"]] * n_batch)
    assert set(res["status"].tolist()) >= ({M.APPENDED} if n_batch == 1 else {M.APPENDED, M.TOPUP, M.IGNORED_BAD_SIGNATURE})


def test_signing_roots(engine_factory, pool):
    e = engine_factory(device=0)
    rng = np.random.default_rng(3)
    domain = rng.bytes(32)
    deposits = [dep(rng.bytes(48), rng.bytes(96), int(rng.integers(0, 2**63)) * 2 + 1, rng.bytes(32)) for _ in range(65)]
    got = e.deposit_signing_roots([(d.pubkey, d.withdrawal_credentials, d.amount, d.signature) for d in deposits], domain)
    assert got.tobytes() == b"".join(M.signing_root(d, domain) for d in deposits)
    assert e.deposit_signing_roots([], domain).shape == (0, 32)


def _keys_at_slot(slot, slots, count, rng):
    out = []
    while len(out) < count:
        pk = rng.bytes(48)
        if M.index_slot(pk, slots) == slot:
            out.append(pk)
    return out


def test_probe_paths(engine_factory, pool):
    """First-slot hit, a chain that wraps the table's end, a miss that walks that chain, a duplicated pubkey."""
    n_reg, n_batch = 1000, 8
    slots = M.index_slots(n_reg + n_batch)
    assert slots == 2048
    reg = registry(n_reg, 5)
    rng = np.random.default_rng(11)
    chain = _keys_at_slot(slots - 1, slots, 4, rng)      # all start at the last slot: the chain runs 2047, 0, 1, 2
    walker = _keys_at_slot(slots - 1, slots, 1, rng)[0]  # not in the registry: walks the whole chain to an empty slot
    for k, v in zip(chain, (100, 200, 300, 400)):
        reg.pubkeys[v] = k
    for v in range(n_reg):                               # nobody else may sit on the chain's path
        if v not in (100, 200, 300, 400):
            while M.index_slot(reg.pubkeys[v], slots) in (slots - 1, 0, 1, 2, 3):
                reg.pubkeys[v] = rng.bytes(48)
    reg.pubkeys[900] = reg.pubkeys[17]                   # a duplicate: the lowest index is the match
    reg.pubkeys[950] = reg.pubkeys[17]
    rig = Rig(engine_factory, reg)
    deposits = [dep(reg.pubkeys[5]), dep(chain[3], amount=3), dep(chain[0], amount=5), dep(walker), dep(reg.pubkeys[950], amount=7),
                dep(chain[2], amount=11), dep(reg.pubkeys[999]), dep(walker)]
    res = rig.run(deposits, [False] * n_batch, [pool["msg"]] * n_batch)
    assert res["index"].tolist() == [5, 400, 100, M.NONE, 17, 300, 999, M.NONE]
    assert rig.e.deposit_index_info()["slots"] == slots and rig.e.deposit_index_info()["keys"] == n_reg


def test_batch_order_of_one_new_key(engine_factory, pool):
    keys, msg = pool["keys"], pool["msg"]
    rig = Rig(engine_factory, registry(65, 9))
    n0 = len(rig.reg)
    (pa, sa), (pb, sb), (pc, sc), (pd, sd) = keys[:4]
    deposits = [dep(pa, sa), dep(pa, sb), dep(pa, sa),                 # valid first: then top-ups, whatever the signature
                dep(pb, sa), dep(pb, sc), dep(pb, sb), dep(pb, sa),    # invalid, invalid, valid, top-up
                dep(pc, sa), dep(pc, sb), dep(pc, sd)]                 # all invalid: nothing appended
    sig_ok = [True, False, True, False, False, True, False, False, False, False]
    res = rig.run(deposits, sig_ok, [msg] * len(deposits))
    assert res["status"].tolist() == [0, 1, 1, 2, 2, 0, 1, 2, 2, 2] and res["index"].tolist()[:7] == [n0, n0, n0, M.NONE, M.NONE, n0 + 1, n0 + 1]
    # many top-ups of ONE existing validator (atomic adds), and a new key interleaved with top-ups of the key created before it
    before = rig.reg.balances[3]
    deposits = [dep(rig.reg.pubkeys[3], amount=ETH + i) for i in range(200)]
    deposits[50:50] = [dep(pd, sd, 31 * ETH), dep(pd, sa, 2 * ETH)]
    deposits[120:120] = [dep(pc, sa), dep(pd, bytes(96), 5), dep(pc, sc, 7)]
    sig_ok = [False] * len(deposits)
    sig_ok[50] = sig_ok[122] = True
    res = rig.run(deposits, sig_ok, [msg] * len(deposits))
    assert rig.reg.balances[3] == before + sum(ETH + i for i in range(200)) and res["n_appended"] == 2
    assert rig.reg.effective_balance[n0 + 2] == 31 * ETH and rig.reg.balances[n0 + 2] == 33 * ETH + 5


def test_signature_kinds(engine_factory, pool):
    keys, msg = pool["keys"], pool["msg"]
    rig = Rig(engine_factory, registry(64, 13))
    outside_g1 = g1.curve_point_from_x(7)
    assert not g1.in_subgroup(outside_g1)
    outside_g2 = None
    for x0 in range(1, 64):                                 # a curve point of E'(Fp2) that is no multiple of the generator
        enc = bytes([0x80]) + bytes(47) + int(x0).to_bytes(48, "big")
        try:
            outside_g2 = g2.decompress(enc)
        except Exception:
            outside_g2 = None
        if outside_g2 is not None and g2.mul(R_ORDER, outside_g2) is not None:
            break
    assert outside_g2 is not None
    deposits = [dep(keys[4][0], keys[4][1]),                 # real
                dep(keys[5][0], keys[5][1]),                 # real, but the caller's message point is another one
                dep(g1.compress(outside_g1), keys[6][1]),    # a key that fails KeyValidate: outside the subgroup
                dep(bytes([0xC0]) + bytes(47), keys[6][1]),  # ... the identity
                dep(keys[7][0], g2.compress(outside_g2)),    # a signature outside G2
                dep(keys[8][0], bytes([0x20]) + bytes(95)),  # a signature that does not decode (no compression flag)
                dep(keys[9][0], bytes([0xC0]) + bytes(95)),  # the identity signature: decodes, in G2, pairing fails
                dep(keys[10][0], keys[10][1])]               # real
    msgs = [msg, pool["wrong_msg"]] + [msg] * 6
    res = rig.run(deposits, [True, False, False, False, False, False, False, True], msgs)
    assert res["status"].tolist() == [0, 2, 2, 2, 2, 2, 2, 0]


def test_proofs(engine_factory, pool):
    keys, msg = pool["keys"], pool["msg"]
    rig = Rig(engine_factory, registry(63, 21))
    deposits = [dep(keys[0][0], keys[0][1]), dep(rig.reg.pubkeys[7], amount=9), dep(keys[1][0], keys[0][1]), dep(keys[1][0], keys[1][1]),
                dep(rig.reg.pubkeys[8])]
    sig_ok = [True, False, False, True, False]
    msgs = [msg] * 5
    leaves = [M.deposit_data_root(d) for d in deposits]
    for first in (0, 1):                                     # a real deposit tree, at eth1_deposit_index 0 and 1
        root, proofs = M.deposit_tree_proofs(leaves, first)
        assert all(M.is_valid_merkle_branch(leaves[i], proofs[i], 33, first + i, root) for i in range(5))
        for level in (0, 31, 32):                            # one bad sibling: nothing applied, the others still reported
            bad = [list(p) for p in proofs]
            bad[2][level] = bytes(31) + b"\x01" if bad[2][level] == bytes(32) else bytes(32)
            snap = rig.snapshot()
            res = rig.run(deposits, sig_ok, msgs, bad, first, root)
            assert res["status"].tolist() == [0, 1, M.BAD_PROOF, 0, 1] and res["n_appended"] == 0
            after = rig.snapshot()
            assert all(np.array_equal(snap[k], after[k]) for k in snap)
    # indices beyond 2^32: the walk takes the 64-bit index bit by bit; every deposit against one root needs one branch each,
    # so the root is the first deposit's and the others fail
    rng = np.random.default_rng(2)
    base = 2**32 - 1 + 5
    proofs = [[rng.bytes(32) for _ in range(33)] for _ in range(5)]
    root = M.branch_root(leaves[0], proofs[0], base)
    res = rig.run(deposits, sig_ok, msgs, proofs, base, root)
    assert res["status"].tolist() == [0, M.BAD_PROOF, M.BAD_PROOF, M.BAD_PROOF, M.BAD_PROOF]
    res = rig.run(deposits[:1], sig_ok[:1], msgs[:1], proofs[:1], base, root)          # alone it is applied
    assert res["status"].tolist() == [0]
    root1, proofs1 = M.deposit_tree_proofs(leaves[1:], 1)
    rig.run(deposits[1:], sig_ok[1:], msgs[1:], proofs1, 1, root1)                      # a valid batch, applied
    rig.run([dep(keys[2][0], keys[2][1])], [True], [msg], None)                         # proofs = NULL


def test_growth_and_what_follows(engine_factory, pool):
    """An append that crosses the capacity, two calls in a row (the second sees the first's keys as hits), then the epoch
    boundary and get_head over the grown registry."""
    from pos_evolution_amd import synth
    from pos_evolution_amd.engine import BALANCES_RESIDENT
    from tests import registry_updates_model as RU
    from tests import rewards_model as RW

    keys, msg = pool["keys"], pool["msg"]
    n = 64
    reg = registry(n, 31)
    cur, fin = 20, 18
    reg.activation_epoch = [0] * n                              # everybody active, nobody leaving: a plain registry
    reg.exit_epoch = [M.FAR_FUTURE_EPOCH] * n
    reg.withdrawable_epoch = [M.FAR_FUTURE_EPOCH] * n
    reg.activation_eligibility_epoch = [0] * n
    reg.effective_balance = [32 * ETH] * n
    reg.slashed = [0] * n
    reg.balances = [32 * ETH + 1000 * v for v in range(n)]      # sizes the rewards' products stay inside uint64 with
    reg.inactivity_scores = [v % 7 for v in range(n)]
    tree = synth.random_tree(16, 1, "branchy")

    def store(e):
        e.store_init(0, 0, tree.roots[0].tobytes())
        for i in range(1, 16):
            e.add_block(tree.roots[i].tobytes(), tree.roots[int(tree.parent[i])].tobytes(), int(tree.slot[i]))

    rig = Rig(engine_factory, reg, prepare=store, active=True)
    e = rig.e
    votes = np.arange(n, dtype=np.uint32) % 16
    ep, sl = np.ones(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
    e._check(e._lib.pe_set_latest_messages(e._h, n, ep.ctypes.data, votes.ctypes.data, sl.ctypes.data))
    head_before, weights_before = e.get_head(), e.get_weights().copy()
    first = [dep(keys[i][0], keys[i][1]) for i in range(10)]
    rig.run(first, [True] * 10, [msg] * 10)                     # 64 -> 74: beyond what the arrays were allocated for
    second = [dep(keys[i][0], bytes(96), amount=ETH) for i in range(10)] + [dep(keys[i][0], keys[i][1]) for i in range(10, 24)]
    res = rig.run(second, [False] * 10 + [True] * 14, [msg] * 24)   # the first call's keys are hits now; 74 -> 88
    assert res["index"].tolist()[:10] == list(range(64, 74)) and res["n_appended"] == 14
    assert e.deposit_index_info()["keys"] == 88
    assert e.get_head() == head_before and np.array_equal(e.get_weights(), weights_before)   # get_head cannot see them
    # the epoch boundary over the grown arrays
    a = {"elig": np.array(reg.activation_eligibility_epoch, dtype=np.uint64), "act": np.array(reg.activation_epoch, dtype=np.uint64),
         "ext": np.array(reg.exit_epoch, dtype=np.uint64), "wdr": np.array(reg.withdrawable_epoch, dtype=np.uint64),
         "eff": np.array(reg.effective_balance, dtype=np.uint64), "bal": np.array(reg.balances, dtype=np.uint64),
         "slashed": np.zeros(len(reg), dtype=np.uint8)}
    want, st = RU.registry_updates_sequential(a, cur, fin, RU.Params())
    got = e.registry_updates(cur, fin)
    assert got["n_marked_eligible"] == st["n_marked_eligible"] == 24   # every new validator has the full effective balance
    act, ext, _ = e.registry_get_epochs()
    elig = e.registry_static()[2]
    assert np.array_equal(elig, want["elig"]) and np.array_equal(act, want["act"]) and np.array_equal(ext, want["ext"])
    reg.activation_eligibility_epoch = [int(x) for x in want["elig"]]
    n_active, total, idx = e.active_set(cur, want_indices=True)
    assert n_active == 64 and idx.tolist() == list(range(64)) and total == 64 * 32 * ETH
    snap = rig.snapshot()
    rp = dict(vars(RW.Params()))
    rp.pop("increment")
    want_bal, want_sc, _ = RW.run_numpy(snap["eff"], snap["flags"], snap["prev"], snap["wdr"], snap["bal"], snap["score"], cur, fin)
    e.rewards_and_penalties(cur, fin, rp)
    bal, sc, _, _ = e.state_get_balances()
    assert np.array_equal(bal, want_bal) and np.array_equal(sc, want_sc) and not np.array_equal(bal, snap["bal"])
    assert np.array_equal(bal[64:], snap["bal"][64:])            # not active in the previous epoch: not eligible
    reg.balances, reg.inactivity_scores = [int(x) for x in bal], [int(x) for x in sc]
    changed, eff_new = e.effective_balance_updates(BALANCES_RESIDENT)
    model_eff = [min(b - b % ETH, 32 * ETH) if (b + ETH // 4 < f or f + 5 * (ETH // 4) < b) else f
                 for b, f in zip(reg.balances, reg.effective_balance)]
    assert eff_new.tolist() == model_eff
    reg.effective_balance = model_eff
    assert e.state_roots() == S.state_roots(reg)


def test_the_pubkey_table_grows_with_the_registry(engine_factory, pool):
    """Where keys are loaded the creators' decoded keys follow the registry's points, in both field forms: sums over new and
    old indices, KeyValidate over the whole table."""
    from pos_evolution_amd import synth

    keys, msg = pool["keys"], pool["msg"]
    n = 64
    held = {}

    def points(e):
        held["pts"] = synth.registry_points(e, n)
        return held["pts"]

    rig = Rig(engine_factory, registry(n, 41), points=points)
    e = rig.e
    deposits = [dep(keys[0][0], keys[0][1]), dep(rig.reg.pubkeys[3]), dep(keys[1][0], keys[0][1]), dep(keys[2][0], keys[2][1]),
                dep(keys[1][0], keys[1][1])]
    res = rig.run(deposits, [True, False, False, True, True], [msg] * 5)
    assert res["index"].tolist() == [64, 3, M.NONE, 65, 66]
    new = [g1.decompress(keys[k][0]) for k in (0, 2, 1)]           # validators 64, 65, 66
    got = e.g1_sum(np.array([0, 3, 4, 6], dtype=np.uint32), np.array([64, 65, 66, 5, 66, 7], dtype=np.uint32))
    assert got[0].tobytes() == g1.to_bytes96(g1.sum_points(new))
    assert got[1].tobytes() == held["pts"][5].tobytes()
    assert got[2].tobytes() == g1.to_bytes96(g1.add(new[2], g1.from_bytes96(held["pts"][7].tobytes())))
    assert e.g1_key_validate().tolist() == [0] * 67


def test_refusals(engine_factory, pool):
    import pos_evolution_amd as pea
    from pos_evolution_amd import _abi

    keys, msg = pool["keys"], pool["msg"]
    one = [dep(keys[0][0], keys[0][1])]

    def refused(e, code, deposits=one):
        n = e.num_validators
        with pytest.raises(pea.EngineError) as err:
            e.process_deposits([(d.pubkey, d.withdrawal_credentials, d.amount, d.signature) for d in deposits],
                               np.frombuffer(msg * len(deposits), dtype=np.uint8))
        assert err.value.status == code and e.num_validators == n

    reg = registry(8, 1)
    n = len(reg)
    eff, flags = np.array(reg.effective_balance, dtype=np.uint64), np.zeros(n, dtype=np.uint8)
    balances = np.array(reg.balances, dtype=np.uint64)          # copies: the registry below grows
    pubkeys = np.frombuffer(b"".join(reg.pubkeys), dtype=np.uint8).reshape(n, 48).copy()
    parts = [lambda e: e.registry_set_epochs(np.zeros(n, dtype=np.uint64), np.full(n, M.FAR_FUTURE_EPOCH, dtype=np.uint64)),
             lambda e: e.state_set_balances(balances),
             lambda e: e.registry_set_static(pubkeys, np.zeros((n, 32), dtype=np.uint8), np.zeros(n, dtype=np.uint64))]
    for missing in range(3):                                    # each missing resident part
        e = engine_factory(device=0)
        e.set_validators(eff, flags)
        for k, load in enumerate(parts):
            if k != missing:
                load(e)
        refused(e, _abi.PE_ERR_STATE)
    rig = Rig(engine_factory, reg, prepare=lambda e: e.store_init(0, 0, bytes(32)))   # the slasher needs a store
    e = rig.e
    before = rig.snapshot()
    refused(e, _abi.PE_ERR_INVALID_ARG, [dep(keys[0][0], keys[0][1], amount=2**63 + 1)])
    e.slasher_enable(4, 16)
    refused(e, _abi.PE_ERR_STATE)
    after = rig.snapshot()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    e.slasher_disable()
    rig.run([dep(keys[0][0], keys[0][1], amount=2**63)], [True], [msg])     # 2^63 itself is allowed
    d = engine_factory(device=0)                                # a handle that exchanges with other ranks
    d.set_validators(eff, flags)
    for load in parts:
        load(d)
    d.dist_init_custom(0, 1, lambda *a: 0, lambda *a: 0)
    refused(d, _abi.PE_ERR_STATE)
