"""-m gpu: the registry's per-validator columns (reg_columns.h) through every call that sizes, grows or fills them, at the
sizes where sizing can go wrong: registries of 1, 3, 4, 5, 6 and 9 validators straddle the four-row padding, and the growth
steps cross the allocation a smaller registry left.

After every step every column is read back through the getters and compared, all rows, with a model that is a dict of lists:
pe_set_validators grown and shrunk with votes and participation written in between (old rows kept, fresh rows without a
message and without participation, the dependent sets dropped), with and without vote expiry and pubkeys; deposits appended
to a fully set registry of 3 (3 -> 4 -> 5 -> 9: tests/deposits_model.py through the rig of tests/test_gpu_deposits.py), then
pe_state_roots, pe_ffg_balances and get_head over the grown arrays; the setters in both orders and a second time at the same n."""
import numpy as np
import pytest

from oracle import cport
from tests import deposits_model as M
from tests import ssz_model as S
from tests.test_gpu_deposits import ETH, Rig, dep, pool, registry  # noqa: F401  (pool: the module's key fixture)
from tests.test_gpu_ffg_sums import _want as ffg_model
from tests.test_gpu_prune import _lm_slots, _set_lm

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
N_BLOCKS = 6
FAR = 2**64 - 1


def store(e):
    """A chain of N_BLOCKS blocks: the latest messages name block indices."""
    roots = [bytes([i + 1]) * 32 for i in range(N_BLOCKS)]
    e.store_init(0, 0, roots[0])
    for i in range(1, N_BLOCKS):
        e.add_block(roots[i], roots[i - 1], i)
    return roots


def fresh_model():
    return {k: [] for k in ("bal", "flags", "vote_epoch", "vote_block", "vote_slot", "cur", "prev")} | {
        "view": None, "epochs": None, "balances": None, "static": None}


def model_set_validators(m, bal, flags):
    """pe_set_validators: the justified data replaced, messages and participation kept for the rows that stay, fresh rows empty;
    a registry of another size drops the epochs, the resident balances and the static part."""
    n, old = len(bal), len(m["bal"])
    m["bal"], m["flags"] = [int(b) for b in bal], [int(f) for f in flags]
    for key, empty in (("vote_epoch", 0), ("vote_block", NONE), ("vote_slot", 0), ("cur", 0), ("prev", 0)):
        m[key] = m[key][:n] + [empty] * max(0, n - old)
    if n != old:
        m["epochs"] = m["balances"] = m["static"] = None
    if m["view"] is not None:    # a view of its own keeps the rows that stay; the caller writes the others
        m["view"] = ([b for b in m["view"][0][:n]], [f for f in m["view"][1][:n]])


def check(e, m, expiry):
    n = len(m["bal"])
    assert e.num_validators == n
    ep, bi = e.latest_messages()
    assert ep.tolist() == m["vote_epoch"] and bi.tolist() == m["vote_block"]
    assert _lm_slots(e).tolist() == (m["vote_slot"] if expiry else [0] * n)
    assert e.participation_get(0).tolist() == m["cur"] and e.participation_get(1).tolist() == m["prev"]
    assert e.validator_flags().tolist() == m["flags"]
    eff, sflags, is_set = e.state_validators()
    if m["view"] is None:        # the view mirrors the registry: active now => active in the previous epoch
        assert not is_set and eff.tolist() == m["bal"] and sflags.tolist() == [(f & 3) | (8 if f & 1 else 0) for f in m["flags"]]
    else:
        k = len(m["view"][0])    # the rows somebody has written
        assert is_set and eff[:k].tolist() == m["view"][0] and sflags[:k].tolist() == m["view"][1]
    act, ext, is_set = e.registry_get_epochs()
    assert is_set == (m["epochs"] is not None) and (not is_set or [act.tolist(), ext.tolist()] == m["epochs"])
    b, sc, wd, is_set = e.state_get_balances()
    assert is_set == (m["balances"] is not None) and (not is_set or [b.tolist(), sc.tolist(), wd.tolist()] == m["balances"])
    leaf, wc, el, is_set = e.registry_static()
    assert is_set == (m["static"] is not None)
    if is_set:
        pk, want_wc, want_el = m["static"]
        assert leaf.tobytes() == b"".join(S.pubkey_leaf(p) for p in pk) and wc.tobytes() == b"".join(want_wc) and el.tolist() == want_el


def write_rows(e, m, rng, expiry, static_first):
    """Every column the caller writes, with values of this step: messages, participation, the view, and the three dependent
    sets in either order -- each of those twice, the second time at the same n (no re-allocation: the set stays set)."""
    n = len(m["bal"])
    m["vote_epoch"] = [int(x) for x in rng.integers(1, 9, size=n)]
    m["vote_block"] = [int(x) for x in rng.integers(0, N_BLOCKS, size=n)]
    m["vote_block"][n // 2], m["vote_epoch"][n // 2] = NONE, 0                  # one validator without a message
    m["vote_slot"] = [int(x) for x in rng.integers(0, 64, size=n)] if expiry else [0] * n
    _set_lm(e, m["vote_epoch"], m["vote_block"], m["vote_slot"] if expiry else None)
    m["cur"], m["prev"] = ([int(x) for x in rng.integers(0, 8, size=n)] for _ in range(2))
    e.participation_set(0, np.array(m["cur"], dtype=np.uint8))
    e.participation_set(1, np.array(m["prev"], dtype=np.uint8))

    def epochs():
        m["epochs"] = [[int(x) for x in rng.integers(0, 50, size=n)], [int(x) for x in rng.integers(50, 99, size=n)]]
        e.registry_set_epochs(*m["epochs"])

    def balances():
        m["balances"] = [[int(x) for x in rng.integers(1, 40 * ETH, size=n)], [int(x) for x in rng.integers(0, 9, size=n)],
                         [int(x) for x in rng.integers(0, 99, size=n)]]
        e.state_set_balances(*m["balances"])

    def static():
        m["static"] = ([rng.bytes(48) for _ in range(n)], [rng.bytes(32) for _ in range(n)], [int(x) for x in rng.integers(0, 99, size=n)])
        pk, wc, el = m["static"]
        e.registry_set_static(np.frombuffer(b"".join(pk), dtype=np.uint8), np.frombuffer(b"".join(wc), dtype=np.uint8), el)

    for setter in ((static, balances, epochs) if static_first else (epochs, balances, static)):
        setter()
        check(e, m, expiry)
        setter()
        check(e, m, expiry)


@pytest.mark.parametrize("expiry", [0, 4])
@pytest.mark.parametrize("with_points", [False, True])
def test_set_validators_grows_and_shrinks(engine_factory, expiry, with_points):
    from pos_evolution_amd import synth

    e = engine_factory(device=0, vote_expiry_slots=expiry)
    store(e)
    rng = np.random.default_rng(17 + expiry)
    m = fresh_model()
    pts = synth.registry_points(e, 9) if with_points else None
    for step, n in enumerate((3, 5, 9, 3, 6)):
        bal = rng.integers(1, 33, size=n).astype(np.uint64) * np.uint64(ETH)
        flags = rng.choice(np.array([0, 1, 1, 3], dtype=np.uint8), size=n)
        e.set_validators(bal, flags, None if pts is None else pts[:n])
        model_set_validators(m, bal, flags)
        check(e, m, expiry)                                   # old rows kept, fresh rows empty, the dependent sets dropped
        if pts is not None:                                   # the pubkey table in both field forms: a sum reads d_points30
            got = e.g1_sum(np.array([0, 1, 2], dtype=np.uint32), np.array([n - 1, 0], dtype=np.uint32))
            assert got[0].tobytes() == pts[n - 1].tobytes() and got[1].tobytes() == pts[0].tobytes()
        if step >= 1:                                         # from the second step on the view is one of its own
            m["view"] = ([int(x) for x in rng.integers(1, 33, size=n) * ETH], [int(x) for x in rng.choice([0, 1, 2, 3, 8, 9, 11], size=n)])
            e.state_set_validators(np.array(m["view"][0], dtype=np.uint64), np.array(m["view"][1], dtype=np.uint8))
        write_rows(e, m, rng, expiry, static_first=bool(step & 1))
        view = m["view"] or (m["bal"], [(f & 3) | (8 if f & 1 else 0) for f in m["flags"]])
        assert e.ffg_balances() == ffg_model(np.array(view[0], dtype=np.uint64), np.array(view[1], dtype=np.uint8),
                                             np.array(m["cur"], dtype=np.uint8), np.array(m["prev"], dtype=np.uint8))


@pytest.mark.parametrize("n", [1, 4])
def test_a_first_registry_at_the_padding(engine_factory, n):
    """One validator and a whole block of four, set once: the smallest registries, every column at its floor."""
    e = engine_factory(device=0, vote_expiry_slots=2)
    store(e)
    m, rng = fresh_model(), np.random.default_rng(n)
    bal, flags = np.full(n, 32 * ETH, dtype=np.uint64), np.ones(n, dtype=np.uint8)
    e.set_validators(bal, flags)
    model_set_validators(m, bal, flags)
    check(e, m, 2)
    write_rows(e, m, rng, 2, static_first=n == 4)


class GrownRig(Rig):
    """The deposit tests' rig over an engine with a store, with the static part set before or after the balances."""

    def __init__(self, engine_factory, reg, expiry, points, static_first):
        self.e = e = engine_factory(device=0, vote_expiry_slots=expiry)
        self.reg, self.roots = reg, store(e)
        n = len(reg)
        self.eff = np.array(reg.effective_balance, dtype=np.uint64)
        self.flags = np.array([2 * s + 1 for s in reg.slashed], dtype=np.uint8)
        e.set_validators(self.eff, self.flags, points(e) if points else None)
        e.state_set_validators(self.eff, self.flags | np.uint8(8))
        e.registry_set_epochs(np.array(reg.activation_epoch, dtype=np.uint64), np.array(reg.exit_epoch, dtype=np.uint64))

        def balances():
            e.state_set_balances(np.array(reg.balances, dtype=np.uint64), np.array(reg.inactivity_scores, dtype=np.uint64),
                                 np.array(reg.withdrawable_epoch, dtype=np.uint64))

        def static():
            e.registry_set_static(np.frombuffer(b"".join(reg.pubkeys), dtype=np.uint8).reshape(n, 48),
                                  np.frombuffer(b"".join(reg.withdrawal_credentials), dtype=np.uint8).reshape(n, 32),
                                  np.array(reg.activation_eligibility_epoch, dtype=np.uint64))

        for setter in ((static, balances) if static_first else (balances, static)):
            setter()
        e.participation_set(0, np.array(reg.current_epoch_participation, dtype=np.uint8))
        e.participation_set(1, np.array(reg.previous_epoch_participation, dtype=np.uint8))


@pytest.mark.parametrize("expiry,with_points,static_first", [(0, False, False), (4, True, True)])
def test_deposits_append_across_the_padding_and_the_capacity(engine_factory, pool, expiry, with_points, static_first):  # noqa: F811
    from pos_evolution_amd import synth

    keys, msg = pool["keys"], pool["msg"]
    held = {}

    def points(e):
        held["pts"] = synth.registry_points(e, 3)
        return held["pts"]

    rig = GrownRig(engine_factory, registry(3, 3), expiry, points if with_points else None, static_first)
    e = rig.e
    votes = {"epoch": [2, 3, 1], "block": [1, N_BLOCKS - 1, 2], "slot": [5, 6, 7] if expiry else [0, 0, 0]}
    _set_lm(e, votes["epoch"], votes["block"], votes["slot"] if expiry else None)
    first_key = 0
    for n_more in (1, 1, 4):                              # 3 -> 4: the padded block's last row; 4 -> 5; 5 -> 9: past the capacity
        deposits = [dep(keys[first_key + i][0], keys[first_key + i][1]) for i in range(n_more)]
        first_key += n_more
        rig.run(deposits, [True] * n_more, [msg] * n_more)     # every resident array and pe_state_roots against the model
        n = len(rig.reg)
        ep, bi = e.latest_messages()                      # the columns the rig does not read: no message, no justified data
        assert ep.tolist() == votes["epoch"] + [0] * (n - 3) and bi.tolist() == votes["block"] + [NONE] * (n - 3)
        assert _lm_slots(e).tolist() == votes["slot"] + [0] * (n - 3)
        assert e.validator_flags().tolist() == rig.flags.tolist() + [0] * (n - 3)
    assert len(rig.reg) == 9
    # ... and over the grown arrays: the roots (in rig.run), the FFG sums, get_head
    snap = rig.snapshot()
    assert e.ffg_balances() == ffg_model(snap["eff"], snap["flags"], snap["cur"], snap["prev"])
    parent = np.array([NONE] + list(range(N_BLOCKS - 1)), dtype=np.uint32)
    bal9 = np.concatenate([rig.eff, np.zeros(6, dtype=np.uint64)])
    flags9 = np.concatenate([rig.flags, np.zeros(6, dtype=np.uint8)])
    vote_block = np.array(votes["block"] + [NONE] * 6, dtype=np.uint32)
    head, weights = cport.get_head(parent, np.ones(N_BLOCKS, dtype=np.uint8), np.frombuffer(b"".join(rig.roots), dtype=np.uint8),
                                   vote_block, bal9, flags9, 0)
    assert np.array_equal(e.get_weights(), weights) and e.get_head() == rig.roots[head]
    if with_points:                                       # the creators' keys behind the registry's, in both field forms
        from oracle import g1
        got = e.g1_sum(np.array([0, 1, 2], dtype=np.uint32), np.array([8, 2], dtype=np.uint32))
        assert got[0].tobytes() == g1.to_bytes96(g1.decompress(keys[5][0])) and got[1].tobytes() == held["pts"][2].tobytes()
