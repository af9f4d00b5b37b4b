"""CPU: the model of the epoch-boundary functions (tests/epoch_model.py) is pinned to the reference's own text --
compute_proposer_index (pe:604-618) and process_effective_balance_updates (pe:122-133), whose fences are taken from the
reference's Markdown at test time and executed as they stand (tests/golden/generate_epoch.py; nothing of that text is
committed) -- and to tests/golden/epoch_vectors.json, the recorded answers of those fences, which travels everywhere.
The GPU tests (tests/test_gpu_epoch.py) hold the engine to the same model and file."""
import hashlib
import importlib.util
import os

import numpy as np
import pytest

from oracle import ref_extract
from tests import epoch_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ETH = 10**9
QUARTER = ETH // 4


def _generator():
    spec_ = importlib.util.spec_from_file_location("generate_epoch", os.path.join(HERE, "golden", "generate_epoch.py"))
    mod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(mod)
    return mod


GEN = _generator()
PROPOSER_ROWS, HYSTERESIS_ROWS = GEN.load()
needs_reference = pytest.mark.skipif(not ref_extract.reference_available(), reason="the reference's Markdown is not on this machine")


@pytest.fixture(scope="module")
def ref_ns():
    return GEN.reference_namespace()


# ---------------------------------------------------------------- the golden file: coverage, then the model against it
def test_golden_covers_the_late_acceptance_classes():
    late = [r for r in PROPOSER_ROWS if r["tag"] == "late"]
    assert all(r["n_active"] == 3 and r["eff_eth"] == 1 and r["indices"] is None for r in late)
    tries = {r["tries"] for r in late}
    for i in (0, 31, 32, 63, 64):
        assert i in tries, i
    assert any(t >= 128 for t in tries)


def test_golden_covers_a_registry_without_balance():
    zero = [r for r in PROPOSER_ROWS if r["tag"] == "zero"]
    assert all(r["eff_eth"] == 0 and r["max_tries"] == 128 for r in zero)
    assert any(r["proposer"] is not None and r["tries"] < 128 for r in zero)       # accepted through a random byte of 0
    assert any(r["proposer"] is None and r["tries"] == 128 for r in zero)          # exhausted
    for r in zero:
        if r["proposer"] is not None:
            seed = bytes.fromhex(r["seed"])
            assert hashlib.sha256(seed + (r["tries"] // 32).to_bytes(8, "little")).digest()[r["tries"] % 32] == 0


def test_golden_covers_the_shape_edges():
    edge = [r for r in PROPOSER_ROWS if r["tag"] == "edge"]
    assert sorted({r["n_active"] for r in edge}) == [1, 2, 3, 255, 256, 257, 1000]
    assert {r["rounds"] for r in edge} == {10, 90}
    assert any(r["indices"] is not None and r["n_val"] > r["n_active"] for r in edge)
    assert any(isinstance(r["eff_eth"], list) and 0 in r["eff_eth"] for r in edge)
    assert any(r["eff_eth"] == 32 for r in edge) and any(r["eff_eth"] == 1 for r in edge)


def test_golden_covers_the_hysteresis_thresholds():
    row = next(r for r in HYSTERESIS_ROWS if r["tag"] == "thresholds")
    assert (row["increment"], row["quotient"], row["down"], row["up"], row["max_eff"]) == (ETH, 4, 1, 5, 32 * ETH)
    cases = set(zip(row["eff"], row["balances"]))
    got = dict(zip(zip(row["eff"], row["balances"]), row["new"]))
    several = [n * ETH for n in (1, 2, 16, 31, 32)]
    for e in several:
        for d in (-1, 0, 1):
            assert (e, e - QUARTER + d) in cases and (e, e + 5 * QUARTER + d) in cases
        # one Gwei below the downward threshold moves, the threshold itself and above do not; mirrored upwards
        assert got[(e, e - QUARTER - 1)] == e - ETH and got[(e, e - QUARTER)] == e and got[(e, e - QUARTER + 1)] == e
        assert got[(e, e + 5 * QUARTER)] == e and got[(e, e + 5 * QUARTER - 1)] == e
        assert got[(e, e + 5 * QUARTER + 1)] == min(e + ETH, 32 * ETH)
        assert got[(e, 40 * ETH)] == 32 * ETH                     # above the cap
        assert got[(e, 0)] == 0                                   # balance 0
        assert (e, ETH - 1) in cases                              # below one increment
    assert got[(ETH, ETH - 1)] == ETH and got[(2 * ETH, ETH - 1)] == 0   # ... inside the band it stays, outside it is 0
    assert any(r["tag"] == "constants" and r["increment"] != ETH and r["max_eff"] != 32 * ETH for r in HYSTERESIS_ROWS)


@pytest.mark.parametrize("k", range(len(PROPOSER_ROWS)))
def test_model_proposer_equals_golden(k):
    r = PROPOSER_ROWS[k]
    got = M.proposer(GEN.expand_indices(r), GEN.expand_eff(r), bytes.fromhex(r["seed"]), r["rounds"], r["max_eff"],
                     r["max_tries"])
    assert got == (r["proposer"], r["tries"])


@pytest.mark.parametrize("k", range(len(HYSTERESIS_ROWS)))
def test_model_hysteresis_equals_golden(k):
    r = HYSTERESIS_ROWS[k]
    new, n_changed = M.effective_balance_updates(r["balances"], r["eff"], r["increment"], r["quotient"], r["down"], r["up"],
                                                 r["max_eff"])
    assert new.tolist() == r["new"] and n_changed == r["n_changed"]


# ---------------------------------------------------------------- the reference's text
@needs_reference
def test_golden_file_is_what_the_reference_text_gives():
    """Byte for byte: the committed vectors are the output of the reference's two fences."""
    assert GEN.render() == open(GEN.OUT).read()


@needs_reference
def test_model_proposer_equals_the_reference_text(ref_ns):
    rng = np.random.default_rng(2024)
    for case in range(60):
        n_val = int(rng.integers(1, 400))
        n_active = int(rng.integers(1, n_val + 1))
        indices = np.sort(rng.choice(n_val, size=n_active, replace=False)).tolist()
        eff = (rng.choice([0, 1, 5, 17, 32], size=n_val) * ETH).tolist()
        rounds = int(rng.choice([0, 1, 10, 90]))
        seed = hashlib.sha256(b"model-%d" % case).digest()
        max_tries = int(rng.choice([1, 33, 64, 65, 300]))
        want = GEN.ref_proposer(ref_ns, indices, eff, seed, rounds, 32 * ETH, max_tries)
        assert M.proposer(indices, eff, seed, rounds, 32 * ETH, max_tries) == want, case


@needs_reference
def test_model_hysteresis_equals_the_reference_text(ref_ns):
    rng = np.random.default_rng(122)
    for case in range(40):
        n = int(rng.integers(1, 300))
        increment = int(rng.choice([1, 10**6, ETH, 3 * ETH]))
        quotient, down, up = (int(x) for x in rng.integers(1, 9, size=3))
        max_eff = int(rng.integers(0, 64)) * increment
        eff = (rng.integers(0, 64, size=n) * increment).tolist()
        bal = [max(0, e + int(d)) for e, d in zip(eff, rng.integers(-3 * increment, 3 * increment + 1, size=n))]
        want = GEN.ref_balance_updates(ref_ns, bal, eff, increment, quotient, down, up, max_eff)
        new, n_changed = M.effective_balance_updates(bal, eff, increment, quotient, down, up, max_eff)
        assert new.tolist() == want, case
        assert n_changed == sum(1 for a, b in zip(eff, want) if a != b)
    # balances at the top of the uint64 range: the model's differences do not wrap
    top = 2**64 - 1
    want = GEN.ref_balance_updates(ref_ns, [top, top - 1, 0], [0, 32 * ETH, top - top % ETH], ETH, 4, 1, 5, 32 * ETH)
    new, _ = M.effective_balance_updates([top, top - 1, 0], [0, 32 * ETH, top - top % ETH], ETH, 4, 1, 5, 32 * ETH)
    assert new.tolist() == want == [32 * ETH, 32 * ETH, 0]
