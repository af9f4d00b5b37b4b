"""CPU: the two forms of tests/registry_updates_model.py held to each other -- the specification's sequential loop against
the closed form of the exit queue and the sorted head of the activation queue that the kernels compute -- on random
registries and at the churn edges; the churn limit against forkchoice.get_validator_churn_limit; the committed vectors; and
the kernels' resource log (no scratch)."""
import importlib.util
import json
import os
import re

import numpy as np
import pytest

from tests import registry_updates_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUR, FIN = 20, 18


def same_registry(x, y):
    return all(np.array_equal(x[k], y[k]) for k in M.FIELDS)


def both(a, cur, fin, p):
    s_out, s_st = M.registry_updates_sequential(a, cur, fin, p)
    n_out, n_st = M.registry_updates_numpy(a, cur, fin, p)
    assert s_st == n_st, (s_st, n_st)
    for k in M.FIELDS:
        assert np.array_equal(s_out[k], n_out[k]), k
    return n_out, n_st


@pytest.mark.parametrize("limit", [1, 2, 3, 4, 7])
def test_closed_form_against_sequential_on_random_registries(limit):
    p = M.Params(min_per_epoch_churn_limit=limit, max_per_epoch_activation_churn_limit=0 if limit % 2 else 2)
    for seed in range(40):
        n = 1 + (seed * 37) % 420
        a, _ = M.random_registry(n, 100 * limit + seed, CUR, FIN, p)
        before = M.copy_registry(a)
        both(a, CUR, FIN, p)
        assert same_registry(a, before)          # the model does not write its input


def test_every_class_occurs_from_256_validators_on():
    for n in (256, 257, 1023, 4097):
        a, counters = M.random_registry(n, n, CUR, FIN)
        assert M.every_class_occurred(counters), counters
        out, st = both(a, CUR, FIN, M.Params(min_per_epoch_churn_limit=3))
        assert st["n_ejected"] > 3 and st["queue_len"] > st["n_activated"] > 0 and st["n_marked_eligible"] > 0
        assert st["last_exit_epoch"] > st["first_exit_epoch"]


@pytest.mark.parametrize("L", [1, 2, 5])
def test_closed_form_at_the_churn_edges(L):
    for c0 in {0, L - 1, L, L + 1}:
        for e0_beyond in (False, True):
            fill = 0 if c0 >= L else c0
            for n_eject in {0, 1, L - fill, L - fill + 1, 3 * L + 2}:
                for interleave in (False, True):
                    a, p = M.exit_queue_case(300, CUR, L, c0, e0_beyond, n_eject, interleave)
                    out, st = both(a, CUR, FIN, p)
                    assert st["n_ejected"] == n_eject
                    if n_eject > L - fill:
                        assert st["last_exit_epoch"] > st["first_exit_epoch"]


def test_activation_queue_order_and_cap():
    p = M.Params(min_per_epoch_churn_limit=12, max_per_epoch_activation_churn_limit=8)
    a = M.blank_registry(300, p)
    q = np.arange(10, 290, 7)
    a["act"][q] = M.FAR
    a["elig"][q] = FIN
    a["elig"][q[-3:]] = [FIN - 2, FIN - 1, FIN + 1]     # later indices, earlier epochs: they go first; FIN + 1 is not queued
    out, st = both(a, CUR, FIN, p)
    assert st["activation_churn_limit"] == 8 and st["queue_len"] == q.size - 1 and st["n_activated"] == 8
    assert out["act"][q[-3]] != M.FAR and out["act"][q[-2]] != M.FAR and out["act"][q[-1]] == M.FAR
    assert (out["act"][q[:6]] != M.FAR).all() and (out["act"][q[6:-3]] == M.FAR).all()
    out, st = both(a, CUR, FIN, M.Params(min_per_epoch_churn_limit=12))
    assert st["n_activated"] == 12


def test_churn_limit_agrees_with_forkchoice():
    from pos_evolution_amd import forkchoice as fc
    for n_active in (0, 1, 4 * 65536 - 1, 4 * 65536, 5 * 65536 + 7, 10**6):
        for min_churn, quotient in ((4, 65536), (1, 4), (7, 1000)):
            p = M.Params(min_per_epoch_churn_limit=min_churn, churn_limit_quotient=quotient)
            want = fc.get_validator_churn_limit(None, n_active=n_active,
                                                preset={"MIN_PER_EPOCH_CHURN_LIMIT": min_churn, "CHURN_LIMIT_QUOTIENT": quotient})
            assert M.churn_limits(n_active, p)[0] == want


def test_refusals():
    a, _ = M.random_registry(300, 9, CUR, FIN)
    for form in (M.registry_updates_sequential, M.registry_updates_numpy):
        with pytest.raises(ValueError):
            form(a, CUR, FIN, M.Params(churn_limit_quotient=0))
        with pytest.raises(ValueError):
            form(a, M.FAR - 5, FIN, M.Params())
        with pytest.raises(ValueError):
            form(a, CUR, FIN, M.Params(min_validator_withdrawability_delay=M.FAR - CUR - 6))
        form(a, CUR, FIN, M.Params(min_validator_withdrawability_delay=256))


@pytest.mark.parametrize("sum_slashings", [0, 1, 10**9, 10**13, 2**62])
def test_slashings_forms_agree(sum_slashings):
    for seed, n in ((1, 1), (2, 300), (3, 1025)):
        a, _ = M.random_registry(n, seed, CUR, FIN, vector=64)
        flags = M.view_flags(a, CUR)
        bal_s, st_s = M.slashings_sequential(a, flags, CUR, sum_slashings, 3, 64)
        bal_n, st_n = M.slashings_numpy(a, flags, CUR, sum_slashings, 3, 64)
        assert st_s == st_n and np.array_equal(bal_s, bal_n)
        if n >= 256 and sum_slashings >= 10**13:          # large enough for a penalty of whole increments
            assert st_n["n_penalised"] > 0 and st_n["n_saturated"] > 0 and st_n["penalties"] > 0
    with pytest.raises(ValueError):
        M.slashings_numpy(a, flags, CUR, 2**63, 3, 64)
    with pytest.raises(ValueError):
        M.slashings_sequential(a, flags, M.FAR - 3, 1, 3, 64)


def test_golden_vectors_reproduce():
    spec = importlib.util.spec_from_file_location("generate_registry_updates",
                                                  os.path.join(ROOT, "tests", "golden", "generate_registry_updates.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    cases = json.load(open(M.GOLDEN_PATH))
    assert len(cases) >= 5 and os.path.getsize(M.GOLDEN_PATH) < 100 * 1024
    assert json.loads(json.dumps(gen.cases())) == cases                # the generator still writes this file
    # what the file pins: exits that spill over epochs, a churn limit the quotient decides, a queue longer than its cap, a
    # total above get_total_balance's floor, penalties on both sides of the min, penalties cut at the balance
    stats, slash = [c["stats"] for c in cases], [s["stats"] for c in cases for s in c["slashings"]]
    assert sum(st["n_ejected"] > st["churn_limit"] and st["last_exit_epoch"] > st["first_exit_epoch"] for st in stats) >= 3
    assert any(st["churn_limit"] > c["params"]["min_per_epoch_churn_limit"] for st, c in zip(stats, cases))
    assert any(st["queue_len"] > st["n_activated"] > 0 for st in stats) and any(st["n_marked_eligible"] for st in stats)
    assert any(st["n_active"] > 60 for st in stats)
    assert any(s["total_active_balance"] > M.ETH and s["n_saturated"] and s["n_saturated"] < s["n_penalised"] for s in slash)
    assert any(0 < s["adjusted_total_slashing_balance"] < s["total_active_balance"] and s["penalties"] for s in slash)
    assert any(s["adjusted_total_slashing_balance"] == s["total_active_balance"] > M.ETH for s in slash)
    for c in cases:
        a, p = gen.from_json(c["registry"]), M.Params(**c["params"])
        for form in (M.registry_updates_sequential, M.registry_updates_numpy):
            out, st = form(a, c["current_epoch"], c["finalized_epoch"], p)
            assert st == c["stats"], c["name"]
            for k in ("elig", "act", "ext", "wdr"):
                assert [int(x) for x in out[k]] == c["after"][k], (c["name"], k)
        flags = M.view_flags(a, c["current_epoch"])
        for s in c["slashings"]:
            bal, st = M.slashings_numpy(a, flags, c["current_epoch"], s["sum_slashings"], 3, c["vector"])
            assert [int(x) for x in bal] == s["balances"] and st == s["stats"], c["name"]


def test_registry_kernels_use_no_scratch():
    """Every new kernel: no spill, no dynamic stack (the Makefile keeps the compiler's report)."""
    log = os.path.join(ROOT, "pos_evolution_amd", "csrc", "registry_kernels.resource.log")
    if not os.path.exists(log):
        pytest.skip("registry_kernels.resource.log is written by the build")
    text = open(log).read()
    for kernel in ("k_registry_census", "k_registry_scan", "k_registry_select", "k_registry_ties", "k_registry_applyILb0",
                   "k_registry_applyILb1", "k_slashings_census", "k_slashings_apply"):
        m = re.search(r"Function Name: \S*" + kernel + r"\S*(.*?)(?=Function Name:|\Z)", text, flags=re.S)
        assert m, kernel
        block = m.group(1)
        assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", block), kernel
        assert "Dynamic Stack: False" in block, kernel
