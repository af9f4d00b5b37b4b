"""CPU: the model of the device-formed G1 plan (tests/g1_plan_model.py) is pinned to the text of the sources it models,
and every shape of tests/test_gpu_g1_plan_shapes.py is shown to reach the branch it is there for -- under BOTH lane targets
an engine may run with -- so that no GPU test can silently miss its branch.  The (k, L) a device took is never read back:
it is inferred from this formula, which is why the formula is pinned."""
import numpy as np
import pytest

from oracle import g1
from tests import g1_plan_model as M
from tests import helpers as H


# ---------------------------------------------------------------- the sources say what the model says
def test_the_constants_are_the_sources():
    pins = M.source_pins()
    assert pins["G1_WG"] == M.G1_WG
    assert pins["G1_MIN_K"] == M.G1_MIN_K
    assert pins["G1_TARGET_LANES"] == M.G1_TARGET_LANES
    assert pins["targets"] == ["G1_TARGET_LANES", "G1_TARGET_LANES / 2"]
    assert M.TARGETS == (M.G1_TARGET_LANES, M.G1_TARGET_LANES // 2)


def test_the_host_sizing_is_the_models():
    pins = M.source_pins()
    assert pins["slot_cap"] == "std::max<uint32_t>(2 * G1_TARGET_LANES, (n + G1_WG - 1) / G1_WG * G1_WG)"
    assert pins["slot_cap_handed_on"] == "slot_cap" and pins["min_k_handed_on"] == "G1_MIN_K"
    assert pins["target_handed_on"] == "target"
    assert pins["lanes_sized"] == 2, "both lane-partial buffers (the arenas' and the engine's) are sized by slot_cap"
    for n in (0, 1, 255, 256, 257, 4992, 262144, 262145, 300000):
        assert M.slot_cap_of(n) == max(2 * 131072, -(-n // 256) * 256)


def test_the_formula_is_the_kernels():
    pins, own = M.source_pins(), M.model_pins()
    assert pins["k0"] == "max((unsigned long long)a.min_k, (total_members + a.target_slots - 1) / a.target_slots)"
    assert pins["tasks"] == "(uint32_t)((max_size + k0 - 1) / k0)"
    assert pins["tasks_cap"] == "if (tasks > (uint32_t)G1_WG) tasks = G1_WG;"
    assert pins["log2"] == "while ((1u << L) < tasks) ++L;"
    assert pins["clamp_cmp"] == own["clamp_cmp"] == ">"
    assert pins["k"] == "max(a.min_k, (max_size + (1u << L) - 1) >> L)"
    assert own["k"] == "max(min_k, (max_size + (1 << L) - 1) >> L)"
    assert pins["n_slots"] == "p.n_groups << L"
    assert pins["sizes_ok_only"] == (1, 1), "max_size and total_members count the groups with st == ST_OK only"


# ---------------------------------------------------------------- every shape reaches its branch, whatever the lane target
@pytest.mark.parametrize("target", M.TARGETS)
@pytest.mark.parametrize("tag", sorted(M.SHAPES))
def test_each_shape_yields_its_k_and_L(tag, target):
    s = M.SHAPES[tag]
    ok = [z for i, z in enumerate(s["sizes"]) if i not in s["refused"]]
    assert sum(ok) <= 4 * 65536, "k0 must stay min_k under both targets"
    k, L, n_slots, slot_cap = M.shape_plan(tag, target)
    assert (k, L) == s["expect"]
    assert n_slots == len(s["sizes"]) << L <= slot_cap
    big = max(ok)
    assert ((big + k - 1) // k) <= (1 << L) <= M.G1_WG, "the largest group's tasks fit its block; a block fits a workgroup"
    assert len(s["sizes"]) % 32 == 0 or tag == "refused_big"


def test_the_shapes_are_what_they_are_there_for():
    S = M.SHAPES
    T = M.TARGETS[0]
    assert sorted(set(S["tiny"]["sizes"])) == [1, 2, 3, 4] and len(S["tiny"]["sizes"]) == 64
    assert sorted(set(S["five"]["sizes"])) == [1, 2, 3, 4, 5] and S["five"]["sizes"].count(5) == 1
    for tag, n, big, rest in (("edge1024", 1024, 1024, 4), ("over1024", 1056, 1024, 4), ("size1025", 64, 1025, 4),
                              ("cap8192", 64, 8192, 129), ("deep", 4992, 8192, 4), ("refused_big", 65, 4096, 4)):
        sizes, at = S[tag]["sizes"], S[tag]["big"]
        assert len(sizes) == n and sizes[at] == big and 0 < at < n - 1
        assert sizes.count(rest) == n - 1
    assert S["refused_big"]["refused"] == (S["refused_big"]["big"],)
    # edge1024: the clamp's boundary from the passing side -- the partial buffer filled to its last lane; doubled rows keep it
    assert M.shape_plan("edge1024", T)[2:] == (262144, 262144)
    assert M.shape_plan("edge1024", T, rows_per_group=2) == M.shape_plan("edge1024", T)
    # over1024: one step of the clamp, k re-derived; deep: three steps (L = 8 without the clamp in both)
    unclamped = lambda tag: M.plan(S[tag]["sizes"], 0, T, n_groups=1)[1]
    assert unclamped("over1024") - S["over1024"]["expect"][1] == 1
    assert unclamped("deep") - S["deep"]["expect"][1] == 3
    # size1025 / cap8192: tasks beyond a workgroup's lanes are capped (257 -> 256, 2048 -> 256); k says so
    assert -(-1025 // M.G1_MIN_K) == 257 and S["size1025"]["expect"] == (5, 8)
    assert -(-8192 // M.G1_MIN_K) == 2048 and S["cap8192"]["expect"] == (32, 8)
    # refused_big: with the refused group's 4096 the plan would be another one
    assert M.plan(S["refused_big"]["sizes"], 65, T)[:2] == (16, 8)


def test_the_clamp_and_the_cap_at_their_edges():
    T = M.TARGETS[0]
    cap = M.slot_cap_of(0)
    for ng, L in ((cap >> 8, 8), ((cap >> 8) + 1, 7), (cap >> 7, 7), ((cap >> 7) + 1, 6), (cap, 0), (cap + 1, 0)):
        k, l, n_slots, sc = M.plan([1024] + [4] * (ng - 1), ng, T)
        assert l == L and k == max(4, 1024 >> L) and (n_slots <= sc or L == 0)
    assert M.plan([], 0, T) == (4, 0, 0, cap)
    assert M.plan([1], 1, T) == (4, 0, 1, cap)
    assert M.plan([4 * 256], 1, T)[:2] == (4, 8) and M.plan([4 * 256 + 1], 1, T)[:2] == (5, 8)
    # a batch of more rows than 2 * G1_TARGET_LANES widens the buffer with it
    assert M.plan([1024] + [4] * 1024, 1025 * 256, T) == (4, 8, 1025 * 256, 1025 * 256)


# ---------------------------------------------------------------- the batched closed form the GPU tests compare with
def test_closed_form_sums_is_closed_form_sum():
    a, b = 0x1234567, 0x89ABCDE
    sets = [[], [0], [7], [3, 9, 20000], list(range(0, 28000, 7)), np.arange(8192, dtype=np.uint32) * 3 + 1]
    got = H.closed_form_sums(sets, a, b)
    assert [bytes(x) for x in got] == [H.closed_form_sum(s, a, b) for s in sets]
    assert got[0] == g1.to_bytes96(None)
    pts = [g1.add(g1.mul(a, g1.G), g1.mul(i * b, g1.G)) for i in sets[3]]
    assert got[3] == g1.to_bytes96(g1.sum_points(pts))
