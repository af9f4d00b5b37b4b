"""An own-words model of the G1 plan that k_att_plan forms ON THE DEVICE when attestation rows are resident
(pos_evolution_amd/csrc/att_bodies.inc, "4. arrive; the last workgroup writes the plan"): one (k, L) for every group --
k members per accumulation lane, blocks of 2^L lanes, group g at lanes [g << L, (g + 1) << L) -- from the largest and the
summed size of the groups that resolved with ST_OK, the lane target and the bound of the lane-partial buffer
(engine_resident.cpp: slot_cap).  Plain Python integers; nothing here looks at a built kernel.

The plan the device actually took is never read back: the GPU tests (tests/test_gpu_g1_plan_shapes.py) INFER the branch a
shape reaches from this model, and tests/test_g1_plan_model.py pins the model's constants and comparisons to the sources'
text, so a change to the kernel's formula fails a CPU test until the model (and the shapes below) are revisited."""
import inspect
import os
import re

G1_WG = 256                  # lanes per workgroup: a group never spans workgroups in a device-formed plan
G1_MIN_K = 4                 # fewest members per lane
G1_TARGET_LANES = 131072
TARGETS = (G1_TARGET_LANES, G1_TARGET_LANES // 2)   # the lane targets an engine may run with (g1_target_slots)


def slot_cap_of(n_rows: int) -> int:
    """Lanes the lane-partial buffer is sized for: the plan's n_slots never exceeds it."""
    return max(2 * G1_TARGET_LANES, (n_rows + G1_WG - 1) // G1_WG * G1_WG)


def plan(sizes_ok, n_rows: int, target_slots: int, n_groups=None):
    """-> (k, L, n_slots, slot_cap).  sizes_ok: the sizes of the groups that resolve with ST_OK; n_groups: all groups formed,
    refused ones included (default: every group is fine)."""
    sizes_ok = [int(s) for s in sizes_ok]
    n_groups = len(sizes_ok) if n_groups is None else int(n_groups)
    max_size = max(sizes_ok, default=0)
    total_members = sum(sizes_ok)
    slot_cap = slot_cap_of(n_rows)
    min_k = G1_MIN_K
    k0 = max(min_k, (total_members + target_slots - 1) // target_slots)
    tasks = min((max_size + k0 - 1) // k0, G1_WG)
    L = 0
    while (1 << L) < tasks:
        L += 1
    while L > 0 and (n_groups << L) > slot_cap:
        L -= 1
    k = max(min_k, (max_size + (1 << L) - 1) >> L)
    if k == 0:
        k = 1
    return k, L, n_groups << L, slot_cap


# ---------------------------------------------------------------- the shapes of the GPU tests
# tag -> sizes of the attested committees in batch order (one group each), the position of the big one, the groups that
# are refused (ST_BITS_LENGTH: they form a group, their size must not shape the plan) and the (k, L) the model must yield
def _with_big(n, big_size, rest):
    sizes = [rest(i) if callable(rest) else rest for i in range(n)]
    at = n // 3                      # neither first nor last in batch order
    sizes[at] = big_size
    return sizes, at


def _shape(sizes, big, expect, refused=()):
    return dict(sizes=sizes, big=big, expect=expect, refused=tuple(refused))


def _cycle(i):
    return 1 + i % 4


SHAPES = {
    "tiny": _shape([_cycle(i) for i in range(64)], None, (4, 0)),
    "five": _shape(*_with_big(64, 5, _cycle), (4, 1)),
    "edge1024": _shape(*_with_big(1024, 1024, 4), (4, 8)),
    "over1024": _shape(*_with_big(1056, 1024, 4), (8, 7)),
    "size1025": _shape(*_with_big(64, 1025, 4), (5, 8)),
    "cap8192": _shape(*_with_big(64, 8192, 129), (32, 8)),
    "deep": _shape(*_with_big(4992, 8192, 4), (256, 5)),
    "refused_big": _shape(*_with_big(65, 4096, 4), (4, 0), refused=(65 // 3,)),
}


def shape_plan(tag: str, target_slots: int, rows_per_group: int = 1):
    s = SHAPES[tag]
    ok = [z for i, z in enumerate(s["sizes"]) if i not in s["refused"]]
    return plan(ok, rows_per_group * len(s["sizes"]), target_slots, n_groups=len(s["sizes"]))


# ---------------------------------------------------------------- what the sources say, as text
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pos_evolution_amd", "csrc")


def _text(name: str) -> str:
    with open(os.path.join(_CSRC, name)) as f:
        return f.read()


def _one(pattern: str, text: str, what: str):
    m = re.findall(pattern, text)
    assert len(m) == 1, f"{what}: expected exactly one match of {pattern!r}, found {len(m)}"
    return m[0]


def source_pins() -> dict:
    """The constants and the lines of the formula as the sources spell them (white space squeezed)."""
    kernels, internal = _text("kernels.h"), _text("engine_internal.h")
    resident, bodies = _text("engine_resident.cpp"), _text("att_bodies.inc")
    sq = lambda s: re.sub(r"\s+", " ", s).strip()
    section = bodies[bodies.index("---- 4. arrive; the last workgroup writes the plan"):]
    return dict(
        G1_WG=int(_one(r"constexpr int G1_WG = (\d+);", kernels, "G1_WG")),
        G1_MIN_K=int(_one(r"constexpr uint32_t G1_MIN_K = (\d+);", internal, "G1_MIN_K")),
        G1_TARGET_LANES=int(_one(r"constexpr uint32_t G1_TARGET_LANES = (\d+);", internal, "G1_TARGET_LANES")),
        slot_cap=sq(_one(r"const uint32_t slot_cap = ([^;]+);", resident, "slot_cap")),
        slot_cap_handed_on=sq(_one(r"pa\.slot_cap = ([^;]+);", resident, "pa.slot_cap")),
        min_k_handed_on=sq(_one(r"pa\.min_k = ([^;]+);", resident, "pa.min_k")),
        target_handed_on=sq(_one(r"pa\.target_slots = ([^;]+);", resident, "pa.target_slots")),
        targets=sorted(set(re.findall(r"return (?:h->g1_target_slots \? h->g1_target_slots : )?(G1_TARGET_LANES(?: / 2)?);",
                                      resident[resident.index("uint32_t g1_target_slots("):][:400]))),
        lanes_sized=len(re.findall(r"d_lane_partials, \(size_t\)G1_LANE_PARTIAL_BYTES \* slot_cap\)", resident)),
        k0=sq(_one(r"const unsigned long long k0 = ([^;]+);", section, "k0")),
        tasks=sq(_one(r"uint32_t tasks = ([^;]+);", section, "tasks")),
        tasks_cap=sq(_one(r"(if \(tasks > [^;]+;)", section, "the cap on tasks")),
        log2=sq(_one(r"(while \(\(1u << L\) < tasks\) \+\+L;)", section, "L from tasks")),
        clamp_cmp=_one(r"while \(L > 0 && \(\(unsigned long long\)ng << L\) (\S+) a\.slot_cap\) --L;", section, "the clamp"),
        k=sq(_one(r"\n\s+k = ([^;]+);", section, "the re-derived k")),
        n_slots=sq(_one(r"p\.n_slots = ([^;]+);", section, "n_slots")),
        sizes_ok_only=(len(re.findall(r"wave_max\(ok \? size : 0u\)", bodies)),
                       len(re.findall(r"wave_sum\(ok \? \(unsigned long long\)size : 0ull\)", bodies))),
    )


def model_pins() -> dict:
    """The same lines as this model spells them: what tests/test_g1_plan_model.py holds against source_pins()."""
    src = inspect.getsource(plan)
    return dict(
        clamp_cmp=_one(r"while L > 0 and \(n_groups << L\) (\S+) slot_cap:", src, "the model's clamp"),
        k=_one(r"\n    k = ([^\n]+)\n", src, "the model's re-derived k"),
    )
