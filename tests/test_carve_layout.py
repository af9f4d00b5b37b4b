"""carve.h: the workspace layouts of the synchronous BLS and slasher calls against the offset chains they were written with.

tests/native/carve_layout_main.cpp takes every region of the eight layouts through carve.h, in the calls' order and element
types, and prints the offsets; here the same layouts are plain arithmetic (`up256`, one term per region), as the calls had them
before carve.h.  The program is host code with its own main, built with the host compiler under AddressSanitizer and UBSan;
nothing is loaded into python.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pos_evolution_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "carve_layout_main.cpp")
KERNELS_H = open(os.path.join(CSRC, "kernels.h")).read()
PAIR_WORDS, GT_WORDS, FAN = (int(re.search(r"constexpr \w+ %s = (\d+);" % name, KERNELS_H).group(1))
                             for name in ("BLS_PAIR_WORDS", "BLS_GT_WORDS", "BLS_BATCH_FAN"))
GROUP, SLASH_ROW, SLASH_TABLE = 32, 32, 24      # sizeof G1Group, SlashRow, SlashTable (kernels.h: 8 words, 8 words, 3 pointers)
DEFAULT_CHUNK = 2                               # pe_engine::batch_chunk
NS = (0, 1, 2, 63, 64, 65)

up256 = lambda v: (v + 255) & ~255


def chain(*regions):
    """[(name, bytes as the chain adds them)] -> ({name: offset}, total): o_next = o_this + bytes."""
    offs, o = {}, 0
    for name, size in regions:
        offs[name] = o
        o += size
    return offs, o


def pairing(n_pairs, ng, out576):
    rows = max(1, n_pairs)
    return chain(("g1", up256(96 * rows)), ("g2", up256(192 * rows)), ("off", up256(4 * (ng + 1))),
                 ("ws", up256(4 * PAIR_WORDS * rows)), ("flag", up256(4 * rows)), ("gt", up256(4 * GT_WORDS * ng)),
                 ("bad", up256(4 * ng)), ("verdict", up256(4 * ng)), ("out", up256(576 * ng) if out576 else 0))


def batch(n, c, fan):
    max_chunks = (n + c - 1) // c
    rows, lvl = n + max_chunks, (max_chunks + fan - 1) // fan
    return chain(("pk", up256(96 * n)), ("msg", up256(192 * n)), ("sig", up256(192 * n)), ("scal", up256(8 * n)), ("neg", 256),
                 ("status", up256(4 * n)), ("pkm", up256(96 * n)), ("msgm", up256(192 * n)), ("sigm", up256(192 * n)),
                 ("live", up256(4 * n)), ("scaled", up256(384 * n)), ("ws", up256(4 * PAIR_WORDS * rows)), ("flag", up256(4 * rows)),
                 ("off", up256(4 * (max_chunks + 1))), ("gt", up256(4 * GT_WORDS * max_chunks)), ("lvl0", up256(4 * GT_WORDS * lvl)),
                 ("lvl1", up256(4 * GT_WORDS * lvl)), ("bad", up256(4 * max_chunks)), ("zero", 256),
                 ("verdict", up256(4 * max_chunks)), ("out", up256(576)))


def sums(total, ng, partials2, partials1):
    gbytes = GROUP * ng
    return chain(("index", up256(4 * total)), ("signer", up256(4 * total)), ("scal", up256(8 * total)), ("gr2", up256(gbytes)),
                 ("gr1", up256(gbytes)), ("part2", up256(384 * partials2)), ("part1", up256(192 * partials1)),
                 ("pk", up256(96 * ng)), ("sig", up256(192 * ng)))


def locate(n_again):
    return chain(("rows", up256(8 * n_again)), ("be96", up256(96 * n_again)), ("be192", up256(192 * n_again)))


def aggregate(kept, ng, partials):
    return chain(("keep", up256(4 * kept)), ("g", up256(GROUP * ng)), ("part", up256(384 * partials)), ("out", up256(192 * ng)))


def resident(ng, n_in, n_points, por, in_place):
    offs, total = chain(("head", 256), ("por", up256(4 * n_in if por else 0)), ("msg", up256(0 if in_place else 192 * n_points)),
                        ("off", up256(4 * (ng + 1))), ("ws", up256(4 * PAIR_WORDS * 2 * ng)), ("flag", up256(8 * ng)),
                        ("gt", up256(4 * GT_WORDS * ng)), ("gbad", up256(4 * ng)), ("fe", up256(4 * ng)), ("ident", up256(4 * ng)),
                        ("sub", up256(4 * ng)), ("out", 64 + 4 * ng))    # counters | verdicts: not rounded
    offs["verdict"] = offs["out"] + 64
    return offs, total


def res_points(n):
    rows = max(n, 1)
    return chain(("pk", up256(192 * rows)), ("sig", up256(192 * rows)), ("bad", up256(4 * rows)))


def slash_rows(ng, cand, n_keys):
    return chain(*((name, up256(size)) for name, size in (
        ("err", 16), ("status", 4 * ng), ("cslot", 4 * ng), ("id", 4 * ng), ("rows", SLASH_ROW * ng), ("cand", 4 * cand),
        ("cnt", 4 * n_keys), ("start", 4 * n_keys), ("cursor", 4 * n_keys), ("list", 4 * ng), ("tabs", 2 * SLASH_TABLE))))


def cases():
    """[(the program's input line, the chain's answer)]"""
    out = []
    for n in NS:
        for out576 in (0, 1):
            out.append(("pairing %d %d %d" % (2 * n, n, out576), pairing(2 * n, n, out576)))
            out.append(("pairing 0 %d %d" % (n, out576), pairing(0, n, out576)))        # groups without pairs
        out.append(("pairing %d 1 0" % n, pairing(n, 1, 0)))
        for c in (1, DEFAULT_CHUNK):
            out.append(("batch %d %d %d" % (n, c, FAN), batch(n, c, FAN)))
        for ng in (1, 3):
            out.append(("sums %d %d %d %d" % (n, ng, n + ng, n // 2 + ng), sums(n, ng, n + ng, n // 2 + ng)))
            out.append(("aggregate %d %d %d" % (n, ng, n // 4 + 1), aggregate(n, ng, n // 4 + 1)))
        out.append(("sums 0 %d 0 0" % n, sums(0, n, 0, 0)))
        out.append(("locate %d" % n, locate(n)))
        for por in (0, 1):
            for in_place in (0, 1):
                args = (max(n, 1), 2 * n + 1, n + 3, por, in_place)
                out.append(("resident %d %d %d %d %d" % args, resident(*args)))
        out.append(("res_points %d" % n, res_points(n)))
        cand = 64
        while cand < 2 * n:
            cand <<= 1
        for n_keys in (1, 65):
            out.append(("slash_rows %d %d %d" % (n, cand, n_keys), slash_rows(n, cand, n_keys)))
    return out


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("carve") / "carve_layout"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, SRC, "-o", str(exe)])

    def run(text):
        out = subprocess.run([str(exe)] + [str(v) for v in (PAIR_WORDS, GT_WORDS, GROUP, SLASH_ROW, SLASH_TABLE)], input=text,
                             capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        return out.stdout.splitlines()
    return run


def test_every_layout_equals_its_chain(program):
    todo = cases()
    assert len({line.split()[0] for line, _ in todo}) == 8
    lines = program("\n".join(line for line, _ in todo) + "\n")
    assert len(lines) == len(todo) + 2
    for (line, (offs, total)), got in zip(todo, lines):
        fields = got.split()
        assert fields[0] == line.split()[0]
        got_offs = {k: int(v) for k, v in (f.split("=") for f in fields[1:])}
        assert got_offs.pop("total") == total, (line, got)
        assert got_offs == offs, (line, got)
        assert all(v % 256 == 0 for k, v in got_offs.items() if k not in ("por", "verdict")), got   # (parts of a block)


def test_a_zero_count_region_shares_its_offset_with_its_successor(program):
    lines = program("pairing 4 2 0\nresident 3 5 4 0 1\n")
    out = dict(f.split("=") for f in lines[0].split()[1:])
    assert out["out"] == out["total"]                              # no out576: the region is empty and the total ends there
    res = dict(f.split("=") for f in lines[1].split()[1:])
    assert res["msg"] == res["off"]                                # message points read in place
    assert lines[2] == "zero_count empty=256 next=256"


def test_a_transfer_of_one_element_more_is_refused(program):
    assert program("")[-1] == "holds count=1 count_plus_1=0 empty_0=1 empty_1=0"


def test_the_calls_take_their_regions_through_carve_h():
    """No offset chain, no cast of base + offset left in the units that moved; the header stays free of HIP."""
    for unit in ("engine_bls.cpp", "engine_batch.cpp", "engine_sigverify.cpp", "engine_resident_verify.cpp", "engine_slash.cpp"):
        text = open(os.path.join(CSRC, unit)).read()
        assert "up256" not in text and "Layout" in text and ".bind(" in text, unit
        assert not re.search(r"reinterpret_cast<[^>]*>\(\s*\w+\s*\+\s*o_", text), unit
    internal = open(os.path.join(CSRC, "engine_internal.h")).read()
    assert "up256" not in internal and '#include "carve.h"' in internal
    assert not re.search(r"#include\s*[<\"](hip|engine_internal|kernels)", open(os.path.join(CSRC, "carve.h")).read())
    assert re.search(r"^engine_%\.o:.*\bcarve\.h\b", open(os.path.join(CSRC, "Makefile")).read(), re.M)
