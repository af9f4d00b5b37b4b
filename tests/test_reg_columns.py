"""reg_columns.h: the registry's per-validator columns against the formulas their call sites were written with.

tests/native/reg_columns_main.cpp prints the header's table and answers reg_rows / reg_column_bytes / reg_grown_capacity; here
the sizes every site asked for before there was a table are plain arithmetic, and registry_grow's list of columns stands
literally.  The program is host code with its own main, built with the host compiler under AddressSanitizer and UBSan; nothing
is loaded into python.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pos_evolution_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "reg_columns_main.cpp")
NS = (0, 1, 3, 4, 5, 63, 64, 65, 2**20 + 1, 2**32 - 2)
POINT = 128      # 4 * G1_ROW_WORDS (kernels.h)

n4 = lambda n: (n + 3) & ~3  # noqa: E731

# registry_grow's list as it stood: name -> (element size, the byte a new row takes; -1: the caller writes the rows)
GROW_LIST = {
    "d_sbalance": (8, -1), "d_sflags": (1, -1), "d_incr": (2, -1),
    "d_activation_epoch": (8, -1), "d_exit_epoch": (8, -1), "d_activation_eligibility": (8, -1),
    "d_withdrawable": (8, -1), "d_pubkey_leaf": (32, -1), "d_withdrawal_credentials": (32, -1),
    "d_rbalance": (8, 0), "d_inactivity": (8, 0), "d_part_cur": (1, 0),
    "d_part_prev": (1, 0), "d_balance": (8, 0), "d_flags": (1, 0),
    "d_vote_key": (8, 0), "d_vote_block": (4, 0xFF), "d_vote_slot": (4, 0),
    "d_points": (POINT, -1), "d_points30": (POINT, -1),
}
# what the other sites asked for, per column: [formula(elem, n)].  Every column also had registry_grow's max(64, elem * cap) at a
# capacity that is a multiple of four; the least such capacity that holds n validators is n4(n).
PADDED = lambda e, n: max(64, e * n4(n))  # noqa: E731  ensure_validator_arrays, upload_balances, pe_set_validators, the view's sites
PLAIN = lambda e, n: max(64, e * n)       # noqa: E731  pe_registry_set_epochs, pe_state_set_balances, pe_registry_set_static
SITES = {name: [PADDED] for name in ("d_balance", "d_flags", "d_incr", "d_sbalance", "d_sflags", "d_vote_key", "d_vote_block",
                                     "d_vote_slot", "d_part_cur", "d_part_prev")}
SITES.update({name: [PADDED, PLAIN] for name in ("d_activation_epoch", "d_exit_epoch", "d_rbalance", "d_inactivity", "d_withdrawable",
                                                 "d_pubkey_leaf", "d_withdrawal_credentials", "d_activation_eligibility")})
SITES["d_points"] = [PADDED, lambda e, n: e * n]                # pe_set_validators, pe_set_pubkeys_compressed: no floor
SITES["d_points30"] = [PADDED, lambda e, n: max(128, e * n)]    # build_points30
GROUP_NAMES = ("justified", "votes", "vote slot", "participation", "view", "epochs", "balances", "static", "points", "points30")


def old_capacity(capacity, n_old, n_new):
    """registry_grow's three lines."""
    cap = max(capacity, n_old)
    if n_new > capacity:
        cap = max(n_new, 2 * cap)
    return min((cap + 3) & ~3, 0x100000000)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("reg_columns") / "reg_columns"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, SRC, "-o", str(exe)])

    def run(lines):
        out = subprocess.run([str(exe)], input="".join(line + "\n" for line in lines), capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        rows = out.stdout.splitlines()
        head = [r.split() for r in rows if r.startswith(("column ", "groups "))]
        table = {f[1]: (int(f[2]), int(f[3]), int(f[4])) for f in head if f[0] == "column"}
        assert len(table) == sum(f[0] == "column" for f in head), "a name twice"
        return table, int(head[-1][1]), [int(r) for r in rows[len(head):]]
    return run


def test_the_table_is_the_list_registry_grow_had(program):
    table, all_groups, _ = program([])
    assert {name: (elem, fill) for name, (elem, _, fill) in table.items()} == GROW_LIST and len(table) == 20
    groups = {}
    for name, (_, group, _) in table.items():
        assert group and group & (group - 1) == 0 and group & all_groups, name       # one bit each
        groups.setdefault(group, []).append(name)
    assert sorted(groups) == [1 << k for k in range(len(GROUP_NAMES))] and all_groups == (1 << len(GROUP_NAMES)) - 1
    by_name = dict(zip(GROUP_NAMES, (groups[1 << k] for k in range(len(GROUP_NAMES)))))
    assert by_name == {"justified": ["d_balance", "d_flags"], "votes": ["d_vote_key", "d_vote_block"], "vote slot": ["d_vote_slot"],
                       "participation": ["d_part_cur", "d_part_prev"], "view": ["d_sbalance", "d_sflags", "d_incr"],
                       "epochs": ["d_activation_epoch", "d_exit_epoch"], "balances": ["d_rbalance", "d_inactivity", "d_withdrawable"],
                       "static": ["d_pubkey_leaf", "d_withdrawal_credentials", "d_activation_eligibility"],
                       "points": ["d_points"], "points30": ["d_points30"]}


def test_no_column_is_smaller_than_any_site_asked_for(program):
    assert set(SITES) == set(GROW_LIST)
    asks = [(name, n) for name in SITES for n in NS]
    _, _, got = program(["rows %d" % n for n in NS] + ["bytes %d %d" % (GROW_LIST[name][0], n) for name, n in asks])
    assert got[:len(NS)] == [n4(n) for n in NS]
    for (name, n), bytes_ in zip(asks, got[len(NS):]):
        elem = GROW_LIST[name][0]
        for formula in SITES[name]:
            assert bytes_ >= formula(elem, n), (name, n, bytes_)
        if SITES[name] == [PADDED]:
            assert bytes_ == max(64, elem * n4(n)), (name, n, bytes_)
        assert bytes_ % 4 == 0 and bytes_ >= elem * n4(n)           # whole padded rows: a fill through reg_rows(n) stays inside


def test_the_capacity_rule_is_registry_grows(program):
    top = 2**32
    caps = (0, 1, 3, 4, 5, 64, 100, 2**20, 2**31 - 4, 2**31, top - 8, top - 4)
    grid = set()
    for capacity in caps:
        for n_new in (1, capacity, capacity + 1, 2 * capacity + 1, 2 * capacity + 5, top - 5, top - 4, top - 3, top - 2):
            if not 0 < n_new <= top - 2:
                continue
            for n_old in (0, 1, capacity // 2, max(capacity - 1, 0), capacity, capacity + 3, n_new - 1):   # (a stale capacity too)
                if 0 <= n_old < n_new:
                    grid.add((capacity, n_old, n_new))
    grid = sorted(grid)
    assert len(grid) > 200
    _, _, got = program(["cap %d %d %d" % point for point in grid])
    for point, cap in zip(grid, got):
        assert cap == old_capacity(*point), point
        assert cap >= point[2] and cap % 4 == 0 and cap <= top, point


def test_the_sites_size_their_columns_through_the_table():
    members = "|".join(GROW_LIST)
    for unit in ("engine_store.cpp", "engine_epoch.cpp", "engine_ssz.cpp", "engine_deposit.cpp", "engine_g1.cpp"):
        text = open(os.path.join(CSRC, unit)).read()
        assert not re.search(r"\b(%s)\s*\.\s*ensure\s*\(" % members, text), unit
    assert "struct Column" not in open(os.path.join(CSRC, "engine_deposit.cpp")).read()
    header = open(os.path.join(CSRC, "reg_columns.h")).read()
    assert set(re.findall(r"#include\s*[<\"]([^>\"]+)[>\"]", header)) == {"stdint.h", "cstddef"}
    assert '#include "reg_columns.h"' in open(os.path.join(CSRC, "engine_internal.h")).read()
    assert re.search(r"^engine_%\.o:.*\breg_columns\.h\b", open(os.path.join(CSRC, "Makefile")).read(), re.M)
