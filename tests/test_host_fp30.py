"""CPU: the S30 field form (pos_evolution_amd/csrc/fp381_s30.h: 13 signed limbs of 30 bits, lazy Montgomery with R = 2^390,
every product factor a balanced digit) and the XYZZ accumulation / tree adds over it (g1_s30.h), compiled for the HOST from
the very source the gfx950 kernels use (tests/native/fp30_host.cpp) and held against Python integers and oracle/g1.py.
A second build runs the products with a checked 128-bit column accumulator: no column may leave the int64 range."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from oracle import g1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = g1.P
B, N = 30, 13
MASK = (1 << B) - 1
R = 1 << (B * N)
R32 = 1 << 384
HALF = 1 << (B - 1)
# the operand bounds fp381_s30.h documents for fq_mul / fq_sqr
OP_LIMB = HALF + 16        # limbs 0..11
OP_TOP = 1 << 24           # the top limb


def _build(tmp_path_factory, name, extra):
    out = tmp_path_factory.mktemp(name) / f"lib{name}.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-shared",
                           "-fPIC", *extra, os.path.join(ROOT, "tests", "native", "fp30_host.cpp"), "-o", str(out)])
    return C.CDLL(str(out))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return _build(tmp_path_factory, "fp30", [])


@pytest.fixture(scope="module")
def checked(tmp_path_factory):
    return _build(tmp_path_factory, "fp30chk", ["-DFP30_COLUMN_CHECK"])


def carried(v):
    out = []
    for _ in range(N - 1):
        out.append(v & MASK)
        v >>= B
    out.append(v)
    return np.array(out, dtype=np.int32)


def balanced(v):
    out = []
    for _ in range(N - 1):
        d = ((v & MASK) ^ HALF) - HALF
        out.append(d)
        v = (v - d) >> B
    out.append(v)
    return np.array(out, dtype=np.int32)


def value_of(l):
    return sum(int(x) << (B * i) for i, x in enumerate(l))


def rand_operand(rng, top=1 << 22):
    """Random product operand at the documented limb bounds: limbs 0..11 anywhere in [-(2^29 + 16), 2^29 + 16]."""
    return np.array([rng.randrange(-OP_LIMB, OP_LIMB + 1) for _ in range(N - 1)] + [rng.randrange(-top, top + 1)],
                    dtype=np.int32)


def mixed(rng, v):
    """v with limbs of both forms: balanced digits, some of them turned into carried ones (d < 0 -> d + 2^30, one less in
    the next limb) -- what the exact reductions accept (|limb| <= 2^30 + 8)."""
    l = [int(x) for x in balanced(v)]
    for i in range(N - 1):
        if l[i] < 0 and rng.random() < 0.5:
            l[i] += 1 << B
            l[i + 1] -= 1
    assert value_of(l) == v
    return np.array(l, dtype=np.int32)


def ptr(a, t=C.c_int32):
    return a.ctypes.data_as(C.POINTER(t))


def _check_product(r_limbs, a, b):
    """r = a b / R mod p, with the lazy bound of a signed Montgomery digit string: r R = a b + m p, |m| <= 2^29 (R-1)/(2^30-1)."""
    r = value_of(r_limbs)
    num = r * R - a * b
    assert num % P == 0
    m = num // P
    assert abs(m) <= HALF * (R - 1) // (MASK) + 1, (m, R)
    assert abs(r - a * b / R) < P / 2 * (1 + 2.0 ** -29) + 1
    assert all(-HALF <= int(x) < HALF for x in r_limbs[:-1])                  # exact balanced digits
    return r


def test_product_and_square_against_python_integers(lib):
    rng = random.Random(30)
    out = np.zeros(N, dtype=np.int32)
    cases = [(0, 0), (1, 1), (P - 1, P - 1), (-(P - 1), P - 1), (3 * P - 3, -3 * P + 11)]
    for _ in range(3000):
        cases.append((rng.randrange(-4 * P, 4 * P), rng.randrange(-4 * P, 4 * P)))
    for a, b in cases:
        ra, rb = rand_operand(rng), rand_operand(rng)
        for la, lb in ((balanced(a), balanced(b)), (ra, rb), (balanced(a), rb)):
            lib.fq30_mul(ptr(la), ptr(lb), ptr(out))
            r = _check_product(out, value_of(la), value_of(lb))
            assert abs(r) < 0.55 * P and abs(int(out[-1])) < (1 << 21)
        for la in (balanced(a), ra):
            lib.fq30_sqr(ptr(la), ptr(out))
            _check_product(out, value_of(la), value_of(la))


def _adversarial_operands(rng):
    """Every limb at +-(2^29 + 16), the top limb at +-2^24: all-equal signs, alternating signs, and random sign patterns."""
    pats = [[1] * N, [-1] * N, [(-1) ** i for i in range(N)], [-((-1) ** i) for i in range(N)]]
    pats += [[rng.choice((1, -1)) for _ in range(N)] for _ in range(60)]
    ops = []
    for s in pats:
        l = np.array([s[i] * OP_LIMB for i in range(N - 1)] + [s[-1] * OP_TOP], dtype=np.int32)
        ops.append(l)
        l2 = l.copy()
        l2[-1] = rng.randrange(-OP_TOP, OP_TOP + 1)
        ops.append(l2)
    return ops


@pytest.mark.parametrize("which", ["plain", "checked"])
def test_adversarial_limbs(lib, checked, which):
    """Operands at the documented bounds: the product must stay exact (a wrapped 64-bit column breaks the congruence), and
    in the checked build no column value may leave the int64 range."""
    L = lib if which == "plain" else checked
    rng = random.Random(7)
    out = np.zeros(N, dtype=np.int32)
    w = C.c_double(0)
    if which == "checked":
        L.fq30_column_report(C.byref(w), 1)
    ops = _adversarial_operands(rng)
    for i, la in enumerate(ops):
        for lb in (ops[(i * 7 + 3) % len(ops)], ops[(i * 13 + 1) % len(ops)], la):
            a, b = value_of(la), value_of(lb)
            L.fq30_mul(ptr(la), ptr(lb), ptr(out))
            _check_product(out, a, b)
        L.fq30_sqr(ptr(la), ptr(out))
        _check_product(out, value_of(la), value_of(la))
    if which == "checked":
        n = L.fq30_column_report(C.byref(w), 1)
        assert n == 0, f"{n} column values left the int64 range"
        assert 61 <= w.value < 63, w.value          # the a b half of a column alone reaches ~11 x 2^58 here


def test_column_bound_from_the_documented_limb_bounds():
    """Each column's worst case, derived from the limb bounds fp381_s30.h documents (operands: limbs 0..11 |l| <= 2^29 + 16,
    top |l| <= 2^24; m digits |m| <= 2^29; p's balanced limbs as generated), plus the carry from the column below, stays
    below 2^63 -- for the product and for the squaring (doubled cross products)."""
    pl = [int(x) for x in balanced(P)]
    ab = [OP_LIMB] * (N - 1) + [OP_TOP]
    m = HALF
    worst = 0
    for sq in (False, True):
        carry = 0
        for k in range(2 * N - 1):
            lo = max(0, k - (N - 1))
            if not sq:
                col = sum(ab[i] * ab[k - i] for i in range(lo, min(k, N - 1) + 1))
            else:
                col = sum(2 * ab[i] * ab[k - i] for i in range(lo, min(k, N - 1) + 1) if 2 * i < k)
                if k % 2 == 0:
                    col += ab[k // 2] ** 2
            col += sum(m * abs(pl[k - i]) for i in range(lo, min(k, N - 1) + 1))
            total = col + carry
            assert total < 1 << 63, (sq, k, total.bit_length())
            worst = max(worst, total)
            carry = (total >> B) + 1
    assert worst.bit_length() == 63          # 23 full terms: about 2^62.6


def test_carry_pass_combinations_canonical_forms_and_the_zero_test(lib):
    rng = random.Random(5)
    out = np.zeros(N, dtype=np.int32)
    filt = C.c_int(0)
    for _ in range(2000):
        l = np.array([rng.randrange(-(1 << 31), 1 << 31) for _ in range(N - 1)] + [rng.randrange(-50, 50)], dtype=np.int32)
        lib.fq30_norm(ptr(l), ptr(out))
        assert value_of(out) == value_of(l) and all(abs(int(x)) <= HALF + 2 for x in out[:-1])
        # the shapes of the formulas: a - b (normed / product values), a - b - 2c (three product outputs), a + b
        prods = [np.array([rng.choice((-HALF, HALF - 1, rng.randrange(-HALF, HALF))) for _ in range(N - 1)]
                          + [rng.randrange(-(1 << 20), 1 << 20)], dtype=np.int32) for _ in range(3)]
        a, b, c = prods
        for shape, want in ((0, value_of(a) - value_of(b)), (1, value_of(a) - value_of(b) - 2 * value_of(c)),
                            (2, value_of(a) + value_of(b))):
            lib.fq30_combine(ptr(a), ptr(b), ptr(c), shape, ptr(out))
            assert value_of(out) == want and all(abs(int(x)) <= HALF + 2 for x in out[:-1])
        v = rng.randrange(-7 * P, 8 * P)
        lv = mixed(rng, v)
        lib.fq30_canonical(ptr(lv), ptr(out), 0)
        assert np.array_equal(out, carried(v % P))
        w = rng.randrange(-P + 1, 2 * P)
        lib.fq30_canonical(ptr(mixed(rng, w)), ptr(out), 1)
        assert np.array_equal(out, carried(w % P))
        assert lib.fq30_is_zero_modp(ptr(lv), C.byref(filt)) == (1 if v % P == 0 else 0)
    # the extreme sums a - b - 2c of product outputs stay inside int32
    lo = np.array([-HALF] * (N - 1) + [0], dtype=np.int32)
    hi = np.array([HALF - 1] * (N - 1) + [0], dtype=np.int32)
    for a, b, c in ((hi, lo, lo), (lo, hi, hi)):
        lib.fq30_combine(ptr(a), ptr(b), ptr(c), 1, ptr(out))
        assert value_of(out) == value_of(a) - value_of(b) - 2 * value_of(c)
    for k in range(-8, 9):                       # every multiple of p the tests recognise
        for rep in (balanced(k * P), carried(k * P), mixed(rng, k * P)):
            assert lib.fq30_is_zero_modp(ptr(rep), C.byref(filt)) == 1 and filt.value == 1
        assert lib.fq30_is_zero_modp(ptr(mixed(rng, k * P + 1)), C.byref(filt)) == 0
    v = 3 * P + (1 << B) * 12345                 # same low 30 bits as 3p, not a multiple of p: the filter passes it
    assert lib.fq30_is_zero_modp(ptr(balanced(v)), C.byref(filt)) == 0 and filt.value == 1


def test_hand_over_between_the_two_montgomery_forms(lib):
    rng = random.Random(11)
    w = np.zeros(12, dtype=np.uint32)
    back = np.zeros(12, dtype=np.uint32)
    out = np.zeros(N, dtype=np.int32)
    for x in [0, 1, P - 1] + [rng.randrange(P) for _ in range(500)]:
        m32 = x * R32 % P
        w[:] = [(m32 >> (32 * j)) & 0xFFFFFFFF for j in range(12)]
        lib.fq30_words(ptr(w, C.c_uint32), ptr(out), ptr(back, C.c_uint32))
        assert value_of(out) == m32 and np.array_equal(back, w)          # pure re-packing, both ways
        lib.fq30_from_mont32(ptr(w, C.c_uint32), ptr(out))
        assert np.array_equal(out, balanced(x * R % P))                  # x 2^384 -> x R: balanced digits of the residue
        lib.fq30_to_mont32(ptr(balanced(x * R % P + rng.randrange(-3, 4) * P)), ptr(back, C.c_uint32))
        assert np.array_equal(back, w)                                   # and back, from a lazy value
        op = rand_operand(rng)                                           # ... and from any product operand
        lib.fq30_to_mont32(ptr(op), ptr(back, C.c_uint32))
        want = value_of(op) * pow(R, -1, P) * R32 % P
        assert sum(int(back[j]) << (32 * j) for j in range(12)) == want


def _row(pt):
    if pt is None:
        return [0] * 24
    out = []
    for c in pt:
        m = c * R32 % P
        out += [(m >> (32 * j)) & 0xFFFFFFFF for j in range(12)]
    return out


def _point_of(words48):
    vals = [sum(int(words48[12 * c + j]) << (32 * j) for j in range(12)) for c in range(4)]
    assert all(v < P for v in vals)
    x, y, zz, zzz = vals
    if zz == 0:
        return None
    inv = pow(R32, -1, P)
    x, y, zz, zzz = (v * inv % P for v in (x, y, zz, zzz))
    assert pow(zz, 3, P) == pow(zzz, 2, P)
    return (x * pow(zz, -1, P) % P, y * pow(zzz, -1, P) % P)


def _worst_ok(worst):
    # limbs: balanced digits plus a carry pass's slack; top limbs: values within a few p
    assert worst[0] <= HALF + 2 and worst[1] < 1 << 23, list(worst)


def _run(lib, pts):
    rows = np.array([w for pt in pts for w in _row(pt)], dtype=np.uint32) if pts else np.zeros(24, dtype=np.uint32)
    out = np.zeros(48, dtype=np.uint32)
    worst = np.zeros(2, dtype=np.int32)
    lib.g1q30_run(ptr(rows, C.c_uint32), len(pts), ptr(out, C.c_uint32), ptr(worst))
    _worst_ok(worst)
    return _point_of(out)


def _run_kernel_way(lib, pts):
    rows = np.array([w for pt in pts for w in _row(pt)], dtype=np.uint32) if pts else np.zeros(24, dtype=np.uint32)
    out = np.zeros(48, dtype=np.uint32)
    worst = np.zeros(2, dtype=np.int32)
    slow = C.c_int(0)
    lib.g1q30_run_kernel_way(ptr(rows, C.c_uint32), len(pts), ptr(out, C.c_uint32), ptr(worst), C.byref(slow))
    _worst_ok(worst)
    return _point_of(out), bool(slow.value)


def _run_tree(lib, pts, k):
    rows = np.array([w for pt in pts for w in _row(pt)], dtype=np.uint32) if pts else np.zeros(24, dtype=np.uint32)
    out = np.zeros(48, dtype=np.uint32)
    worst = np.zeros(2, dtype=np.int32)
    lib.g1q30_tree_run(ptr(rows, C.c_uint32), len(pts), k, ptr(out, C.c_uint32), ptr(worst))
    _worst_ok(worst)
    return _point_of(out)


@pytest.mark.parametrize("which", ["plain", "checked"])
def test_madd_fast_chains_and_the_rare_paths(lib, checked, which):
    """k_g1_accumulate's lane logic over S30: first point taken as it is, the general body for every add, same-x cases
    detected and the run redone by the complete add (P + P, P + (-P), infinity in the middle).  The checked build runs the
    same chains with every column recomputed in 128 bits."""
    L = lib if which == "plain" else checked
    w = C.c_double(0)
    if which == "checked":
        L.fq30_column_report(C.byref(w), 1)
    rng = random.Random(31)
    base = [g1.mul(rng.randrange(1, g1.R_ORDER), g1.G) for _ in range(40)]
    for n in (1, 2, 3, 8, 16, 40):
        got, slow = _run_kernel_way(L, base[:n])
        assert got == g1.sum_points(base[:n]) and not slow
    pts = [None, base[0], None, None, base[1], base[2], None]
    got, slow = _run_kernel_way(L, pts)
    assert got == g1.sum_points([p for p in pts if p]) and not slow
    assert _run_kernel_way(L, [None, None]) == (None, False) and _run_kernel_way(L, []) == (None, False)
    A, Bp = base[0], base[1]
    for pts, want in (([A, A], g1.double(A)), ([A, g1.neg(A)], None), ([A, g1.neg(A), Bp], Bp),
                      ([A, Bp, g1.add(A, Bp)], g1.double(g1.add(A, Bp))), ([A, Bp, g1.neg(g1.add(A, Bp))], None),
                      ([A, A, A, A], g1.mul(4, A)), ([g1.G] * 9, g1.mul(9, g1.G)),
                      ([g1.mul(i + 1, g1.G) for i in range(12)], g1.mul(78, g1.G))):
        got, slow = _run_kernel_way(L, pts)
        assert got == want and slow, (got, want, slow)
        assert _run(L, pts) == want
    if which == "checked":
        assert L.fq30_column_report(C.byref(w), 1) == 0


@pytest.mark.parametrize("which", ["plain", "checked"])
def test_the_trees_complete_adds_over_the_lanes_accumulators(lib, checked, which):
    """g1q_add (what k_g1_tree's cooperative adds spread over lanes and fall back to) over lanes' accumulators, level by
    level, against the oracle: random points, empty lanes, and every special case of the group law between lanes."""
    L = lib if which == "plain" else checked
    w = C.c_double(0)
    if which == "checked":
        L.fq30_column_report(C.byref(w), 1)
    rng = random.Random(77)
    base = [g1.mul(rng.randrange(1, g1.R_ORDER), g1.G) for _ in range(64)]
    for n, k in ((1, 4), (2, 1), (3, 1), (7, 2), (16, 4), (33, 4), (64, 1), (64, 5)):
        assert _run_tree(L, base[:n], k) == g1.sum_points(base[:n]), (n, k)
    assert _run_tree(L, [], 4) is None
    A, Bp, Cp = base[0], base[1], base[2]
    Nn = g1.neg
    assert _run_tree(L, [None, None, A, Bp], 2) == g1.add(A, Bp)
    assert _run_tree(L, [A, Bp, None, None], 2) == g1.add(A, Bp)
    assert _run_tree(L, [None] * 8 + [A] + [None] * 7, 4) == A
    assert _run_tree(L, [None] * 16, 4) is None
    assert _run_tree(L, [A, A], 1) == g1.double(A)
    assert _run_tree(L, [A, Nn(A)], 1) is None
    assert _run_tree(L, [A, Bp, A, Bp], 2) == g1.double(g1.add(A, Bp))
    assert _run_tree(L, [A, Bp, Nn(A), Nn(Bp)], 2) is None
    assert _run_tree(L, [A, Bp, Nn(Bp), Nn(A), Cp], 2) == Cp
    assert _run_tree(L, [A, Bp, g1.add(A, Bp), None], 2) == g1.double(g1.add(A, Bp))
    assert _run_tree(L, [A] * 32, 1) == g1.mul(32, A)
    seq = [g1.mul(i + 1, g1.G) for i in range(32)]
    assert _run_tree(L, seq, 4) == g1.mul(32 * 33 // 2, g1.G)
    if which == "checked":
        assert L.fq30_column_report(C.byref(w), 1) == 0


def test_generated_constants_are_current():
    """fp381_s30_consts.inc is what tools/gen_fq_consts.py 30 prints (everything in it follows from the prime)."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_fq_consts.py"), "30"], capture_output=True,
                         text=True, check=True).stdout
    assert out == open(os.path.join(ROOT, "pos_evolution_amd", "csrc", "fp381_s30_consts.inc")).read()
    n0 = int(out.split("FQ_N0INV = ")[1].split("u;")[0])
    assert (n0 * P + 1) % (1 << B) == 0
