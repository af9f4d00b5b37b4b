"""CPU: tests/native/fp_device_ops.hip (the device harness of tests/test_gpu_fp_device.py) cross-compiles for gfx950 with the
library's flags, and tests/fp_device_model.py, the reference those GPU tests compare with, is held to pow() and to a second,
naive Fp2 -- so that neither rots on a machine without a GPU."""
import os
import random
import re
import struct
import subprocess

from tests import fp_device_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pos_evolution_amd", "csrc")
P, R = M.P, M.R
RNG = random.Random(12 * 32)
VALUES = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, M.R1, M.R2] + [RNG.randrange(P) for _ in range(60)]


def test_harness_compiles_for_gfx950(tmp_path):
    src = os.path.join(ROOT, *M.HARNESS_SOURCE)
    subprocess.check_call(["/opt/rocm/bin/hipcc", *M.HARNESS_FLAGS, "-Wall", "-Wno-unused-function", "-Werror", "-I", CSRC, "-c", src,
                           "-o", str(tmp_path / "fp_device_ops.o")])


def test_harness_and_model_name_the_same_ops():
    """Every op id of the model's table is registered in the program, with the same operand and output counts."""
    text = open(os.path.join(ROOT, *M.HARNESS_SOURCE)).read()
    shape = {m.group(1): (int(m.group(2)), int(m.group(3)))
             for m in re.finditer(r"struct (Op\w+) \{\s*static constexpr int NIN = (\d+), NOUT = (\d+);", text)}
    ids = {int(m.group(3)): shape[m.group(2)] for m in re.finditer(r"(lane|pair)_op<(Op\w+?)(?:<[^()]*>)?>\((\d+)\)", text)}
    for m in re.finditer(r"(lane|pair)_op<(Op\w+)<K(?:, \w+)?>>\((\d+) \+ K\)", text):
        for k in range(13):
            ids[int(m.group(3)) + k] = shape[m.group(2)]
    assert ids == M.SHAPES
    limbs = [int(w, 16) for w in re.search(r"TWO_P256_MONT\[12\] = \{([^}]*)\}", text).group(1).replace("u", "").split(",")]
    assert M.from_limbs(limbs) == M.to_mont(1 << 256)


def test_montgomery_forms_round_trip():
    assert M.R1 == M.to_mont(1) and M.R2 == M.to_mont(M.R1) and (P * M.NINV + 1) % R == 0
    for x in VALUES:
        assert M.from_mont(M.to_mont(x)) == x == M.to_mont(M.from_mont(x))
        assert M.from_limbs(M.limbs(x)) == x
        for y in VALUES[:12]:
            assert M.mont_mul(M.to_mont(x), M.to_mont(y)) == M.to_mont(x * y % P)
            t = M.mont_acc(x, y)
            assert 0 <= t < 2 * P and t % P == M.mont_mul(x, y)


def test_inverse_square_root_and_halving_against_pow():
    for x in VALUES:
        a = M.to_mont(x)
        want = pow(x, -1, P) if x else 0
        assert M.from_mont(M.fp_inv(a)) == want == M.fp_inv_plain(a)
        assert M.fp_half(x) * 2 % P == x and 0 <= M.fp_half(x) < P
        flag, root = M.fp_sqrt(a)
        r = M.from_mont(root)
        assert flag == (pow(x, (P - 1) // 2, P) in (0, 1))
        assert r * r % P == (x if flag else P - x)
        assert M.fp_is_larger_half(a) == (x > P - x and x != 0)
    assert P % 4 == 3 and M.fp_sqrt(M.to_mont(P - 1))[0] == 0


def _naive_mul(a, b):
    """(a0 + a1 u)(b0 + b1 u) by polynomial multiplication and reduction by u^2 + 1."""
    c = [0, 0, 0]
    for i in range(2):
        for j in range(2):
            c[i + j] += a[i] * b[j]
    return ((c[0] - c[2]) % P, c[1] % P)


def test_fp2_formulas_against_a_naive_implementation():
    vals = [(x, y) for x in VALUES[:9] for y in VALUES[:9]] + [(RNG.randrange(P), RNG.randrange(P)) for _ in range(40)]
    paths, statuses = set(), set()
    for i, a in enumerate(vals):
        b = vals[(7 * i + 3) % len(vals)]
        assert M.f2_mul(a, b) == _naive_mul(a, b)
        assert M.f2_sqr(a) == _naive_mul(a, a)
        assert M.f2_mul_xi(a) == _naive_mul(a, (1, 1))
        assert _naive_mul(a, M.f2_inv(a)) == ((1, 0) if a != (0, 0) else (0, 0))
        assert M.p2(M.dev_f2_mul(M.m2(a), M.m2(b))) == _naive_mul(a, b) and M.dev_f2_inv_plain(M.m2(a)) == M.f2_inv(a)
        for x in (_naive_mul(a, a), a):
            path = []
            y0, y1, st = M.f2_sqrt_lane(x, path)
            paths.update(path)
            statuses.add(st)
            norm = (x[0] * x[0] + x[1] * x[1]) % P
            assert (st == 0) == (pow(norm, (P - 1) // 2, P) in (0, 1))          # a is a square iff its norm is one
            assert _naive_mul((y0, y1), (y0, y1)) == x if st == 0 else (y0, y1) == (0, 0)
    assert statuses == M.F2_SQRT_STATUSES
    assert paths == {"fp residue", "fp non-residue", "d residue", "d non-residue", "norm non-residue"}


def test_byte_order_round_trip_and_sections():
    words = list(range(0xE0000001, 0xE000000D))
    ls, stored = M.be48_round_trip(words)
    raw = struct.pack("<12I", *words)
    assert M.from_limbs(ls) == int.from_bytes(raw, "big") % (1 << 381)
    assert struct.pack("<12I", *stored) == bytes([raw[0] & 0x1F]) + raw[1:]
    blob = M.pack_section(M.FP_ADD, [(1, 2), (P - 1, 3)])
    assert len(blob) == 8 + 2 * 2 * 48 and struct.unpack_from("<2I", blob) == (M.FP_ADD, 2)
    out = M.unpack_sections(struct.pack("<26I", *range(26)), [(M.FP_ADD, 1), (M.FP_SQRT, 1), (M.FP_IS_CANONICAL, 1)])
    assert [len(s[0]) for s in out] == [12, 13, 1]
