"""The integer model of the 12 x 32 Montgomery field ops of pos_evolution_amd/csrc (fp381.h, fp_inv_safegcd.h via g1.h, fp_sqrt.h,
g2.h, fp12.h's f2_mul_xi) and the record format of tests/native/fp_device_ops.hip.  THE REFERENCE of tests/test_gpu_fp_device.py:
plain Python integers mod p, nothing approximate -- every comparison there is equality of all twelve limbs.

A device value is twelve little-endian 32-bit limbs, i.e. an integer below 2^384; what the ops do to those integers:

    mont_mul(a, b) = a b R^-1 mod p,  R = 2^384        to_mont(a) = a R,  from_mont(a) = a R^-1
    fp_inv:  Montgomery in, Montgomery out;  fp_inv_plain: Montgomery in, plain out;  the inverse of 0 is 0 (g1.h)
    fp_sqrt: Montgomery in and out.  The root is ALWAYS the candidate x^((p+1)/4) (p = 3 mod 4), whichever of the two roots that
             is; the flag says whether its square is x.  For a non-residue the candidate squares to -x and the flag is false
             (fp_sqrt.h: fp_sqrt_candidate, fp_sqrt).
    Fp2 = Fp[u]/(u^2 + 1), a pair (c0, c1).  f2_sqrt_lane (fp_sqrt.h, the "complex method"): status 0 and a root, or status 2
             and y = 0 where the norm is no square.  Which root: the header's own steps, restated in f2_sqrt_lane below.
"""
import struct

P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R = 1 << 384
RINV = pow(R, -1, P)
R1 = R % P
R2 = R * R % P
NINV = (-pow(P, -1, R)) % R        # -p^-1 mod R
M32 = (1 << 32) - 1
HALF = (P - 1) // 2
F2_SQRT_STATUSES = {0, 2}          # fp_sqrt.h: "st stays 0 iff a is a square ... otherwise it becomes 2"


# ---------------------------------------------------------------- limbs and records
def limbs(v):
    assert 0 <= v < R
    return [(v >> (32 * j)) & M32 for j in range(12)]


def from_limbs(ws):
    return sum(int(w) << (32 * j) for j, w in enumerate(ws))


def truncate(v, k):
    """The integer a kernel of the constant family holds: limbs j < k of v, literal zeros above."""
    return v & ((1 << (32 * k)) - 1)


# ---------------------------------------------------------------- Fp
def fp_add(a, b):
    return (a + b) % P


def fp_sub(a, b):
    return (a - b) % P


def fp_neg(a):
    return (-a) % P


def fp_dbl(a):
    return 2 * a % P


def mont_mul(a, b):
    return a * b * RINV % P


def mont_acc(a, b):
    """The product's accumulator before its one conditional subtraction: t = (a b + m p) / R in [0, 2p)."""
    ab = a * b
    m = (ab % R) * NINV % R
    t, rem = divmod(ab + m * P, R)
    assert rem == 0
    return t


def mont_sqr(a):
    return mont_mul(a, a)


def to_mont(a):
    return a * R % P


def from_mont(a):
    return a * RINV % P


def inv(x):
    return pow(x, P - 2, P)           # 0 -> 0


def fp_inv(a):
    return to_mont(inv(from_mont(a)))


def fp_inv_plain(a):
    return inv(from_mont(a))


def sqrt_candidate(x):
    return pow(x, (P + 1) // 4, P)


def fp_sqrt(a):
    """(flag, root), Montgomery in and out."""
    x = from_mont(a)
    r = sqrt_candidate(x)
    return int(r * r % P == x), to_mont(r)


def fp_half(a):
    return (a + (P if a & 1 else 0)) >> 1


def fp_is_larger_half(a):
    return int(from_mont(a) > HALF)


def fp_is_canonical(a):
    return int(a < P)


def be48_round_trip(words):
    """fp_load_be48 of 48 bytes (given as the twelve u32 the device reads), then fp_store_be48: (limbs, stored words)."""
    raw = struct.pack("<12I", *words)
    v = int.from_bytes(raw, "big") & ((1 << 381) - 1)     # the three flag bits of byte 0 are masked
    ls = limbs(v)
    return ls, list(struct.unpack("<12I", v.to_bytes(48, "big")))


def h2c_reduce(hi, lo):
    """hi 2^256 + lo mod p as Montgomery words (h2c_kernels.hip)."""
    return to_mont((hi << 256) + lo)


# ---------------------------------------------------------------- Fp2, plain values
def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_sqr(a):
    return ((a[0] + a[1]) * (a[0] - a[1]) % P, 2 * a[0] * a[1] % P)


def f2_inv(a):
    n = inv((a[0] * a[0] + a[1] * a[1]) % P)
    return (a[0] * n % P, -a[1] * n % P)


def f2_mul_xi(a):
    return ((a[0] - a[1]) % P, (a[0] + a[1]) % P)


def f2_sqrt_lane(a, path=None):
    """(y0, y1, st) for a plain a = (a0, a1); fp_sqrt.h's steps, every one of them a field operation.  path, a list, receives the
    name of the branch taken."""
    path = [] if path is None else path
    a0, a1 = a
    if a1 == 0:
        t = sqrt_candidate(a0)
        path.append("fp residue" if t * t % P == a0 else "fp non-residue")
        return (t, 0, 0) if t * t % P == a0 else (0, t, 0)
    n = (a0 * a0 + a1 * a1) % P
    s = sqrt_candidate(n)
    if s * s % P != n:
        path.append("norm non-residue")
        return 0, 0, 2
    d = (a0 + s) * inv(2) % P
    w = pow(d, (P - 3) // 4, P)
    t = d * w % P
    v = a1 * w * inv(2) % P
    path.append("d residue" if t * t % P == d else "d non-residue")
    if t * t % P == d:
        return t, v, 0
    return (-v) % P, t, 0


# the same ops on Montgomery words, as the device sees them
def m2(a):
    return (to_mont(a[0]), to_mont(a[1]))


def p2(a):
    return (from_mont(a[0]), from_mont(a[1]))


def dev_f2_mul(a, b):
    return m2(f2_mul(p2(a), p2(b)))


def dev_f2_sqr(a):
    return m2(f2_sqr(p2(a)))


def dev_f2_inv_plain(a):
    return f2_inv(p2(a))


def dev_f2_sqrt_lane(a, path=None):
    y0, y1, st = f2_sqrt_lane(p2(a), path)
    return to_mont(y0), to_mont(y1), st


# ---------------------------------------------------------------- the harness's ops: id -> (operands in, words out)
FP_ADD, FP_SUB, FP_NEG, FP_DBL, FP_MUL, FP_SQR, FP_TO_MONT, FP_FROM_MONT = 1, 2, 3, 4, 5, 6, 7, 8
FP_INV, FP_INV_PLAIN, FP_SQRT, FP_HALF, FP_IS_LARGER_HALF, FP_IS_CANONICAL, FP_BE48 = 9, 10, 11, 12, 13, 14, 15
F2_MUL, F2_SQR, F2_INV_PLAIN, F2_IS_ZERO, F2_MUL_XI, F2_SQRT_LANE = 20, 21, 22, 23, 24, 25
MUL_CONST, TO_MONT_CONST, FROM_MONT_CONST = 100, 140, 160   # MUL_CONST + 13 SIDE + K;  TO/FROM_MONT_CONST + K
SIDE_A, SIDE_B, SIDE_BOTH = 0, 1, 2
H2C_REDUCE_BARRIER, H2C_REDUCE_PLAIN = 180, 181
MUL_LITERAL_B, MUL_LITERAL_A, ADD_TO_MONT_LITERAL = 190, 192, 194   # + 0: the literal 1, + 1: the literal 4

SHAPES = {FP_ADD: (2, 12), FP_SUB: (2, 12), FP_NEG: (1, 12), FP_DBL: (1, 12), FP_MUL: (2, 12), FP_SQR: (1, 12),
          FP_TO_MONT: (1, 12), FP_FROM_MONT: (1, 12), FP_INV: (1, 12), FP_INV_PLAIN: (1, 12), FP_SQRT: (1, 13), FP_HALF: (1, 12),
          FP_IS_LARGER_HALF: (1, 1), FP_IS_CANONICAL: (1, 1), FP_BE48: (1, 24),
          F2_MUL: (4, 24), F2_SQR: (2, 24), F2_INV_PLAIN: (2, 24), F2_IS_ZERO: (2, 2), F2_MUL_XI: (2, 24), F2_SQRT_LANE: (2, 25),
          H2C_REDUCE_BARRIER: (2, 12), H2C_REDUCE_PLAIN: (2, 12)}
for _k in range(13):
    for _side in range(3):
        SHAPES[MUL_CONST + 13 * _side + _k] = (2, 12)
    SHAPES[TO_MONT_CONST + _k] = (1, 12)
    SHAPES[FROM_MONT_CONST + _k] = (1, 12)
for _lit in range(2):
    SHAPES[MUL_LITERAL_B + _lit] = (1, 12)
    SHAPES[MUL_LITERAL_A + _lit] = (1, 12)
    SHAPES[ADD_TO_MONT_LITERAL + _lit] = (1, 12)


HARNESS_SOURCE = ("tests", "native", "fp_device_ops.hip")
HARNESS_FLAGS = ("--offload-arch=gfx950", "-O3", "-std=c++17")     # the library's own (csrc/Makefile): the optimiser is the subject


def pack_section(op, records):
    """One section of an operand file: op id, count, then the records' operands as twelve limbs each."""
    nin = SHAPES[op][0]
    out = [struct.pack("<2I", op, len(records))]
    for rec in records:
        assert len(rec) == nin
        for v in rec:
            out.append(struct.pack("<12I", *limbs(v)))
    return b"".join(out)


def unpack_sections(blob, sections):
    """sections: [(op, n)] in file order -> per section a list of n tuples of output words."""
    out, at = [], 0
    for op, n in sections:
        nout = SHAPES[op][1]
        words = struct.unpack_from(f"<{n * nout}I", blob, at)
        at += 4 * n * nout
        out.append([words[i * nout:(i + 1) * nout] for i in range(n)])
    assert at == len(blob), "the output file has another length than the sections ask for"
    return out
