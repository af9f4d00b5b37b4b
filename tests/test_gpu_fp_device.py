"""-m gpu: the 12 x 32 Montgomery field ops (fp381.h, g1.h's inversions, fp_sqrt.h, g2.h's lane-pair Fp2, f2_mul_xi) applied ON
THE DEVICE to chosen operands and held, limb for limb, to Python integers (tests/fp_device_model.py).  The product is 288
multiply-add pairs in inline-assembly statements that no host compiler can run: the other GPU tests reach it only through whole
curve and pairing operations, which never choose a field operand such as p - 1, one all-ones limb, or a sum that lands on p.

tests/native/fp_device_ops.hip is the program (its own main, the library's compiler flags, the inline product); every test writes
an operand file, runs it ONCE as a child process and compares every record.  The constant-operand family hands the product
operands whose upper limbs are literal zeros in the kernel -- the pattern of fp_from_mont's {1, 0, ...}, of the curve kernels'
four = {4, 0, ...} and of h2c_reduce's 256-bit halves -- and requires the product of the integer the kernel's
value IS."""
import json
import os
import random
import subprocess

import pytest

from tests import fp_device_model as M
from tests.hash_to_curve_model import expand_message_xmd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pos_evolution_amd", "csrc")
SRC = os.path.join(ROOT, *M.HARNESS_SOURCE)
BIN = SRC[:-len(".hip")]
P, R = M.P, M.R
_UNUSABLE = []        # why the program must not be started again in this session, once a child faulted or hung


# ---------------------------------------------------------------- operands: the same list for every op
def _edge_list():
    e = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, M.R1, M.R2]
    for k in range(1, 12):                                  # every limb-carry edge
        e += [(1 << (32 * k)) - 1, 1 << (32 * k)]
    e += [(0xFFFFFFFF << (32 * j)) % P for j in range(12)]  # limb j alone all ones (j = 11 is above p: reduced)
    e.append(((1 << 380) - 1) % P)                          # all ones below bit 380
    return e


_RNG = random.Random(0x381)
EDGES = _edge_list()
RANDOMS = [_RNG.randrange(P) for _ in range(40)]
OPERANDS = EDGES + RANDOMS
SEARCH = [_RNG.randrange(P) for _ in range(400)]            # second factors for the search of test_fp_mul_at_its_subtraction
assert all(0 <= v < P for v in OPERANDS) and len(OPERANDS) == 84


# ---------------------------------------------------------------- building and running the program
@pytest.fixture(scope="session")
def harness():
    deps = [SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".inc"))]
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", *M.HARNESS_FLAGS, "-I", CSRC, SRC, "-o", BIN])
    return BIN


def _child(binary, in_path, out_path):
    return subprocess.run([binary, in_path, out_path], capture_output=True, text=True, timeout=120)


def run_sections(binary, tmp_path, sections):
    """sections: [(op, records)] -> per section the list of output word tuples.  One child process, one launch per section."""
    if _UNUSABLE:
        pytest.skip("fp_device_ops is not started again: " + _UNUSABLE[0])
    in_path, out_path = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(in_path, "wb") as f:
        f.write(b"".join(M.pack_section(op, recs) for op, recs in sections))
    try:
        out = _child(binary, in_path, out_path)
    except subprocess.TimeoutExpired as e:
        _UNUSABLE.append("an earlier child process ran into its time limit")
        pytest.fail(f"fp_device_ops timed out\n{e.stdout}\n{e.stderr}")
    text = f"exit status {out.returncode}\n{out.stdout[-3000:]}\n{out.stderr[-3000:]}"
    if out.returncode in (134, 139, -6, -11, 2) or "HIP error" in out.stderr:
        _UNUSABLE.append(f"an earlier child process ended with status {out.returncode}")
        pytest.fail("fp_device_ops faulted: " + text)
    assert out.returncode == 0, text
    with open(out_path, "rb") as f:
        return M.unpack_sections(f.read(), [(op, len(recs)) for op, recs in sections])


def _fp(v):
    return tuple(M.limbs(v))


def mismatches(got, want, records):
    """Every record compared; the first few differences spelled out."""
    assert len(got) == len(want) == len(records)
    bad = [i for i in range(len(want)) if tuple(got[i]) != tuple(want[i])]
    show = [f"  record {i}: operands {[hex(v) for v in records[i]]}\n    device {[hex(w) for w in got[i]]}\n    model  "
            f"{[hex(w) for w in want[i]]}" for i in bad[:3]]
    return bad, "\n".join(show)


def hold(binary, tmp_path, cases):
    """cases: [(label, op, records, model)], model(record) -> the expected output words.  One child; every record of every section
    must equal the model, and a failure names every section that differs with its count."""
    out = run_sections(binary, tmp_path, [(op, recs) for _, op, recs, _ in cases])
    report = []
    for (label, _, recs, model), got in zip(cases, out):
        bad, text = mismatches(got, [tuple(model(r)) for r in recs], recs)
        print(f"{label}: {len(recs) - len(bad)} of {len(recs)} records equal the model")
        if bad:
            report.append(f"{label}: {len(bad)} of {len(recs)} records differ\n{text}")
    assert not report, "\n".join(report)


# ---------------------------------------------------------------- Fp, one lane per record
def _pairs_for(op):
    pairs = [(a, b) for a in OPERANDS for b in OPERANDS]
    if op == M.FP_ADD:        # both sides of the conditional subtraction: a + b = p - 1, p, p + 1
        pairs += [(a, s - a) for a in OPERANDS for s in (P - 1, P, P + 1) if 0 <= s - a < P]
    elif op == M.FP_SUB:      # a = b, a = b - 1, a = b + 1
        pairs += [(b + d, b) for b in OPERANDS for d in (0, -1, 1) if 0 <= b + d < P]
    else:                     # Montgomery products 0, 1 and p - 1, made with the model's inverse
        pairs += [(a, 0) for a in OPERANDS] + [(0, a) for a in OPERANDS]
        for a in OPERANDS:
            if a:
                pairs += [(a, t * R % P * M.inv(a) % P) for t in (1, P - 1)]
    return pairs


@pytest.mark.parametrize("name,op,model", [("fp_add", M.FP_ADD, M.fp_add), ("fp_sub", M.FP_SUB, M.fp_sub),
                                           ("fp_mul", M.FP_MUL, M.mont_mul)])
def test_binary_op_on_every_pair_of_the_operand_list(harness, tmp_path, name, op, model):
    pairs = _pairs_for(op)
    if op == M.FP_MUL:
        tail = [M.mont_mul(a, b) for a, b in pairs[-2 * (len(OPERANDS) - 1):]]
        assert set(tail) == {1, P - 1} and M.mont_mul(*pairs[len(OPERANDS) ** 2]) == 0
    hold(harness, tmp_path, [(name, op, pairs, lambda r: _fp(model(*r)))])


def test_fp_mul_at_its_subtraction(harness, tmp_path):
    """The product's accumulator t = (a b + m p) / R lies in [0, 2p) and is reduced by ONE conditional subtraction of p: pairs whose
    t falls within p / 2^10 of p, on either side, by search over the seeded values (40 x 400 pairs; t / p is spread over [0, 2), so
    about eight pairs are expected on each side; the seed gives 12 below and 18 above)."""
    window = P >> 10
    below, above = [], []
    for a in RANDOMS:
        for b in SEARCH:
            t = M.mont_acc(a, b)
            if P - window <= t < P:
                below.append((a, b))
            elif P <= t < P + window:
                above.append((a, b))
    print(f"accumulator just below p: {len(below)} pairs, at or just above p: {len(above)} pairs")
    assert below and above
    hold(harness, tmp_path, [("fp_mul, t just below p", M.FP_MUL, below, lambda r: _fp(M.mont_mul(*r))),
                             ("fp_mul, t just above p", M.FP_MUL, above, lambda r: _fp(M.mont_mul(*r)))])


def test_unary_ops_on_the_operand_list(harness, tmp_path):
    recs = [(a,) for a in OPERANDS]
    one = [("fp_neg", M.FP_NEG, M.fp_neg), ("fp_dbl", M.FP_DBL, M.fp_dbl), ("fp_sqr", M.FP_SQR, M.mont_sqr),
           ("fp_to_mont", M.FP_TO_MONT, M.to_mont), ("fp_from_mont", M.FP_FROM_MONT, M.from_mont), ("fp_half", M.FP_HALF, M.fp_half)]
    cases = [(name, op, recs, lambda r, f=f: _fp(f(r[0]))) for name, op, f in one]
    # fp_is_larger_half takes Montgomery words: both the list itself and the list as the PLAIN values, (p - 1)/2 and (p + 1)/2 among them
    larger = recs + [(M.to_mont(a),) for a in OPERANDS]
    cases.append(("fp_is_larger_half", M.FP_IS_LARGER_HALF, larger, lambda r: (M.fp_is_larger_half(r[0]),)))
    assert {M.fp_is_larger_half(r[0]) for r in larger} == {0, 1}
    hold(harness, tmp_path, cases)


def test_canonical_check_and_byte_order_on_any_384_bit_value(harness, tmp_path):
    """fp_is_canonical and fp_load_be48 / fp_store_be48 take what the wire brings: values at and above p, flag bits set."""
    rng = random.Random(48)
    raw = OPERANDS + [P, P + 1, R - 1, 0xFFFFFFFF << 352, (1 << 381) - 1, 1 << 381, 1 << 383] + [rng.getrandbits(384) for _ in range(40)]
    raw += [P - 1 + (d << (32 * j)) for j in range(12) for d in (-1, 1) if 0 <= P - 1 + (d << (32 * j)) < R]
    recs = [(v,) for v in raw]
    assert {M.fp_is_canonical(v) for v in raw} == {0, 1}

    def be48(r):
        ls, stored = M.be48_round_trip(M.limbs(r[0]))
        return tuple(ls) + tuple(stored)

    hold(harness, tmp_path, [("fp_is_canonical", M.FP_IS_CANONICAL, recs, lambda r: (M.fp_is_canonical(r[0]),)),
                             ("fp_load_be48 / fp_store_be48", M.FP_BE48, recs, be48)])


def test_inversions_and_their_products_on_the_device(harness, tmp_path):
    """fp_inv and fp_inv_plain (0 -> 0), then a * inv(a) by fp_mul ON THE DEVICE, on the inverses the device returned."""
    vals = [0, 1, P - 1, 2] + [1 << k for k in (1, 31, 32, 33, 380)] + RANDOMS
    vals += [M.to_mont(v) for v in vals]                     # the same values as the PLAIN residues behind the Montgomery words
    recs = [(a,) for a in vals]
    (tmp_path / "inv").mkdir()
    inv_m, inv_p = run_sections(harness, tmp_path / "inv", [(M.FP_INV, recs), (M.FP_INV_PLAIN, recs)])
    for label, got, f in (("fp_inv", inv_m, M.fp_inv), ("fp_inv_plain", inv_p, M.fp_inv_plain)):
        bad, text = mismatches(got, [_fp(f(a)) for a in vals], recs)
        assert not bad, f"{label}: {len(bad)} of {len(recs)} records differ\n{text}"
    back_m = [(a, M.from_limbs(w)) for a, w in zip(vals, inv_m)]
    back_p = [(a, M.from_limbs(w)) for a, w in zip(vals, inv_p)]
    hold(harness, tmp_path, [("a * fp_inv(a) = the Montgomery one", M.FP_MUL, back_m, lambda r: _fp(M.R1 if r[0] else 0)),
                             ("a * fp_inv_plain(a) = the plain one", M.FP_MUL, back_p, lambda r: _fp(1 if r[0] else 0))])


def test_square_roots_residues_and_non_residues(harness, tmp_path):
    """fp_sqrt returns the candidate x^((p+1)/4) and whether it squares to x.  p - 1 is a non-residue (p = 3 mod 4), and so is
    p - 1 times any non-zero square."""
    squares = [a * a % P for a in OPERANDS]
    plain = [0, 1, P - 1] + squares + [(P - 1) * s % P for s in squares]
    recs = [(M.to_mont(x),) for x in plain]
    want = [M.fp_sqrt(r[0]) for r in recs]
    assert {flag for flag, _ in want} == {0, 1}
    assert all(flag == (pow(x, (P - 1) // 2, P) in (0, 1)) for x, (flag, _) in zip(plain, want))
    hold(harness, tmp_path, [("fp_sqrt", M.FP_SQRT, recs, lambda r: _fp(M.fp_sqrt(r[0])[1]) + (M.fp_sqrt(r[0])[0],))])


# ---------------------------------------------------------------- Fp2, one lane pair per record
def _f2_list():
    vals = [(e, 0) for e in EDGES] + [(0, e) for e in EDGES] + [(P - 1, P - 1)]
    return vals + [(RANDOMS[2 * i], RANDOMS[2 * i + 1]) for i in range(10)]


F2_VALUES = _f2_list()


def _f2_words(v):
    return _fp(v[0]) + _fp(v[1])


def test_fp2_lane_pair_ops(harness, tmp_path):
    """f2_mul, f2_sqr, f2_inv_plain, f2_is_zero (g2.h) and f2_mul_xi (fp12.h): the operand list on each component with the other
    component zero, both components p - 1, a = conj(b), and random values; 98 values are 196 lanes, more than three waves."""
    n = len(F2_VALUES)
    mul = [(a, F2_VALUES[(i + s) % n]) for i, a in enumerate(F2_VALUES) for s in (0, 1, 7, 31)]
    mul += [(a, (a[0], (P - a[1]) % P)) for a in F2_VALUES]                                   # a = conj(b)
    mul_recs = [(a[0], a[1], b[0], b[1]) for a, b in mul]
    recs = [tuple(a) for a in F2_VALUES]
    zero = recs + [(0, 0), (0, 1), (1, 0)]
    assert {int(r == (0, 0)) for r in zero} == {0, 1}
    hold(harness, tmp_path, [
        ("f2_mul", M.F2_MUL, mul_recs, lambda r: _f2_words(M.dev_f2_mul(r[:2], r[2:]))),
        ("f2_sqr", M.F2_SQR, recs, lambda r: _f2_words(M.dev_f2_sqr(r))),
        ("f2_inv_plain", M.F2_INV_PLAIN, recs, lambda r: _f2_words(M.dev_f2_inv_plain(r))),
        ("f2_is_zero", M.F2_IS_ZERO, zero, lambda r: (int(r == (0, 0)),) * 2),               # both lanes of the pair answer
        ("f2_mul_xi", M.F2_MUL_XI, recs, lambda r: _f2_words(M.f2_mul_xi(r))),
    ])


def test_fp2_square_root_in_one_lane_every_branch_and_status(harness, tmp_path):
    """f2_sqrt_lane: squares (status 0, the root the header's steps give) and non-squares (status 2, y left zero).  Every branch of
    the header is taken -- a in Fp a residue and a non-residue, d a residue and a non-residue, the norm a non-residue -- and the
    statuses seen are exactly the ones fp_sqrt.h documents."""
    squares = [M.f2_sqr(a) for a in F2_VALUES]
    non_square = next((c, 1) for c in range(1, 50) if pow(c * c + 1, (P - 1) // 2, P) == P - 1)   # its norm is no residue
    plain = squares + [M.f2_mul(non_square, s) for s in squares]
    recs = [M.m2(x) for x in plain]
    paths, want = [], []
    for r in recs:
        y0, y1, st = M.dev_f2_sqrt_lane(r, paths)
        want.append(_fp(y0) + _fp(y1) + (st,))
    assert set(paths) == {"fp residue", "fp non-residue", "d residue", "d non-residue", "norm non-residue"}
    out = run_sections(harness, tmp_path, [(M.F2_SQRT_LANE, recs)])[0]
    bad, text = mismatches(out, want, recs)
    assert not bad, f"f2_sqrt_lane: {len(bad)} of {len(recs)} records differ\n{text}"
    assert {w[24] for w in out} == M.F2_SQRT_STATUSES


# ---------------------------------------------------------------- the constant-operand family
def _cut_list(k):
    """The loaded limbs: every operand of the edge list cut to k limbs, and the randoms; once each."""
    seen = []
    for v in OPERANDS:
        if M.truncate(v, k) not in seen:
            seen.append(M.truncate(v, k))
    return seen


FULL = [P - 1, M.R2, ((1 << 380) - 1) % P, RANDOMS[0]]       # the fully loaded operand beside a cut one


@pytest.mark.parametrize("side", [M.SIDE_A, M.SIDE_B, M.SIDE_BOTH], ids=["a", "b", "both"])
def test_product_with_literal_zero_upper_limbs(harness, tmp_path, side):
    """OpMulConst<K, SIDE> of the harness, K = 0 .. 12: limbs j >= K of the operand(s) named by SIDE are literal zeros in the kernel, no register
    barrier anywhere.  The kernel ignores the file's limbs above K; the model multiplies the integer that is left."""
    cases = []
    for k in range(13):
        cut = _cut_list(k)
        if side == M.SIDE_A:
            recs = [(a, b) for a in cut for b in FULL]
        elif side == M.SIDE_B:
            recs = [(a, b) for b in cut for a in FULL]
        else:
            recs = [(a, cut[(i + s) % len(cut)]) for i, a in enumerate(cut) for s in (0, 1, 5)]
        # the file carries all-ones above limb K: a kernel that read them would not pass
        pad = (R - 1) ^ ((1 << (32 * k)) - 1)
        filed = [(a | pad if side != M.SIDE_B else a, b | pad if side != M.SIDE_A else b) for a, b in recs]
        cases.append((f"K = {k}", M.MUL_CONST + 13 * side + k, filed,
                      lambda r, k=k: _fp(M.mont_mul(M.truncate(r[0], k) if side != M.SIDE_B else r[0],
                                                    M.truncate(r[1], k) if side != M.SIDE_A else r[1]))))
    hold(harness, tmp_path, cases)


@pytest.mark.parametrize("name,base,model", [("fp_to_mont", M.TO_MONT_CONST, M.to_mont), ("fp_from_mont", M.FROM_MONT_CONST, M.from_mont)])
def test_conversion_of_a_value_with_literal_zero_upper_limbs(harness, tmp_path, name, base, model):
    cases = []
    for k in range(13):
        pad = (R - 1) ^ ((1 << (32 * k)) - 1)
        cases.append((f"{name}, K = {k}", base + k, [(a | pad,) for a in _cut_list(k)], lambda r, k=k: _fp(model(M.truncate(r[0], k)))))
    hold(harness, tmp_path, cases)


def test_low_literal_over_literal_zeros(harness, tmp_path):
    """l[0] = 1 or 4 over literal zeros: fp_from_mont's multiplier, and four = to_mont({4, 0, ...}) added to a loaded value (the
    curve equation's right-hand side in k_g1_decompress, k_g2_decompress and wire_points.h)."""
    recs = [(a,) for a in OPERANDS]
    cases = []
    for i, v in enumerate((1, 4)):
        cases += [(f"fp_mul(a, {{{v}, 0, ...}})", M.MUL_LITERAL_B + i, recs, lambda r, v=v: _fp(M.mont_mul(r[0], v))),
                  (f"fp_mul({{{v}, 0, ...}}, a)", M.MUL_LITERAL_A + i, recs, lambda r, v=v: _fp(M.mont_mul(v, r[0]))),
                  (f"a + fp_to_mont({{{v}, 0, ...}})", M.ADD_TO_MONT_LITERAL + i, recs, lambda r, v=v: _fp(M.fp_add(r[0], M.to_mont(v))))]
    hold(harness, tmp_path, cases)


def _rfc_halves():
    """The (hi, lo) halves hash_to_field reduces for the RFC 9380 known answers of tests/golden/hash_to_curve_vectors.json."""
    with open(os.path.join(ROOT, "tests", "golden", "hash_to_curve_vectors.json")) as f:
        vec = json.load(f)
    out = []
    for pt in vec["points"]:
        uniform = expand_message_xmd(pt["msg"].encode(), vec["dst"].encode(), 256)
        for k in range(4):
            e = uniform[64 * k:64 * k + 64]
            out.append((int.from_bytes(e[:32], "big"), int.from_bytes(e[32:], "big")))
    return out


@pytest.mark.parametrize("name,op", [("with the register barrier", M.H2C_REDUCE_BARRIER), ("without a barrier", M.H2C_REDUCE_PLAIN)])
def test_h2c_reduce_shape(harness, tmp_path, name, op):
    """hi 2^256 + lo mod p from two 256-bit halves, h2c_reduce's very statements: two fp_to_mont, one fp_mul by the Montgomery form
    of 2^256, one fp_add -- with the halves' limbs behind a register barrier, and as plain values whose upper four limbs the
    compiler knows to be zero."""
    rng = random.Random(256)
    special = [0, 1, (1 << 256) - 1, P & ((1 << 256) - 1)]
    recs = [(h, l) for h in special for l in special] + _rfc_halves()
    recs += [(rng.getrandbits(256), rng.getrandbits(256)) for _ in range(100)]
    assert len(_rfc_halves()) == 8
    hold(harness, tmp_path, [(f"h2c_reduce {name}", op, recs, lambda r: _fp(M.h2c_reduce(*r)))])
