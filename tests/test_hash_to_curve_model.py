"""CPU: tests/hash_to_curve_model.py, the specification of pe_hash_to_g2 / pe_map_to_g2 -- the RFC's known answers and the
expander's digests, outputs in G2, the derived isogeny as a homomorphism with kernel (x0, .), clear_cofactor against the plain
scalar product, and the generated constants of the kernels."""
import os
import random
import re
import subprocess
import sys

from oracle import g2
from oracle.g1 import P, R_ORDER
from tests import hash_to_curve_model as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pos_evolution_amd", "csrc")


def test_known_answers_and_expander_digests():
    v = hm.load_vectors()
    assert [c["msg"] for c in v["points"]] == ["", "abc"]
    for case in v["points"]:
        want = (tuple(int(t, 16) for t in case["x"]), tuple(int(t, 16) for t in case["y"]))
        assert g2.is_on_curve(want)
        assert hm.hash_to_g2(case["msg"].encode(), v["dst"].encode()) == want
    digests = {c["msg"]: c["uniform_bytes"] for c in v["expander"]}
    assert digests[""].startswith("68a985b8") and digests[""].endswith("f07235")
    assert digests["abc"].startswith("d8ccab23") and digests["abc"].endswith("605615")
    for c in v["expander"]:
        assert hm.expand_message_xmd(c["msg"].encode(), v["expander_dst"].encode(), c["len"]).hex() == c["uniform_bytes"]
    # the other sign of Y is a point of E2 as well, and not the answer: the known answers do fix it
    old = hm.Y_SIGN
    try:
        hm.Y_SIGN = -old
        flipped = hm.iso3(hm.map_to_curve_g2(hm.hash_to_field(b"", v["dst"].encode())[0]))
        assert g2.is_on_curve(flipped)
    finally:
        hm.Y_SIGN = old
    assert g2.neg(flipped) == hm.iso3(hm.map_to_curve_g2(hm.hash_to_field(b"", v["dst"].encode())[0]))


def test_hash_to_field_byte_order():
    u0, u1 = hm.hash_to_field(b"abc", hm.ETH2_DST)
    uniform = hm.expand_message_xmd(b"abc", hm.ETH2_DST, 256)
    assert u0[0] == int.from_bytes(uniform[:64], "big") % P and u1[1] == int.from_bytes(uniform[192:], "big") % P
    assert len(hm.u_to_bytes(u0, u1)) == 192


def test_outputs_lie_in_g2():
    for msg in (b"", b"\x00" * 32, bytes(range(32)), b"a" * 255):
        q = hm.hash_to_g2(msg)
        assert q is not None and g2.is_on_curve(q) and hm.curve_mul(R_ORDER, q) is None


def _iso_add(p1, p2):
    """affine addition on E' (a = A')"""
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    if p1[0] == p2[0]:
        if p1[1] != p2[1] or p1[1] == (0, 0):
            return None
        lam = g2.f2_mul(g2.f2_add(g2.f2_scalar(g2.f2_sqr(p1[0]), 3), hm.A_ISO), g2.f2_inv(g2.f2_scalar(p1[1], 2)))
    else:
        lam = g2.f2_mul(g2.f2_sub(p2[1], p1[1]), g2.f2_inv(g2.f2_sub(p2[0], p1[0])))
    x3 = g2.f2_sub(g2.f2_sub(g2.f2_sqr(lam), p1[0]), p2[0])
    return (x3, g2.f2_sub(g2.f2_mul(lam, g2.f2_sub(p1[0], x3)), p1[1]))


def test_iso3_is_a_homomorphism_with_kernel_x0():
    rng = random.Random(11)
    pts = [hm.map_to_curve_g2((rng.randrange(P), rng.randrange(P))) for _ in range(4)]
    for p in pts:
        assert g2.f2_sqr(p[1]) == hm.g_iso(p[0])
        assert g2.is_on_curve(hm.iso3(p))
    for a, b in ((pts[0], pts[1]), (pts[2], pts[3]), (pts[0], pts[0])):
        assert hm.iso3(_iso_add(a, b)) == g2.add(hm.iso3(a), hm.iso3(b))
    # the kernel: x = x0 goes to the identity whatever y is.  Its points have y^2 = g(x0) = 4 (1 + i), no square in Fp2: the
    # kernel is rational as a SET only, so no u reaches it and the map never returns the identity
    assert hm.Y0_SQ == (4, 4) and not hm.f2_is_square(hm.Y0_SQ)
    assert hm.iso3((hm.X0, (1, 2))) is None and hm.iso3((hm.X0, (P - 1, P - 2))) is None


def test_swu_edges():
    x, y = hm.map_to_curve_g2((0, 0))                        # the exceptional case
    assert x == g2.f2_mul(hm.B_ISO, g2.f2_inv(g2.f2_mul(hm.Z_SWU, hm.A_ISO))) and hm.sgn0(y) == 0
    for u in ((0, 1), (0, 2), (1, 0), (2, 5)):
        assert hm.sgn0(hm.map_to_curve_g2(u)[1]) == hm.sgn0(u)
    assert hm.sgn0((0, 1)) == 1 and hm.sgn0((0, 2)) == 0 and hm.sgn0((2, 1)) == 0
    u = (5, 7)
    assert hm.map_to_g2(u, g2.f2_neg(u)) is None             # opposite points: the identity
    q = hm.iso3(hm.map_to_curve_g2(u))
    assert hm.map_to_g2(u, u) == hm.clear_cofactor(g2.double(q))


def test_clear_cofactor_is_the_scalar_product():
    c = hm.C_PARAM
    rng = random.Random(12)
    for _ in range(2):
        pt = hm.iso3(hm.map_to_curve_g2((rng.randrange(P), rng.randrange(P))))   # on E2, outside G2
        assert hm.curve_mul(R_ORDER, pt) is not None
        want = g2.add(g2.add(hm.curve_mul(c * c - c - 1, pt), hm.curve_mul(c - 1, hm.psi(pt))),
                      hm.curve_mul(2, hm.psi(hm.psi(pt))))
        assert hm.clear_cofactor(pt) == want
    # on G2 itself psi acts as [c]: the whole map is one scalar, evaluated with g2.mul
    pt = g2.mul(rng.randrange(1, R_ORDER), g2.G2)
    k = (c * c - c - 1) + (c - 1) * c + 2 * c * c
    assert hm.clear_cofactor(pt) == g2.mul(k % R_ORDER, pt)


def test_the_kernels_expander_on_the_host_agrees_with_hashlib(tmp_path):
    """pos_evolution_amd/csrc/h2c_expand.h -- the text k_h2c_expand runs -- compiled by the host compiler: the 256 uniform bytes
    at the padding edges of the message (b0's last block) and of the tag (b_i's), and at both bounds of either length."""
    import ctypes
    out = tmp_path / "libh2c_expand_host.so"
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", str(out),
                    os.path.join(ROOT, "tests", "native", "h2c_expand_host.cpp")], check=True)
    lib = ctypes.CDLL(str(out))

    def run(msg, dst):
        buf = ctypes.create_string_buffer(256)
        lib.h2c_host_expand256(msg, len(msg), dst, len(dst), buf)
        return buf.raw

    rng = random.Random(13)
    text = lambda n: bytes(rng.randrange(256) for _ in range(n))
    for msg_len in (0, 8, 9, 16, 17, 32, 255):
        msg = text(msg_len)
        assert run(msg, hm.ETH2_DST) == hm.expand_message_xmd(msg, hm.ETH2_DST, 256), msg_len
    for dst_len in (1, 20, 21, 22, 23, 255):
        dst = text(dst_len)
        assert run(b"abc", dst) == hm.expand_message_xmd(b"abc", dst, 256), dst_len
    for msg_len in range(40):           # every residue of the 64-byte block around the tag's 43 bytes
        msg = text(msg_len)
        assert run(msg, hm.ETH2_DST) == hm.expand_message_xmd(msg, hm.ETH2_DST, 256), msg_len


def test_generated_constants_are_current():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_h2c_consts.py")], capture_output=True, text=True,
                         check=True).stdout
    assert out == open(os.path.join(CSRC, "h2c_consts.inc")).read(), "h2c_consts.inc: run tools/gen_h2c_consts.py"

    def limbs(name, comp):
        body = out[out.index(name + "[2][12]"):]
        rows = re.findall(r"\{((?:0x[0-9a-f]{8}u,? ?){12})\}", body)[comp]
        return sum(int(w, 16) << (32 * j) for j, w in enumerate(re.findall(r"0x([0-9a-f]{8})u", rows)))

    mont = lambda v: v * (1 << 384) % P
    for name, val in (("H2C_V", hm.V_VELU), ("H2C_UQ", hm.UQ_VELU), ("H2C_X0", hm.X0), ("H2C_Z", hm.Z_SWU),
                      ("H2C_PSI_CX", hm.CX), ("H2C_PSI_CY", hm.CY)):
        assert (limbs(name, 0), limbs(name, 1)) == (mont(val[0]), mont(val[1])), name


def test_header_binding_and_surface():
    from pos_evolution_amd import _abi, engine, forkchoice
    boundary = open(os.path.join(ROOT, "include", "posevo.h")).read()
    for name in ("pe_hash_to_g2", "pe_map_to_g2"):
        args = re.search(r"\bint %s\s*\(([^)]*)\)" % name, boundary).group(1)
        assert len(args.split(",")) == len(_abi.SIGNATURES[name][1]), name
        assert hasattr(_abi.load(), name)
    assert callable(engine.Engine.hash_to_g2) and callable(engine.Engine.map_to_g2)
    assert forkchoice.ETH2_DST == hm.ETH2_DST == _abi.ETH2_DST and callable(forkchoice.hash_to_curve_g2)
    log = open(os.path.join(CSRC, "h2c_kernels.resource.log")).read()
    names = re.findall(r"Function Name: (\S+)", log)
    for want in ("k_h2c_expand", "k_h2c_map", "k_h2c_finish"):
        assert any(want in n for n in names), want
