"""CPU: what the pairing check commits as generated or derived text stays what its generator writes, its kernels use no
scratch memory, and the header and the binding agree on the new entry points."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pos_evolution_amd", "csrc")


def _generator():
    spec = importlib.util.spec_from_file_location("generate_pairing", os.path.join(ROOT, "tests", "golden", "generate_pairing.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_frobenius_constants_follow_from_p_and_the_tower():
    from tests import pairing_model as pm
    from oracle.g1 import P
    from oracle.g2 import f2_mul
    xi6 = [pm.f2_pow(pm.XI, (P ** n - 1) // 6) for n in (1, 2, 3)]      # w^(p^n - 1)
    for n in range(3):
        acc = (1, 0)
        for k in range(6):
            assert pm.FROB[n][k] == acc
            acc = f2_mul(acc, xi6[n])
        assert pm.f2_pow(xi6[n], 6) == pm.f2_pow(pm.XI, P ** (n + 1) - 1)
    assert all(c[1] == 0 for c in pm.FROB[1])                          # the p^2 constants lie in Fp


def test_committed_constants_are_the_generated_ones():
    gen = _generator()
    assert open(gen.INC_PATH).read() == gen.inc_text(), "bls_consts.inc: run tests/golden/generate_pairing.py"


def test_committed_vectors_are_the_generated_ones():
    gen = _generator()
    assert open(gen.JSON_PATH).read() == gen.json_text(), "pairing_vectors.json: run tests/golden/generate_pairing.py"
    names = [g["name"] for g in gen.vectors()["groups"]]
    assert names == ["one_pair", "two_pairs", "three_pairs", "with_infinity", "seven_pairs", "thirteen_pairs",
                     "thirteen_pairs_infinity_at_6_and_12"]


def test_no_kernel_of_the_pairing_check_uses_scratch():
    log = open(os.path.join(CSRC, "bls_kernels.resource.log")).read()
    names = re.findall(r"Function Name: (\S+)", log)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", log)]
    assert len(names) == len(scratch) >= 3
    for want in ("k_bls_prepare", "k_bls_miller", "k_bls_final_exp"):
        assert any(want in n for n in names), want
    assert all(v == 0 for v in scratch), list(zip(names, scratch))


def test_header_and_binding_agree_on_the_new_entry_points():
    from pos_evolution_amd import _abi
    boundary = open(os.path.join(ROOT, "include", "posevo.h")).read()
    profile = open(os.path.join(ROOT, "include", "posevo_profile.h")).read()
    for name in ("pe_pairing_check", "pe_fast_aggregate_verify"):
        assert re.search(r"\bint %s\s*\(" % name, boundary) and name in _abi.SIGNATURES
    assert re.search(r"\bint pe_profile_pairing_gt\s*\(", profile) and "pe_profile_pairing_gt" not in boundary
    assert "pe_profile_pairing_gt" in _abi.SIGNATURES
    # argument counts: the C declarations against the ctypes lists (handle included)
    for name, text in (("pe_pairing_check", boundary), ("pe_fast_aggregate_verify", boundary), ("pe_profile_pairing_gt", profile)):
        args = re.search(r"\bint %s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(args.split(",")) == len(_abi.SIGNATURES[name][1]), name
    assert int(re.search(r"#define\s+PE_ABI_VERSION\s+(\d+)", boundary).group(1)) == 15
    lib = _abi.load()
    for name in ("pe_pairing_check", "pe_fast_aggregate_verify", "pe_profile_pairing_gt"):
        assert hasattr(lib, name)
