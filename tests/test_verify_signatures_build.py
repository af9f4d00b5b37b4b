"""CPU: the build side of pe_verify_signatures -- the header and the binding agree on the new entry points, the profile hooks stay
out of the boundary header, and no kernel of sigverify_kernels.hip uses scratch memory (a resource log of its own)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pos_evolution_amd", "csrc")
PUBLIC = ("pe_verify_signatures",)
HOOKS = ("pe_profile_verify_set_stripe", "pe_profile_verify_stats", "pe_profile_verify_sums")


def test_header_and_binding_agree_on_the_entry_points():
    from pos_evolution_amd import _abi
    boundary = open(os.path.join(ROOT, "include", "posevo.h")).read()
    profile = open(os.path.join(ROOT, "include", "posevo_profile.h")).read()
    for names, text in ((PUBLIC, boundary), (HOOKS, profile)):
        for name in names:
            args = re.search(r"\bint %s\s*\(([^)]*)\)" % name, text).group(1)
            assert len(args.split(",")) == len(_abi.SIGNATURES[name][1]), name     # handle included
    for name in HOOKS:
        assert name not in boundary                                                 # measurement is not boundary
    doc = re.search(r"/\*((?:(?!\*/).)*)\*/\s*#define PE_SIG_STATUS_IDENTITY", boundary, re.S).group(1).lower()
    assert "unpredictable" in doc
    assert int(re.search(r"#define\s+PE_SIG_STATUS_IDENTITY\s+(\d+)", boundary).group(1)) == _abi.PE_SIG_STATUS_IDENTITY
    lib = _abi.load()
    for name in PUBLIC + HOOKS:
        assert hasattr(lib, name), name


def test_python_surface():
    from pos_evolution_amd import engine, forkchoice
    assert callable(engine.Engine.verify_signatures)
    assert callable(forkchoice.verify_attestation_signatures)


def test_no_kernel_of_the_weighted_sums_uses_scratch():
    log = open(os.path.join(CSRC, "sigverify_kernels.resource.log")).read()
    names = re.findall(r"Function Name: (\S+)", log)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", log)]
    assert len(names) == len(scratch) >= 5
    for want in ("k_g2_weighted_accumulate", "k_g1_weighted_accumulate", "k_sv_mark_identity", "k_sv_rows_g1", "k_sv_rows_g2"):
        assert any(want in n for n in names), want
    assert all(v == 0 for v in scratch), list(zip(names, scratch))
    # the plain sums keep their own logs, and the new file builds none of their kernels again
    for other in ("g2_kernels", "g1_kernels", "bls_batch_kernels"):
        old = re.findall(r"Function Name: (\S+)", open(os.path.join(CSRC, other + ".resource.log")).read())
        assert not set(old) & set(names), other


def test_the_stripe_of_the_model_is_the_handles():
    from tests import verify_signatures_model as vm
    internal = open(os.path.join(CSRC, "engine_internal.h")).read()
    assert int(re.search(r"verify_stripe\s*=\s*(\d+)", internal).group(1)) == vm.STRIPE
    profile = open(os.path.join(ROOT, "include", "posevo_profile.h")).read()
    kernels = open(os.path.join(CSRC, "kernels.h")).read()
    assert (int(re.search(r"PE_VERIFY_STRIPE_MAX\s+(\d+)", profile).group(1))
            == int(re.search(r"SV_STRIPE_MAX\s*=\s*(\d+)", kernels).group(1)) == 16)        # a plane's mask is 16 bits
