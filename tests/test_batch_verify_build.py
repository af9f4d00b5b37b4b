"""CPU: the build side of pe_batch_verify -- the header and the binding agree on the new entry points, the profile hooks stay out
of the boundary header, and no kernel of bls_batch_kernels.hip uses scratch memory (a resource log of its own)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pos_evolution_amd", "csrc")
PUBLIC = ("pe_batch_verify", "pe_batch_fast_aggregate_verify")
HOOKS = ("pe_profile_batch_set_chunk", "pe_profile_batch_stats", "pe_profile_batch_gt")


def test_header_and_binding_agree_on_the_batch_entry_points():
    from pos_evolution_amd import _abi
    boundary = open(os.path.join(ROOT, "include", "posevo.h")).read()
    profile = open(os.path.join(ROOT, "include", "posevo_profile.h")).read()
    for names, text in ((PUBLIC, boundary), (HOOKS, profile)):
        for name in names:
            args = re.search(r"\bint %s\s*\(([^)]*)\)" % name, text).group(1)
            assert len(args.split(",")) == len(_abi.SIGNATURES[name][1]), name     # handle included
    for name in HOOKS:
        assert name not in boundary                                                 # measurement is not boundary
    assert int(re.search(r"#define\s+PE_ABI_VERSION\s+(\d+)", boundary).group(1)) == 15    # additions only
    assert "unpredictable" in re.search(r"/\*((?:(?!\*/).)*)\*/\s*int pe_batch_verify", boundary, re.S).group(1).lower()
    lib = _abi.load()
    for name in PUBLIC + HOOKS:
        assert hasattr(lib, name), name


def test_python_surface():
    from pos_evolution_amd import engine, forkchoice
    for name in ("batch_verify", "batch_fast_aggregate_verify"):
        assert callable(getattr(engine.Engine, name))
    assert callable(forkchoice.batch_fast_aggregate_verify)


def test_no_kernel_of_the_batch_path_uses_scratch():
    log = open(os.path.join(CSRC, "bls_batch_kernels.resource.log")).read()
    names = re.findall(r"Function Name: (\S+)", log)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", log)]
    assert len(names) == len(scratch) >= 5
    for want in ("k_bls_batch_settle", "k_bls_scale_g1", "k_bls_scale_g2", "k_bls_chunk_sig", "k_bls_gt_product"):
        assert any(want in n for n in names), want
    assert all(v == 0 for v in scratch), list(zip(names, scratch))
    # the per-group kernels keep their own log, and the new file builds none of them again
    old = re.findall(r"Function Name: (\S+)", open(os.path.join(CSRC, "bls_kernels.resource.log")).read())
    assert not set(old) & set(names)


def test_fan_in_of_the_model_is_the_kernels():
    from tests import batch_verify_model as bm
    text = open(os.path.join(CSRC, "kernels.h")).read()
    assert int(re.search(r"BLS_BATCH_FAN\s*=\s*(\d+)", text).group(1)) == bm.FAN
    internal = open(os.path.join(CSRC, "engine_internal.h")).read()
    assert int(re.search(r"batch_chunk\s*=\s*(\d+)", internal).group(1)) == bm.CHUNK
