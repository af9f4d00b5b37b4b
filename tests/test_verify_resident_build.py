"""CPU: the build side of pe_verify_resident -- the library exports the call and its stats hook, and neither kernel of
bls_resident_kernels.hip uses scratch memory (a resource log of its own).  Skipped where the library is not built."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pos_evolution_amd", "csrc")
LOG = os.path.join(CSRC, "bls_resident_kernels.resource.log")

pytestmark = pytest.mark.skipif(not os.path.exists(LOG) or not os.path.exists(os.path.join(ROOT, "pos_evolution_amd", "libposevo.so")),
                                reason="libposevo.so is not built")


def test_neither_kernel_uses_scratch():
    log = open(LOG).read()
    names = re.findall(r"Function Name: (\S+)", log)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", log)]
    assert len(names) == len(scratch) == 2
    for want in ("k_bls_resident_prepare", "k_bls_resident_settle"):
        assert any(want in n for n in names), want
    assert all(v == 0 for v in scratch), list(zip(names, scratch))
    # the long kernels are reused, not built again: they keep their own log
    old = re.findall(r"Function Name: (\S+)", open(os.path.join(CSRC, "bls_kernels.resource.log")).read())
    assert not set(old) & set(names)


def test_wave_priority_is_not_raised():
    text = open(os.path.join(CSRC, "bls_resident_kernels.hip")).read()
    code = re.sub(r"//[^\n]*", "", text)
    assert "setprio" not in code and "asm" not in code


def test_the_library_exports_the_call_and_its_hook():
    from pos_evolution_amd import _abi
    lib = _abi.load()
    for name in ("pe_verify_resident", "pe_profile_verify_resident_stats"):
        assert hasattr(lib, name), name
