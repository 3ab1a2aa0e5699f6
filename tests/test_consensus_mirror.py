"""The consensus half of the C++ mirror (include/hsv_crypto.hpp, namespace
consensus): Block, Vote and Timeout whose signature checks fill an
hsv_proposal (or the object's bincode bytes) and make one verification call.
tests/native/consensus_mirror.cpp signs a block with a QC and a TC, a vote and
a timeout with the mirror's own signer and checks the verdicts -- stage and
index -- without and with an explicit committee."""
import os
import subprocess

import pytest

from conftest import PKG, ROOT

BIN = os.path.join(ROOT, "build", "consensus_mirror")


@pytest.fixture(scope="module")
def mirror_bin():
    from hsverify import _lib
    _lib.load(require=True)  # libhsv.so must exist (built by __graft_entry__.build)
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    libdir = os.path.join(PKG, "hsverify")
    tmp = f"{BIN}.{os.getpid()}.tmp"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "csrc"),
                    os.path.join(ROOT, "tests", "native", "consensus_mirror.cpp"),
                    "-L", libdir, "-lhsv", f"-Wl,-rpath,{libdir}", "-lpthread", "-o", tmp], check=True)
    os.replace(tmp, BIN)
    return BIN


def test_consensus_mirror_raises_infrastructure_error_without_gpu(mirror_bin):
    """No GPU: the first verify is an InfrastructureError, never Err."""
    from hsverify import _lib
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    r = subprocess.run([mirror_bin], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3, (r.returncode, r.stderr[-800:])
    assert "InfrastructureError" in r.stderr and "no HIP device" in r.stderr


@pytest.mark.gpu
def test_consensus_mirror_verdicts_on_gpu(mirror_bin, hsv):
    r = subprocess.run([mirror_bin], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert "consensus mirror ok" in r.stdout
