"""hsv::Signer::sign_msgs, the C++ mirror of the message signer
(include/hsv_crypto.hpp): tests/native/msgsign_mirror.cpp compiles against the
header and libhsv.so, signs messages of differing lengths in one call, and has
hsv_sign agree byte for byte and hsv_verify_msgs accept them."""
import os
import subprocess

import pytest

from conftest import PKG, ROOT

BIN = os.path.join(ROOT, "build", "msgsign_mirror")


@pytest.fixture(scope="module")
def mirror_bin():
    from hsverify import _lib
    _lib.load(require=True)  # libhsv.so must exist
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    libdir = os.path.join(PKG, "hsverify")
    tmp = f"{BIN}.{os.getpid()}.tmp"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "msgsign_mirror.cpp"), "-L", libdir, "-lhsv",
                    f"-Wl,-rpath,{libdir}", "-lpthread", "-o", tmp], check=True)
    os.replace(tmp, BIN)
    return BIN


def test_mirror_compiles_and_raises_infrastructure_error_without_gpu(mirror_bin):
    from hsverify import _lib
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    r = subprocess.run([mirror_bin], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3, (r.stdout, r.stderr)
    assert "InfrastructureError" in r.stderr and "hsv_signer_create" in r.stderr


def test_mirror_declares_both_forms():
    hdr = open(os.path.join(ROOT, "include", "hsv_crypto.hpp")).read()
    assert "std::vector<uint8_t> sign_msgs(" in hdr and "void sign_msgs_device(" in hdr


@pytest.mark.gpu
def test_mirror_signs_what_the_host_signer_signs(mirror_bin, hsv):
    r = subprocess.run([mirror_bin], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "all passed" in r.stdout
