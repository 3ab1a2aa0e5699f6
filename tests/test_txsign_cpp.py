"""hsv::Signer::sign_transactions, the C++ mirror of the transaction signer
(include/hsv_crypto.hpp): tests/native/txsign_mirror.cpp compiles against the
header and libhsv.so, signs transactions in place and has the mempool check
accept them."""
import os
import subprocess

import pytest

from conftest import PKG, ROOT

BIN = os.path.join(ROOT, "build", "txsign_mirror")


@pytest.fixture(scope="module")
def mirror_bin():
    from hsverify import _lib
    _lib.load(require=True)  # libhsv.so must exist
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    libdir = os.path.join(PKG, "hsverify")
    tmp = f"{BIN}.{os.getpid()}.tmp"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "txsign_mirror.cpp"), "-L", libdir, "-lhsv",
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


def test_mirror_declares_the_device_form():
    hdr = open(os.path.join(ROOT, "include", "hsv_crypto.hpp")).read()
    assert "void sign_transactions(" in hdr and "void sign_transactions_device(" in hdr


@pytest.mark.gpu
def test_mirror_signs_what_the_mempool_check_accepts(mirror_bin, hsv):
    r = subprocess.run([mirror_bin], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "all passed" in r.stdout
