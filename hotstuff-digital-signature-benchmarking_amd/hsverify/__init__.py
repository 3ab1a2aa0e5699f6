"""hsverify -- MI355X-native Ed25519 batch verification for the HotStuff crypto crate.

Layers (top to bottom):
  hsverify.crypto    mirror of the reference's crypto crate API (crypto/src/lib.rs)
  hsverify.verifier  array / device-tensor entry points
  hsverify.mempool   transaction-signature checks (mempool/src/batch_maker.rs:79-85)
  hsverify.signer    batch key derivation and signing on the GPU (load generation)
  hsverify._lib      ctypes binding of libhsv.so (C ABI, include/hsv.h)
  csrc/              gfx950 HIP kernels + C ABI + host signing
"""
from ._lib import (A_OK, EQ_OK, PARSE_OK, R_OK, S_OK, SMALL_A, SMALL_R, STRICT_OK,  # noqa: F401
                   HsvLibraryError, LIB_PATH, device_count, load, version)
from .signer import Signer  # noqa: F401
from .verifier import verify_msgs, verify_msgs_device  # noqa: F401

__all__ = ["crypto", "verifier", "mempool", "signer", "Signer", "verify_msgs", "verify_msgs_device", "load", "device_count", "version", "HsvLibraryError",
           "STRICT_OK", "EQ_OK", "PARSE_OK", "SMALL_A", "SMALL_R", "S_OK", "A_OK", "R_OK"]
