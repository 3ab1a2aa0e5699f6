#!/usr/bin/env python3
"""The host build's lattice answers, as a fixture for the GPU test.

tests/test_prims_gpu.py compares lattice_reduce on the device word for word
with the host build of the same text (csrc/hsv_lattice.hpp through
csrc/hsv_test_prims.hpp).  A GPU machine runs no host build of the headers, so
the host's answers travel as recorded output: for each bound of
prim_vectors.LATTICE_BOUNDS (133, 138) and each challenge of
prim_vectors.lattice_ks(), in that order, 12 little-endian 32-bit words
    ok, c0_neg, c0[5], c1[5]
as tests/native/prims_host.cpp --scalar prints them.
tests/test_prims_host.py asserts that the committed file is what this script
produces now.

Output: tests/golden/lattice_prims.bin.
Run from the repo root (needs g++):  python tests/golden/make_lattice_prims.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))

import numpy as np  # noqa: E402

import prim_vectors as pv  # noqa: E402


def generate(binary):
    """The fixture's bytes from a built prims_host."""
    ks = pv.lattice_ks()
    parts = []
    for bits in pv.LATTICE_BOUNDS:
        out = pv.run_prims_host(binary, "scalar", pv.lattice_records(ks, bits))
        assert (out[:, 0] == pv.DONE).all()
        parts.append(np.ascontiguousarray(out[:, 1:13], dtype="<u4"))
    return np.concatenate(parts).tobytes()


if __name__ == "__main__":
    data = generate(pv.build_prims_host())
    with open(pv.LATTICE_FIXTURE, "wb") as f:
        f.write(data)
    print(f"{pv.LATTICE_FIXTURE}: {len(data)} bytes")
