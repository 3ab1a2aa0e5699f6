"""ISA-level checks of the three launches of hsv_signer_sign_msgs*
(hsv_msgsign.hip; no GPU: hipcc -S only, resource comments only).

The nonce and the response kernel are the verifier's message prepass with
another head and another ending: they may use no more scratch and reach no
fewer waves per SIMD than hsv_msg_prep_kernel (hsv_msgs.hip), and stage through
the same LDS.  The point kernel is sign_lane without its two hashes: it may be
no heavier than hsv_sign_kernel<G, true> (hsv_signer.hip) at the same G.
"""
import os
import re

import pytest

from conftest import PKG
from test_kernel_isa import HIPCC, _compile
from test_msgs_small_isa import resources

LDS_BYTES = 4 * 64 * 9 * 16  # 4 waves x 64 lanes x 9 chunks of 16 bytes


def waves_per_simd(vgprs):
    """512 VGPRs per SIMD lane, allocated in blocks of 8."""
    return 512 // ((vgprs + 7) // 8 * 8)


@pytest.fixture(scope="module")
def res():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = {}
    for f in ("hsv_msgsign", "hsv_msgs", "hsv_signer"):
        out[f] = resources(_compile(os.path.join(PKG, "csrc", f + ".hip"), f + ".hip.s"))
    return out


def one(table, pattern):
    names = [k for k in table if re.search(pattern, k)]
    assert len(names) == 1, (pattern, sorted(table))
    r = table[names[0]]
    assert set(r) == {"vgprs", "scratch", "lds"}, (names[0], r)
    return r


@pytest.mark.parametrize("kernel", ("hsv_msg_nonce_kernel", "hsv_msg_response_kernel"))
def test_hashing_kernels_are_no_heavier_than_the_message_prepass(res, kernel):
    k = one(res["hsv_msgsign"], kernel)
    prep = one(res["hsv_msgs"], "hsv_msg_prep_kernel")
    print(f"{kernel}: {k} waves/SIMD {waves_per_simd(k['vgprs'])}; hsv_msg_prep_kernel: {prep} "
          f"waves/SIMD {waves_per_simd(prep['vgprs'])}")
    assert k["scratch"] <= prep["scratch"], (k, prep)
    assert waves_per_simd(k["vgprs"]) >= waves_per_simd(prep["vgprs"]), (k, prep)
    assert k["lds"] == LDS_BYTES, k


@pytest.mark.parametrize("g", (1, 2, 4, 8, 16))
def test_point_kernel_is_no_heavier_than_the_fast_signing_kernel(res, g):
    # template arguments mangled: ILi<G>E for the point kernel, ILi<G>ELb1E for hsv_sign_kernel<G, true>
    p = one(res["hsv_msgsign"], r"hsv_msg_point_kernelILi%dEE" % g)
    s = one(res["hsv_signer"], r"hsv_sign_kernelILi%dELb1EE" % g)
    print(f"G={g}: point {p} waves/SIMD {waves_per_simd(p['vgprs'])}; hsv_sign_kernel<G, true> {s} "
          f"waves/SIMD {waves_per_simd(s['vgprs'])}")
    assert p["scratch"] <= s["scratch"], (g, p, s)
    assert waves_per_simd(p["vgprs"]) >= waves_per_simd(s["vgprs"]), (g, p, s)
