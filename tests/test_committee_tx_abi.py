"""Argument checks of hsv_committee_verify_transactions* that need no GPU: they
are made before any device work."""
import ctypes

import numpy as np
import pytest

INVALID_ARG = -3


@pytest.fixture(scope="module")
def lib():
    from hsverify import _lib
    return _lib.load(require=True)


def test_empty_batch_is_ok_without_a_committee(lib):
    assert lib.hsv_committee_verify_transactions(None, None, None, 0, 0, None) == 0
    assert lib.hsv_committee_verify_transactions_device(None, None, None, 0, 0, None, None, None, None) == 0


def test_null_committee_is_an_argument_error(lib):
    txs = np.zeros(2 * 128, np.uint8)
    offsets = np.array([0, 128, 256], np.uint64)
    flags = np.full(2, 0xff, np.uint8)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    assert lib.hsv_committee_verify_transactions(None, p(txs), p(offsets), 0, 2, p(flags)) == INVALID_ARG
    assert lib.hsv_committee_verify_transactions(None, p(txs), None, 128, 2, p(flags)) == INVALID_ARG
    assert (flags == 0xff).all()
    assert lib.hsv_committee_verify_transactions_device(None, p(txs), None, 128, 2, p(flags), None, None,
                                                        None) == INVALID_ARG
    from hsverify import _lib
    assert "null" in _lib.last_error()


def test_device_form_needs_an_output(lib):
    txs = np.zeros(2 * 128, np.uint8)
    assert lib.hsv_committee_verify_transactions_device(None, ctypes.c_void_p(txs.ctypes.data), None, 128, 2, None,
                                                        None, None, None) == INVALID_ARG


class _NoCommittee:
    """Committee's wrappers over a NULL handle (a committee cannot be built
    without a device)."""

    def __init__(self):
        from hsverify import _lib
        self._lib = _lib.load()
        self._h = None


def test_python_wrappers_raise_on_those_codes(lib):
    from hsverify import _lib, mempool
    from hsverify.committee import Committee
    for name in ("verify_transactions", "verify_transactions_fixed", "verify_transactions_device"):
        assert callable(getattr(Committee, name))
    c = _NoCommittee()
    with pytest.raises(_lib.HsvLibraryError, match="HSV_ERR_INVALID_ARG"):
        Committee.verify_transactions(c, [bytes(128), bytes(200)])
    with pytest.raises(_lib.HsvLibraryError, match="HSV_ERR_INVALID_ARG"):
        Committee.verify_transactions_fixed(c, np.zeros((3, 128), np.uint8))
    import torch
    t, f = torch.zeros(256, dtype=torch.uint8), torch.zeros(2, dtype=torch.uint8)
    with pytest.raises(_lib.HsvLibraryError, match="HSV_ERR_INVALID_ARG"):  # refused before the pointers matter
        Committee.verify_transactions_device(c, t, None, tx_size=128, flags=f, stream=0)
    assert Committee.verify_transactions(c, []).size == 0
    assert Committee.verify_transactions_fixed(c, np.zeros((0, 128), np.uint8)).size == 0
    # the mempool call shapes take the committee as a keyword; None keeps them as they were
    assert mempool.verify_batch_transactions([], committee=None) is True
    assert mempool.filter_transactions([], committee=None) == []
