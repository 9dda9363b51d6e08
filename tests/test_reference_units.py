"""Bit-exact checks of the building blocks against the reference's own translation units that compile on their own
(random.c, decomposition.c, parallel.c -> oracle/_ref/libcomd_ref.so, built by oracle/Makefile when the reference checkout is present).
What that library computes is stored in tests/golden/reference_rng_streams.json: the checks always run against the stored streams, and
against the library itself as well wherever it was built."""
import ctypes
import json
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "libcomd_ref.so")
GOLDEN = json.load(open(os.path.join(HERE, "golden", "reference_rng_streams.json")))


@pytest.fixture(scope="module")
def ref():
    """The reference's streams: the stored ones, checked against the live library when it exists."""
    stored = [(s0, s1, tuple(float.fromhex(v) for v in vals)) for s0, s1, vals in GOLDEN["streams"]]
    assert GOLDEN["ids"] == IDS and len(stored) == 2 * len(IDS)
    if os.path.exists(REF):
        assert _streams(_ref_lib(), ("lcg61", "gasdev", "mkSeed"), IDS) == stored
    return stored


def _ref_lib():
    L = ctypes.CDLL(REF)
    L.lcg61.argtypes = [ctypes.POINTER(ctypes.c_uint64)]
    L.lcg61.restype = ctypes.c_double
    L.gasdev.argtypes = [ctypes.POINTER(ctypes.c_uint64)]
    L.gasdev.restype = ctypes.c_double
    L.mkSeed.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    L.mkSeed.restype = ctypes.c_uint64
    return L


def _streams(L, names, ids):
    lcg, gas, mk = (getattr(L, n) for n in names)
    out = []
    for gid in ids:
        for site in (123, 457):
            s = ctypes.c_uint64(mk(gid, site))
            seed0 = s.value
            vals = [lcg(ctypes.byref(s)) for _ in range(4)] + [gas(ctypes.byref(s)) for _ in range(3)]
            out.append((seed0, s.value, tuple(vals)))
    return out


IDS = [0, 1, 2, 3, 31999, 2047999, 16383999, 67108863, 2**31 - 1, 2**32 - 1]


def test_oracle_rng_is_the_reference_rng(ref, orc):
    got = _streams(orc.lib(), ("oracle_lcg61", "oracle_gasdev", "oracle_mkSeed"), IDS)
    assert got == ref


def test_product_rng_is_the_reference_rng(ref, pkg):
    host = pkg.lib_host()
    host.lcg61.argtypes = [ctypes.POINTER(ctypes.c_uint64)]
    host.lcg61.restype = ctypes.c_double
    host.gasdev.argtypes = [ctypes.POINTER(ctypes.c_uint64)]
    host.gasdev.restype = ctypes.c_double
    host.mkSeed.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    host.mkSeed.restype = ctypes.c_uint64
    assert _streams(host, ("lcg61", "gasdev", "mkSeed"), IDS) == ref
