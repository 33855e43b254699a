"""gf_cluster_fit_feasible_sets at the drop-in boundary (no GPU): declared in include/gangfit.h, exported by libgangfit.so, bound
in gangfit/_native.py with its eleven arguments, refusing a NULL context before anything else; and the binding's bit packing
(gangfit.pack_node_sets) against rows written out by hand: bit (n & 63) of word n >> 6 = node n, little-endian, the padding 0."""
import ctypes

import numpy as np
import pytest

import gangfit
from gangfit import _native, build
from test_abi_overhead import _declared_symbols


def test_cluster_fit_feasible_sets_is_declared_exported_and_bound():
    assert "gf_cluster_fit_feasible_sets" in _declared_symbols()
    lib = ctypes.CDLL(build.build_native())
    assert hasattr(lib, "gf_cluster_fit_feasible_sets")
    assert "gf_cluster_fit_feasible_sets" in _native.EXPORTED_SYMBOLS
    L = _native.load()
    assert L.gf_cluster_fit_feasible_sets.restype is ctypes.c_int32 and len(L.gf_cluster_fit_feasible_sets.argtypes) == 11


def test_a_null_context_is_invalid():
    L = _native.load()
    apps = np.zeros(1, dtype=_native.APP_DTYPE)
    words = np.ones(1, dtype=np.uint64)
    app_set = np.zeros(1, dtype=np.uint32)
    out = np.full(1, 0xAB, dtype=np.uint8)
    rc = L.gf_cluster_fit_feasible_sets(None, 0, None, None, None, 1, _native.ptr(words), _native.ptr(app_set), 1, _native.ptr(apps),
                                        _native.ptr(out))
    assert rc == _native.GF_ERR_INVALID and out[0] == 0xAB


# (n_nodes, nodes of the set, the row by hand)
HAND = [
    (1, [0], [0x1]),
    (63, [0, 5, 62], [0x4000000000000021]),
    (64, [63], [0x8000000000000000]),
    (64, [0, 1, 32], [0x0000000100000003]),
    (65, [64], [0x0, 0x1]),                                   # the only node of the last chunk
    (65, [0, 63, 64], [0x8000000000000001, 0x1]),
    (130, [129], [0x0, 0x0, 0x2]),                            # the last node, in the last chunk
    (130, [7, 64, 100, 128], [0x80, 0x0000001000000001, 0x1]),
]


@pytest.mark.parametrize("n, nodes, row", HAND)
def test_the_bit_packing_equals_a_row_written_by_hand(n, nodes, row):
    sets = np.zeros((2, n), dtype=bool)
    sets[1, nodes] = True  # row 0 stays empty
    words = gangfit.pack_node_sets(sets, n)
    assert words.dtype == np.uint64 and words.flags["C_CONTIGUOUS"] and words.shape == (2, (n + 63) // 64)
    assert [int(w) for w in words[1]] == row and not words[0].any()
    assert words[1].tobytes() == b"".join(int(w).to_bytes(8, "little") for w in row)


def test_a_full_row_has_no_bit_behind_the_last_node():
    for n in (1, 63, 64, 65, 130):
        words = gangfit.pack_node_sets(np.ones((1, n), dtype=np.uint8), n)
        assert sum(bin(int(w)).count("1") for w in words[0]) == n
        assert int(words[0, -1]) == (1 << ((n - 1) % 64 + 1)) - 1
