"""gf_cluster_fit_feasible at the drop-in boundary (no GPU): declared in include/gangfit.h, exported by libgangfit.so, bound in
gangfit/_native.py, and refusing a NULL context before anything else.  Plus the CPU check of what the scan rests on: the
order-free predicate (some fitting driver candidate d with S - cap(d) + cap'(d) >= K, per zone for the single-AZ packers)
equals the oracle's HasCapacity for every packer on the cases the GPU test uses."""
import ctypes

import numpy as np

import cluster_scan_cases as cs
from gangfit import _native, build
from test_abi_overhead import _declared_symbols


def test_cluster_fit_feasible_is_declared_exported_and_bound():
    assert "gf_cluster_fit_feasible" in _declared_symbols()
    lib = ctypes.CDLL(build.build_native())
    assert hasattr(lib, "gf_cluster_fit_feasible")
    assert "gf_cluster_fit_feasible" in _native.EXPORTED_SYMBOLS
    L = _native.load()
    assert L.gf_cluster_fit_feasible.restype is ctypes.c_int32 and len(L.gf_cluster_fit_feasible.argtypes) == 9


def test_a_null_context_is_invalid():
    L = _native.load()
    apps = np.zeros(1, dtype=_native.APP_DTYPE)
    out = np.full(1, 0xAB, dtype=np.uint8)
    assert L.gf_cluster_fit_feasible(None, 0, None, None, None, None, 1, _native.ptr(apps), _native.ptr(out)) == _native.GF_ERR_INVALID
    assert out[0] == 0xAB


def test_the_order_free_predicate_is_the_oracles_answer():
    for n, n_zones in ((1, 1), (63, 3), (65, 64), (130, 3)):
        seed = cs.seed_of(n, n_zones)
        c = cs.cluster(seed, n, n_zones)
        drv, exe, k = cs.applications(seed, c)
        drop = c["zone"] != c["zone"][0]
        for select, over in ((np.ones(n, dtype=bool), None), (np.ones(n, dtype=bool), c["overhead"]), (drop, c["overhead"])):
            ref = cs.reference(c, select, drv, exe, k, overhead=over)
            for algo in cs.ALGOS:
                mine = [cs.predicate(c, select, drv[a], exe[a], int(k[a]), algo in cs.SINGLE_AZ, overhead=over)[0] for a in range(len(k))]
                assert np.array_equal(np.asarray(mine, dtype=np.uint8), ref[algo]), (n, n_zones, algo)
