"""Inputs of the many-sets capacity scan tests (gf_cluster_fit_feasible_sets): the clusters of cluster_scan_cases, families of
node sets that sit on the edges of the kernel's row walk (64 nodes a word, 64 words a group), seventy applications dealt over a
family's sets whose executor counts sit on the capacity edges of their OWN set, and the reference answer: the CPU oracle on the
snapshot of every set by itself, for the applications of that set.  An empty set needs no oracle: the reference packs onto no
node, so no driver candidate exists and every application is turned down."""
import functools

import numpy as np

import cluster_scan_cases as cs

GROUP = 64 * 64                                   # nodes one group of 64 row words covers
SMALL = cs.NODE_COUNTS                            # the chunk edges of the one-set scan
LARGE = (GROUP - 1, GROUP, GROUP + 1, GROUP + 65)  # the group edges: one group short of a node, full, a second group of 1 and 65 nodes
NODE_COUNTS = SMALL + LARGE
ZONE_COUNTS = cs.ZONE_COUNTS
N_APPS = cs.N_APPS
MANY_SETS_AT = 130                                # the size that also gets 65 sets: more rows than a wavefront has lanes


def families_of(n):
    """The family names of a size.  `second_group` needs a node at or behind 4 096: at 4 095 and 4 096 nodes no such node exists
    (the set would be the empty set, which `empty` covers), so the family starts at 4 097."""
    names = ["contiguous", "scattered", "overlapping", "full", "empty", "last", "gaps"]
    if n > GROUP:
        names.append("second_group")
    if n == MANY_SETS_AT:
        names.append("many")
    return names


def CASES():
    return [(n, z, f) for n in NODE_COUNTS for z in ZONE_COUNTS for f in families_of(n)]


def sets_of(family, n):
    """(n_sets, n) truth array"""
    i = np.arange(n)
    if family == "contiguous":      # three instance groups one behind the other
        cut = [0, n // 3, (2 * n) // 3, n]
        rows = [(i >= cut[s]) & (i < cut[s + 1]) for s in range(3)]
    elif family == "scattered":     # ... dealt node by node
        rows = [i % 3 == s for s in range(3)]
    elif family == "overlapping":
        rows = [i < (2 * n + 2) // 3, i >= n // 3, i % 2 == 0]
    elif family == "full":
        rows = [np.ones(n, dtype=bool)]
    elif family == "empty":         # an empty set between two others
        rows = [i < (n + 1) // 2, np.zeros(n, dtype=bool), i % 2 == n % 2]
    elif family == "last":          # the last bit of the last word
        rows = [i == n - 1]
    elif family == "gaps":          # words 0, 2, 5, 8, ... and the last one; every other word of the row is zero
        w = i // 64
        rows = [((w == 0) | (w % 3 == 2) | (w == (n - 1) // 64)) & (i % 5 != 1)]
    elif family == "second_group":  # the first group's 64 words are all zero
        rows = [i >= GROUP, i < GROUP]
    elif family == "many":
        rows = [(i * 7 + s) % 65 < 24 for s in range(65)]
    else:
        raise KeyError(family)
    return np.stack(rows).astype(bool)


# Seeds at which the ORACLE alone answers at least five applications each way for every packer, with and without the overhead,
# over the applications of the family's non-empty sets together (searched once on the CPU; the tests assert it on every run).
# The default is cluster_scan_cases.seed_of's; the entries below are the cases where that one misses.
_SEEDS = {
    (4095, 1, 'last'): 4095037,
    (4095, 3, 'empty'): 4095032,
    (4095, 3, 'last'): 4095037,
    (4095, 64, 'empty'): 4095642,
    (4095, 64, 'last'): 4095641,
    (4096, 1, 'last'): 4096011,
    (4096, 3, 'empty'): 4096032,
    (4096, 3, 'last'): 4096039,
    (4096, 64, 'contiguous'): 4096641,
    (4096, 64, 'empty'): 4096642,
    (4096, 64, 'last'): 4096645,
    (4096, 64, 'overlapping'): 4096641,
    (4096, 64, 'scattered'): 4096641,
    (4097, 1, 'last'): 4097014,
    (4097, 64, 'last'): 4097650,
    (4097, 64, 'second_group'): 4097642,
    (4161, 1, 'last'): 4161018,
    (4161, 3, 'empty'): 4161031,
    (4161, 3, 'last'): 4161037,
    (4161, 64, 'empty'): 4161641,
    (4161, 64, 'last'): 4161641,
}


def seed_of(n, n_zones, family):
    return _SEEDS.get((n, n_zones, family), cs.seed_of(n, n_zones))


N_MIXED = 8
MIXED_K = (1, 2, 3, 5, 12, 30, 64, 100)


def n_apps_of(n):
    """Seventy applications at the small sizes.  At the group edges the oracle's time grows with nodes x executors, so the cases
    there ask twenty-four applications (every edge twice) whose executors are sixteen-fold and take a node's eight gpus: the gpu
    minority holds one each, a few hundred in all, and the walk over four thousand nodes is what these sizes are about.  Eight
    more (N_MIXED) are the ordinary cpu- and memory-bound applications with a small executor count, so every node of a set is a
    driver candidate and holds executors: they fit a large set at the first candidate and split on a set of one node."""
    return N_APPS if n <= max(SMALL) else 24 + N_MIXED


def applications(seed, c, sets, app_set):
    """cluster_scan_cases.applications with every application's executor-count edges taken on its own set (without the overhead;
    the same applications are asked with it)."""
    rng = np.random.default_rng(seed + 7)
    GIB = cs.GIB
    n_apps = len(app_set)
    big = 1 if len(c["alloc"]) <= max(SMALL) else 16
    n_edge = n_apps if big == 1 else n_apps - N_MIXED

    def shapes(r, count):
        return (np.stack([r.choice([500, 1000, 2000, 4000], size=count), r.choice([1, 2, 4, 8], size=count) * GIB,
                          (r.random(count) < 0.1).astype(np.int64)], axis=1).astype(np.int64),
                np.stack([r.choice([1000, 2000, 4000, 8000], size=count), r.choice([2, 4, 8, 16, 32], size=count) * GIB,
                          (r.random(count) < 0.2).astype(np.int64)], axis=1).astype(np.int64))

    drv, exe = shapes(rng, n_edge)
    exe[:, :2] *= big
    if big > 1:
        exe[:, 2] = 8
        drv[:, 2] = 1  # (an application that does not fit costs the oracle a packing per driver candidate: the gpu minority only)
    exe[3, 1] = 0  # a dimension that never limits
    exe[4, 0] = 0
    k = np.zeros(n_apps, dtype=np.int64)
    if big > 1:  # the mixed tail: no gpu anywhere, executors of the ordinary size, a small count
        mdrv, mexe = shapes(np.random.default_rng(seed + 11), N_MIXED)
        mdrv[:, 2] = 0
        mexe[:, 2] = 0
        drv, exe = np.concatenate([drv, mdrv]), np.concatenate([exe, mexe])
        k[n_edge:] = MIXED_K
    for a in range(n_edge):
        row = sets[app_set[a]]
        d, e = [int(v) for v in drv[a]], [int(v) for v in exe[a]]
        _, s, total = cs.predicate(c, row, d, e, 1 << 20, per_zone=False)
        _, zs, ztotal = cs.predicate(c, row, d, e, 1 << 20, per_zone=True)
        edges = [0, 1, total, total + 1, s, ztotal, ztotal + 1, 3 * s + 5, total // 2, int(rng.integers(0, max(s, 1) + 1)), 2, zs]
        # the applications of one set walk the edges one after the other, every set from another start
        k[a] = min(max(edges[(a // len(sets) + 5 * int(app_set[a])) % len(edges)], 0), 1 << 20)
    return drv, exe, k.astype(np.int32)


def reference(c, sets, app_set, drv, exe, k, overhead=None):
    """{algo: HasCapacity bytes}: cluster_scan_cases.reference per set, for the applications of that set"""
    out = {algo: np.zeros(len(k), dtype=np.uint8) for algo in cs.ALGOS}
    for s, row in enumerate(sets):
        idx = np.nonzero(app_set == s)[0]
        if len(idx) == 0 or not row.any():
            continue  # (an empty set: nothing to pack onto, HasCapacity false)
        ref = cs.reference(c, row, drv[idx], exe[idx], k[idx], overhead=overhead)
        for algo in cs.ALGOS:
            out[algo][idx] = ref[algo]
    return out


def answers_both_ways(case):
    """the condition on the inputs: per packer and overhead, (fits, does not fit) among the applications of the non-empty sets"""
    live = case["sets"].any(axis=1)[case["app_set"]]
    return {(algo, with_over): (int(ref[algo][live].sum()), int((ref[algo][live] == 0).sum()))
            for with_over, ref in ((False, case["ref"]), (True, case["ref_over"])) for algo in cs.ALGOS}


@functools.lru_cache(maxsize=None)
def case(n, n_zones, family, seed=None):
    """Everything a test needs of one (size, zone count, family), computed once and shared: treat it as read-only."""
    seed = seed_of(n, n_zones, family) if seed is None else seed
    c = cs.cluster(seed, n, n_zones)
    sets = sets_of(family, n)
    app_set = (np.arange(n_apps_of(n)) % len(sets)).astype(np.uint32)  # interleaved: neighbours in a workgroup ask different sets
    drv, exe, k = applications(seed, c, sets, app_set)
    return dict(c=c, sets=sets, app_set=app_set, drv=drv, exe=exe, k=k,
                ref=reference(c, sets, app_set, drv, exe, k), ref_over=reference(c, sets, app_set, drv, exe, k, overhead=c["overhead"]))
