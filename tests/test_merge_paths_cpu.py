"""merge_paths (the host-side classification of the k > 64 merges) against a plain
NumPy sort, and the lattice constructions of merge_cases under the oracle alone:
every constructed distance is an exact integer and the keys fall where the GPU
tests rely on them."""
import numpy as np
import pytest

import merge_cases as mc
import merge_paths as mp
from oracle import oracle as O


def by_sort(u, k):
    """(passes, n) of the radix select from a full sort: the kernel leaves after pass 1 when
    the keys up to the end of the k-th key's 16-bit bucket number <= 128 (k <= 128), after
    pass 2 when those up to the end of its 24-bit bucket number <= 512, else after pass 4."""
    u = np.sort(np.asarray(u, np.uint32)).astype(np.int64)
    if u.size <= k:
        return 0, int(u.size)
    kth = int(u[k - 1])
    n16 = int(np.searchsorted(u, kth | 0xFFFF, side="right"))
    n24 = int(np.searchsorted(u, kth | 0xFF, side="right"))
    if k <= 128 and n16 <= 128:
        return 1, n16
    if n24 <= 512:
        return 2, n24
    return 4, int(np.searchsorted(u, kth, side="right"))


def key_sets():
    rng = np.random.default_rng(1)
    sets = {
        "uniform": rng.uniform(0, 100, 3000),
        "narrow": 1000 + rng.uniform(0, 1e-3, 3000),
        "both_signs": rng.normal(size=2500),
        "all_tied": np.full(1500, 3.5),
        "tied_zero_signs": np.where(np.arange(900) % 2 == 0, 0.0, -0.0),
        "ints": rng.integers(-40, 40, 2000).astype(np.float64),
        "one24": -(2.0 ** 23 + 256 * 7 + np.repeat(np.arange(256), 3)),
        "one16": -(2.0 ** 23 + 256 * np.arange(256) + (91 * np.arange(256)) % 256),
        "spread": -(256.0 * np.arange(256) + (37 * np.arange(256)) % 256),
        "few": rng.uniform(0, 1, 50),
        "exactly_k": rng.uniform(0, 1, 100),
    }
    return {n: np.asarray(v, np.float32) for n, v in sets.items()}


def test_ukeys_order_floats():
    v = np.array([-np.inf, -3e38, -1.5, -1e-30, -0.0, 0.0, 1e-30, 2.0, 3e38, np.inf], np.float32)
    u = mp.ukeys(v).astype(np.int64)
    assert u[4] == u[5]  # -0 folded into +0
    assert (np.diff(np.delete(u, 4)) > 0).all()
    assert u.max() < 0xFFFFFFFF


@pytest.mark.parametrize("k", [65, 100, 128, 129, 200, 300, 512])
@pytest.mark.parametrize("name", list(key_sets()))
def test_radix_select_matches_sort(name, k):
    u = mp.ukeys(key_sets()[name])
    passes, T, n = mp.radix_select(u, k)
    assert (passes, n) == by_sort(u, k)
    assert n == np.count_nonzero(u <= np.uint32(T))
    if passes:  # T is the k-th key with the digits not examined set: the k best are below or at it
        kth = int(np.sort(u)[k - 1])
        shift = {1: 16, 2: 8, 4: 0}[passes]
        assert T == kth | ((1 << shift) - 1) and n >= k


def test_radix_exits_all_reached():
    """The synthetic sets reach every exit and both sides of both buffer limits."""
    ks = key_sets()
    seen = {(n, k): mp.classify_query(mp.ukeys(v), 1, k) for n, v in ks.items() for k in (100, 128, 200)}
    assert seen["spread", 100]["passes"] == 1 and seen["spread", 100]["regsort"] and seen["spread", 100]["n"] == 100
    assert seen["spread", 200]["passes"] == 2 and not seen["spread", 200]["regsort"]
    assert seen["one16", 100]["passes"] == 2 and seen["one16", 100]["n"] == 100
    assert seen["one24", 100]["passes"] == 4 and seen["one24", 100]["n"] == 102 and seen["one24", 100]["regsort"]
    assert seen["one24", 128]["n"] == 129 and not seen["one24", 128]["regsort"] and not seen["one24", 128]["overflow"]
    assert seen["all_tied", 100]["overflow"] and seen["all_tied", 100]["n"] == 1500
    assert seen["tied_zero_signs", 128]["overflow"]
    assert seen["few", 100]["passes"] == 0 and seen["few", 100]["regsort"] and seen["few", 100]["n"] == 50
    assert seen["exactly_k", 100]["passes"] == 0 and seen["exactly_k", 100]["n"] == 100


def test_classify_arrays():
    """classify on synthetic (count, key) arrays: unscanned probes and entries past a list's
    count are ignored, the kernel follows (nprobe, k), the big merge's figures a plain sort."""
    rng = np.random.default_rng(2)
    nq, nprobe, k = 5, 8, 300
    keys = np.sort(rng.uniform(0, 10, size=(nq, nprobe, 4, k)).astype(np.float32), axis=-1)
    counts = rng.integers(0, k + 1, size=(nq, nprobe, 4))
    scanned = rng.random((nq, nprobe)) < 0.7
    scanned[0] = False
    counts[1] = k
    scanned[1] = True
    keys[2] = 1.25  # every entry tied
    counts[2], scanned[2] = k, True
    out = mp.classify(counts, keys, scanned, nprobe, k)
    for q in range(nq):
        u = np.sort(np.concatenate([keys[q, p, w, :counts[q, p, w]] for p in range(nprobe) if scanned[q, p]
                                    for w in range(4)] + [np.zeros(0, np.float32)]))
        c = out[q]
        assert c["kernel"] == "big" and c["C"] == u.size
        assert c["rounds_entered"] == (u.size > 600) and c["r"] == -(-u.size // 1280)
        want = u.size if u.size <= k else int(np.count_nonzero(u <= u[k - 1]))
        assert c["n_le_T"] == want and c["overflow_certain"] == (want > 2048)
    assert out[0]["C"] == 0 and mp.label(out[0]) == "big merged no rounds"
    assert out[1]["C"] == 32 * k and mp.label(out[1]) == "big merged r>1"
    assert mp.label(out[2]) == "big overflow"
    assert mp.kernel_for(6, 300) == "radix" and mp.kernel_for(7, 300) == "big"
    assert mp.kernel_for(8, 256) == "radix" and mp.kernel_for(64, 65) == "big" and mp.kernel_for(65, 65) == "full"
    assert mp.kernel_for(2, 1024) == "radix" and mp.kernel_for(3, 1024) == "big"
    r = mp.classify(counts[:, :2], keys[:, :2], scanned[:, :2], 2, k)
    assert all(c["kernel"] == "radix" for c in r) and r[2]["overflow"] and r[2]["n"] == 8 * k
    assert mp.label(mp.classify_query(mp.ukeys(keys[1].reshape(-1)), 65, k)) == "full"


def oracle_of(c):
    ox = O.OracleIVFPQ(mc.D, c.nlist, mc.M, metric=O.METRIC_INNER_PRODUCT if c.metric == mc.IP else O.METRIC_L2)
    ox.set_trained(c.cent, c.cb)
    ox.add_preencoded(c.list_no, c.codes, c.ids)
    return ox


def test_lattice_sims_exact_under_oracle():
    c = mc.lattice()
    ox = oracle_of(c)
    xq = mc.lattice_queries(3, zero=(2,))
    for l in mc.LAT_A:
        rows = np.full((3, 1), l, np.int64)
        n = int(c.sizes[l])
        Dr, Ir = ox.search_preassigned(xq, n, rows)
        want = np.sort(mc.lattice_sims(c, l))[::-1].astype(np.float32)
        assert want.astype(np.int64).max() < 2 ** 24
        np.testing.assert_array_equal(Dr[0], want)
        np.testing.assert_array_equal(Dr[1], want)
        assert (Dr[2] == 0).all() and (np.diff(Ir[2]) > 0).all()  # the zero query: ties, by label
    # where the keys fall: -sim as the merges see them
    def path(lists, k):
        u = mp.ukeys(-np.concatenate([mc.lattice_sims(c, l) for l in lists]).astype(np.float32))
        return mp.classify_query(u, len(lists), k)
    assert path([mc.LAT_SPREAD], 128)["passes"] == 1 and path([mc.LAT_SPREAD], 200)["passes"] == 2
    assert path([mc.LAT_ONE16], 100)["passes"] == 2 and path([mc.LAT_ONE16], 128)["n"] == 128
    assert path(mc.LAT_ONE24, 100)["passes"] == 4 and path(mc.LAT_ONE24, 200)["n"] == 201
    s = mc.lattice_sims(c, mc.LAT_SIGNS)
    assert 0 < (s > 0).sum() < 100 and (s == 0).sum() == 0
    s8 = np.concatenate([mc.lattice_sims(c, l) for l in mc.LAT_SIGNS8])
    assert 0 < (s8 > 0).sum() < 300


@pytest.mark.parametrize("metric", [mc.L2, mc.IP])
def test_tied_and_rounds_distances_are_integers(metric):
    c = mc.tied(metric, "interleave")
    ox = oracle_of(c)
    xq = mc.tied_queries(metric, 4)
    rows = np.tile(np.asarray([0, 3, mc.TIED_BETTER, 15, 16, 20, 21, 22], np.int64), (4, 1))
    Dr, Ir = ox.search_preassigned(xq, 100, rows, c.dis0(xq, rows))
    assert (Dr == np.round(Dr)).all()
    tk = mc.tied_key(metric, xq)
    # 30 better rows, then the tied ones, label order walking across both lists
    assert ((Dr[:, :30] < tk[:, None]) if metric == mc.L2 else (Dr[:, :30] > tk[:, None])).all()
    np.testing.assert_array_equal(Dr[:, 30:], np.repeat(tk[:, None], 70, 1))
    want = np.sort(np.concatenate([c.ids[c.list_no == 0], c.ids[c.list_no == 3]]))[:70]
    np.testing.assert_array_equal(Ir[:, 30:], np.tile(want, (4, 1)))
    assert set((want % 8).tolist()) == {0, 3}
    r = mc.rounds(metric)
    ox = oracle_of(r)
    xq = mc.rounds_queries(4)
    rows = np.tile(np.asarray([0, 13, 24, mc.RS_LONG, 90, 91], np.int64), (4, 1))
    Dr, _ = ox.search_preassigned(xq, 1000, rows, r.dis0(xq, rows))
    assert (Dr == np.round(Dr)).all() and np.abs(Dr).max() < 2 ** 24
    rows = np.full((4, 1), mc.RS_LONG, np.int64)
    Dr, _ = ox.search_preassigned(xq, mc.RS_LONG_ROWS, rows, r.dis0(xq, rows))
    for q in range(4):  # 8 distinct keys, 1024 rows each
        v, n = np.unique(Dr[q], return_counts=True)
        assert v.size == 8 and (n == 1024).all()
