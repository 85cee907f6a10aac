"""The three device merges behind every k > 64 result (k_merge_radix, k_merge_big and
k_merge_probes<R>'s full merge, ivfpq_kernels.hip), each reached on purpose.

Every case builds a tiny hand-made index (merge_cases.py: d = 32, M = 8, integer
lattice, so keys are exact and ties are intended), searches it, compares D and I
with the CPU oracle bit for bit, and then asserts through merge_paths.py -- from the
partial lists the scan left in the workspace -- that every designated query took
the path the case is named for: which kernel, which exit of the radix select, which
final sort, whether the sampled rounds ran and at which stride, and whether the
query overflowed its kernel's buffer and was handed to the full merge.  A case
that misses its path fails.

Lists of at most 256 rows give every scan wave fewer than k rows, so no bound is
ever published and a query's candidate count is the sum of its lists' sizes; the
long lists hold tied rows, which the bound always admits.  Both make the
classification independent of timing.

Each printed "PATHS" line counts the classes of one search.
"""
import collections
import functools

import numpy as np
import pytest

import faiss_amd as faiss
import merge_cases as mc
import merge_paths as mp
from oracle import oracle as O

pytestmark = pytest.mark.gpu

METRICS = [mc.L2, mc.IP]
FMAX = np.finfo(np.float32).max


def rows_for(k):
    return 2 if k <= 128 else 4 if k <= 256 else 8 if k <= 512 else 16


@functools.lru_cache(maxsize=None)
def contents(name, *args):
    c = getattr(mc, name)(*args)
    ox = O.OracleIVFPQ(mc.D, c.nlist, mc.M, metric=O.METRIC_INNER_PRODUCT if c.metric == mc.IP else O.METRIC_L2)
    ox.set_trained(c.cent, c.cb)
    ox.add_preencoded(c.list_no, c.codes, c.ids)
    return c, ox


def gpu_index(c):
    ix = faiss.IndexIVFPQ(None, mc.D, c.nlist, mc.M, 8,
                          faiss.METRIC_INNER_PRODUCT if c.metric == mc.IP else faiss.METRIC_L2, device=0)
    ix.set_trained(c.cent, c.cb)
    ix.add_preencoded(c.list_no, c.codes, c.ids)
    return ix


def run(c, ox, xq, k, rows=None, nprobe=None, ix=None, grown=False):
    """One search (preassigned `rows`, or the plain search at `nprobe`) on a fresh handle
    (or on `ix`) against the oracle; returns the queries' paths and the oracle's (D, I)."""
    ix = ix or gpu_index(c)
    np_ = rows.shape[1] if rows is not None else nprobe
    ix.nprobe = ox.nprobe = np_
    rs0 = ix.repair_stats()
    ep = mp.epochs(ix)
    if rows is None:
        ref = ox.search(xq, k)
        got = ix.search(xq, k)
    else:
        dq = c.dis0(xq, rows)
        ref = ox.search_preassigned(xq, k, rows, dq)
        got = ix.search_preassigned(xq, k, rows, dq)
    paths = mp.read(ix, ep, xq.shape[0], np_, k, grown=grown)
    labels = [mp.label(p) + (f" R={rows_for(k)}" if p["kernel"] == "full" else "") for p in paths]
    print("PATHS", c.metric, f"k={k} nprobe={np_}", dict(collections.Counter(labels)))
    bad = np.nonzero((got[1] != ref[1]).any(1) | (got[0] != ref[0]).any(1))[0]
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[0], ref[0]), \
        f"queries {bad.tolist()} differ from the oracle; paths {[labels[q] for q in bad]}"
    assert ix.error_count() == 0
    assert ix.repair_stats() == rs0
    return paths, ref


def expect(paths, qs, **want):
    """Every query of qs has exactly these path fields."""
    for q in qs:
        got = {f: paths[q][f] for f in want}
        assert got == want, f"query {q} missed its path: {paths[q]}, wanted {want}"


def padded(ref, q, n, ip):
    """The oracle's row q holds n results and then padding (which the GPU equals bit for bit)."""
    D, I = ref
    assert (I[q, :n] >= 0).all() and (I[q, n:] == -1).all()
    assert (D[q, n:] == (-FMAX if ip else FMAX)).all()


def tied_rows(nq, nprobe, ntied, fill, first=0):
    """Row q: ntied(q) of the eight big tied lists (a different run of them per query) among
    `fill`(q) lists, the tied ones at every other position from `first` on."""
    rows = np.full((nq, nprobe), -1, np.int64)
    for q in range(nq):
        t = [mc.TIED_BIG[(q + i) % 8] for i in range(ntied(q))]
        f = list(fill(q))[:nprobe - len(t)]
        row = []
        while t or f:
            if f and (len(row) < first or len(row) % 2 == 1 or not t):
                row.append(f.pop(0))
            else:
                row.append(t.pop(0))
        rows[q, :len(row)] = row
    return rows


def tie_is_kth(c, ref, xq, qs, k):
    """The oracle's k-th result of every query of qs is a tied row, so the candidates at or
    below the k-th key include every tied entry of every probed tied list."""
    tk = mc.tied_key(c.metric, xq)
    for q in qs:
        assert ref[0][q, k - 1] == tk[q], (q, ref[0][q, k - 1], tk[q])


# ------------------------------------------------------------ radix overflow -> full merge
@pytest.mark.parametrize("k", [65, 128, 129, 256, 300, 512])
@pytest.mark.parametrize("variant", ["interleave", "permuted"])
@pytest.mark.parametrize("metric", METRICS)
def test_radix_overflow_tied_lists(metric, variant, k):
    """3 to 8 tied lists of 4096 identical rows: 4 waves x k tied entries per list, more than
    the 512 the radix merge holds, beside the better list and random lists (R = 2, 4, 8)."""
    c, ox = contents("tied", metric, variant)
    nprobe = min(8, 2048 // k)
    nq = 8
    xq = mc.tied_queries(metric, nq, seed=k)
    rows = tied_rows(nq, nprobe, lambda q: min(3 + q % 6, nprobe),
                     lambda q: [mc.TIED_BETTER, 20 + q, 60 + q, 100 + q, 140 + q], first=1)
    paths, ref = run(c, ox, xq, k, rows)
    tie_is_kth(c, ref, xq, range(nq), k)
    expect(paths, range(nq), kernel="radix", overflow=True)
    for q in range(nq):
        assert paths[q]["n"] >= 4 * k * min(3 + q % 6, nprobe)
    if variant == "interleave":  # label order walks across the tied lists: the top-k draws from all of them
        for q in range(nq):
            tied = ref[1][q][ref[0][q] == mc.tied_key(metric, xq)[q]]
            assert len(set((tied % 8).tolist())) == min(3 + q % 6, nprobe)


@pytest.mark.parametrize("k", [129, 256, 300, 512])
@pytest.mark.parametrize("metric", METRICS)
def test_radix_overflow_single_list(metric, k):
    """The plain search at nprobe 1 over one list of 16384 identical rows: its 4 waves' k
    entries already exceed 512 (R = 4 and 8)."""
    c, ox = contents("single", metric)
    xq = mc.tied_queries(metric, 4, seed=k)
    paths, ref = run(c, ox, xq, k, nprobe=1)
    assert (ref[0] == mc.tied_key(metric, xq)[:, None]).all()
    expect(paths, range(4), kernel="radix", overflow=True, n=4 * k, C=4 * k)


@pytest.mark.parametrize("metric", METRICS)
def test_radix_boundary_512_513(metric):
    """Exactly 512 (even queries: merged in place, leaving after pass 2) and exactly 513 (odd
    queries: all four passes, then overflow) entries at the k-th key, in four tied lists of 128
    or 129 rows; k = 300, so every wave keeps all of its rows.  The two random lists' rows are
    far worse (another exponent), so the pass-2 bucket holds the ties only."""
    c, ox = contents("tied", metric, "interleave")
    k, nq = 300, 6
    xq = mc.tied_queries(metric, nq, seed=1)
    rows = np.asarray([[20 + q, mc.TIED_128[0] if q % 2 == 0 else mc.TIED_129, *mc.TIED_128[1:], 60 + q]
                       for q in range(nq)], np.int64)
    paths, ref = run(c, ox, xq, k, rows)
    tie_is_kth(c, ref, xq, range(nq), k)
    expect(paths, range(0, nq, 2), kernel="radix", n=512, passes=2, overflow=False, regsort=False)
    expect(paths, range(1, nq, 2), kernel="radix", n=513, passes=4, overflow=True)


# ------------------------------------------------------------ radix exits (IP lattice)
def lattice_batch():
    """Six queries at nprobe 3: the 768 keys of one 24-bit bucket; the same lists for the
    zero query (768 ties); keys over many top bytes; one 16-bit bucket of 256 keys with
    distinct third bytes; 50 keys; similarities of both signs."""
    xq = mc.lattice_queries(6, zero=(1,))
    rows = np.stack([mc.pad_rows(r, 3) for r in (mc.LAT_ONE24, mc.LAT_ONE24, [mc.LAT_SPREAD], [mc.LAT_ONE16],
                                                 [mc.LAT_FEW], [mc.LAT_SIGNS])])
    rows[3] = [-1, mc.LAT_ONE16, -1]
    rows[4] = [-1, -1, mc.LAT_FEW]
    return xq, rows


@pytest.mark.parametrize("k", [100, 128, 200])
def test_radix_exits(k):
    c, ox = contents("lattice")
    xq, rows = lattice_batch()
    paths, ref = run(c, ox, xq, k, rows)
    small = k <= 128
    n24 = {100: 102, 128: 129, 200: 201}[k]  # three copies of every key: the k best and the k-th key's ties
    expect(paths, [0], kernel="radix", C=768, passes=4, n=n24, overflow=False, regsort=n24 <= 128)
    expect(paths, [1], kernel="radix", C=768, n=768, overflow=True)
    assert (ref[0][1] == 0).all() and (np.diff(ref[1][1]) > 0).all()
    expect(paths, [2], kernel="radix", C=256, passes=1 if small else 2, n=k, overflow=False, regsort=small)
    expect(paths, [3], kernel="radix", C=256, passes=2, n=k, overflow=False, regsort=small)
    expect(paths, [4], kernel="radix", C=50, passes=0, n=50, overflow=False, regsort=small)
    padded(ref, 4, 50, True)
    expect(paths, [5], kernel="radix", C=256, overflow=False)
    assert ref[0][5, 0] > 0 > ref[0][5, k - 1]  # the k best straddle zero


def test_big_keys_of_both_signs():
    """k = 300 at nprobe 9 (k_merge_big): similarities of both signs among the 300 best; the
    zero query, whose 2304 candidates all tie (overflow); the same lists for a lattice query."""
    c, ox = contents("lattice")
    k = 300
    nine = [0, 1, 2, 3, 4, 6, 7, 8, 14]
    xq = mc.lattice_queries(3, zero=(1,))
    rows = np.stack([mc.pad_rows(mc.LAT_SIGNS8, 9), np.asarray(nine, np.int64), np.asarray(nine[::-1], np.int64)])
    paths, ref = run(c, ox, xq, k, rows)
    expect(paths, [0], kernel="big", C=2048, rounds_entered=True, r=2, overflow_certain=False)
    assert ref[0][0, 0] > 0 > ref[0][0, k - 1]
    expect(paths, [1], kernel="big", C=2304, n_le_T=2304, overflow_certain=True)
    assert (ref[0][1] == 0).all() and (np.diff(ref[1][1]) > 0).all()
    expect(paths, [2], kernel="big", C=2304, rounds_entered=True, r=2, overflow_certain=False)


# ------------------------------------------------------------ k_merge_big, round structure
@pytest.mark.parametrize("k", [300, 1000])
@pytest.mark.parametrize("metric", METRICS)
def test_big_round_threshold(metric, k):
    """C one list below, at and one list above max(2k, k + 64) (the rounds run only above it;
    k = 300: 650 candidates are sampled at stride 1, exact, no bisection; k = 1000: 2200 at
    stride 2, bisection), fewer than k candidates (padded) and a query without a probe."""
    c, ox = contents("rounds", metric)
    lists, n = (mc.RS_50, 50) if k == 300 else (mc.RS_200, 200)
    cmax = max(2 * k, k + 64)
    at = cmax // n
    assert at * n == cmax and at + 1 == len(lists)
    nprobe = len(lists)
    assert mp.kernel_for(nprobe, k) == "big"
    few = (k - 1) // n - 1
    rows = np.stack([mc.pad_rows(lists[:at - 1], nprobe), mc.pad_rows(lists[1:at + 1], nprobe),
                     np.asarray(lists[::-1], np.int64), mc.pad_rows(lists[2:2 + few], nprobe),
                     mc.pad_rows([], nprobe)])
    xq = mc.rounds_queries(5, seed=k)
    paths, ref = run(c, ox, xq, k, rows)
    expect(paths, [0], kernel="big", C=cmax - n, rounds_entered=False, overflow_certain=False)
    expect(paths, [1], kernel="big", C=cmax, rounds_entered=False, overflow_certain=False)
    expect(paths, [2], kernel="big", C=cmax + n, rounds_entered=True, r=1 if k == 300 else 2, overflow_certain=False)
    expect(paths, [3], kernel="big", C=few * n, rounds_entered=False)
    padded(ref, 3, few * n, metric == mc.IP)
    expect(paths, [4], kernel="big", C=0)
    padded(ref, 4, 0, metric == mc.IP)


@pytest.mark.parametrize("k", [300, 1000])
@pytest.mark.parametrize("metric", METRICS)
def test_big_64_probes_all_slots(metric, k):
    """nprobe = 64 exactly, 256 rows in every list: all 256 list slots hold 64 entries
    (C = 16384, first stride 13, bisection)."""
    c, ox = contents("rounds", metric)
    rng = np.random.default_rng(k)
    rows = np.stack([rng.permutation(mc.RS_256) for _ in range(4)]).astype(np.int64)
    paths, _ = run(c, ox, mc.rounds_queries(4, seed=k + 1), k, rows)
    expect(paths, range(4), kernel="big", C=16384, rounds_entered=True, r=13, overflow_certain=False)


@pytest.mark.parametrize("k", [300, 1000])
@pytest.mark.parametrize("metric", METRICS)
def test_big_uneven_lists(metric, k):
    """One list holds more than 95 % of the candidates (8192 rows in 8 key classes: each wave
    keeps its k best, and the k-th key's class is never pruned), the 19 others 0 to 3 entries,
    so most lists contribute no sample."""
    c, ox = contents("rounds", metric)
    nq, nprobe = 4, 20
    rows = np.stack([np.insert(np.roll(mc.RS_TINY, q), 5 * q, mc.RS_LONG) for q in range(nq)]).astype(np.int64)
    tiny = int(c.sizes[mc.RS_TINY].sum())
    paths, _ = run(c, ox, mc.rounds_queries(nq, seed=k + 2), k, rows)
    for q in range(nq):
        p = paths[q]
        assert p["C"] == 4 * k + tiny and tiny < 0.05 * p["C"], p
    expect(paths, range(nq), kernel="big", rounds_entered=True, r=1 if k == 300 else 4, overflow_certain=False)


@pytest.mark.parametrize("k", [300, 1000])
@pytest.mark.parametrize("metric", METRICS)
def test_big_half_of_the_probes_masked(metric, k):
    c, ox = contents("rounds", metric)
    lists, n = (mc.RS_50, 50) if k == 300 else (mc.RS_200, 200)
    nprobe, nq = 2 * len(lists), 4
    rows = np.full((nq, nprobe), -1, np.int64)
    for q in range(nq):
        rows[q, (q % 2)::2] = np.roll(lists, q)
    paths, _ = run(c, ox, mc.rounds_queries(nq, seed=k + 3), k, rows)
    expect(paths, range(nq), kernel="big", C=n * len(lists), rounds_entered=True, r=1 if k == 300 else 2,
           overflow_certain=False)


# ------------------------------------------------------------ big overflow -> full merge
@pytest.mark.parametrize("k,ntied", [(300, 8), (600, 4), (1024, 4)])
@pytest.mark.parametrize("variant", ["interleave", "permuted"])
@pytest.mark.parametrize("metric", METRICS)
def test_big_overflow_tied_lists(metric, variant, k, ntied):
    """More than 2048 tied entries at the k-th key (R = 8 and 16); the last two queries probe
    random lists only and are merged by k_merge_big in the same launch."""
    c, ox = contents("tied", metric, variant)
    nq, nprobe = 6, ntied
    xq = mc.tied_queries(metric, nq, seed=k)
    rows = tied_rows(nq, nprobe, lambda q: ntied if q < 4 else 0, lambda q: range(20 + 10 * q, 160))
    paths, ref = run(c, ox, xq, k, rows)
    tie_is_kth(c, ref, xq, range(4), k)
    expect(paths, range(4), kernel="big", C=4 * k * ntied, n_le_T=4 * k * ntied, overflow_certain=True)
    expect(paths, [4, 5], kernel="big", overflow_certain=False)


@pytest.mark.parametrize("k", [600, 1024])
@pytest.mark.parametrize("metric", METRICS)
def test_big_overflow_single_list(metric, k):
    """The plain search at nprobe 4: one list of 16384 identical rows (4 waves x k tied
    entries) and three random lists (R = 16)."""
    c, ox = contents("single", metric)
    xq = mc.tied_queries(metric, 4, seed=k)
    paths, ref = run(c, ox, xq, k, nprobe=4)
    assert (ref[0] == mc.tied_key(metric, xq)[:, None]).all()
    expect(paths, range(4), kernel="big", overflow_certain=True)
    for p in paths:
        assert p["n_le_T"] >= 4 * k


# ------------------------------------------------------------ nprobe > 64 with k > 64
@pytest.mark.parametrize("k", [65, 129, 257, 1024])
@pytest.mark.parametrize("nprobe", [65, 128])
@pytest.mark.parametrize("metric", METRICS)
def test_full_merge_many_probes(metric, nprobe, k):
    """Two mask words per query (R = 2, 4, 8, 16): tied lists in both words, probes masked in
    the first word only and in the second only, a query with no probe, fewer than k results."""
    c, ox = contents("tied", metric, "interleave")
    nq = 8
    rng = np.random.default_rng(nprobe + k)
    second = 64 if nprobe == 65 else 70
    rows = np.empty((nq, nprobe), np.int64)
    for q in range(nq):
        rows[q] = rng.permutation(mc.TIED_RANDOM)[:nprobe]
        rows[q, 3], rows[q, second] = mc.TIED_BIG[q % 8], mc.TIED_BIG[(q + 3) % 8]
    rows[1, 0:64:2] = -1   # first word only
    rows[2, 64:] = -1      # second word only
    rows[3] = -1
    rows[4] = -1
    rows[4, 1], rows[4, second] = mc.TIED_SMALL
    rows[5, 5] = mc.TIED_BETTER
    xq = mc.tied_queries(metric, nq, seed=nprobe + k)
    paths, ref = run(c, ox, xq, k, rows)
    expect(paths, range(nq), kernel="full")
    tie_is_kth(c, ref, xq, [0, 1, 2, 5, 6, 7], k)
    padded(ref, 3, 0, metric == mc.IP)
    padded(ref, 4, 40, metric == mc.IP)
    assert paths[3]["C"] == 0 and paths[4]["C"] == 40


# ------------------------------------------------------------ mixed batch, carried state
def mixed_batch(metric, nprobe=8):
    """16 queries: random lists only (merged), tied lists (overflow), tied lists with the
    better list and masked probes (overflow), 40 rows in all (padded), no probe at all."""
    nq = 16
    rows = tied_rows(nq, nprobe, lambda q: [0, 3, 0, 8, 0, 5, 0, 4][q % 8],
                     lambda q: [mc.TIED_BETTER] * (q % 4 == 3) + list(range(20 + 8 * q, 160)), first=1)
    rows[5, 1::2] = -1
    for q in (6, 12):
        rows[q] = mc.pad_rows([-1, mc.TIED_SMALL[0], -1, mc.TIED_SMALL[1]], nprobe)
    for q in (8, 14):
        rows[q] = -1
    return mc.tied_queries(metric, nq, seed=99), rows


@pytest.mark.parametrize("k", [100, 300])
@pytest.mark.parametrize("metric", METRICS)
def test_mixed_batch_and_carried_state(metric, k):
    """Merged, overflowed, padded and unprobed queries in one launch (k = 100: k_merge_radix,
    k = 300: k_merge_big), twice, with device-resident inputs, with the queries in reverse
    order (an overflowed query where a merged one was), and again after a k <= 64 search of
    another size on the same handle: a qdone word that survived a batch would skip a merge."""
    import torch

    c, ox = contents("tied", metric, "permuted")
    xq, rows = mixed_batch(metric)
    kernel = mp.kernel_for(8, k)
    over = "overflow" if kernel == "radix" else "overflow_certain"
    ix = gpu_index(c)
    want = None
    for xs, rs in ((xq, rows), (xq, rows), (xq[::-1].copy(), rows[::-1].copy()), (xq, rows)):
        paths, ref = run(c, ox, xs, k, rs, ix=ix, grown=True)
        labels = [mp.label(p) for p in paths]
        if want is None:
            want = labels
            tie_is_kth(c, ref, xq, [1, 3, 5, 7, 9, 11, 13, 15], k)
            expect(paths, [1, 3, 5, 7, 9, 11, 13, 15], kernel=kernel, **{over: True})
            expect(paths, [0, 2, 4, 10], kernel=kernel, **{over: False})
            assert all(paths[q]["C"] > 100 for q in (0, 2, 4, 10))  # (k = 100: a select, not a copy)
            expect(paths, [6, 12], kernel=kernel, C=40, **{over: False})
            expect(paths, [8, 14], kernel=kernel, C=0, **{over: False})
            padded(ref, 6, 40, metric == mc.IP)
            padded(ref, 8, 0, metric == mc.IP)
        else:  # (timing may change how many worse entries the scan keeps, never the class)
            assert labels == (want if xs is xq else want[::-1])
    dq = c.dis0(xq, rows)
    ref = ox.search_preassigned(xq, k, rows, dq)
    D, I = ix.search_preassigned_device(torch.from_numpy(xq).cuda(), k, torch.from_numpy(rows).cuda(),
                                        torch.from_numpy(dq).cuda() if dq is not None else None)
    torch.cuda.synchronize()
    assert np.array_equal(I.cpu().numpy(), ref[1]) and np.array_equal(D.cpu().numpy(), ref[0])
    # another nq and k <= 64 on the same handle, then the first batch again
    r5 = rows[3:8]
    d5 = c.dis0(xq[3:8], r5)
    got = ix.search_preassigned(xq[3:8], 10, r5, d5)
    ref5 = ox.search_preassigned(xq[3:8], 10, r5, d5)
    assert np.array_equal(got[1], ref5[1]) and np.array_equal(got[0], ref5[0])
    paths, _ = run(c, ox, xq, k, rows, ix=ix, grown=True)
    assert [mp.label(p) for p in paths] == want
    assert ix.error_count() == 0 and ix.repair_stats() == (0, 0)


# ------------------------------------------------------------ shard merge
def shard_lists(S, n, k, ip, seed, key_range):
    """Sorted partial results [S][n][k] with heavy ties across shards and distinct labels per
    query; query 0 is all padding, query 1 full, the others hold random counts."""
    rng = np.random.default_rng(seed)
    pad = -FMAX if ip else FMAX
    Ds = np.full((S, n, k), pad, np.float32)
    Is = np.full((S, n, k), -1, np.int64)
    for q in range(1, n):
        labels = rng.permutation(4 * S * k)
        for s in range(S):
            m = k if q == 1 else int(rng.integers(0, k + 1))
            d = rng.integers(-key_range, key_range + 1, size=m).astype(np.float32)
            i = labels[s * k:s * k + m].astype(np.int64)
            o = np.lexsort((i, -d if ip else d))
            Ds[s, q, :m], Is[s, q, :m] = d[o], i[o]
    return Ds, Is


def shard_reference(Ds, Is, ip):
    """Plain lexsort by (key, label), -1 labels last."""
    S, n, k = Ds.shape
    D = np.empty((n, k), np.float32)
    I = np.empty((n, k), np.int64)
    for q in range(n):
        d, i = Ds[:, q].reshape(-1), Is[:, q].reshape(-1)
        o = np.lexsort((np.where(i < 0, np.iinfo(np.int64).max, i), -d if ip else d))[:k]
        D[q], I[q] = d[o], i[o]
    return D, I


@pytest.mark.parametrize("S,k", [(3, 1000), (8, 300), (1, 100), (2, 1024), (5, 409), (5, 410)])
@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
def test_shard_merge(S, k, ip):
    """merge_topk_device staged in LDS (S k <= 2048: (2, 1024), (5, 409), (1, 100)) and from
    global memory (S k > 2048), both metrics, padded tails, a query that is all padding, keys
    of both signs drawn from 7 values (ties across shards, distinct labels)."""
    import torch

    Ds, Is = shard_lists(S, 6, k, ip, seed=S * k + ip, key_range=3)
    D, I = faiss.merge_topk_device(torch.from_numpy(Ds).cuda(), torch.from_numpy(Is).cuda(),
                                   metric=faiss.METRIC_INNER_PRODUCT if ip else faiss.METRIC_L2)
    torch.cuda.synchronize()
    Dr, Ir = shard_reference(Ds, Is, ip)
    assert (Ir[0] == -1).all() and (Ir[1] >= 0).all()
    np.testing.assert_array_equal(I.cpu().numpy(), Ir)
    np.testing.assert_array_equal(D.cpu().numpy(), Dr)
