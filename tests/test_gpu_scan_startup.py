"""The list scan's first claim: workgroup b starts with work item b, later claims come
from the counter (ivfpq_kernels.hip SCAN_STATIC_CLAIM, profiles/scan_startup.md).

The claim can only go wrong where static and dynamic claims meet: fewer items than
workgroups, exactly as many, a few more, and the counter's state from one batch to the
next.  So the shapes are tiny lists and many items: 1024 lists of 1 to 16 rows, and probe
rows built by hand so that the batch has exactly N work items -- asserted on the counts
the scan leaves in hdr[0..1], as tests/test_gpu_plan_fill.py does.  N runs through 0, 1, 3,
every value 470..490 and 760..776 (the persistent grids of the benchmark's device with
and without batches in flight lie inside; the test does not know the grid) and 4000.
Every result is compared bit for bit, D and I, with the CPU oracle, on integer-valued
tables (many exact ties).

A list used by a batch of N >= 12 items has one first-probe pair and 4 (t - 1) other
pairs: t items, one of them a lead item.  Smaller batches and the all-lead cases give
every used list one first-probe pair alone.
"""
import ctypes
import functools

import numpy as np
import pytest

import faiss_amd as faiss
from faiss_amd import _lib
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def epochs(ix):
    """The epoch (batches planned so far) of each of the handle's three workspaces."""
    out = []
    for ws in range(3):
        nb = ctypes.c_int64(0)
        ep = np.zeros(1, np.uint64)
        _lib.check(_lib.load().ivfpq_debug_workspace(ix._h, ws, 7, ep.ctypes.data, 8, ctypes.byref(nb)))
        out.append(int(ep[0]))
    return out


def item_counts(ix, before):
    """hdr[0], hdr[1] of the workspace that planned the one batch searched since
    `before` = epochs(ix): the one whose epoch moved."""
    after = epochs(ix)
    moved = [ws for ws in range(3) if after[ws] != before[ws]]
    assert len(moved) == 1 and after[moved[0]] == before[moved[0]] + 1, (before, after)
    nb = ctypes.c_int64(0)
    hdr = np.zeros(16, np.int32)
    _lib.check(_lib.load().ivfpq_debug_workspace(ix._h, moved[0], 4, hdr.ctypes.data, hdr.nbytes, ctypes.byref(nb)))
    assert nb.value >= hdr.nbytes
    return int(hdr[0]), int(hdr[1])


def check(got, ref, msg):
    np.testing.assert_array_equal(got[1], ref[1], err_msg=msg)
    np.testing.assert_array_equal(got[0], ref[0], err_msg=msg)

D = 32
NLIST = 1024
G = 4
COUNTS = [0, 1, 3] + list(range(470, 491)) + list(range(760, 777)) + [4000]


def list_sizes(nlist, big=None):
    s = 1 + (np.arange(nlist) * 7) % 16
    if big is not None:
        s[big] = 1537  # longer than one super-batch of the lean scan, and the largest list: item 0
    return s


@functools.lru_cache(maxsize=None)
def make_pair(M, metric, nlist=NLIST, lo=0, hi=None, big=None):
    """GPU index and oracle on the same integer-valued tables and codes; lists outside
    [lo, hi) stay empty in both."""
    hi = nlist if hi is None else hi
    ip = metric == "ip"
    rng = np.random.default_rng(9000 + M + ip + nlist)
    cent = rng.integers(-3, 4, size=(nlist, D)).astype(np.float32)
    cb = rng.integers(-2, 3, size=(M, 256, D // M)).astype(np.float32)
    sizes = np.where((np.arange(nlist) >= lo) & (np.arange(nlist) < hi), list_sizes(nlist, big), 0)
    n = int(sizes.sum())
    codes = rng.integers(0, 256, size=(n, M), dtype=np.uint8)
    list_no = np.repeat(np.arange(nlist, dtype=np.int64), sizes)
    ids = np.arange(n, dtype=np.int64) * 3 + 1
    ix = faiss.IndexIVFPQ(None, D, nlist, M, 8, faiss.METRIC_INNER_PRODUCT if ip else faiss.METRIC_L2, device=0)
    ix.set_trained(cent, cb)
    if (lo, hi) != (0, nlist):
        ix.set_list_range(lo, hi)
    ix.add_preencoded(list_no, codes, ids)
    ox = O.OracleIVFPQ(D, nlist, M, metric=O.METRIC_INNER_PRODUCT if ip else O.METRIC_L2)
    ox.set_trained(cent, cb)
    ox.add_preencoded(list_no, codes, ids)
    return ix, ox, cent


def build_rows(n_items, lists, all_lead=False, g=G):
    """Probe rows over `lists` (every one non-empty) that make exactly n_items work items
    at g pairs per item, and the number of lead items among them."""
    if n_items == 0:
        return np.full((1, 1), -1, np.int64), 0
    if all_lead or n_items < 12:
        assert n_items <= len(lists)
        return np.asarray(lists[:n_items], np.int64).reshape(-1, 1), n_items
    m = max(2, -(-n_items // (len(lists) - 1)))  # items per used list
    full, r = divmod(n_items, m)
    t = [m] * full + ([r] if r else [])
    assert len(t) <= len(lists)
    rows = [[lists[j]] for j in range(len(t))]
    for j, tj in enumerate(t):
        c1 = g * (tj - 1)
        assert c1 < len(rows)
        for s in range(c1):  # a later probe of the c1 rows behind its own
            rows[(j + 1 + s) % len(rows)].append(lists[j])
    out = np.full((len(rows), max(len(r) for r in rows)), -1, np.int64)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out, len(t)


def expected_items(rows, g=G):
    """(items, lead items) of the rows by the planner's rule, every probed list usable."""
    c = {}
    for row in rows:
        first = True
        for l in row:
            if l >= 0:
                c.setdefault(int(l), [0, 0])[0 if first else 1] += 1
                first = False
    return (sum(-(-(c0 + c1) // g) for c0, c1 in c.values()), sum(-(-c0 // g) for c0, _ in c.values()))


@functools.lru_cache(maxsize=None)
def batch(n_items, lo=0, hi=NLIST, all_lead=False, seed=1):
    """Rows, queries and dis0 of a batch of n_items work items over the lists [lo, hi)."""
    rng = np.random.default_rng(100 * n_items + seed)
    rows, lead = build_rows(n_items, [int(l) for l in lo + rng.permutation(hi - lo)], all_lead)
    assert expected_items(rows) == (n_items, lead)
    xq = rng.integers(-3, 4, size=(rows.shape[0], D)).astype(np.float32)
    dq = rng.integers(0, 5, size=rows.shape).astype(np.float32)
    return rows, xq, dq, lead


def run_batch(ix, ox, metric, k, b, assert_hdr=True, msg=""):
    rows, xq, dq, lead = b
    dq = None if metric == "ip" else dq
    ix.nprobe = rows.shape[1]
    ref = ox.search_preassigned(xq, k, rows, dq)
    for inflight in (False, True):
        ix.inflight = inflight
        try:
            ep = epochs(ix)
            check(ix.search_preassigned(xq, k, rows, dq), ref, f"{msg} k={k} inflight={inflight}")
            if assert_hdr:
                got = item_counts(ix, ep)
                want = expected_items(rows)
                assert got == want, f"{msg} k={k} inflight={inflight}: hdr {got}, expected {want}"
        finally:
            ix.inflight = False


def clean(ix, e0, rs0):
    rs = ix.repair_stats()
    assert ix.error_count() == e0 == 0
    assert (rs[0] - rs0[0], rs[1] - rs0[1]) == (0, 0)


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("M", [8, 16])
def test_item_counts_around_the_grids(M, metric):
    ix, ox, _ = make_pair(M, metric)
    e0, rs0 = ix.error_count(), ix.repair_stats()
    for n in COUNTS:
        for k in (10, 1):
            run_batch(ix, ox, metric, k, batch(n), msg=f"items={n}")
    clean(ix, e0, rs0)


@pytest.mark.parametrize("M", [8, 16])
def test_consecutive_batches_of_different_counts(M):
    """4000 -> 3 -> 770 items on one handle: the counter is zero again for every batch."""
    ix, ox, _ = make_pair(M, "l2")
    e0, rs0 = ix.error_count(), ix.repair_stats()
    for seq in ((4000, 3), (4000, 3, 770), (770, 0, 1, 4000)):
        for n in seq:
            run_batch(ix, ox, "l2", 10, batch(n), msg=f"sequence {seq} items={n}")
    clean(ix, e0, rs0)


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_list_range_shard(metric):
    """A shard of 100 lists: up to 8 items per list."""
    ix, ox, _ = make_pair(16, metric, NLIST, 200, 300)
    e0, rs0 = ix.error_count(), ix.repair_stats()
    for n in (3, 99, 480, 770, 771):
        run_batch(ix, ox, metric, 10, batch(n, 200, 300), msg=f"shard items={n}")
    clean(ix, e0, rs0)


@pytest.mark.parametrize("M", [8, 16])
def test_plain_search_with_the_inflight_grid(M):
    """The full search (coarse step, planning in its epilogue), whose scan leaves CUs free
    with batches in flight.  Query i is centroid c_i and nprobe is 1, so the batch has one
    lead item per query; with nprobe 4 the counts are the coarse step's."""
    ix, ox, cent = make_pair(M, "l2")
    assert len(np.unique(cent, axis=0)) == NLIST
    e0, rs0 = ix.error_count(), ix.repair_stats()
    perm = np.random.default_rng(3).permutation(NLIST)
    try:
        for inflight in (False, True):
            ix.inflight = inflight
            ix.nprobe = ox.nprobe = 1
            for n in [1, 3] + list(range(470, 491, 3)) + list(range(760, 777, 2)) + [1024]:
                xq = cent[perm[:n]]
                ep = epochs(ix)
                check(ix.search(xq, 10), ox.search(xq, 10), f"plain items={n} inflight={inflight}")
                assert item_counts(ix, ep) == (n, n), (n, inflight)
            ix.nprobe = ox.nprobe = 4
            for n in (121, 193, 1000):
                xq = cent[perm[:n]] + 1.0
                check(ix.search(xq, 10), ox.search(xq, 10), f"plain nprobe=4 nq={n} inflight={inflight}")
    finally:
        ix.inflight = False
    clean(ix, e0, rs0)


@pytest.mark.parametrize("M", [8, 16])
def test_k100_queue_scan(M):
    """k = 100: k_scan_lists.  One first-probe pair per list, so the item count does not
    depend on the pairs per item."""
    ix, ox, _ = make_pair(M, "l2")
    e0, rs0 = ix.error_count(), ix.repair_stats()
    for n in (3, 770):
        run_batch(ix, ox, "l2", 100, batch(n, all_lead=True), msg=f"k=100 items={n}")
    run_batch(ix, ox, "l2", 100, batch(770), assert_hdr=False, msg="k=100 mixed")
    clean(ix, e0, rs0)


def test_non_fused_records():
    """More than 1024 lists in the shard: the items come from the planner's records."""
    nlist = 1032
    ix, ox, _ = make_pair(8, "l2", nlist)
    e0, rs0 = ix.error_count(), ix.repair_stats()
    for n in (3, 770, 1500):  # 1500 items: 3000 rows' worth of pairs (750 lists, 5 pairs each)
        run_batch(ix, ox, "l2", 10, batch(n, 0, nlist), msg=f"non-fused items={n}")
    clean(ix, e0, rs0)


@pytest.mark.parametrize("M", [8, 16])
def test_long_list_is_a_first_item(M):
    """List 5 holds 1537 rows (a second super-batch) and is the largest, so its lead item is
    item 0: workgroup 0's first."""
    ix, ox, _ = make_pair(M, "l2", big=5)
    e0, rs0 = ix.error_count(), ix.repair_stats()
    for n in (2, 770):
        lists = [5] + [int(l) for l in np.random.default_rng(n).permutation(NLIST) if l != 5]
        rows, lead = build_rows(n, lists, all_lead=n < 12)
        assert expected_items(rows) == (n, lead) and rows[0, 0] == 5
        rng = np.random.default_rng(50 + n)
        xq = rng.integers(-3, 4, size=(rows.shape[0], D)).astype(np.float32)
        dq = rng.integers(0, 5, size=rows.shape).astype(np.float32)
        for k in (10, 1):
            run_batch(ix, ox, "l2", k, (rows, xq, dq, lead), msg=f"long list items={n}")
    clean(ix, e0, rs0)


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_all_lead_items(metric):
    ix, ox, _ = make_pair(16, metric)
    e0, rs0 = ix.error_count(), ix.repair_stats()
    for n in (480, 481, 768, 769, 1024):
        run_batch(ix, ox, metric, 10, batch(n, all_lead=True), msg=f"all lead items={n}")
    clean(ix, e0, rs0)
