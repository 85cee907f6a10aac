"""The first claim of k_scan_lists_h: workgroup b starts with work item b, later claims come from the
counter -- tests/test_gpu_scan_startup.py with float16 lookup tables on, whose scan has its own copy of the
static first claim and of the next-record prefetch, and grids of its own.

The half grids are the occupancy of the launched instantiation times the CUs (two or
three workgroups per CU, 512 or 768 on the benchmark's device, 480 or 720 with batches in flight; the test
does not know the grid).  So N, the number of work items of a batch, runs through 0, 1, 3, every value
470..490, 504..520, 712..728 and 760..776, and 4000, at three shapes with the pairs per item that the half
scan has there:

    (M = 32, k = 10)   G = 4
    (M = 64, k = 10)   G = 2
    (M = 8, k = 100)   G = 2

1024 lists of 1 to 16 rows and probe rows built by hand (test_gpu_scan_startup.build_rows at G) give exactly
N items, asserted on hdr[0..1]; every batch runs without and with batches in flight, one after the other on
the same handle, so the counter's state carries over.  The tables are small integers, exact in half
(asserted), so D and I are compared bit for bit with the CPU oracle."""
import functools

import numpy as np
import pytest

import faiss_amd as faiss
import ivfpq_f16lut_ref as RH
import test_gpu_scan_startup as SS
from oracle import oracle as O

pytestmark = pytest.mark.gpu

NLIST = SS.NLIST
SHAPES = {"d32_m32_k10": (32, 32, 10, 4), "d64_m64_k10": (64, 64, 10, 2), "d32_m8_k100": (32, 8, 100, 2)}  # d, M, k, G
COUNTS = [0, 1, 3] + list(range(470, 491)) + list(range(504, 521)) + list(range(712, 729)) + \
    list(range(760, 777)) + [4000]


@functools.lru_cache(maxsize=None)
def make_pair(shape, metric):
    """GpuIndexIVFPQ with the flag on and the oracle, on the same integer-valued tables and codes."""
    d, M, _, _ = SHAPES[shape]
    ip = metric == "ip"
    rng = np.random.default_rng(9100 + M + ip)
    cent = rng.integers(-3, 4, size=(NLIST, d)).astype(np.float32)
    cb = rng.integers(-2, 3, size=(M, 256, d // M)).astype(np.float32)
    # any query in [-3, 3]^d: |T1| <= |c|^2 + 2 |<cent, c>|, |T3| <= 3 |c|_1, integers, exact in half below 2048
    c2, c1 = (cb ** 2).sum(-1).max(), np.abs(cb).sum(-1).max()
    assert c2 + 2 * 3 * c1 + 2 * 3 * c1 < 2048
    lut = RH.lut32(O.ip_table(cent[:1], cb)[0], O.precompute_T1(cent[1:2], cb)[0], ip)
    np.testing.assert_array_equal(RH.entries(lut), lut)
    sizes = SS.list_sizes(NLIST)
    n = int(sizes.sum())
    codes = rng.integers(0, 256, size=(n, M), dtype=np.uint8)
    list_no = np.repeat(np.arange(NLIST, dtype=np.int64), sizes)
    ids = np.arange(n, dtype=np.int64) * 3 + 1
    ix = faiss.GpuIndexIVFPQ(None, d, NLIST, M, 8, faiss.METRIC_INNER_PRODUCT if ip else faiss.METRIC_L2, 0)
    ix.set_trained(cent, cb)
    ix.add_preencoded(list_no, codes, ids)
    ix.use_float16_lut = True
    ox = O.OracleIVFPQ(d, NLIST, M, metric=O.METRIC_INNER_PRODUCT if ip else O.METRIC_L2)
    ox.set_trained(cent, cb)
    ox.add_preencoded(list_no, codes, ids)
    return ix, ox


@functools.lru_cache(maxsize=None)
def batch(n_items, d, g, all_lead=False):
    """Rows, queries and dis0 of a batch of n_items work items at g pairs per item."""
    rng = np.random.default_rng(100 * n_items + g)
    rows, lead = SS.build_rows(n_items, [int(l) for l in rng.permutation(NLIST)], all_lead, g)
    assert SS.expected_items(rows, g) == (n_items, lead)
    xq = rng.integers(-3, 4, size=(rows.shape[0], d)).astype(np.float32)
    dq = rng.integers(0, 5, size=rows.shape).astype(np.float32)
    return rows, xq, dq


def run_batch(ix, ox, metric, k, g, b, msg):
    rows, xq, dq = b
    dq = None if metric == "ip" else dq
    ix.nprobe = rows.shape[1]
    ref = ox.search_preassigned(xq, k, rows, dq)
    want = SS.expected_items(rows, g)
    for inflight in (False, True):
        ix.inflight = inflight
        try:
            ep = SS.epochs(ix)
            SS.check(ix.search_preassigned(xq, k, rows, dq), ref, f"{msg} inflight={inflight}")
            got = SS.item_counts(ix, ep)
            assert got == want, f"{msg} inflight={inflight}: hdr {got}, expected {want}"
        finally:
            ix.inflight = False


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_item_counts_around_the_grids(shape, metric):
    d, _, k, g = SHAPES[shape]
    ix, ox = make_pair(shape, metric)
    assert ix.use_float16_lut
    e0, rs0 = ix.error_count(), ix.repair_stats()
    for n in COUNTS:
        run_batch(ix, ox, metric, k, g, batch(n, d, g), f"items={n}")
    SS.clean(ix, e0, rs0)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_consecutive_batches_of_different_counts(shape):
    """4000 -> 3 -> 770 items and back on one handle: the counter is zero again for every batch; all-lead
    batches (one pair per item) on both sides of the grids in between."""
    d, _, k, g = SHAPES[shape]
    ix, ox = make_pair(shape, "l2")
    e0, rs0 = ix.error_count(), ix.repair_stats()
    for seq in ((4000, 3), (4000, 3, 770), (516, 0, 1, 4000)):
        for n in seq:
            run_batch(ix, ox, "l2", k, g, batch(n, d, g), f"sequence {seq} items={n}")
    for n in (512, 513, 768, 769, 1024):
        run_batch(ix, ox, "l2", k, g, batch(n, d, g, all_lead=True), f"all lead items={n}")
    SS.clean(ix, e0, rs0)
