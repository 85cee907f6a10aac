"""k_scan_lists_h (IVF-PQ with float16 lookup tables) under worst-case key order, in
every (M, k) class, against tests/ivfpq_f16lut_ref.py bit for bit: tests/test_gpu_scan_order.py for the flag.

The half scan is a second copy of the list scan's item loop, with its own admission pass, packed prefix-sum
push, `full` / `loose` / `pend` stops, drain, early bounds, s_wb / tau publishing, static first claim and
next-record prefetch.  In random order row i of a list is admitted with probability about k / i, so on random
codes those branches run a handful of times at the head of a list, if at all.  The result of a search does
not depend on the order of the rows, so here only the inputs change: tests/scan_order.py
pq_contents(half=True) (its preconditions are held by tests/test_scan_order_cpu.py) gives four lists of 4700,
1537, 300 and 0 rows whose *half* keys, for the designated query, arrive in one of three orders.

`improving` (every row beats all before it: each wave admits every row of every chunk)
    aims at the per-chunk admission with its `full` stop -- the queue is drained and the same chunk admitted
    again -- at the packed prefix-sum push once the bound is tight but the queue still has room
    (qmax + tot <= QG, FB = 32 / G bits per pair: 8 bits at G = 4), at `pend` (the drain the last chunk of a
    super-batch asks for) and, inside the drain, at the bulk merges: kc_bulk_merge (R = 1),
    kc_bulk_merge_rows (R >= 2) and kc_row16_merge (k <= 16), which under the flag runs at every M and at
    QG = 64 with JB = 4.  Five copies of the designated query put four such pairs into one G = 4 item (every
    queue overflows in the same chunk) and one into a second item.
`worsening` (the first k rows are the result)
    aims at the `loose` stop (drain after the first chunk that admits anything), at the early bounds of
    R = 1 and of R >= 2 (the latter exists only when JB * 64 >= k: k <= 384 at M <= 16, k <= 256 at M >= 32),
    at `insert` (at most 4 candidates pass a drain) and at a bound that is tight at once and published to
    s_wb and tau: later items and the other waves must then admit nothing and lose nothing.
`one_wave` (the rows with (i >> 6) & 3 == 0 hold the best keys, improving; the rest worsen)
    one wave keeps admitting while the others admit nothing once a bound exists: a bound taken from s_wb or
    tau must never prune a true result.

The random queries of the batch see the same lists in an unrelated order.  nprobe = 4 scans every list for
every query (later items start under a bound from earlier ones); nprobe = 1 sends every query to the 4700-row
list, so the bound comes from that list alone.  The tables tell the half scan from the fp32 one (L2: about 290
inexact entries per table up to 68 000, exact ties, entries clamped at 65504; inner product: 228 inexact
entries, one clamped), so a build that ran the fp32 kernels under the flag fails here.

Half scan classes, R = rows_for(k) (1: k <= 64, 2: <= 128, 4: <= 256, 8 and 16 above), G pairs per item =
scan_group_h(M, R), QG = 256 / G queue entries per wave and pair, JB chunks of 256 rows per super-batch:

    M        R = 1 (k 1 10 16 64)   R = 2 (100)   R = 4 (200)   R >= 8 (300 400 1000)   JB
    8, 16    G 4, QG 64             G 2, QG 128   G 2, QG 128   G 1, QG 256             6
    32       G 4, QG 64             G 4, QG 64    G 2, QG 128   G 1, QG 256             4
    48, 64   G 2, QG 128            G 2, QG 128   G 2, QG 128   G 1, QG 256             4

All are k_scan_lists_h<M, G, R, JB>: with the flag on there is no lean and no row-packed scan, whether the
plan is fused (up to 1024 lists) or comes from the planner's records (more).
"""
import functools

import numpy as np
import pytest

import faiss_amd as faiss
import ivfpq_f16lut_ref as RH
import scan_order as SO

pytestmark = pytest.mark.gpu

KS = (1, 10, 16, 64, 100, 200, 300, 400, 1000)
KMAX = max(KS)
ROWK_NLIST, ROWK_PLACE = 1032, (0, 1023, 1024, 1031)  # both sides of the planner's 1024-list block
METRICS = pytest.mark.parametrize("metric", [SO.L2, SO.IP])
ORDERS = pytest.mark.parametrize("order", SO.ORDERS)


@functools.lru_cache(maxsize=None)
def make_index(shape, metric, order, nlist=4, place=(0, 1, 2, 3)):
    """The half contents in a GpuIndexIVFPQ from index_cpu_to_gpu with useFloat16."""
    c = SO.pq_contents(shape, metric, order, nlist, place, half=True)
    mt = faiss.METRIC_INNER_PRODUCT if metric == SO.IP else faiss.METRIC_L2
    co = faiss.GpuClonerOptions()
    co.useFloat16 = True
    ix = faiss.index_cpu_to_gpu(None, 0, faiss.IndexIVFPQ(None, c.d, nlist, c.M, 8, mt, device=0), co)
    ix.set_trained(c.cent, c.cb)
    ix.add_preencoded(c.list_no, c.codes, c.ids)
    assert ix.use_float16_lut
    return ix, c


def all_lists(c):
    """Probe rows naming all four lists, each query starting at another one."""
    return np.stack([np.roll(SO.probe_rows(c, 1, range(4))[0], q) for q in range(len(c.xq))])


@functools.lru_cache(maxsize=None)
def reference(shape, metric, order, nlist=4, place=(0, 1, 2, 3), which="all"):
    """The half reference's KMAX best of every query of the batch over all four lists (what a search with
    nprobe = 4 and nlist = 4 returns, whatever the probe order) or over the 4700-row list alone; a prefix
    of it is the answer for a smaller k.  Computed once and left unchanged."""
    c = SO.pq_contents(shape, metric, order, nlist, place, half=True)
    rows = all_lists(c) if which == "all" else SO.probe_rows(c, len(c.xq), [0])
    lcodes, lids = SO.pq_lists(c)
    D, I = RH.search_preassigned(c.xq, KMAX, rows, SO.dis0(c, c.xq, rows), c.cent, c.cb, lcodes, lids,
                                 ip=metric == SO.IP)
    D.setflags(write=False)
    I.setflags(write=False)
    return D, I


def check(got, ref, msg):
    np.testing.assert_array_equal(got[1], ref[1], err_msg=msg)
    np.testing.assert_array_equal(got[0].view(np.uint32), ref[0].view(np.uint32), err_msg=msg)


@ORDERS
@METRICS
@pytest.mark.parametrize("shape", list(SO.PQ_SHAPES))
def test_every_class_matches_reference(shape, metric, order):
    """nlist = 4 (the fused plan): k_scan_lists_h in every (M, R) class of the table above."""
    ix, c = make_index(shape, metric, order)
    ref4, ref1 = reference(shape, metric, order), reference(shape, metric, order, which="one")
    e0, rs0 = ix.error_count(), ix.repair_stats()
    one = SO.probe_rows(c, len(c.xq), [0])
    d_one = SO.dis0(c, c.xq, one)
    for k in KS:
        ix.nprobe = 4
        check(ix.search(c.xq, k), RH.prefix(ref4, k), f"search nprobe=4 k={k}")
        ix.nprobe = 1
        want = RH.prefix(ref1, k)
        np.testing.assert_array_equal(want[1][0], SO.expected_ids(c.list_ids[0], order, k))
        check(ix.search_preassigned(c.xq, k, one, d_one), want, f"preassigned nprobe=1 k={k}")
    assert ix.error_count() == e0
    assert ix.repair_stats() == rs0


@ORDERS
@METRICS
@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("shape", ["d32_m8", "d64_m32"])
def test_non_fused_plan_matches_reference(shape, k, metric, order):
    """nlist = 1032: the items come from the planner's records (k_plan_items), at G = 4 (M = 8 and 32 at
    k = 10, M = 32 at k = 100) and G = 2.  The probes are given, since a coarse search over 1032 centroids
    would pick other lists."""
    ix, c = make_index(shape, metric, order, ROWK_NLIST, ROWK_PLACE)
    e0, rs0 = ix.error_count(), ix.repair_stats()
    for which, rows in (("all", all_lists(c)), ("one", SO.probe_rows(c, len(c.xq), [0]))):
        want = RH.prefix(reference(shape, metric, order, ROWK_NLIST, ROWK_PLACE, which), k)
        if which == "one":
            np.testing.assert_array_equal(want[1][0], SO.expected_ids(c.list_ids[0], order, k))
        ix.nprobe = rows.shape[1]
        check(ix.search_preassigned(c.xq, k, rows, SO.dis0(c, c.xq, rows)), want, f"nprobe={rows.shape[1]} k={k}")
    assert ix.error_count() == e0
    assert ix.repair_stats() == rs0


@METRICS
@pytest.mark.parametrize("shape,k", [("d64_m32", 100), ("d128_m64", 200)])
def test_improving_batches_in_flight(shape, k, metric):
    """Eight batches in flight on two streams, each into its own output buffers, equal the one-at-a-time
    searches and the reference, with no stale read or repair."""
    import torch

    ix, c = make_index(shape, metric, "improving")
    ref4 = RH.prefix(reference(shape, metric, "improving"), k)
    ix.nprobe = 4
    nq, nb = len(c.xq), 8
    rng = np.random.default_rng(77)
    perms = [rng.permutation(nq) for _ in range(nb)]
    xd = [torch.from_numpy(c.xq[p]).cuda() for p in perms]
    e0, rs0 = ix.error_count(), ix.repair_stats()
    ref = []
    for b in range(nb):
        D, I = ix.search_device(xd[b], k)
        torch.cuda.synchronize()
        ref.append((D.cpu().numpy(), I.cpu().numpy()))
        check(ref[b], (ref4[0][perms[b]], ref4[1][perms[b]]), f"batch {b} alone")
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [(torch.empty((nq, k), device="cuda"), torch.empty((nq, k), dtype=torch.int64, device="cuda"))
            for _ in range(nb)]
    ix.inflight = True
    try:
        torch.cuda.synchronize()
        for b in range(nb):
            ix.search_device(xd[b], k, outs[b][0], outs[b][1], stream=streams[b % 2].cuda_stream)
        torch.cuda.synchronize()
    finally:
        ix.inflight = False
    for b in range(nb):
        check((outs[b][0].cpu().numpy(), outs[b][1].cpu().numpy()), ref[b], f"batch {b} in flight")
    assert ix.repair_stats() == rs0
    assert ix.error_count() == e0
