"""The IVF-PQ list scans under worst-case key order, in every (M, k) class, against the CPU
oracle bit for bit.

A scan takes a row into a wave's top-k only if it beats the k-th best key seen so far by that
wave, by the other waves of its workgroup (s_wb) or by other workgroups (tau).  In random
order row i of a list is admitted with probability about k / i, so after a few hundred rows
a scan sits in its "one ballot, nothing to do" path and the branches that handle heavy
admission run a handful of times at the head of a list, if at all.  The result of a search
does not depend on the order of the rows, so here only the inputs change (tests/scan_order.py;
their preconditions are held by tests/test_scan_order_cpu.py): four lists of 4700, 1537, 300
and 0 rows whose keys, for the designated query, arrive in one of three orders.

`improving` (every row beats all before it: each wave admits every row of every chunk)
    aims at the per-chunk admission with its `full` stop -- the queue is drained and the same
    chunk admitted again -- at the packed prefix-sum push once the bound is tight but the
    queue still has room (qmax + tot <= QG, FB = 32 / G bits per pair), at `pend` (the drain
    the last chunk of a super-batch asks for) and, inside the drain, at the bulk merges:
    kc_bulk_merge (R = 1), kc_bulk_merge_rows (R >= 2), kc_row16_merge (k <= 16) and the
    row-packed drain_rows of k_scan_lists<M, 4, 1, JB, true> (k <= 16, M <= 16, more than 1024
    lists: the non-fused plan).  Five copies of the designated query put four such pairs into
    one G = 4 item (every queue overflows in the same chunk) and one into a second item.
`worsening` (the first k rows are the result)
    aims at the `loose` stop (drain after the first chunk that admits anything), at the early
    bound of k > 64 (it exists only when JB * 64 >= k: k <= 384 at M <= 16, k <= 256 at
    M >= 32, so k = 300 has one at M = 16 and none at M = 32, and k = 400 has none), at
    `insert` (at most 4 candidates pass a drain) and at a bound that is tight at once and
    published to s_wb and tau: later items and the other waves must then admit nothing and
    lose nothing.
`one_wave` (the rows with (i >> 6) & 3 == 0 hold the best keys, improving; the rest worsen)
    one wave keeps admitting while the others admit nothing once a bound exists: a bound taken
    from s_wb or tau must never prune a true result.

The random queries of the batch see the same lists in an unrelated order.  nprobe = 4 scans
every list for every query (later items start under a bound from earlier ones); nprobe = 1
sends every query to the 4700-row list, so the bound comes from that list alone.

Scan classes, R = rows_for(k) (1: k <= 64, 2: <= 128, 4: <= 256, 8: <= 512, 16 above), G pairs
per item = scan_group(M, R), QG = 256 / G queue entries per wave and pair, JB chunks of 256
rows per super-batch (1536 rows at JB = 6, 1024 at JB = 4):

    M        R = 1 (k 1 10 16 64)   R = 2 (100)   R = 4 (200)   R = 8 (300 400)   R = 16 (1000)   JB
    8, 16    G 4, QG 64  (*)        G 2, QG 128   G 2, QG 128   G 1, QG 256       G 1, QG 256     6
    32       G 2, QG 128            G 2, QG 128   G 2, QG 128   G 1, QG 256       G 1, QG 256     4
    48, 64   G 1, QG 256            G 1, QG 256   G 1, QG 256   G 1, QG 256       G 1, QG 256     4

All are k_scan_lists<M, G, R, JB>, except (*) at k <= 16: k_scan_lean with up to 1024 lists
(the main grid), k_scan_lists<M, 4, 1, 6, true> (row-packed) with more (the row-packed grid).
"""
import functools

import numpy as np
import pytest

import faiss_amd as faiss
import scan_order as SO
from oracle import oracle as O

pytestmark = pytest.mark.gpu

KS = (1, 10, 16, 64, 100, 200, 300, 400, 1000)
KS_ROWK = (1, 10, 16)
ROWK_NLIST, ROWK_PLACE = 1032, (0, 1023, 1024, 1031)  # both sides of the planner's 1024-list block
METRICS = pytest.mark.parametrize("metric", [SO.L2, SO.IP])
ORDERS = pytest.mark.parametrize("order", SO.ORDERS)


@functools.lru_cache(maxsize=None)
def make_pair(shape, metric, order, nlist=4, place=(0, 1, 2, 3)):
    c = SO.pq_contents(shape, metric, order, nlist, place)
    ip = metric == SO.IP
    ix = faiss.IndexIVFPQ(None, c.d, nlist, c.M, 8, faiss.METRIC_INNER_PRODUCT if ip else faiss.METRIC_L2, device=0)
    ix.set_trained(c.cent, c.cb)
    ix.add_preencoded(c.list_no, c.codes, c.ids)
    ox = O.OracleIVFPQ(c.d, nlist, c.M, metric=O.METRIC_INNER_PRODUCT if ip else O.METRIC_L2)
    ox.set_trained(c.cent, c.cb)
    ox.add_preencoded(c.list_no, c.codes, c.ids)
    ox.nthreads = min(ox.nthreads, 8)  # 13 queries: a thread per core of a large host costs more than the search
    return ix, ox, c


def check(got, ref, msg):
    np.testing.assert_array_equal(got[1], ref[1], err_msg=msg)
    np.testing.assert_array_equal(got[0], ref[0], err_msg=msg)


def all_lists(c):
    """Probe rows naming all four lists, each query starting at another one."""
    nq = len(c.xq)
    return np.stack([np.roll(SO.probe_rows(c, 1, range(4))[0], q) for q in range(nq)])


@ORDERS
@METRICS
@pytest.mark.parametrize("shape", list(SO.PQ_SHAPES))
def test_every_class_matches_oracle(shape, metric, order):
    """nlist = 4: k_scan_lean (k <= 16 at M <= 16) and k_scan_lists in every (M, R) class."""
    ix, ox, c = make_pair(shape, metric, order)
    e0, rs0 = ix.error_count(), ix.repair_stats()
    one = SO.probe_rows(c, len(c.xq), [0])
    d_one = SO.dis0(c, c.xq, one)
    for k in KS:
        ix.nprobe = ox.nprobe = 4
        got, ref = ix.search(c.xq, k), ox.search(c.xq, k)
        check(got, ref, f"search nprobe=4 k={k}")
        ix.nprobe = ox.nprobe = 1
        ref = ox.search_preassigned(c.xq, k, one, d_one)
        np.testing.assert_array_equal(ref[1][0], SO.expected_ids(c.list_ids[0], order, k))
        check(ix.search_preassigned(c.xq, k, one, d_one), ref, f"preassigned nprobe=1 k={k}")
    assert ix.error_count() == e0
    assert ix.repair_stats() == rs0


@ORDERS
@METRICS
@pytest.mark.parametrize("shape", ["d32_m8", "d64_m16"])
def test_row_packed_scan_matches_oracle(shape, metric, order):
    """nlist = 1032 (the non-fused plan): k <= 16 runs the row-packed k_scan_lists (drain_rows).
    The probes are given, since a coarse search over 1032 centroids would pick other lists."""
    ix, ox, c = make_pair(shape, metric, order, ROWK_NLIST, ROWK_PLACE)
    e0, rs0 = ix.error_count(), ix.repair_stats()
    for rows in (all_lists(c), SO.probe_rows(c, len(c.xq), [0])):
        ix.nprobe = ox.nprobe = rows.shape[1]
        dq = SO.dis0(c, c.xq, rows)
        for k in KS_ROWK:
            ref = ox.search_preassigned(c.xq, k, rows, dq)
            if rows.shape[1] == 1:
                np.testing.assert_array_equal(ref[1][0], SO.expected_ids(c.list_ids[0], order, k))
            check(ix.search_preassigned(c.xq, k, rows, dq), ref, f"nprobe={rows.shape[1]} k={k}")
    assert ix.error_count() == e0
    assert ix.repair_stats() == rs0


@METRICS
@pytest.mark.parametrize("shape,k", [("d64_m16", 100), ("d128_m64", 400)])
def test_improving_batches_in_flight(shape, k, metric):
    """Batches in flight on two streams, each into its own output buffers, equal the
    one-at-a-time searches (and so the oracle), with no stale read or repair."""
    import torch

    ix, ox, c = make_pair(shape, metric, "improving")
    ix.nprobe = ox.nprobe = 4
    nq, nb = len(c.xq), 8
    rng = np.random.default_rng(77)
    batches = [c.xq[rng.permutation(nq)] for _ in range(nb)]
    xd = [torch.from_numpy(b).cuda() for b in batches]
    ref = []
    for b in range(nb):
        D, I = ix.search_device(xd[b], k)
        torch.cuda.synchronize()
        ref.append((D.cpu().numpy(), I.cpu().numpy()))
    for b in (0, nb - 1):
        check(ref[b], ox.search(batches[b], k), f"batch {b}")
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [(torch.empty((nq, k), device="cuda"), torch.empty((nq, k), dtype=torch.int64, device="cuda"))
            for _ in range(nb)]
    e0, rs0 = ix.error_count(), ix.repair_stats()
    ix.inflight = True
    try:
        torch.cuda.synchronize()
        for b in range(nb):
            ix.search_device(xd[b], k, outs[b][0], outs[b][1], stream=streams[b % 2].cuda_stream)
        torch.cuda.synchronize()
    finally:
        ix.inflight = False
    for b in range(nb):
        check((outs[b][0].cpu().numpy(), outs[b][1].cpu().numpy()), ref[b], f"batch {b}")
    assert ix.repair_stats() == rs0
    assert ix.error_count() == e0
