"""The item-wide bound of k_scan_lean: what an item leaves in tau_q is the k-th smallest key of
the union of its four waves' partial lists, not the best of the four per-wave k-th keys.

Results.  D and I equal the CPU oracle's bit for bit in every case: M = 8 (the one-pass form)
and M = 16 (the split form), k = 1, 10, 16, L2 and the inner product, nprobe = 1 and 4,
`search_preassigned` and the plain search, the three key orders of tests/scan_order.py (whose
preconditions tests/test_scan_order_cpu.py holds), and once with batches in flight on two
streams.

The bound.  After a one-batch search the workspace still holds the scan's partial lists
(`ivfpq_debug_workspace` what = 0: per (query, probe, wave) k records {key bits, tag, position})
and the tau words (what = 3).  Per query the host takes, over the query's scanned pairs (the
probe mask the merges read, what = 2: an empty list is not scanned and its slots hold anything), the
minimum of the k-th smallest key of the union of the pair's four lists; a pair whose union has
fewer than k real entries is left out.  The tau word must EQUAL the ordered word of that
minimum under the batch's tag: everything else the kernel publishes (a wave's k-th, the loose
bound T of a wave's lane minima) is k real codes of one wave, so it is at least the item-wide
k-th.  A query without such a pair has no wave with k entries either, so its word must not
carry the batch's tag at all.

That the equality can fail.  For k > 1 it separates the item-wide rule from the per-wave one
only where the best k rows of a list lie in more than one wave's quarter (chunk j of a
super-batch at sb: wave w scans rows sb + 256 j + 64 w .. + 63).  For the designated query that
is NOT so in the 4700-row list: `worsening` has its best 16 rows at positions 0..15 and
`improving` at 4684..4699, which are wave 0's and wave 1's alone (4672..4699 is wave 1's
share of the last super-batch), and `one_wave` is in wave 0 by construction.  It is so in the
1537-row list in `improving` order: the best row, 1536, is the one row of the second
super-batch (wave 0), the next fifteen, 1521..1535, are wave 3's (1472..1535).  So the
condition "item-wide minimum strictly below the smallest per-wave k-th key" is computed from
the partial lists and asserted there, for every (M, k > 1, metric); in the cases where all of
a list's best rows are one wave's, and at k = 1, the two are asserted equal.  A library built
with -DSCAN_ITEM_BOUND=0 fails the equality in the strict cases (profiles/scan_item_bound.md).

Boundaries: a workgroup's last item (nprobe = 1 on one list: every workgroup's only item is
its last), items with fewer than four pairs (13 queries on one list: 4 + 4 + 4 + 1), lists of
more than one super-batch (4700 and 1537 rows), the empty list, and a list of 7 rows, shorter
than k = 10 and 16 (a fifth list, in an index of its own).
"""
import functools

import numpy as np
import pytest

import faiss_amd as faiss
import merge_paths as MP
import scan_order as SO
from oracle import oracle as O

pytestmark = pytest.mark.gpu

KS = (1, 10, 16)
SHAPES = ("d32_m8", "d64_m16")
SHORT = 7                                   # rows of the list shorter than k
SIZES5 = SO.SIZES + (SHORT,)
METRICS = pytest.mark.parametrize("metric", [SO.L2, SO.IP])
ORDERS = pytest.mark.parametrize("order", SO.ORDERS)
SHAPE = pytest.mark.parametrize("shape", SHAPES)
NONE32 = 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def make_pair(shape, metric, order, short=False):
    if short:
        c = SO.pq_contents(shape, metric, order, nlist=5, place=(0, 1, 2, 3, 4), sizes=SIZES5)
    else:
        c = SO.pq_contents(shape, metric, order)
    ip = metric == SO.IP
    ix = faiss.IndexIVFPQ(None, c.d, c.nlist, c.M, 8, faiss.METRIC_INNER_PRODUCT if ip else faiss.METRIC_L2, device=0)
    ix.set_trained(c.cent, c.cb)
    ix.add_preencoded(c.list_no, c.codes, c.ids)
    ox = O.OracleIVFPQ(c.d, c.nlist, c.M, metric=O.METRIC_INNER_PRODUCT if ip else O.METRIC_L2)
    ox.set_trained(c.cent, c.cb)
    ox.add_preencoded(c.list_no, c.codes, c.ids)
    ox.nthreads = min(ox.nthreads, 8)
    return ix, ox, c


def check(got, ref, msg):
    np.testing.assert_array_equal(got[1], ref[1], err_msg=msg)
    np.testing.assert_array_equal(got[0], ref[0], err_msg=msg)


def kth_smallest(u, k):
    return None if u.size < k else int(np.partition(u, k - 1)[k - 1])


def bounds(ix, before, nq, nprobe, k):
    """Of the one batch searched since `before` = MP.epochs(ix): per query the tau word, the
    word the item-wide rule asks for (None: no pair with k entries), and the smallest per-wave
    k-th key word (None: no wave with k entries)."""
    after = MP.epochs(ix)
    moved = [ws for ws in range(3) if after[ws] != before[ws]]
    assert len(moved) == 1 and after[moved[0]] == before[moved[0]] + 1, (before, after)
    ws, epoch = moved[0], after[moved[0]]
    nslot = nq * nprobe * 4
    part, pbytes = MP._ws(ix, ws, 0, np.uint32)
    assert pbytes >= nslot * k * 16, (pbytes, nslot * k * 16)
    rec = part[:nslot * k * 4].reshape(nq, nprobe, 4, k, 4)
    expect = ((epoch * MP.TAG_MULT + np.arange(nslot, dtype=np.int64)) & MP.TAG_MASK).reshape(nq, nprobe, 4, 1)
    # the probes the scan covered (what = 2, read by the merges): an empty list has no item, and its
    # slots hold whatever the memory held, possibly another handle's records of the same epoch
    qmw = (nprobe + 63) // 64
    qm, qbytes = MP._ws(ix, ws, 2, np.uint64)
    assert qbytes >= nq * qmw * 8
    p = np.arange(nprobe)
    scanned = ((qm[:nq * qmw].reshape(nq, qmw)[:, p >> 6] >> (p & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)
    fresh = (rec[..., 1].astype(np.int64) & MP.TAG_MASK) == expect          # written by this batch's scan
    assert fresh[scanned].all(), "a scanned pair's records are not this batch's"
    real = fresh & scanned[:, :, None, None]
    real &= ~((rec[..., 2] == NONE32) & (rec[..., 3] == NONE32))            # position -1: an empty entry
    keys = np.where(real, np.ascontiguousarray(rec[..., 0]).view(np.float32), np.float32(0))  # (others: any bits)
    u = MP.ukeys(keys)
    tau, tbytes = MP._ws(ix, ws, 3, np.uint64)
    assert tbytes >= nq * 8
    tag = np.uint64((~epoch) & NONE32)
    out = []
    for q in range(nq):
        item, wave = [], []
        for p in range(nprobe):
            item.append(kth_smallest(u[q, p][real[q, p]], k))
            wave += [kth_smallest(u[q, p, w][real[q, p, w]], k) for w in range(4)]
        item = [v for v in item if v is not None]
        wave = [v for v in wave if v is not None]
        out.append((int(tau[q]), (int(tag) << 32 | min(item)) if item else None, min(wave) if wave else None))
        if not item:
            assert not wave
    return out, int(tag)


def check_bounds(got, tag, msg):
    for q, (tau, want, _) in enumerate(got):
        if want is None:
            assert tau >> 32 != tag, f"{msg}: query {q} has a bound {tau:#x} but no pair with k entries"
        else:
            assert tau == want, f"{msg}: query {q} tau {tau:#x}, item-wide k-th {want:#x}"


def searched(ix, ox, c, k, rows, plain):
    """One batch through the GPU and the oracle; (bounds, tag) of the GPU's."""
    nq, nprobe = rows.shape
    ix.nprobe = ox.nprobe = nprobe
    before = MP.epochs(ix)
    if plain:
        got, ref = ix.search(c.xq, k), ox.search(c.xq, k)
    else:
        dq = SO.dis0(c, c.xq, rows)
        got, ref = ix.search_preassigned(c.xq, k, rows, dq), ox.search_preassigned(c.xq, k, rows, dq)
    msg = f"{'search' if plain else 'preassigned'} nprobe={nprobe} k={k}"
    check(got, ref, msg)
    b, tag = bounds(ix, before, nq, nprobe, k)
    check_bounds(b, tag, msg)
    return b


@ORDERS
@METRICS
@SHAPE
def test_tau_is_the_item_wide_kth(shape, metric, order):
    ix, ox, c = make_pair(shape, metric, order)
    e0, rs0 = ix.error_count(), ix.repair_stats()
    nq = len(c.xq)
    every = np.stack([np.roll(SO.probe_rows(c, 1, range(4))[0], q) for q in range(nq)])
    for k in KS:
        for plain in (False, True):
            searched(ix, ox, c, k, every, plain)
            searched(ix, ox, c, k, SO.probe_rows(c, nq, [0]), plain)
        # one list of 4700 rows for every query: for the designated query its best rows are one wave's
        _, want, wave = searched(ix, ox, c, k, SO.probe_rows(c, nq, [0]), False)[0]
        assert want is not None and want & NONE32 == wave
        # the 1537-row list: in `improving` order its best k > 1 rows are in waves 0 and 3
        _, want, wave = searched(ix, ox, c, k, SO.probe_rows(c, nq, [1]), False)[0]
        assert want is not None
        if order == "improving" and k > 1:
            assert want & NONE32 < wave, f"k={k}: the item-wide k-th is not below every wave's own"
        else:
            assert want & NONE32 == wave
        # the empty list alone: no bound at all
        assert all(w is None for _, w, _ in searched(ix, ox, c, k, SO.probe_rows(c, nq, [3]), False))
    assert ix.error_count() == e0
    assert ix.repair_stats() == rs0


@METRICS
@SHAPE
def test_list_shorter_than_k(shape, metric):
    """A 7-row list: at k = 10 and 16 its items publish nothing (the union has 7 entries), at
    k = 1 they do; beside the other lists the query's bound comes from those."""
    ix, ox, c = make_pair(shape, metric, "improving", short=True)
    e0, rs0 = ix.error_count(), ix.repair_stats()
    nq = len(c.xq)
    for k in KS:
        alone = searched(ix, ox, c, k, SO.probe_rows(c, nq, [4]), False)
        assert all((w is None) == (k > SHORT) for _, w, _ in alone)
        searched(ix, ox, c, k, SO.probe_rows(c, nq, [4, 2, 3, 0, 1]), False)
        searched(ix, ox, c, k, SO.probe_rows(c, nq, [4, 3]), False)
    assert ix.error_count() == e0
    assert ix.repair_stats() == rs0


@METRICS
@SHAPE
def test_batches_in_flight(shape, metric):
    """Two streams in flight: the bounds of concurrent items must never prune a result."""
    import torch

    k = 10
    ix, ox, c = make_pair(shape, metric, "improving")
    ix.nprobe = ox.nprobe = 4
    nq, nb = len(c.xq), 8
    rng = np.random.default_rng(78)
    batches = [c.xq[rng.permutation(nq)] for _ in range(nb)]
    xd = [torch.from_numpy(b).cuda() for b in batches]
    ref = [ox.search(b, k) for b in batches]
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
