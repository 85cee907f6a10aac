"""Item composition of the list scan: a list's first-probe (lead) items take the
list's other pairs into their free slots (ivfpq_kernels.hip list_items).

A list with c0 kind-0 pairs (a query's first usable probe) and c1 kind-1 pairs
forms ceil((c0 + c1) / G) items; the first ceil(c0 / G) are lead items.  Which
item carries a pair must change nothing in the results, so every search here is
compared bit for bit with the CPU oracle, on integer-valued tables (many exact
ties).  The probe rows are built by hand, so every list's (c0, c1) is known:

* scenario "c0_0to5": c0 = 0, 1, 2, 3, 4, 5 with c1 >= 10;
* scenario "c0_1": c0 = 1 (f = 3 free slots at G = 4) with c1 = 0, 1 (< f), 3 (= f),
  4 and 5, and c0 = 4 exactly (no mixing);
* scenario "range": a shard that keeps lists [1, 7) of the 8.

Rows carry -1 entries, the empty list 3 and (range) lists outside the shard in
front of their first usable probe, so "first usable probe" is not probe 0, and one
row has no usable probe at all.  Lists 1 and 2 hold 1537 and 3073 codes (longer
than one and two super-batches of the lean scan) and always get a mixed item.

For the shapes the lean scan serves (G = 4) the item counts the scan leaves in
hdr[0] / hdr[1] must equal sum ceil((c0 + c1) / 4) and sum ceil(c0 / 4), computed
here from the probe rows over usable pairs only.
"""
import ctypes
import functools

import numpy as np
import pytest

import faiss_amd as faiss
from faiss_amd import _lib
from oracle import oracle as O

pytestmark = pytest.mark.gpu

NLIST = 8
SIZES = [300, 1537, 3073, 0, 65, 257, 100, 40]
SHAPES = {"d64_m16": (64, 16), "d32_m8": (32, 8)}
G = 4  # pairs per item of the lean scan (k <= 16, M = 8 or 16)

# scenario -> (list range, nprobe, {list: (c0, c1)})
SCENARIOS = {
    "c0_0to5": ((0, 8), 9, {0: (0, 15), 1: (1, 14), 2: (2, 13), 4: (3, 12), 5: (4, 11), 6: (5, 10), 7: (0, 15)}),
    "c0_1": ((0, 8), 6, {0: (1, 0), 1: (1, 1), 2: (1, 3), 4: (1, 4), 5: (1, 5), 6: (4, 2), 7: (0, 6)}),
    "range": ((1, 7), 7, {1: (1, 3), 2: (2, 5), 4: (0, 4), 5: (5, 2), 6: (1, 0)}),
}


def make_rows(spec, nprobe, unusable, seed):
    """Probe rows [nq, nprobe] in which list l is the first usable probe of c0 rows and
    a later probe of c1 rows, spec = {l: (c0, c1)}.  The other entries are `unusable`
    list numbers (each at most once per row) and -1; row i has i mod (pads + 1) of them
    in front of its first usable probe.  The last row has no usable probe."""
    rng = np.random.default_rng(seed)
    rows = [[l] for l, (c0, _) in spec.items() for _ in range(c0)]
    for l, (_, c1) in spec.items():
        cand = sorted((r for r in rows if l not in r), key=len)  # (stable: least filled first)
        assert len(cand) >= c1, (l, c1)
        for r in cand[:c1]:
            r.append(l)
    out = np.full((len(rows) + 1, nprobe), -1, np.int64)
    for i, r in enumerate(rows):
        npad = nprobe - len(r)
        assert npad >= 0, r
        pads = (list(unusable) + [-1] * nprobe)[:npad]
        pads = [pads[(i + j) % npad] for j in range(npad)] if npad else []
        nfront = i % (npad + 1)
        rest = r[1:] + pads[nfront:]
        rng.shuffle(rest)
        out[i] = pads[:nfront] + [r[0]] + rest
    out[-1, :len(unusable)] = unusable
    return out


def pair_counts(rows, lo, hi):
    """Per list (c0, c1) of the usable pairs of the rows: in range and not empty."""
    c = np.zeros((NLIST, 2), np.int64)
    for row in rows:
        first = True
        for l in row:
            if lo <= l < hi and SIZES[l] > 0:
                c[l, 0 if first else 1] += 1
                first = False
    return c


def expected_items(rows, lo, hi, g=G):
    c = pair_counts(rows, lo, hi)
    return int(np.sum(-(-(c[:, 0] + c[:, 1]) // g))), int(np.sum(-(-c[:, 0] // g)))


def epochs(ix):
    """The epoch (batches planned so far) of each of the handle's workspaces."""
    lib = _lib.load()
    out = []
    for ws in range(3):
        nb = ctypes.c_int64(0)
        ep = np.zeros(1, np.uint64)
        _lib.check(lib.ivfpq_debug_workspace(ix._h, ws, 7, ep.ctypes.data, 8, ctypes.byref(nb)))
        out.append(int(ep[0]))
    return out


def item_counts(ix, before):
    """hdr[0], hdr[1] of the workspace that planned the one batch searched since
    `before` = epochs(ix).  A handle keeps three workspaces and takes the least recently
    used one once the previous call has been waited for, as the reads here do, so the
    latest batch's workspace is the one whose epoch moved, not the largest epoch."""
    after = epochs(ix)
    moved = [ws for ws in range(3) if after[ws] != before[ws]]
    assert len(moved) == 1 and after[moved[0]] == before[moved[0]] + 1, (before, after)
    nb = ctypes.c_int64(0)
    hdr = np.zeros(16, np.int32)
    _lib.check(_lib.load().ivfpq_debug_workspace(ix._h, moved[0], 4, hdr.ctypes.data, hdr.nbytes, ctypes.byref(nb)))
    assert nb.value >= hdr.nbytes
    return int(hdr[0]), int(hdr[1])


@functools.lru_cache(maxsize=None)
def make_pair(shape, metric, lo, hi, nq):
    """GPU index and oracle on the same integer-valued tables and codes; lists outside
    [lo, hi) stay empty in both (the shard keeps its own lists only)."""
    d, M = SHAPES[shape]
    ip = metric == "ip"
    rng = np.random.default_rng(4100 + 10 * list(SHAPES).index(shape) + ip)
    cent = rng.integers(-3, 4, size=(NLIST, d)).astype(np.float32)
    cb = rng.integers(-2, 3, size=(M, 256, d // M)).astype(np.float32)
    xq = rng.integers(-3, 4, size=(nq, d)).astype(np.float32)
    sizes = [s if lo <= l < hi else 0 for l, s in enumerate(SIZES)]
    n = int(np.sum(sizes))
    codes = rng.integers(0, 256, size=(n, M), dtype=np.uint8)
    list_no = np.repeat(np.arange(NLIST, dtype=np.int64), sizes)
    ids = np.arange(n, dtype=np.int64) * 3 + 1
    ix = faiss.IndexIVFPQ(None, d, NLIST, M, 8, faiss.METRIC_INNER_PRODUCT if ip else faiss.METRIC_L2, device=0)
    ix.set_trained(cent, cb)
    if (lo, hi) != (0, NLIST):
        ix.set_list_range(lo, hi)
    ix.add_preencoded(list_no, codes, ids)
    ox = O.OracleIVFPQ(d, NLIST, M, metric=O.METRIC_INNER_PRODUCT if ip else O.METRIC_L2)
    ox.set_trained(cent, cb)
    ox.add_preencoded(list_no, codes, ids)
    return ix, ox, xq


def scenario(name, shape, metric):
    (lo, hi), nprobe, spec = SCENARIOS[name]
    unusable = [3] + [l for l in range(NLIST) if not lo <= l < hi]
    rows = make_rows(spec, nprobe, unusable, seed=len(name))
    c = pair_counts(rows, lo, hi)
    for l in range(NLIST):  # the rows give every list the counts the scenario names
        assert tuple(c[l]) == spec.get(l, (0, 0)), (l, tuple(c[l]))
    ix, ox, xq = make_pair(shape, metric, lo, hi, 16)
    xq = xq[np.arange(rows.shape[0]) % xq.shape[0]]
    # L2: integer dis0 per pair; IP: the scan's own <x, centroid>
    dq = None if metric == "ip" else np.random.default_rng(5).integers(0, 5, size=rows.shape).astype(np.float32)
    return ix, ox, xq, rows, dq, (lo, hi)


def check(got, ref, msg):
    np.testing.assert_array_equal(got[1], ref[1], err_msg=msg)
    np.testing.assert_array_equal(got[0], ref[0], err_msg=msg)


@pytest.mark.parametrize("name", list(SCENARIOS))
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_preassigned_rows_match_oracle(shape, metric, name):
    import torch

    ix, ox, xq, rows, dq, (lo, hi) = scenario(name, shape, metric)
    ix.nprobe = rows.shape[1]
    e0 = ix.error_count()
    want = expected_items(rows, lo, hi)
    for k in (1, 10, 16, 100):  # k <= 16: the lean scan (G = 4); k = 100: k_scan_lists (G = 2)
        ref = ox.search_preassigned(xq, k, rows, dq)
        ep = epochs(ix)
        check(ix.search_preassigned(xq, k, rows, dq), ref, f"k={k}")
        if k <= 16:
            got = item_counts(ix, ep)
            print(f"{shape} {metric} {name} k={k}: items (all, lead) {got}, expected {want}")
            assert got == want, f"k={k}"
    xd, rd = torch.from_numpy(xq).cuda(), torch.from_numpy(rows).cuda()
    dd = torch.from_numpy(dq).cuda() if dq is not None else None
    for k in (10, 100):
        D, I = ix.search_preassigned_device(xd, k, rd, dd)
        torch.cuda.synchronize()
        check((D.cpu().numpy(), I.cpu().numpy()), ox.search_preassigned(xq, k, rows, dq), f"device k={k}")
    assert ix.error_count() == e0


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_single_probe_has_lead_items_only(shape, metric):
    """nprobe = 1: no kind-1 pair exists, every item is a lead item."""
    ix, ox, xq = make_pair(shape, metric, 0, NLIST, 16)
    rows = np.array([1, 1, 1, 1, 1, 2, -1, 3, 4, 4, 6, 2, 7, 0, 5, 5, 5, 5, 5], np.int64).reshape(-1, 1)
    xq = xq[np.arange(rows.shape[0]) % xq.shape[0]]
    ix.nprobe = 1
    want = expected_items(rows, 0, NLIST)
    assert want[0] == want[1]
    for k in (1, 10, 16, 100):
        ep = epochs(ix)
        check(ix.search_preassigned(xq, k, rows), ox.search_preassigned(xq, k, rows), f"k={k}")
        if k <= 16:
            assert item_counts(ix, ep) == want, f"k={k}"
    assert ix.error_count() == 0


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_plain_search_matches_oracle(shape, metric):
    """The full search (coarse step, planning in its epilogue): 37 queries over 8 lists,
    so every list has c0 + c1 of about 14 (nprobe 3) or 32 to 37 (nprobe 8)."""
    ix, ox, xq = make_pair(shape, metric, 0, NLIST, 37)
    for nprobe in (3, 8):
        ix.nprobe = ox.nprobe = nprobe
        for k in (1, 10, 16, 100):
            check(ix.search(xq, k), ox.search(xq, k), f"nprobe={nprobe} k={k}")
    assert ix.error_count() == 0


@pytest.mark.parametrize("nlist", [1032, 4104], ids=["plan_small", "plan_big"])
def test_non_fused_planner_matches_oracle(nlist):
    """More than 1024 lists in the shard (scan_fused_plan: nloc <= 1024) send the items
    through k_plan_items_small (nloc <= 4096) or k_plan_items_big and k_scan_lists.  Eight
    lists on both sides of the 1024-list blocks of the planners hold the codes; the rows of
    scenario "c0_1" and "c0_0to5" address them."""
    d, M = SHAPES["d32_m8"]
    place = [0, 1, 1023, 7, 1024, 1025, nlist - 2, nlist - 1]  # list l of the scenarios -> list place[l]
    rng = np.random.default_rng(nlist)
    cent = rng.integers(-3, 4, size=(nlist, d)).astype(np.float32)
    cb = rng.integers(-2, 3, size=(M, 256, d // M)).astype(np.float32)
    n = int(np.sum(SIZES))
    codes = rng.integers(0, 256, size=(n, M), dtype=np.uint8)
    list_no = np.repeat(np.asarray(place, np.int64), SIZES)
    ids = np.arange(n, dtype=np.int64) * 3 + 1
    ix = faiss.IndexIVFPQ(None, d, nlist, M, 8, faiss.METRIC_L2, device=0)
    ix.set_trained(cent, cb)
    ix.add_preencoded(list_no, codes, ids)
    ox = O.OracleIVFPQ(d, nlist, M)
    ox.set_trained(cent, cb)
    ox.add_preencoded(list_no, codes, ids)
    for name in ("c0_1", "c0_0to5"):
        _, nprobe, spec = SCENARIOS[name]
        rows0 = make_rows(spec, nprobe, [3], seed=len(name))
        rows = np.where(rows0 >= 0, np.asarray(place, np.int64)[np.maximum(rows0, 0)], -1)
        xq = rng.integers(-3, 4, size=(rows.shape[0], d)).astype(np.float32)
        dq = rng.integers(0, 5, size=rows.shape).astype(np.float32)
        ix.nprobe = nprobe
        want = expected_items(rows0, 0, NLIST)
        for k in (1, 10, 100):
            ep = epochs(ix)
            check(ix.search_preassigned(xq, k, rows, dq), ox.search_preassigned(xq, k, rows, dq), f"{name} k={k}")
            if k <= 16:  # G = 4; the planner kernel wrote the counts
                assert item_counts(ix, ep) == want, f"{name} k={k}"
    assert ix.error_count() == 0


def test_two_streams_in_flight():
    """Batches in flight on two streams equal the one-at-a-time searches (and so the
    oracle), with no stale read, no repair and no index error."""
    import torch

    ix, ox, xq, rows, dq, _ = scenario("c0_0to5", "d64_m16", "l2")
    ix.nprobe = rows.shape[1]
    k, nb = 10, 8
    rng = np.random.default_rng(77)
    perms = [rng.permutation(rows.shape[0]) for _ in range(nb)]
    xd = [torch.from_numpy(xq[p]).cuda() for p in perms]
    rd = [torch.from_numpy(rows[p]).cuda() for p in perms]
    dd = [torch.from_numpy(dq[p]).cuda() for p in perms]
    ref = []
    for b in range(nb):
        D, I = ix.search_preassigned_device(xd[b], k, rd[b], dd[b])
        torch.cuda.synchronize()
        ref.append((D.cpu().numpy(), I.cpu().numpy()))
    for b in (0, nb - 1):
        check(ref[b], ox.search_preassigned(xq[perms[b]], k, rows[perms[b]], dq[perms[b]]), f"batch {b}")
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [(torch.empty((rows.shape[0], k), device="cuda"),
             torch.empty((rows.shape[0], k), dtype=torch.int64, device="cuda")) for _ in range(nb)]
    e0, rs0 = ix.error_count(), ix.repair_stats()
    ix.inflight = True
    try:
        torch.cuda.synchronize()
        for b in range(nb):
            ix.search_preassigned_device(xd[b], k, rd[b], dd[b], outs[b][0], outs[b][1],
                                         stream=streams[b % 2].cuda_stream)
        torch.cuda.synchronize()
    finally:
        ix.inflight = False
    for b in range(nb):
        check((outs[b][0].cpu().numpy(), outs[b][1].cpu().numpy()), ref[b], f"batch {b}")
    rs = ix.repair_stats()
    assert (rs[0] - rs0[0], rs[1] - rs0[1]) == (0, 0)
    assert ix.error_count() == e0
