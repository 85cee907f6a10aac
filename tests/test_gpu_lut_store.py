"""Every slot of the list scan's LUT, in every pair position g, against the CPU oracle bit for bit.

The table build of k_scan_lean stores an item's LUT -- T1[list] - 2 T3[query] (L2) or -T3[query]
(inner product), four pairs interleaved -- into LDS in one of three forms (ivfpq_kernels.hip,
SCAN_LUT_DWORD and SCAN_LUT_ROTATE): a thread holds one column of a pass's rows, or four
consecutive entries of a row, stored in order or rotated by its lane (lut_store4).  A slot
that got another slot's value, or a pair another pair's, changes only the keys of the codes
that read it, so the contents here make every slot read, and make it matter:

  * 16 lists of 16 rows; row i of list L has code byte m = ((16 L + i) (2 m + 1) + 17 m) mod 256,
    so every sub-quantizer m sees each of the 256 byte values once across the lists;
  * four distinct queries per list, each probing that list alone, at k = 16: one item of four
    pairs per list, and all 16 rows of every pair come back, so a wrong entry in any g shows
    in D (and, usually, in the order of I);
  * the codebook and the centroids are random reals, so no two entries of a table agree;
  * lists 16, 17 and 18 are probed by 1, 2 and 3 queries: items with absent pairs;
  * list 19 holds 1537 rows (tests/scan_order.py's list of one super-batch + 1, in its
    `improving` order for the list's first query): the two-pass scan rebuilds the low half
    of the LUT from the table rows for the second super-batch.

The queries sit next to their list's centroid (8 e_L plus noise), so the plain search with
nprobe = 1 probes the same lists as search_preassigned; both are compared with the oracle,
for M = 8 and 16 and both metrics.  The same contents at k = 100 (M = 16 and 32: items of two
pairs, 8-byte LUT vectors) and at M = 32 and 64 (M = 64: one pair, 4-byte vectors) go through
the build of k_scan_lists; there a short list returns its 16 rows and 84 empty entries.  The
file looks at results only; every build form must pass it (profiles/build_variants.sh:
`lutlinear`, `lutrotate`).
"""
import functools

import numpy as np
import pytest

import faiss_amd as faiss
import scan_order as SO
from oracle import oracle as O

pytestmark = pytest.mark.gpu

F = np.float32
K = 16
# (shape, k): k_scan_lean, then the classes of k_scan_lists with G = 2 and G = 1 pairs per item
CASES = [("d32_m8", K), ("d64_m16", K), ("d64_m16", 100), ("d64_m32", K), ("d64_m32", 100), ("d128_m64", K)]
N_FULL, ROWS = 16, 16                  # lists probed by four queries, rows per short list
PARTIAL = ((16, 1), (17, 2), (18, 3))  # (list, queries probing it)
LONG, LONG_ROWS = 19, SO.SIZES[1]      # one JB = 6 super-batch + 1
NLIST = 20


def code_bytes(M, row_no):
    """Code byte m of the short lists' row number 16 L + i."""
    m = np.arange(M, dtype=np.int64)
    return ((row_no[:, None] * (2 * m + 1) + 17 * m) % 256).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def contents(shape, metric):
    d, M = SO.PQ_SHAPES[shape]
    rng = np.random.default_rng(SO.seed_of("lut_store", shape, metric))
    cent = rng.uniform(-0.5, 0.5, size=(NLIST, d)).astype(F)
    cent[np.arange(NLIST), np.arange(NLIST)] += 8
    cb = rng.standard_normal((M, 256, d // M)).astype(F)
    probed = [(L, 4) for L in range(N_FULL)] + list(PARTIAL) + [(LONG, 4)]
    rows = np.concatenate([np.full(n, L, np.int64) for L, n in probed])[:, None]
    xq = (cent[rows[:, 0]] + rng.uniform(-0.5, 0.5, size=(len(rows), d))).astype(F)
    assert len(np.unique(xq, axis=0)) == len(xq)

    n_short = (N_FULL + len(PARTIAL)) * ROWS
    row_no = np.arange(n_short, dtype=np.int64)
    codes_short = code_bytes(M, row_no)
    for m in range(M):  # every byte value once per sub-quantizer across the 16 full lists
        assert len(np.unique(codes_short[:N_FULL * ROWS, m])) == 256
    cand = rng.integers(0, 256, size=(SO.DRAW * LONG_ROWS, M), dtype=np.uint8)
    q_long = xq[np.nonzero(rows[:, 0] == LONG)[0][0]]
    pos = SO.arrange(SO.pq_keys(cent[LONG], cb, q_long, cand, metric).astype(F), LONG_ROWS, "improving", rng)
    list_no = np.concatenate([row_no // ROWS, np.full(LONG_ROWS, LONG, np.int64)])
    ids = np.concatenate([SO.list_ids(L, ROWS) for L in range(N_FULL + len(PARTIAL))] + [SO.list_ids(LONG, LONG_ROWS)])
    codes = np.ascontiguousarray(np.concatenate([codes_short, cand[pos]]))

    ip = metric == SO.IP
    ix = faiss.IndexIVFPQ(None, d, NLIST, M, 8, faiss.METRIC_INNER_PRODUCT if ip else faiss.METRIC_L2, device=0)
    ix.set_trained(cent, cb)
    ix.add_preencoded(list_no, codes, ids)
    ox = O.OracleIVFPQ(d, NLIST, M, metric=O.METRIC_INNER_PRODUCT if ip else O.METRIC_L2)
    ox.set_trained(cent, cb)
    ox.add_preencoded(list_no, codes, ids)
    ox.nthreads = min(ox.nthreads, 8)
    ix.nprobe = ox.nprobe = 1
    if ip:
        dis0 = None
    else:
        dis0 = ((xq.astype(np.float64) - cent[rows[:, 0]].astype(np.float64)) ** 2).sum(1).astype(F)[:, None]
    return ix, ox, xq, rows, dis0


def check(got, ref, rows, msg):
    # the reference itself returns what the test is about: all 16 rows of the probed list
    # (the k best of the long one), nothing of any other list, and empty entries behind them
    want = 1_000_000 * (rows + 1)
    assert ((ref[1] == -1) | ((ref[1] >= want) & (ref[1] < want + 1_000_000))).all(), msg
    short = rows[:, 0] != LONG
    np.testing.assert_array_equal(np.sort(ref[1][short][:, :ROWS], axis=1),
                                  want[short] + 3 * np.arange(ROWS, dtype=np.int64)[None, :], err_msg=msg)
    assert (ref[1][short][:, ROWS:] == -1).all() and (ref[1][~short] >= 0).all(), msg
    np.testing.assert_array_equal(got[1], ref[1], err_msg=msg)
    np.testing.assert_array_equal(got[0], ref[0], err_msg=msg)


@pytest.mark.parametrize("metric", [SO.L2, SO.IP])
@pytest.mark.parametrize("shape,k", CASES)
def test_preassigned_reads_every_slot(shape, k, metric):
    ix, ox, xq, rows, dis0 = contents(shape, metric)
    e0, rs0 = ix.error_count(), ix.repair_stats()
    check(ix.search_preassigned(xq, k, rows, dis0), ox.search_preassigned(xq, k, rows, dis0), rows, "preassigned")
    assert ix.error_count() == e0
    assert ix.repair_stats() == rs0


@pytest.mark.parametrize("metric", [SO.L2, SO.IP])
@pytest.mark.parametrize("shape,k", CASES)
def test_search_reads_every_slot(shape, k, metric):
    ix, ox, xq, rows, _ = contents(shape, metric)
    e0, rs0 = ix.error_count(), ix.repair_stats()
    check(ix.search(xq, k), ox.search(xq, k), rows, "search")
    assert ix.error_count() == e0
    assert ix.repair_stats() == rs0
