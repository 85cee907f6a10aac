"""The exact and scalar-quantizer scans (k_ivfflat_scan, k_ivfsq_scan, k_sq_scan, k_flat_scan)
under worst-case key order: the three orders of tests/scan_order.py -- `improving` (every row
is admitted), `worsening` (nothing after the first k), `one_wave` (the rows t0 + 0..63 of
every 256-row pass hold the best keys, so one wave keeps admitting under a bound the others
published; in k_flat_scan a wave keeps whole queries and sees every row of a pass, so there
the same rows alternate runs of 64 admitted rows with runs of rejected ones) -- for the
designated query, five copies of it and random queries beside them, each index against the
reference its own test file uses, bit for bit, for both metrics.

d = 36 is one staged step of 32 and the 4-wide remainder.  The IVF indexes hold the four lists
of 4700 (two row ranges), 1537, 300 and 0 rows, searched at nprobe = 4 (every list) and with
one preassigned probe (the 4700-row list alone); the flat ones 4700 and 4096 + 4700 rows, in
order as a whole.  k = 10 and 64 merge at once (R = 1); 100, 300 and 1000 are the three queued
classes.  The preconditions (distinct keys, the order, the references' answers) are held by
tests/test_scan_order_cpu.py.
"""
import numpy as np
import pytest

import faiss_amd as faiss
import indexflat_ref as RFLAT
import indexsq_ref as RSQ
import ivfflat_ref as RIVF
import ivfsq_ref as RIVFSQ
import scan_order as SO

pytestmark = pytest.mark.gpu

KS = (10, 64, 100, 300, 1000)
F = np.float32
METRICS = pytest.mark.parametrize("metric", [SO.L2, SO.IP])
ORDERS = pytest.mark.parametrize("order", SO.ORDERS)
QTYPES = pytest.mark.parametrize("qtype", [RSQ.QT_FP16, RSQ.QT_8BIT], ids=["fp16", "8bit"])


def check(got, want, msg):
    np.testing.assert_array_equal(got[1], want[1], err_msg=msg)
    np.testing.assert_array_equal(got[0], want[0], err_msg=msg)


def first_list(c):
    """One preassigned probe per query: the 4700-row list; and each query's <q, its centroid>."""
    Iq = np.zeros((len(c.xq), 1), np.int64)
    Dq = (c.xq.astype(np.float64) @ c.cent[0].astype(np.float64)).astype(F).reshape(-1, 1)
    return Iq, Dq


@ORDERS
@METRICS
def test_ivfflat(metric, order):
    c = SO.ivfflat_case(metric, order)
    m = SO.metric_id(metric)
    ix = faiss.IndexIVFFlat(None, SO.EXACT_D, len(c.cent), m)
    ix.set_trained(c.cent)
    ix.add_with_ids(c.xb, c.ids)
    np.testing.assert_array_equal(ix.invlists.list_sizes(), SO.SIZES)
    ref = RIVF.Ref(c.xb, c.cent, m, c.ids)
    Iq, _ = first_list(c)
    for k in KS:
        ix.nprobe = 4
        check(ix.search(c.xq, k), ref.search(c.xq, k, nprobe=4), f"nprobe=4 k={k}")
        ix.nprobe = 1
        want = ref.search(c.xq, k, Iq=Iq)
        np.testing.assert_array_equal(want[1][0], SO.expected_ids(c.list_ids[0], order, k))
        check(ix.search_preassigned(c.xq, k, Iq), want, f"preassigned nprobe=1 k={k}")


@ORDERS
@METRICS
@pytest.mark.parametrize("by_residual", [False, True], ids=["plain", "residual"])
@QTYPES
def test_ivfsq(qtype, by_residual, metric, order):
    c = SO.ivfsq_case(qtype, by_residual, metric, order)
    m = SO.metric_id(metric)
    ix = faiss.IndexIVFScalarQuantizer(None, SO.EXACT_D, len(c.cent), qtype, m, by_residual)
    ix.set_trained(c.cent, c.trained)
    ix.add_with_ids(c.xb, c.ids)
    np.testing.assert_array_equal(ix.invlists.list_sizes(), SO.SIZES)
    ref = RIVFSQ.Ref(c.xb, c.cent, qtype, m, by_residual, c.ids, c.trained)
    Iq, Dq = first_list(c)
    for k in KS:
        ix.nprobe = 4
        check(ix.search(c.xq, k), ref.search(c.xq, k, nprobe=4), f"nprobe=4 k={k}")
        ix.nprobe = 1
        want = ref.search(c.xq, k, Iq=Iq, Dq=Dq)
        np.testing.assert_array_equal(want[1][0], SO.expected_ids(c.list_ids[0], order, k))
        check(ix.search_preassigned(c.xq, k, Iq, Dq), want, f"preassigned nprobe=1 k={k}")


@ORDERS
@METRICS
@pytest.mark.parametrize("nb", [4700, 4096 + 4700])
@QTYPES
def test_indexsq(qtype, nb, metric, order):
    c = SO.sq_case(qtype, nb, metric, order)
    m = SO.metric_id(metric)
    ix = faiss.IndexScalarQuantizer(SO.EXACT_D, qtype, m)
    if qtype == RSQ.QT_8BIT:
        ix.set_trained(c.trained)
    ix.add(c.xb)
    ref = RSQ.Ref(c.xb, qtype, m, c.trained)
    for k in KS:
        want = ref.search(c.xq, k)
        np.testing.assert_array_equal(want[1][0], SO.expected_ids(np.arange(nb), order, k))
        check(ix.search(c.xq, k), want, f"k={k}")


@ORDERS
@METRICS
@pytest.mark.parametrize("nb,nq", [(4700, 13), (8796, 70)])  # the 16-query tile; the 64-query tile and a partial one
def test_indexflat(nb, nq, metric, order):
    c = SO.flat_case(nb, nq, metric, order)
    m = SO.metric_id(metric)
    ix = faiss.IndexFlat(SO.EXACT_D, m)
    ix.add(c.xb)
    for k in KS:
        want = RFLAT.search(c.xq, c.xb, k, m)
        np.testing.assert_array_equal(want[1][0], SO.expected_ids(np.arange(nb), order, k))
        check(ix.search(c.xq, k), want, f"k={k}")
