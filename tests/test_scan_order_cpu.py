"""The preconditions of the key-order GPU tests (tests/test_gpu_scan_order.py and
tests/test_gpu_exact_scan_order.py), held on the CPU with NumPy, the oracle and the tests' own
references: for every (shape, metric, order) those tests use, the designated query's keys are
pairwise distinct in fp32 (and exact integers below 2^24 wherever the data is integer-valued),
the rows sorted by label have the promised order, every list has the size the GPU tests were
given (a recipe that yields too few distinct keys fails here), and the reference's top-k for
the designated query over one list is the expected id sequence -- the last k ids descending
for `improving`, the first k for `worsening`.  These are what make the GPU cases mean what
they claim."""
import numpy as np
import pytest

import indexflat_ref as RFLAT
import indexsq_ref as RSQ
import ivfflat_ref as RIVF
import ivfsq_ref as RIVFSQ
import scan_order as SO
from oracle import oracle as O

F = np.float32
METRICS = pytest.mark.parametrize("metric", [SO.L2, SO.IP])
ORDERS = pytest.mark.parametrize("order", SO.ORDERS)
K = 100


def assert_order(keys, ids, order, integer):
    """keys, ids of one list in position order."""
    keys = np.asarray(keys, np.float64)
    n = len(keys)
    assert len(ids) == n and (np.diff(ids) > 0).all()  # the label sort keeps the positions
    k32 = keys.astype(F)
    assert (k32.astype(np.float64) == keys).all()
    assert len(np.unique(k32)) == n
    if integer:
        assert (keys == np.round(keys)).all() and (np.abs(keys) < 2 ** 24).all()
    if order == "improving":
        assert (np.diff(keys) < 0).all()
    elif order == "worsening":
        assert (np.diff(keys) > 0).all()
    else:
        w = SO.wave0(n)
        assert (np.diff(keys[w]) < 0).all() and (np.diff(keys[~w]) > 0).all()
        if w.any() and (~w).any():
            assert keys[w].max() < keys[~w].min()


def assert_exact_in_fp32(xq, y, metric):
    """Every term and partial sum of any query's key over the rows y (float64) is an integer
    below 2^24, in whatever order they are added."""
    x = np.abs(xq.astype(np.float64))
    if metric == SO.IP:
        assert (x @ np.abs(y).T).max() < 2 ** 24
    else:  # also |x|^2 + |y|^2 and 2 <x, y>, the terms of the flat scan's expansion
        assert 2 * ((x.max() + np.abs(y)) ** 2).sum(1).max() < 2 ** 24
    assert (y == np.round(y)).all() and (xq == np.round(xq)).all()


def assert_topk(I, D, c, l, k, metric):
    """(D, I) of the designated query over list l alone."""
    ids, keys = c.list_ids[l], c.keys[l]
    kk = min(k, len(ids))
    if c.order == "improving":
        want = ids[::-1][:kk]
    elif c.order == "worsening":
        want = ids[:kk]
    else:
        w = SO.wave0(len(ids))
        want = np.concatenate([ids[w][::-1], ids[~w]])[:kk]
    np.testing.assert_array_equal(I[:kk], want)
    np.testing.assert_array_equal(SO.expected_ids(ids, c.order, k), want)
    best = np.sort(keys)[:kk]
    np.testing.assert_array_equal(-D[:kk] if metric == SO.IP else D[:kk], best.astype(F))
    assert (I[kk:] == -1).all()


# ---------------------------------------------------------------- IVF-PQ
PQ_GRID = [(s, 4, (0, 1, 2, 3)) for s in SO.PQ_SHAPES] + \
          [(s, 1032, (0, 1023, 1024, 1031)) for s in ("d32_m8", "d64_m16")]


@ORDERS
@METRICS
@pytest.mark.parametrize("shape,nlist,place", PQ_GRID, ids=[f"{s}_nlist{n}" for s, n, _ in PQ_GRID])
def test_ivfpq_contents(shape, nlist, place, metric, order):
    c = SO.pq_contents(shape, metric, order, nlist, place)
    assert c.sizes == (4700, 1537, 300, 0) and c.xq.shape == (13, c.d)
    assert (c.xq[:5] == c.q).all() and not (c.xq[5:] == c.q).all(1).any()
    assert np.unique(c.ids).size == c.ids.size
    np.testing.assert_array_equal(np.bincount(c.list_no, minlength=nlist)[list(place)], c.sizes)
    for l, n in enumerate(c.sizes):
        assert len(c.keys[l]) == n
        assert_order(c.keys[l], c.list_ids[l], order, integer=True)
    # the largest intermediate of any query: |x - y|^2 or |<x, y>| over the whole vector
    y = c.cb[np.arange(c.M)[None, :], c.codes].reshape(len(c.codes), c.d).astype(np.float64) + c.cent[c.list_no]
    assert_exact_in_fp32(c.xq, y, metric)
    ox = O.OracleIVFPQ(c.d, nlist, c.M, metric=SO.metric_id(metric))
    ox.set_trained(c.cent, c.cb)
    ox.add_preencoded(c.list_no, c.codes, c.ids)
    for l in (0, 1, 2):
        rows = SO.probe_rows(c, 1, [l])
        for k in (K, 1000):
            D, I = ox.search_preassigned(c.xq[:1], k, rows, SO.dis0(c, c.xq[:1], rows))
            assert_topk(I[0], D[0], c, l, k, metric)


# ---------------------------------------------------------------- the exact scans
def assert_exact_lists(c, integer):
    assert c.sizes == SO.SIZES and c.xq.shape == (13, SO.EXACT_D)
    assert (c.xq[:5] == c.q).all()
    for l, n in enumerate(c.sizes):
        assert len(c.keys[l]) == n
        assert_order(c.keys[l], c.list_ids[l], c.order, integer)
    if integer:
        assert_exact_in_fp32(c.xq, c.xb.astype(np.float64), c.metric)


@ORDERS
@METRICS
def test_ivfflat_contents(metric, order):
    c = SO.ivfflat_case(metric, order)
    assert_exact_lists(c, integer=True)
    ref = RIVF.Ref(c.xb, c.cent, SO.metric_id(metric), c.ids)
    np.testing.assert_array_equal(ref.list_of, c.list_of)
    for l in (0, 1, 2):
        np.testing.assert_array_equal(ref.lists()[l][0], c.list_ids[l])
        for k in (K, 1000):
            D, I = ref.search(c.xq[:1], k, Iq=np.array([[l]]))
            assert_topk(I[0], D[0], c, l, k, metric)


@ORDERS
@METRICS
@pytest.mark.parametrize("by_residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("qtype", [RSQ.QT_FP16, RSQ.QT_8BIT], ids=["fp16", "8bit"])
def test_ivfsq_contents(qtype, by_residual, metric, order):
    c = SO.ivfsq_case(qtype, by_residual, metric, order)
    assert_exact_lists(c, integer=qtype == RSQ.QT_FP16)
    ref = RIVFSQ.Ref(c.xb, c.cent, qtype, SO.metric_id(metric), by_residual, c.ids, c.trained)
    np.testing.assert_array_equal(ref.list_of, c.list_of)
    if qtype == RSQ.QT_8BIT:  # the point of the 8-bit cases: keys that are no integers
        assert (ref.dec != np.round(ref.dec)).any()
    for l in (0, 1, 2):
        Iq = np.array([[l]])
        Dq = (c.xq[:1].astype(np.float64) @ c.cent[l].astype(np.float64)).astype(F).reshape(1, 1)
        for k in (K, 1000):
            D, I = ref.search(c.xq[:1], k, Iq=Iq, Dq=Dq)
            assert_topk(I[0], D[0], c, l, k, metric)


@ORDERS
@METRICS
@pytest.mark.parametrize("nb", [4700, 4096 + 4700])
@pytest.mark.parametrize("qtype", [RSQ.QT_FP16, RSQ.QT_8BIT], ids=["fp16", "8bit"])
def test_indexsq_contents(qtype, nb, metric, order):
    c = SO.sq_case(qtype, nb, metric, order)
    assert c.sizes == (nb,) and len(c.xb) == nb
    c.list_ids[0] = np.arange(nb)  # labels are positions
    assert_order(c.keys[0], c.list_ids[0], order, integer=qtype == RSQ.QT_FP16)
    ref = RSQ.Ref(c.xb, qtype, SO.metric_id(metric), c.trained)
    for k in (K, 1000):
        D, I = ref.search(c.xq[:1], k)
        assert_topk(I[0], D[0], c, 0, k, metric)


@ORDERS
@METRICS
@pytest.mark.parametrize("nb,nq", [(4700, 13), (8796, 70)])
def test_indexflat_contents(nb, nq, metric, order):
    c = SO.flat_case(nb, nq, metric, order)
    assert len(c.xb) == nb and c.xq.shape == (nq, SO.EXACT_D) and (c.xq[:5] == c.q).all()
    c.list_ids[0] = np.arange(nb)
    assert_order(c.keys[0], c.list_ids[0], order, integer=True)
    assert_exact_in_fp32(c.xq, c.xb.astype(np.float64), metric)
    for k in (K, 1000):
        D, I = RFLAT.search(c.xq[:1], c.xb, k, SO.metric_id(metric))
        assert_topk(I[0], D[0], c, 0, k, metric)
