"""Shared reference of the IndexPQ path tests (tests/test_gpu_indexpq_paths.py, and the
CPU checks of this module in tests/test_indexpq_cpu.py): a numpy restatement of Faiss's
IndexPQ::search that is fast enough for thousands of queries, and the scan plan of the
library (``ivfpq_pq_debug_plan``), so that a test asserts the path it claims to reach.

``tree_np`` restates the oracle's ``or_tree`` (Faiss's AVX fvec reduction) on whole arrays:
every numpy float32 operation is one IEEE rounding, exactly as in the scalar loop, and the
order of the additions per output element is the same, so it equals ``O.tree`` bit for bit.
"""
import ctypes
from types import SimpleNamespace

import numpy as np

import faiss_amd as faiss
from faiss_amd import _lib
from oracle import oracle as O

IP, L2 = faiss.METRIC_INNER_PRODUCT, faiss.METRIC_L2
FMAX = np.finfo(np.float32).max
KIND_IP, KIND_L2 = 0, 1


def tree_np(x, y, kind):
    """or_tree over the last axis of float32 arrays x, y (broadcast against each other)."""
    x = np.asarray(x, np.float32)
    y = np.asarray(y, np.float32)
    if kind == KIND_IP:
        p = x * y
    else:
        t = x - y
        p = t * t
    assert p.dtype == np.float32
    d = p.shape[-1]
    a8 = np.zeros(p.shape[:-1] + (8,), np.float32)
    i = 0
    while i + 8 <= d:  # 8 accumulators
        a8 = a8 + p[..., i:i + 8]
        i += 8
    a4 = a8[..., 4:] + a8[..., :4]  # fold to 4
    if i + 4 <= d:  # the 4-wide step
        a4 = a4 + p[..., i:i + 4]
        i += 4
    if i < d:  # the masked tail
        a4 = a4.copy()
        a4[..., :d - i] = a4[..., :d - i] + p[..., i:]
    return (a4[..., 0] + a4[..., 1]) + (a4[..., 2] + a4[..., 3])


def ref_tables(xq, cb, metric):
    """[nq][M][256]: compute_inner_prod_table (the oracle's) or compute_distance_table."""
    if metric == IP:
        return O.ip_table(xq, cb)
    M, ksub, dsub = cb.shape
    tab = np.empty((xq.shape[0], M, ksub), np.float32)
    for m in range(M):
        tab[:, m, :] = tree_np(xq[:, None, m * dsub:(m + 1) * dsub], cb[m][None], KIND_L2)
    return tab


def ref_sums(tab, codes):
    """acc = 0; acc += tab[m][code[m]] in ascending m, float32 (pq_knn_search_with_tables)."""
    # row-major [row][query], so that a sub-quantizer's gather copies whole table rows
    tab_t = np.ascontiguousarray(tab.transpose(1, 2, 0))
    acc = np.zeros((codes.shape[0], tab.shape[0]), np.float32)
    for m in range(tab.shape[1]):
        acc += tab_t[m][codes[:, m]]
    return np.ascontiguousarray(acc.T)


def ref_order(acc, kmax, metric):
    """Per query the labels of the kmax best rows by (key, label); its first k columns are
    the order of every k <= kmax, so one sort serves all of a test's k."""
    key = -acc if metric == IP else acc
    return np.argsort(key, axis=1, kind="stable")[:, :kmax]


def ref_topk(acc, k, metric, order=None):
    nq, nb = acc.shape
    if order is None:
        order = ref_order(acc, k, metric)
    order = order[:, :k]
    D = np.full((nq, k), -FMAX if metric == IP else FMAX, np.float32)
    I = np.full((nq, k), -1, np.int64)
    D[:, :order.shape[1]] = np.take_along_axis(acc, order, 1)
    I[:, :order.shape[1]] = order
    return D, I


def ref_encode(x, cb):
    """The oracle's encoder against one all-zero centroid (x - 0 is exact)."""
    M, _, dsub = cb.shape
    ox = O.OracleIVFPQ(M * dsub, 1, M)
    ox.set_trained(np.zeros((1, M * dsub), np.float32), cb)
    return ox.encode(x)[1]


def sums64(xq, cb, codes, metric, absolute=False):
    """The same sums in float64 from the float32 inputs; absolute: of the absolute values of
    the d products (for L2 the squared differences, which are their own absolute values)."""
    M, _, dsub = cb.shape
    acc = np.zeros((xq.shape[0], codes.shape[0]), np.float64)
    for m in range(M):
        qm = xq[:, None, m * dsub:(m + 1) * dsub].astype(np.float64)
        c = cb[m].astype(np.float64)[None]
        if metric == IP:
            t = np.abs(qm * c).sum(2) if absolute else (qm * c).sum(2)
        else:
            t = ((qm - c) ** 2).sum(2)
        acc += t[:, codes[:, m]]
    return acc


def plan(M, k, nq, nb):
    """ivfpq_pq_debug_plan: how a search of nq queries over nb codes is split."""
    G, ranges, S = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rows, chunk = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(_lib.load().ivfpq_pq_debug_plan(M, k, nq, nb, ctypes.byref(G), ctypes.byref(ranges), ctypes.byref(rows),
                                               ctypes.byref(S), ctypes.byref(chunk)))
    return SimpleNamespace(G=G.value, ranges=ranges.value, rows=rows.value, S=S.value, chunk=chunk.value)


def pass_rows(k):
    """Rows a scan workgroup takes per pass over its range (256 threads x 8, or x 4 with queues)."""
    return 2048 if k <= 64 else 1024
