"""Shared reference of the IndexIVFFlat tests (tests/test_gpu_ivfflat.py, and the CPU
checks of this module in tests/test_ivfflat_cpu.py): Faiss's IndexIVFFlat::search in numpy
on the oracle's pieces.

* assignment = the oracle's coarse top-1, probes = its coarse top-nprobe;
* distances = ``tree_np`` (tests/indexpq_ref.py: the oracle's ``or_tree`` on whole arrays,
  bit for bit) of the query against every vector -- computed once per (queries, metric) and
  masked by the probed lists, so that one matrix serves every nprobe and k of a sweep;
* top-k = the k smallest (key, label), key = distance (L2) or -similarity (IP), padded with
  (FLT_MAX | -FLT_MAX, -1).
"""
import numpy as np

import faiss_amd as faiss
from indexpq_ref import KIND_IP, KIND_L2, tree_np
from oracle import oracle as O

IP, L2 = faiss.METRIC_INNER_PRODUCT, faiss.METRIC_L2
FMAX = np.finfo(np.float32).max
RANGE_ROWS = 4096  # kIvfFlatRangeRows of csrc/ivf_flat.h (tests/test_ivfflat_cpu.py checks it)


def assign(x, cent, metric):
    """The list of every vector: the coarse quantizer's top-1."""
    return O.coarse_search(x, cent, 1, metric=metric)[1][:, 0]


def probes(xq, cent, nprobe, metric):
    return O.coarse_search(xq, cent, nprobe, metric=metric)[1]


class Ref:
    """An IVF-Flat index over xb (labels ids, default 0..nb-1) with centroids cent."""

    def __init__(self, xb, cent, metric, ids=None):
        self.xb = np.ascontiguousarray(xb, np.float32)
        self.cent = np.ascontiguousarray(cent, np.float32)
        self.metric = metric
        self.ids = np.arange(len(self.xb), dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
        self.list_of = assign(self.xb, self.cent, metric) if len(self.xb) else np.zeros(0, np.int64)
        self._dist = {}

    def lists(self):
        """Per list (ids ascending, the vectors in that order): the device image."""
        out = []
        for l in range(len(self.cent)):
            sel = np.nonzero(self.list_of == l)[0]
            sel = sel[np.argsort(self.ids[sel], kind="stable")]
            out.append((self.ids[sel], self.xb[sel]))
        return out

    def dist(self, xq):
        """[nq][nb] fvec_L2sqr / fvec_inner_product of every query with every vector."""
        xq = np.ascontiguousarray(xq, np.float32)
        key = xq.tobytes()
        if key not in self._dist:
            kind = KIND_IP if self.metric == IP else KIND_L2
            # in blocks of vectors, so that the [nq][rows][d] products stay small
            step = max(1, (1 << 22) // max(1, xq.shape[0] * xq.shape[1]))
            self._dist[key] = np.concatenate(
                [tree_np(xq[:, None, :], self.xb[None, i:i + step], kind) for i in range(0, len(self.xb), step)] or
                [np.zeros((xq.shape[0], 0), np.float32)], axis=1)
        return self._dist[key]

    def dist64(self, xq):
        x = np.asarray(xq, np.float64)
        y = self.xb.astype(np.float64)
        if self.metric == IP:
            return x @ y.T
        return ((x[:, None, :] - y[None]) ** 2).sum(2)

    def search(self, xq, k, nprobe=None, Iq=None):
        """(D, I) of search (nprobe) or search_preassigned (Iq: -1 skips, repeats count once)."""
        xq = np.ascontiguousarray(xq, np.float32)
        if Iq is None:
            Iq = probes(xq, self.cent, nprobe, self.metric)
        dis = self.dist(xq)
        nq = xq.shape[0]
        D = np.full((nq, k), -FMAX if self.metric == IP else FMAX, np.float32)
        I = np.full((nq, k), -1, np.int64)
        for q in range(nq):
            sel = np.nonzero(np.isin(self.list_of, Iq[q][Iq[q] >= 0]))[0]
            key = -dis[q, sel] if self.metric == IP else dis[q, sel]
            order = sel[np.lexsort((self.ids[sel], key))[:k]]
            D[q, :len(order)] = dis[q, order]
            I[q, :len(order)] = self.ids[order]
        return D, I
