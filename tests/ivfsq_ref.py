"""Shared reference of the IndexIVFScalarQuantizer tests (tests/test_gpu_ivfsq.py, and the CPU
checks of this module in tests/test_ivfsq_cpu.py): Faiss's IndexIVFScalarQuantizer in numpy, built
from the references of its two halves.

* assignment and probes = the oracle's coarse search (tests/ivfflat_ref.py ``assign``; probes and
  their coarse values from ``O.coarse_search``);
* per list: the base rows (minus the list's centroid when by_residual, one fp32 subtraction per
  component) -> codes -> decoded rows (tests/indexsq_ref.py ``train`` / ``encode`` / ``decode``);
  the quantizer is trained on those (residual) rows unless its table is given;
* per (query, probed list): ``tree_np`` (tests/indexpq_ref.py) of q (q - centroid for L2 with
  by_residual) against the list's decoded rows; for the inner product with by_residual the
  pair's coarse value is added, ``coarse + ip`` in float32 -- the oracle's ``coarse_search``
  value for ``search``, the caller's ``Dq`` (None: zeros) for ``search_preassigned``;
* a list repeated in a row of ``Iq`` is scanned once, with the coarse value of its first column;
  -1 skips a probe;
* top-k = the k smallest (key, label), key = distance (L2) or -similarity (IP), padded with
  (FLT_MAX | -FLT_MAX, -1).
"""
import numpy as np

import faiss_amd as faiss
import indexsq_ref as S
from indexpq_ref import KIND_IP, KIND_L2, tree_np
from ivfflat_ref import assign
from oracle import oracle as O

IP, L2 = faiss.METRIC_INNER_PRODUCT, faiss.METRIC_L2
FMAX = np.finfo(np.float32).max
F = np.float32
QT_8BIT, QT_8BIT_UNIFORM, QT_FP16 = S.QT_8BIT, S.QT_8BIT_UNIFORM, S.QT_FP16
SQ_TRAIN_ROWS, SQ_TRAIN_SEED = 100000, 1234  # the subsample of the quantizer's training


def residuals(x, cent, list_of):
    r = np.ascontiguousarray(x, F) - np.ascontiguousarray(cent, F)[list_of]
    assert r.dtype == F
    return r


def train_rows(n):
    """The rows the scalar quantizer trains on: all of them up to SQ_TRAIN_ROWS, else the first
    SQ_TRAIN_ROWS of the library's rand_perm(n, SQ_TRAIN_SEED)."""
    if n <= SQ_TRAIN_ROWS:
        return np.arange(n, dtype=np.int64)
    return O.rand_perm_prefix(n, SQ_TRAIN_ROWS, SQ_TRAIN_SEED)


def train_sq(x, cent, qtype, metric, by_residual):
    """sq.trained of Index.train(x) once the centroids are ``cent``."""
    x = np.ascontiguousarray(x, F)[train_rows(len(x))]
    if by_residual:
        x = residuals(x, cent, assign(x, cent, metric))
    return S.train(x, qtype)


class Ref:
    """An IVF scalar-quantizer index over xb (labels ids, default 0..nb-1) with centroids cent;
    trained: sq.trained (default: trained on xb's own rows or residuals)."""

    def __init__(self, xb, cent, qtype, metric, by_residual, ids=None, trained=None):
        self.xb = np.ascontiguousarray(xb, F)
        self.cent = np.ascontiguousarray(cent, F)
        self.qtype, self.metric, self.by_residual = qtype, metric, bool(by_residual)
        self.d = self.cent.shape[1]
        self.ids = np.arange(len(self.xb), dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
        self.list_of = assign(self.xb, self.cent, metric) if len(self.xb) else np.zeros(0, np.int64)
        base = residuals(self.xb, self.cent, self.list_of) if self.by_residual else self.xb
        self.trained = S.train(base, qtype) if trained is None else np.asarray(trained, F)
        self.codes = S.encode(base, qtype, self.trained)
        self.dec = S.decode(self.codes, qtype, self.trained, self.d)
        self.rows_of = [np.nonzero(self.list_of == l)[0] for l in range(len(self.cent))]

    def lists(self):
        """Per list (ids ascending, the codes in that order): the device image."""
        out = []
        for sel in self.rows_of:
            sel = sel[np.argsort(self.ids[sel], kind="stable")]
            out.append((self.ids[sel], self.codes[sel]))
        return out

    def pair(self, q, l, coarse):
        """Distances of query row q against the decoded rows of list l (coarse: the pair's value)."""
        y = self.dec[self.rows_of[l]]
        if self.metric == IP:
            dis = tree_np(q[None], y, KIND_IP)
            if self.by_residual:
                dis = F(coarse) + dis
                assert dis.dtype == F
            return dis
        qr = q - self.cent[l] if self.by_residual else q
        assert qr.dtype == F
        return tree_np(qr[None], y, KIND_L2)

    def search(self, xq, k, nprobe=None, Iq=None, Dq=None):
        """(D, I) of search (nprobe) or search_preassigned (Iq, Dq)."""
        xq = np.ascontiguousarray(xq, F)
        if Iq is None:
            Dq, Iq = O.coarse_search(xq, self.cent, nprobe, metric=self.metric)
        elif Dq is None:
            Dq = np.zeros(np.shape(Iq), F)
        Iq = np.asarray(Iq, np.int64)
        nq = xq.shape[0]
        D = np.full((nq, k), -FMAX if self.metric == IP else FMAX, F)
        I = np.full((nq, k), -1, np.int64)
        for q in range(nq):
            seen, dis, lab = set(), [np.zeros(0, F)], [np.zeros(0, np.int64)]
            for p, l in enumerate(Iq[q]):
                if l < 0 or l in seen:
                    continue
                seen.add(int(l))
                dis.append(self.pair(xq[q], int(l), Dq[q, p]))
                lab.append(self.ids[self.rows_of[l]])
            dis, lab = np.concatenate(dis), np.concatenate(lab)
            order = np.lexsort((lab, -dis if self.metric == IP else dis))[:k]
            D[q, :len(order)] = dis[order]
            I[q, :len(order)] = lab[order]
        return D, I

    def brute64(self, xq, k, nprobe):
        """The same search in float64 from the float32 decoded rows (and float32 coarse values):
        (keys [nq][<= k] ascending, labels)."""
        xq = np.ascontiguousarray(xq, F)
        Dq, Iq = O.coarse_search(xq, self.cent, nprobe, metric=self.metric)
        keys, labels = [], []
        for q in range(xq.shape[0]):
            sel = np.nonzero(np.isin(self.list_of, Iq[q]))[0]
            y, x = self.dec[sel].astype(np.float64), xq[q].astype(np.float64)
            c = self.cent[self.list_of[sel]].astype(np.float64)
            if self.metric == IP:
                col = {int(l): float(Dq[q, p]) for p, l in enumerate(Iq[q])}
                key = -(y @ x + (np.array([col[int(l)] for l in self.list_of[sel]]) if self.by_residual else 0.0))
            else:
                key = (((x - c if self.by_residual else x) - y) ** 2).sum(1)
            order = np.argsort(key, kind="stable")[:k]
            keys.append(key[order])
            labels.append(self.ids[sel][order])
        return keys, labels
