"""Shared reference of the IndexScalarQuantizer tests (tests/test_gpu_indexsq.py, and the CPU
checks of this module in tests/test_indexsq_cpu.py): Faiss's scalar quantizer restated in numpy.

The contract: Faiss's scalar-build formulas for encode and decode, every operation one fp32
rounding (numpy float32 arithmetic is exactly that), no fusion, and the project's distance
order (``tree_np`` of tests/indexpq_ref.py) over the decoded vector.

* train (RS_minmax, rangestat_arg = 0): vmin = min, vdiff = max - vmin, per dimension
  (QT_8bit: trained = [vmin (d), vdiff (d)]) or over all entries (QT_8bit_uniform:
  [vmin, vdiff]); QT_fp16 trains nothing (trained is empty);
* encode, 8-bit: xi = vdiff != 0 ? (x - vmin) / vdiff : 0, clamped to [0, 1],
  code = (uint8)(int)(255.f * xi); fp16: round to nearest even (``astype(float16)``);
* decode, 8-bit: vmin + (((float)code + 0.5f) / 255.0f) * vdiff; fp16: (float)half;
* distances = tree_np of the query against every decoded vector;
* top-k = the k smallest (key, label), key = distance (L2) or -similarity (IP), labels =
  positions, padded with (FLT_MAX | -FLT_MAX, -1).
"""
import numpy as np

import faiss_amd as faiss
from indexpq_ref import KIND_IP, KIND_L2, ref_order, ref_topk, tree_np

IP, L2 = faiss.METRIC_INNER_PRODUCT, faiss.METRIC_L2
FMAX = np.finfo(np.float32).max
QT_8BIT, QT_8BIT_UNIFORM, QT_FP16 = 0, 2, 4
RANGE_ROWS = 4096  # rows per range of the scan (kIvfFlatRangeRows of csrc/ivf_flat.h)
F = np.float32


def code_size(qtype, d):
    return 2 * d if qtype == QT_FP16 else d


def train(x, qtype):
    """sq.trained for the training set x."""
    x = np.ascontiguousarray(x, F)
    if qtype == QT_FP16:
        return np.zeros(0, F)
    if qtype == QT_8BIT_UNIFORM:
        vmin = x.min()
        return np.array([vmin, x.max() - vmin], F)
    vmin = x.min(0)
    return np.concatenate([vmin, x.max(0) - vmin]).astype(F)


def expand(trained, qtype, d):
    """(vmin [d], vdiff [d]) of an 8-bit quantizer."""
    t = np.asarray(trained, F)
    if qtype == QT_8BIT_UNIFORM:
        return np.full(d, t[0], F), np.full(d, t[1], F)
    return t[:d].copy(), t[d:].copy()


def encode(x, qtype, trained):
    """float32 [n][d] -> uint8 [n][code_size]."""
    x = np.ascontiguousarray(x, F)
    n, d = x.shape
    if qtype == QT_FP16:
        return x.astype(np.float16).view(np.uint8).reshape(n, 2 * d)
    vmin, vdiff = expand(trained, qtype, d)
    num = x - vmin
    assert num.dtype == F
    xi = np.divide(num, vdiff[None], out=np.zeros_like(num), where=(vdiff != 0)[None])
    xi = np.where(xi < 0, F(0), xi)
    xi = np.where(xi > 1, F(1), xi).astype(F)
    scaled = F(255) * xi
    assert scaled.dtype == F
    return scaled.astype(np.int32).astype(np.uint8)  # truncation


def decode(codes, qtype, trained, d):
    """uint8 [n][code_size] -> float32 [n][d]."""
    codes = np.ascontiguousarray(codes, np.uint8).reshape(-1, code_size(qtype, d))
    if qtype == QT_FP16:
        return codes.view(np.float16).astype(F)
    vmin, vdiff = expand(trained, qtype, d)
    unit = (codes.astype(F) + F(0.5)) / F(255)
    y = vmin[None] + unit * vdiff[None]
    assert y.dtype == F
    return y


class Ref:
    """A scalar-quantizer index over xb, trained on it (or with the given parameters)."""

    def __init__(self, xb, qtype, metric, trained=None):
        xb = np.ascontiguousarray(xb, F)
        self.qtype, self.metric, self.d = qtype, metric, xb.shape[1]
        self.trained = train(xb, qtype) if trained is None else np.asarray(trained, F)
        self.codes = encode(xb, qtype, self.trained)
        self.dec = decode(self.codes, qtype, self.trained, self.d)
        self._dist = {}

    def dist(self, xq):
        """[nq][nb] fvec_L2sqr / fvec_inner_product of every query with every decoded vector."""
        xq = np.ascontiguousarray(xq, F)
        key = xq.tobytes()
        if key not in self._dist:
            kind = KIND_IP if self.metric == IP else KIND_L2
            step = max(1, (1 << 22) // max(1, xq.shape[0] * xq.shape[1]))
            self._dist[key] = np.concatenate(
                [tree_np(xq[:, None, :], self.dec[None, i:i + step], kind) for i in range(0, len(self.dec), step)] or
                [np.zeros((xq.shape[0], 0), F)], axis=1)
        return self._dist[key]

    def dist64(self, xq):
        x = np.asarray(xq, np.float64)
        y = self.dec.astype(np.float64)
        if self.metric == IP:
            return x @ y.T
        return ((x[:, None, :] - y[None]) ** 2).sum(2)

    def search(self, xq, k):
        dis = self.dist(xq)
        return ref_topk(dis, k, self.metric, ref_order(dis, min(k, dis.shape[1]), self.metric))
