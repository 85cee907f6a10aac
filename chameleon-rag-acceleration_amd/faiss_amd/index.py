"""Faiss-compatible index classes backed by the gfx950 engine (libivfpq.so).

The surface mirrors what Chameleon's callers use on ``faiss`` (SURVEY.md
§8(b)):

* ``IndexIVFPQ(quantizer, d, nlist, M, nbits)`` with ``train / add /
  add_with_ids / search / search_preassigned / reset``, ``nprobe``,
  ``ntotal``, ``d``, ``is_trained``, ``quantizer``, ``pq.centroids``,
  ``invlists.{list_size,get_ids,get_codes,imbalance_factor}``,
  ``precomputed_table``, ``parallel_mode``
  (``bench_polysemous_1bn.py:272-291, 343-345, 368, 422, 430``;
  ``beir/beir/retrieval/search/dense/faiss_index.py:13-96``;
  ``ralm/retriever/faiss_retriever.py:18-275``;
  ``my_faiss_extract_scripts/extract_FPGA_required_data.py:174-248``);
* ``IndexPQ(d, M, nbits, metric)`` (beir ``faiss_search.py:168-224``
  PQFaissSearch, plain or behind ``IndexPreTransform(OPQMatrix, ...)``);
* ``IndexIVFFlat(quantizer, d, nlist, metric)`` (``bench_gpu_1bn.py:575-578``
  index keys ending in ``,Flat``; ``compute_ground_truth.py:311`` "IVF1,Flat");
* ``IndexScalarQuantizer(d, qtype, metric)`` and the ``ScalarQuantizer.QT_*`` constants
  (beir ``faiss_search.py:415-459`` SQFaissSearch: "QT_fp16"; "QT_8bit" by name);
* ``IndexBinaryFlat(d)`` with ``index_binary_factory``, ``write_index_binary`` and
  ``read_index_binary`` (beir ``faiss_search.py:134-166`` BinaryFaissSearch through
  ``faiss_index.py:98-174`` FaissBinaryIndex: Hamming candidates, then a float re-rank);
* ``IndexFlat(d, metric)``, ``IndexFlatL2``, ``IndexFlatIP`` (the coarse quantizer; standalone,
  exact search over device-resident rows: beir ``faiss_index.py:39-42``, ``faiss_search.py:337``;
  ``bench_gpu_1bn.py:444-455``; ``ralm/index_scanner/index_scanner.py:34-77``);
* ``index_factory``, ``ParameterSpace``, ``read_index / write_index``,
  ``swig_ptr``, ``vector_to_array``, ``get_num_gpus``.

Numpy conventions as Faiss: float32 C-contiguous in; ``D`` float32 and ``I``
int64 out; missing results are (FLT_MAX, -1).  Errors raise ``RuntimeError``
(Faiss's SWIG layer turns ``FaissException`` into ``RuntimeError`` too).
"""
from __future__ import annotations

import ctypes
import re

import numpy as np

from . import _lib, faiss_io
from ._handle import MAX_K, _default_device, _f32, _HandleIndex, _ids_ptr, _ListsView, _ptr  # noqa: F401

METRIC_INNER_PRODUCT = 0
METRIC_L2 = 1


def swig_ptr(a):
    """Faiss passes raw pointers to the 8-argument search_preassigned; here the
    array itself is passed through (faiss_retriever.py:217-223)."""
    return a


def vector_to_array(v):
    return np.asarray(v).copy()


def downcast_index(index):
    """faiss.downcast_index: Python objects already have their concrete type."""
    return index


def extract_index_ivf(index):
    """faiss.extract_index_ivf: the IndexIVFPQ inside an IndexPreTransform."""
    return getattr(index, "index", index)


def get_num_gpus():
    return int(_lib.load().ivfpq_device_count())


class IndexFlat(_HandleIndex):
    """Exact search over the raw vectors (faiss.IndexFlat(d, metric)): L2 returns the k
    smallest distances ascending, inner product the k largest descending, ties by label (the
    row position), missing results (FLT_MAX | -FLT_MAX, -1).

    Two roles share the class.  As an IVF quantizer it only holds the coarse centroids
    (``quantizer.xb``, extract_FPGA_required_data.py:174-184): ``add``, ``reset``, ``xb``,
    ``reconstruct``, ``reconstruct_n`` and ``ntotal`` work on a host buffer that grows
    geometrically and need neither a GPU nor the library.  Standalone (beir
    faiss_index.py:39-42 FlatIP, the IndexScanner coarse service of
    ralm/index_scanner/index_scanner.py:61-77, the ground truth of bench_gpu_1bn.py:444-455)
    the rows are resident in HBM: the device image is created at the first device use and
    extended from the rows not yet uploaded, ``add_device`` appends to it directly, and the
    host accessors fetch the rows the host has not seen.  ``search`` runs the fused
    matrix-core scan over the image (csrc/flat_scan.hip); its results are those of the
    stateless ``ivfpq_flat_search`` bit for bit."""

    _c = _lib.Family("ivfpq_flat_index_")
    _faiss_name = "IndexFlat"
    is_trained = True

    def __init__(self, d, metric=METRIC_L2, device=None):
        # (d >= 1 is checked where the device image is created: an IVF index validates its own d)
        if metric not in (METRIC_L2, METRIC_INNER_PRODUCT):
            raise RuntimeError(f"IndexFlat: unknown metric {metric}")
        _HandleIndex.__init__(self, d, metric, device)
        self._h = None
        self._buf = np.empty((0, max(self.d, 0)), np.float32)  # host rows [0, _nhost); _buf.shape[0] is the capacity
        self._nhost = 0   # rows the host buffer holds (a prefix of the index)
        self._ndev = 0    # rows the device image holds (a prefix of the index)
        self._ntotal = 0
        self._range_rows = 0

    @property
    def ntotal(self):
        return self._ntotal

    @property
    def capacity(self):
        """Rows the host buffer has room for (it doubles when full)."""
        return self._buf.shape[0]

    # -------------------------------------------------------------- host rows
    def _host_reserve(self, n):
        need = self._nhost + n
        if need <= self._buf.shape[0]:
            return
        buf = np.empty((max(need, 2 * self._buf.shape[0], 64), self.d), np.float32)
        buf[:self._nhost] = self._buf[:self._nhost]
        self._buf = buf

    def _sync_host(self):
        """Fetch the rows only the device image holds (after add_device)."""
        n = self._ntotal - self._nhost
        if n <= 0:
            return
        self._host_reserve(n)
        out = self._buf[self._nhost:self._ntotal]
        _lib.check(self._c.get_rows(self._h, self._nhost, n, _ptr(out)))
        self._nhost = self._ntotal

    def _handle(self):
        """Create the device image at its first use and upload the rows it lacks."""
        if self._h is None:
            self._create(self.device, self.d, self.metric_type)
            self._ndev = 0
            if self._range_rows:
                _lib.check(self._c.set_range_rows(self._h, self._range_rows))
        n = self._ntotal - self._ndev
        if n > 0:
            rows = self._buf[self._ndev:self._ntotal]
            _lib.check(self._c.add(self._h, n, _ptr(rows)))
            self._ndev = self._ntotal
        return self._h

    @property
    def xb(self):
        self._sync_host()
        return self._buf[:self._ntotal].reshape(-1)

    def add(self, x):
        x = _f32(x, self.d)
        self._sync_host()
        self._host_reserve(x.shape[0])
        self._buf[self._nhost:self._nhost + x.shape[0]] = x
        self._nhost += x.shape[0]
        self._ntotal = self._nhost

    def add_device(self, x, stream=None):
        """add with the vectors already in HBM (torch float32 CUDA tensor [n, d]): appended
        straight to the device image; returns once the rows are in place."""
        _HandleIndex.add_device(self, x, stream)
        self._ntotal += x.shape[0]
        self._ndev = self._ntotal

    def _faiss_bytes(self):
        return faiss_io.serialize_flat(self.d, self.metric_type, self.xb.reshape(-1, self.d))

    def reset(self):
        if self._h is not None:
            _lib.check(self._c.reset(self._h))
        self._buf = np.empty((0, self.d), np.float32)
        self._nhost = self._ndev = self._ntotal = 0

    def reconstruct(self, i):
        i = int(i)
        if not 0 <= i < self._ntotal:
            raise RuntimeError(f"reconstruct: {i} outside [0, {self._ntotal})")
        self._sync_host()
        return self._buf[i].copy()

    def reconstruct_n(self, i0, n):
        self._sync_host()
        return self._buf[i0:min(i0 + n, self._ntotal)].copy()

    def train(self, x):
        pass

    def set_range_rows(self, rows):
        """The base rows one scan workgroup takes (0 = chosen per search so that the grid
        fills the device).  Results do not depend on it; tests use it to cut small bases into
        several ranges (``flat_search_plan`` tells the split)."""
        rows = int(rows)
        if rows < 0:
            raise RuntimeError("negative range size")
        self._range_rows = rows
        if self._h is not None:
            _lib.check(self._c.set_range_rows(self._h, rows))

    def uploaded_rows(self):
        """Rows copied from the host into the device image since it was created (the image is
        extended, not rebuilt: every row counts once)."""
        if self._h is None:
            return 0
        out = ctypes.c_int64(0)
        _lib.check(self._c.get_stats(self._h, ctypes.byref(out), None, None))
        return out.value


def flat_search_plan(nq, nb, k, range_rows=0):
    """How an IndexFlat search of nq queries for k results over nb rows is split
    (ivfpq_flat_index_get_plan; host arithmetic, no device): dict of tile_q, range_rows,
    ranges, S, fan, rounds, query_chunk."""
    ints = {n: ctypes.c_int() for n in ("tile_q", "ranges", "S", "fan", "rounds")}
    rows, qc = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(_lib.load().ivfpq_flat_index_get_plan(int(nq), int(nb), int(k), int(range_rows),
                                                     ctypes.byref(ints["tile_q"]), ctypes.byref(rows),
                                                     ctypes.byref(ints["ranges"]), ctypes.byref(ints["S"]),
                                                     ctypes.byref(ints["fan"]), ctypes.byref(ints["rounds"]),
                                                     ctypes.byref(qc)))
    out = {n: v.value for n, v in ints.items()}
    out.update(range_rows=rows.value, query_chunk=qc.value)
    return out


# How the host cuts a batch into chunks ("Host-side splits"): each function returns
# what the library's own loop computes (host arithmetic, no device); the tests assert their cuts
# from these.
def _i64_from(name, *args):
    out = ctypes.c_int64()
    _lib.check(getattr(_lib.load(), name)(*[int(a) for a in args], ctypes.byref(out)))
    return out.value


def ivf_search_split(nq, nlist, k, nprobe, d, slots, entry_bytes=8, resid_queries=False):
    """An IndexIVFFlat / IndexIVFScalarQuantizer search of nq queries whose probed lists hold at
    most ``slots`` row ranges (ivfpq_ivf_get_plan, ivfpq_ivf_get_query_chunk): dict of S, fan,
    query_chunk.  entry_bytes is 12 and resid_queries true as the C header says."""
    S, fan = ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load().ivfpq_ivf_get_plan(int(k), int(slots), ctypes.byref(S), ctypes.byref(fan)))
    qc = _i64_from("ivfpq_ivf_get_query_chunk", nq, nlist, entry_bytes, S.value, k, nprobe, d, bool(resid_queries))
    return dict(S=S.value, fan=fan.value, query_chunk=qc)


def ivf_pass_rows(n, nlist, d, staged=False):
    """Rows per pass of an IVF add or scalar-quantizer training pass (ivfpq_ivf_get_pass_rows)."""
    return _i64_from("ivfpq_ivf_get_pass_rows", n, nlist, d, bool(staged))


def sq_search_plan(nq, nb, k):
    """An IndexScalarQuantizer search (ivfpq_sq_get_plan): dict of S, fan, query_chunk."""
    S, fan, qc = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    _lib.check(_lib.load().ivfpq_sq_get_plan(int(nq), int(nb), int(k), ctypes.byref(S), ctypes.byref(fan),
                                             ctypes.byref(qc)))
    return dict(S=S.value, fan=fan.value, query_chunk=qc.value)


def ivfpq_query_chunk(nq, nlist, M, nprobe, k, nbits=8, nloc=None):
    """Queries per chunk of an IndexIVFPQ search (ivfpq_get_query_chunk); nloc: the lists a
    list-range shard holds (default: all)."""
    return _i64_from("ivfpq_get_query_chunk", nq, nlist, M, nbits, nlist if nloc is None else nloc, nprobe, k)


def host_pass_rows(n, in_bytes):
    """Rows per pass of n host rows through a flat index's staging buffer (ivfpq_host_get_pass_rows)."""
    return _i64_from("ivfpq_host_get_pass_rows", n, in_bytes)


def flat_search_query_chunk(n, nb):
    """Queries per chunk of the stateless exact search (ivfpq_flat_search_get_query_chunk)."""
    return _i64_from("ivfpq_flat_search_get_query_chunk", n, nb)


def kmeans_assign_rows(n, k):
    """Rows per pass of a k-means assignment to k centroids (ivfpq_kmeans_get_assign_rows)."""
    return _i64_from("ivfpq_kmeans_get_assign_rows", n, k)


class IndexFlatL2(IndexFlat):
    """faiss.IndexFlatL2(d): IndexFlat with the L2 metric (the default coarse quantizer)."""

    metric_type = METRIC_L2

    def __init__(self, d, device=None):
        IndexFlat.__init__(self, d, type(self).metric_type, device)


class IndexFlatIP(IndexFlatL2):
    """Exact inner-product search (faiss.IndexFlatIP): the quantizer of an
    inner-product IndexIVFPQ and beir's flat IP index
    (beir/beir/retrieval/search/dense/faiss_search.py:14-131).  Results are the
    k largest inner products, descending."""

    metric_type = METRIC_INNER_PRODUCT


class _ProductQuantizer:
    """index.pq view: M, nbits, ksub, dsub and ``centroids`` (M*256*dsub floats,
    the layout of faiss pq.centroids)."""

    def __init__(self, owner):
        self._o = owner

    M = property(lambda self: self._o.M)
    nbits = property(lambda self: self._o.nbits)
    ksub = property(lambda self: 1 << self._o.nbits)
    dsub = property(lambda self: self._o.d // self._o.M)
    code_size = property(lambda self: self._o.M * self._o.nbits // 8)

    @property
    def centroids(self):
        return self._o.codebook().reshape(-1)

    def get_centroids(self, m, j):
        return self._o.codebook()[m, j].copy()


class _InvertedLists(_ListsView):
    """index.invlists of an IndexIVFPQ: the codes of a list are its rows' PQ codes, M bytes each."""

    def export(self):
        """All lists at once: (list_no int64 [ntotal], codes uint8 [ntotal][M], ids
        int64 [ntotal]) in list order (each list in its stored order), the input of
        add_preencoded -- one list-size query instead of one per list."""
        sizes = self.list_sizes()
        tot = int(sizes.sum())
        codes = np.empty((tot, self._o.M), np.uint8)
        ids = np.empty(tot, np.int64)
        off = np.concatenate([[0], np.cumsum(sizes)])
        for l in np.nonzero(sizes)[0]:
            _lib.check(self._o._c.get_list(self._o._h, int(l), _ptr(codes[off[l]:]), _ptr(ids[off[l]:])))
        return np.repeat(np.arange(self._o.nlist, dtype=np.int64), sizes), codes, ids


def overlap_built():
    """True: the batches-in-flight overlap is available (ivfpq_overlap_built; kept
    for callers of the r04 interface, where it was a build option)."""
    return bool(_lib.load().ivfpq_overlap_built())


def _pq_codebook(index):
    """codebook() of the two product-quantizer indexes: float32 [M][2^nbits][d/M], fetched once and kept
    until the next train / set_trained clears ``_codebook_cache``."""
    if index._codebook_cache is None:
        cb = np.empty((index.M, 1 << index.nbits, index.d // index.M), np.float32)
        _lib.check(index._c.get_codebook(index._h, _ptr(cb)))
        index._codebook_cache = cb
    return index._codebook_cache


class _IVFIndex(_HandleIndex):
    """What the three indexes over inverted lists share: the coarse quantizer, ``nprobe``, adds with
    labels and the searches of preassigned lists.  ``Dq`` is passed on where it is given; each class
    says whether its scan reads it."""

    def __init__(self, quantizer, d, nlist, metric, device):
        _HandleIndex.__init__(self, d, metric, device)
        self.nlist = int(nlist)
        if quantizer is None:
            quantizer = (IndexFlatIP if metric == METRIC_INNER_PRODUCT else IndexFlatL2)(d, self.device)
        self.quantizer = quantizer
        self.parallel_mode = 0  # accepted for faiss_retriever.py:71; queries are always independent
        self.niter_coarse = 25
        self.seed = 1234

    @property
    def nprobe(self):
        return int(self._c.get_nprobe(self._h))

    @nprobe.setter
    def nprobe(self, p):
        _lib.check(self._c.set_nprobe(self._h, int(p)))

    def centroids(self):
        c = np.empty((self.nlist, self.d), np.float32)
        _lib.check(self._c.get_centroids(self._h, _ptr(c)))
        return c

    def _sync_quantizer(self):
        if isinstance(self.quantizer, IndexFlatL2):  # IndexFlatIP too
            self.quantizer.reset()
            self.quantizer.add(self.centroids())

    def add(self, x):
        self.add_with_ids(x, None)

    def add_with_ids(self, x, ids):
        x = _f32(x, self.d)
        _lib.check(self._c.add(self._h, x.shape[0], _ptr(x), _ids_ptr(ids, x.shape[0], "x")))

    def _add_listed(self, fn, list_no, codes, ids):
        """Append codes uint8 [n][code_size] to the lists ``list_no`` [n] with labels ``ids`` (None: sequential)."""
        list_no = np.ascontiguousarray(list_no, np.int64).reshape(-1)
        codes = np.ascontiguousarray(codes, np.uint8).reshape(-1, self.code_size)
        n = list_no.shape[0]
        if codes.shape[0] != n:
            raise RuntimeError("codes and list_no have different lengths")
        _lib.check(fn(self._h, n, _ptr(list_no), _ptr(codes), _ids_ptr(ids, n, "list_no")))

    def add_device(self, x, ids=None, stream=None):
        """add / add_with_ids with the vectors already in HBM (torch float32 CUDA
        tensor [n, d]; ids: int64 CUDA tensor [n] or None for sequential ids).
        Assignment, encoding and the list-image merge run on the GPU; returns
        once the new image is in place."""
        import torch

        n = self._dev_rows(x)
        if ids is not None:
            self._check_dev(ids, "ids", torch.int64, (n,))
        _lib.check(self._c.add_device(self._h, n, x.data_ptr(), ids.data_ptr() if ids is not None else None,
                                      ctypes.c_void_p(self._stream(x, stream))))

    def search_preassigned(self, *args):
        """Either ``search_preassigned(x, k, Iq, Dq=None) -> (D, I)`` or the
        Faiss C++ form ``search_preassigned(n, x, k, Iq, Dq, D, I, store_pairs)``
        that fills D and I (faiss_retriever.py:217-223)."""
        if len(args) >= 7:
            n, x, k, Iq, Dq, D, I = args[:7]
            if len(args) > 7 and args[7]:
                raise RuntimeError("store_pairs is not supported")
            Dr, Ir = self._search_preassigned(x, k, Iq, Dq)
            np.copyto(np.asarray(D).reshape(Dr.shape), Dr)
            np.copyto(np.asarray(I).reshape(Ir.shape), Ir)
            return None
        x, k, Iq = args[:3]
        Dq = args[3] if len(args) > 3 else None
        return self._search_preassigned(x, k, Iq, Dq)

    def _search_preassigned(self, x, k, Iq, Dq=None):
        x = _f32(np.asarray(x).reshape(-1, self.d), self.d)
        self._check_k(k)
        n = x.shape[0]
        Iq = np.ascontiguousarray(Iq, np.int64).reshape(n, -1)
        if Iq.shape[1] != self.nprobe:
            raise RuntimeError(f"Iq must have nprobe={self.nprobe} columns, got {Iq.shape[1]}")
        if Dq is not None:
            Dq = _ptr(np.ascontiguousarray(Dq, np.float32).reshape(Iq.shape))
        D = np.empty((n, k), np.float32)
        I = np.empty((n, k), np.int64)
        _lib.check(self._c.search_preassigned(self._h, n, _ptr(x), int(k), _ptr(Iq), Dq, _ptr(D), _ptr(I)))
        return D, I

    def search_preassigned_device(self, x, k, Iq, Dq=None, D=None, I=None, stream=None):
        """search_preassigned with HBM-resident inputs."""
        return self._preassigned_device(self._c.search_preassigned_device, x, k, Iq, Dq, D, I, stream)

    def _preassigned_device(self, fn, x, k, Iq, Dq, D, I, stream, *token):
        import torch

        self._check_k(k)
        n = self._dev_rows(x)
        self._check_dev(Iq, "Iq", torch.int64, (n, self.nprobe))
        if Dq is not None:
            self._check_dev(Dq, "Dq", torch.float32, (n, self.nprobe))
        D, I = self._dev_outputs(x, k, D, I)
        _lib.check(fn(self._h, n, x.data_ptr(), int(k), Iq.data_ptr(), Dq.data_ptr() if Dq is not None else None,
                      D.data_ptr(), I.data_ptr(), *token, ctypes.c_void_p(self._stream(x, stream))))
        return D, I


class IndexIVFPQ(_IVFIndex):
    """faiss.IndexIVFPQ (by_residual; METRIC_L2 with precomputed tables, or
    METRIC_INNER_PRODUCT) on one MI355X.  Device searches of one index may be issued on
    different streams without synchronizing: the library orders each search after those still
    in flight on other streams, or, with ``inflight`` on, lets them overlap."""

    _c = _lib.Family("ivfpq_")
    _faiss_name = "IndexIVFPQ"
    by_residual = True
    use_precomputed_table = 1
    polysemous_ht = 0

    def __init__(self, quantizer, d, nlist, M, nbits=8, metric=METRIC_L2, device=None, _handle=None):
        _IVFIndex.__init__(self, quantizer, d, nlist, metric, device)
        self.M = int(M)
        self.nbits = int(nbits)
        self.niter_pq = 25
        if _handle is not None:
            self._h = _handle
        else:
            self._create(self.d, self.nlist, self.M, self.nbits, metric, self.device)
        self.pq = _ProductQuantizer(self)
        self.invlists = _InvertedLists(self)
        self._codebook_cache = None

    @property
    def code_size(self):
        return self.M

    def codebook(self):
        return _pq_codebook(self)

    @property
    def precomputed_table(self):
        t = np.empty((self.nlist, self.M, 1 << self.nbits), np.float32)
        _lib.check(self._c.get_precomputed_table(self._h, _ptr(t)))
        return t.reshape(-1)

    # ----------------------------------------------------------- build path
    def train(self, x):
        x = _f32(x, self.d)
        _lib.check(self._c.train(self._h, x.shape[0], _ptr(x), self.niter_coarse, self.niter_pq, self.seed))
        self._codebook_cache = None
        self._sync_quantizer()

    def set_trained(self, centroids, codebook):
        """Install trained quantizers (coarse centroids [nlist][d], PQ codebook [M][256][d/M])."""
        c = _f32(np.asarray(centroids).reshape(self.nlist, self.d), self.d, "centroids")
        cb = np.ascontiguousarray(codebook, np.float32).reshape(-1)
        if cb.size != self.M * (1 << self.nbits) * (self.d // self.M):
            raise RuntimeError("codebook has the wrong size")
        _lib.check(self._c.set_trained(self._h, _ptr(c), _ptr(cb)))
        self._codebook_cache = None
        self._sync_quantizer()

    def add_preencoded(self, list_no, codes, ids=None):
        self._add_listed(self._c.add_preencoded, list_no, codes, ids)

    def set_list_range(self, lo, hi):
        """Keep and scan only inverted lists [lo, hi) (list-range sharding)."""
        _lib.check(self._c.set_list_range(self._h, int(lo), int(hi)))

    def _faiss_bytes(self):
        inv = self.invlists
        lists = [(inv.get_ids(l), inv.get_codes(l).reshape(-1, self.code_size)) for l in range(self.nlist)]
        return faiss_io.serialize_ivfpq(self.d, self.nlist, self.nprobe, self.M, self.nbits, self.metric_type,
                                        self.centroids(), self.codebook(), lists)

    # ------------------------------------------------------------ search path
    def serve_request(self, msg, batch_size, dim, with_lists=False, nprobe=None, out=None):
        """One FaissServer request (RALM wire format, ``faiss_amd.wire``) in, the
        encoded answer out: decode + search (or search_preassigned) + encode in
        one native call (``ivfpq_serve_request``).  ``out``: optional writable
        buffer of at least ``answer_message_len(k, batch_size)`` bytes, filled
        in place; returns the answer as ``bytearray`` (or ``out``'s view)."""
        buf = np.frombuffer(msg, np.uint8)
        np_ = int(self.nprobe if nprobe is None else nprobe)
        if out is None:
            from .wire import peek_k

            k = peek_k(msg, with_lists)
            out = bytearray(max(1, batch_size * k * 12))
        ans = np.frombuffer(out, np.uint8)
        if not ans.flags.writeable:
            raise RuntimeError("answer buffer must be writable")
        ln = ctypes.c_int64(0)
        # a plain request is searched with the index's nprobe: an explicit nprobe
        # applies for this call only (with lists, it is the request's column count)
        saved = self.nprobe
        if not with_lists and nprobe is not None:
            self.nprobe = np_
        try:
            _lib.check(self._c.serve_request(self._h, _ptr(buf), buf.size, int(bool(with_lists)), int(batch_size),
                                             int(dim), np_, _ptr(ans), ans.size, ctypes.byref(ln)))
        finally:
            if self.nprobe != saved:
                self.nprobe = saved
        return out if len(out) == ln.value else memoryview(out)[:ln.value]

    # ------------------------------------------------------------ stage timing
    STAGES = ("coarse", "tables", "scan", "lists")

    def set_timing(self, on=True, lists_only=False):
        """Record HIP events around every stage (or, lists_only, around the list-scan kernel alone)."""
        _lib.check(self._c.set_timing(self._h, (2 if lists_only else 1) if on else 0))

    def get_timing(self):
        """{stage: (total_ms, launches)} since the last call (waits for the events)."""
        ms = (ctypes.c_double * len(self.STAGES))()
        cnt = (ctypes.c_int64 * len(self.STAGES))()
        _lib.check(self._c.get_timing(self._h, ms, cnt))
        return {s: (ms[i], cnt[i]) for i, s in enumerate(self.STAGES)}

    # ------------------------------------------------- device (torch) entry points
    @property
    def inflight(self):
        """Batches in flight: True lets device searches issued on different
        streams overlap (each stream keeps its own workspace, up to three);
        False (default, unless IVFPQ_INFLIGHT=1 at creation) orders each search
        after those still in flight on other streams.  Results are the same in
        both modes (tests/test_gpu_parity.py
        test_batches_in_flight_stress)."""
        return bool(self._c.get_inflight(self._h))

    @inflight.setter
    def inflight(self, on):
        _lib.check(self._c.set_inflight(self._h, int(bool(on))))

    def error_count(self):
        """Index-check violations counted by the merge kernels since creation
        (ivfpq_get_error_count; 0 on a correct run).  Waits for in-flight searches."""
        out = ctypes.c_int64(0)
        _lib.check(self._c.get_error_count(self._h, ctypes.byref(out)))
        return out.value

    def repair_stats(self):
        """(stale_reads, repairs) since creation: (query, merge launch) pairs that read a
        partial-list entry this batch's scan did not leave there, and the probes the merge
        rescanned because of one (ivfpq_get_repair_stats).  Waits for in-flight searches."""
        st, rp = ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(self._c.get_repair_stats(self._h, ctypes.byref(st), ctypes.byref(rp)))
        return st.value, rp.value

    def repair_log(self, max_events=192):
        """The first stale-entry events as dicts (ivfpq_get_repair_log)."""
        buf = (ctypes.c_uint32 * (8 * max_events))()
        n = ctypes.c_int(0)
        _lib.check(self._c.get_repair_log(self._h, buf, int(max_events), ctypes.byref(n)))
        out = []
        for e in range(n.value):
            w = buf[8 * e:8 * e + 8]
            out.append({"site": w[0] & 0xFF, "reader_xcd": (w[0] >> 8) & 0xF, "query": w[1], "list": w[2] & 0xFFFF,
                         "rank": w[2] >> 16, "expected_tag": w[3], "found_tag": w[4] & 0x0FFFFFFF,
                         "writer_xcd": w[4] >> 28, "found_key_bits": w[5], "epoch": w[6], "reread": w[7]})
        return out

    def set_fault_injection(self, every):
        """Test hook: later searches skip the partial-list stores of slots with
        slot % every == 1 (0 = off); results must stay exact (repairs)."""
        _lib.check(self._c.set_fault_injection(self._h, int(every)))

    def search_preassigned_device(self, x, k, Iq, Dq=None, D=None, I=None, stream=None, tables=None):
        """search_preassigned with HBM-resident inputs.  ``tables``: the token of a
        ``precompute_tables_device(x)`` call for exactly these queries, whose T3
        this search consumes instead of building its own."""
        if tables is None:
            return _IVFIndex.search_preassigned_device(self, x, k, Iq, Dq, D, I, stream)
        return self._preassigned_device(self._c.search_preassigned_tables_device, x, k, Iq, Dq, D, I, stream,
                                        ctypes.c_uint64(int(tables)))

    def precompute_tables_device(self, x, stream=None):
        """T3 of the queries x (torch CUDA [n, d]) on ``stream``; returns the token
        that ``search_preassigned_device(x, ..., tables=token)`` consumes.  The
        shard flow runs it on a side stream while the coarse step and the probe
        all-gather run.  Up to three tokens can be pending."""
        n = self._dev_rows(x)
        tok = ctypes.c_uint64(0)
        _lib.check(self._c.precompute_tables_device(self._h, n, x.data_ptr(), ctypes.c_void_p(self._stream(x, stream)),
                                                    ctypes.byref(tok)))
        return tok.value

    def _coarse_outputs(self, x, n, Iq, Dq):
        import torch

        p = min(self.nprobe, self.nlist)
        if Iq is None:
            Iq = torch.empty((n, p), dtype=torch.int64, device=x.device)
        if Dq is None:
            Dq = torch.empty((n, p), dtype=torch.float32, device=x.device)
        self._check_dev(Iq, "Iq", torch.int64, (n, p))
        self._check_dev(Dq, "Dq", torch.float32, (n, p))
        return Iq, Dq

    def coarse_device(self, x, Iq=None, Dq=None, stream=None):
        """The coarse quantizer alone: (Dq, Iq) [n, min(nprobe, nlist)] -- L2
        distances ascending or inner products descending."""
        n = self._dev_rows(x)
        Iq, Dq = self._coarse_outputs(x, n, Iq, Dq)
        _lib.check(self._c.coarse_device(self._h, n, x.data_ptr(), Iq.data_ptr(), Dq.data_ptr(),
                                         ctypes.c_void_p(self._stream(x, stream))))
        return Dq, Iq

    def coarse_tables_device(self, x, x_tables, Iq=None, Dq=None, stream=None):
        """The list-range shard step's front half on one stream: the coarse quantizer
        of this rank's queries ``x`` and T3 of the global batch ``x_tables`` (one
        launch at nlist < 8192).  Returns (Dq, Iq, token); the token goes to
        ``search_preassigned_device(x_tables, ..., tables=token)``."""
        n = self._dev_rows(x)
        nt = self._dev_rows(x_tables, "x_tables")
        Iq, Dq = self._coarse_outputs(x, n, Iq, Dq)
        tok = ctypes.c_uint64(0)
        _lib.check(self._c.coarse_tables_device(self._h, n, x.data_ptr(), Iq.data_ptr(), Dq.data_ptr(), nt,
                                                x_tables.data_ptr(), ctypes.c_void_p(self._stream(x, stream)),
                                                ctypes.byref(tok)))
        return Dq, Iq, tok.value


class IndexPQ(_HandleIndex):
    """faiss.IndexPQ: one product quantizer over the raw vectors, every code
    scanned for every query (beir faiss_search.py:168-224, nbits_experiments_fix_m.py:89).
    Labels are positions: there is no id map, as in Faiss."""

    _c = _lib.Family("ivfpq_pq_")
    _faiss_name = "IndexPQ"
    polysemous_ht = 0

    def __init__(self, d, M, nbits=8, metric=METRIC_L2, device=None):
        _HandleIndex.__init__(self, d, metric, device)
        self.M = int(M)
        self.nbits = int(nbits)
        self.niter_pq = 25
        self.seed = 1234
        self._create(self.d, self.M, self.nbits, metric, self.device)
        self.pq = _ProductQuantizer(self)
        self._codebook_cache = None

    @property
    def code_size(self):
        return self.M

    def codebook(self):
        return _pq_codebook(self)

    @property
    def codes(self):
        """uint8 [ntotal * M] (faiss.vector_to_array(index.codes))."""
        return self._codes(0, self.ntotal).reshape(-1)

    # ----------------------------------------------------------- build path
    def train(self, x):
        x = _f32(x, self.d)
        _lib.check(self._c.train(self._h, x.shape[0], _ptr(x), self.niter_pq, self.seed))
        self._codebook_cache = None

    def set_trained(self, codebook):
        """Install a trained codebook [M][256][d/M]."""
        cb = np.ascontiguousarray(codebook, np.float32).reshape(-1)
        if cb.size != self.M * (1 << self.nbits) * (self.d // self.M):
            raise RuntimeError("codebook has the wrong size")
        _lib.check(self._c.set_trained(self._h, _ptr(cb)))
        self._codebook_cache = None

    def add_codes(self, codes):
        """Append precomputed codes uint8 [n][M]."""
        codes = np.ascontiguousarray(codes, np.uint8).reshape(-1, self.M)
        _lib.check(self._c.add_codes(self._h, codes.shape[0], _ptr(codes)))

    def reconstruct_n(self, i0, n):
        """Decoded on the host from the codebook and the codes."""
        return decode_pq(self.codebook(), self._codes(i0, n))

    def reconstruct(self, i):
        return self.reconstruct_n(i, 1)[0]

    def _faiss_bytes(self):
        return faiss_io.serialize_pq(self.d, self.M, self.nbits, self.metric_type, self.codebook(),
                                     self._codes(0, self.ntotal))


class _FlatInvertedLists(_ListsView):
    """index.invlists of an IndexIVFFlat: the codes of a list are its vectors' bytes,
    ``code_size = 4 * d``."""

    _row = np.float32

    def get_vectors(self, l):
        """The list's vectors float32 [size][d], label-sorted."""
        return self._get(l)[0]


class IndexIVFFlat(_IVFIndex):
    """faiss.IndexIVFFlat: IVF over the raw fp32 vectors with exact distances
    (``bench_gpu_1bn.py:575-578`` index keys ending in ``,Flat``; the ``IVF1,Flat``
    ground truth of ``compute_ground_truth.py:311``).  The coarse quantizer is the
    IndexIVFPQ one; the lists live in HBM only.  ``search_preassigned`` accepts ``Dq``
    and ignores it: the scan computes whole distances."""

    _c = _lib.Family("ivfpq_ivfflat_")
    _faiss_name = "IndexIVFFlat"

    def __init__(self, quantizer, d, nlist, metric=METRIC_L2, device=None):
        _IVFIndex.__init__(self, quantizer, d, nlist, metric, device)
        self._create(self.d, self.nlist, metric, self.device)
        self.invlists = _FlatInvertedLists(self)

    @property
    def code_size(self):
        return 4 * self.d

    def train(self, x):
        x = _f32(x, self.d)
        _lib.check(self._c.train(self._h, x.shape[0], _ptr(x), self.niter_coarse, self.seed))
        self._sync_quantizer()

    def set_trained(self, centroids):
        """Install trained coarse centroids [nlist][d]."""
        c = _f32(np.asarray(centroids).reshape(self.nlist, self.d), self.d, "centroids")
        _lib.check(self._c.set_trained(self._h, _ptr(c)))
        self._sync_quantizer()

    def _faiss_bytes(self):
        inv = self.invlists
        lists = [(inv.get_ids(l), inv.get_vectors(l)) for l in range(self.nlist)]
        return faiss_io.serialize_ivfflat(self.d, self.nlist, self.nprobe, self.metric_type, self.centroids(), lists)


class ScalarQuantizer:
    """faiss.ScalarQuantizer: the QuantizerType values (beir faiss_search.py:423 looks the
    type up by name with getattr), and the ``index.sq`` view of an IndexScalarQuantizer."""

    QT_8bit = 0
    QT_4bit = 1
    QT_8bit_uniform = 2
    QT_4bit_uniform = 3
    QT_fp16 = 4
    QT_8bit_direct = 5
    QT_6bit = 6

    def __init__(self, owner):
        self._owner = owner
        self.qtype = owner.qtype
        self.d = owner.d
        self.code_size = owner.code_size

    @property
    def trained(self):
        """float32: [vmin (d), vdiff (d)] (QT_8bit), [vmin, vdiff] (QT_8bit_uniform), empty (QT_fp16);
        read from the owner's family: one call for the length, one for the values."""
        ix = self._owner
        if not ix.is_trained:
            return np.zeros(0, np.float32)
        n = ctypes.c_int64()
        _lib.check(ix._c.get_trained(ix._h, None, ctypes.byref(n)))
        out = np.empty(n.value, np.float32)
        if n.value:
            _lib.check(ix._c.get_trained(ix._h, _ptr(out), None))
        return out


_SQ_NAMES = {v: n for n, v in vars(ScalarQuantizer).items() if n.startswith("QT_")}


class IndexScalarQuantizer(_HandleIndex):
    """faiss.IndexScalarQuantizer(d, qtype, metric) for QT_fp16, QT_8bit and QT_8bit_uniform
    (beir faiss_search.py:415-459 SQFaissSearch): every code is decoded and compared with
    every query in one fused scan.  Labels are positions: there is no id map, as in Faiss."""

    _c = _lib.Family("ivfpq_sq_")
    _faiss_name = "IndexScalarQuantizer"

    def __init__(self, d, qtype, metric=METRIC_L2, device=None):
        _HandleIndex.__init__(self, d, metric, device)
        self.qtype = int(qtype)
        self._create(self.d, self.qtype, metric, self.device)
        cs = ctypes.c_int()
        _lib.check(self._c.get_dims(self._h, None, None, None, ctypes.byref(cs)))
        self.code_size = cs.value
        self.sq = ScalarQuantizer(self)

    def sa_code_size(self):
        return self.code_size

    @property
    def codes(self):
        """uint8 [ntotal * code_size] (faiss.vector_to_array(index.codes))."""
        return self._codes(0, self.ntotal).reshape(-1)

    def _code_rows(self, codes):
        codes = np.ascontiguousarray(codes, np.uint8)
        if codes.size % self.code_size:
            raise RuntimeError(f"codes must hold whole rows of {self.code_size} bytes")
        return codes.reshape(-1, self.code_size)

    # ----------------------------------------------------------- build path
    def train(self, x):
        x = _f32(x, self.d)
        _lib.check(self._c.train(self._h, x.shape[0], _ptr(x)))

    def set_trained(self, trained):
        """Install ``sq.trained`` (see ScalarQuantizer.trained)."""
        t = np.ascontiguousarray(trained, np.float32).reshape(-1)
        _lib.check(self._c.set_trained(self._h, _ptr(t), t.size))

    def add_codes(self, codes):
        """Append precomputed codes uint8 [n][code_size]."""
        codes = self._code_rows(codes)
        _lib.check(self._c.add_codes(self._h, codes.shape[0], _ptr(codes)))

    def sa_encode(self, x):
        """float32 [n][d] -> uint8 [n][code_size], encoded on the GPU."""
        x = _f32(x, self.d)
        out = np.empty((x.shape[0], self.code_size), np.uint8)
        _lib.check(self._c.encode(self._h, x.shape[0], _ptr(x), _ptr(out)))
        return out

    def sa_decode(self, codes):
        """uint8 [n][code_size] -> float32 [n][d], decoded on the GPU."""
        codes = self._code_rows(codes)
        out = np.empty((codes.shape[0], self.d), np.float32)
        _lib.check(self._c.decode(self._h, codes.shape[0], _ptr(codes), _ptr(out)))
        return out

    def reconstruct_n(self, i0, n):
        return self.sa_decode(self._codes(i0, n))

    def reconstruct(self, i):
        return self.reconstruct_n(i, 1)[0]

    def _faiss_bytes(self):
        return faiss_io.serialize_sq(self.d, self.qtype, self.metric_type, self.sq.trained,
                                     self._codes(0, self.ntotal))


class _CodeInvertedLists(_ListsView):
    """index.invlists of an IndexIVFScalarQuantizer: the codes of a list are its rows'
    scalar-quantizer codes, ``code_size`` bytes each."""


class IndexIVFScalarQuantizer(IndexIVFFlat):
    """faiss.IndexIVFScalarQuantizer(quantizer, d, nlist, qtype, metric, by_residual) for QT_fp16,
    QT_8bit and QT_8bit_uniform (the ``IVF<nlist>,SQ8`` / ``IVF<nlist>,SQfp16`` factory keys): an
    IndexIVFFlat whose lists hold IndexScalarQuantizer's codes, of the vector or (``by_residual``,
    the default) of the vector minus its list's centroid, decoded inside the scan.  With QT_fp16
    and ``by_residual=False`` it is what ``co.useFloat16 = True`` makes of an ``IVF..,Flat`` key in
    ``bench_gpu_1bn.py``.  Every method of IndexIVFFlat; ``search_preassigned`` reads ``Dq`` for the
    inner product with ``by_residual`` (None: zeros) and ignores it otherwise."""

    _c = _lib.Family("ivfpq_ivfsq_")
    _faiss_name = "IndexIVFScalarQuantizer"

    def __init__(self, quantizer, d, nlist, qtype, metric=METRIC_L2, by_residual=True, device=None):
        _IVFIndex.__init__(self, quantizer, d, nlist, metric, device)
        self.qtype = int(qtype)
        self.by_residual = bool(by_residual)
        self._create(self.d, self.nlist, self.qtype, metric, int(self.by_residual), self.device)
        cs = ctypes.c_int()
        _lib.check(self._c.get_dims(self._h, None, None, None, None, None, ctypes.byref(cs)))
        self._code_size = cs.value
        self.sq = ScalarQuantizer(self)
        self.invlists = _CodeInvertedLists(self)

    @property
    def code_size(self):
        return self._code_size

    def set_trained(self, centroids, sq_trained=()):
        """Install trained coarse centroids [nlist][d] and ``sq.trained`` (see ScalarQuantizer.trained)."""
        c = _f32(np.asarray(centroids).reshape(self.nlist, self.d), self.d, "centroids")
        t = np.ascontiguousarray(sq_trained, np.float32).reshape(-1)
        _lib.check(self._c.set_trained(self._h, _ptr(c), _ptr(t), t.size))
        self._sync_quantizer()

    def add_codes(self, list_no, codes, ids=None):
        """Append precomputed codes uint8 [n][code_size] to the lists ``list_no`` [n] with labels
        ``ids`` (None: sequential), as read from an index file."""
        self._add_listed(self._c.add_codes, list_no, codes, ids)

    def _faiss_bytes(self):
        lists = [self.invlists._get(l)[::-1] for l in range(self.nlist)]
        return faiss_io.serialize_ivfsq(self.d, self.nlist, self.nprobe, self.qtype, self.metric_type,
                                        self.by_residual, self.centroids(), self.sq.trained, lists)


class IndexBinaryFlat(_HandleIndex):
    """faiss.IndexBinaryFlat(d): exact Hamming search over uint8 codes of ``d`` bits (beir
    faiss_search.py BinaryFaissSearch builds ``IndexBinaryFlat(dim * 8)``).  ``search`` returns
    ``D`` int32 and ``I`` int64: per query the k smallest (hamming, label) pairs ascending, ties
    by label, padded with (2147483647, -1).  The distances equal Faiss's for either value of
    ``use_heap``; the labels equal ``use_heap = False`` (hammings_knn_mc, first-seen ids per
    distance), while Faiss's default heap path may keep other ties at the k-th distance and
    orders equal distances arbitrarily.  Labels are positions: there is no id map.  Queries and
    rows are uint8 [n, code_size], on the host and in HBM (``search_device``, ``add_device``)."""

    _c = _lib.Family("ivfpq_bin_")
    _dist = "int32"
    is_trained = True

    def __init__(self, d, device=None):
        _HandleIndex.__init__(self, d, METRIC_L2, device)  # the metric as Faiss's IndexBinary
        self.use_heap = True          # accepted, no effect: see the class comment
        self.query_batch_size = 32    # accepted, no effect
        self._create(self.d, self.device)
        self.code_size = self.d // 8

    def _host_rows(self, x):
        a = np.ascontiguousarray(x)
        if a.dtype != np.uint8 or a.ndim != 2 or a.shape[1] != self.code_size:
            raise RuntimeError(f"x must be a uint8 matrix with {self.code_size} columns, got {a.dtype} {a.shape}")
        return a

    def _dev_row(self):
        import torch

        return torch.uint8, self.code_size

    @property
    def xb(self):
        """uint8 [ntotal * code_size] (faiss.vector_to_array(index.xb))."""
        return self._codes(0, self.ntotal).reshape(-1)

    def train(self, x):
        pass

    def reconstruct_n(self, i0, n):
        return self._codes(i0, n)

    def reconstruct(self, i):
        return self._codes(i, 1)[0]


def decode_pq(codebook, codes):
    """ProductQuantizer::decode: codebook [M][256][dsub], codes uint8 [n][M] -> float32 [n][M * dsub]."""
    M, _, dsub = codebook.shape
    codes = np.asarray(codes, np.uint8).reshape(-1, M)
    out = np.empty((codes.shape[0], M * dsub), np.float32)
    for m in range(M):
        out[:, m * dsub:(m + 1) * dsub] = codebook[m][codes[:, m]]
    return out


def merge_topk_device(Ds, Is, metric=METRIC_L2, stream=None):
    """Merge S sorted partial results (torch [S, n, k]) into [n, k] on the GPU:
    ascending L2 distances, or descending inner products (metric)."""
    import torch

    if Ds.dim() != 3 or Is.shape != Ds.shape or Ds.dtype != torch.float32 or Is.dtype != torch.int64:
        raise RuntimeError("merge_topk_device: Ds float32 [S, n, k] and Is int64 of the same shape")
    if not (Ds.is_cuda and Is.is_cuda and Ds.device == Is.device):
        raise RuntimeError("merge_topk_device: inputs must be on one CUDA device")
    Ds, Is = Ds.contiguous(), Is.contiguous()
    S, n, k = Ds.shape
    D = torch.empty((n, k), dtype=torch.float32, device=Ds.device)
    I = torch.empty((n, k), dtype=torch.int64, device=Ds.device)
    s = stream if stream is not None else torch.cuda.current_stream(Ds.device).cuda_stream
    _lib.check(_lib.load().ivfpq_merge_topk_device(S, n, k, int(metric), Ds.data_ptr(), Is.data_ptr(),
                                                   D.data_ptr(), I.data_ptr(), ctypes.c_void_p(s)))
    return D, I


# ------------------------------------------------------------------ factory / IO

_PQ_FACTORY_RE = re.compile(r"^(?:OPQ(\d+)(?:_(\d+))?,)?PQ(\d+)(?:x(\d+))?$")
_FACTORY_RE = re.compile(r"^(?:OPQ(\d+)(?:_(\d+))?,)?IVF(\d+),PQ(\d+)(?:x(\d+))?$")
_IVFFLAT_FACTORY_RE = re.compile(r"^IVF(\d+),Flat$")
_SQ_FACTORY_RE = re.compile(r"^SQ(\w+)$")
_SQ_FACTORY_TYPES = {"8": ScalarQuantizer.QT_8bit, "fp16": ScalarQuantizer.QT_fp16}
_IVFSQ_FACTORY_RE = re.compile(r"^IVF(\d+),SQ(\w+)$")
_PCA_FRONT_RE = re.compile(r"^PCA(W?)(R?)(\d+),(.+)$")


def parse_factory(key):
    """'[OPQ<M>[_<dout>],]IVF<nlist>,PQ<M>[x8]' -> (nlist, M, nbits) or, with an
    OPQ front, (nlist, M, nbits, opq_M, opq_dout) (opq_dout = -1: d)."""
    m = _FACTORY_RE.match(key.replace(" ", ""))
    if not m:
        raise RuntimeError(f"index_factory: unsupported key {key!r} "
                           "(supported: '[OPQ<M>[_<dout>],]IVF<nlist>,PQ<M>[x8]', '[OPQ<M>[_<dout>],]PQ<M>[x8]', "
                           "'IVF<nlist>,Flat', 'IVF<nlist>,SQ8', 'IVF<nlist>,SQfp16', 'SQ8', 'SQfp16', 'Flat', each also behind a 'PCA[W][R]<dout>,' front)")
    nbits = int(m.group(5)) if m.group(5) else 8
    base = (int(m.group(3)), int(m.group(4)), nbits)
    if m.group(1) is None:
        return base
    return base + (int(m.group(1)), int(m.group(2)) if m.group(2) else -1)


def parse_pq_factory(key):
    """'[OPQ<M>[_<dout>],]PQ<M>[x8]' -> (M, nbits) or (M, nbits, opq_M, opq_dout)
    (opq_dout = -1: d); None for any other key."""
    m = _PQ_FACTORY_RE.match(key.replace(" ", ""))
    if not m:
        return None
    base = (int(m.group(3)), int(m.group(4)) if m.group(4) else 8)
    if m.group(1) is None:
        return base
    return base + (int(m.group(1)), int(m.group(2)) if m.group(2) else -1)


def parse_pca_front(key):
    """'PCA[W][R]<dout>,<rest>' -> (dout, eigen_power, random_rotation, rest): W whitens
    (eigen_power = -0.5), R adds the random rotation; None for a key that does not start with
    'PCA'; any other 'PCA...' front raises, naming the key."""
    key = key.replace(" ", "")
    if not key.startswith("PCA"):
        return None
    m = _PCA_FRONT_RE.match(key)
    if not m:
        raise RuntimeError(f"index_factory: unsupported key {key!r} (a PCA front is 'PCA<dout>,', 'PCAR<dout>,', "
                           "'PCAW<dout>,' or 'PCAWR<dout>,' before a supported key)")
    return int(m.group(3)), -0.5 if m.group(1) else 0.0, bool(m.group(2)), m.group(4)


def parse_ivfflat_factory(key):
    """'IVF<nlist>,Flat' -> nlist; None for any other key."""
    m = _IVFFLAT_FACTORY_RE.match(key.replace(" ", ""))
    return int(m.group(1)) if m else None


def parse_sq_factory(key):
    """'SQ8' / 'SQfp16' -> the quantizer type; None for a key that does not start a scalar
    quantizer; any other 'SQ<x>' (Faiss also has SQ4 and SQ6) raises, naming the key."""
    m = _SQ_FACTORY_RE.match(key.replace(" ", ""))
    if not m:
        return None
    if m.group(1) not in _SQ_FACTORY_TYPES:
        raise RuntimeError(f"index_factory: unsupported scalar quantizer key {key!r} (supported: 'SQ8', 'SQfp16')")
    return _SQ_FACTORY_TYPES[m.group(1)]


def parse_ivfsq_factory(key):
    """'IVF<nlist>,SQ8' / 'IVF<nlist>,SQfp16' -> (nlist, quantizer type); None for any other key;
    'IVF<nlist>,SQ<x>' with another x (Faiss also has SQ4 and SQ6) raises, naming the key."""
    m = _IVFSQ_FACTORY_RE.match(key.replace(" ", ""))
    if not m:
        return None
    if m.group(2) not in _SQ_FACTORY_TYPES:
        raise RuntimeError(f"index_factory: unsupported scalar quantizer key {key!r} "
                           "(supported: 'IVF<nlist>,SQ8', 'IVF<nlist>,SQfp16')")
    return int(m.group(1)), _SQ_FACTORY_TYPES[m.group(2)]


def parse_binary_factory(key):
    """'BFlat' -> True; any other key raises, naming it (Faiss also has BIVF, BHNSW, BHash)."""
    if key.replace(" ", "") != "BFlat":
        raise RuntimeError(f"index_binary_factory: unsupported key {key!r} (supported: 'BFlat')")
    return True


def index_binary_factory(d, key, device=None):
    """faiss.index_binary_factory(d, "BFlat"): d in bits."""
    parse_binary_factory(key)
    return IndexBinaryFlat(d, device)


def index_factory(d, key, metric=METRIC_L2, device=None):
    """faiss.index_factory(d, "IVF1024,PQ16") (bench_polysemous_1bn.py:272), the
    OPQ-fronted "OPQ16,IVF262144,PQ16" (bench_gpu_1bn.py:10-17), the flat
    "PQ96" / "OPQ96_384,PQ96" (the indexes of beir faiss_search.py:168-224) and
    "IVF<nlist>,Flat" (bench_on_disk_performance.py:37; the "IVF1,Flat" ground
    truth of compute_ground_truth.py:311), "IVF<nlist>,SQ8" / "IVF<nlist>,SQfp16" (an
    IndexIVFScalarQuantizer, by_residual as in Faiss), the flat scalar quantizers "SQ8" / "SQfp16", and
    "Flat" (an IndexFlat of the given metric: beir faiss_search.py:337).  Each may stand behind
    a PCA front, "PCA<dout>," / "PCAR<dout>," / "PCAW<dout>," / "PCAWR<dout>," (bench_gpu_1bn.py:
    490-492): IndexPreTransform(PCAMatrix(d, dout, ...), the rest built at dout)."""
    from .transform import IndexPreTransform, OPQMatrix, PCAMatrix

    front = parse_pca_front(key)
    if front is not None:
        dout, eigen_power, rotate, rest = front
        pca = PCAMatrix(d, dout, eigen_power, rotate)
        pca._check_trainable()  # (dout > d raises here, naming both)
        inner = index_factory(dout, rest, metric, device)
        if isinstance(inner, IndexPreTransform):  # "PCA64,OPQ16,IVF..": one chain
            return IndexPreTransform([pca] + list(inner.chain), inner.index)
        return IndexPreTransform(pca, inner)
    if key.replace(" ", "") == "Flat":
        return IndexFlat(d, metric, device)
    qtype = parse_sq_factory(key)
    if qtype is not None:
        return IndexScalarQuantizer(d, qtype, metric, device)
    nlist = parse_ivfflat_factory(key)
    if nlist is not None:
        return IndexIVFFlat(None, d, nlist, metric, device)
    f = parse_ivfsq_factory(key)
    if f is not None:
        return IndexIVFScalarQuantizer(None, d, f[0], f[1], metric, True, device)
    f = parse_pq_factory(key)
    if f is not None:
        if len(f) == 2:
            return IndexPQ(d, f[0], f[1], metric, device)
        opq = OPQMatrix(d, f[2], f[3])
        return IndexPreTransform(opq, IndexPQ(opq.d_out, f[0], f[1], metric, device))
    f = parse_factory(key)
    if len(f) == 3:
        nlist, M, nbits = f
        return IndexIVFPQ(None, d, nlist, M, nbits, metric, device)
    nlist, M, nbits, opq_M, opq_dout = f
    opq = OPQMatrix(d, opq_M, opq_dout)
    return IndexPreTransform(opq, IndexIVFPQ(None, opq.d_out, nlist, M, nbits, metric, device))


class ParameterSpace:
    """faiss.ParameterSpace subset: set_index_parameters(index, "nprobe=16")."""

    def initialize(self, index):
        pass

    def set_index_parameter(self, index, name, value):
        if name != "nprobe":
            raise RuntimeError(f"unsupported parameter {name}")
        index.nprobe = int(value)

    def set_index_parameters(self, index, params):
        for kv in params.split(","):
            if not kv:
                continue
            name, value = kv.split("=")
            self.set_index_parameter(index, name.strip(), float(value))


def write_index(index, path, fmt="faiss"):
    """Persist ``index``.  fmt "faiss": the Faiss 1.7.1 IndexIVFPQ / IndexPQ /
    IndexIVFFlat / IndexIVFScalarQuantizer / IndexScalarQuantizer / IndexFlat / IndexPreTransform binary layout (``faiss.read_index`` loads it; faiss_io.py);
    "native": this library's CHIVFPQ1 image (also keeps untrained indexes; IVF-PQ only)."""
    from .transform import IndexPreTransform, _transform_bytes

    # every class that has a Faiss layout states it: _faiss_bytes() and, for the messages, _faiss_name
    if isinstance(index, IndexPreTransform):
        if fmt != "faiss" or not index.is_trained:
            raise RuntimeError("IndexPreTransform is written in the Faiss layout once trained")
        chain = [_transform_bytes(t) for t in index.chain]
        buf = faiss_io.serialize_pretransform(index.d, index.metric_type, chain, index.index._faiss_bytes(),
                                              index.ntotal)
    elif not isinstance(index, IndexIVFPQ):
        if fmt != "faiss":
            raise RuntimeError(f"{index._faiss_name} is written in the Faiss layout")
        if not index.is_trained:
            raise RuntimeError(f"{index._faiss_name} is written once trained")
        buf = index._faiss_bytes()
    elif fmt == "native" or not index.is_trained:
        _lib.check(index._c.save(index._h, str(path).encode()))
        return
    elif fmt != "faiss":
        raise RuntimeError(f"unknown index file format {fmt!r}")
    else:
        buf = index._faiss_bytes()
    with open(path, "wb") as f:
        f.write(buf)


def _listed(lists):
    """The non-empty lists [(ids, rows)] of a parsed file as one (list_no, rows, ids), or None."""
    nonempty = [(l, ids, rows) for l, (ids, rows) in enumerate(lists) if len(ids)]
    if not nonempty:
        return None
    return (np.concatenate([np.full(len(ids), l, np.int64) for l, ids, _ in nonempty]),
            np.concatenate([rows for _, _, rows in nonempty]), np.concatenate([ids for _, ids, _ in nonempty]))


def _ivfpq_from_dict(z, device):
    idx = IndexIVFPQ(None, z["d"], z["nlist"], z["M"], z["nbits"], z["metric"], device)
    if z["is_trained"]:
        idx.set_trained(z["centroids"], z["codebook"])
        listed = _listed(z["lists"])
        if listed:
            idx.add_preencoded(*listed)
    idx.nprobe = max(1, min(int(z["nprobe"]), z["nlist"]))
    return idx


def _pq_from_dict(z, device):
    idx = IndexPQ(z["d"], z["M"], z["nbits"], z["metric"], device)
    if z["is_trained"]:
        idx.set_trained(z["codebook"])
        if z["ntotal"]:
            idx.add_codes(z["codes"])
    return idx


def _ivfflat_from_dict(z, device):
    """The lists' vectors are added with their ids: each is assigned again by the
    coarse quantizer, which puts a vector this library wrote back into its list."""
    idx = IndexIVFFlat(None, z["d"], z["nlist"], z["metric"], device)
    if z["is_trained"]:
        idx.set_trained(z["centroids"])
        listed = _listed(z["lists"])
        if listed:
            idx.add_with_ids(listed[1], listed[2])
    idx.nprobe = max(1, min(int(z["nprobe"]), z["nlist"]))
    return idx


def _ivfsq_from_dict(z, device):
    """Centroids, quantizer table and the lists' codes and ids are installed as read: nothing
    is assigned or encoded again."""
    idx = IndexIVFScalarQuantizer(None, z["d"], z["nlist"], z["qtype"], z["metric"], z["by_residual"], device)
    if z["is_trained"]:
        idx.set_trained(z["centroids"], z["trained"])
        listed = _listed(z["lists"])
        if listed:
            idx.add_codes(*listed)
    idx.nprobe = max(1, min(int(z["nprobe"]), z["nlist"]))
    return idx


def _sq_from_dict(z, device):
    idx = IndexScalarQuantizer(z["d"], z["qtype"], z["metric"], device)
    if z["is_trained"]:
        idx.set_trained(z["trained"])
        if z["ntotal"]:
            idx.add_codes(z["codes"])
    return idx


def _flat_from_dict(z, device):
    cls = {METRIC_L2: IndexFlatL2, METRIC_INNER_PRODUCT: IndexFlatIP}[z["metric"]]
    idx = cls(z["d"], device)
    if z["ntotal"]:
        idx.add(z["xb"])
    return idx


_FROM_DICT = {"flat": _flat_from_dict, "ivfflat": _ivfflat_from_dict, "ivfsq": _ivfsq_from_dict, "sq": _sq_from_dict,
              "pq": _pq_from_dict, "ivfpq": _ivfpq_from_dict}  # by faiss_io.parse_index's "kind"


def read_index(path, device=None):
    """Load a Faiss IndexIVFPQ ("IwPQ") / IndexPQ ("IxPq") / IndexIVFFlat ("IwFl") / IndexIVFScalarQuantizer ("IwSq") / IndexScalarQuantizer ("IxSQ") / IndexFlatL2 ("IxF2") / IndexFlatIP ("IxFI") / IndexPreTransform ("IxPT")
    file or a CHIVFPQ1 image onto ``device``."""
    device = _default_device() if device is None else device
    with open(path, "rb") as f:
        if f.read(4) == faiss_io.FOURCC_BINARY_FLAT:
            raise RuntimeError(f"{path}: fourcc {faiss_io.FOURCC_BINARY_FLAT!r} is a binary index "
                               "(IndexBinaryFlat): read it with read_index_binary")
    if faiss_io.is_faiss_file(path):
        with open(path, "rb") as f:
            z = faiss_io.parse_index(f.read())
        if z["kind"] != "pretransform":
            return _FROM_DICT[z["kind"]](z, device)
        from .transform import IndexPreTransform, _linear_from_dict

        sub = z["index"]
        return IndexPreTransform([_linear_from_dict(t) for t in z["chain"]], _FROM_DICT[sub["kind"]](sub, device))
    h = _lib.c_handle()
    L = _lib.load()
    _lib.check(L.ivfpq_load(str(path).encode(), device, ctypes.byref(h)))
    dims = [ctypes.c_int() for _ in range(5)]
    _lib.check(L.ivfpq_get_dims(h, *[ctypes.byref(v) for v in dims]))
    d, nlist, M, nbits, metric = [v.value for v in dims]
    idx = IndexIVFPQ(None, d, nlist, M, nbits, metric, device, _handle=h)
    if idx.is_trained:
        idx._sync_quantizer()
    return idx


def write_index_binary(index, path):
    """faiss.write_index_binary: an IndexBinaryFlat in Faiss's "IBxF" layout (faiss_io.py)."""
    if not isinstance(index, IndexBinaryFlat):
        raise RuntimeError(f"write_index_binary takes an IndexBinaryFlat, got {type(index).__name__}")
    with open(path, "wb") as f:
        f.write(faiss_io.serialize_binary_flat(index.d, index._codes(0, index.ntotal)))


def read_index_binary(path, device=None):
    """faiss.read_index_binary: load an "IBxF" file onto ``device``."""
    with open(path, "rb") as f:
        z = faiss_io.parse_index_binary(f.read())
    idx = IndexBinaryFlat(z["d"], device)
    if z["ntotal"]:
        idx.add(z["codes"])
    return idx
