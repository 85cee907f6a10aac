"""faiss.Kmeans / faiss.Clustering: k-means as a stand-alone object.

Lloyd iterations resident on the GPU (csrc/clustering.cpp, csrc/km_update.hip): the rows are
assigned by the flat index's fused scan, ordered by cluster and added in ascending row order
in fp64, so the centroids are those of the library's other trainers and of ``oracle.kmeans``
bit for bit.  Callers: ``bench_gpu_1bn.py:522-542`` (``train_coarse_quantizer``:
``Clustering(d, k)``, ``train(x, index)``, ``vector_float_to_array(clus.centroids)``) and
``wav2vec_cluster_faiss.py:186-203`` (``normalize_L2``, ``Kmeans(..., spherical=...,
gpu=True, nredo=3)``, ``train``, ``centroids``).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .index import (METRIC_INNER_PRODUCT, METRIC_L2, IndexFlatIP, IndexFlatL2, _default_device, _f32, _ptr,
                    vector_to_array)

vector_float_to_array = vector_to_array


def normalize_L2(x):
    """faiss.normalize_L2: every row of x scaled to unit L2 norm, in place, with the
    arithmetic of the spherical trainer (float32 sum of squares in ascending order, one
    multiplication by float32(1 / sqrt)); rows of zero norm are left untouched."""
    if not (isinstance(x, np.ndarray) and x.dtype == np.float32 and x.ndim == 2 and x.flags.c_contiguous):
        raise RuntimeError("normalize_L2: x must be a C-contiguous float32 matrix")
    if not x.flags.writeable:
        raise RuntimeError("normalize_L2: x must be writeable")
    nr = np.zeros(x.shape[0], np.float32)
    for t in range(x.shape[1]):  # one ascending float32 chain per row
        nr += x[:, t] * x[:, t]
    ok = nr > 0
    inv = np.ones(x.shape[0], np.float32)
    inv[ok] = (1.0 / np.sqrt(nr[ok]).astype(np.float64)).astype(np.float32)
    x *= inv[:, None]


def rand_perm_prefix(n, k, seed):
    """The first k entries of the library's seeded random permutation of [0, n): the initial
    centroids of a run, and the rows a subsampled training keeps (not Faiss's generator)."""
    out = np.empty(int(k), np.int64)
    _lib.check(_lib.load().ivfpq_clus_rand_perm_prefix(int(n), int(k), int(seed) & (2**64 - 1),
                                                       _ptr(out, _lib.c_i64p)))
    return out


_REJECTED = ("int_centroids", "frozen_centroids", "weights")


class _Engine:
    """The training both classes share: parameters as attributes, one C-ABI handle per run."""

    def _init_params(self, d, k):
        self.d = int(d)
        self.k = int(k)
        self.niter = 25
        self.nredo = 1
        self.verbose = False
        self.spherical = False
        self.seed = 1234
        self.min_points_per_centroid = 39
        self.max_points_per_centroid = 256
        self.update_index = False  # accepted, no effect
        self.int_centroids = False
        self.frozen_centroids = False
        self.pass_rows = 0
        self.iteration_stats = []
        self.obj = np.zeros(0, np.float64)

    def set_pass_rows(self, rows):
        """Rows of one pass of an iteration (0 = chosen per call); a value > 0 also makes
        ``train`` stream its host rows in every iteration.  Results do not depend on it."""
        rows = int(rows)
        if rows < 0:
            raise RuntimeError("negative pass size")
        self.pass_rows = rows

    def _check_options(self, weights=None):
        for name in ("int_centroids", "frozen_centroids"):
            if getattr(self, name):
                raise RuntimeError(f"Clustering: {name} is not supported")
        if weights is not None:
            raise RuntimeError("Clustering: weights are not supported")
        if int(self.niter) < 0:
            raise RuntimeError(f"Clustering: niter must be at least 0 (niter = {self.niter})")
        if int(self.nredo) < 1:
            raise RuntimeError(f"Clustering: nredo must be at least 1 (nredo = {self.nredo})")

    def _subsample(self, n):
        """Row numbers of the training subsample, or None when all n rows train."""
        kmax = self.k * int(self.max_points_per_centroid)
        if n > kmax:
            if self.verbose:
                print(f"Sampling a subset of {kmax} / {n} for training")
            return rand_perm_prefix(n, kmax, self.seed)
        if n < self.k * int(self.min_points_per_centroid) and self.verbose:
            print(f"WARNING clustering {n} points to {self.k} centroids: please provide at least "
                  f"{self.k * int(self.min_points_per_centroid)} training points")
        return None

    def _run(self, metric, device, x, x_dev, init, stream=None):
        """Train on host rows x or device rows x_dev; returns the centroids [k, d]."""
        L = _lib.load()
        h = _lib.c_handle()
        _lib.check(L.ivfpq_clus_create(self.d, self.k, int(metric), int(bool(self.spherical)), int(device),
                                       ctypes.byref(h)))
        try:
            if self.pass_rows:
                _lib.check(L.ivfpq_clus_set_pass_rows(h, self.pass_rows))
            ip = None
            if init is not None:
                init = _f32(np.asarray(init).reshape(-1, self.d), self.d, "init_centroids")
                if init.shape[0] != self.k:
                    raise RuntimeError(f"init_centroids must hold {self.k} rows, got {init.shape[0]}")
                ip = _ptr(init, _lib.c_f32p)
            seed = int(self.seed) & (2**64 - 1)
            if x_dev is None:
                _lib.check(L.ivfpq_clus_train(h, x.shape[0], _ptr(x, _lib.c_f32p), int(self.niter), int(self.nredo),
                                              seed, ip))
            else:
                _lib.check(L.ivfpq_clus_train_device(h, x_dev.shape[0], x_dev.data_ptr(), int(self.niter),
                                                     int(self.nredo), seed, ip, ctypes.c_void_p(stream)))
            cent = np.empty((self.k, self.d), np.float32)
            _lib.check(L.ivfpq_clus_get_centroids(h, _ptr(cent, _lib.c_f32p)))
            niter = int(self.niter)
            obj = np.zeros(niter, np.float64)
            nsplit = np.zeros(niter, np.int64)
            _lib.check(L.ivfpq_clus_get_stats(h, None, obj.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                              _ptr(nsplit, _lib.c_i64p)))
        finally:
            L.ivfpq_clus_free(h)
        self.obj = obj
        self.iteration_stats = [{"obj": float(obj[i]), "nsplit": int(nsplit[i])} for i in range(niter)]
        if self.verbose:
            for i, st in enumerate(self.iteration_stats):
                print(f"  Iteration {i} objective={st['obj']:g} nsplit={st['nsplit']}")
        return cent

    def _train_host(self, metric, device, x, init):
        x = _f32(x, self.d)
        p = self._subsample(x.shape[0])
        if p is not None:
            x = np.ascontiguousarray(x[p])
        return self._run(metric, device, x, None, init)

    def _train_dev(self, metric, device, x, init, stream=None):
        import torch

        if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
            raise RuntimeError("x must be a CUDA tensor")
        if x.device.index != device:
            raise RuntimeError(f"x is on cuda:{x.device.index}, the clustering on cuda:{device}")
        if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != self.d or not x.is_contiguous():
            raise RuntimeError(f"x must be a contiguous float32 tensor with {self.d} columns")
        if stream is None:
            stream = torch.cuda.current_stream(x.device).cuda_stream
        p = self._subsample(x.shape[0])
        if p is not None:
            x = x.index_select(0, torch.from_numpy(p).to(x.device)).contiguous()
        return self._run(metric, device, None, x, init, stream)


class Kmeans(_Engine):
    """faiss.Kmeans(d, k, niter=25, ...): ``train(x)`` sets ``centroids`` [k, d], ``obj``
    [niter], ``iteration_stats`` and ``index`` (an IndexFlatL2, or IndexFlatIP for spherical
    training, holding the centroids) and returns the final objective.  It always runs on the
    GPU (``gpu`` is accepted and has no effect); ``int_centroids``, ``frozen_centroids`` and
    ``weights`` are not supported."""

    def __init__(self, d, k, niter=25, verbose=False, spherical=False, max_points_per_centroid=256,
                 min_points_per_centroid=39, nredo=1, seed=1234, gpu=False, device=None, **kw):
        self._init_params(d, k)
        self.niter = int(niter)
        self.verbose = bool(verbose)
        self.spherical = bool(spherical)
        self.max_points_per_centroid = int(max_points_per_centroid)
        self.min_points_per_centroid = int(min_points_per_centroid)
        self.nredo = int(nredo)
        self.seed = int(seed)
        self.gpu = gpu
        self.device = _default_device() if device is None else int(device)
        for name, v in kw.items():
            if name in _REJECTED:
                if v is not None and v is not False:
                    raise RuntimeError(f"Kmeans: {name} is not supported")
            elif name == "update_index":
                self.update_index = v
            else:
                raise RuntimeError(f"Kmeans: unknown option {name}")
        self.centroids = None
        self.index = None

    @property
    def _metric(self):
        return METRIC_INNER_PRODUCT if self.spherical else METRIC_L2

    def _finish(self, cent):
        self.centroids = cent
        self.index = (IndexFlatIP if self.spherical else IndexFlatL2)(self.d, self.device)
        self.index.add(cent)
        return float(self.obj[-1]) if len(self.obj) else 0.0

    def train(self, x, weights=None, init_centroids=None):
        self._check_options(weights)
        return self._finish(self._train_host(self._metric, self.device, x, init_centroids))

    def train_device(self, x, init_centroids=None, stream=None):
        """train with the rows already in HBM (torch float32 CUDA tensor [n, d])."""
        self._check_options()
        return self._finish(self._train_dev(self._metric, self.device, x, init_centroids, stream))

    def assign(self, x):
        if self.index is None:
            raise RuntimeError("should train before assigning")
        D, I = self.index.search(_f32(x, self.d), 1)
        return D.ravel(), I.ravel()


class Clustering(_Engine):
    """faiss.Clustering(d, k): parameters as attributes, ``train(x, index)`` with a flat index
    whose metric is the clustering's; afterwards ``index`` holds the k centroids and
    ``centroids`` is the flat float32 array of k d numbers."""

    def __init__(self, d, k):
        self._init_params(d, k)
        self.centroids = np.zeros(0, np.float32)

    def train(self, x, index, weights=None):
        self._check_options(weights)
        if int(getattr(index, "d", self.d)) != self.d:
            raise RuntimeError(f"Clustering: the index has d = {index.d}, the clustering d = {self.d}")
        if index.ntotal != 0:
            raise RuntimeError("Clustering: the index must be empty (ntotal == 0) and trained")
        device = getattr(index, "device", None)
        cent = self._train_host(index.metric_type, _default_device() if device is None else device, x, None)
        index.add(cent)
        self.centroids = cent.reshape(-1)
