"""The ``faiss.Gpu*`` names the reference's GPU scripts use (``bench_gpu_sift1m.py``; the ``-float16`` switch
of ``bench_gpu_1bn*.py``).  On a flat index: ``StandardGpuResources``, ``GpuIndexFlatConfig`` (``device``,
``useFloat16``), ``GpuIndexFlat``, ``GpuIndexFlatL2``, ``GpuIndexFlatIP``.  Every index of this package lives
on the GPU already, so the classes are ``IndexFlat`` with Faiss-GPU's constructor; what ``useFloat16`` adds
is the half-precision device image and its scan (csrc/flat_scan_f16.hip).  On an IVF index
(``bench_gpu_sift1m.py:71-88``): ``GpuClonerOptions``, ``index_cpu_to_gpu``, and the ``GpuIndexIVFPQ`` /
``GpuIndexIVFFlat`` it returns, which carry ``setNumProbes`` and, for IVF-PQ, ``use_float16_lut`` (float16
lookup tables in the list scan, csrc/ivfpq_kernels.hip k_scan_lists_h).

The package resolves these names on attribute access (``faiss_amd.GpuIndexFlatL2`` and
``from faiss_amd import GpuIndexFlatL2`` both work; ``faiss_amd/__init__.py``) and loads this module then."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._handle import _f32
from .index import METRIC_INNER_PRODUCT, METRIC_L2, IndexFlat, IndexIVFFlat, IndexIVFPQ
from .transform import IndexPreTransform

__all__ = ["StandardGpuResources", "GpuIndexFlatConfig", "GpuIndexFlat", "GpuIndexFlatL2", "GpuIndexFlatIP",
           "GpuClonerOptions", "GpuIndexIVFPQ", "GpuIndexIVFFlat", "index_cpu_to_gpu"]


class StandardGpuResources:
    """faiss.StandardGpuResources(): an empty holder (bench_gpu_sift1m.py:33; bench_gpu_1bn.py
    calls noTempMemory / setTempMemory on it).  The workspaces here belong to the index handles,
    so the temporary-memory calls do nothing."""

    def noTempMemory(self):
        pass

    def setTempMemory(self, n):
        pass


class GpuIndexFlatConfig:
    """faiss.GpuIndexFlatConfig(): ``device`` and ``useFloat16`` (bench_gpu_sift1m.py:42-43)."""

    def __init__(self):
        self.device = 0
        self.useFloat16 = False


class GpuIndexFlat(IndexFlat):
    """faiss.GpuIndexFlat(res, d, metric, config).  With ``config.useFloat16`` false it is an
    ``IndexFlat`` on ``config.device``.  With it true the device image holds IEEE halves, 2 d
    bytes per row, and the search runs csrc/flat_scan_f16.hip (Faiss-GPU's arithmetic: rows and
    queries rounded to half, nearest even, values beyond the half range to +-inf; products and
    sums in fp32 on the matrix cores; L2 from the norms of the rounded values).  The host buffer
    holds the rounded rows too, so ``xb``, ``reconstruct*`` and ``write_index`` -- an ordinary
    IxF2 / IxFI file, what index_gpu_to_cpu + write_index give in Faiss -- agree with the
    image; ``read_index`` of that file is a plain ``IndexFlat``."""

    def __init__(self, res, d, metric=METRIC_L2, config=None):
        IndexFlat.__init__(self, d, metric, None if config is None else config.device)
        self._f16 = bool(config is not None and config.useFloat16)

    def _create(self, *args):
        h = _lib.c_handle()
        _lib.check((self._c.create_f16 if self._f16 else self._c.create)(*args, ctypes.byref(h)))
        self._h = h

    def add(self, x):
        x = _f32(x, self.d)
        if self._f16:
            with np.errstate(over="ignore"):  # beyond the half range: +-inf, as the device rounds
                x = x.astype(np.float16).astype(np.float32)
        IndexFlat.add(self, x)


class GpuIndexFlatL2(GpuIndexFlat):
    """faiss.GpuIndexFlatL2(res, d, config) (bench_gpu_sift1m.py:45)."""

    def __init__(self, res, d, config=None):
        GpuIndexFlat.__init__(self, res, d, METRIC_L2, config)


class GpuIndexFlatIP(GpuIndexFlat):
    """faiss.GpuIndexFlatIP(res, d, config)."""

    def __init__(self, res, d, config=None):
        GpuIndexFlat.__init__(self, res, d, METRIC_INNER_PRODUCT, config)


class GpuClonerOptions:
    """faiss.GpuClonerOptions() (bench_gpu_sift1m.py:73-77, bench_gpu_1bn.py:600-612).  ``useFloat16`` is what
    ``index_cpu_to_gpu`` acts on; ``useFloat16CoarseQuantizer`` must stay False (the coarse quantizer here is
    fp32 only); the other fields are accepted and stored (tables are always precomputed, labels always
    64-bit on the device, memory grows on demand)."""

    def __init__(self):
        self.useFloat16 = False
        self.useFloat16CoarseQuantizer = False
        self.usePrecomputed = False
        self.indicesOptions = 0
        self.reserveVecs = 0
        self.verbose = False


class GpuIndexIVFPQ(IndexIVFPQ):
    """faiss.GpuIndexIVFPQ as ``index_cpu_to_gpu`` returns it: an ``IndexIVFPQ`` with ``setNumProbes`` and the
    float16 lookup tables of ``GpuClonerOptions.useFloat16``."""

    @property
    def use_float16_lut(self):
        """True: every search scans with lookup-table entries clamped to +-65504 and rounded once to IEEE
        half; the sums stay fp32 (ivfpq_set_float16_lut).  Per index, default False,
        may be changed between searches, not written to index files."""
        return bool(self._c.get_float16_lut(self._h))

    @use_float16_lut.setter
    def use_float16_lut(self, on):
        _lib.check(self._c.set_float16_lut(self._h, int(bool(on))))

    def setNumProbes(self, n):
        self.nprobe = n


class GpuIndexIVFFlat(IndexIVFFlat):
    """faiss.GpuIndexIVFFlat as ``index_cpu_to_gpu`` returns it: an ``IndexIVFFlat`` with ``setNumProbes``."""

    def setNumProbes(self, n):
        self.nprobe = n


def _clone_ivf(src, dst):
    """The training parameters, the quantizers and the lists of ``src`` into the new index ``dst``."""
    dst.niter_coarse, dst.seed = src.niter_coarse, src.seed
    if src.is_trained:
        if isinstance(src, IndexIVFPQ):
            dst.set_trained(src.centroids(), src.codebook())
            if src.ntotal:
                dst.add_preencoded(*src.invlists.export())
        else:
            dst.set_trained(src.centroids())
            for l in np.nonzero(src.invlists.list_sizes())[0]:
                dst.add_with_ids(src.invlists.get_vectors(l), src.invlists.get_ids(l))
    dst.nprobe = src.nprobe
    return dst


def index_cpu_to_gpu(res, device, index, co=None):
    """faiss.index_cpu_to_gpu(res, device, index, co): a copy of ``index`` on ``device``.  An ``IndexIVFPQ``
    (bare or under ``IndexPreTransform``) comes back as a ``GpuIndexIVFPQ`` with ``use_float16_lut`` from
    ``co.useFloat16``; an ``IndexFlat`` as a ``GpuIndexFlat`` with ``useFloat16``; an ``IndexIVFFlat`` as a
    ``GpuIndexIVFFlat`` (with ``useFloat16`` it raises: half-precision lists are
    ``IndexIVFScalarQuantizer(QT_fp16)``).  Any other index is already on a GPU and is returned as it is,
    which needs ``device`` to be its own."""
    co = co or GpuClonerOptions()
    if co.useFloat16CoarseQuantizer:
        raise RuntimeError("useFloat16CoarseQuantizer is not supported: the coarse quantizer is fp32")
    device = int(device)
    if isinstance(index, IndexPreTransform):
        return IndexPreTransform(list(index.chain), index_cpu_to_gpu(res, device, index.index, co))
    if type(index) in (IndexIVFPQ, GpuIndexIVFPQ):
        out = GpuIndexIVFPQ(None, index.d, index.nlist, index.M, index.nbits, index.metric_type, device)
        out.niter_pq = index.niter_pq
        _clone_ivf(index, out).use_float16_lut = co.useFloat16
        return out
    if type(index) in (IndexIVFFlat, GpuIndexIVFFlat):
        if co.useFloat16:
            raise RuntimeError("IndexIVFFlat has no float16 form: use IndexIVFScalarQuantizer(QT_fp16) "
                               "(index_factory 'IVFn,SQfp16') for half-precision lists")
        return _clone_ivf(index, GpuIndexIVFFlat(None, index.d, index.nlist, index.metric_type, device))
    if isinstance(index, IndexFlat):
        cfg = GpuIndexFlatConfig()
        cfg.device, cfg.useFloat16 = device, bool(co.useFloat16)
        out = GpuIndexFlat(res, index.d, index.metric_type, cfg)
        if index.ntotal:
            out.add(index.xb)
        return out
    if index.device != device:
        raise RuntimeError(f"{type(index).__name__} lives on device {index.device}; it is not copied to {device}")
    return index
