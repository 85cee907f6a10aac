"""The ``faiss.Gpu*`` names the reference's GPU scripts use on a flat index (``bench_gpu_sift1m.py:33-53``;
the ``-float16`` switch of ``bench_gpu_1bn*.py``): ``StandardGpuResources``, ``GpuIndexFlatConfig``
(``device``, ``useFloat16``), ``GpuIndexFlat``, ``GpuIndexFlatL2``, ``GpuIndexFlatIP``.  Every index of this
package lives on the GPU already, so the classes are ``IndexFlat`` with Faiss-GPU's constructor; what
``useFloat16`` adds is the half-precision device image and its scan (csrc/flat_scan_f16.hip).

The package resolves these five names on attribute access (``faiss_amd.GpuIndexFlatL2`` and
``from faiss_amd import GpuIndexFlatL2`` both work; ``faiss_amd/__init__.py``) and loads this module then."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._handle import _f32
from .index import METRIC_INNER_PRODUCT, METRIC_L2, IndexFlat

__all__ = ["StandardGpuResources", "GpuIndexFlatConfig", "GpuIndexFlat", "GpuIndexFlatL2", "GpuIndexFlatIP"]


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
