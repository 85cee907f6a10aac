"""What the index classes of ``faiss_amd.index`` are built on: the handle of one C-ABI family, the
argument checks in front of the raw pointers, and the calls that read the same in every family."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib

MAX_K = 1024
_C_PTR = {np.dtype(t): p for t, p in ((np.float32, _lib.c_f32p), (np.int64, _lib.c_i64p), (np.uint8, _lib.c_u8p),
                                      (np.int32, _lib.c_i32p))}


def _f32(x, d=None, name="x"):
    a = np.ascontiguousarray(x, dtype=np.float32)
    if a.ndim != 2 or (d is not None and a.shape[1] != d):
        raise RuntimeError(f"{name} must be a float32 matrix with {d} columns, got shape {a.shape}")
    return a


def _ptr(a, t=None):
    """The array's data as the C pointer of its dtype (or ``t``); the pointer keeps the array alive."""
    return a.ctypes.data_as(t or _C_PTR[a.dtype])


def _ids_ptr(ids, n, rows):
    """The labels argument of an add: NULL for None (sequential labels), else ``ids`` as n int64."""
    if ids is None:
        return None
    ids = np.ascontiguousarray(ids, np.int64).reshape(-1)
    if ids.shape[0] != n:
        raise RuntimeError(f"ids and {rows} have different lengths")
    return _ptr(ids)


def _default_device():
    try:
        import torch

        if torch.cuda.is_available():
            return torch.cuda.current_device()
    except Exception:
        pass
    return 0


class _HandleIndex:
    """An index behind a library handle ``_h``.  A subclass names its C-ABI family (``_c``), makes the
    handle in its constructor (``_create``) and writes only what its family alone has; the rest is here.
    Where the rows are not float32 [n, d], it overrides ``_host_rows``, ``_dev_row`` and ``_dist``."""

    _c = None          # _lib.Family(prefix): _c.search is <prefix>search
    _dist = "float32"  # dtype of the distances D

    def __init__(self, d, metric, device):
        self.d = int(d)
        self.metric_type = metric
        self.device = _default_device() if device is None else int(device)
        self.verbose = False

    def _create(self, *args):
        h = _lib.c_handle()
        _lib.check(self._c.create(*args, ctypes.byref(h)))
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and _lib._lib is not None:
            self._c.free(h)
            self._h = None

    def _handle(self):
        """The handle, as the last step before a call that searches or adds (IndexFlat makes its own here)."""
        return self._h

    @property
    def ntotal(self):
        return int(self._c.ntotal(self._h))

    @property
    def is_trained(self):
        return bool(self._c.is_trained(self._h))

    def reset(self):
        _lib.check(self._c.reset(self._h))

    def _codes(self, i0, n):
        """Rows [i0, i0 + n) of a flat index of codes: uint8 [n][code_size]."""
        out = np.empty((n, self.code_size), np.uint8)
        _lib.check(self._c.get_codes(self._h, int(i0), int(n), _ptr(out)))
        return out

    # ---------------------------------------------------------------- host arrays
    def _host_rows(self, x):
        return _f32(x, self.d)

    def add(self, x):
        x = self._host_rows(x)
        _lib.check(self._c.add(self._handle(), x.shape[0], _ptr(x)))

    def add_with_ids(self, x, ids):
        raise RuntimeError("add_with_ids not implemented for this type of index")  # Faiss Index::add_with_ids

    def search(self, x, k):
        x = self._host_rows(x)
        self._check_k(k)
        n = x.shape[0]
        D = np.empty((n, k), self._dist)
        I = np.empty((n, k), np.int64)
        _lib.check(self._c.search(self._handle(), n, _ptr(x), int(k), _ptr(D), _ptr(I)))
        return D, I

    # ------------------------------------------------- device (torch) arguments
    def _check_k(self, k):
        if not 1 <= int(k) <= MAX_K:
            raise RuntimeError(f"k must be in [1, {MAX_K}], got {k}")

    def _check_dev(self, t, name, dtype, shape):
        """The C-ABI takes raw device pointers: anything but a contiguous tensor of
        the exact dtype and shape on this index's device would be read or written
        out of bounds, so it is rejected here (as the host path rejects bad arrays)."""
        import torch

        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise RuntimeError(f"{name} must be a CUDA tensor")
        if t.device.index != self.device:
            raise RuntimeError(f"{name} is on cuda:{t.device.index}, the index on cuda:{self.device}")
        if t.dtype != dtype:
            raise RuntimeError(f"{name} must be {dtype}, got {t.dtype}")
        if tuple(t.shape) != tuple(shape):
            raise RuntimeError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
        if not t.is_contiguous():
            raise RuntimeError(f"{name} must be contiguous")
        return t

    def _dev_row(self):
        """(dtype, width) of one row of queries or vectors in HBM."""
        import torch

        return torch.float32, self.d

    def _dev_rows(self, t, name="x"):
        """The row count of the device argument ``t``, checked as [n, width] rows of this index
        (anything but a 2-D tensor has no row count and fails the check)."""
        dtype, width = self._dev_row()
        n = t.shape[0] if hasattr(t, "dim") and t.dim() == 2 else -1
        self._check_dev(t, name, dtype, (n, width))
        return n

    def _dev_outputs(self, x, k, D, I):
        import torch

        n, dist = x.shape[0], getattr(torch, self._dist)
        if D is None:
            D = torch.empty((n, k), dtype=dist, device=x.device)
        if I is None:
            I = torch.empty((n, k), dtype=torch.int64, device=x.device)
        self._check_dev(D, "D", dist, (n, k))
        self._check_dev(I, "I", torch.int64, (n, k))
        return D, I

    def _stream(self, x, stream):
        import torch

        return stream if stream is not None else torch.cuda.current_stream(x.device).cuda_stream

    def search_device(self, x, k, D=None, I=None, stream=None):
        """Search with the queries resident in HBM (torch CUDA tensor [n, d] float32; an IndexBinaryFlat's
        are [n, code_size] uint8) on the index's device; returns torch (D, I) there, launched on
        ``stream`` (default: torch's current stream)."""
        self._check_k(k)
        n = self._dev_rows(x)
        D, I = self._dev_outputs(x, k, D, I)
        _lib.check(self._c.search_device(self._handle(), n, x.data_ptr(), int(k), D.data_ptr(), I.data_ptr(),
                                         ctypes.c_void_p(self._stream(x, stream))))
        return D, I

    def add_device(self, x, stream=None):
        """add with the rows already in HBM (as ``search_device``'s queries); returns once they are in place."""
        n = self._dev_rows(x)
        _lib.check(self._c.add_device(self._handle(), n, x.data_ptr(), ctypes.c_void_p(self._stream(x, stream))))


class _ListsView:
    """index.invlists of an IVF index (faiss ArrayInvertedLists read API), read through the owner's
    family: a list's rows are ``code_size`` bytes each, ``_row`` values in the library."""

    _row = np.uint8

    def __init__(self, owner):
        self._o = owner

    @property
    def nlist(self):
        return self._o.nlist

    @property
    def code_size(self):
        return self._o.code_size

    def list_sizes(self):
        out = np.empty(self._o.nlist, np.int64)
        _lib.check(self._o._c.get_list_sizes(self._o._h, _ptr(out)))
        return out

    def list_size(self, l):
        return int(self.list_sizes()[l])

    def _get(self, l):
        rows = np.empty((self.list_size(l), self.code_size // np.dtype(self._row).itemsize), self._row)
        ids = np.empty(rows.shape[0], np.int64)
        _lib.check(self._o._c.get_list(self._o._h, int(l), _ptr(rows), _ptr(ids)))
        return rows, ids

    def get_codes(self, l):
        return self._get(l)[0].view(np.uint8).reshape(-1)

    def get_ids(self, l):
        return self._get(l)[1]

    def imbalance_factor(self):
        """faiss InvertedLists::imbalance_factor: nlist * sum(n_l^2) / ntotal^2."""
        s = self.list_sizes().astype(np.float64)
        tot = s.sum()
        return float(len(s) * (s * s).sum() / (tot * tot)) if tot else 0.0
