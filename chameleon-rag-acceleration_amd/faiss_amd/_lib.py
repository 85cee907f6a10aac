"""ctypes binding of libivfpq.so (C-ABI declared in include/ivfpq.h).

The library is the only compute path: if it cannot be loaded the import of the
functions that need it fails loudly (there is no CPU fallback).
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import threading

_PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_PKG)  # chameleon-rag-acceleration_amd/
LIB_PATH = os.environ.get("IVFPQ_LIB") or os.path.join(ROOT, "lib", "libivfpq.so")  # IVFPQ_LIB: A/B builds
CSRC = os.path.join(ROOT, "csrc")

_lock = threading.Lock()
_lib = None

c_f32p = ctypes.POINTER(ctypes.c_float)
c_i64p = ctypes.POINTER(ctypes.c_int64)
c_u8p = ctypes.POINTER(ctypes.c_uint8)
c_i32p = ctypes.POINTER(ctypes.c_int32)
c_handle = ctypes.c_void_p

_int, _i64, _u64, _vp = ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_void_p
_intp, _u64p, _f64p = ctypes.POINTER(_int), ctypes.POINTER(_u64), ctypes.POINTER(ctypes.c_double)
_new = ctypes.POINTER(c_handle)


def _rc(*argtypes):
    """(restype, argtypes) of a function that returns the status code."""
    return (_int, list(argtypes))


def _create(n):
    return _rc(*[_int] * n, _new)


def _dims(n):
    return _rc(c_handle, *[_intp] * n)


# The argument lists that more than one index family declares (include/ivfpq.h).
HANDLE = _rc(c_handle)                                   # free, reset, is_trained, get_nprobe
NTOTAL = (_i64, [c_handle])
SET_INT = _rc(c_handle, _int)                            # set_nprobe and the other switches
SET_I64 = _rc(c_handle, _i64)
F32_ROWS = _rc(c_handle, _i64, c_f32p)                   # add without ids
U8_ROWS = _rc(c_handle, _i64, c_u8p)                     # add_codes
ADD_IDS = _rc(c_handle, _i64, c_f32p, c_i64p)            # add of an IVF family: ids or NULL
ADD_DEVICE = _rc(c_handle, _i64, _vp, _vp)
ADD_DEVICE_IDS = _rc(c_handle, _i64, _vp, _vp, _vp)
ADD_LISTED = _rc(c_handle, _i64, c_i64p, c_u8p, c_i64p)  # codes with their list numbers and ids
TRAIN = _rc(c_handle, _i64, c_f32p, _int, _u64)          # rows, iterations, seed
SEARCH = _rc(c_handle, _i64, c_f32p, _int, c_f32p, c_i64p)
SEARCH_DEVICE = _rc(c_handle, _i64, _vp, _int, _vp, _vp, _vp)
SEARCH_PREASSIGNED = _rc(c_handle, _i64, c_f32p, _int, c_i64p, c_f32p, c_f32p, c_i64p)
SEARCH_PREASSIGNED_DEVICE = _rc(c_handle, _i64, _vp, _int, _vp, _vp, _vp, _vp, _vp)
F32_ARRAY = _rc(c_handle, c_f32p)                        # get_centroids, get_codebook, a one-table set_trained
I64_ARRAY = _rc(c_handle, c_i64p)                        # get_list_sizes
GET_TRAINED = _rc(c_handle, c_f32p, c_i64p)
GET_CODES = _rc(c_handle, _i64, _i64, c_u8p)
QUERY_CHUNK = _rc(_i64, _i64, c_i64p)


def _family(prefix, **own):
    """The signatures of one index family: what all seven have, then its own (which may replace one)."""
    every = dict(free=HANDLE, reset=HANDLE, ntotal=NTOTAL, search=SEARCH, search_device=SEARCH_DEVICE)
    return {prefix + name: sig for name, sig in {**every, **own}.items()}


def _ivf(list_row):
    """What the three IVF families add to _family's; list_row: the pointer type of a list's rows."""
    return dict(is_trained=HANDLE, add=ADD_IDS, add_device=ADD_DEVICE_IDS, set_nprobe=SET_INT, get_nprobe=HANDLE,
                search_preassigned=SEARCH_PREASSIGNED, search_preassigned_device=SEARCH_PREASSIGNED_DEVICE,
                get_centroids=F32_ARRAY, get_list_sizes=I64_ARRAY, get_list=_rc(c_handle, _int, list_row, c_i64p))


# name -> (restype, argtypes); mirrors include/ivfpq.h one to one, plus the
# test hooks of include/ivfpq_test.h (used only by tests/).
SIGNATURES = {
    "ivfpq_last_error": (ctypes.c_char_p, []),
    "ivfpq_device_count": _rc(),
    "ivfpq_overlap_built": _rc(),
    "ivfpq_load": _rc(ctypes.c_char_p, _int, _new),
    "ivfpq_flat_search": _rc(_int, _int, _i64, c_f32p, _i64, c_f32p, _int, _int, c_f32p, c_i64p),
    "ivfpq_merge_topk_device": _rc(_int, _i64, _int, _int, _vp, _vp, _vp, _vp, _vp),
    "ivfpq_linear_transform_device": _rc(_i64, _int, _int, _vp, _vp, _vp, _vp, _vp),
    # PCA training moments (PCAMatrix.train), their chunk setting and plan
    "ivfpq_pca_moments_device": _rc(_i64, _int, _vp, _vp, _vp, _vp),
    "ivfpq_pca_set_chunk_rows": _rc(_i64),
    "ivfpq_pca_get_plan": _rc(_i64, _int, _intp, c_i64p, _intp),
    # IVF-PQ (IndexIVFPQ)
    **_family(
        "ivfpq_", **_ivf(c_u8p), create=_create(6), get_dims=_dims(5),
        train=_rc(c_handle, _i64, c_f32p, _int, _int, _u64), set_trained=_rc(c_handle, c_f32p, c_f32p),
        add_preencoded=ADD_LISTED, set_list_range=_rc(c_handle, _int, _int),
        get_codebook=F32_ARRAY, get_precomputed_table=F32_ARRAY, save=_rc(c_handle, ctypes.c_char_p),
        precompute_tables_device=_rc(c_handle, _i64, _vp, _vp, _u64p),
        search_preassigned_tables_device=_rc(c_handle, _i64, _vp, _int, _vp, _vp, _vp, _vp, _u64, _vp),
        coarse_device=_rc(c_handle, _i64, _vp, _vp, _vp, _vp),
        coarse_tables_device=_rc(c_handle, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _u64p),
        serve_request=_rc(c_handle, c_u8p, _i64, _int, _int, _int, _int, c_u8p, _i64, c_i64p),
        set_inflight=SET_INT, get_inflight=HANDLE, set_timing=SET_INT, get_timing=_rc(c_handle, _f64p, c_i64p),
        get_error_count=I64_ARRAY, get_repair_stats=_rc(c_handle, c_i64p, c_i64p),
        get_repair_log=_rc(c_handle, ctypes.POINTER(ctypes.c_uint32), _int, _intp), set_fault_injection=SET_INT,
        debug_workspace=_rc(c_handle, _int, _int, _vp, _i64, c_i64p), debug_seed_tau=_rc(c_handle, _i64, _vp)),
    # flat product quantizer (IndexPQ)
    **_family(
        "ivfpq_pq_", create=_create(5), get_dims=_dims(4), is_trained=HANDLE, train=TRAIN, set_trained=F32_ARRAY,
        add=F32_ROWS, add_device=ADD_DEVICE, add_codes=U8_ROWS, get_codebook=F32_ARRAY, get_codes=GET_CODES,
        debug_plan=_rc(_int, _int, _i64, _i64, _intp, _intp, c_i64p, _intp, c_i64p)),
    # IVF over raw vectors (IndexIVFFlat)
    **_family("ivfpq_ivfflat_", **_ivf(c_f32p), create=_create(4), get_dims=_dims(3), train=TRAIN,
              set_trained=F32_ARRAY),
    # flat scalar quantizer (IndexScalarQuantizer)
    **_family(
        "ivfpq_sq_", create=_create(4), get_dims=_dims(4), is_trained=HANDLE, train=F32_ROWS,
        set_trained=_rc(c_handle, c_f32p, _i64), get_trained=GET_TRAINED, add=F32_ROWS, add_device=ADD_DEVICE,
        add_codes=U8_ROWS, get_codes=GET_CODES, encode=_rc(c_handle, _i64, c_f32p, c_u8p),
        decode=_rc(c_handle, _i64, c_u8p, c_f32p), get_plan=_rc(_i64, _i64, _int, _intp, _intp, c_i64p)),
    # IVF over scalar-quantizer codes (IndexIVFScalarQuantizer)
    **_family("ivfpq_ivfsq_", **_ivf(c_u8p), create=_create(6), get_dims=_dims(6), train=TRAIN,
              set_trained=_rc(c_handle, c_f32p, c_f32p, _i64), get_trained=GET_TRAINED, add_codes=ADD_LISTED),
    # flat binary codes (IndexBinaryFlat)
    **_family(
        "ivfpq_bin_", create=_create(2), get_dims=_dims(2), add=U8_ROWS, add_device=ADD_DEVICE, get_codes=GET_CODES,
        search=_rc(c_handle, _i64, c_u8p, _int, c_i32p, c_i64p),
        get_plan=_rc(_int, _i64, _i64, _int, _intp, _intp, _intp, c_i64p, c_i64p)),
    # flat fp32 rows (IndexFlat / IndexFlatL2 / IndexFlatIP)
    **_family(
        "ivfpq_flat_index_", create=_create(3), get_dims=_dims(2), add=F32_ROWS, add_device=ADD_DEVICE,
        get_rows=_rc(c_handle, _i64, _i64, c_f32p), get_stats=_rc(c_handle, c_i64p, c_i64p, c_i64p),
        set_range_rows=SET_I64,
        get_plan=_rc(_i64, _i64, _int, _i64, _intp, c_i64p, _intp, _intp, _intp, _intp, c_i64p)),
    # stand-alone k-means (Kmeans / Clustering)
    "ivfpq_clus_create": _create(5),
    "ivfpq_clus_free": HANDLE,
    "ivfpq_clus_train": _rc(c_handle, _i64, c_f32p, _int, _int, _u64, c_f32p),
    "ivfpq_clus_train_device": _rc(c_handle, _i64, _vp, _int, _int, _u64, c_f32p, _vp),
    "ivfpq_clus_get_centroids": F32_ARRAY,
    "ivfpq_clus_get_stats": _rc(c_handle, _intp, _f64p, c_i64p),
    "ivfpq_clus_set_pass_rows": SET_I64,
    "ivfpq_clus_rand_perm_prefix": _rc(_i64, _i64, _u64, c_i64p),
    # how the host cuts a batch into chunks (host arithmetic; faiss_amd.index.*_split)
    "ivfpq_ivf_get_plan": _rc(_int, _i64, _intp, _intp),
    "ivfpq_ivf_get_query_chunk": _rc(_i64, *[_int] * 7, c_i64p),
    "ivfpq_ivf_get_pass_rows": _rc(_i64, _int, _int, _int, c_i64p),
    "ivfpq_get_query_chunk": _rc(_i64, *[_int] * 6, c_i64p),
    "ivfpq_host_get_pass_rows": QUERY_CHUNK,
    "ivfpq_flat_search_get_query_chunk": QUERY_CHUNK,
    "ivfpq_kmeans_get_assign_rows": _rc(_i64, _int, c_i64p),
}


def kernel_source_sha256() -> str:
    """sha256 of what the GPU kernels are compiled from (the kernel source, its
    headers, the Makefile's flags): the key under which counter measurements of
    the kernels stay valid across builds that change host code only."""
    import hashlib

    h = hashlib.sha256()
    for f in ("ivfpq_kernels.hip", "ivfpq_kernels.h", "ivfpq_diag.h", "Makefile"):
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(f.encode() + b"\0" + fh.read() + b"\0")
    return h.hexdigest()


def build(force: bool = False) -> str:
    """Compile libivfpq.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp", ".h"))]
    srcs += [os.path.join(os.path.dirname(ROOT), "include", h) for h in ("ivfpq.h", "ivfpq_test.h")]
    stale = not os.path.exists(LIB_PATH) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if force or stale:
        subprocess.check_call(["make", "-s", "-C", CSRC, "-j4"])
    return LIB_PATH


def _preload_torch_runtime():
    # Share one HIP runtime with PyTorch: torch bundles libamdhip64.so.7 with
    # the same soname, so importing torch first makes our NEEDED entry resolve
    # to the already-loaded runtime (device pointers stay valid across both).
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch absent
        pass


def load():
    """Load (building first if stale in a dev tree) and bind libivfpq.so."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH) and os.path.isdir(CSRC):
            try:
                build()
            except Exception as e:  # pragma: no cover
                raise ImportError(f"libivfpq.so missing and build failed: {e}") from e
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"HIP extension missing: {LIB_PATH} (run __graft_entry__.build())")
        _preload_torch_runtime()
        lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return _lib


class Family:
    """The functions of one C-ABI family: ``Family("ivfpq_pq_").search`` is ``ivfpq_pq_search``.  Each is
    looked up in the loaded library at its first use and kept, so a later call costs one attribute read
    (``load()`` takes a lock)."""

    def __init__(self, prefix):
        self.prefix = prefix

    def __getattr__(self, name):  # reached only for a name that is not kept yet
        fn = self.__dict__[name] = getattr(load(), self.prefix + name)
        return fn


def check(rc: int):
    if rc != 0:
        raise RuntimeError(load().ivfpq_last_error().decode("utf-8", "replace"))
