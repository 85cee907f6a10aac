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

# name -> (restype, argtypes); mirrors include/ivfpq.h one to one, plus the
# test hooks of include/ivfpq_test.h (used only by tests/).
SIGNATURES = {
    "ivfpq_last_error": (ctypes.c_char_p, []),
    "ivfpq_device_count": (ctypes.c_int, []),
    "ivfpq_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                    ctypes.c_int, ctypes.POINTER(c_handle)]),
    "ivfpq_free": (ctypes.c_int, [c_handle]),
    "ivfpq_train": (ctypes.c_int, [c_handle, ctypes.c_int64, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_uint64]),
    "ivfpq_add": (ctypes.c_int, [c_handle, ctypes.c_int64, c_f32p, c_i64p]),
    "ivfpq_precompute_tables_device": (ctypes.c_int, [c_handle, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                                      ctypes.POINTER(ctypes.c_uint64)]),
    "ivfpq_search_preassigned_tables_device": (ctypes.c_int, [c_handle, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int,
                                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                              ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
    "ivfpq_set_inflight": (ctypes.c_int, [c_handle, ctypes.c_int]),
    "ivfpq_get_inflight": (ctypes.c_int, [c_handle]),
    "ivfpq_overlap_built": (ctypes.c_int, []),
    "ivfpq_get_error_count": (ctypes.c_int, [c_handle, c_i64p]),
    "ivfpq_get_repair_stats": (ctypes.c_int, [c_handle, c_i64p, c_i64p]),
    "ivfpq_get_repair_log": (ctypes.c_int, [c_handle, ctypes.POINTER(ctypes.c_uint32), ctypes.c_int,
                                            ctypes.POINTER(ctypes.c_int)]),
    "ivfpq_set_fault_injection": (ctypes.c_int, [c_handle, ctypes.c_int]),
    "ivfpq_debug_workspace": (ctypes.c_int, [c_handle, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64,
                                             c_i64p]),
    "ivfpq_debug_seed_tau": (ctypes.c_int, [c_handle, ctypes.c_int64, ctypes.c_void_p]),
    "ivfpq_add_device": (ctypes.c_int, [c_handle, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p]),
    "ivfpq_add_preencoded": (ctypes.c_int, [c_handle, ctypes.c_int64, c_i64p, c_u8p, c_i64p]),
    "ivfpq_reset": (ctypes.c_int, [c_handle]),
    "ivfpq_set_nprobe": (ctypes.c_int, [c_handle, ctypes.c_int]),
    "ivfpq_get_nprobe": (ctypes.c_int, [c_handle]),
    "ivfpq_set_list_range": (ctypes.c_int, [c_handle, ctypes.c_int, ctypes.c_int]),
    "ivfpq_search": (ctypes.c_int, [c_handle, ctypes.c_int64, c_f32p, ctypes.c_int, c_f32p, c_i64p]),
    "ivfpq_search_preassigned": (ctypes.c_int, [c_handle, ctypes.c_int64, c_f32p, ctypes.c_int, c_i64p, c_f32p,
                                                c_f32p, c_i64p]),
    "ivfpq_search_device": (ctypes.c_int, [c_handle, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "ivfpq_search_preassigned_device": (ctypes.c_int, [c_handle, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int,
                                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                       ctypes.c_void_p, ctypes.c_void_p]),
    "ivfpq_serve_request": (ctypes.c_int, [c_handle, c_u8p, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_int, c_u8p, ctypes.c_int64, c_i64p]),
    "ivfpq_coarse_device": (ctypes.c_int, [c_handle, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p]),
    "ivfpq_coarse_tables_device": (ctypes.c_int, [c_handle, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.POINTER(ctypes.c_uint64)]),
    "ivfpq_merge_topk_device": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p]),
    "ivfpq_linear_transform_device": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                     ctypes.c_void_p]),
    # PCA training moments (PCAMatrix.train), their chunk setting and plan
    "ivfpq_pca_moments_device": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_void_p]),
    "ivfpq_pca_set_chunk_rows": (ctypes.c_int, [ctypes.c_int64]),
    "ivfpq_pca_get_plan": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int), c_i64p,
                                          ctypes.POINTER(ctypes.c_int)]),
    "ivfpq_set_timing": (ctypes.c_int, [c_handle, ctypes.c_int]),
    "ivfpq_get_timing": (ctypes.c_int, [c_handle, ctypes.POINTER(ctypes.c_double), c_i64p]),
    "ivfpq_ntotal": (ctypes.c_int64, [c_handle]),
    "ivfpq_is_trained": (ctypes.c_int, [c_handle]),
    "ivfpq_get_dims": (ctypes.c_int, [c_handle] + [ctypes.POINTER(ctypes.c_int)] * 5),
    "ivfpq_get_centroids": (ctypes.c_int, [c_handle, c_f32p]),
    "ivfpq_get_codebook": (ctypes.c_int, [c_handle, c_f32p]),
    "ivfpq_set_trained": (ctypes.c_int, [c_handle, c_f32p, c_f32p]),
    "ivfpq_get_list_sizes": (ctypes.c_int, [c_handle, c_i64p]),
    "ivfpq_get_list": (ctypes.c_int, [c_handle, ctypes.c_int, c_u8p, c_i64p]),
    "ivfpq_get_precomputed_table": (ctypes.c_int, [c_handle, c_f32p]),
    "ivfpq_save": (ctypes.c_int, [c_handle, ctypes.c_char_p]),
    "ivfpq_load": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(c_handle)]),
    "ivfpq_flat_search": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int64, c_f32p, ctypes.c_int64,
                                         c_f32p, ctypes.c_int, ctypes.c_int, c_f32p, c_i64p]),
    # flat product quantizer (IndexPQ)
    "ivfpq_pq_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.POINTER(c_handle)]),
    "ivfpq_pq_free": (ctypes.c_int, [c_handle]),
    "ivfpq_pq_train": (ctypes.c_int, [c_handle, ctypes.c_int64, c_f32p, ctypes.c_int, ctypes.c_uint64]),
    "ivfpq_pq_set_trained": (ctypes.c_int, [c_handle, c_f32p]),
    "ivfpq_pq_add": (ctypes.c_int, [c_handle, ctypes.c_int64, c_f32p]),
    "ivfpq_pq_add_device": (ctypes.c_int, [c_handle, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "ivfpq_pq_add_codes": (ctypes.c_int, [c_handle, ctypes.c_int64, c_u8p]),
    "ivfpq_pq_reset": (ctypes.c_int, [c_handle]),
    "ivfpq_pq_search": (ctypes.c_int, [c_handle, ctypes.c_int64, c_f32p, ctypes.c_int, c_f32p, c_i64p]),
    "ivfpq_pq_search_device": (ctypes.c_int, [c_handle, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int,
                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "ivfpq_pq_ntotal": (ctypes.c_int64, [c_handle]),
    "ivfpq_pq_is_trained": (ctypes.c_int, [c_handle]),
    "ivfpq_pq_get_dims": (ctypes.c_int, [c_handle] + [ctypes.POINTER(ctypes.c_int)] * 4),
    "ivfpq_pq_get_codebook": (ctypes.c_int, [c_handle, c_f32p]),
    "ivfpq_pq_get_codes": (ctypes.c_int, [c_handle, ctypes.c_int64, ctypes.c_int64, c_u8p]),
    "ivfpq_pq_debug_plan": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int64,
                                           ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), c_i64p,
                                           ctypes.POINTER(ctypes.c_int), c_i64p]),
    # IVF over raw vectors (IndexIVFFlat)
    "ivfpq_ivfflat_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.POINTER(c_handle)]),
    "ivfpq_ivfflat_free": (ctypes.c_int, [c_handle]),
    "ivfpq_ivfflat_train": (ctypes.c_int, [c_handle, ctypes.c_int64, c_f32p, ctypes.c_int, ctypes.c_uint64]),
    "ivfpq_ivfflat_set_trained": (ctypes.c_int, [c_handle, c_f32p]),
    "ivfpq_ivfflat_add": (ctypes.c_int, [c_handle, ctypes.c_int64, c_f32p, c_i64p]),
    "ivfpq_ivfflat_add_device": (ctypes.c_int, [c_handle, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_void_p]),
    "ivfpq_ivfflat_reset": (ctypes.c_int, [c_handle]),
    "ivfpq_ivfflat_set_nprobe": (ctypes.c_int, [c_handle, ctypes.c_int]),
    "ivfpq_ivfflat_get_nprobe": (ctypes.c_int, [c_handle]),
    "ivfpq_ivfflat_search": (ctypes.c_int, [c_handle, ctypes.c_int64, c_f32p, ctypes.c_int, c_f32p, c_i64p]),
    "ivfpq_ivfflat_search_preassigned": (ctypes.c_int, [c_handle, ctypes.c_int64, c_f32p, ctypes.c_int, c_i64p,
                                                        c_f32p, c_f32p, c_i64p]),
    "ivfpq_ivfflat_search_device": (ctypes.c_int, [c_handle, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int,
                                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "ivfpq_ivfflat_search_preassigned_device": (ctypes.c_int, [c_handle, ctypes.c_int64, ctypes.c_void_p,
                                                               ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "ivfpq_ivfflat_ntotal": (ctypes.c_int64, [c_handle]),
    "ivfpq_ivfflat_is_trained": (ctypes.c_int, [c_handle]),
    "ivfpq_ivfflat_get_dims": (ctypes.c_int, [c_handle] + [ctypes.POINTER(ctypes.c_int)] * 3),
    "ivfpq_ivfflat_get_centroids": (ctypes.c_int, [c_handle, c_f32p]),
    "ivfpq_ivfflat_get_list_sizes": (ctypes.c_int, [c_handle, c_i64p]),
    "ivfpq_ivfflat_get_list": (ctypes.c_int, [c_handle, ctypes.c_int, c_f32p, c_i64p]),
    # flat scalar quantizer (IndexScalarQuantizer)
    "ivfpq_sq_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.POINTER(c_handle)]),
    "ivfpq_sq_free": (ctypes.c_int, [c_handle]),
    "ivfpq_sq_train": (ctypes.c_int, [c_handle, ctypes.c_int64, c_f32p]),
    "ivfpq_sq_set_trained": (ctypes.c_int, [c_handle, c_f32p, ctypes.c_int64]),
    "ivfpq_sq_add": (ctypes.c_int, [c_handle, ctypes.c_int64, c_f32p]),
    "ivfpq_sq_add_device": (ctypes.c_int, [c_handle, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "ivfpq_sq_add_codes": (ctypes.c_int, [c_handle, ctypes.c_int64, c_u8p]),
    "ivfpq_sq_reset": (ctypes.c_int, [c_handle]),
    "ivfpq_sq_search": (ctypes.c_int, [c_handle, ctypes.c_int64, c_f32p, ctypes.c_int, c_f32p, c_i64p]),
    "ivfpq_sq_search_device": (ctypes.c_int, [c_handle, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int,
                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "ivfpq_sq_ntotal": (ctypes.c_int64, [c_handle]),
    "ivfpq_sq_is_trained": (ctypes.c_int, [c_handle]),
    "ivfpq_sq_get_dims": (ctypes.c_int, [c_handle] + [ctypes.POINTER(ctypes.c_int)] * 4),
    "ivfpq_sq_get_trained": (ctypes.c_int, [c_handle, c_f32p, c_i64p]),
    "ivfpq_sq_get_codes": (ctypes.c_int, [c_handle, ctypes.c_int64, ctypes.c_int64, c_u8p]),
    "ivfpq_sq_encode": (ctypes.c_int, [c_handle, ctypes.c_int64, c_f32p, c_u8p]),
    "ivfpq_sq_decode": (ctypes.c_int, [c_handle, ctypes.c_int64, c_u8p, c_f32p]),
    # IVF over scalar-quantizer codes (IndexIVFScalarQuantizer)
    "ivfpq_ivfsq_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, ctypes.POINTER(c_handle)]),
    "ivfpq_ivfsq_free": (ctypes.c_int, [c_handle]),
    "ivfpq_ivfsq_train": (ctypes.c_int, [c_handle, ctypes.c_int64, c_f32p, ctypes.c_int, ctypes.c_uint64]),
    "ivfpq_ivfsq_set_trained": (ctypes.c_int, [c_handle, c_f32p, c_f32p, ctypes.c_int64]),
    "ivfpq_ivfsq_add": (ctypes.c_int, [c_handle, ctypes.c_int64, c_f32p, c_i64p]),
    "ivfpq_ivfsq_add_device": (ctypes.c_int, [c_handle, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_void_p]),
    "ivfpq_ivfsq_add_codes": (ctypes.c_int, [c_handle, ctypes.c_int64, c_i64p, c_u8p, c_i64p]),
    "ivfpq_ivfsq_reset": (ctypes.c_int, [c_handle]),
    "ivfpq_ivfsq_set_nprobe": (ctypes.c_int, [c_handle, ctypes.c_int]),
    "ivfpq_ivfsq_get_nprobe": (ctypes.c_int, [c_handle]),
    "ivfpq_ivfsq_search": (ctypes.c_int, [c_handle, ctypes.c_int64, c_f32p, ctypes.c_int, c_f32p, c_i64p]),
    "ivfpq_ivfsq_search_preassigned": (ctypes.c_int, [c_handle, ctypes.c_int64, c_f32p, ctypes.c_int, c_i64p,
                                                      c_f32p, c_f32p, c_i64p]),
    "ivfpq_ivfsq_search_device": (ctypes.c_int, [c_handle, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int,
                                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "ivfpq_ivfsq_search_preassigned_device": (ctypes.c_int, [c_handle, ctypes.c_int64, ctypes.c_void_p,
                                                             ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "ivfpq_ivfsq_ntotal": (ctypes.c_int64, [c_handle]),
    "ivfpq_ivfsq_is_trained": (ctypes.c_int, [c_handle]),
    "ivfpq_ivfsq_get_dims": (ctypes.c_int, [c_handle] + [ctypes.POINTER(ctypes.c_int)] * 6),
    "ivfpq_ivfsq_get_centroids": (ctypes.c_int, [c_handle, c_f32p]),
    "ivfpq_ivfsq_get_trained": (ctypes.c_int, [c_handle, c_f32p, c_i64p]),
    "ivfpq_ivfsq_get_list_sizes": (ctypes.c_int, [c_handle, c_i64p]),
    "ivfpq_ivfsq_get_list": (ctypes.c_int, [c_handle, ctypes.c_int, c_u8p, c_i64p]),
    # flat binary codes (IndexBinaryFlat)
    "ivfpq_bin_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(c_handle)]),
    "ivfpq_bin_free": (ctypes.c_int, [c_handle]),
    "ivfpq_bin_reset": (ctypes.c_int, [c_handle]),
    "ivfpq_bin_add": (ctypes.c_int, [c_handle, ctypes.c_int64, c_u8p]),
    "ivfpq_bin_add_device": (ctypes.c_int, [c_handle, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "ivfpq_bin_search": (ctypes.c_int, [c_handle, ctypes.c_int64, c_u8p, ctypes.c_int, c_i32p, c_i64p]),
    "ivfpq_bin_search_device": (ctypes.c_int, [c_handle, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "ivfpq_bin_ntotal": (ctypes.c_int64, [c_handle]),
    "ivfpq_bin_get_dims": (ctypes.c_int, [c_handle] + [ctypes.POINTER(ctypes.c_int)] * 2),
    "ivfpq_bin_get_codes": (ctypes.c_int, [c_handle, ctypes.c_int64, ctypes.c_int64, c_u8p]),
    "ivfpq_bin_get_plan": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                                          ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                          ctypes.POINTER(ctypes.c_int), c_i64p, c_i64p]),
    # flat fp32 rows (IndexFlat / IndexFlatL2 / IndexFlatIP)
    "ivfpq_flat_index_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(c_handle)]),
    "ivfpq_flat_index_free": (ctypes.c_int, [c_handle]),
    "ivfpq_flat_index_reset": (ctypes.c_int, [c_handle]),
    "ivfpq_flat_index_add": (ctypes.c_int, [c_handle, ctypes.c_int64, c_f32p]),
    "ivfpq_flat_index_add_device": (ctypes.c_int, [c_handle, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "ivfpq_flat_index_search": (ctypes.c_int, [c_handle, ctypes.c_int64, c_f32p, ctypes.c_int, c_f32p, c_i64p]),
    "ivfpq_flat_index_search_device": (ctypes.c_int, [c_handle, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int,
                                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "ivfpq_flat_index_ntotal": (ctypes.c_int64, [c_handle]),
    "ivfpq_flat_index_get_dims": (ctypes.c_int, [c_handle] + [ctypes.POINTER(ctypes.c_int)] * 2),
    "ivfpq_flat_index_get_rows": (ctypes.c_int, [c_handle, ctypes.c_int64, ctypes.c_int64, c_f32p]),
    "ivfpq_flat_index_get_stats": (ctypes.c_int, [c_handle, c_i64p, c_i64p, c_i64p]),
    "ivfpq_flat_index_set_range_rows": (ctypes.c_int, [c_handle, ctypes.c_int64]),
    "ivfpq_flat_index_get_plan": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int64,
                                                 ctypes.POINTER(ctypes.c_int), c_i64p, ctypes.POINTER(ctypes.c_int),
                                                 ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                                 ctypes.POINTER(ctypes.c_int), c_i64p]),
    # stand-alone k-means (Kmeans / Clustering)
    "ivfpq_clus_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.POINTER(c_handle)]),
    "ivfpq_clus_free": (ctypes.c_int, [c_handle]),
    "ivfpq_clus_train": (ctypes.c_int, [c_handle, ctypes.c_int64, c_f32p, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_uint64, c_f32p]),
    "ivfpq_clus_train_device": (ctypes.c_int, [c_handle, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_uint64, c_f32p, ctypes.c_void_p]),
    "ivfpq_clus_get_centroids": (ctypes.c_int, [c_handle, c_f32p]),
    "ivfpq_clus_get_stats": (ctypes.c_int, [c_handle, ctypes.POINTER(ctypes.c_int),
                                            ctypes.POINTER(ctypes.c_double), c_i64p]),
    "ivfpq_clus_set_pass_rows": (ctypes.c_int, [c_handle, ctypes.c_int64]),
    "ivfpq_clus_rand_perm_prefix": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, ctypes.c_uint64, c_i64p]),
    # how the host cuts a batch into chunks (host arithmetic; faiss_amd.index.*_split)
    "ivfpq_ivf_get_plan": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, ctypes.POINTER(ctypes.c_int),
                                          ctypes.POINTER(ctypes.c_int)]),
    "ivfpq_ivf_get_query_chunk": (ctypes.c_int, [ctypes.c_int64] + [ctypes.c_int] * 7 + [c_i64p]),
    "ivfpq_ivf_get_pass_rows": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_i64p]),
    "ivfpq_sq_get_plan": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                         ctypes.POINTER(ctypes.c_int), c_i64p]),
    "ivfpq_get_query_chunk": (ctypes.c_int, [ctypes.c_int64] + [ctypes.c_int] * 6 + [c_i64p]),
    "ivfpq_host_get_pass_rows": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, c_i64p]),
    "ivfpq_flat_search_get_query_chunk": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, c_i64p]),
    "ivfpq_kmeans_get_assign_rows": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, c_i64p]),
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


def check(rc: int):
    if rc != 0:
        raise RuntimeError(load().ivfpq_last_error().decode("utf-8", "replace"))
