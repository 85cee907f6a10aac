"""The Python surface of faiss_amd.index, pinned name by name: the index classes share private bases
(faiss_amd/_handle.py, _IVFIndex), and a shared base must not leak ``nprobe`` into IndexPQ or
``codebook`` into IndexIVFFlat, nor may a class take its methods from an unrelated one by assignment.
Needs neither a GPU nor a device: nothing here creates a library handle."""
import inspect
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import faiss_amd as faiss
from faiss_amd import index as fidx

CLASS_SURFACE = {  # sorted(public names of dir(cls)) at the commit before the shared bases
    "IndexFlat": [  # 15
        "add", "add_device", "add_with_ids", "capacity", "is_trained", "ntotal", "reconstruct", "reconstruct_n",
        "reset", "search", "search_device", "set_range_rows", "train", "uploaded_rows", "xb"],
    "IndexFlatL2": [  # 16
        "add", "add_device", "add_with_ids", "capacity", "is_trained", "metric_type", "ntotal", "reconstruct",
        "reconstruct_n", "reset", "search", "search_device", "set_range_rows", "train", "uploaded_rows", "xb"],
    "IndexFlatIP": [  # 16
        "add", "add_device", "add_with_ids", "capacity", "is_trained", "metric_type", "ntotal", "reconstruct",
        "reconstruct_n", "reset", "search", "search_device", "set_range_rows", "train", "uploaded_rows", "xb"],
    "IndexIVFPQ": [  # 34
        "STAGES", "add", "add_device", "add_preencoded", "add_with_ids", "by_residual", "centroids",
        "coarse_device", "coarse_tables_device", "code_size", "codebook", "error_count", "get_timing", "inflight",
        "is_trained", "nprobe", "ntotal", "polysemous_ht", "precompute_tables_device", "precomputed_table",
        "repair_log", "repair_stats", "reset", "search", "search_device", "search_preassigned",
        "search_preassigned_device", "serve_request", "set_fault_injection", "set_list_range", "set_timing",
        "set_trained", "train", "use_precomputed_table"],
    "IndexPQ": [  # 17
        "add", "add_codes", "add_device", "add_with_ids", "code_size", "codebook", "codes", "is_trained", "ntotal",
        "polysemous_ht", "reconstruct", "reconstruct_n", "reset", "search", "search_device", "set_trained", "train"],
    "IndexIVFFlat": [  # 15
        "add", "add_device", "add_with_ids", "centroids", "code_size", "is_trained", "nprobe", "ntotal", "reset",
        "search", "search_device", "search_preassigned", "search_preassigned_device", "set_trained", "train"],
    "IndexScalarQuantizer": [  # 17
        "add", "add_codes", "add_device", "add_with_ids", "codes", "is_trained", "ntotal", "reconstruct",
        "reconstruct_n", "reset", "sa_code_size", "sa_decode", "sa_encode", "search", "search_device",
        "set_trained", "train"],
    "IndexIVFScalarQuantizer": [  # 16
        "add", "add_codes", "add_device", "add_with_ids", "centroids", "code_size", "is_trained", "nprobe",
        "ntotal", "reset", "search", "search_device", "search_preassigned", "search_preassigned_device",
        "set_trained", "train"],
    "IndexBinaryFlat": [  # 12
        "add", "add_device", "add_with_ids", "is_trained", "ntotal", "reconstruct", "reconstruct_n", "reset",
        "search", "search_device", "train", "xb"],
}

INDEX_MODULE = [
    "IndexBinaryFlat", "IndexFlat", "IndexFlatIP", "IndexFlatL2", "IndexIVFFlat", "IndexIVFPQ",
    "IndexIVFScalarQuantizer", "IndexPQ", "IndexScalarQuantizer", "MAX_K", "METRIC_INNER_PRODUCT", "METRIC_L2",
    "ParameterSpace", "ScalarQuantizer", "annotations", "ctypes", "decode_pq", "downcast_index", "extract_index_ivf",
    "faiss_io", "flat_search_plan", "flat_search_query_chunk", "get_num_gpus", "host_pass_rows",
    "index_binary_factory", "index_factory", "ivf_pass_rows", "ivf_search_split", "ivfpq_query_chunk",
    "kmeans_assign_rows", "merge_topk_device", "np", "overlap_built", "parse_binary_factory", "parse_factory",
    "parse_ivfflat_factory", "parse_ivfsq_factory", "parse_pca_front", "parse_pq_factory", "parse_sq_factory", "re",
    "read_index", "read_index_binary", "sq_search_plan", "swig_ptr", "vector_to_array", "write_index",
    "write_index_binary"]
PACKAGE = [
    "Clustering", "IndexBinaryFlat", "IndexFlat", "IndexFlatIP", "IndexFlatL2", "IndexIVFFlat", "IndexIVFPQ",
    "IndexIVFScalarQuantizer", "IndexPQ", "IndexPreTransform", "IndexScalarQuantizer", "Kmeans", "LinearTransform",
    "MAX_K", "METRIC_INNER_PRODUCT", "METRIC_L2", "OPQMatrix", "PCAMatrix", "ParameterSpace", "ScalarQuantizer",
    "clustering", "contrib", "datasets", "downcast_VectorTransform", "downcast_index", "extract_index_ivf", "faiss_io",
    "get_num_gpus", "index_binary_factory", "index_factory", "index", "ivf_tools", "merge_topk_device", "normalize_L2",
    "overlap_built", "read_VectorTransform", "read_index", "read_index_binary", "swig_ptr", "transform",
    "vector_float_to_array", "vector_to_array", "write_VectorTransform", "write_index", "write_index_binary"]


def public(names):
    return sorted(n for n in names if not n.startswith("_"))


@pytest.mark.parametrize("name", sorted(CLASS_SURFACE))
def test_class_surface(name):
    assert public(dir(getattr(fidx, name))) == CLASS_SURFACE[name]


def test_module_surfaces():
    """In a fresh interpreter: a package also shows the submodules that an earlier test happened to import."""
    code = ("import json, faiss_amd, faiss_amd.index as i; "
            "print(json.dumps([[n for n in dir(m) if not n.startswith('_')] for m in (i, faiss_amd)]))")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    index_names, package_names = json.loads(subprocess.check_output([sys.executable, "-c", code], env=env))
    assert len(INDEX_MODULE) == 48
    assert sorted(index_names) == INDEX_MODULE
    assert sorted(package_names) == sorted(PACKAGE)
    assert public(dir(fidx)) == INDEX_MODULE


def test_subclass_relations():
    assert issubclass(faiss.IndexIVFScalarQuantizer, faiss.IndexIVFFlat)
    assert issubclass(faiss.IndexFlatIP, faiss.IndexFlatL2)
    assert issubclass(faiss.IndexFlatL2, faiss.IndexFlat)
    for a, b in [(faiss.IndexPQ, faiss.IndexIVFPQ), (faiss.IndexIVFFlat, faiss.IndexIVFPQ),
                 (faiss.IndexScalarQuantizer, faiss.IndexIVFPQ), (faiss.IndexBinaryFlat, faiss.IndexIVFPQ),
                 (faiss.IndexFlat, faiss.IndexIVFPQ), (faiss.IndexIVFPQ, faiss.IndexIVFFlat)]:
        assert not issubclass(a, b), (a, b)


def non_tensors():
    import torch

    x = np.zeros((2, 8), np.float32)
    return [x, torch.from_numpy(x), x.tolist()]


@pytest.mark.parametrize("cls", [faiss.IndexFlat, faiss.IndexFlatL2, faiss.IndexFlatIP])
def test_indexflat_device_entry_points_reject_what_is_not_a_cuda_tensor(cls):
    ix = cls(8)
    ix.add(np.ones((3, 8), np.float32))
    for bad in non_tensors():
        with pytest.raises(RuntimeError, match="x must be a CUDA tensor"):
            ix.search_device(bad, 1)
        with pytest.raises(RuntimeError, match="x must be a CUDA tensor"):
            ix.add_device(bad)
    assert ix._h is None and ix.ntotal == 3  # rejected before the device image would be made
    assert public(vars(faiss.IndexFlatL2(8))) == ["d", "device", "metric_type", "verbose"]


def test_indexflat_k_message():
    ix = faiss.IndexFlatL2(8)
    for k in (0, 1025):
        with pytest.raises(RuntimeError, match=rf"k must be in \[1, 1024\], got {k}"):
            ix.search(np.zeros((2, 8), np.float32), k)
    assert ix._h is None


def functions_of(cls):
    """Every plain function a class body can hold: methods, and those inside property,
    staticmethod and classmethod objects."""
    for name, v in vars(cls).items():
        if isinstance(v, property):
            cand = [v.fget, v.fset, v.fdel]
        elif isinstance(v, (staticmethod, classmethod)):
            cand = [v.__func__]
        else:
            cand = [v]
        for f in cand:
            if inspect.isfunction(f):
                yield name, f


def test_nothing_borrowed():
    classes = [c for c in vars(fidx).values() if inspect.isclass(c) and c.__module__.startswith("faiss_amd")]
    assert {c.__name__ for c in classes} >= set(CLASS_SURFACE) | {"_InvertedLists", "_FlatInvertedLists",
                                                                  "_CodeInvertedLists", "_ProductQuantizer"}
    seen = 0
    for cls in classes:
        for name, f in functions_of(cls):
            assert f.__qualname__.startswith(cls.__qualname__ + "."), \
                f"{cls.__name__}.{name} is {f.__qualname__}, defined in another class"
            seen += 1
    assert seen > 100  # (the walk does find the methods)
