"""Kmeans / Clustering without a GPU: the exported names, the C-ABI's argument checks (made
before any device call), the small host functions and the rejected options."""
import ctypes

import numpy as np
import pytest

import faiss_amd as faiss
from faiss_amd import _lib, clustering

CLUS = ["ivfpq_clus_create", "ivfpq_clus_free", "ivfpq_clus_train", "ivfpq_clus_train_device",
        "ivfpq_clus_get_centroids", "ivfpq_clus_get_stats", "ivfpq_clus_set_pass_rows",
        "ivfpq_clus_rand_perm_prefix"]


def last_error(rc):
    assert rc != 0
    return _lib.load().ivfpq_last_error().decode()


def test_exported_and_bound():
    for name in ("Kmeans", "Clustering", "normalize_L2", "vector_float_to_array"):
        assert hasattr(faiss, name)
    assert faiss.vector_float_to_array is faiss.vector_to_array
    L = _lib.load()
    for name in CLUS:
        assert name in _lib.SIGNATURES and getattr(L, name).argtypes is not None


@pytest.mark.parametrize("d,k,metric,spherical,word", [
    (0, 4, faiss.METRIC_L2, 0, "d must be"),
    (-3, 4, faiss.METRIC_L2, 0, "d must be"),
    (8, 0, faiss.METRIC_L2, 0, "k must be"),
    (8, 4, 7, 0, "metric"),
    (8, 4, faiss.METRIC_L2, 1, "L2 with spherical = true"),
    (8, 4, faiss.METRIC_INNER_PRODUCT, 0, "inner product with spherical = false"),
])
def test_create_rejects_before_any_device_call(d, k, metric, spherical, word):
    h = _lib.c_handle()
    # device 1 << 20 does not exist: a device call would fail with another message
    msg = last_error(_lib.load().ivfpq_clus_create(d, k, metric, spherical, 1 << 20, ctypes.byref(h)))
    assert word in msg and not h.value


def test_train_arguments_and_null_handle():
    L = _lib.load()
    x = np.zeros((4, 2), np.float32)
    xp = x.ctypes.data_as(_lib.c_f32p)
    assert "niter" in last_error(L.ivfpq_clus_train(None, 4, xp, -1, 1, 0, None))
    assert "nredo" in last_error(L.ivfpq_clus_train(None, 4, xp, 1, 0, 0, None))
    assert "empty training set" in last_error(L.ivfpq_clus_train(None, 0, xp, 1, 1, 0, None))
    assert "nredo" in last_error(L.ivfpq_clus_train_device(None, 4, None, 1, 0, 0, None, None))
    assert "null index handle" in last_error(L.ivfpq_clus_train(None, 4, xp, 1, 1, 0, None))
    assert "null index handle" in last_error(L.ivfpq_clus_train_device(None, 4, 1 << 12, 1, 1, 0, None, None))
    out = np.zeros(8, np.float32)
    assert "null index handle" in last_error(L.ivfpq_clus_get_centroids(None, out.ctypes.data_as(_lib.c_f32p)))
    assert "null index handle" in last_error(L.ivfpq_clus_get_stats(None, None, None, None))
    assert "null index handle" in last_error(L.ivfpq_clus_set_pass_rows(None, 5))
    assert L.ivfpq_clus_free(None) == 0


def test_rand_perm_prefix_is_the_oracles():
    from oracle import oracle as O

    for n, k, seed in [(10, 10, 1), (1000, 37, 1234), (5, 0, 3)]:
        np.testing.assert_array_equal(clustering.rand_perm_prefix(n, k, seed), O.rand_perm_prefix(n, k, seed))
    with pytest.raises(RuntimeError, match="k <= n"):
        clustering.rand_perm_prefix(3, 4, 0)


def test_normalize_L2():
    rng = np.random.default_rng(0)
    x = (rng.normal(size=(200, 33)) * 10.0 ** rng.integers(-3, 4, size=(200, 1))).astype(np.float32)
    x[7] = 0.0
    x[150] = 0.0
    keep = x
    before = x.copy()
    assert faiss.normalize_L2(x) is None and x is keep  # in place
    norms = np.sqrt((x.astype(np.float64) ** 2).sum(1))
    live = np.ones(200, bool)
    live[[7, 150]] = False
    assert np.all(np.abs(norms[live] - 1.0) <= 4 * np.finfo(np.float32).eps)
    assert not x[7].any() and not x[150].any()
    # renorm_rows' arithmetic, row by row
    for i in (0, 1, 99):
        nr = np.float32(0)
        for v in before[i]:
            nr = np.float32(nr + np.float32(v * v))
        inv = np.float32(1.0 / np.float64(np.sqrt(nr)))
        np.testing.assert_array_equal(x[i], before[i] * inv)
    with pytest.raises(RuntimeError, match="float32"):
        faiss.normalize_L2(np.ones((3, 4), np.float64))
    with pytest.raises(RuntimeError, match="contiguous"):
        faiss.normalize_L2(np.ones((4, 6), np.float32)[:, ::2])
    with pytest.raises(RuntimeError, match="matrix"):
        faiss.normalize_L2(np.ones(4, np.float32))


def test_vector_float_to_array():
    v = np.arange(6, dtype=np.float32)
    a = faiss.vector_float_to_array(v)
    np.testing.assert_array_equal(a, v)
    a[0] = 9
    assert v[0] == 0


def test_rejected_options_name_themselves():
    x = np.zeros((10, 4), np.float32)
    with pytest.raises(RuntimeError, match="weights"):
        faiss.Kmeans(4, 2).train(x, weights=np.ones(10, np.float32))
    with pytest.raises(RuntimeError, match="int_centroids"):
        faiss.Kmeans(4, 2, int_centroids=True)
    with pytest.raises(RuntimeError, match="frozen_centroids"):
        faiss.Kmeans(4, 2, frozen_centroids=True)
    with pytest.raises(RuntimeError, match="nope"):
        faiss.Kmeans(4, 2, nope=1)
    clus = faiss.Clustering(4, 2)
    clus.int_centroids = True
    with pytest.raises(RuntimeError, match="int_centroids"):
        clus.train(x, faiss.IndexFlatL2(4))
    clus = faiss.Clustering(4, 2)
    clus.frozen_centroids = True
    with pytest.raises(RuntimeError, match="frozen_centroids"):
        clus.train(x, faiss.IndexFlatL2(4))
    with pytest.raises(RuntimeError, match="weights"):
        faiss.Clustering(4, 2).train(x, faiss.IndexFlatL2(4), weights=np.ones(10, np.float32))
    with pytest.raises(RuntimeError, match="niter"):
        faiss.Kmeans(4, 2, niter=-1).train(x)
    with pytest.raises(RuntimeError, match="nredo"):
        faiss.Kmeans(4, 2, nredo=0).train(x)
    km = faiss.Kmeans(4, 2, gpu=True, update_index=True)  # accepted, no effect
    assert km.niter == 25 and km.nredo == 1 and km.seed == 1234
    assert km.max_points_per_centroid == 256 and km.min_points_per_centroid == 39
    with pytest.raises(RuntimeError, match="train before"):
        km.assign(x)


def test_clustering_attributes_and_non_empty_index():
    clus = faiss.Clustering(4, 2)
    for name, v in [("niter", 25), ("nredo", 1), ("verbose", False), ("spherical", False), ("seed", 1234),
                    ("min_points_per_centroid", 39), ("max_points_per_centroid", 256)]:
        assert getattr(clus, name) == v
    index = faiss.IndexFlatL2(4)
    index.add(np.ones((3, 4), np.float32))
    with pytest.raises(RuntimeError, match="empty"):
        clus.train(np.zeros((10, 4), np.float32), index)
