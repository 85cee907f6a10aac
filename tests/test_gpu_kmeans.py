"""Kmeans / Clustering on the GPU against the oracle's k-means (oracle.kmeans), bit for bit.

The resident trainer (csrc/clustering.cpp, csrc/km_update.hip) assigns with the flat index's
fused scan at k = 1, orders every pass by cluster and adds each cluster's rows in ascending
row order in fp64: the order of the oracle's or_kmeans_update, so centroids are compared with
assert_array_equal.  The objective is an fp64 sum in another (fixed) order than the test's
numpy sum, so it is compared within the bound on reordering an fp64 sum of n non-negative
terms, relative n 2^-52.
"""
import numpy as np
import pytest

import faiss_amd as faiss
from faiss_amd import datasets
from oracle import oracle as O

pytestmark = pytest.mark.gpu
STEP = 15486557  # the seed step between redos
NITER = 4
SEED = 77


def clustered(n, d, seed, n_centres=20):
    return datasets.synthetic_sift_like(n, d, seed=seed, n_centres=n_centres)


def skewed(n, d, seed):
    """n - 300 rows within 1e-3 of one point, 300 rows spread out: one long chain beside
    clusters of a few rows."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, d)).astype(np.float32)
    heavy = rng.permutation(n)[:n - 300]
    x[heavy] = x[heavy[0]] + rng.uniform(-1e-3, 1e-3, size=(n - 300, d)).astype(np.float32)
    return np.ascontiguousarray(x, np.float32)


_cache = {}


def data(kind, n, d):
    key = (kind, n, d)
    if key not in _cache:
        x = skewed(n, d, 5) if kind == "skew" else clustered(n, d, 31 + d)
        x.setflags(write=False)
        _cache[key] = x
    return _cache[key]


def oracle_cent(kind, n, d, k, niter=NITER, seed=SEED, metric=O.METRIC_L2):
    key = ("o", kind, n, d, k, niter, seed, metric)
    if key not in _cache:
        c = O.kmeans(data(kind, n, d), k, niter, seed, metric=metric)
        c.setflags(write=False)
        _cache[key] = c
    return _cache[key]


L2_SHAPES = [(12, 16), (64, 37), (200, 256)]


@pytest.mark.parametrize("d,k", L2_SHAPES)
def test_l2_matches_oracle(d, k):
    x = data("clu", 3000, d)
    km = faiss.Kmeans(d, k, niter=NITER, seed=SEED)
    obj = km.train(x)
    assert km.centroids.shape == (k, d) and km.centroids.dtype == np.float32
    np.testing.assert_array_equal(km.centroids, oracle_cent("clu", 3000, d, k))
    assert isinstance(km.index, faiss.IndexFlatL2) and km.index.ntotal == k
    assert km.obj.shape == (NITER,) and km.obj.dtype == np.float64 and obj == km.obj[-1]
    assert [s["obj"] for s in km.iteration_stats] == list(km.obj)


def test_single_centroid():
    """One chain of 3000 rows (max_points_per_centroid raised: the default would subsample 256)."""
    x = data("clu", 3000, 12)
    km = faiss.Kmeans(12, 1, niter=2, seed=SEED, max_points_per_centroid=3000)
    km.train(x)
    np.testing.assert_array_equal(km.centroids, O.kmeans(x, 1, 2, SEED))


def test_one_row_per_centroid():
    x = data("clu", 300, 24)
    km = faiss.Kmeans(24, 300, niter=3, seed=SEED)
    km.train(x)
    np.testing.assert_array_equal(km.centroids, O.kmeans(x, 300, 3, SEED))


def test_fewer_rows_than_centroids_raises():
    with pytest.raises(RuntimeError, match="at least as many training points as centroids"):
        faiss.Kmeans(8, 50, niter=1).train(data("clu", 300, 8)[:40])


@pytest.mark.parametrize("rows", ["raw", "nonnegative"])
def test_spherical_matches_oracle(rows):
    d, k = 32, 24
    if rows == "raw":  # both signs, not normalised
        x = np.random.default_rng(9).normal(size=(3000, d)).astype(np.float32) * 3.0
    else:  # the rows of tests/test_gpu_ip.py's spherical training
        x = datasets.synthetic_sift_like(3000, d, seed=11, n_centres=40)
    km = faiss.Kmeans(d, k, niter=NITER, seed=SEED, spherical=True)
    km.train(x)
    np.testing.assert_array_equal(km.centroids, O.kmeans(x, k, NITER, SEED, metric=O.METRIC_INNER_PRODUCT))
    assert isinstance(km.index, faiss.IndexFlatIP)
    np.testing.assert_allclose(np.linalg.norm(km.centroids.astype(np.float64), axis=1), 1.0, atol=1e-6)


def test_empty_clusters_are_split():
    rng = np.random.default_rng(3)
    x = np.ascontiguousarray(rng.normal(size=(5, 16)).astype(np.float32)[rng.integers(0, 5, size=2000)])
    km = faiss.Kmeans(16, 8, niter=3, seed=SEED)
    km.train(x)
    assert km.iteration_stats[0]["nsplit"] > 0
    np.testing.assert_array_equal(km.centroids, O.kmeans(x, 8, 3, SEED))


def test_skewed_clusters():
    x = data("skew", 3000, 64)
    km = faiss.Kmeans(64, 32, niter=NITER, seed=SEED)
    km.train(x)
    np.testing.assert_array_equal(km.centroids, oracle_cent("skew", 3000, 64, 32))


@pytest.mark.parametrize("kind,d,k", [("clu",) + s for s in L2_SHAPES] + [("skew", 64, 32)])
def test_passes_continue_the_chains(kind, d, k):
    """Four passes (the last one ragged) give the single pass' bits and the oracle's, for host
    rows streamed in every iteration and for rows resident in HBM."""
    import torch

    x = data(kind, 3500, d)
    ref = oracle_cent(kind, 3500, d, k)
    one = faiss.Kmeans(d, k, niter=NITER, seed=SEED)
    one.train(x)
    np.testing.assert_array_equal(one.centroids, ref)
    streamed = faiss.Kmeans(d, k, niter=NITER, seed=SEED)
    streamed.set_pass_rows(1000)
    streamed.train(x)
    np.testing.assert_array_equal(streamed.centroids, ref)
    xd = torch.from_numpy(np.array(x)).cuda()
    for rows in (0, 1000):
        dev = faiss.Kmeans(d, k, niter=NITER, seed=SEED)
        dev.set_pass_rows(rows)
        dev.train_device(xd)
        np.testing.assert_array_equal(dev.centroids, ref)
    np.testing.assert_allclose(streamed.obj, one.obj, rtol=3500 * 2.0**-52, atol=0)


def test_more_than_65536_centroids():
    """One iteration: the oracle side of two (2 x 10^10 multiply-adds) was measured at 12 s on
    8 oracle threads, above the few seconds a test may take."""
    rng = np.random.default_rng(17)
    x = rng.normal(size=(70000, 4)).astype(np.float32)
    km = faiss.Kmeans(4, 66000, niter=1, seed=SEED)
    km.train(x)
    np.testing.assert_array_equal(km.centroids, O.kmeans(x, 66000, 1, SEED))


def test_objective():
    d, k, n = 64, 37, 3000
    x = data("clu", n, d)
    km = faiss.Kmeans(d, k, niter=NITER, seed=SEED)
    km.train(x)
    for t in range(NITER):
        cent = x[O.rand_perm_prefix(n, k, SEED)] if t == 0 else oracle_cent("clu", n, d, k, niter=t)
        D, _ = O.coarse_search(x, cent, 1)
        ref = float(np.sum(D.astype(np.float64)))
        print(f"obj[{t}] = {km.obj[t]!r}, reference {ref!r}")
        assert abs(km.obj[t] - ref) <= n * 2.0**-52 * ref
    again = faiss.Kmeans(d, k, niter=NITER, seed=SEED)
    again.train(x)
    assert again.obj.tobytes() == km.obj.tobytes()
    np.testing.assert_array_equal(again.centroids, km.centroids)


def test_nredo_keeps_the_best_run():
    d, k = 16, 12
    x = clustered(2000, d, 8, n_centres=30)
    singles = []
    for r in range(3):
        km = faiss.Kmeans(d, k, niter=3, seed=SEED + STEP * r)
        singles.append((km.train(x), km.centroids))
    objs = [o for o, _ in singles]
    assert len(set(objs)) == 3
    best = int(np.argmin(objs))
    km = faiss.Kmeans(d, k, niter=3, seed=SEED, nredo=3)
    assert km.train(x) == objs[best]
    np.testing.assert_array_equal(km.centroids, singles[best][1])


def test_subsampling():
    x = clustered(4000, 16, 21)
    km = faiss.Kmeans(16, 16, niter=3, seed=SEED, max_points_per_centroid=100)
    km.train(x)
    sub = np.ascontiguousarray(x[O.rand_perm_prefix(4000, 1600, SEED)])
    np.testing.assert_array_equal(km.centroids, O.kmeans(sub, 16, 3, SEED))
    import torch

    dev = faiss.Kmeans(16, 16, niter=3, seed=SEED, max_points_per_centroid=100)
    dev.train_device(torch.from_numpy(x).cuda())
    np.testing.assert_array_equal(dev.centroids, km.centroids)


def test_init_centroids():
    d, k = 64, 37
    x = data("clu", 3000, d)
    km = faiss.Kmeans(d, k, niter=NITER, seed=SEED + 5)  # (another seed: only the initial centroids decide)
    km.train(x, init_centroids=x[O.rand_perm_prefix(3000, k, SEED)])
    np.testing.assert_array_equal(km.centroids, oracle_cent("clu", 3000, d, k))


def test_unsupported_pair_is_named():
    clus = faiss.Clustering(8, 4)
    with pytest.raises(RuntimeError, match="spherical"):
        clus.train(data("clu", 300, 8), faiss.IndexFlatIP(8))


def test_train_coarse_quantizer_replay():
    """bench_gpu_1bn.py:522-542, then the centroids installed in an IndexIVFFlat."""
    d, ncent = 32, 24
    x = clustered(3000, d, 2)
    xb = clustered(5000, d, 3)
    xq = clustered(50, d, 4)
    clus = faiss.Clustering(d, ncent)
    clus.verbose = False
    clus.max_points_per_centroid = 10000000
    clus.niter = 5
    clus.seed = SEED
    index = faiss.IndexFlatL2(d)
    clus.train(x, index)
    centroids = faiss.vector_float_to_array(clus.centroids).reshape(ncent, d)
    np.testing.assert_array_equal(centroids, O.kmeans(x, ncent, 5, SEED))
    assert index.ntotal == ncent
    assert [s["nsplit"] for s in clus.iteration_stats] == [0] * 5 and len(clus.obj) == 5
    coarse = faiss.IndexFlatL2(d)
    coarse.add(centroids)
    ix = faiss.IndexIVFFlat(coarse, d, ncent, faiss.METRIC_L2)
    ix.set_trained(centroids)
    ix.add(xb)
    ix.nprobe = 4
    D, I = ix.search(xq, 10)
    ref = faiss.IndexIVFFlat(None, d, ncent, faiss.METRIC_L2)
    ref.niter_coarse, ref.seed = 5, SEED
    ref.train(x)
    ref.add(xb)
    ref.nprobe = 4
    Dr, Ir = ref.search(xq, 10)
    np.testing.assert_array_equal(I, Ir)
    np.testing.assert_array_equal(D, Dr)


def test_wav2vec_replay():
    """wav2vec_cluster_faiss.py:186-203."""
    d, n_clus = 24, 10
    x = np.array(clustered(2000, d, 6))
    faiss.normalize_L2(x)
    kmeans = faiss.Kmeans(d, n_clus, niter=5, verbose=False, spherical=True, max_points_per_centroid=x.shape[0],
                          gpu=True, nredo=3)
    kmeans.train(x)
    assert kmeans.centroids.shape == (n_clus, d)
    D, I = kmeans.assign(x)
    Dr, Ir = kmeans.index.search(x, 1)
    np.testing.assert_array_equal(D, Dr.ravel())
    np.testing.assert_array_equal(I, Ir.ravel())
    assert D.shape == (2000,) and I.shape == (2000,)


@pytest.mark.parametrize("metric", [faiss.METRIC_L2, faiss.METRIC_INNER_PRODUCT])
def test_existing_trainer_gives_the_same_centroids(metric):
    d, k = 32, 24
    x = datasets.synthetic_sift_like(3000, d, seed=11, n_centres=40)
    ix = faiss.IndexIVFFlat(None, d, k, metric)
    ix.niter_coarse, ix.seed = NITER, SEED
    ix.train(x)
    km = faiss.Kmeans(d, k, niter=NITER, seed=SEED, spherical=metric == faiss.METRIC_INNER_PRODUCT)
    km.train(x)
    np.testing.assert_array_equal(km.centroids, ix.centroids())
