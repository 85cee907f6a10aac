"""IndexPQ on the GPU against a numpy restatement of Faiss's IndexPQ::search.

The reference (``ref_search``): per query the M x 256 table -- ``O.ip_table`` for inner
product, ``O.tree(q_m, C_mj, 1)`` per entry for L2 (fvec_L2sqr order) -- then
``acc = 0; acc += tab[m][code[m]]`` in ascending m in float32 (pq_knn_search_with_tables'
loop) and the k best by (key, label), padded with (FLT_MAX | -FLT_MAX, -1).  Labels and
distances must be identical to it, and within 1e-4 relative of the same sums in float64.
The float64 check uses non-negative data (every term of every sum is >= 0, so there is no
cancellation and the fp32 error of a sum of d products is a few d * 2^-24 relative, well
inside 1e-4).

Quantizers are installed with ``set_trained`` from a seeded random codebook, except in
the training test.  Code ranges: a batch is split into ranges of a multiple of 2048 rows
(``kPqTileRows`` in csrc/pq_flat.h), at most 12288 / (4 k) of them (``pq_scan_plan``);
NB_RANGES = 2 * 2048 + 777 gives three ranges with a ragged last one at every (nq, k)
used here, k = 1024 included.  Each of those ranges is 2048 rows, which at k <= 64 is a
single pass of a scan workgroup (two passes of 1024 rows above): the scan loop over several
passes at k <= 64, the other table widths and blockings, the k and nb boundaries and the
candidate queue's worst case are in tests/test_gpu_indexpq_paths.py.
"""
import functools

import numpy as np
import pytest

import faiss_amd as faiss
from oracle import oracle as O

pytestmark = pytest.mark.gpu

RTOL = 1e-4
IP, L2 = faiss.METRIC_INNER_PRODUCT, faiss.METRIC_L2
FMAX = np.finfo(np.float32).max
NB_RANGES = 2 * 2048 + 777
KS = [1, 10, 64, 65, 100, 1000, 1024]


# ------------------------------------------------------------------ reference
def ref_tables(xq, cb, metric):
    if metric == IP:
        return O.ip_table(xq, cb)
    M, ksub, dsub = cb.shape
    tab = np.empty((xq.shape[0], M, ksub), np.float32)
    for q in range(xq.shape[0]):
        for m in range(M):
            qm = xq[q, m * dsub:(m + 1) * dsub]
            for j in range(ksub):
                tab[q, m, j] = O.tree(qm, cb[m, j], 1)
    return tab


def ref_sums(tab, codes):
    acc = np.zeros((tab.shape[0], codes.shape[0]), np.float32)
    for m in range(tab.shape[1]):
        acc += tab[:, m, codes[:, m]]
    return acc


def ref_topk(acc, k, metric):
    nq, nb = acc.shape
    D = np.full((nq, k), -FMAX if metric == IP else FMAX, np.float32)
    I = np.full((nq, k), -1, np.int64)
    labels = np.arange(nb)
    for q in range(nq):
        key = -acc[q] if metric == IP else acc[q]
        order = np.lexsort((labels, key))[:k]
        D[q, :len(order)] = acc[q][order]
        I[q, :len(order)] = order
    return D, I


def sums64(xq, cb, codes, metric):
    """The same sums in float64 from the float32 inputs."""
    M, _, dsub = cb.shape
    acc = np.zeros((xq.shape[0], codes.shape[0]), np.float64)
    for m in range(M):
        qm = xq[:, None, m * dsub:(m + 1) * dsub].astype(np.float64)
        c = cb[m].astype(np.float64)[None]
        t = (qm * c).sum(2) if metric == IP else ((qm - c) ** 2).sum(2)
        acc += t[:, codes[:, m]]
    return acc


def ref_encode(x, cb):
    """The oracle's encoder against one all-zero centroid (x - 0 is exact)."""
    M, _, dsub = cb.shape
    ox = O.OracleIVFPQ(M * dsub, 1, M)
    ox.set_trained(np.zeros((1, M * dsub), np.float32), cb)
    return ox.encode(x)[1]


def check(D, I, acc, k, metric, acc64=None):
    Dr, Ir = ref_topk(acc, k, metric)
    np.testing.assert_array_equal(I, Ir)
    np.testing.assert_array_equal(D, Dr)
    if acc64 is not None:
        ok = I >= 0
        want = np.take_along_axis(acc64, np.where(ok, I, 0), 1)
        np.testing.assert_allclose(D[ok], want[ok], rtol=RTOL, atol=0)


def data(seed, n, d):
    return np.random.default_rng(seed).random((n, d), dtype=np.float32)


def codebook(seed, d, M):
    return np.random.default_rng(seed).random((M, 256, d // M), dtype=np.float32)


def make_index(d, M, metric, cb, xb=None):
    ix = faiss.IndexPQ(d, M, 8, metric)
    ix.set_trained(cb)
    if xb is not None and len(xb):
        ix.add(xb)
    return ix


# --------------------------------------------------------------------- parity
D0, M0, NQ0 = 32, 8, 37


@functools.lru_cache(maxsize=None)
def parity_tables(metric):
    cb = codebook(11, D0, M0)
    xq = data(12, NQ0, D0)
    return cb, xq, ref_tables(xq, cb, metric)


@pytest.mark.parametrize("nb", [1, 63, 257, 3001, NB_RANGES])
@pytest.mark.parametrize("metric", [L2, IP], ids=["l2", "ip"])
def test_parity(metric, nb):
    cb, xq, tab = parity_tables(metric)
    xb = data(100 + nb, nb, D0)
    ix = make_index(D0, M0, metric, cb, xb)
    assert ix.ntotal == nb and ix.is_trained and ix.d == D0 and ix.metric_type == metric
    codes = ix.codes.reshape(nb, M0)
    np.testing.assert_array_equal(codes, ref_encode(xb, cb))
    acc = ref_sums(tab, codes)
    acc64 = sums64(xq, cb, codes, metric)
    for nq in (1, 5, 37):
        for k in KS:
            D, I = ix.search(xq[:nq], k)
            check(D, I, acc[:nq], k, metric, acc64[:nq])


@pytest.mark.parametrize("metric", [L2, IP], ids=["l2", "ip"])
def test_empty_index(metric):
    cb, xq, _ = parity_tables(metric)
    ix = make_index(D0, M0, metric, cb)
    D, I = ix.search(xq[:5], 10)
    assert (I == -1).all()
    assert (D == (-FMAX if metric == IP else FMAX)).all()
    import torch

    Dd, Id = ix.search_device(torch.from_numpy(xq[:5]).cuda(), 10)
    assert (Id.cpu().numpy() == -1).all() and (Dd.cpu().numpy() == D).all()


# --------------------------------------------------------- m-blocked tables
@pytest.mark.parametrize("d,metric", [(768, IP), (384, L2)], ids=["d768_ip", "d384_l2_dsub4"])
def test_m96_blocked_table(d, metric):
    M, nb, nq = 96, 5000, 5
    cb = codebook(21, d, M)
    xb = data(22, nb, d)
    xq = data(23, nq, d)
    ix = make_index(d, M, metric, cb, xb)
    codes = ix.codes.reshape(nb, M)
    np.testing.assert_array_equal(codes[:300], ref_encode(xb[:300], cb))
    acc = ref_sums(ref_tables(xq, cb, metric), codes)
    acc64 = sums64(xq, cb, codes, metric)
    for k in (10, 1000):
        D, I = ix.search(xq, k)
        check(D, I, acc, k, metric, acc64)


# ----------------------------------------------------------------------- ties
@pytest.mark.parametrize("metric", [L2, IP], ids=["l2", "ip"])
def test_ties_come_back_in_label_order(metric):
    cb, xq, tab = parity_tables(metric)
    nb = 1500
    xb = data(31, nb, D0)
    ix = make_index(D0, M0, metric, cb, np.concatenate([xb, xb]))
    codes = ix.codes.reshape(2 * nb, M0)
    np.testing.assert_array_equal(codes[:nb], codes[nb:])
    acc = ref_sums(tab[:5], codes)
    for k in (10, 100, 1000):
        D, I = ix.search(xq[:5], k)
        check(D, I, acc, k, metric)
        # every vector ties with its copy: equal distances come back lower label first
        tie = D[:, :-1] == D[:, 1:]
        assert tie.sum() >= 5 * (k // 2)
        assert (I[:, :-1][tie] < I[:, 1:][tie]).all()


# ------------------------------------------------------------------ add paths
def test_add_paths():
    import torch

    cb, xq, tab = parity_tables(L2)
    nb = 2600
    xb = data(41, nb, D0)
    want = ref_encode(xb, cb)
    one = make_index(D0, M0, L2, cb, xb)
    np.testing.assert_array_equal(one.codes.reshape(nb, M0), want)

    chunks = make_index(D0, M0, L2, cb)
    for a, b in ((0, 7), (7, 1800), (1800, nb)):  # the second add outgrows the first allocation
        chunks.add(xb[a:b])
    assert chunks.ntotal == nb
    np.testing.assert_array_equal(chunks.codes, one.codes)

    dev = make_index(D0, M0, L2, cb)
    dev.add_device(torch.from_numpy(xb).cuda())
    np.testing.assert_array_equal(dev.codes, one.codes)

    pre = make_index(D0, M0, L2, cb)
    pre.add_codes(want[:1000])
    pre.add_codes(want[1000:])
    np.testing.assert_array_equal(pre.codes, one.codes)

    D1, I1 = one.search(xq, 10)
    for ix in (chunks, dev, pre):
        D, I = ix.search(xq, 10)
        np.testing.assert_array_equal(I, I1)
        np.testing.assert_array_equal(D, D1)

    one.reset()
    assert one.ntotal == 0 and one.is_trained
    assert (one.search(xq[:2], 3)[1] == -1).all()
    one.add(xb[:500])
    assert one.ntotal == 500
    D, I = one.search(xq, 10)
    check(D, I, ref_sums(tab, want[:500]), 10, L2)

    with pytest.raises(RuntimeError):
        one.add_with_ids(xb[:2], np.arange(2))
    np.testing.assert_array_equal(one.reconstruct_n(3, 5), faiss.index.decode_pq(cb, want[3:8]))
    np.testing.assert_array_equal(one.reconstruct(4), faiss.index.decode_pq(cb, want[4:5])[0])


# ------------------------------------------------------------------- training
def test_train_matches_oracle_kmeans():
    n, d, M, niter = 4000, 32, 8, 4
    dsub = d // M
    x = faiss.datasets.synthetic_sift_like(n, d, seed=7, n_centres=50)
    ix = faiss.IndexPQ(d, M)
    assert not ix.is_trained
    ix.niter_pq = niter
    ix.seed = 99
    ix.train(x)
    assert ix.is_trained
    cb = ix.pq.centroids.reshape(M, 256, dsub)
    assert (ix.pq.M, ix.pq.nbits, ix.pq.ksub, ix.pq.dsub, ix.pq.code_size) == (M, 8, 256, dsub, M)
    for m in range(M):
        np.testing.assert_array_equal(
            cb[m], O.kmeans(np.ascontiguousarray(x[:, m * dsub:(m + 1) * dsub]), 256, niter, 99 + 1 + m))


# -------------------------------------------------------------- device search
def test_search_device_on_side_stream():
    import torch

    cb, xq, _ = parity_tables(IP)
    ix = make_index(D0, M0, IP, cb, data(51, 3001, D0))
    xd = torch.from_numpy(xq).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    for k in (10, 100):
        D, I = ix.search(xq, k)
        with torch.cuda.stream(s):
            Dd, Id = ix.search_device(xd, k, stream=s.cuda_stream)
        s.synchronize()
        np.testing.assert_array_equal(Id.cpu().numpy(), I)
        np.testing.assert_array_equal(Dd.cpu().numpy(), D)


# ------------------------------------------------ against the shipped engine
def test_matches_ivfpq_over_zero_centroid_lists():
    d, M, nb, nq, nlist = 64, 16, 6000, 9, 4
    cb = codebook(61, d, M)
    xb = data(62, nb, d)
    xq = data(63, nq, d)
    pq = make_index(d, M, IP, cb, xb)
    codes = pq.codes.reshape(nb, M)
    ivf = faiss.IndexIVFPQ(None, d, nlist, M, 8, IP)
    ivf.set_trained(np.zeros((nlist, d), np.float32), cb)
    ivf.add_preencoded(np.arange(nb, dtype=np.int64) % nlist, codes, np.arange(nb, dtype=np.int64))
    ivf.nprobe = nlist
    Iq = np.tile(np.arange(nlist, dtype=np.int64), (nq, 1))
    for k in (10, 100):
        D, I = pq.search(xq, k)
        Dv, Iv = ivf.search_preassigned(xq, k, Iq)
        np.testing.assert_array_equal(I, Iv)
        np.testing.assert_array_equal(D, Dv)


# ----------------------------------------------------------------- BEIR replay
def _beir_corpus():
    rng = np.random.default_rng(5)
    d, n = 768, 20_000
    centres = rng.standard_normal((400, d)).astype(np.float32)
    emb = (centres[rng.integers(0, 400, n)] + 0.35 * rng.standard_normal((n, d))).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    queries = (emb[rng.integers(0, n, 12)] + 0.05 * rng.standard_normal((12, d))).astype(np.float32)
    passage_ids = np.array(rng.permutation(n) + 10_000, dtype=np.int64)
    return emb, queries, passage_ids


def _beir_build_and_search(index, emb, queries, passage_ids, k=1000, buffer_size=8000):
    # FaissTrainIndex.build: train on every embedding, then FaissIndex.build's chunked adds
    index.train(emb)
    for start in range(0, len(passage_ids), buffer_size):
        index.add(emb[start:start + buffer_size])
    scores_arr, ids_arr = index.search(queries, k)  # FaissIndex.search
    mapped = passage_ids[ids_arr.reshape(-1)].reshape(queries.shape[0], -1)  # faiss_index.py:24-25
    return scores_arr, ids_arr, mapped


def test_beir_pq_faiss_search_replay():
    """PQFaissSearch.index: faiss.IndexPQ(768, 96, 8, METRIC_INNER_PRODUCT) (faiss_search.py:194)."""
    emb, queries, passage_ids = _beir_corpus()
    index = faiss.IndexPQ(768, 96, 8, faiss.METRIC_INNER_PRODUCT)
    index.niter_pq = 3
    D, I, mapped = _beir_build_and_search(index, emb, queries, passage_ids)
    cb = index.pq.centroids.reshape(96, 256, 8)
    codes = faiss.vector_to_array(index.codes).reshape(-1, 96)
    np.testing.assert_array_equal(codes[:500], ref_encode(emb[:500], cb))
    check(D, I, ref_sums(ref_tables(queries, cb, IP), codes), 1000, IP)
    assert (I >= 0).all()
    np.testing.assert_array_equal(mapped, passage_ids[I])


def test_beir_pq_faiss_search_replay_with_rotation():
    """use_rotation: IndexPreTransform(OPQMatrix(768, 96, 384), IndexPQ(384, 96, 8, IP))
    (faiss_search.py:186-192), built here through index_factory."""
    emb, queries, passage_ids = _beir_corpus()
    index = faiss.index_factory(768, "OPQ96_384,PQ96", faiss.METRIC_INNER_PRODUCT)
    assert isinstance(index, faiss.IndexPreTransform) and isinstance(index.index, faiss.IndexPQ)
    assert (index.index.d, index.index.M, index.d) == (384, 96, 768)
    opq = index.chain.at(0)
    opq.niter, opq.niter_pq_0, opq.niter_pq, opq.max_train_points = 1, 2, 1, 2048  # a short host-side OPQ fit
    index.index.niter_pq = 3
    index.nprobe = 8  # forwarded to nothing: an IndexPQ has no lists
    D, I, mapped = _beir_build_and_search(index, emb, queries, passage_ids)
    assert index.is_trained and index.ntotal == len(emb)
    cb = index.index.pq.centroids.reshape(96, 256, 4)
    codes = index.index.codes.reshape(-1, 96)
    # the stored codes are those of the transformed vectors (a prefix: the oracle's
    # transform is a scalar loop), the scan is checked on all of them
    np.testing.assert_array_equal(codes[:1500], ref_encode(O.linear_transform(emb[:1500], opq.A), cb))
    tq = O.linear_transform(queries, opq.A)
    check(D, I, ref_sums(ref_tables(tq, cb, IP), codes), 1000, IP)
    np.testing.assert_array_equal(mapped, passage_ids[I])


# --------------------------------------------------------------- save and load
@pytest.mark.parametrize("wrapped", [False, True], ids=["plain", "IxPT"])
def test_write_read_round_trip(tmp_path, wrapped):
    d, M, nb = 64, 16, 3001
    metric = IP
    rng = np.random.default_rng(71)
    xb = data(72, nb, d)
    xq = data(73, 7, d)
    if wrapped:
        opq = faiss.OPQMatrix(d, 8, 32)
        q, _ = np.linalg.qr(rng.standard_normal((d, d)))
        opq.set_matrix(q.T[:32].astype(np.float32))
        inner = faiss.IndexPQ(32, 8, 8, metric)
        inner.set_trained(codebook(74, 32, 8))
        index = faiss.IndexPreTransform(opq, inner)
    else:
        index = make_index(d, M, metric, codebook(74, d, M))
    index.add(xb)
    path = str(tmp_path / "pq.index")
    faiss.write_index(index, path)
    with open(path, "rb") as f:
        assert f.read(4) == (b"IxPT" if wrapped else b"IxPq")
    back = faiss.read_index(path)
    assert type(back) is type(index) and back.ntotal == nb and back.is_trained
    inner_a, inner_b = (index.index, back.index) if wrapped else (index, back)
    assert isinstance(inner_b, faiss.IndexPQ) and inner_b.metric_type == metric
    np.testing.assert_array_equal(inner_a.codes, inner_b.codes)
    np.testing.assert_array_equal(inner_a.pq.centroids, inner_b.pq.centroids)
    for k in (10, 100):
        D, I = index.search(xq, k)
        Db, Ib = back.search(xq, k)
        np.testing.assert_array_equal(I, Ib)
        np.testing.assert_array_equal(D, Db)
