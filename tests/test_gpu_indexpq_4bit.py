"""IndexPQ with 4-bit codes (PQ<M>x4) against the numpy restatement of Faiss's IndexPQ::search
that tests/test_gpu_indexpq.py uses, with 16 columns and an explicit unpack of the code bytes
(``lo = b & 15``, ``hi = b >> 4``, interleaved: sub-quantizer 2i is the low nibble of byte i).

Labels and distances must be identical to the float32 restatement, and within 1e-4 relative of
the float64 sums on non-negative data (the argument is in that file's docstring).  Quantizers
are installed with ``set_trained`` from seeded random [M][16][dsub] codebooks, except in the
training test.  The CPU-side checks at the end need no GPU.

The encode check is specified as: the stored bytes of the first 200 rows equal the packed first-argmin
codes of ``O.tree`` distances.  This file departs from that wording: the 200 rows' distances come from
``indexpq_ref.tree_np``, not from 200 x M x 16 single ``O.tree`` calls (8 s per case at M = 256).  ``tree_np`` is ``O.tree`` on whole arrays, asserted equal to it bit
for bit in tests/test_indexpq_cpu.py, and the first four rows of every case are also computed with
``O.tree`` itself.
"""
import ctypes
import functools

import numpy as np
import pytest

import faiss_amd as faiss
from faiss_amd import _lib
from faiss_amd import index as fidx
from indexpq_ref import tree_np
from oracle import oracle as O
from test_gpu_indexpq import KS, NB_RANGES, check, data, ref_sums, ref_tables, sums64

gpu = pytest.mark.gpu
IP, L2 = faiss.METRIC_INNER_PRODUCT, faiss.METRIC_L2
SHAPES = [(64, 32), (192, 96), (512, 256)]  # one 16-byte piece per row, three, two table blocks


def codebook(seed, d, M):
    return np.random.default_rng(seed).random((M, 16, d // M), dtype=np.float32)


def unpack(rows):
    return np.stack([rows & 15, rows >> 4], axis=2).reshape(rows.shape[0], -1)


def pack(codes):
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).astype(np.uint8)


def ref_encode(x, cb):
    """First argmin over the 16 centroids of O.tree distances, packed.  The distances of all rows come
    from indexpq_ref.tree_np (O.tree on whole arrays, bit for bit: tests/test_indexpq_cpu.py), those of
    the first rows from O.tree itself."""
    M, _, dsub = cb.shape
    codes = np.stack([np.argmin(tree_np(x[:, None, m * dsub:(m + 1) * dsub], cb[m][None], 1), axis=1)
                      for m in range(M)], axis=1).astype(np.uint8)
    for i in range(min(4, x.shape[0])):
        for m in range(M):
            dis = np.array([O.tree(x[i, m * dsub:(m + 1) * dsub], cb[m, j], 1) for j in range(16)], np.float32)
            assert codes[i, m] == np.argmin(dis)
    return pack(codes)


def make_index(d, M, metric, cb, xb=None):
    ix = faiss.IndexPQ(d, M, 4, metric)
    ix.set_trained(cb)
    if xb is not None:
        ix.add(xb)
    return ix


@functools.lru_cache(maxsize=None)
def tables(d, M, metric):
    cb = codebook(11, d, M)
    xq = data(12, 37, d)
    return cb, xq, ref_tables(xq, cb, metric)


@gpu
@pytest.mark.parametrize("nb", [1, 63, NB_RANGES])
@pytest.mark.parametrize("metric", [L2, IP], ids=["l2", "ip"])
@pytest.mark.parametrize("d,M", SHAPES)
def test_parity(d, M, metric, nb):
    cb, xq, tab = tables(d, M, metric)
    xb = data(100 + nb, nb, d)
    ix = make_index(d, M, metric, cb, xb)
    assert ix.ntotal == nb and ix.code_size == M // 2
    rows = ix.codes.reshape(nb, M // 2)
    np.testing.assert_array_equal(rows[:200], ref_encode(xb[:200], cb))
    codes = unpack(rows)
    acc = ref_sums(tab, codes)
    acc64 = sums64(xq, cb, codes, metric)
    for nq in (1, 5, 37):
        for k in KS:
            D, I = ix.search(xq[:nq], k)
            check(D, I, acc[:nq], k, metric, acc64[:nq])


@gpu
@pytest.mark.parametrize("metric", [L2, IP], ids=["l2", "ip"])
def test_ties_come_back_in_label_order(metric):
    d, M, nb = 64, 32, 1500
    cb, xq, tab = tables(d, M, metric)
    xb = data(31, nb, d)
    ix = make_index(d, M, metric, cb, np.concatenate([xb, xb]))
    codes = unpack(ix.codes.reshape(2 * nb, M // 2))
    np.testing.assert_array_equal(codes[:nb], codes[nb:])
    acc = ref_sums(tab[:5], codes)
    for k in (10, 100, 1000):
        D, I = ix.search(xq[:5], k)
        check(D, I, acc, k, metric)
        tie = D[:, :-1] == D[:, 1:]
        assert tie.sum() >= 5 * (k // 2)
        assert (I[:, :-1][tie] < I[:, 1:][tie]).all()


@gpu
def test_add_paths():
    import torch

    d, M, nb = 64, 32, 2600
    cb, xq, _ = tables(d, M, L2)
    xb = data(41, nb, d)
    one = make_index(d, M, L2, cb, xb)
    want = one.codes.reshape(nb, M // 2)
    np.testing.assert_array_equal(want[:100], ref_encode(xb[:100], cb))

    chunks = make_index(d, M, L2, cb)
    for a, b in ((0, 7), (7, 1800), (1800, nb)):  # the second add outgrows the first allocation
        chunks.add(xb[a:b])
    dev = make_index(d, M, L2, cb)
    dev.add_device(torch.from_numpy(xb).cuda())
    pre = make_index(d, M, L2, cb)
    pre.add_codes(pack(unpack(want[:1000])))  # hand-packed bytes
    pre.add_codes(want[1000:])
    D1, I1 = one.search(xq, 10)
    for ix in (chunks, dev, pre):
        assert ix.ntotal == nb
        np.testing.assert_array_equal(ix.codes, one.codes)
        D, I = ix.search(xq, 10)
        np.testing.assert_array_equal(I, I1)
        np.testing.assert_array_equal(D, D1)
    codes = unpack(want[3:8])
    dec = np.concatenate([cb[m][codes[:, m]] for m in range(M)], axis=1)
    np.testing.assert_array_equal(one.reconstruct_n(3, 5), dec)
    np.testing.assert_array_equal(one.reconstruct(4), dec[1])
    one.reset()
    assert one.ntotal == 0 and one.is_trained and (one.search(xq[:2], 3)[1] == -1).all()


@gpu
def test_train_matches_oracle_kmeans():
    n, d, M, niter = 2000, 64, 32, 4
    dsub = d // M
    x = faiss.datasets.synthetic_sift_like(n, d, seed=7, n_centres=50)
    ix = faiss.IndexPQ(d, M, 4)
    ix.niter_pq = niter
    ix.seed = 99
    ix.train(x)
    assert ix.is_trained and (ix.pq.nbits, ix.pq.ksub, ix.pq.code_size) == (4, 16, 16)
    cb = ix.pq.centroids.reshape(M, 16, dsub)
    for m in range(M):
        np.testing.assert_array_equal(
            cb[m], O.kmeans(np.ascontiguousarray(x[:, m * dsub:(m + 1) * dsub]), 16, niter, 99 + 1 + m))


@gpu
@pytest.mark.parametrize("wrapped", [False, True], ids=["plain", "IxPT"])
def test_write_read_round_trip(tmp_path, wrapped):
    d, M, nb = 64, 32, 3001
    xb, xq = data(72, nb, d), data(73, 7, d)
    if wrapped:
        index = faiss.index_factory(d, "OPQ32,PQ32x4")
        q, _ = np.linalg.qr(np.random.default_rng(71).standard_normal((d, d)))
        index.chain.at(0).set_matrix(q.astype(np.float32))
        index.index.set_trained(codebook(74, d, M))
    else:
        index = faiss.index_factory(d, "PQ32x4")
        index.set_trained(codebook(74, d, M))
    index.add(xb)
    path = str(tmp_path / "pq4.index")
    faiss.write_index(index, path)
    with open(path, "rb") as f:
        assert f.read(4) == (b"IxPT" if wrapped else b"IxPq")
    back = faiss.read_index(path)
    assert type(back) is type(index) and back.ntotal == nb and back.is_trained
    a, b = (index.index, back.index) if wrapped else (index, back)
    assert isinstance(b, faiss.IndexPQ) and (b.nbits, b.code_size, b.pq.code_size) == (4, M // 2, M // 2)
    np.testing.assert_array_equal(a.codes, b.codes)
    np.testing.assert_array_equal(a.pq.centroids, b.pq.centroids)
    for k in (10, 100):
        D, I = index.search(xq, k)
        Db, Ib = back.search(xq, k)
        np.testing.assert_array_equal(I, Ib)
        np.testing.assert_array_equal(D, Db)


# ------------------------------------------------------------------ without a GPU
def test_create_checks_nbits_before_any_device_call():
    lib = _lib.load()

    def create(d, M, nbits):
        h = ctypes.c_void_p()
        rc = lib.ivfpq_pq_create(d, M, nbits, L2, 0, ctypes.byref(h))
        msg = lib.ivfpq_last_error().decode() if rc else ""
        if h.value:
            lib.ivfpq_pq_free(h)
        return rc, msg

    # a supported 4-bit shape gets exactly as far as the 8-bit one (to the device, where there is one)
    assert create(64, 32, 4) == create(64, 32, 8)
    for args in ((128, 48, 4), (128, 32, 5)):
        rc, msg = create(*args)
        assert rc != 0 and "nbits" in msg
    assert fidx.parse_pq_factory("PQ32x4") == (32, 4)
    assert fidx.parse_pq_factory("OPQ32_64,PQ32x4") == (32, 4, 32, 64)


# (M, k, nq, nb) -> (G, ranges, rows, S, query chunk), by hand from pq_scan_plan_group with G = 4:
#   chunk = min(nq, 256 MiB / (64 M bytes), 4096), groups = ceil(min(nq, chunk) / 4), tiles = ceil(nb / 2048),
#   r = min(ceil(1024 / groups), max(1, 12288 // (4 k)), tiles), rows = ceil(tiles / r) * 2048, S = 4 ceil(nb / rows)
@pytest.mark.parametrize("args,want", [
    ((32, 10, 5, 4873), (4, 3, 2048, 12, 5)),          # 2 groups: min(512, 307, 3 tiles)
    ((256, 10, 5000, 4873), (4, 1, 6144, 4, 4096)),    # 16 KiB of table per query: 16384 > the cap of 4096 (M KiB: 1024)
    ((96, 1000, 1, 18432), (4, 3, 6144, 12, 1)),       # 12288 // 4000 = 3, 9 tiles
])
def test_4bit_plan_values(args, want):
    lib = _lib.load()
    G, ranges, S = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rows, chunk = ctypes.c_int64(), ctypes.c_int64()
    M, k, nq, nb = args
    _lib.check(lib.ivfpq_pq_get_plan(M, 4, k, nq, nb, ctypes.byref(G), ctypes.byref(ranges), ctypes.byref(rows),
                                     ctypes.byref(S), ctypes.byref(chunk)))
    assert (G.value, ranges.value, rows.value, S.value, chunk.value) == want
    assert lib.ivfpq_pq_get_plan(48, 4, 10, 5, 100, None, None, None, None, None) != 0
    assert "nbits" in lib.ivfpq_last_error().decode()
