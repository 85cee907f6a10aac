"""IndexBinaryFlat on the GPU against the numpy reference (tests/indexbinary_ref.py): D and I
must be identical to it in every case - the distances are small integers and ties go by label,
so there is no tolerance anywhere.

The scan cuts the codes into row segments and the queries into blocks of QB (16 up to 1024
bits, 8 above); a work item is one (segment, block).  ivfpq_bin_get_plan reports the cut, so the
cases that depend on it (segment boundaries, ties across one) read it instead of assuming it.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import faiss_amd as faiss
import indexbinary_ref as R
from faiss_amd import _lib

pytestmark = pytest.mark.gpu


def codes(seed, n, d):
    return np.random.default_rng(seed).integers(0, 256, (n, d // 8), dtype=np.uint8)


def build(xb, d):
    ix = faiss.IndexBinaryFlat(d)
    ix.add(xb)
    return ix


def check(got, want):
    D, I = got
    Dr, Ir = want
    assert D.dtype == np.int32 and I.dtype == np.int64
    np.testing.assert_array_equal(D, Dr)
    np.testing.assert_array_equal(I, Ir)


def plan(d, nb, nq, k=10):
    """(stride, query block, segments, rows per segment, queries per chunk) of a search."""
    stride, qb, sg = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rows, qc = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(_lib.load().ivfpq_bin_get_plan(d, nb, nq, k, ctypes.byref(stride), ctypes.byref(qb),
                                              ctypes.byref(sg), ctypes.byref(rows), ctypes.byref(qc)))
    return stride.value, qb.value, sg.value, rows.value, qc.value


# ------------------------------------------------------------------ base sweep
@functools.lru_cache(maxsize=None)
def base(d):
    nb, nq = 5000, 37  # 37 is a multiple of no query block; 5000 ends in a partial tile
    xb, xq = codes(1, nb, d), codes(3, nq, d)
    return build(xb, d), xq, functools.lru_cache(maxsize=None)(lambda k: R.Ref(xb).search(xq, k))


@pytest.mark.parametrize("k", [1, 10, 64, 65, 100, 1000, 1024])
@pytest.mark.parametrize("d", [8, 40, 64, 256, 768, 2048])
def test_base_sweep(d, k):
    ix, xq, ref = base(d)
    assert ix.ntotal == 5000 and ix.is_trained and ix.code_size == d // 8 and ix.metric_type == faiss.METRIC_L2
    assert plan(d, 5000, 37, k)[2] >= 2
    check(ix.search(xq, k), ref(k))


# ------------------------------------------------------------------ segments and blocks
@pytest.mark.parametrize("d", [64, 768])
def test_one_query_many_segments(d):
    xb, xq = codes(11, 20000, d), codes(13, 1, d)
    assert plan(d, 20000, 1)[2] >= 16
    ix = build(xb, d)
    for k in (10, 300):
        check(ix.search(xq, k), R.Ref(xb).search(xq, k))


@pytest.mark.parametrize("d", [64, 2048])
def test_many_blocks_few_segments(d):
    xb, xq = codes(17, 3000, d), codes(19, 300, d)
    _, qb, sg, _, qc = plan(d, 3000, 300)
    assert qc == 300 and 300 / qb > 4 and 2 <= sg <= 12
    check(build(xb, d).search(xq, 20), R.Ref(xb).search(xq, 20))


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_rows_around_a_segment_boundary(delta):
    d, nq = 128, 8
    rows = plan(d, 4000, nq)[3]
    nb = 3 * rows + delta  # one less than, equal to, one more than the third boundary
    sg = plan(d, nb, nq)[2]
    assert sg >= 2 and plan(d, nb, nq)[3] * (sg - 1) < nb
    xb, xq = codes(23, nb, d), codes(29, nq, d)
    xq[0] = xb[nb - 1]  # the last row is somebody's nearest neighbour
    check(build(xb, d).search(xq, 33), R.Ref(xb).search(xq, 33))


def test_queries_in_two_chunks_of_the_histogram_workspace():
    d, nb, nq = 2048, 40, 12500  # 12500 x 2049 x 4 bytes of histograms: past the workspace budget
    qb, sg, qc = plan(d, nb, nq)[1], plan(d, nb, nq)[2], plan(d, nb, nq)[4]
    assert sg == 1 and qc < nq <= 2 * qc and qc % qb == 0 and (nq - qc) % qb != 0
    xb, xq = codes(211, nb, d), codes(223, nq, d)
    xq[qc - 1], xq[qc], xq[-1] = xb[3], xb[4], xb[5]  # the rows on either side of the cut, and the last
    D, I = build(xb, d).search(xq, 5)
    assert D[qc - 1, 0] == 0 and I[qc - 1, 0] == 3 and I[qc, 0] == 4 and I[-1, 0] == 5
    check((D, I), R.Ref(xb).search(xq, 5))


# ------------------------------------------------------------------ ties
@pytest.mark.parametrize("k", [100, 1000])
def test_every_rank_is_a_tie(k):
    xb, xq = codes(31, 5000, 8), codes(37, 20, 8)  # 9 distinct distances over 5000 rows
    check(build(xb, 8).search(xq, k), R.Ref(xb).search(xq, k))


def test_rows_from_a_small_pool():
    rng = np.random.default_rng(41)
    pool = codes(43, 40, 96)
    xb = pool[rng.integers(0, 40, 4000)]
    xq = np.concatenate([pool[:5], codes(47, 6, 96)])
    ix = build(xb, 96)
    for k in (7, 150, 1024):
        check(ix.search(xq, k), R.Ref(xb).search(xq, k))


@pytest.mark.parametrize("k", [1, 17, 1000])
def test_all_rows_identical(k):
    xb = np.repeat(codes(53, 1, 256), 3000, 0)
    xq = np.concatenate([xb[:1], codes(59, 2, 256)])
    D, I = build(xb, 256).search(xq, k)
    np.testing.assert_array_equal(I, np.tile(np.arange(k), (3, 1)))
    check((D, I), R.Ref(xb).search(xq, k))


def test_ties_at_the_kth_distance_straddle_a_segment_boundary():
    d, nb, nq = 64, 4000, 3
    _, _, sg, rows, _ = plan(d, nb, nq)
    assert sg >= 2 and rows < nb
    rng = np.random.default_rng(61)
    xq = codes(67, nq, d)
    xb = xq[0] ^ np.uint8(0xFF)  # every row at distance 64 from query 0 ...
    xb = np.repeat(xb[None], nb, 0)
    near = xq[0].copy()
    near[0] ^= 0x07          # ... except a run at distance 3 across the first boundary
    xb[rows - 5:rows + 6] = near
    xb[rng.choice(rows - 10, 4, replace=False)] = xq[0]  # and four exact copies before it
    ix, ref = build(xb, d), R.Ref(xb)
    for k in (4, 5, 9, 10, 12, 15, 16, 40):  # the k-th result: a copy, inside the run on either side, past it
        check(ix.search(xq, k), ref.search(xq, k))


# ------------------------------------------------------------------ edges
def test_fewer_rows_than_k_is_padded():
    xb, xq = codes(71, 7, 72), codes(73, 5, 72)
    D, I = build(xb, 72).search(xq, 10)
    assert (D[:, 7:] == 2147483647).all() and (I[:, 7:] == -1).all()
    check((D, I), R.Ref(xb).search(xq, 10))


def test_empty_index():
    ix = faiss.IndexBinaryFlat(64)
    D, I = ix.search(codes(79, 3, 64), 5)
    assert D.dtype == np.int32 and I.dtype == np.int64 and ix.ntotal == 0
    assert (D == 2147483647).all() and (I == -1).all()
    assert ix.xb.size == 0


def test_k_equals_the_number_of_rows():
    xb, xq = codes(83, 700, 128), codes(89, 9, 128)
    check(build(xb, 128).search(xq, 700), R.Ref(xb).search(xq, 700))


def test_a_query_that_is_a_stored_row():
    xb = codes(97, 2500, 768)
    xq = xb[[5, 1234, 2499]]
    D, I = build(xb, 768).search(xq, 8)
    assert (D[:, 0] == 0).all() and I[:, 0].tolist() == [5, 1234, 2499]
    check((D, I), R.Ref(xb).search(xq, 8))


def test_all_zero_against_all_ones_at_2048_bits():
    xb = np.zeros((600, 256), np.uint8)
    xb[300:] = 0xFF
    xq = np.stack([np.zeros(256, np.uint8), np.full(256, 0xFF, np.uint8)])
    D, I = build(xb, 2048).search(xq, 400)
    assert (D[0, :300] == 0).all() and (D[0, 300:] == 2048).all() and (D[1, :300] == 0).all()
    check((D, I), R.Ref(xb).search(xq, 400))


# ------------------------------------------------------------------ index life cycle
def test_life_cycle():
    d = 40  # rows padded in the image: what comes back has no pad bytes
    xb, xq = codes(101, 3000, d), codes(103, 11, d)
    ref = R.Ref(xb).search(xq, 25)
    ix = faiss.IndexBinaryFlat(d)
    ix.train(xb)
    for lo, hi in ((0, 1), (1, 1100), (1100, 3000)):  # three uneven chunks, across the first allocation
        ix.add(xb[lo:hi])
    assert ix.ntotal == 3000
    check(ix.search(xq, 25), ref)
    check(build(xb, d).search(xq, 25), ref)
    np.testing.assert_array_equal(faiss.vector_to_array(ix.xb), xb.reshape(-1))
    np.testing.assert_array_equal(ix.reconstruct(1099), xb[1099])
    np.testing.assert_array_equal(ix.reconstruct_n(1020, 100), xb[1020:1120])
    with pytest.raises(RuntimeError):
        ix.reconstruct_n(2990, 11)
    with pytest.raises(RuntimeError, match="add_with_ids"):
        ix.add_with_ids(xb[:2], np.arange(2))
    with pytest.raises(RuntimeError, match="uint8"):
        ix.add(xb[:2].astype(np.float32))
    ix.use_heap, ix.query_batch_size = False, 7  # plain attributes, no effect
    check(ix.search(xq, 25), ref)
    ix.reset()
    assert ix.ntotal == 0 and (ix.search(xq, 3)[1] == -1).all()
    ix.add(xb[:500])
    check(ix.search(xq, 25), R.Ref(xb[:500]).search(xq, 25))


def test_growth_across_reallocations():
    d = 256
    xb, xq = codes(107, 9000, d), codes(109, 6, d)
    ix = faiss.IndexBinaryFlat(d)
    for lo in range(0, 9000, 900):  # 1024 rows first, then doubled three times
        ix.add(xb[lo:lo + 900])
    check(ix.search(xq, 40), R.Ref(xb).search(xq, 40))
    np.testing.assert_array_equal(ix.reconstruct_n(0, 9000), xb)


# ------------------------------------------------------------------ device path
def test_device_path():
    d = 768
    xb, xq = codes(113, 4000, d), codes(127, 21, d)
    ix = build(xb, d)
    want = ix.search(xq, 30)
    check(want, R.Ref(xb).search(xq, 30))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        tq = torch.from_numpy(xq).cuda()
        D, I = ix.search_device(tq, 30, stream=s.cuda_stream)
    s.synchronize()
    assert D.dtype == torch.int32 and I.dtype == torch.int64 and D.is_cuda and D.shape == (21, 30)
    check((D.cpu().numpy(), I.cpu().numpy()), want)
    Dp = torch.empty((21, 30), dtype=torch.int32, device="cuda")
    Ip = torch.empty((21, 30), dtype=torch.int64, device="cuda")
    D2, I2 = ix.search_device(tq, 30, D=Dp, I=Ip)
    torch.cuda.synchronize()
    assert D2 is Dp and I2 is Ip
    check((Dp.cpu().numpy(), Ip.cpu().numpy()), want)
    with pytest.raises(RuntimeError):
        ix.search_device(tq.to(torch.int32), 30)
    with pytest.raises(RuntimeError):
        ix.search_device(tq, 30, D=torch.empty((21, 30), dtype=torch.float32, device="cuda"))
    iy = faiss.IndexBinaryFlat(d)
    iy.add_device(torch.from_numpy(xb[:1500]).cuda())
    iy.add_device(torch.from_numpy(xb[1500:]).cuda())
    assert iy.ntotal == 4000
    check(iy.search(xq, 30), want)
    np.testing.assert_array_equal(iy.reconstruct_n(0, 4000), xb)


# ------------------------------------------------------------------ file
def test_write_read_index_binary(tmp_path):
    d = 72
    xb, xq = codes(131, 2000, d), codes(137, 5, d)
    ix = faiss.index_binary_factory(d, "BFlat")
    assert isinstance(ix, faiss.IndexBinaryFlat)
    ix.add(xb)
    p = str(tmp_path / "bin.index")
    faiss.write_index_binary(ix, p)
    iy = faiss.read_index_binary(p)
    assert isinstance(iy, faiss.IndexBinaryFlat) and iy.d == d and iy.ntotal == 2000
    check(iy.search(xq, 12), ix.search(xq, 12))
    check(iy.search(xq, 12), R.Ref(xb).search(xq, 12))
    with pytest.raises(RuntimeError, match="IBxF"):
        faiss.read_index(p)
    f = str(tmp_path / "flat.index")
    sq = faiss.IndexScalarQuantizer(8, faiss.ScalarQuantizer.QT_fp16)
    faiss.write_index(sq, f)
    with pytest.raises(RuntimeError, match="IxSQ"):
        faiss.read_index_binary(f)
    with pytest.raises(RuntimeError):
        faiss.write_index_binary(sq, f)


# ------------------------------------------------------------------ independent cross-check
def test_against_index_flat_ip_over_the_sign_expansion():
    d, nb, nq, k = 64, 3000, 20, 50
    xb, xq = codes(139, nb, d), codes(149, nq, d)
    D, I = build(xb, d).search(xq, k)
    expand = lambda c: np.unpackbits(c, axis=1).astype(np.float32) * 2 - 1  # noqa: E731
    flat = faiss.IndexFlatIP(d)
    flat.add(expand(xb))
    Dip, Iip = flat.search(expand(xq), k)
    np.testing.assert_array_equal(Dip, (d - 2 * D).astype(np.float32))  # ip = d - 2 * hamming, exact in fp32
    for q in range(nq):
        below = D[q] < D[q, -1]  # strictly inside the k-th distance: the sets agree whatever the tie rule
        assert set(I[q][below]) == set(Iip[q][below])


# ------------------------------------------------------------------ caller replay
class BinaryIndexReplay:
    """beir faiss_index.py FaissBinaryIndex.build / .search, restated: Hamming candidates from the
    binary index, then a re-rank of the candidates by float query x unpacked +-1 passage."""

    def __init__(self, index_cls, passage_ids, emb, chunk=2500):
        self.ids = np.asarray(passage_ids)
        bits = np.packbits(np.where(emb > 0, 1, 0), axis=1).reshape(emb.shape[0], -1)
        self.index = index_cls(emb.shape[1])
        for lo in range(0, len(bits), chunk):
            self.index.add(bits[lo:lo + chunk])
        self.bits = bits

    def search(self, q, k, binary_k=1000, rerank=True):
        bin_q = np.packbits(np.where(q > 0, 1, 0), axis=1).reshape(q.shape[0], -1)
        if not rerank:
            D, I = self.index.search(bin_q, k)
            return D, self.ids[I]
        _, cand = self.index.search(bin_q, binary_k)
        pe = np.unpackbits(self.bits[cand.reshape(-1)], axis=1).reshape(q.shape[0], binary_k, -1)
        pe = pe.astype(np.float32) * 2 - 1
        scores = np.einsum("ijk,ik->ij", pe, q)
        order = np.argsort(-scores, axis=1, kind="stable")[:, :k]
        return np.take_along_axis(scores, order, 1), self.ids[np.take_along_axis(cand, order, 1)]


class RefBinaryIndex:
    def __init__(self, d):
        self.rows = []

    def add(self, x):
        self.rows.append(x)

    def search(self, x, k):
        return R.Ref(np.concatenate(self.rows)).search(x, k)


def test_beir_binary_search_replay():
    rng = np.random.default_rng(151)
    emb = rng.standard_normal((6000, 96)).astype(np.float32)
    q = rng.standard_normal((12, 96)).astype(np.float32)
    ids = np.arange(6000) + 100000
    got = BinaryIndexReplay(lambda d: faiss.IndexBinaryFlat(d), ids, emb)
    want = BinaryIndexReplay(RefBinaryIndex, ids, emb)
    assert got.index.ntotal == 6000 and got.index.d == 96
    for rerank in (True, False):
        S, P = got.search(q, 10, rerank=rerank)
        Sr, Pr = want.search(q, 10, rerank=rerank)
        np.testing.assert_array_equal(P, Pr)
        np.testing.assert_array_equal(S, Sr)
