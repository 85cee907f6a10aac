"""IndexScalarQuantizer on the GPU against the scalar quantizer restated in numpy
(tests/indexsq_ref.py): codes, reconstructions, labels and distances must be identical to it,
and on the random-data cases the distances within 1e-4 relative of the same sums over the
decoded vectors in float64.  The float64 check needs sums without cancellation, as in
tests/test_gpu_ivfflat.py: for L2 every term is a square; for inner product the data are
uniform [0, 1), so that vmin >= 0 and every decoded 8-bit value is >= 0.  Each of the eight
accumulators adds d / 8 such terms, so the fp32 sum is within (d / 8 + 4) * 2^-24 relative
of the exact one: 1.6e-5 at d = 2048, inside 1e-4.

The scan cuts the codes into row ranges of RANGE_ROWS rows, each giving four sorted partial
lists (one per wave) per query; k <= 64, k <= 256 and k <= 1024 are three kernels.
"""
import functools

import numpy as np
import pytest

import faiss_amd as faiss
import indexsq_ref as R

pytestmark = pytest.mark.gpu

RTOL = 1e-4
IP, L2 = faiss.METRIC_INNER_PRODUCT, faiss.METRIC_L2
METRICS = [pytest.param(IP, id="ip"), pytest.param(L2, id="l2")]
QTYPES = [pytest.param(R.QT_FP16, id="fp16"), pytest.param(R.QT_8BIT, id="8bit"),
          pytest.param(R.QT_8BIT_UNIFORM, id="8bit_uniform")]
QTYPES_8 = QTYPES[1:]
G = R.RANGE_ROWS


def data(seed, n, d, metric):
    """Seeded vectors: uniform [0, 1) for inner product (non-negative), normal for L2."""
    rng = np.random.default_rng(seed)
    return (rng.random((n, d)) if metric == IP else rng.standard_normal((n, d))).astype(np.float32)


def build(xb, qtype, metric):
    ix = faiss.IndexScalarQuantizer(xb.shape[1], qtype, metric)
    ix.train(xb)
    ix.add(xb)
    return ix


def check(got, want, ref=None, xq=None):
    D, I = got
    Dr, Ir = want
    np.testing.assert_array_equal(I, Ir)
    np.testing.assert_array_equal(D, Dr)
    if ref is not None:  # against the float64 sums, where a result exists
        d64 = ref.dist64(xq)
        for q in range(len(I)):
            ok = I[q] >= 0
            np.testing.assert_allclose(D[q][ok], d64[q, I[q][ok]], rtol=RTOL, atol=0)


# ------------------------------------------------------------------ base sweep
@functools.lru_cache(maxsize=None)
def base(qtype, metric):
    d, nb, nq = 32, 5000, 37  # crosses a row range and ends in a partial tile; nq is a multiple of neither G
    xb, xq = data(1, nb, d, metric), data(3, nq, d, metric)
    return build(xb, qtype, metric), R.Ref(xb, qtype, metric), xq


@pytest.mark.parametrize("k", [1, 10, 64, 65, 100, 1024])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("qtype", QTYPES)
def test_base_sweep(qtype, metric, k):
    ix, ref, xq = base(qtype, metric)
    assert ix.ntotal == 5000 and ix.is_trained and ix.code_size == R.code_size(qtype, 32) == ix.sa_code_size()
    check(ix.search(xq, k), ref.search(xq, k), ref, xq)


# ------------------------------------------------- every phase of the reduction
@pytest.mark.parametrize("d,nb", [(4, 1500), (12, 1500), (200, 1500), (2048, 300)],
                         ids=["d4-remainder", "d12-8+4", "d200-chunks", "d2048"])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("qtype", QTYPES)
def test_reduction_phases(qtype, metric, d, nb):
    xb, xq = data(11, nb, d, metric), data(13, 9, d, metric)
    ix, ref = build(xb, qtype, metric), R.Ref(xb, qtype, metric)
    for k in (10, 100):
        check(ix.search(xq, k), ref.search(xq, k), ref, xq)


# ------------------------------------------------------------------ exact ties
@pytest.mark.parametrize("metric", METRICS)
def test_fp16_exact_ties_are_ordered_by_label(metric):
    rng = np.random.default_rng(21)
    xb = rng.integers(0, 4, (4000, 8)).astype(np.float32)
    xq = rng.integers(0, 4, (9, 8)).astype(np.float32)
    ix, ref = build(xb, R.QT_FP16, metric), R.Ref(xb, R.QT_FP16, metric)
    np.testing.assert_array_equal(ref.dec, xb)  # small integers are halves
    want = ref.search(xq, 100)
    assert max(len(np.unique(row)) for row in want[0]) < 60  # nearly every rank is decided by label
    check(ix.search(xq, 100), want)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("qtype", QTYPES_8)
def test_8bit_exact_ties_are_ordered_by_label(qtype, metric):
    rng = np.random.default_rng(22)
    pool = data(23, 40, 16, metric)
    xb = pool[rng.integers(0, 40, 4000)]
    xq = data(24, 9, 16, metric)
    ix, ref = build(xb, qtype, metric), R.Ref(xb, qtype, metric)
    want = ref.search(xq, 100)
    assert max(len(np.unique(row)) for row in want[0]) < 60
    check(ix.search(xq, 100), want)


# ------------------------------------------------------------ several row ranges
@functools.lru_cache(maxsize=None)
def ranges(qtype, metric):
    d, nb = 16, 3 * G + 5
    xb, xq = data(31, nb, d, metric), data(32, 6, d, metric)
    return build(xb, qtype, metric), R.Ref(xb, qtype, metric), xq


@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("qtype", QTYPES)
def test_several_row_ranges(qtype, metric, k):
    ix, ref, xq = ranges(qtype, metric)
    check(ix.search(xq, k), ref.search(xq, k), ref, xq)


# ----------------------------------------------------------------------- edges
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("qtype", QTYPES)
def test_edge_shapes(qtype, metric):
    d = 8
    xb, xq = data(51, 40, d, metric), data(52, 3, d, metric)
    pad = -R.FMAX if metric == IP else R.FMAX
    ix = faiss.IndexScalarQuantizer(d, qtype, metric)
    assert ix.is_trained == (qtype == R.QT_FP16)
    ix.train(xb)
    assert ix.is_trained and ix.ntotal == 0
    D, I = ix.search(xq, 5)  # an empty index
    assert (I == -1).all() and (D == pad).all()
    trained = R.train(xb, qtype)
    ix.add(xb[:1])  # one vector
    check(ix.search(xq, 1), R.Ref(xb[:1], qtype, metric, trained).search(xq, 1))
    D, I = ix.search(xq, 3)
    assert (I[:, 0] == 0).all() and (I[:, 1:] == -1).all() and (D[:, 1:] == pad).all()
    ix.add(xb[1:])  # fewer vectors than k: padded
    ref = R.Ref(xb, qtype, metric, trained)
    want = ref.search(xq, 64)
    assert (want[1][:, 40:] == -1).all() and (want[1][:, :40] >= 0).all()
    check(ix.search(xq, 64), want, ref, xq)
    check(ix.search(xq, 100), ref.search(xq, 100))
    check(ix.search(xq[:1], 10), ref.search(xq[:1], 10))  # a single query
    with pytest.raises(RuntimeError):
        ix.search(xq, 0)
    with pytest.raises(RuntimeError):
        ix.search(xq, 1025)
    with pytest.raises(RuntimeError):
        ix.add_with_ids(xb, np.arange(40))


# ----------------------------------------------------------- encode and decode
def special_inputs(qtype, metric, d=12):
    """Training rows and rows to encode: a constant dimension, values outside the trained
    range, and for fp16 a half subnormal and -0."""
    xt = data(61, 500, d, metric)
    xt[:, 3] = np.float32(0.625)  # a constant dimension: vdiff = 0
    x = data(62, 300, d, metric)
    x[:, 3] = np.float32(0.625)
    x[0] = xt.min() - np.float32(3.0)  # below every vmin: code 0
    x[1] = xt.max() + np.float32(3.0)  # above every maximum: code 255
    x[2, :4] = [3e-6, -0.0, -3e-6, 6.1e-5]
    return xt, x


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("qtype", QTYPES)
def test_encode_decode_and_training_match_the_reference(qtype, metric):
    d = 12
    xt, x = special_inputs(qtype, metric, d)
    ix = faiss.IndexScalarQuantizer(d, qtype, metric)
    ix.train(xt)
    trained = R.train(xt, qtype)
    assert ix.sq.trained.dtype == np.float32 and ix.sq.trained.tobytes() == trained.tobytes()  # numpy's min / max
    assert (ix.sq.qtype, ix.sq.d, ix.sq.code_size) == (qtype, d, R.code_size(qtype, d))
    want = R.encode(x, qtype, trained)
    codes = ix.sa_encode(x)
    assert codes.dtype == np.uint8 and codes.shape == want.shape
    np.testing.assert_array_equal(codes, want)
    if qtype == R.QT_FP16:
        h = codes.view(np.float16)
        assert h[2, 0] != 0 and abs(float(h[2, 0])) < 6.1e-5  # a half subnormal is kept
        assert h[2, 1] == 0 and np.signbit(h[2, 1])  # and so is -0
    else:
        assert (codes[0] == 0).all() and (codes[1][np.arange(d) != 3] == 255).all()
        if qtype == R.QT_8BIT:
            assert (codes[:, 3] == 0).all()  # the constant dimension
    dec = ix.sa_decode(codes)
    assert dec.dtype == np.float32 and dec.tobytes() == R.decode(want, qtype, trained, d).tobytes()
    if qtype == R.QT_8BIT:
        assert (dec[:, 3] == np.float32(0.625)).all()
    ix.add(x)
    np.testing.assert_array_equal(ix.codes, want.reshape(-1))
    assert ix.reconstruct_n(0, len(x)).tobytes() == dec.tobytes()
    assert ix.reconstruct_n(7, 20).tobytes() == dec[7:27].tobytes()
    assert ix.reconstruct(5).tobytes() == dec[5].tobytes()
    # set_trained followed by add gives the same codes as train followed by add
    other = faiss.IndexScalarQuantizer(d, qtype, metric)
    other.set_trained(trained)
    assert other.is_trained and other.sq.trained.tobytes() == trained.tobytes()
    other.add(x)
    np.testing.assert_array_equal(other.codes, ix.codes)
    with pytest.raises(RuntimeError):
        other.set_trained(np.zeros(5, np.float32))


# ------------------------------------------------------------------------ adds
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("qtype", QTYPES)
def test_add_paths_build_the_same_codes(qtype, metric):
    import torch

    ix, ref, _ = base(qtype, metric)
    d, xb = 32, data(1, 5000, 32, metric)
    np.testing.assert_array_equal(ix.codes, ref.codes.reshape(-1))

    def fresh():
        o = faiss.IndexScalarQuantizer(d, qtype, metric)
        o.set_trained(ref.trained)
        return o
    parts = fresh()
    for sl in np.array_split(np.arange(5000), 5):  # geometric growth of the image
        parts.add(xb[sl])
    dev = fresh()
    tx = torch.from_numpy(xb).cuda()
    dev.add_device(tx[:2000].contiguous())
    dev.add_device(tx[2000:].contiguous())
    pre = fresh()
    pre.add_codes(pre.sa_encode(xb))
    for o in (parts, dev, pre):
        assert o.ntotal == 5000
        np.testing.assert_array_equal(o.codes, ix.codes)
    # reset drops the codes and keeps the trained state
    parts.reset()
    assert parts.ntotal == 0 and parts.is_trained and parts.sq.trained.tobytes() == ref.trained.tobytes()
    assert (parts.search(xb[:2], 3)[1] == -1).all()
    parts.add(xb[:100])
    np.testing.assert_array_equal(parts.codes, ref.codes[:100].reshape(-1))


# ------------------------------------------------- equivalence with IVF1,Flat
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("qtype", QTYPES)
def test_equals_ivf1_flat_over_the_decoded_vectors(qtype, metric):
    ix, ref, xq = base(qtype, metric)
    flat = faiss.index_factory(32, "IVF1,Flat", metric)
    flat.set_trained(np.zeros((1, 32), np.float32))
    flat.add(ix.sa_decode(ix.codes))
    for k in (10, 100):
        check(ix.search(xq, k), flat.search(xq, k))


# ---------------------------------------------------------- device entry points
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("qtype", QTYPES)
def test_device_entry_points_on_a_side_stream(qtype, metric):
    import torch

    ix, ref, xq = base(qtype, metric)
    want = ref.search(xq, 10)
    tx = torch.from_numpy(xq).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        D, I = ix.search_device(tx, 10)
    D2, I2 = ix.search_device(tx, 10)  # torch's current stream: ordered after the side stream's call
    Dp = torch.empty((len(xq), 10), dtype=torch.float32, device="cuda")
    Ip = torch.empty((len(xq), 10), dtype=torch.int64, device="cuda")
    assert ix.search_device(tx, 10, Dp, Ip)[0] is Dp
    side.synchronize()
    torch.cuda.synchronize()
    for d_, i_ in ((D, I), (D2, I2), (Dp, Ip)):
        check((d_.cpu().numpy(), i_.cpu().numpy()), want)
    with pytest.raises(RuntimeError):
        ix.search_device(tx.double(), 10)
    with pytest.raises(RuntimeError):
        ix.add_device(tx.double())


# ------------------------------------------------------------- file round trip
@pytest.mark.parametrize("wrapped", [False, True], ids=["plain", "IxPT"])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("qtype", QTYPES)
def test_write_read_index_round_trip(qtype, metric, wrapped, tmp_path):
    d, nb = 32, 3001
    xb, xq = data(71, nb, d, metric), data(73, 7, d, metric)
    if wrapped:
        lt = faiss.LinearTransform(d, 16)
        q, _ = np.linalg.qr(np.random.default_rng(74).standard_normal((d, d)))
        lt.set_matrix(np.abs(q.T[:16]).astype(np.float32))
        index = faiss.IndexPreTransform(lt, faiss.IndexScalarQuantizer(16, qtype, metric))
    else:
        index = faiss.IndexScalarQuantizer(d, qtype, metric)
    index.train(xb)
    index.add(xb)
    path = str(tmp_path / "sq.index")
    faiss.write_index(index, path)
    with open(path, "rb") as f:
        assert f.read(4) == (b"IxPT" if wrapped else b"IxSQ")
    back = faiss.read_index(path)
    assert type(back) is type(index) and back.ntotal == nb and back.is_trained
    a, b = (index.index, back.index) if wrapped else (index, back)
    assert isinstance(b, faiss.IndexScalarQuantizer)
    assert (b.d, b.qtype, b.metric_type, b.code_size) == (a.d, qtype, metric, a.code_size)
    assert b.sq.trained.tobytes() == a.sq.trained.tobytes()
    np.testing.assert_array_equal(a.codes, b.codes)
    for k in (10, 100):
        check(back.search(xq, k), index.search(xq, k))
    if not wrapped:
        check(back.search(xq, 10), R.Ref(xb, qtype, metric).search(xq, 10))
        with pytest.raises(RuntimeError):
            faiss.write_index(index, path + ".native", fmt="native")


def test_factory_builds_the_index():
    for key, qtype in (("SQ8", R.QT_8BIT), ("SQfp16", R.QT_FP16)):
        ix = faiss.index_factory(32, key, IP)
        assert isinstance(ix, faiss.IndexScalarQuantizer) and (ix.qtype, ix.metric_type, ix.d) == (qtype, IP, 32)
    assert faiss.index_factory(32, "SQ8").metric_type == L2


# --------------------------------------------------------------- caller replay
def test_beir_sq_faiss_search_replay(tmp_path):
    """beir faiss_search.py:415-459 SQFaissSearch: the quantizer type looked up by name,
    IndexScalarQuantizer(dim, qtype, METRIC_INNER_PRODUCT), train, add, save
    (write_index to a ".sq" file), load (read_index) and search."""
    d, nb, nq, k = 64, 3000, 20, 10
    xb, xq = data(81, nb, d, IP), data(82, nq, d, IP)
    qtype = getattr(faiss.ScalarQuantizer, "QT_fp16")
    base_index = faiss.IndexScalarQuantizer(d, qtype, faiss.METRIC_INNER_PRODUCT)
    base_index.train(xb)
    base_index.add(xb)
    path = str(tmp_path / "my-index.sq")
    faiss.write_index(base_index, path)
    loaded = faiss.read_index(path)
    ref = R.Ref(xb, R.QT_FP16, IP)
    check(loaded.search(xq, k), ref.search(xq, k), ref, xq)
    check(base_index.search(xq, k), ref.search(xq, k))
