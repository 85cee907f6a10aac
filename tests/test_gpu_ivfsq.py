"""IndexIVFScalarQuantizer on the GPU against Faiss's IndexIVFScalarQuantizer restated in numpy
on the oracle and the scalar quantizer's reference (tests/ivfsq_ref.py): labels and distances
must be bit-identical to it in every case; there is no tolerance.

The base index has eight lists whose sizes are chosen to meet every boundary of the scan: one
longer than RANGE_ROWS (two row ranges, the second one short), lists of 255, 256 and 257 rows
(the 256-row tile), one of a single row and an empty one.  The data are the centroids plus
noise, the centroids +-4 e_i, so that the coarse top-1 of a row is the centroid it was drawn
around under either metric; the tests assert the sizes from ``invlists.list_sizes()``.
Labels are a permutation with gaps, so label order is not add order.
"""
import functools

import numpy as np
import pytest

import faiss_amd as faiss
import ivfflat_ref as RF
import ivfsq_ref as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu

IP, L2 = faiss.METRIC_INNER_PRODUCT, faiss.METRIC_L2
METRICS = [pytest.param(IP, id="ip"), pytest.param(L2, id="l2")]
QT_FP16, QT_8BIT, QT_UNIFORM = R.QT_FP16, R.QT_8BIT, R.QT_8BIT_UNIFORM
QTYPES = [pytest.param(QT_FP16, id="fp16"), pytest.param(QT_8BIT, id="8bit"), pytest.param(QT_UNIFORM, id="uniform")]
RESIDUAL = [pytest.param(False, id="plain"), pytest.param(True, id="residual")]
NLIST = 8
BASE_SIZES = (R.S.RANGE_ROWS + 104, 255, 256, 257, 1, 0, 300, 327)  # 5 596 rows
WIDE_SIZES = (300, 0, 1, 99, 100, 50, 25, 25)                       # 600 rows (d = 2048)


def centroids(d, nlist=NLIST):
    """+-4 e_i (i < 4) and, past four dimensions, small seeded values elsewhere."""
    cent = (0.1 * np.random.default_rng(100 + d).standard_normal((nlist, d))).astype(np.float32)
    cent[:, :4] = 0
    for l in range(nlist):
        cent[l, l % 4] = 4.0 if l < 4 else -4.0
    return cent


def around(seed, cent, sizes, scale=0.3):
    """Rows drawn around the centroids, sizes[l] of them around centroid l, shuffled."""
    rng = np.random.default_rng(seed)
    of = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    return (cent[of] + scale * rng.standard_normal((len(of), cent.shape[1]))).astype(np.float32)


def gapped_ids(seed, n):
    return (np.random.default_rng(seed).permutation(3 * n)[:n]).astype(np.int64) + 11


@functools.lru_cache(maxsize=None)
def dataset(d, sizes=BASE_SIZES, nq=37):
    cent = centroids(d)
    xb = around(1, cent, sizes)
    xq = around(2, cent, [nq // NLIST + (1 if l < nq % NLIST else 0) for l in range(NLIST)], 0.5)
    return cent, xb, xq, gapped_ids(3, len(xb))


def build(xb, cent, qtype, metric, by_residual, trained, ids=None):
    ix = faiss.IndexIVFScalarQuantizer(None, xb.shape[1], len(cent), qtype, metric, by_residual)
    assert not ix.is_trained
    ix.set_trained(cent, trained)
    assert ix.is_trained and ix.by_residual == by_residual and ix.code_size == R.S.code_size(qtype, xb.shape[1])
    if ids is None:
        ix.add(xb)
    else:
        ix.add_with_ids(xb, ids)
    return ix


@functools.lru_cache(maxsize=None)
def case(d, qtype, metric, by_residual, sizes=BASE_SIZES):
    """(index, reference, queries) over dataset(d, sizes); the quantizer's table is the reference's."""
    cent, xb, xq, ids = dataset(d, sizes, 37 if sizes is BASE_SIZES else 5)
    ref = R.Ref(xb, cent, qtype, metric, by_residual, ids)
    ix = build(xb, cent, qtype, metric, by_residual, ref.trained, ids)
    np.testing.assert_array_equal(ix.invlists.list_sizes(), sizes)  # the boundaries the sizes were chosen for
    return ix, ref, xq


def check(got, want):
    D, I = got
    Dr, Ir = want
    np.testing.assert_array_equal(I, Ir)
    assert D.dtype == np.float32 and D.tobytes() == Dr.tobytes(), np.abs(D - Dr).max()


# ------------------------------------------------------------------ the sweeps
@pytest.mark.parametrize("by_residual", RESIDUAL)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("qtype", QTYPES)
@pytest.mark.parametrize("d", [4, 12, 64, 68, 136])
def test_sweep_dimensions_types_metrics(d, qtype, metric, by_residual):
    """d: below one 64-dimension step, one step exactly, a step + the 4-wide remainder, two steps + 8."""
    ix, ref, xq = case(d, qtype, metric, by_residual)
    ix.nprobe = 3
    assert ix.sq.trained.tobytes() == ref.trained.tobytes() and ix.sq.qtype == qtype
    check(ix.search(xq, 10), ref.search(xq, 10, nprobe=3))


@pytest.mark.parametrize("k", [1, 64, 65, 256, 257, 1024])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("qtype", [pytest.param(QT_FP16, id="fp16"), pytest.param(QT_8BIT, id="8bit")])
def test_sweep_k_classes_probes_and_query_counts(qtype, metric, k):
    """k at the edges of the (G, R) classes; one probe and every list; a lone query and nine
    (one pair past a group of eight, two groups of four and one)."""
    ix, ref, xq = case(68, qtype, metric, True)
    for nprobe in (1, 8):
        ix.nprobe = nprobe
        for nq in (1, 9):
            check(ix.search(xq[:nq], k), ref.search(xq[:nq], k, nprobe=nprobe))


@pytest.mark.parametrize("by_residual", RESIDUAL)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("qtype", [pytest.param(QT_FP16, id="fp16"), pytest.param(QT_8BIT, id="8bit")])
def test_sweep_widest_rows(qtype, metric, by_residual):
    ix, ref, xq = case(2048, qtype, metric, by_residual, WIDE_SIZES)
    ix.nprobe = 3
    check(ix.search(xq, 10), ref.search(xq, 10, nprobe=3))


# ------------------------------------------------------------------ equivalences
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("qtype", QTYPES)
def test_plain_codes_equal_ivfflat_over_the_decoded_rows(qtype, metric):
    ix, ref, xq = case(68, qtype, metric, False)
    sq = faiss.IndexScalarQuantizer(68, qtype, metric)
    sq.set_trained(ref.trained)
    dec = sq.sa_decode(sq.sa_encode(ref.xb))
    assert dec.tobytes() == ref.dec.tobytes()
    flat = faiss.IndexIVFFlat(None, 68, NLIST, metric)
    flat.set_trained(ref.cent)
    flat.add_with_ids(dec, ref.ids)
    np.testing.assert_array_equal(flat.invlists.list_sizes(), ix.invlists.list_sizes())
    for k, nprobe in ((10, 3), (100, 8)):
        ix.nprobe = flat.nprobe = nprobe
        check(ix.search(xq, k), flat.search(xq, k))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("qtype", QTYPES)
def test_one_list_of_plain_codes_equals_the_flat_scalar_quantizer(qtype, metric):
    cent, xb, xq, _ = dataset(68)
    trained = R.S.train(xb, qtype)
    ix = build(xb, np.zeros((1, 68), np.float32), qtype, metric, False, trained)
    sq = faiss.IndexScalarQuantizer(68, qtype, metric)
    sq.set_trained(trained)
    sq.add(xb)
    assert ix.invlists.get_codes(0).tobytes() == sq.codes.tobytes()
    for k in (10, 100):
        check(ix.search(xq, k), sq.search(xq, k))


# ------------------------------------------------------------------ preassigned
@pytest.mark.parametrize("by_residual", RESIDUAL)
@pytest.mark.parametrize("metric", METRICS)
def test_search_preassigned(metric, by_residual):
    import torch

    ix, ref, xq = case(68, QT_8BIT, metric, by_residual)
    ix.nprobe = 4
    Dc, Iq = O.coarse_search(xq, ref.cent, 4, metric=metric)
    Iq = Iq.copy()
    Iq[0, 2] = -1
    Iq[1] = -1            # nothing to scan
    Iq[2, 3] = Iq[2, 0]   # a repeated list is scanned once
    Iq[3, :] = Iq[3, 0]
    Dq = np.random.default_rng(56).standard_normal(Iq.shape).astype(np.float32)  # not the coarse values
    want = ref.search(xq, 20, Iq=Iq, Dq=Dq)
    want0 = ref.search(xq, 20, Iq=Iq)  # Dq = None: zeros
    assert (want[1][1] == -1).all()
    if metric == IP and by_residual:  # Dq is part of the result ...
        assert want[0].tobytes() != want0[0].tobytes()
        assert want0[0].tobytes() != ref.search(xq, 20, Iq=Iq, Dq=Dc)[0].tobytes()
    else:                             # ... and otherwise ignored, whatever it holds
        assert want[0].tobytes() == want0[0].tobytes() and want[1].tobytes() == want0[1].tobytes()
        Dq[:] = np.float32(3e38)
        Dq[0, 0] = np.nan
    check(ix.search_preassigned(xq, 20, Iq, Dq), want)
    check(ix.search_preassigned(xq, 20, Iq), want0)
    check(faiss.ivf_tools.search_preassigned(ix, xq, 20, Iq), want0)
    D = np.empty((len(xq), 20), np.float32)
    I = np.empty((len(xq), 20), np.int64)
    assert ix.search_preassigned(len(xq), faiss.swig_ptr(xq), 20, faiss.swig_ptr(Iq), faiss.swig_ptr(Dq),
                                 faiss.swig_ptr(D), faiss.swig_ptr(I), False) is None
    check((D, I), want)
    with pytest.raises(RuntimeError, match="nprobe"):
        ix.search_preassigned(xq, 20, Iq[:, :3])
    # the device entry point, with and without Dq
    tx, tIq, tDq = torch.from_numpy(xq).cuda(), torch.from_numpy(Iq).cuda(), torch.from_numpy(Dq).cuda()
    Dd, Id = ix.search_preassigned_device(tx, 20, tIq, tDq)
    D0, I0 = ix.search_preassigned_device(tx, 20, tIq)
    torch.cuda.synchronize()
    check((Dd.cpu().numpy(), Id.cpu().numpy()), want)
    check((D0.cpu().numpy(), I0.cpu().numpy()), want0)
    # search is search_preassigned with the coarse quantizer's own probes and values
    check(ix.search(xq, 20), ref.search(xq, 20, Iq=O.coarse_search(xq, ref.cent, 4, metric=metric)[1], Dq=Dc))


@pytest.mark.parametrize("metric", METRICS)
def test_queries_taken_in_chunks_of_the_residual_workspace(metric):
    """The residual queries are [chunk][nprobe][d] floats within 256 MiB: at d = 2048 and 1024 probe
    columns a chunk is 32 queries, so 70 queries go in three chunks, each with its own rows of Iq
    and Dq.  (Two columns of a row hold lists, wherever they stand; the rest are skipped.  The inner
    product has no residual workspace and takes the queries at once, reading Dq at those columns.)"""
    ix, ref, _ = case(2048, QT_FP16, metric, True, WIDE_SIZES)
    nq, ncol = 70, 1024
    assert (1 << 28) // (4 * ncol * 2048) == 32 and nq > 2 * 32
    rng = np.random.default_rng(57)
    xq = around(58, ref.cent, [9, 9, 9, 9, 9, 9, 8, 8], 0.5)
    Iq = np.full((nq, ncol), -1, np.int64)
    for q in range(nq):
        Iq[q, rng.choice(ncol, 2, replace=False)] = rng.choice(NLIST, 2, replace=False)
    Dq = rng.standard_normal(Iq.shape).astype(np.float32)
    ix.nprobe = ncol
    check(ix.search_preassigned(xq, 10, Iq, Dq), ref.search(xq, 10, Iq=Iq, Dq=Dq))


# ------------------------------------------------------------------------ edges
@pytest.mark.parametrize("by_residual", RESIDUAL)
@pytest.mark.parametrize("metric", METRICS)
def test_fewer_rows_than_k_empty_index_and_reset(metric, by_residual):
    cent = centroids(12)
    xb = around(5, cent, (9, 0, 3, 0, 0, 1, 0, 7))
    xq = around(6, cent, (1,) * NLIST, 0.5)
    ref = R.Ref(xb, cent, QT_8BIT, metric, by_residual)
    ix = faiss.IndexIVFScalarQuantizer(None, 12, NLIST, QT_8BIT, metric, by_residual)
    ix.set_trained(cent, ref.trained)
    pad = -R.FMAX if metric == IP else R.FMAX
    D, I = ix.search(xq, 5)  # the empty index
    assert ix.ntotal == 0 and (I == -1).all() and (D == pad).all()
    ix.add(xb)
    ix.nprobe = NLIST
    want = ref.search(xq, 64, nprobe=NLIST)
    assert (want[1][:, 20:] == -1).all() and (want[1][:, :20] >= 0).all()
    check(ix.search(xq, 64), want)
    ix.nprobe = 50  # > nlist: clamped
    check(ix.search(xq, 64), want)
    ix.reset()
    assert ix.ntotal == 0 and ix.is_trained and ix.sq.trained.tobytes() == ref.trained.tobytes()
    np.testing.assert_array_equal(ix.centroids(), cent)
    D, I = ix.search(xq, 5)
    assert (I == -1).all() and (D == pad).all()
    ix.add(xb[:10])
    assert ix.ntotal == 10 and ix.invlists.list_sizes().sum() == 10


def test_a_query_equal_to_a_stored_row_is_at_distance_zero():
    cent, xb, _, ids = dataset(68)
    xb = xb.astype(np.float16).astype(np.float32)  # rows the fp16 codec stores exactly
    ref = R.Ref(xb, cent, QT_FP16, L2, False, ids)
    ix = build(xb, cent, QT_FP16, L2, False, ref.trained, ids)
    rows = np.array([0, 17, len(xb) - 1])
    ix.nprobe = 2
    D, I = ix.search(xb[rows], 3)
    check((D, I), ref.search(xb[rows], 3, nprobe=2))
    np.testing.assert_array_equal(I[:, 0], ids[rows])
    assert (D[:, 0] == 0).all() and (D[:, 1] > 0).all()


# ------------------------------------------------------------------------ adds
@pytest.mark.parametrize("by_residual", RESIDUAL)
@pytest.mark.parametrize("qtype", QTYPES)
def test_adds_build_the_same_label_sorted_lists(qtype, by_residual):
    import torch

    metric = L2
    _, ref, xq = case(68, qtype, metric, by_residual)
    xb, cent, ids, nb = ref.xb, ref.cent, ref.ids, len(ref.xb)
    want = ref.lists()
    parts = faiss.IndexIVFScalarQuantizer(None, 68, NLIST, qtype, metric, by_residual)
    parts.set_trained(cent, ref.trained)
    parts.nprobe = 3
    done = 0
    for n in (1, 4300, nb - 4301):  # three uneven adds, a search after each (the pending set is merged)
        parts.add_with_ids(xb[done:done + n], ids[done:done + n])
        done += n
        sub = R.Ref(xb[:done], cent, qtype, metric, by_residual, ids[:done], ref.trained)
        check(parts.search(xq, 10), sub.search(xq, 10, nprobe=3))
    dev = faiss.IndexIVFScalarQuantizer(None, 68, NLIST, qtype, metric, by_residual)
    dev.set_trained(cent, ref.trained)
    tx, tid = torch.from_numpy(xb).cuda(), torch.from_numpy(ids).cuda()
    dev.add_device(tx[:2000], tid[:2000])
    dev.add_device(tx[2000:], tid[2000:])
    for ix in (parts, dev):
        assert ix.ntotal == nb and ix.invlists.code_size == ix.code_size
        np.testing.assert_array_equal(ix.invlists.list_sizes(), BASE_SIZES)
        for l in range(NLIST):
            got = ix.invlists.get_ids(l)
            assert (np.diff(got) > 0).all()
            np.testing.assert_array_equal(got, want[l][0])
            codes = ix.invlists.get_codes(l)
            assert codes.dtype == np.uint8 and codes.tobytes() == want[l][1].tobytes()
            assert ix.invlists.list_size(l) == BASE_SIZES[l]
        sizes = np.array(BASE_SIZES, float)
        assert ix.invlists.imbalance_factor() == pytest.approx(NLIST * (sizes ** 2).sum() / nb ** 2)
    # sequential ids: add_device without ids, then add
    seq = faiss.IndexIVFScalarQuantizer(None, 68, NLIST, qtype, metric, by_residual)
    seq.set_trained(cent, ref.trained)
    seq.add_device(tx[:5])
    seq.add(xb[5:8])
    assert sorted(np.concatenate([seq.invlists.get_ids(l) for l in range(NLIST)])) == list(range(8))


@pytest.mark.parametrize("by_residual", RESIDUAL)
@pytest.mark.parametrize("metric", METRICS)
def test_search_device_on_a_side_stream_into_the_callers_outputs(metric, by_residual):
    import torch

    ix, ref, xq = case(68, QT_FP16, metric, by_residual)
    ix.nprobe = 4
    want = ref.search(xq, 10, nprobe=4)
    tx = torch.from_numpy(xq).cuda()
    D = torch.empty((len(xq), 10), dtype=torch.float32, device="cuda")
    I = torch.empty((len(xq), 10), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        Ds, Is = ix.search_device(tx, 10, D, I)
    D2, I2 = ix.search_device(tx, 10)  # torch's current stream: ordered after the side stream's call
    side.synchronize()
    torch.cuda.synchronize()
    assert Ds.data_ptr() == D.data_ptr() and Is.data_ptr() == I.data_ptr()
    check((D.cpu().numpy(), I.cpu().numpy()), want)
    check((D2.cpu().numpy(), I2.cpu().numpy()), want)
    with pytest.raises(RuntimeError):
        ix.search_device(tx.double(), 10)


# -------------------------------------------------------------------- training
@pytest.mark.parametrize("by_residual", RESIDUAL)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("qtype", QTYPES)
def test_training(qtype, metric, by_residual):
    d, n, niter, seed = 12, 3000, 4, 99
    x = around(71, centroids(d), (375,) * NLIST, 1.0)
    ix = faiss.IndexIVFScalarQuantizer(None, d, NLIST, qtype, metric, by_residual)
    flat = faiss.IndexIVFFlat(None, d, NLIST, metric)
    assert not ix.is_trained and ix.sq.trained.size == 0
    ix.niter_coarse, ix.seed = flat.niter_coarse, flat.seed = niter, seed
    ix.train(x)
    flat.train(x)
    assert ix.is_trained
    np.testing.assert_array_equal(ix.centroids(), flat.centroids())  # exactly IndexIVFFlat.train's
    np.testing.assert_array_equal(ix.centroids(), O.kmeans(x, NLIST, niter, seed, metric=metric))
    assert ix.quantizer.ntotal == NLIST
    np.testing.assert_array_equal(ix.quantizer.xb.reshape(NLIST, d), ix.centroids())
    want = R.train_sq(x, ix.centroids(), qtype, metric, by_residual)
    assert ix.sq.trained.dtype == np.float32 and ix.sq.trained.tobytes() == want.tobytes()
    if qtype != QT_FP16:  # the residuals' table is not the rows'
        assert (want.tobytes() != R.S.train(x, qtype).tobytes()) == by_residual


@pytest.mark.parametrize("by_residual", RESIDUAL)
def test_training_subsamples_100000_rows_of_the_librarys_permutation(by_residual):
    d, n = 4, 100500
    rng = np.random.default_rng(72)
    x = rng.standard_normal((n, d)).astype(np.float32)
    rows = O.rand_perm_prefix(n, R.SQ_TRAIN_ROWS, R.SQ_TRAIN_SEED)
    np.testing.assert_array_equal(rows, R.train_rows(n))
    left_out = np.setdiff1d(np.arange(n), rows)
    assert len(left_out) == 500
    x[left_out[:250]] *= 50  # the extremes of the full set lie in rows the subsample leaves out
    ix = faiss.IndexIVFScalarQuantizer(None, d, 2, QT_8BIT, L2, by_residual)
    ix.niter_coarse = 1
    ix.train(x)
    want = R.train_sq(x, ix.centroids(), QT_8BIT, L2, by_residual)
    got = ix.sq.trained
    assert got.tobytes() == want.tobytes()
    full = R.S.train(x if not by_residual else R.residuals(x, ix.centroids(), RF.assign(x, ix.centroids(), L2)),
                     QT_8BIT)
    assert (got[:d] > full[:d]).all() and (got[:d] + got[d:] < full[:d] + full[d:]).all()


# ------------------------------------------------------------- file round trip
@pytest.mark.parametrize("by_residual", RESIDUAL)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("qtype", QTYPES)
def test_write_read_index_round_trip(qtype, metric, by_residual, tmp_path):
    ix, ref, xq = case(12, qtype, metric, by_residual)
    ix.nprobe = 4
    path = str(tmp_path / "ivfsq.index")
    faiss.write_index(ix, path)
    with pytest.raises(RuntimeError):
        faiss.write_index(ix, path + ".native", fmt="native")
    assert faiss.faiss_io.is_faiss_file(path)
    back = faiss.read_index(path)
    assert type(back) is faiss.IndexIVFScalarQuantizer
    assert (back.d, back.nlist, back.nprobe, back.ntotal, back.metric_type, back.qtype, back.by_residual) == \
        (ix.d, ix.nlist, 4, ix.ntotal, metric, qtype, by_residual)
    np.testing.assert_array_equal(back.centroids(), ix.centroids())
    assert back.sq.trained.tobytes() == ix.sq.trained.tobytes()
    for l in range(ix.nlist):
        np.testing.assert_array_equal(back.invlists.get_ids(l), ix.invlists.get_ids(l))
        assert back.invlists.get_codes(l).tobytes() == ix.invlists.get_codes(l).tobytes()
    check(back.search(xq, 10), ix.search(xq, 10))
    check(back.search(xq, 10), ref.search(xq, 10, nprobe=4))


# --------------------------------------------------------------------- factory
@pytest.mark.parametrize("metric", METRICS)
def test_index_factory_keys_build_train_add_and_search(metric):
    d = 64
    cent, xb, xq, _ = dataset(d)
    ix = faiss.index_factory(d, "IVF8,SQ8", metric)
    assert type(ix) is faiss.IndexIVFScalarQuantizer and ix.by_residual and ix.qtype == QT_8BIT
    assert (ix.d, ix.nlist, ix.metric_type, ix.code_size) == (d, 8, metric, d)
    assert faiss.downcast_index(ix) is ix and faiss.extract_index_ivf(ix) is ix
    ix.niter_coarse = 3
    ix.train(xb)
    ix.add(xb)
    faiss.ParameterSpace().set_index_parameters(ix, "nprobe=3")
    assert ix.nprobe == 3
    ref = R.Ref(xb, ix.centroids(), QT_8BIT, metric, True, trained=ix.sq.trained)
    check(ix.search(xq, 10), ref.search(xq, 10, nprobe=3))
    # behind a PCA front
    pt = faiss.index_factory(d, "PCA32,IVF8,SQfp16", metric)
    inner = faiss.extract_index_ivf(pt)
    assert type(inner) is faiss.IndexIVFScalarQuantizer and (inner.d, inner.qtype, inner.by_residual) == (32, QT_FP16, True)
    inner.niter_coarse = 3
    pt.train(xb)
    pt.add(xb)
    inner.nprobe = 3
    assert pt.is_trained and pt.ntotal == len(xb)
    yb, yq = pt.apply_chain(xb), pt.apply_chain(xq)
    ref = R.Ref(yb, inner.centroids(), QT_FP16, metric, True)
    check(pt.search(xq, 10), ref.search(yq, 10, nprobe=3))


# --------------------------------------------------------------- caller replay
def test_bench_gpu_1bn_float16_replay():
    """bench_gpu_1bn.py:571-595 with an index key ending in ",Flat" and -float16 (co.useFloat16 =
    True): here IndexIVFScalarQuantizer(coarse_quantizer, d, ncent, QT_fp16, METRIC_L2, False);
    train, the base added in slices (:598-658), ParameterSpace nprobe, the queries searched in
    blocks (:788-806)."""
    d, ncent, nb, nq, topK = 32, 32, 6000, 50, 10
    rng = np.random.default_rng(81)
    xt, xb, xq = (rng.standard_normal((n, d)).astype(np.float32) for n in (3000, nb, nq))
    coarse_quantizer = faiss.IndexFlatL2(d)
    idx_model = faiss.IndexIVFScalarQuantizer(coarse_quantizer, d, ncent, faiss.ScalarQuantizer.QT_fp16,
                                              faiss.METRIC_L2, False)
    idx_model.niter_coarse = 3
    idx_model.train(xt)
    assert coarse_quantizer.ntotal == ncent and idx_model.is_trained
    for i0 in range(0, nb, 2500):  # add_batch_size slices
        idx_model.add_with_ids(xb[i0:i0 + 2500], np.arange(i0, min(nb, i0 + 2500)))
    assert idx_model.ntotal == nb
    ps = faiss.ParameterSpace()
    ps.initialize(idx_model)
    ref = R.Ref(xb, idx_model.centroids(), QT_FP16, L2, False)
    for nprobe in (1, 8):
        ps.set_index_parameter(idx_model, "nprobe", nprobe)
        D = np.empty((nq, topK), np.float32)
        I = np.empty((nq, topK), np.int64)
        for q0 in range(0, nq, 16):  # query blocks of qbs
            D[q0:q0 + 16], I[q0:q0 + 16] = idx_model.search(xq[q0:q0 + 16], topK)
        check((D, I), ref.search(xq, topK, nprobe=nprobe))
