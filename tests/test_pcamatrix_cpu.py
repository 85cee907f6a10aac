"""PCAMatrix without a GPU: the host half of training (train_from_moments / prepare_Ab)
against tests/pca_ref.py, the "PcAm" file record, the factory fronts and copy_from."""
import struct

import numpy as np
import pytest

import faiss_amd as faiss
import pca_ref as R
from faiss_amd import faiss_io
from faiss_amd import index as fidx

D = 12
SPECTRUM = 3.0 ** -np.arange(D) * 500.0  # well separated, all positive


def _moments(spectrum=SPECTRUM, seed=5):
    """A hand-built symmetric matrix Q diag(spectrum) Q^T and a mean."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((len(spectrum), len(spectrum))))
    S = (q * np.asarray(spectrum)[None, :]) @ q.T
    return rng.standard_normal(len(spectrum)).astype(np.float32) * 3, (S + S.T) / 2


@pytest.mark.parametrize("eigen_power", [0.0, -0.5])
@pytest.mark.parametrize("rotate", [False, True])
def test_train_from_moments_matches_ref(eigen_power, rotate):
    mean, S = _moments()
    d_out = 5
    pca = faiss.PCAMatrix(D, d_out, eigen_power, rotate)
    assert not pca.is_trained and pca.have_bias
    assert (pca.balanced_bins, pca.max_points_per_d, pca.seed) == (0, 1000, 1234)
    pca.train_from_moments(mean, S)
    ref = R.train_from_moments(mean, S, d_out, eigen_power, rotate)
    assert pca.is_trained
    for name in ("mean", "eigenvalues", "PCAMat", "A", "b"):
        got = faiss.vector_to_array(getattr(pca, name))
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got.reshape(-1), ref[name].reshape(-1), err_msg=name)
    assert pca.A.shape == (d_out, D) and pca.b.shape == (d_out,)
    assert np.all(np.diff(pca.eigenvalues) <= 0)
    np.testing.assert_allclose(pca.eigenvalues, SPECTRUM, rtol=1e-5)
    if eigen_power == 0:  # orthonormal rows, rotated or not
        np.testing.assert_allclose(pca.A.astype(np.float64) @ pca.A.astype(np.float64).T, np.eye(d_out), atol=1e-6)
    if not rotate and eigen_power == 0:
        np.testing.assert_array_equal(pca.A, pca.PCAMat.reshape(D, D)[:d_out])
    # y = A (x - mean): the mean itself maps to (nearly) 0
    y0 = pca.A.astype(np.float64) @ mean.astype(np.float64) + pca.b
    assert np.abs(y0).max() <= 1e-5 * max(1.0, np.abs(pca.A).max() * np.abs(mean).max() * D)


def test_whitening_scales_rows():
    mean, S = _moments()
    plain = faiss.PCAMatrix(D, 4)
    white = faiss.PCAMatrix(D, 4, -0.5)
    plain.train_from_moments(mean, S)
    white.train_from_moments(mean, S)
    scale = plain.eigenvalues[:4].astype(np.float64) ** -0.5
    np.testing.assert_allclose(white.A, plain.A * scale[:, None], rtol=1e-6)


def test_errors():
    mean, S = _moments(np.concatenate([SPECTRUM[:6], np.zeros(D - 6)]))
    # (an exactly singular matrix: eigh returns tiny values of either sign for the null space;
    # the first one at or below zero is named)
    S = np.diag(np.concatenate([SPECTRUM[:6], np.zeros(D - 6)]))
    pca = faiss.PCAMatrix(D, 8, -0.5)
    with pytest.raises(RuntimeError, match="eigenvalue 6"):
        pca.train_from_moments(mean, S)
    ok = faiss.PCAMatrix(D, 6, -0.5)
    ok.train_from_moments(mean, S)  # the needed ones are positive
    assert ok.is_trained
    with pytest.raises(RuntimeError, match="d_out"):
        faiss.PCAMatrix(D, D + 1).train_from_moments(mean, S)
    bins = faiss.PCAMatrix(D, 4)
    bins.balanced_bins = 2
    with pytest.raises(RuntimeError, match="balanced_bins"):
        bins.train_from_moments(mean, S)
    with pytest.raises(RuntimeError, match="balanced_bins"):
        bins.train(np.zeros((4, D), np.float32))
    with pytest.raises(RuntimeError):
        faiss.PCAMatrix(D, 4).train_from_moments(mean[:-1], S)
    with pytest.raises(RuntimeError):
        faiss.PCAMatrix(D, 4).prepare_Ab()


def _trained(d_out=5, eigen_power=-0.5, rotate=True):
    mean, S = _moments()
    pca = faiss.PCAMatrix(D, d_out, eigen_power, rotate)
    pca.train_from_moments(mean, S)
    return pca


def _vec(a):
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    return struct.pack("<Q", a.size) + a.tobytes()


def test_pcam_record_layout(tmp_path):
    pca = _trained()
    # the record assembled by hand, field by field
    rec = b"".join([b"PcAm", struct.pack("<f", -0.5), struct.pack("<B", 1), struct.pack("<i", 0),
                    _vec(pca.mean), _vec(pca.eigenvalues), _vec(pca.PCAMat),
                    struct.pack("<B", 1), _vec(pca.A), _vec(pca.b), struct.pack("<i", D), struct.pack("<i", 5),
                    struct.pack("<B", 1)])
    t = faiss_io.parse_vector_transform(rec)
    assert t["kind"] == "pca" and (t["d_in"], t["d_out"], t["have_bias"], t["is_trained"]) == (D, 5, True, True)
    assert t["eigen_power"] == -0.5 and t["random_rotation"] is True and t["balanced_bins"] == 0
    for name in ("mean", "eigenvalues", "PCAMat", "A", "b"):
        np.testing.assert_array_equal(np.asarray(t[name]).reshape(-1), getattr(pca, name).reshape(-1), err_msg=name)
    # serialize is the inverse
    buf = faiss_io.serialize_pca(pca.eigen_power, pca.random_rotation, pca.balanced_bins, pca.mean, pca.eigenvalues,
                                 pca.PCAMat, pca.A, pca.b, pca.d_in, pca.d_out)
    assert buf == rec
    with pytest.raises(RuntimeError, match="truncated"):
        faiss_io.parse_vector_transform(rec[:-3])
    # write_VectorTransform / read_VectorTransform
    p = tmp_path / "pca.vt"
    faiss.write_VectorTransform(pca, str(p))
    assert p.read_bytes() == rec
    back = faiss.read_VectorTransform(str(p))
    assert type(back) is faiss.PCAMatrix and back.is_trained
    assert (back.d_in, back.d_out, back.eigen_power, back.random_rotation) == (D, 5, -0.5, True)
    for name in ("mean", "eigenvalues", "PCAMat", "A", "b"):
        np.testing.assert_array_equal(getattr(back, name).reshape(-1), getattr(pca, name).reshape(-1), err_msg=name)


def test_ltra_still_linear_transform(tmp_path):
    rng = np.random.default_rng(3)
    lt = faiss.LinearTransform(6, 4, True)
    lt.set_matrix(rng.standard_normal((4, 6)), rng.standard_normal(4))
    p = tmp_path / "lt.vt"
    faiss.write_VectorTransform(lt, str(p))
    assert p.read_bytes()[:4] == b"LTra"
    back = faiss.read_VectorTransform(str(p))
    assert type(back) is faiss.LinearTransform
    np.testing.assert_array_equal(back.A, lt.A)
    np.testing.assert_array_equal(back.b, lt.b)
    with pytest.raises(RuntimeError, match="LTra.*PcAm"):
        faiss_io.parse_vector_transform(b"XxXx" + p.read_bytes()[4:])


def test_ixpt_pcam_flat_round_trip(tmp_path):
    """IndexPreTransform(PCAMatrix, IndexFlatIP) through write_index / read_index: the flat
    index's rows live on the host until a search, so no GPU is touched."""
    pca = _trained(d_out=4, eigen_power=0.0, rotate=False)
    inner = faiss.IndexFlatIP(4)
    ix = faiss.IndexPreTransform(pca, inner)
    assert ix.is_trained and ix.d == D
    rows = np.random.default_rng(9).standard_normal((37, 4)).astype(np.float32)
    inner.add(rows)
    p = tmp_path / "pca_flat.index"
    faiss.write_index(ix, str(p))
    buf = p.read_bytes()
    assert buf[:4] == b"IxPT" and b"PcAm" in buf and b"IxFI" in buf
    z = faiss_io.parse_index(buf)
    assert z["kind"] == "pretransform" and z["chain"][0]["kind"] == "pca" and z["index"]["kind"] == "flat"
    back = faiss.read_index(str(p), device=0)
    assert isinstance(back, faiss.IndexPreTransform)
    bp = back.chain.at(0)
    assert type(bp) is faiss.PCAMatrix and type(back.index) is faiss.IndexFlatIP
    for name in ("mean", "eigenvalues", "PCAMat", "A", "b"):
        np.testing.assert_array_equal(getattr(bp, name).reshape(-1), getattr(pca, name).reshape(-1), err_msg=name)
    assert back.ntotal == 37
    np.testing.assert_array_equal(back.index.xb.reshape(37, 4), rows)


FRONTS = {"PCA": (0.0, False), "PCAR": (0.0, True), "PCAW": (-0.5, False), "PCAWR": (-0.5, True)}
INNER = {"Flat": faiss.IndexFlat, "PQ4": faiss.IndexPQ, "IVF8,PQ4": faiss.IndexIVFPQ, "IVF8,Flat": faiss.IndexIVFFlat,
         "SQ8": faiss.IndexScalarQuantizer, "SQfp16": faiss.IndexScalarQuantizer}


@pytest.mark.parametrize("front", sorted(FRONTS))
def test_factory_front_parse(front):
    power, rotate = FRONTS[front]
    for rest in INNER:
        assert fidx.parse_pca_front(f"{front}16,{rest}") == (16, power, rotate, rest)
    assert fidx.parse_pca_front("IVF8,PQ4") is None and fidx.parse_pca_front("OPQ8,PQ8") is None
    # built: the flat inner index needs no device (the other inner keys: test_gpu_pcamatrix.py)
    for metric in (faiss.METRIC_L2, faiss.METRIC_INNER_PRODUCT):
        ix = faiss.index_factory(32, f" {front}16, Flat", metric, device=0)
        pca = ix.chain.at(0)
        assert type(ix) is faiss.IndexPreTransform and type(pca) is faiss.PCAMatrix and len(ix.chain) == 1
        assert (pca.d_in, pca.d_out, pca.eigen_power, pca.random_rotation) == (32, 16, power, rotate)
        assert isinstance(ix.index, faiss.IndexFlat) and ix.index.d == 16 and ix.index.metric_type == metric
        assert ix.d == 32 and not ix.is_trained


def test_factory_rejects():
    for key in ("PCAX8,Flat", "PCA,Flat", "PCA8", "PCARW8,Flat"):
        with pytest.raises(RuntimeError, match=key):
            faiss.index_factory(32, key)
    with pytest.raises(RuntimeError, match="HNSW32"):
        faiss.index_factory(32, "PCA16,HNSW32")
    with pytest.raises(RuntimeError, match="PCA.*dout"):
        faiss.index_factory(32, "HNSW32")
    with pytest.raises(RuntimeError, match="d_out"):
        faiss.index_factory(32, "PCA64,Flat")


def test_plan_is_host_arithmetic():
    """The scatter's split depends on (n, d) and the chunk length alone; no device is asked."""
    from faiss_amd import transform as T

    assert T.pca_plan(768000, 768) == {"chunks": 14, "chunk_rows": 54880, "tiles": 78}
    assert T.pca_plan(128000, 128) == {"chunks": 334, "chunk_rows": 384, "tiles": 3}
    assert T.pca_plan(1, 7) == {"chunks": 1, "chunk_rows": 256, "tiles": 1}
    try:
        T.pca_set_chunk_rows(64)
        assert T.pca_plan(1000, 48) == {"chunks": 16, "chunk_rows": 64, "tiles": 1}
        T.pca_set_chunk_rows(33)  # rounded up to the staged step
        assert T.pca_plan(1000, 65) == {"chunks": 16, "chunk_rows": 64, "tiles": 3}
        T.pca_set_chunk_rows(32)
        with pytest.raises(RuntimeError, match="chunk"):  # more chunks than one launch takes
            T.pca_plan(32 * 65536, 8)
        with pytest.raises(RuntimeError):
            T.pca_set_chunk_rows(-1)
    finally:
        T.pca_set_chunk_rows(0)
    assert T.pca_plan(1000, 48)["chunks"] == 4
    for n, d in ((0, 8), (-1, 8), (4, 0), (4, 65537)):
        with pytest.raises(RuntimeError):
            T.pca_plan(n, d)


def test_copy_from_returns_self():
    pca = _trained()
    other = faiss.PCAMatrix()
    got = other.copy_from(pca)
    assert got is other
    for name in ("d_in", "d_out", "have_bias", "is_trained", "eigen_power", "random_rotation", "balanced_bins",
                 "max_points_per_d", "seed"):
        assert getattr(other, name) == getattr(pca, name), name
    for name in ("A", "b", "mean", "eigenvalues", "PCAMat"):
        np.testing.assert_array_equal(getattr(other, name), getattr(pca, name), err_msg=name)
        assert getattr(other, name) is not getattr(pca, name)
