"""GPU: the PCA training moments (csrc/pca_moments.hip through ivfpq_pca_moments_device)
against float64, PCAMatrix training against the float64 eigendecomposition with derived
perturbation bounds, and PCA-fronted indexes end to end against the same inner index fed
oracle.linear_transform of base and queries.

The scatter bound is the standard one of an fp32 sum of n products in any order with one
rounding per product, plus one addition per chunk partial: with xc = x - mean_gpu formed in
float32 (the kernel's own input) and S64 = xc^T xc in float64,
|S_gpu - S64|_ij <= (n + chunks + 2) 2^-24 sum_r |xc_ri| |xc_rj|  (pca_ref.scatter_bound)."""
import ctypes
import functools

import numpy as np
import pytest

import faiss_amd as faiss
import pca_ref as R
from faiss_amd import _lib, datasets
from faiss_amd import transform as T
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def _gpu_moments(x):
    import torch

    mean, S = T.pca_moments_device(torch.from_numpy(x).cuda())
    return mean.cpu().numpy(), S.cpu().numpy()


# (n, d, chunk length through the hook (0: default), column offset)
MOMENT_CASES = [(1, 7, 0, 0.0), (3, 16, 0, 0.0), (257, 100, 0, 0.0), (1000, 128, 0, 0.0), (300, 768, 0, 0.0),
                (1000, 48, 64, 0.0), (1000, 48, 0, 100.0), (130, 67, 32, 100.0)]


@pytest.mark.parametrize("n,d,chunk_rows,offset", MOMENT_CASES)
def test_moments_against_float64(n, d, chunk_rows, offset):
    rng = np.random.default_rng(1000 * n + d)
    x = (rng.standard_normal((n, d)) + offset).astype(np.float32)
    T.pca_set_chunk_rows(chunk_rows)
    try:
        plan = T.pca_plan(n, d)
        tb = (d + 63) // 64
        assert plan["tiles"] == tb * (tb + 1) // 2
        if chunk_rows:  # the multi-chunk reduce is reached
            assert plan["chunk_rows"] == chunk_rows and plan["chunks"] == -(-n // chunk_rows) > 1
        else:
            assert plan["chunks"] == -(-n // plan["chunk_rows"])
        mean, S = _gpu_moments(x)
        mean2, S2 = _gpu_moments(x)
    finally:
        T.pca_set_chunk_rows(0)
    # mean: within 1 fp32 ulp of the float64 column mean
    m64 = x.astype(np.float64).mean(0)
    ulp = np.spacing(np.abs(m64).astype(np.float32)).astype(np.float64)
    err = np.abs(mean.astype(np.float64) - m64)
    print(f"mean: max error / ulp = {(err / ulp).max():.3f}")
    assert mean.dtype == np.float32 and np.all(err <= ulp)
    # scatter: the derived element bound, exact symmetry, reproducible bits
    S64, absprod = R.scatter_of_centred(x, mean)
    bound = R.scatter_bound(n, plan["chunks"], absprod)
    diff = np.abs(S.astype(np.float64) - S64)
    print(f"scatter: max |S_gpu - S64| / bound = {(diff[bound > 0] / bound[bound > 0]).max() if (bound > 0).any() else 0:.4f}"
          f" (chunks {plan['chunks']}, tiles {plan['tiles']})")
    assert S.shape == (d, d) and S.dtype == np.float32
    assert np.all(diff <= bound)
    np.testing.assert_array_equal(S, S.T)
    np.testing.assert_array_equal(S, S2)
    np.testing.assert_array_equal(mean, mean2)
    if n == 1:
        assert not S.any()


def test_chunk_length_changes_order_not_value():
    """Two chunk lengths give two summation orders; both stay inside the bound of the finer one."""
    n, d = 700, 80
    x = np.random.default_rng(7).standard_normal((n, d)).astype(np.float32) * 3 + 2
    out = []
    try:
        for rows in (32, 256):
            T.pca_set_chunk_rows(rows)
            assert T.pca_plan(n, d)["chunks"] == -(-n // rows)
            out.append(_gpu_moments(x))
    finally:
        T.pca_set_chunk_rows(0)
    np.testing.assert_array_equal(out[0][0], out[1][0])  # the mean has its own fixed chunks
    S64, absprod = R.scatter_of_centred(x, out[0][0])
    for (_, S), rows in zip(out, (32, 256)):
        assert np.all(np.abs(S - S64) <= R.scatter_bound(n, -(-n // rows), absprod))


def test_moments_errors():
    import torch

    L = _lib.load()
    x = torch.zeros((4, 8), device="cuda")
    m = torch.zeros(8, device="cuda")
    S = torch.zeros((8, 8), device="cuda")
    assert L.ivfpq_pca_moments_device(0, 8, x.data_ptr(), m.data_ptr(), S.data_ptr(), None) != 0
    assert "at least one row" in L.ivfpq_last_error().decode()
    assert L.ivfpq_pca_moments_device(4, 0, x.data_ptr(), m.data_ptr(), S.data_ptr(), None) != 0
    assert L.ivfpq_pca_moments_device(4, 8, None, m.data_ptr(), S.data_ptr(), None) != 0
    assert L.ivfpq_pca_get_plan(0, 8, None, None, None) != 0
    assert L.ivfpq_pca_set_chunk_rows(-1) != 0
    chunks = ctypes.c_int()
    assert L.ivfpq_pca_get_plan(10 ** 9, 8, ctypes.byref(chunks), None, None) == 0 and chunks.value >= 1
    with pytest.raises(RuntimeError):
        T.pca_moments_device(torch.zeros((0, 8), device="cuda"))
    with pytest.raises(RuntimeError):
        faiss.PCAMatrix(8, 4).train(np.zeros((0, 8), np.float32))


# ---------------------------------------------------------------- training

D_TRAIN, DOUT_TRAIN, N_TRAIN = 24, 4, 1500


@functools.lru_cache(maxsize=None)
def _train_data():
    """z diag(s) Q + mu: the first DOUT_TRAIN + 1 scales fall by 1.5 each, the rest sit at half
    the last of them."""
    rng = np.random.default_rng(99)
    s = np.concatenate([1.5 ** -np.arange(DOUT_TRAIN + 1), np.full(D_TRAIN - DOUT_TRAIN - 1, 0.5 * 1.5 ** -DOUT_TRAIN)])
    q, _ = np.linalg.qr(rng.standard_normal((D_TRAIN, D_TRAIN)))
    x = (rng.standard_normal((N_TRAIN, D_TRAIN)) * (4 * s)[None, :]) @ q + rng.standard_normal(D_TRAIN) * 5
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def test_training_against_float64():
    import torch

    x = _train_data()
    pca = faiss.PCAMatrix(D_TRAIN, DOUT_TRAIN)
    pca.train_device(torch.from_numpy(x.copy()).cuda())
    assert pca.is_trained and pca.A.shape == (DOUT_TRAIN, D_TRAIN)
    chunks = T.pca_plan(N_TRAIN, D_TRAIN)["chunks"]
    S64, absprod = R.scatter_of_centred(x, pca.mean)
    E = np.linalg.norm(R.scatter_bound(N_TRAIN, chunks, absprod))  # ||E||_F
    w, P = R.eig_desc(S64)
    # Weyl: every eigenvalue moves by at most ||E||_2 <= ||E||_F
    ev_err = np.abs(pca.eigenvalues.astype(np.float64) - w)
    print(f"eigenvalues: max error {ev_err.max():.3e}, ||E||_F {E:.3e}, lambda_1 {w[0]:.3e}")
    assert np.all(np.diff(pca.eigenvalues) <= 0)
    assert np.all(ev_err <= E)
    # Davis-Kahan: each of the first d_out eigenvectors, up to sign, within 2 ||E||_F / gap
    PM = pca.PCAMat.reshape(D_TRAIN, D_TRAIN).astype(np.float64)
    for i in range(DOUT_TRAIN):
        gap = min(w[i] - w[i + 1], w[i - 1] - w[i] if i else np.inf)
        thr = 2 * E / gap
        sign = 1.0 if PM[i] @ P[i] >= 0 else -1.0
        dist = np.linalg.norm(PM[i] - sign * P[i])
        print(f"eigenvector {i}: distance {dist:.3e}, threshold {thr:.3e}")
        assert thr < 0.05 and dist <= thr
    # the fields follow from the moments the GPU returned, by the reference's rules
    A, b = R.prepare_Ab(pca.mean, pca.eigenvalues, pca.PCAMat, DOUT_TRAIN)
    np.testing.assert_array_equal(pca.A, A)
    np.testing.assert_array_equal(pca.b, b)
    # train (numpy) and train_device agree bit for bit, subsampled or not
    host = faiss.PCAMatrix(D_TRAIN, DOUT_TRAIN)
    host.train(x)
    np.testing.assert_array_equal(host.A, pca.A)
    np.testing.assert_array_equal(host.b, pca.b)
    np.testing.assert_array_equal(host.eigenvalues, pca.eigenvalues)
    sub_h, sub_d = faiss.PCAMatrix(D_TRAIN, DOUT_TRAIN, -0.5, True), faiss.PCAMatrix(D_TRAIN, DOUT_TRAIN, -0.5, True)
    sub_h.max_points_per_d = sub_d.max_points_per_d = 20  # 480 of the 1500 rows
    sub_h.train(x)
    sub_d.train_device(torch.from_numpy(x.copy()).cuda())
    np.testing.assert_array_equal(sub_h.A, sub_d.A)
    assert not np.array_equal(sub_h.mean, pca.mean)
    keep = np.sort(np.random.default_rng(1234).choice(N_TRAIN, 480, replace=False))
    np.testing.assert_array_equal(sub_h.mean, _gpu_moments(np.ascontiguousarray(x[keep]))[0])
    # whitened and rotated: the transformed training rows have a scatter close to the identity
    y = sub_h.apply(x[keep])
    np.testing.assert_allclose(y.astype(np.float64).T @ y.astype(np.float64), np.eye(DOUT_TRAIN), atol=1e-3)


# ---------------------------------------------------------------- end to end

D_E2E, K = 64, 10


@functools.lru_cache(maxsize=None)
def _e2e_data():
    xt = datasets.synthetic_sift_like(4000, D_E2E, seed=31, n_centres=200)
    xb = datasets.synthetic_sift_like(3000, D_E2E, seed=32, n_centres=200)
    xq = datasets.synthetic_sift_like(200, D_E2E, seed=33, n_centres=200)
    for a in (xt, xb, xq):
        a.setflags(write=False)
    return xt, xb, xq


def _make(case):
    if case == "pretransform_flatip":
        return faiss.IndexPreTransform(faiss.PCAMatrix(D_E2E, 16), faiss.IndexFlatIP(16))
    return faiss.index_factory(D_E2E, case)


def _twin(ix):
    """The same inner index type with the same trained state, empty."""
    inner = ix.index
    if isinstance(inner, faiss.IndexPQ):
        twin = faiss.IndexPQ(inner.d, inner.M, inner.nbits, inner.metric_type)
        twin.set_trained(inner.codebook())
        return twin
    return faiss.IndexFlat(inner.d, inner.metric_type)


@pytest.mark.parametrize("case", ["pretransform_flatip", "PCAR16,Flat", "PCA32,PQ8"])
def test_index_matches_inner_on_oracle_transform(case, tmp_path):
    import torch

    xt, xb, xq = _e2e_data()
    ix = _make(case)
    pca = ix.chain.at(0)
    assert isinstance(ix, faiss.IndexPreTransform) and type(pca) is faiss.PCAMatrix and not ix.is_trained
    # beir's FaissTrainIndex.build: train, then buffered add
    ix.train(xt)
    assert ix.is_trained and pca.is_trained
    for start in range(0, len(xb), 1024):
        ix.add(xb[start:start + 1024])
    assert ix.ntotal == len(xb)
    D, I = ix.search(xq, K)
    A, b = faiss.vector_to_array(pca.A).reshape(pca.d_out, D_E2E), faiss.vector_to_array(pca.b)
    if pca.random_rotation:
        np.testing.assert_allclose(A.astype(np.float64) @ A.astype(np.float64).T, np.eye(pca.d_out), atol=1e-5)
    twin = _twin(ix)
    twin.add(O.linear_transform(xb, A, b))
    Dr, Ir = twin.search(O.linear_transform(xq, A, b), K)
    np.testing.assert_array_equal(I, Ir)
    np.testing.assert_array_equal(D, Dr)
    Dd, Id = ix.search_device(torch.from_numpy(xq).cuda(), K)
    np.testing.assert_array_equal(Id.cpu().numpy(), I)
    np.testing.assert_array_equal(Dd.cpu().numpy(), D)
    # save / load: the index file and the transform alone
    p = tmp_path / "my-index.pca.faiss"
    faiss.write_index(ix, str(p))
    back = faiss.read_index(str(p))
    bp = back.chain.at(0)
    assert isinstance(back, faiss.IndexPreTransform) and type(bp) is faiss.PCAMatrix
    assert type(back.index) is (faiss.IndexPQ if isinstance(ix.index, faiss.IndexPQ) else
                                {0: faiss.IndexFlatIP, 1: faiss.IndexFlatL2}[ix.index.metric_type])
    assert (bp.eigen_power, bp.random_rotation, bp.d_in, bp.d_out) == (pca.eigen_power, pca.random_rotation,
                                                                      pca.d_in, pca.d_out)
    for name in ("mean", "eigenvalues", "PCAMat", "A", "b"):
        np.testing.assert_array_equal(getattr(bp, name).reshape(-1), getattr(pca, name).reshape(-1), err_msg=name)
    D2, I2 = back.search(xq, K)
    np.testing.assert_array_equal(I2, I)
    np.testing.assert_array_equal(D2, D)
    pv = tmp_path / "pca.vt"
    faiss.write_VectorTransform(pca, str(pv))
    vt = faiss.read_VectorTransform(str(pv))
    assert type(vt) is faiss.PCAMatrix
    np.testing.assert_array_equal(vt.A, pca.A)
    np.testing.assert_array_equal(vt.apply(xq), O.linear_transform(xq, A, b))


FRONTS = {"PCA": (0.0, False), "PCAR": (0.0, True), "PCAW": (-0.5, False), "PCAWR": (-0.5, True)}
INNER = {"Flat": faiss.IndexFlat, "PQ8": faiss.IndexPQ, "PQ8x8": faiss.IndexPQ, "IVF8,PQ8": faiss.IndexIVFPQ,
         "IVF8,Flat": faiss.IndexIVFFlat, "SQ8": faiss.IndexScalarQuantizer, "SQfp16": faiss.IndexScalarQuantizer}


@pytest.mark.parametrize("front", sorted(FRONTS))
def test_factory_fronts_build_every_inner_key(front):
    power, rotate = FRONTS[front]
    for rest, cls in INNER.items():
        ix = faiss.index_factory(32, f"{front}16,{rest}")
        pca = ix.chain.at(0)
        assert type(ix) is faiss.IndexPreTransform and type(pca) is faiss.PCAMatrix, rest
        assert (pca.d_in, pca.d_out, pca.eigen_power, pca.random_rotation) == (32, 16, power, rotate), rest
        assert type(ix.index) is cls and ix.index.d == 16, rest
    # behind an OPQ front the two transforms form one chain
    ix = faiss.index_factory(32, f"{front}16,OPQ8,PQ8")
    assert [type(t) for t in ix.chain] == [faiss.PCAMatrix, faiss.OPQMatrix] and type(ix.index) is faiss.IndexPQ
