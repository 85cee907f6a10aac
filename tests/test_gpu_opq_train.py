"""The resident OPQ trainer (csrc/opq_train.hip, csrc/opq.cpp) against float64 numpy.

Kernel cases use integer-valued rows in [-4, 4] whose columns sum to exactly zero (z, -z and a
zero row where n is odd: the fp64 mean is 0, centring changes nothing), integer codebooks in
[-4, 4] and the first d2 rows of a signed permutation as A.  Every product and sum is then exact
in fp32 (|cross| <= 16 n < 2^24) and distance ties fall to the first index on both sides, so the
comparisons are ``assert_array_equal``.  Shapes (n, d, d2, M, chunk_rows):
(37, 24, 16, 4, default) one partial K step; (300, 72, 40, 20, 64) dsub = 2, two row tiles,
five chunks, the last of 44 rows; (257, 130, 96, 8, 128) dsub = 12, sub-quantizer 5 across the
64-column tile edge, a last chunk of one row; (37, 10, 10, 2, default) dsub = 5, which has no
LDS assignment kernel and takes launch_pq_encode_flat.  Real values, every other width, centring
and a handle used more than once are tests/test_gpu_opq_assign.py and tests/test_gpu_opq_rounds.py.
"""
import ctypes
import functools

import numpy as np
import pytest

import faiss_amd as faiss
from faiss_amd import _lib
from faiss_amd.transform import OPQMatrix, opq_set_chunk_rows

pytestmark = pytest.mark.gpu

SHAPES = [(37, 24, 16, 4, 0), (300, 72, 40, 20, 64), (257, 130, 96, 8, 128), (37, 10, 10, 2, 0)]


def _p(a, t):
    return a.ctypes.data_as(t)


class Handle:
    def __init__(self, d, d2, M):
        self.L, self.h, self.shape = _lib.load(), _lib.c_handle(), (d, d2, M)
        _lib.check(self.L.ivfpq_opq_create(d, d2, M, 0, ctypes.byref(self.h)))

    def iterate(self, x, A, niter_pq, init=None, cb=None):
        d, d2, M = self.shape
        _lib.check(self.L.ivfpq_opq_set_rows(self.h, x.shape[0], _p(x, _lib.c_f32p)))
        if cb is not None:
            _lib.check(self.L.ivfpq_opq_set_codebook(self.h, _p(cb, _lib.c_f32p)))
        cross, out = np.empty((d, d2), np.float32), np.empty((M, 256, d2 // M), np.float32)
        _lib.check(self.L.ivfpq_opq_iterate(self.h, _p(A, _lib.c_f32p), niter_pq,
                                            None if init is None else _p(init, _lib.c_i64p), _p(cross, _lib.c_f32p)))
        _lib.check(self.L.ivfpq_opq_get_codebook(self.h, _p(out, _lib.c_f32p)))
        self.L.ivfpq_opq_free(self.h)
        return cross, out


def case(n, d, d2, M, seed=7):
    rng = np.random.default_rng(seed)
    z = rng.integers(-4, 5, (n // 2, d))
    x = np.concatenate([z, -z, np.zeros((n % 2, d), np.int64)])[rng.permutation(n)].astype(np.float32)
    A = np.zeros((d2, d), np.float32)
    A[np.arange(d2), rng.permutation(d)[:d2]] = rng.choice([-1.0, 1.0], d2)
    cb = rng.integers(-4, 5, (M, 256, d2 // M)).astype(np.float32)
    return rng, x, A, cb


def ref_codes(xp, cb):
    """[n][M] first argmin of sum (xp_m - c)^2 in float64."""
    M, _, dsub = cb.shape
    xs = xp.astype(np.float64).reshape(-1, M, 1, dsub)
    return np.argmin(((xs - cb.astype(np.float64)[None]) ** 2).sum(-1), axis=2)


@pytest.fixture
def chunked(request):
    n, d, d2, M, rows = request.param
    opq_set_chunk_rows(rows)
    yield n, d, d2, M
    opq_set_chunk_rows(0)


@pytest.mark.parametrize("chunked", SHAPES, indirect=True)
def test_cross_and_assign(chunked):
    n, d, d2, M = chunked
    _, x, A, cb = case(n, d, d2, M)
    cross, _ = Handle(d, d2, M).iterate(x, A, 0, cb=cb)
    codes = ref_codes(x @ A.T, cb)
    rec = cb.astype(np.float64)[np.arange(M)[None, :], codes].reshape(n, d2)
    np.testing.assert_array_equal(cross, x.astype(np.float64).T @ rec)


@pytest.mark.parametrize("chunked", SHAPES, indirect=True)
def test_lloyd_step(chunked):
    n, d, d2, M = chunked
    rng, x, A, cb = case(n, d, d2, M)
    xp = (x @ A.T).astype(np.float64)
    dsub, init = d2 // M, None
    if n >= 256:  # 256 distinct rows per sub-quantizer, as _pq_kmeans draws them
        init = np.concatenate([rng.choice(n, 256, replace=False) for _ in range(M)]).astype(np.int64)
        cb = np.stack([xp[init[m * 256:(m + 1) * 256], m * dsub:(m + 1) * dsub] for m in range(M)]).astype(np.float32)
    _, got = Handle(d, d2, M).iterate(x, A, 1, init=init, cb=None if init is not None else cb)
    codes, want = ref_codes(xp, cb), cb.copy()
    for m in range(M):
        xs = xp[:, m * dsub:(m + 1) * dsub]
        for j in np.unique(codes[:, m]):  # empty clusters keep their centroid
            want[m, j] = (xs[codes[:, m] == j].sum(0) / (codes[:, m] == j).sum()).astype(np.float32)
    np.testing.assert_array_equal(got, want)


def correlated(n, d, seed):
    """The rows of test_opq_train_rotation_is_orthonormal_and_helps: PQ on the raw axes wastes its sub-spaces."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, 8)).astype(np.float32) * np.linspace(8, 1, 8, dtype=np.float32)
    return (z @ rng.standard_normal((8, d)).astype(np.float32)
            + 0.05 * rng.standard_normal((n, d)).astype(np.float32)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def trained(entry, d=32, d2=-1):
    import torch

    x = correlated(4096, d, 2)
    opq = OPQMatrix(d, 4, d2)
    opq.niter, opq.niter_pq_0, opq.niter_pq = 6, 8, 2
    if entry == "train":
        opq.gpu = True
        opq.train(x)
    else:
        opq.train_device(torch.from_numpy(x).cuda())
    return x, opq.A


def pq_mse(x, M):
    rng = np.random.default_rng(5)
    cb = OPQMatrix._pq_kmeans(x.astype(np.float64), M, [None] * M, 10, rng)
    return float(((x - OPQMatrix._pq_recons(x.astype(np.float64), M, cb)) ** 2).sum(1).mean())


def test_training_is_orthonormal_and_helps():
    x, A = trained("train_device")
    assert A.shape == (32, 32)
    np.testing.assert_allclose(A.astype(np.float64) @ A.T, np.eye(32), atol=1e-5)
    xc = x - x.mean(0)
    rotated = (xc.astype(np.float64) @ A.T.astype(np.float64)).astype(np.float32)
    mse_rot, mse_raw = pq_mse(rotated, 4), pq_mse(xc, 4)
    print(f"PQ MSE rotated {mse_rot:.6g} raw {mse_raw:.6g}")
    assert mse_rot < 0.9 * mse_raw


def test_training_repeats_and_entry_points_agree():
    _, A = trained("train_device")
    np.testing.assert_array_equal(trained.__wrapped__("train_device")[1], A)
    np.testing.assert_array_equal(trained("train")[1], A)


# DESIGN.md 4j, "Tests": the PQ MSE (pq_mse of the centred rows under the trained rotation) of the host
# float64 trainer on correlated(4096, 32, 2), niter 6, niter_pq_0 8, niter_pq 2, at five seeds.  The
# seed-to-seed spread is the noise floor of the alternation; the device trainer at the first of these
# seeds must lie inside the host's range widened by its own width on each side.
HOST_SEEDS = (1234, 1, 2, 3, 4)
HOST_MSE = (243.41114847518844, 184.83728016427463, 246.85872539239386, 286.3353613916478, 206.79266249503348)
MSE_LO = min(HOST_MSE) - (max(HOST_MSE) - min(HOST_MSE))  # 83.339
MSE_HI = max(HOST_MSE) + (max(HOST_MSE) - min(HOST_MSE))  # 387.833


def rotated_mse(x, A):
    xc = x - x.mean(0)
    return pq_mse((xc.astype(np.float64) @ A.T.astype(np.float64)).astype(np.float32), 4)


@functools.lru_cache(maxsize=None)
def host_mse():
    """The five host trainings (CPU, float64), once per session."""
    x, out = correlated(4096, 32, 2), []
    for seed in HOST_SEEDS:
        opq = OPQMatrix(32, 4)
        opq.niter, opq.niter_pq_0, opq.niter_pq, opq.seed = 6, 8, 2, seed
        assert opq.gpu is False
        opq.train(x)
        out.append(rotated_mse(x, opq.A))
    return tuple(out)


def test_device_trainer_against_the_host_trainer():
    x, A = trained("train_device")  # opq.seed is HOST_SEEDS[0], the default
    assert OPQMatrix(32, 4).seed == HOST_SEEDS[0]
    dev, host = rotated_mse(x, A), host_mse()
    print(f"PQ MSE device {dev!r} host {host!r} interval [{MSE_LO:.3f}, {MSE_HI:.3f}]")
    assert MSE_LO <= dev <= MSE_HI
    lo, hi = min(host), max(host)  # the same rule from this session's host trainings
    assert 2 * lo - hi <= dev <= 2 * hi - lo
    assert all(MSE_LO <= v <= MSE_HI for v in host)  # the recorded interval still describes the host trainer


def test_training_reduced_output_dimension():
    _, A = trained("train_device", 48, 32)
    assert A.shape == (32, 48)
    np.testing.assert_allclose(A.astype(np.float64) @ A.T, np.eye(32), atol=1e-5)


def test_factory_path():
    x = correlated(2048, 32, 4)
    ix = faiss.index_factory(32, "OPQ8,PQ8")
    opq = ix.chain.at(0)
    opq.gpu, opq.niter, opq.niter_pq_0, opq.niter_pq = True, 3, 4, 2
    ix.train(x)
    assert ix.is_trained and "device_s" in opq.timing  # (the device path ran)
    np.testing.assert_allclose(opq.A.astype(np.float64) @ opq.A.T, np.eye(32), atol=1e-5)
    ix.add(x)
    D, I = ix.search(x[:16], 4)
    assert I.shape == (16, 4) and ix.ntotal == 2048 and (I >= 0).all() and (np.diff(D, axis=1) >= 0).all()

