"""GpuIndexFlat / GpuIndexFlatL2 / GpuIndexFlatIP with useFloat16 (csrc/flat_scan_f16.hip) against
float64 arithmetic on the half-rounded inputs: L2 = max(0, |x|^2 + |y|^2 - 2 x.y), inner product
x.y, the k best ordered by (key, label), missing results (+-FLT_MAX, -1).  On small integers every
fp32 sum is exact in any order, so results must be equal, ties included; on real-valued data the
bound is derived from the fp32 sums (below).  set_range_rows cuts the base into several ranges."""
import functools

import numpy as np
import pytest

import faiss_amd as faiss

pytestmark = pytest.mark.gpu

IP, L2 = faiss.METRIC_INNER_PRODUCT, faiss.METRIC_L2
METRICS = [pytest.param(IP, id="ip"), pytest.param(L2, id="l2")]
FMAX = np.finfo(np.float32).max


def h(a):
    return np.asarray(a).astype(np.float16).astype(np.float64)


def ref_keys(xq, xb, metric):
    """float64 keys [nq][nb] of the rounded inputs (inner product: the negated similarity)."""
    x, y = h(xq), h(xb)
    if metric == IP:
        return -(x @ y.T)
    return np.maximum(0.0, (x * x).sum(1)[:, None] + (y * y).sum(1)[None, :] - 2.0 * (x @ y.T))


def ref_search(xq, xb, k, metric):
    keys = ref_keys(xq, xb, metric)
    I = np.argsort(keys, axis=1, kind="stable")[:, :k]  # stable: ties by label
    D = np.take_along_axis(keys, I, 1) * (-1.0 if metric == IP else 1.0)
    pad = k - I.shape[1]
    D = np.pad(D, ((0, 0), (0, pad)), constant_values=-FMAX if metric == IP else FMAX)
    return D.astype(np.float32), np.pad(I, ((0, 0), (0, pad)), constant_values=-1)


def half_index(d, metric, range_rows=0):
    cfg = faiss.GpuIndexFlatConfig()
    cfg.useFloat16 = True
    ix = faiss.GpuIndexFlat(faiss.StandardGpuResources(), d, metric, cfg)
    ix.set_range_rows(range_rows)
    return ix


def search_device(ix, xq, k, stream=None):
    import torch

    D, I = ix.search_device(torch.from_numpy(xq).cuda(), k, stream=stream)
    torch.cuda.synchronize()
    return D.cpu().numpy(), I.cpu().numpy()


# ------------------------------------------------------------------ exact on integers
# (d, nb, nq, k, range_rows): every value of every axis of the issue at least once
INT_CASES = [(1, 1, 1, 1, 0), (7, 127, 16, 10, 0), (32, 129, 17, 64, 128), (40, 3001, 65, 65, 512),
             (136, 3001, 65, 256, 640), (136, 3001, 17, 257, 512), (40, 3001, 16, 1024, 1024), (7, 127, 1, 256, 0),
             (32, 1, 65, 10, 0), (136, 129, 1, 1024, 0), (1, 3001, 17, 1, 256)]


@pytest.mark.parametrize("d,nb,nq,k,rows", INT_CASES, ids=["-".join(map(str, c)) for c in INT_CASES])
@pytest.mark.parametrize("metric", METRICS)
def test_integers_equal_the_reference(metric, d, nb, nq, k, rows):
    rng = np.random.default_rng(d * 1000 + nb + nq + k)
    xb = rng.integers(-3, 4, (nb, d)).astype(np.float32)
    xq = rng.integers(-3, 4, (nq, d)).astype(np.float32)
    ix = half_index(d, metric, rows)
    ix.add(xb)
    D, I = ix.search(xq, k)
    Dr, Ir = ref_search(xq, xb, k, metric)
    np.testing.assert_array_equal(I, Ir)
    np.testing.assert_array_equal(D, Dr)


# ------------------------------------------------------------------ real-valued data
@functools.lru_cache(maxsize=None)
def real_case(metric):
    """nb = 3001 in six ranges (the last ragged), nq = 37, d = 136.  Inner product: data in
    [1/16, 1), all products non-negative, so an fp32 sum of the d exact products is within
    (d - 1) 2^-24 relative of the float64 sum in any order: rtol = 1e-4, atol = 0.  L2: standard
    normal data; the three terms carry at most 2 (|x|^2 + |y|^2) and (d + 3) 2^-24 2 < 1e-4, so
    atol = 1e-4 (|x|^2 + |y|^2) per entry.  Returns (index, xq, float64 keys, tolerances)."""
    rng = np.random.default_rng(7 + metric)
    if metric == IP:
        xb, xq = rng.uniform(1 / 16, 1, (3001, 136)), rng.uniform(1 / 16, 1, (37, 136))
    else:
        xb, xq = rng.standard_normal((3001, 136)), rng.standard_normal((37, 136))
    xb, xq = xb.astype(np.float32), xq.astype(np.float32)
    ix = half_index(136, metric, 512)
    ix.add(xb)
    keys = ref_keys(xq, xb, metric)
    tol = 1e-4 * (np.abs(keys) if metric == IP else (h(xq) ** 2).sum(1)[:, None] + (h(xb) ** 2).sum(1)[None, :])
    keys.setflags(write=False)
    tol.setflags(write=False)
    return ix, xq, keys, tol


@pytest.mark.parametrize("k", [10, 100, 1000])
@pytest.mark.parametrize("metric", METRICS)
def test_real_data_within_the_derived_bound(metric, k):
    ix, xq, keys, tol = real_case(metric)
    D, I = ix.search(xq, k)
    Dk = -D.astype(np.float64) if metric == IP else D.astype(np.float64)
    assert ((I >= 0) & (I < keys.shape[1])).all()
    assert all(len(set(row)) == k for row in I.tolist())
    assert (np.diff(Dk, axis=1) >= 0).all()
    assert (np.abs(Dk - np.take_along_axis(keys, I, 1)) <= np.take_along_axis(tol, I, 1)).all()
    missed = np.ones(keys.shape, bool)
    np.put_along_axis(missed, I, False, 1)
    assert (~missed | (keys >= Dk[:, -1:] - tol)).all()  # nothing better was left out


# ------------------------------------------------------------------ surface
@pytest.mark.parametrize("metric", METRICS)
def test_add_paths_agree_and_hold_the_rounded_rows(metric):
    import torch

    rng = np.random.default_rng(11)
    x = rng.standard_normal((700, 24)).astype(np.float32)
    xq = rng.standard_normal((19, 24)).astype(np.float32)
    one, chunks, dev = (half_index(24, metric, 256) for _ in range(3))
    one.add(x)
    for lo in range(0, 700, 300):
        chunks.add(x[lo:lo + 300])
    dev.add_device(torch.from_numpy(x[:400]).cuda())
    dev.add_device(torch.from_numpy(x[400:]).cuda())
    want = one.search(xq, 70)
    for ix in (one, chunks, dev):
        assert ix.ntotal == 700
        np.testing.assert_array_equal(ix.xb.reshape(700, 24), h(x))
        np.testing.assert_array_equal(ix.reconstruct(699), h(x[699]))
        for got in (ix.search(xq, 70), search_device(ix, xq, 70),
                    search_device(ix, xq, 70, stream=torch.cuda.Stream().cuda_stream)):
            np.testing.assert_array_equal(got[1], want[1])
            np.testing.assert_array_equal(got[0], want[0])
    one.reset()
    assert one.ntotal == 0
    one.add(x[:5])
    np.testing.assert_array_equal(one.search(xq, 5)[1], ref_search(xq, x[:5], 5, metric)[1])


@pytest.mark.parametrize("metric", METRICS)
def test_empty_index_returns_the_padding(metric):
    ix = half_index(8, metric)
    xq = np.ones((3, 8), np.float32)
    for D, I in (ix.search(xq, 4), search_device(ix, xq, 4)):
        assert (I == -1).all() and (D == (-FMAX if metric == IP else FMAX)).all()


def test_files_default_config_and_the_reference_script(tmp_path):
    rng = np.random.default_rng(5)
    xb = rng.standard_normal((300, 16)).astype(np.float32)
    xq = rng.standard_normal((9, 16)).astype(np.float32)
    ix = half_index(16, L2)
    ix.add(xb)
    faiss.write_index(ix, str(tmp_path / "half.index"))
    back = faiss.read_index(str(tmp_path / "half.index"))
    assert isinstance(back, faiss.IndexFlat) and not isinstance(back, faiss.GpuIndexFlat) and back.metric_type == L2
    np.testing.assert_array_equal(back.xb, ix.xb)

    res = faiss.StandardGpuResources()
    plain, default = faiss.IndexFlatL2(16), faiss.GpuIndexFlatL2(res, 16)
    plain.add(xb)
    default.add(xb)
    for a, b in zip(plain.search(xq, 12), default.search(xq, 12)):
        np.testing.assert_array_equal(a, b)

    # bench_gpu_sift1m.py, exact-search section
    d = 16
    flat_config = faiss.GpuIndexFlatConfig()
    flat_config.device = 0
    index = faiss.GpuIndexFlatL2(res, d, flat_config)
    index.add(xb)
    D, I = index.search(xq, 123)
    assert D.shape == I.shape == (9, 123)
    np.testing.assert_array_equal(I, plain.search(xq, 123)[1])
