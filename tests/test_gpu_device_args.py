"""The device entry points of every index family reject what their C functions would read or write out
of bounds, with RuntimeError, before anything reaches the library: the same table of bad arguments on
``search_device`` and ``add_device`` of the seven families and on ``search_preassigned_device`` of the
three IVF ones.  A rejected call changes nothing: ``ntotal`` stays, and the same good search returns the
same bits before and after.

One tiny index per family (d = 32, 64 bits for the binary one; nlist 4, M 8, 256 rows, 8 queries,
k = 4); the quantizers are installed with ``set_trained`` from a seeded generator, so nothing trains."""
import numpy as np
import pytest

import faiss_amd as faiss

pytestmark = pytest.mark.gpu

D, BITS, NLIST, M, NB, NQ, K, NPROBE = 32, 64, 4, 8, 256, 8, 4, 2
IVF = ("ivfpq", "ivfflat", "ivfsq")
FAMILIES = IVF + ("pq", "sq", "bin", "flat")

VARS = {  # sorted public keys of vars(index) at the commit before the shared bases
    "ivfpq": ["M", "d", "device", "invlists", "metric_type", "nbits", "niter_coarse", "niter_pq", "nlist",
              "parallel_mode", "pq", "quantizer", "seed", "verbose"],
    "ivfflat": ["d", "device", "invlists", "metric_type", "niter_coarse", "nlist", "parallel_mode", "quantizer",
                "seed", "verbose"],
    "ivfsq": ["by_residual", "d", "device", "invlists", "metric_type", "niter_coarse", "nlist", "parallel_mode",
              "qtype", "quantizer", "seed", "sq", "verbose"],
    "pq": ["M", "d", "device", "metric_type", "nbits", "niter_pq", "pq", "seed", "verbose"],
    "sq": ["code_size", "d", "device", "metric_type", "qtype", "sq", "verbose"],
    "bin": ["code_size", "d", "device", "metric_type", "query_batch_size", "use_heap", "verbose"],
    "flat": ["d", "device", "metric_type", "verbose"],
}


def build(family):
    rng = np.random.default_rng(20)
    xb = rng.standard_normal((NB, D)).astype(np.float32)
    xq = rng.standard_normal((NQ, D)).astype(np.float32)
    cent = rng.standard_normal((NLIST, D)).astype(np.float32)
    codebook = rng.standard_normal((M, 256, D // M)).astype(np.float32)
    sq_range = np.concatenate([xb.min(0), xb.max(0) - xb.min(0)])  # QT_8bit: vmin (d), vdiff (d)
    qt = faiss.ScalarQuantizer.QT_8bit
    if family == "ivfpq":
        ix = faiss.IndexIVFPQ(None, D, NLIST, M)
        ix.set_trained(cent, codebook)
    elif family == "pq":
        ix = faiss.IndexPQ(D, M)
        ix.set_trained(codebook)
    elif family == "ivfflat":
        ix = faiss.IndexIVFFlat(None, D, NLIST)
        ix.set_trained(cent)
    elif family == "sq":
        ix = faiss.IndexScalarQuantizer(D, qt)
        ix.set_trained(sq_range)
    elif family == "ivfsq":
        ix = faiss.IndexIVFScalarQuantizer(None, D, NLIST, qt)
        ix.set_trained(cent, sq_range)
    elif family == "bin":
        ix = faiss.IndexBinaryFlat(BITS)
        xb = rng.integers(0, 256, (NB, BITS // 8), dtype=np.uint8)
        xq = rng.integers(0, 256, (NQ, BITS // 8), dtype=np.uint8)
    else:
        ix = faiss.IndexFlatL2(D)
    ix.add(xb)
    if family in IVF:
        ix.nprobe = NPROBE
    return ix, xb, xq


@pytest.fixture(scope="module", params=FAMILIES)
def case(request):
    import torch

    ix, xb, xq = build(request.param)
    return request.param, ix, torch.from_numpy(xb).cuda(), torch.from_numpy(xq).cuda()


def bad_rows(x):
    """(what, argument) for a good [n, w] device argument x: each must be rejected."""
    import torch

    n, w = x.shape
    twice = torch.cat([x, x])
    assert twice[::2].shape == x.shape and x.t().contiguous().t().shape == x.shape
    return [("wrong dtype", x.to(torch.float16 if x.dtype == torch.float32 else torch.float32)),
            ("wrong column count", x[:, :w - 1].contiguous()),
            ("transposed", x.t()),
            ("transposed storage, right shape", x.t().contiguous().t()),
            ("strided slice of the rows", twice[::2]),
            ("strided slice of the columns", x[:, ::2]),
            ("one-dimensional", x.reshape(-1)),
            ("CPU tensor", x.cpu()),
            ("numpy array", x.cpu().numpy()),
            ("list", x.cpu().tolist())]


def rejected(what, fn, *args, **kw):
    """fn(*args, **kw) raises RuntimeError (any other exception fails the test as it is)."""
    try:
        fn(*args, **kw)
    except RuntimeError:
        return
    pytest.fail(f"{what}: accepted")


def test_vars(case):
    family, ix, _, _ = case
    assert sorted(k for k in vars(ix) if not k.startswith("_")) == VARS[family]


def test_bad_device_arguments_are_rejected_and_change_nothing(case):
    import torch

    family, ix, xb, xq = case
    ntotal = ix.ntotal
    dist = torch.int32 if family == "bin" else torch.float32
    D0, I0 = (t.cpu().numpy() for t in ix.search_device(xq, K))
    assert D0.shape == I0.shape == (NQ, K) and (I0 >= 0).any()

    for what, bad in bad_rows(xq):
        rejected(what, ix.search_device, bad, K)
    for what, bad in bad_rows(xb):
        rejected(what, ix.add_device, bad)
    rejected("D of the wrong shape", ix.search_device, xq, K, D=torch.empty((3, K), dtype=dist, device="cuda"))
    rejected("D of the wrong dtype", ix.search_device, xq, K,
             D=torch.empty((NQ, K), dtype=torch.float64, device="cuda"))
    rejected("I of the wrong dtype", ix.search_device, xq, K, I=torch.empty((NQ, K), dtype=torch.int32, device="cuda"))
    rejected("I on the host", ix.search_device, xq, K, I=torch.empty((NQ, K), dtype=torch.int64))
    for k in (0, 1025):
        rejected(f"k = {k}", ix.search_device, xq, k)
        rejected(f"k = {k}", ix.search, xq.cpu().numpy(), k)

    if family in IVF:
        Iq = torch.arange(NPROBE, device="cuda").repeat(NQ, 1)
        Dq = torch.zeros((NQ, NPROBE), device="cuda")
        P0 = [t.cpu().numpy() for t in ix.search_preassigned_device(xq, K, Iq, Dq)]
        for what, bad in bad_rows(xq):
            rejected(what, ix.search_preassigned_device, bad, K, Iq, Dq)
        short = NPROBE - 1
        rejected("Iq with nprobe - 1 columns", ix.search_preassigned_device, xq, K, Iq[:, :short].contiguous(), None)
        rejected("Iq of the wrong dtype", ix.search_preassigned_device, xq, K, Iq.int(), Dq)
        rejected("Iq a numpy array", ix.search_preassigned_device, xq, K, Iq.cpu().numpy(), Dq)
        rejected("Dq with nprobe - 1 columns", ix.search_preassigned_device, xq, K, Iq, Dq[:, :short].contiguous())
        rejected("D of the wrong shape", ix.search_preassigned_device, xq, K, Iq, Dq,
                 D=torch.empty((3, K), device="cuda"))
        rejected("I of the wrong dtype", ix.search_preassigned_device, xq, K, Iq, Dq,
                 I=torch.empty((NQ, K), dtype=torch.int32, device="cuda"))
        for k in (0, 1025):
            rejected(f"k = {k}", ix.search_preassigned_device, xq, k, Iq, Dq)
        ids = torch.arange(NB, device="cuda")
        rejected("ids of the wrong length", ix.add_device, xb, ids[:NB - 1])
        rejected("ids of the wrong dtype", ix.add_device, xb, ids.int())
        rejected("ids a numpy array", ix.add_device, xb, ids.cpu().numpy())
        P1 = [t.cpu().numpy() for t in ix.search_preassigned_device(xq, K, Iq, Dq)]
        np.testing.assert_array_equal(P1[0], P0[0])
        np.testing.assert_array_equal(P1[1], P0[1])

    assert ix.ntotal == ntotal == NB
    D1, I1 = (t.cpu().numpy() for t in ix.search_device(xq, K))
    assert D1.tobytes() == D0.tobytes() and I1.tobytes() == I0.tobytes()
