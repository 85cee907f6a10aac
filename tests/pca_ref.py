"""NumPy reference of faiss_amd.PCAMatrix for the tests: float64 moments, the host half of
training (the same numpy.linalg.eigh, descending order) and Faiss's prepare_Ab rules, written
independently of transform.py, plus the derived error bounds the GPU tests assert."""
import numpy as np

U32 = 2.0 ** -24  # the unit roundoff of fp32


def scatter_of_centred(x, mean32):
    """What the kernel is asked to sum: xc = x - mean in float32 (its own input), then
    S64 = xc^T xc in float64 and the bound matrix sum_r |xc_ri| |xc_rj|."""
    xc = np.asarray(x, np.float32) - np.asarray(mean32, np.float32)[None, :]
    assert xc.dtype == np.float32
    xc = xc.astype(np.float64)
    a = np.abs(xc)
    return xc.T @ xc, a.T @ a


def scatter_bound(n, chunks, absprod):
    """|S_gpu - S64|_ij <= (n + chunks + 2) 2^-24 sum_r |xc_ri| |xc_rj|: the standard bound of
    an fp32 sum of that many terms in any order, one rounding per product allowed for."""
    return (n + chunks + 2) * U32 * absprod


def eig_desc(scatter):
    """eigenvalues (descending) and the eigenvectors as rows, float64."""
    w, v = np.linalg.eigh(np.asarray(scatter, np.float64))
    return w[::-1].copy(), v[:, ::-1].T.copy()


def rotation(d_out, seed=1234):
    """The seeded random orthonormal matrix: QR of a default_rng(seed) normal matrix with the
    sign fix that makes R's diagonal positive, transposed (OPQMatrix.train's construction)."""
    q, r = np.linalg.qr(np.random.default_rng(seed).standard_normal((d_out, d_out)))
    return (q * np.sign(np.diag(r))[None, :]).T


def prepare_Ab(mean, eigenvalues, PCAMat, d_out, eigen_power=0.0, random_rotation=False, seed=1234):
    """A [d_out][d_in] float32 and b = -A mean (float64 accumulation, rounded once) from the
    float32 fields a trained PCAMatrix holds."""
    mean = np.asarray(mean, np.float32)
    ev = np.asarray(eigenvalues, np.float32).astype(np.float64)
    P = np.asarray(PCAMat, np.float32).astype(np.float64).reshape(mean.size, mean.size)
    A = P[:d_out]
    if eigen_power != 0:
        A = A * (ev[:d_out] ** eigen_power)[:, None]
    if random_rotation:
        A = rotation(d_out, seed) @ A
    A = A.astype(np.float32)
    b = -(A.astype(np.float64) @ mean.astype(np.float64))
    return A, b.astype(np.float32)


def train_from_moments(mean, scatter, d_out, eigen_power=0.0, random_rotation=False, seed=1234):
    """dict of mean, eigenvalues, PCAMat, A, b as PCAMatrix.train_from_moments leaves them."""
    w, P = eig_desc(scatter)
    out = {"mean": np.asarray(mean, np.float32), "eigenvalues": w.astype(np.float32), "PCAMat": P.astype(np.float32)}
    out["A"], out["b"] = prepare_Ab(out["mean"], out["eigenvalues"], out["PCAMat"], d_out, eigen_power,
                                    random_rotation, seed)
    return out
