"""Vector pre-transforms: Faiss ``LinearTransform`` / ``OPQMatrix`` and
``IndexPreTransform``.

The reference's billion-scale indexes are "OPQ16,IVF262144,PQ16"
(``Chameleon/Faiss_experiments/bench_gpu_1bn.py:10-17``): an OPQ rotation
trained with the PQ (``bench_gpu_1bn.py:480-495``) is applied to every base
and query vector before the IVF-PQ, and the FPGA extraction reads the matrix
back out of the index (``my_faiss_extract_scripts/extract_FPGA_required_data.py:
162-165``: ``index.chain.at(0)`` -> ``A`` reshaped ``(d, d)``).

* ``apply`` runs on the GPU (``ivfpq_linear_transform_device``, k_linear_transform:
  a t-ordered fused-multiply-add chain, the order ``oracle.linear_transform``
  restates; Faiss's sgemm leaves the order to BLAS, so parity with Faiss itself
  is unpinned).
* ``OPQMatrix.train`` restates Faiss 1.7.1 ``OPQMatrix::train`` (centre the
  training set, random orthonormal start, then ``niter`` rounds of: rotate, PQ
  k-means (``niter_pq_0`` then ``niter_pq`` iterations, hot-started), encode /
  decode, orthogonal Procrustes by SVD).  It runs on the host in numpy/float64
  like Faiss's LAPACK path; its random start and k-means seeding are not Faiss's
  (Faiss is not importable here), so trained matrices are not Faiss's either.
* ``PCAMatrix.train`` takes the mean and the centred scatter matrix of the training rows on
  the GPU (``ivfpq_pca_moments_device``, csrc/pca_moments.hip: fp64 column sums, the scatter
  on the fp32 matrix cores in a fixed order) and the d x d eigendecomposition on the host in
  float64.  Faiss leaves its scatter's summation order to ssyrk, so trained
  matrices agree with Faiss's to rounding, not bit for bit.
"""
from __future__ import annotations

import ctypes
import warnings

import numpy as np

from . import _lib, faiss_io


class _Chain(list):
    """IndexPreTransform.chain: a list with the SWIG vector's ``at``
    (extract_FPGA_required_data.py:164)."""

    def at(self, i):
        return self[i]


def downcast_VectorTransform(vt):
    return vt


def write_VectorTransform(vt, path):
    """faiss.write_VectorTransform (bench_gpu_1bn.py:507): one "LTra" record, or "PcAm" for
    a PCAMatrix."""
    if not vt.is_trained:
        raise RuntimeError("write_VectorTransform: transform is not trained")
    with open(path, "wb") as f:
        f.write(_transform_bytes(vt))


def read_VectorTransform(path):
    """faiss.read_VectorTransform (bench_gpu_1bn.py:510) -> LinearTransform ("LTra") or
    PCAMatrix ("PcAm")."""
    with open(path, "rb") as f:
        t = faiss_io.parse_vector_transform(f.read())
    return _linear_from_dict(t)


def _linear_from_dict(t):
    if t.get("kind") == "pca":
        return _pca_from_dict(t)
    lt = LinearTransform(t["d_in"], t["d_out"], t["have_bias"])
    if t["is_trained"]:
        lt.set_matrix(t["A"], t["b"])
    return lt


class LinearTransform:
    """y = x A^T (+ b); A: [d_out][d_in] float32 (Faiss layout)."""

    def __init__(self, d_in=0, d_out=0, have_bias=False):
        self.d_in = int(d_in)
        self.d_out = int(d_out)
        self.have_bias = bool(have_bias)
        self.A = None
        self.b = None
        self.is_trained = False
        self._dev = {}

    def set_matrix(self, A, b=None):
        A = np.ascontiguousarray(A, np.float32).reshape(self.d_out, self.d_in)
        self.A = A
        self.b = None if b is None or not self.have_bias else np.ascontiguousarray(b, np.float32).reshape(self.d_out)
        self.is_trained = True
        self._dev = {}

    def _device_mats(self, device):
        import torch

        if device not in self._dev:
            AT = torch.from_numpy(np.ascontiguousarray(self.A.T)).to(f"cuda:{device}")
            b = torch.from_numpy(self.b).to(f"cuda:{device}") if self.b is not None else None
            self._dev[device] = (AT, b)
        return self._dev[device]

    def apply_device(self, x, stream=None):
        """x: torch float32 CUDA [n, d_in] -> y [n, d_out] on the same device (GPU kernel)."""
        import torch

        if not self.is_trained:
            raise RuntimeError("transform is not trained")
        if x.dim() != 2 or x.shape[1] != self.d_in or x.dtype != torch.float32 or not x.is_cuda:
            raise RuntimeError(f"apply_device: x must be a float32 CUDA tensor [n, {self.d_in}]")
        x = x.contiguous()
        AT, b = self._device_mats(x.device.index)
        cur = torch.cuda.current_stream(x.device)
        if stream is None or int(stream) == cur.cuda_stream:
            y = torch.empty((x.shape[0], self.d_out), dtype=torch.float32, device=x.device)
            s = cur.cuda_stream
        else:
            # a caller's stream: it waits for the current stream (x's producer, the
            # copies of AT and b), and y is allocated on it (the caching allocator
            # then never hands y's block to the current stream while it is in use);
            # x, AT and b are marked as used by it
            ext = torch.cuda.ExternalStream(int(stream), device=x.device)
            ext.wait_stream(cur)
            with torch.cuda.stream(ext):
                y = torch.empty((x.shape[0], self.d_out), dtype=torch.float32, device=x.device)
            for t in (x, AT, b):
                if t is not None:
                    t.record_stream(ext)
            s = int(stream)
        _lib.check(_lib.load().ivfpq_linear_transform_device(
            x.shape[0], self.d_in, self.d_out, AT.data_ptr(), b.data_ptr() if b is not None else None,
            x.data_ptr(), y.data_ptr(), ctypes.c_void_p(s)))
        return y

    def apply(self, x, device=0):
        """numpy [n, d_in] -> numpy [n, d_out], computed on GPU ``device``."""
        import torch

        x = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(f"cuda:{device}")
        y = self.apply_device(x)
        return y.cpu().numpy()

    apply_py = apply


class OPQMatrix(LinearTransform):
    """Faiss OPQMatrix(d, M, d2): an orthonormal rotation [d2][d] trained for M sub-quantizers."""

    def __init__(self, d=0, M=1, d2=-1):
        d2 = d if d2 == -1 else d2
        if d2 > d:
            raise RuntimeError("OPQMatrix: d_out > d_in is not supported")
        super().__init__(d, d2, False)
        self.M = int(M)
        self.niter = 50
        self.niter_pq = 4
        self.niter_pq_0 = 40
        self.max_train_points = 256 * 256
        self.seed = 1234
        if d2 % self.M:
            raise RuntimeError("OPQMatrix: d_out must be a multiple of M")

    @staticmethod
    def _pq_kmeans(xp, M, cb, niter, rng):
        n, d2 = xp.shape
        dsub = d2 // M
        for m in range(M):
            xs = xp[:, m * dsub:(m + 1) * dsub]
            if cb[m] is None:  # first round: 256 distinct training points
                cb[m] = xs[rng.choice(n, 256, replace=False)].copy()
            c = cb[m]
            for _ in range(niter):
                a = np.argmin((c * c).sum(1)[None, :] - 2.0 * xs @ c.T, axis=1)
                cnt = np.bincount(a, minlength=256)
                s = np.zeros_like(c)
                np.add.at(s, a, xs)
                nz = cnt > 0
                c[nz] = s[nz] / cnt[nz, None]  # empty centroids keep their position
        return cb

    @staticmethod
    def _pq_recons(xp, M, cb):
        n, d2 = xp.shape
        dsub = d2 // M
        out = np.empty_like(xp)
        for m in range(M):
            xs = xp[:, m * dsub:(m + 1) * dsub]
            c = cb[m]
            a = np.argmin((c * c).sum(1)[None, :] - 2.0 * xs @ c.T, axis=1)
            out[:, m * dsub:(m + 1) * dsub] = c[a]
        return out

    def train(self, x):
        x = np.ascontiguousarray(x, np.float32).reshape(-1, self.d_in)
        rng = np.random.default_rng(self.seed)
        if x.shape[0] > self.max_train_points:
            x = x[np.sort(rng.choice(x.shape[0], self.max_train_points, replace=False))]
        if x.shape[0] < 256:
            raise RuntimeError("OPQMatrix.train needs at least 256 training vectors")
        d, d2 = self.d_in, self.d_out
        xt = x.astype(np.float64)
        xt -= xt.mean(0, keepdims=True)
        if self.A is None:  # random orthonormal start, first d2 rows
            q, r = np.linalg.qr(rng.standard_normal((d, d)))
            A = (q * np.sign(np.diag(r))[None, :]).T[:d2].copy()
        else:
            A = self.A.astype(np.float64)
        cb = [None] * self.M
        for it in range(self.niter):
            xp = xt @ A.T
            cb = self._pq_kmeans(xp, self.M, cb, self.niter_pq_0 if it == 0 else self.niter_pq, rng)
            rec = self._pq_recons(xp, self.M, cb)
            u, _, vt = np.linalg.svd(xt.T @ rec, full_matrices=False)  # [d][d2] = U S V^T
            A = (u @ vt).T  # Procrustes: the rotation closest to mapping xt onto rec
        self.set_matrix(A.astype(np.float32))


def pca_moments_device(x, stream=None):
    """Column mean [d] and centred scatter matrix [d][d] (sum_r (x_r - mean)(x_r - mean)^T,
    not divided by n) of a torch float32 CUDA tensor [n, d], as torch tensors on its device
    (ivfpq_pca_moments_device: fp64 column sums, the scatter on the fp32 matrix cores)."""
    import torch

    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_cuda:
        raise RuntimeError("pca_moments_device: x must be a float32 CUDA tensor [n, d]")
    x = x.contiguous()
    n, d = x.shape
    cur = torch.cuda.current_stream(x.device)
    s = cur.cuda_stream if stream is None else int(stream)
    with torch.cuda.device(x.device):
        mean = torch.empty(d, dtype=torch.float32, device=x.device)
        scatter = torch.empty((d, d), dtype=torch.float32, device=x.device)
        if s != cur.cuda_stream:
            # a caller's stream: x's producer and any pending use of the outputs' blocks are on
            # the current stream; the call itself returns once `stream` has finished
            cur.synchronize()
        _lib.check(_lib.load().ivfpq_pca_moments_device(n, d, x.data_ptr(), mean.data_ptr(), scatter.data_ptr(),
                                                        ctypes.c_void_p(s)))
    return mean, scatter


def pca_plan(n, d):
    """How the scatter of n rows of d dimensions is split under the current chunk length
    (ivfpq_pca_get_plan; host arithmetic): dict of chunks, chunk_rows, tiles."""
    chunks, tiles, rows = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    _lib.check(_lib.load().ivfpq_pca_get_plan(int(n), int(d), ctypes.byref(chunks), ctypes.byref(rows),
                                              ctypes.byref(tiles)))
    return {"chunks": chunks.value, "chunk_rows": rows.value, "tiles": tiles.value}


def pca_set_chunk_rows(rows):
    """The scatter's row chunk (test hook ivfpq_pca_set_chunk_rows); 0 restores the default."""
    _lib.check(_lib.load().ivfpq_pca_set_chunk_rows(int(rows)))


class PCAMatrix(LinearTransform):
    """Faiss PCAMatrix(d_in, d_out, eigen_power, random_rotation): y = A (x - mean), A the
    first d_out principal directions, optionally whitened (eigen_power = -0.5) and followed by
    a random rotation (beir faiss_search.py:359-413; bench_gpu_1bn.py:490-492 "PCAR<dout>,";
    fairseq wav2vec/unsupervised/scripts/pca.py reads ``A`` and ``b`` back).

    ``train`` computes the mean and the scatter matrix on the GPU (csrc/pca_moments.hip) and
    the eigendecomposition on the host in float64 (numpy.linalg.eigh, Faiss's dsyev).  The
    scatter is the centred sum and is not divided by n, so ``eigenvalues`` are those of the
    scatter matrix.  Every n >= 1 takes this path (Faiss's Gram-matrix branch
    for n < d_in is an optimisation).  The apply is LinearTransform's."""

    def __init__(self, d_in=0, d_out=0, eigen_power=0.0, random_rotation=False):
        super().__init__(d_in, d_out, True)
        self.eigen_power = float(eigen_power)
        self.random_rotation = bool(random_rotation)
        self.balanced_bins = 0
        self.max_points_per_d = 1000
        self.seed = 1234
        self.mean = np.zeros(0, np.float32)
        self.eigenvalues = np.zeros(0, np.float32)
        self.PCAMat = np.zeros(0, np.float32)

    def _check_trainable(self):
        if self.balanced_bins != 0:
            raise RuntimeError("PCAMatrix: balanced_bins is not supported")
        if self.d_in < 1:
            raise RuntimeError("PCAMatrix: d_in must be at least 1")
        if self.d_out > self.d_in:
            raise RuntimeError(f"PCAMatrix: d_out = {self.d_out} > d_in = {self.d_in} (widening is not supported)")

    def _subsample(self, n):
        """The sorted rows train keeps of n (None: all), as OPQMatrix.train draws them."""
        cap = self.max_points_per_d * self.d_in
        if n <= cap:
            return None
        return np.sort(np.random.default_rng(self.seed).choice(n, cap, replace=False))

    def train(self, x, device=None):
        """x: numpy [n, d_in]; the kept rows are uploaded to GPU ``device`` for the moments."""
        import torch

        from .index import _default_device

        self._check_trainable()
        x = np.ascontiguousarray(x, np.float32).reshape(-1, self.d_in)
        if x.shape[0] < 1:
            raise RuntimeError("PCAMatrix.train needs at least one training vector")
        keep = self._subsample(x.shape[0])
        if keep is not None:
            x = x[keep]
        device = _default_device() if device is None else int(device)
        with warnings.catch_warnings():  # (a read-only array is only read: the tensor is copied to the device)
            warnings.simplefilter("ignore", UserWarning)
            xd = torch.from_numpy(x).to(f"cuda:{device}")
        self._train_moments_device(xd, None)

    def train_device(self, x, stream=None):
        """train with the vectors already in HBM (torch float32 CUDA tensor [n, d_in])."""
        import torch

        self._check_trainable()
        if x.dim() != 2 or x.shape[1] != self.d_in or x.dtype != torch.float32 or not x.is_cuda:
            raise RuntimeError(f"train_device: x must be a float32 CUDA tensor [n, {self.d_in}]")
        if x.shape[0] < 1:
            raise RuntimeError("PCAMatrix.train needs at least one training vector")
        keep = self._subsample(x.shape[0])
        if keep is not None:
            x = x.index_select(0, torch.from_numpy(keep).to(x.device))
        self._train_moments_device(x, stream)

    def _train_moments_device(self, x, stream):
        mean, scatter = pca_moments_device(x, stream)
        self.train_from_moments(mean.cpu().numpy(), scatter.cpu().numpy())

    def train_from_moments(self, mean, scatter):
        """The host half of train: mean [d_in] and the symmetric scatter (or covariance) matrix
        [d_in][d_in] -> eigenvalues (descending), PCAMat (rows = eigenvectors), A and b."""
        self._check_trainable()
        d = self.d_in
        mean = np.ascontiguousarray(mean, np.float32).reshape(-1)
        S = np.asarray(scatter, np.float64)
        if mean.size != d or S.shape != (d, d):
            raise RuntimeError(f"train_from_moments: mean must be [{d}] and scatter [{d}][{d}]")
        w, v = np.linalg.eigh(S)  # ascending, columns are eigenvectors
        self.mean = mean
        self.eigenvalues = np.ascontiguousarray(w[::-1], np.float32)
        self.PCAMat = np.ascontiguousarray(v[:, ::-1].T, np.float32)
        self.prepare_Ab()

    def prepare_Ab(self):
        """A and b from mean / eigenvalues / PCAMat (Faiss PCAMatrix::prepare_Ab without
        balanced_bins): the first d_out eigenvectors, each scaled by eigenvalue ** eigen_power,
        then the seeded random rotation; b = -A mean."""
        self._check_trainable()
        d, do = self.d_in, self.d_out
        if self.mean.size != d or self.eigenvalues.size != d or self.PCAMat.size != d * d:
            raise RuntimeError("prepare_Ab: mean / eigenvalues / PCAMat are not set")
        A = self.PCAMat.reshape(d, d)[:do].astype(np.float64)
        if self.eigen_power != 0:
            ev = self.eigenvalues[:do].astype(np.float64)
            if self.eigen_power < 0 and (ev <= 0).any():
                i = int(np.argmax(ev <= 0))
                raise RuntimeError(f"PCAMatrix: eigenvalue {i} is {ev[i]:g} <= 0, cannot be raised to the power "
                                   f"{self.eigen_power:g} (lower d_out or eigen_power)")
            A = A * (ev ** self.eigen_power)[:, None]
        if self.random_rotation:
            q, r = np.linalg.qr(np.random.default_rng(self.seed).standard_normal((do, do)))
            A = (q * np.sign(np.diag(r))[None, :]).T @ A
        A = A.astype(np.float32)
        b = -(A.astype(np.float64) @ self.mean.astype(np.float64))
        self.set_matrix(A, b.astype(np.float32))

    def copy_from(self, other):
        """Every field of ``other``; returns self (beir faiss_search.py:389 assigns it)."""
        for name in ("d_in", "d_out", "have_bias", "is_trained", "eigen_power", "random_rotation", "balanced_bins",
                     "max_points_per_d", "seed"):
            setattr(self, name, getattr(other, name))
        for name in ("A", "b", "mean", "eigenvalues", "PCAMat"):
            v = getattr(other, name)
            setattr(self, name, None if v is None else np.array(v, np.float32))
        self._dev = {}
        return self


def _pca_from_dict(t):
    p = PCAMatrix(t["d_in"], t["d_out"], t["eigen_power"], t["random_rotation"])
    p.balanced_bins = t["balanced_bins"]
    p.mean, p.eigenvalues, p.PCAMat = t["mean"], t["eigenvalues"], t["PCAMat"]
    if t["is_trained"]:
        p.set_matrix(t["A"], t["b"])
    return p


def _transform_bytes(vt):
    """One VectorTransform record: "PcAm" for a PCAMatrix, "LTra" for the others."""
    if isinstance(vt, PCAMatrix):
        return faiss_io.serialize_pca(vt.eigen_power, vt.random_rotation, vt.balanced_bins, vt.mean, vt.eigenvalues,
                                      vt.PCAMat, vt.A, vt.b, vt.d_in, vt.d_out, vt.is_trained)
    return faiss_io.serialize_linear(vt.A, vt.b, vt.d_in, vt.d_out, vt.is_trained)


class IndexPreTransform:
    """Faiss IndexPreTransform(chain, index): every vector is transformed on the GPU
    before the wrapped index sees it.  ``chain`` is a list of LinearTransform."""

    def __init__(self, chain, index):
        self.chain = _Chain(chain if isinstance(chain, (list, tuple)) else [chain])
        self.index = index
        self.d = self.chain[0].d_in
        self.metric_type = index.metric_type
        if self.chain[-1].d_out != index.d:
            raise RuntimeError("IndexPreTransform: the chain's output dimension differs from the index's")

    # Faiss attribute forwarding
    @property
    def ntotal(self):
        return self.index.ntotal

    @property
    def is_trained(self):
        return all(t.is_trained for t in self.chain) and self.index.is_trained

    @property
    def nprobe(self):
        return getattr(self.index, "nprobe", 1)  # an IndexPQ has no lists to probe

    @nprobe.setter
    def nprobe(self, p):
        if hasattr(self.index, "nprobe"):
            self.index.nprobe = p

    @property
    def device(self):
        return self.index.device

    def apply_chain(self, x):
        """numpy -> numpy through every transform (GPU)."""
        for t in self.chain:
            x = t.apply(x, self.index.device)
        return x

    def apply_chain_device(self, x, stream=None):
        for t in self.chain:
            x = t.apply_device(x, stream)
        return x

    def train(self, x):
        x = np.ascontiguousarray(x, np.float32).reshape(-1, self.d)
        for t in self.chain:
            if not t.is_trained:
                if isinstance(t, PCAMatrix):  # its moments run on the wrapped index's GPU
                    t.train(x, self.index.device)
                else:
                    t.train(x)
            x = t.apply(x, self.index.device)
        if not self.index.is_trained:
            self.index.train(x)

    def add(self, x):
        self.index.add(self.apply_chain(np.ascontiguousarray(x, np.float32).reshape(-1, self.d)))

    def add_with_ids(self, x, ids):
        self.index.add_with_ids(self.apply_chain(np.ascontiguousarray(x, np.float32).reshape(-1, self.d)), ids)

    def search(self, x, k):
        import torch

        xd = torch.from_numpy(np.ascontiguousarray(x, np.float32).reshape(-1, self.d)).to(f"cuda:{self.index.device}")
        D, I = self.search_device(xd, k)
        return D.cpu().numpy(), I.cpu().numpy()

    def search_device(self, x, k, D=None, I=None, stream=None):
        return self.index.search_device(self.apply_chain_device(x, stream), k, D, I, stream)

    # the rest of the IVF-PQ surface callers reach through an OPQ index
    # (faiss_server.py / faiss_retriever.py: coarse step, preassigned search, wire requests)
    def coarse_device(self, x, Iq=None, Dq=None, stream=None):
        return self.index.coarse_device(self.apply_chain_device(x, stream), Iq, Dq, stream)

    def search_preassigned_device(self, x, k, Iq, Dq=None, D=None, I=None, stream=None):
        return self.index.search_preassigned_device(self.apply_chain_device(x, stream), k, Iq, Dq, D, I, stream)

    def search_preassigned(self, *args):
        """Both forms of IndexIVFPQ.search_preassigned, on the transformed queries."""
        if len(args) >= 7:
            n, x, k, Iq, Dq, D, I = args[:7]
            xt = self.apply_chain(np.ascontiguousarray(x, np.float32).reshape(-1, self.d))
            return self.index.search_preassigned(n, xt, k, Iq, Dq, D, I, *args[7:])
        x, k, Iq = args[:3]
        xt = self.apply_chain(np.ascontiguousarray(x, np.float32).reshape(-1, self.d))
        return self.index.search_preassigned(xt, k, Iq, *args[3:])

    def serve_request(self, msg, batch_size, dim, with_lists=False, nprobe=None, out=None):
        """A wire request on the pre-transform dimension: the queries are decoded,
        transformed on the GPU and re-encoded for the wrapped index."""
        from . import wire

        if dim != self.d:
            raise RuntimeError(f"dim={dim} does not match the index (d={self.d})")
        np_ = int(self.index.nprobe if nprobe is None else nprobe)
        if with_lists:
            k, q, lists = wire.decode_request_with_lists(msg, batch_size, dim, np_)
            msg2 = wire.encode_request_with_lists(self.apply_chain(np.array(q)), lists, batch_size, self.index.d,
                                                  np_, k)
        else:
            k, q = wire.decode_request(msg, batch_size, dim)
            msg2 = wire.encode_request(self.apply_chain(np.array(q)), k, batch_size, self.index.d)
        return self.index.serve_request(msg2, batch_size, self.index.d, with_lists=with_lists, nprobe=nprobe, out=out)

    def reset(self):
        self.index.reset()
