"""Faiss binary index files for IndexIVFPQ.

Chameleon's harnesses persist trained/populated indexes with ``faiss.write_index``
and load them with ``faiss.read_index`` (``Chameleon/Faiss_experiments/
bench_polysemous_1bn.py:287, 290``; beir ``faiss_index.py:29``; the FPGA data
extraction reads such files, ``my_faiss_extract_scripts/extract_FPGA_required_data.py:
174-248``).  This module reads and writes that layout so those files move between
Faiss and faiss_amd unchanged.

The layout is restated from upstream Faiss 1.7.1 ``impl/index_write.cpp`` /
``index_read.cpp`` (not vendored in the reference, not installed here), little-endian:

    "IwPQ"                                   IndexIVFPQ (non-legacy inverted lists)
      index header: d i32, ntotal i64, 2 x dummy i64 (1 << 20), is_trained u8, metric_type i32
                    [metric_arg f32 if metric_type > 1]
      nlist u64, nprobe u64
      quantizer:   "IxF2" (L2) | "IxFI" (IP), index header, xb = u64 count + f32[count]
      direct map:  type u8 (0 = none), array = u64 count + i64[count]
      by_residual u8, code_size u64
      PQ:          d u64, M u64, nbits u64, centroids = u64 count + f32[count]   ([M][ksub][dsub])
      "ilar", nlist u64, code_size u64,
        "full" + u64 count + u64 sizes[nlist]   |   "sprs" + u64 count + u64 (list, size) pairs
        per non-empty list: codes u8[n * code_size], then ids i64[n]

    "IxPT"                                   IndexPreTransform (the OPQ front of "OPQ16,IVF..,PQ16")
      index header (d = the chain's d_in), nt i32, nt x VectorTransform, then the wrapped index
      VectorTransform "LTra" (LinearTransform, and OPQMatrix, which Faiss writes as a plain
      LinearTransform): have_bias u8, A = u64 count + f32[d_out * d_in], b = u64 count + f32[count],
      d_in i32, d_out i32, is_trained u8
      VectorTransform "PcAm" (PCAMatrix; beir faiss_search.py:359-413, the "PCAR<dout>," front of
      bench_gpu_1bn.py:490-492): eigen_power f32, random_rotation u8, balanced_bins i32,
      mean = u64 count + f32[d_in], eigenvalues = u64 count + f32[d_in], PCAMat = u64 count +
      f32[d_in * d_in], then the "LTra" body above from have_bias on.  The 1.7.1 layout: later
      Faiss versions insert an epsilon f32 after eigen_power.  The wrapped index may also be an
      "IxF2" / "IxFI" flat index (beir's PCAFaissSearch over IndexFlatIP).

    "IxPq"                                  IndexPQ (beir faiss_search.py:168-224)
      index header
      PQ:          d u64, M u64, nbits u64, centroids = u64 count + f32[count]   ([M][ksub][dsub])
      codes = u64 count + u8[ntotal * code_size]
      search_type i32 (0 = ST_PQ), encode_signs u8 (0), polysemous_ht i32 (0)
    "IxPT" may wrap it in place of the IndexIVFPQ.

    "IwFl"                                   IndexIVFFlat (bench_gpu_1bn.py:575-578 ",Flat" keys)
      the IVF header of "IwPQ": index header, nlist u64, nprobe u64, quantizer, direct map
      "ilar" as above with code_size = 4 * d: a list's codes are its fp32 vectors
      (no by_residual / code_size / PQ block)
    Unpinned like the others: no Faiss-written "IwFl" file exists on the build machine.

    "IwSq"                                   IndexIVFScalarQuantizer ("IVF<nlist>,SQ8" / ",SQfp16" keys)
      the IVF header of "IwPQ": index header, nlist u64, nprobe u64, quantizer, direct map
      SQ block of "IxSQ" below (qtype, rangestat, rangestat_arg, d, code_size, trained)
      code_size u64, by_residual u8
      "ilar" as above with that code size
    Unpinned like the others: no Faiss-written "IwSq" file exists on the build machine.

    "IxSQ"                                   IndexScalarQuantizer (beir faiss_search.py:415-459)
      index header
      SQ:          qtype i32, rangestat i32 (0 = RS_minmax), rangestat_arg f32 (0), d u64, code_size u64,
                   trained = u64 count + f32[count]   ([vmin (d), vdiff (d)] | [vmin, vdiff] | empty)
      codes = u64 count + u8[ntotal * code_size]
    "IxPT" may wrap it too.
    Unpinned like the others: no Faiss-written "IxSQ" file exists on the build machine.

    "IxF2" (L2) | "IxFI" (IP)                IndexFlatL2 / IndexFlatIP as a file of its own (beir
                                             faiss_index.py:29 save / load of the FlatIP index of
                                             faiss_search.py:337)
      index header
      xb = u64 count + f32[ntotal * d]
    The record the IVF files embed as their quantizer; an IndexFlat(d, metric) is written under the
    fourcc of its metric and read back as IndexFlatL2 / IndexFlatIP, as Faiss does.
    Unpinned like the others: no Faiss-written "IxF2" / "IxFI" file exists on the build machine.

    "IBxF"                                   IndexBinaryFlat (beir faiss_search.py BinaryFaissSearch;
                                             written by write_index_binary, read by read_index_binary)
      d i32 (bits), code_size i32 (d / 8), ntotal i64, is_trained u8, metric_type i32 (1)
      xb = u64 count + u8[ntotal * code_size]
    A binary index has its own header (no dummies) and its own reader: read_index rejects it,
    read_index_binary rejects the float layouts, each naming the fourcc.
    Unpinned like the others: no Faiss-written "IBxF" file exists on the build machine.

Parity is unpinned: no Faiss-written file exists in the reference or this image
(the reference's ``*.index`` files are not shipped), so the tests check a
hand-assembled byte layout and round trips, not a file from real Faiss.
"""
from __future__ import annotations

import struct

import numpy as np

FOURCC_IVFPQ = b"IwPQ"
FOURCC_PQ = b"IxPq"
FOURCC_IVFFLAT = b"IwFl"
FOURCC_SQ = b"IxSQ"
FOURCC_IVFSQ = b"IwSq"
SQ_QT_8BIT, SQ_QT_8BIT_UNIFORM, SQ_QT_FP16 = 0, 2, 4  # the scalar quantizer types that are read and written
FOURCC_BINARY_FLAT = b"IBxF"
FOURCC_FLAT = {0: b"IxFI", 1: b"IxF2"}  # metric_type: 0 = INNER_PRODUCT, 1 = L2
HEADER_DUMMY = 1 << 20


FOURCC_PRETRANSFORM = b"IxPT"
FOURCC_LINEAR = b"LTra"
FOURCC_PCA = b"PcAm"


def is_faiss_file(path) -> bool:
    with open(path, "rb") as f:
        return f.read(4) in (FOURCC_IVFPQ, b"IvPQ", FOURCC_PRETRANSFORM, FOURCC_PQ, FOURCC_IVFFLAT, FOURCC_SQ, FOURCC_IVFSQ,
                             FOURCC_FLAT[0], FOURCC_FLAT[1])


class _Reader:
    def __init__(self, buf: bytes):
        self.b = memoryview(buf)
        self.o = 0

    def take(self, n):
        if self.o + n > len(self.b):
            raise RuntimeError("Faiss index file is truncated")
        v = self.b[self.o:self.o + n]
        self.o += n
        return v

    def fmt(self, f):
        return struct.unpack("<" + f, self.take(struct.calcsize("<" + f)))[0]

    def fourcc(self):
        return bytes(self.take(4))

    def vector(self, dtype):
        n = self.fmt("Q")
        it = np.dtype(dtype).itemsize
        return np.frombuffer(self.take(n * it), dtype=dtype).copy()

    def header(self):
        d = self.fmt("i")
        ntotal = self.fmt("q")
        self.fmt("q")
        self.fmt("q")
        is_trained = self.fmt("B") != 0
        metric = self.fmt("i")
        if metric > 1:
            self.fmt("f")
        return d, ntotal, is_trained, metric


def parse_ivfpq(buf: bytes) -> dict:
    """Faiss IndexIVFPQ bytes -> {d, nlist, nprobe, M, nbits, metric, is_trained,
    centroids [nlist][d], codebook [M][ksub][dsub], lists: [(ids i64[n], codes u8[n][code_size])]}."""
    r = _Reader(buf)
    z = _parse_ivfpq(r, r.fourcc())
    if r.o != len(r.b):
        raise RuntimeError("trailing bytes after the index")
    return z


def parse_index(buf: bytes) -> dict:
    """IndexIVFPQ or IndexPreTransform(LinearTransform..., IndexIVFPQ) bytes.
    IVF-PQ -> parse_ivfpq's dict with kind "ivfpq"; pre-transform -> {kind
    "pretransform", d, ntotal, metric, chain: [{A [d_out][d_in], b, have_bias,
    d_in, d_out, is_trained}], index: the IVF-PQ dict}; IndexPQ -> kind "pq";
    IndexIVFFlat -> kind "ivfflat" (_parse_ivfflat); IndexScalarQuantizer -> kind "sq" (_parse_sq);
    IndexIVFScalarQuantizer -> kind "ivfsq" (_parse_ivfsq);
    a top-level IndexFlatL2 / IndexFlatIP -> kind "flat" (_parse_flat)."""
    r = _Reader(buf)
    h = r.fourcc()
    if h in FOURCC_FLAT.values():
        z = _parse_flat(r, h)
    elif h == FOURCC_PRETRANSFORM:
        d, ntotal, is_trained, metric = r.header()
        nt = r.fmt("i")
        chain = [_parse_linear(r) for _ in range(nt)]
        if not chain or chain[0]["d_in"] != d:
            raise RuntimeError("pre-transform chain does not match the index dimension")
        sub = _parse_sub(r, r.fourcc())
        if sub["d"] != chain[-1]["d_out"]:
            raise RuntimeError("pre-transform output dimension does not match the wrapped index")
        z = {"kind": "pretransform", "d": d, "ntotal": ntotal, "metric": metric, "chain": chain, "index": sub}
    else:
        z = _parse_sub(r, h)
    if r.o != len(r.b):
        raise RuntimeError("trailing bytes after the index")
    return z


def _parse_sub(r: "_Reader", h: bytes) -> dict:
    if h in FOURCC_FLAT.values():
        return _parse_flat(r, h)
    if h == FOURCC_IVFFLAT:
        return _parse_ivfflat(r)
    if h == FOURCC_SQ:
        return _parse_sq(r)
    if h == FOURCC_IVFSQ:
        return _parse_ivfsq(r)
    return _parse_pq(r) if h == FOURCC_PQ else _parse_ivfpq(r, h)


def _parse_flat(r: "_Reader", h: bytes) -> dict:
    """IndexFlatL2 / IndexFlatIP after its fourcc -> {kind "flat", d, ntotal, metric, is_trained,
    xb f32 [ntotal][d]}; the metric is the fourcc's, which the header must repeat."""
    metric = 1 if h == FOURCC_FLAT[1] else 0
    d, ntotal, is_trained, hm = r.header()
    xb = r.vector(np.float32)
    if d <= 0 or ntotal < 0:
        raise RuntimeError(f"IndexFlat header is invalid (d = {d}, ntotal = {ntotal})")
    if hm != metric:
        raise RuntimeError(f"IndexFlat fourcc {h!r} does not match metric_type {hm}")
    if xb.size != ntotal * d:
        raise RuntimeError(f"IndexFlat xb holds {xb.size} floats, ntotal * d = {ntotal * d}")
    return {"kind": "flat", "d": d, "ntotal": ntotal, "metric": metric, "is_trained": is_trained,
            "xb": xb.reshape(ntotal, d)}


def serialize_flat(d, metric, xb) -> bytes:
    """The inverse of parse_index for kind "flat": xb float32 [ntotal][d].
    Unpinned against Faiss, like the other layouts (see the module docstring)."""
    if metric not in FOURCC_FLAT:
        raise RuntimeError(f"IndexFlat: unknown metric {metric}")
    xb = np.ascontiguousarray(xb, np.float32).reshape(-1)
    if d <= 0 or xb.size % d:
        raise RuntimeError(f"xb must hold whole rows of {d} floats")
    return b"".join([FOURCC_FLAT[metric], _header(d, xb.size // d, True, metric), _vector(xb)])


def _parse_pq(r: "_Reader") -> dict:
    """IndexPQ after its fourcc -> {kind "pq", d, ntotal, M, nbits, metric, is_trained,
    codebook [M][ksub][dsub], codes u8 [ntotal][code_size]}."""
    d, ntotal, is_trained, metric = r.header()
    pd = r.fmt("Q")
    M = r.fmt("Q")
    nbits = r.fmt("Q")
    cb = r.vector(np.float32)
    codes = r.vector(np.uint8)
    search_type = r.fmt("i")
    r.fmt("B")  # encode_signs
    r.fmt("i")  # polysemous_ht
    if pd != d or nbits != 8 or M == 0 or d % M or (is_trained and cb.size != M * 256 * (d // M)):
        raise RuntimeError("unsupported PQ shape (8-bit codes)")
    if search_type != 0:
        raise RuntimeError("only IndexPQ search_type ST_PQ is supported")
    if codes.size != ntotal * M:
        raise RuntimeError("IndexPQ codes do not match ntotal")
    return {"kind": "pq", "d": d, "ntotal": ntotal, "M": M, "nbits": nbits, "metric": metric,
            "is_trained": is_trained, "codebook": cb.reshape(M, 256, d // M) if cb.size else cb,
            "codes": codes.reshape(ntotal, M)}


def parse_pq(buf: bytes) -> dict:
    """Faiss IndexPQ ("IxPq") bytes -> _parse_pq's dict."""
    r = _Reader(buf)
    if r.fourcc() != FOURCC_PQ:
        raise RuntimeError("not a Faiss IndexPQ file")
    z = _parse_pq(r)
    if r.o != len(r.b):
        raise RuntimeError("trailing bytes after the index")
    return z


def serialize_pq(d, M, nbits, metric, codebook, codes, is_trained=True) -> bytes:
    """The inverse of parse_pq: codes uint8 [ntotal][M]."""
    codes = np.ascontiguousarray(codes, np.uint8).reshape(-1)
    code_size = M * nbits // 8
    return b"".join([FOURCC_PQ, _header(d, codes.size // code_size, is_trained, metric),
                     struct.pack("<QQQ", d, M, nbits),
                     _vector(np.ascontiguousarray(codebook, np.float32).reshape(-1)), _vector(codes),
                     struct.pack("<iBi", 0, 0, 0)])


def sq_shape(qtype, d):
    """(code_size, len(trained)) of a supported scalar quantizer type."""
    if qtype == SQ_QT_FP16:
        return 2 * d, 0
    if qtype == SQ_QT_8BIT:
        return d, 2 * d
    if qtype == SQ_QT_8BIT_UNIFORM:
        return d, 2
    raise RuntimeError(f"unsupported scalar quantizer type {qtype} (QT_fp16, QT_8bit, QT_8bit_uniform)")


def _parse_sq_block(r: "_Reader"):
    """The ScalarQuantizer record -> (qtype, d, code_size, trained, rangestat)."""
    qtype = r.fmt("i")
    rangestat = r.fmt("i")
    r.fmt("f")  # rangestat_arg
    sd = r.fmt("Q")
    code_size = r.fmt("Q")
    return qtype, sd, code_size, r.vector(np.float32), rangestat


def _check_sq_block(qtype, d, sd, code_size, trained, rangestat, is_trained):
    """The record against the index that holds it (checked once the index is read to its end,
    so that a truncated file is reported as truncated); returns the code size."""
    cs, nt = sq_shape(qtype, d)
    if rangestat != 0:
        raise RuntimeError("only the RS_minmax range statistic is supported")
    if sd != d or code_size != cs or (is_trained and trained.size != nt):
        raise RuntimeError("scalar quantizer shape does not match the index")
    return cs


def _sq_block(d, qtype, trained) -> bytes:
    cs, _ = sq_shape(qtype, d)
    return struct.pack("<iifQQ", qtype, 0, 0.0, d, cs) + _vector(np.ascontiguousarray(trained, np.float32).reshape(-1))


def _parse_sq(r: "_Reader") -> dict:
    """IndexScalarQuantizer after its fourcc -> {kind "sq", d, ntotal, qtype, metric, is_trained,
    code_size, trained f32[...], codes u8 [ntotal][code_size]}."""
    d, ntotal, is_trained, metric = r.header()
    qtype, sd, code_size, trained, rangestat = _parse_sq_block(r)
    codes = r.vector(np.uint8)
    cs = _check_sq_block(qtype, d, sd, code_size, trained, rangestat, is_trained)
    if codes.size != ntotal * cs:
        raise RuntimeError("IndexScalarQuantizer codes do not match ntotal")
    return {"kind": "sq", "d": d, "ntotal": ntotal, "qtype": qtype, "metric": metric, "is_trained": is_trained,
            "code_size": cs, "trained": trained, "codes": codes.reshape(ntotal, cs)}


def serialize_sq(d, qtype, metric, trained, codes, is_trained=True) -> bytes:
    """The inverse of parse_index for kind "sq": codes uint8 [ntotal][code_size].
    Unpinned against Faiss, like the other layouts (see the module docstring)."""
    cs, _ = sq_shape(qtype, d)
    codes = np.ascontiguousarray(codes, np.uint8).reshape(-1)
    return b"".join([FOURCC_SQ, _header(d, codes.size // cs, is_trained, metric), _sq_block(d, qtype, trained),
                     _vector(codes)])


def parse_index_binary(buf: bytes) -> dict:
    """Faiss IndexBinaryFlat ("IBxF") bytes -> {kind "binary_flat", d (bits), code_size, ntotal,
    is_trained, metric, codes u8 [ntotal][code_size]}."""
    r = _Reader(buf)
    h = r.fourcc()
    if h != FOURCC_BINARY_FLAT:
        raise RuntimeError(f"not a Faiss binary index file (fourcc {h!r}; IndexBinaryFlat {FOURCC_BINARY_FLAT!r} "
                           "only - float indexes are read with read_index)")
    d = r.fmt("i")
    code_size = r.fmt("i")
    ntotal = r.fmt("q")
    is_trained = r.fmt("B") != 0
    metric = r.fmt("i")
    codes = r.vector(np.uint8)
    if d <= 0 or d % 8 or code_size != d // 8:
        raise RuntimeError("IndexBinaryFlat code size does not match d")
    if ntotal < 0 or codes.size != ntotal * code_size:
        raise RuntimeError("IndexBinaryFlat xb does not match ntotal")
    if r.o != len(r.b):
        raise RuntimeError("trailing bytes after the index")
    return {"kind": "binary_flat", "d": d, "code_size": code_size, "ntotal": ntotal, "is_trained": is_trained,
            "metric": metric, "codes": codes.reshape(ntotal, code_size)}


def serialize_binary_flat(d, codes) -> bytes:
    """The inverse of parse_index_binary: d in bits, codes uint8 [ntotal][d / 8].
    Unpinned against Faiss, like the other layouts (see the module docstring)."""
    if d <= 0 or d % 8:
        raise RuntimeError(f"IndexBinaryFlat: d must be a positive multiple of 8, got {d}")
    cs = d // 8
    codes = np.ascontiguousarray(codes, np.uint8).reshape(-1)
    if codes.size % cs:
        raise RuntimeError(f"codes must hold whole rows of {cs} bytes")
    return b"".join([FOURCC_BINARY_FLAT, struct.pack("<iiqBi", d, cs, codes.size // cs, 1, 1), _vector(codes)])


def _parse_linear(r: _Reader) -> dict:
    """One VectorTransform record: "LTra" -> the LinearTransform dict; "PcAm" -> the same dict
    with kind "pca" and eigen_power, random_rotation, balanced_bins, mean [d_in], eigenvalues
    [d_in], PCAMat [d_in][d_in] (rows are eigenvectors)."""
    vh = r.fourcc()
    if vh == FOURCC_PCA:
        try:
            head = {"kind": "pca", "eigen_power": r.fmt("f"), "random_rotation": r.fmt("B") != 0,
                    "balanced_bins": r.fmt("i"), "mean": r.vector(np.float32), "eigenvalues": r.vector(np.float32),
                    "PCAMat": r.vector(np.float32)}
            t = _parse_linear_body(r)
        except RuntimeError as e:  # (the fields of another record, or of a later layout, read as counts)
            raise RuntimeError(f"malformed {FOURCC_PCA!r} VectorTransform record: {e}") from None
        d = t["d_in"]
        if t["is_trained"] and (head["mean"].size != d or head["eigenvalues"].size != d
                                or head["PCAMat"].size != d * d):
            raise RuntimeError("PCAMatrix mean / eigenvalues / PCAMat have the wrong size")
        if head["PCAMat"].size == d * d:
            head["PCAMat"] = head["PCAMat"].reshape(d, d)
        t.update(head)
        return t
    if vh != FOURCC_LINEAR:
        raise RuntimeError(f"unsupported VectorTransform {vh!r} (LinearTransform / OPQMatrix {FOURCC_LINEAR!r}, "
                           f"PCAMatrix {FOURCC_PCA!r} only)")
    return _parse_linear_body(r)


def _parse_linear_body(r: _Reader) -> dict:
    """What "LTra" writes after its fourcc (and "PcAm" after its own fields)."""
    have_bias = r.fmt("B") != 0
    A = r.vector(np.float32)
    b = r.vector(np.float32)
    d_in = r.fmt("i")
    d_out = r.fmt("i")
    t_trained = r.fmt("B") != 0
    if t_trained and A.size != d_in * d_out:
        raise RuntimeError("LinearTransform matrix has the wrong size")
    if have_bias and t_trained and b.size != d_out:
        raise RuntimeError("LinearTransform bias has the wrong size")
    return {"A": A.reshape(d_out, d_in) if A.size else A, "b": b if have_bias else None,
            "have_bias": have_bias, "d_in": d_in, "d_out": d_out, "is_trained": t_trained}


def parse_vector_transform(buf: bytes) -> dict:
    """A faiss.write_VectorTransform file (bench_gpu_1bn.py:507-510): one "LTra" or "PcAm" record."""
    r = _Reader(buf)
    t = _parse_linear(r)
    if r.o != len(r.b):
        raise RuntimeError("trailing bytes after the VectorTransform")
    return t


def serialize_linear(A, b, d_in, d_out, is_trained=True) -> bytes:
    A = np.zeros(0, np.float32) if A is None else np.ascontiguousarray(A, np.float32).reshape(-1)
    bb = np.zeros(0, np.float32) if b is None else np.ascontiguousarray(b, np.float32).reshape(-1)
    return b"".join([FOURCC_LINEAR, struct.pack("<B", 0 if b is None else 1), _vector(A), _vector(bb),
                     struct.pack("<iiB", d_in, d_out, 1 if is_trained else 0)])


def serialize_pca(eigen_power, random_rotation, balanced_bins, mean, eigenvalues, PCAMat, A, b, d_in, d_out,
                  is_trained=True) -> bytes:
    """A PCAMatrix as Faiss 1.7.1 writes it: "PcAm", eigen_power f32, random_rotation u8,
    balanced_bins i32, the vectors mean, eigenvalues, PCAMat, then the LinearTransform body
    exactly as "LTra" has it after its fourcc.  (Later Faiss versions insert an ``epsilon``
    f32 after eigen_power: this is the layout without it.)  Unpinned against Faiss, like the
    other layouts (see the module docstring)."""
    def vec(a):
        return _vector(np.zeros(0, np.float32) if a is None else np.ascontiguousarray(a, np.float32).reshape(-1))

    return b"".join([FOURCC_PCA, struct.pack("<fBi", eigen_power, 1 if random_rotation else 0, balanced_bins),
                     vec(mean), vec(eigenvalues), vec(PCAMat),
                     serialize_linear(A, b, d_in, d_out, is_trained)[4:]])


def _parse_ivfpq(r: _Reader, h: bytes) -> dict:
    if h == b"IvPQ":
        raise RuntimeError("legacy IvPQ Faiss files (pre-1.5 inverted lists) are not supported")
    if h != FOURCC_IVFPQ:
        raise RuntimeError(f"not a Faiss IndexIVFPQ file (fourcc {h!r})")
    d, ntotal, is_trained, metric, nlist, nprobe, xb = _parse_ivf_header(r)
    by_residual = r.fmt("B") != 0
    code_size = r.fmt("Q")
    pd = r.fmt("Q")
    M = r.fmt("Q")
    nbits = r.fmt("Q")
    cb = r.vector(np.float32)
    if not by_residual:
        raise RuntimeError("only by_residual IndexIVFPQ is supported")
    if pd != d or nbits != 8 or code_size != M or (is_trained and cb.size != M * 256 * (d // M)):
        raise RuntimeError("unsupported PQ shape (8-bit codes, code_size == M)")
    lists = _parse_ilar(r, nlist, code_size, ntotal)
    return {"kind": "ivfpq", "d": d, "nlist": nlist, "nprobe": nprobe, "M": M, "nbits": nbits, "metric": metric,
            "is_trained": is_trained, "centroids": xb.reshape(nlist, d) if xb.size else xb,
            "codebook": cb.reshape(M, 256, d // M) if cb.size else cb, "lists": lists}


def _parse_ivf_header(r: _Reader):
    """The part every IndexIVF writes first: index header, nlist, nprobe, flat quantizer, direct map."""
    d, ntotal, is_trained, metric = r.header()
    nlist = r.fmt("Q")
    nprobe = r.fmt("Q")
    qh = r.fourcc()
    if qh not in (b"IxF2", b"IxFI"):
        raise RuntimeError(f"unsupported coarse quantizer {qh!r} (IndexFlatL2 / IndexFlatIP only)")
    qd, qn, _, _ = r.header()
    xb = r.vector(np.float32)
    if qd != d or xb.size != qn * d:
        raise RuntimeError("quantizer shape does not match the index")
    dm_type = r.fmt("B")
    dm = r.vector(np.int64)
    if dm_type != 0 or dm.size:
        raise RuntimeError("IVF direct maps are not supported")
    return d, ntotal, is_trained, metric, nlist, nprobe, xb


def _parse_ilar(r: _Reader, nlist, code_size, ntotal):
    """ArrayInvertedLists -> [(ids i64[n], codes u8[n][code_size])] per list."""
    if r.fourcc() != b"ilar":
        raise RuntimeError("only ArrayInvertedLists ('ilar') are supported")
    il_n = r.fmt("Q")
    il_cs = r.fmt("Q")
    if il_n != nlist or il_cs != code_size:
        raise RuntimeError("inverted lists do not match the index")
    kind = r.fourcc()
    if kind == b"full":
        sizes = r.vector(np.uint64).astype(np.int64)
        if sizes.size != nlist:
            raise RuntimeError("inverted list size table has the wrong length")
    elif kind == b"sprs":
        pairs = r.vector(np.uint64).astype(np.int64).reshape(-1, 2)
        sizes = np.zeros(nlist, np.int64)
        sizes[pairs[:, 0]] = pairs[:, 1]
    else:
        raise RuntimeError(f"unknown inverted list size encoding {kind!r}")
    lists = []
    for l in range(nlist):
        n = int(sizes[l])
        if n:
            codes = np.frombuffer(r.take(n * code_size), np.uint8).reshape(n, code_size).copy()
            ids = np.frombuffer(r.take(n * 8), np.int64).copy()
        else:
            codes = np.zeros((0, code_size), np.uint8)
            ids = np.zeros(0, np.int64)
        lists.append((ids, codes))
    if int(sizes.sum()) != ntotal:
        raise RuntimeError("inverted list sizes do not add up to ntotal")
    return lists


def _parse_ivfflat(r: _Reader) -> dict:
    """IndexIVFFlat after its fourcc -> {kind "ivfflat", d, nlist, nprobe, metric, is_trained,
    centroids [nlist][d], lists: [(ids i64[n], vectors f32[n][d])]}."""
    d, ntotal, is_trained, metric, nlist, nprobe, xb = _parse_ivf_header(r)
    lists = [(ids, codes.view(np.float32).reshape(len(ids), d)) for ids, codes in _parse_ilar(r, nlist, 4 * d, ntotal)]
    return {"kind": "ivfflat", "d": d, "nlist": nlist, "nprobe": nprobe, "metric": metric, "is_trained": is_trained,
            "centroids": xb.reshape(nlist, d) if xb.size else xb, "lists": lists}


def _parse_ivfsq(r: _Reader) -> dict:
    """IndexIVFScalarQuantizer after its fourcc -> {kind "ivfsq", d, nlist, nprobe, qtype, metric,
    by_residual, is_trained, code_size, centroids [nlist][d], trained f32[...],
    lists: [(ids i64[n], codes u8[n][code_size])]}."""
    d, ntotal, is_trained, metric, nlist, nprobe, xb = _parse_ivf_header(r)
    qtype, sd, sq_cs, trained, rangestat = _parse_sq_block(r)
    code_size = r.fmt("Q")
    by_residual = r.fmt("B") != 0
    cs = _check_sq_block(qtype, d, sd, sq_cs, trained, rangestat, is_trained)
    if code_size != cs:
        raise RuntimeError("IndexIVFScalarQuantizer code size does not match its quantizer")
    lists = _parse_ilar(r, nlist, cs, ntotal)
    return {"kind": "ivfsq", "d": d, "nlist": nlist, "nprobe": nprobe, "qtype": qtype, "metric": metric,
            "by_residual": by_residual, "is_trained": is_trained, "code_size": cs,
            "centroids": xb.reshape(nlist, d) if xb.size else xb, "trained": trained, "lists": lists}


def serialize_ivfsq(d, nlist, nprobe, qtype, metric, by_residual, centroids, trained, lists, is_trained=True) -> bytes:
    """The inverse of parse_index for kind "ivfsq": lists = [(ids i64[n], codes u8[n][code_size])].
    Unpinned against Faiss, like the other layouts (see the module docstring)."""
    cs, _ = sq_shape(qtype, d)
    out = _ivf_header(FOURCC_IVFSQ, d, nlist, nprobe, metric, centroids, lists, is_trained)
    out += [_sq_block(d, qtype, trained), struct.pack("<QB", cs, 1 if by_residual else 0)]
    return b"".join(out + _ilar(nlist, cs, lists))


def _header(d, ntotal, is_trained, metric):
    return struct.pack("<iqqqBi", d, ntotal, HEADER_DUMMY, HEADER_DUMMY, 1 if is_trained else 0, metric)


def _vector(a):
    a = np.ascontiguousarray(a)
    return struct.pack("<Q", a.size) + a.tobytes()


def serialize_ivfpq(d, nlist, nprobe, M, nbits, metric, centroids, codebook, lists, is_trained=True) -> bytes:
    """The inverse of parse_ivfpq (sizes written as a "full" table, as Faiss does
    when more than half of the lists are non-empty, else "sprs")."""
    code_size = M * nbits // 8
    out = _ivf_header(FOURCC_IVFPQ, d, nlist, nprobe, metric, centroids, lists, is_trained)
    out += [struct.pack("<BQ", 1, code_size), struct.pack("<QQQ", d, M, nbits),
            _vector(np.ascontiguousarray(codebook, np.float32).reshape(-1))]
    return b"".join(out + _ilar(nlist, code_size, lists))


def serialize_ivfflat(d, nlist, nprobe, metric, centroids, lists, is_trained=True) -> bytes:
    """The inverse of parse_index for kind "ivfflat": lists = [(ids i64[n], vectors f32[n][d])].
    Unpinned against Faiss, like the other layouts (see the module docstring)."""
    out = _ivf_header(FOURCC_IVFFLAT, d, nlist, nprobe, metric, centroids, lists, is_trained)
    flat = [(ids, np.ascontiguousarray(v, np.float32).reshape(len(ids), d).view(np.uint8)) for ids, v in lists]
    return b"".join(out + _ilar(nlist, 4 * d, flat))


def _ivf_header(fourcc, d, nlist, nprobe, metric, centroids, lists, is_trained):
    ntotal = sum(len(ids) for ids, _ in lists)
    cent = np.ascontiguousarray(centroids, np.float32).reshape(-1)
    return [fourcc, _header(d, ntotal, is_trained, metric), struct.pack("<QQ", nlist, nprobe),
            FOURCC_FLAT[metric], _header(d, nlist if cent.size else 0, True, metric), _vector(cent),
            struct.pack("<B", 0), _vector(np.zeros(0, np.int64))]


def _ilar(nlist, code_size, lists):
    out = [b"ilar", struct.pack("<QQ", nlist, code_size)]
    sizes = np.array([len(ids) for ids, _ in lists], np.uint64)
    nz = np.nonzero(sizes)[0]
    if len(nz) > nlist // 2:
        out += [b"full", _vector(sizes)]
    else:
        out += [b"sprs", _vector(np.stack([nz.astype(np.uint64), sizes[nz]], 1).reshape(-1))]
    for ids, codes in lists:
        if len(ids):
            out.append(np.ascontiguousarray(codes, np.uint8).tobytes())
            out.append(np.ascontiguousarray(ids, np.int64).tobytes())
    return out


def serialize_pretransform(d, metric, chain, sub: bytes, ntotal, is_trained=True) -> bytes:
    """IndexPreTransform bytes: chain = [(A [d_out][d_in] | None, b | None, d_in, d_out, is_trained)
    | the bytes of one VectorTransform record (serialize_linear, serialize_pca)],
    sub = the wrapped index's bytes (serialize_ivfpq)."""
    out = [FOURCC_PRETRANSFORM, _header(d, ntotal, is_trained, metric), struct.pack("<i", len(chain))]
    out += [t if isinstance(t, bytes) else serialize_linear(*t) for t in chain]
    out.append(sub)
    return b"".join(out)
