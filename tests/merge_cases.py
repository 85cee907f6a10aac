"""Hand-built index contents for the k > 64 probe-merge tests (NumPy only).

Every index is d = 32, M = 8 (4 dimensions per sub-quantizer) on an integer
lattice: centroids, codebook and queries are small integers, so every L2 or IP
term and every partial sum is an integer below 2^24 and exact in fp32, whatever
the order of the additions.  Sub-quantizer 0's centroid j is (j, 0, 0, 0) and
entry 0 of every sub-quantizer is the zero vector, so a row whose code is all
zeros reconstructs to its list's centroid.

`tied`     lists with identical centroids and identical rows (equal keys across
           probes and waves), a few better rows, small random lists.
`single`   one list of 16384 identical rows beside three random lists.
`lattice`  inner product: sim = A + b + 256 a (A per list, code (b, a, 0...)),
           sub-quantizer 1's centroid j being (256 j, 0, 0, 0).
`rounds`   lists of 50, 200 and 256 rows (every scan wave sees fewer than k rows,
           so nothing is pruned and a query's candidate count is the sum of its
           lists' sizes), one list of 8192 rows in 8 key classes, lists of 0-3 rows.
"""
import numpy as np

D, M, DSUB = 32, 8, 4
L2, IP = "l2", "ip"


class Contents:
    def __init__(self, metric, cent, cb):
        self.metric, self.cent, self.cb = metric, cent.astype(np.float32), cb.astype(np.float32)
        self.nlist = cent.shape[0]
        self.list_no, self.codes, self.ids = [], [], []
        self.next_id = 1_000_000

    def add(self, l, codes, ids=None):
        codes = np.asarray(codes, np.uint8).reshape(-1, M)
        n = codes.shape[0]
        if ids is None:
            ids = np.arange(self.next_id, self.next_id + n, dtype=np.int64)
            self.next_id += n
        self.list_no.append(np.full(n, l, np.int64))
        self.codes.append(codes)
        self.ids.append(np.asarray(ids, np.int64))

    def finish(self):
        self.list_no = np.concatenate(self.list_no)
        self.codes = np.ascontiguousarray(np.concatenate(self.codes))
        self.ids = np.concatenate(self.ids)
        assert np.unique(self.ids).size == self.ids.size
        self.sizes = np.bincount(self.list_no, minlength=self.nlist)
        return self

    def dis0(self, xq, rows):
        """The coarse distances a preassigned L2 search is given: |x - c|^2, exact integers
        (None for inner product, where the scan forms <x, c> itself)."""
        if self.metric == IP:
            return None
        c = self.cent[np.maximum(rows, 0)].astype(np.float64)
        d2 = ((xq[:, None, :].astype(np.float64) - c) ** 2).sum(-1)
        assert d2.max() < 2 ** 24
        return np.where(rows >= 0, d2, 0).astype(np.float32)


def codebook(rng, lattice=False):
    cb = rng.integers(-2, 3, size=(M, 256, DSUB)).astype(np.float32)
    cb[:, 0, :] = 0
    cb[0] = 0
    cb[0, :, 0] = np.arange(256)
    if lattice:
        cb[1:] = 0
        cb[1, :, 0] = 256 * np.arange(256)
    return cb


def zero_codes(n):
    return np.zeros((n, M), np.uint8)


def random_codes(rng, n):
    return rng.integers(0, 256, size=(n, M), dtype=np.uint8)


# ---------------------------------------------------------------- tied lists
TIED_NLIST = 160
TIED_BIG = list(range(8))        # 4096 identical rows each
TIED_BETTER = 8                  # 30 rows better than the tied ones
TIED_128 = [10, 11, 12, 13]      # 128 tied rows each
TIED_129 = 14                    # 129 tied rows
TIED_SMALL = [15, 16]            # 20 random rows each
TIED_RANDOM = list(range(20, 160))  # 0-60 random rows each
TIED_ROWS = 4096


def tied_A(metric):
    return 4096 if metric == IP else 64


def tied(metric, id_variant):
    """id_variant "interleave": id = row * 8 + list over the eight big tied lists (label order
    walks across the lists); "permuted": a random permutation of those labels."""
    rng = np.random.default_rng(7001 + (metric == IP))
    cent = rng.integers(-3, 4, size=(TIED_NLIST, D)).astype(np.float32)
    ct = np.zeros(D, np.float32)
    ct[0] = tied_A(metric)
    for l in TIED_BIG + [TIED_BETTER] + TIED_128 + [TIED_129]:
        cent[l] = ct
    c = Contents(metric, cent, codebook(rng))
    lab = np.arange(TIED_ROWS * 8, dtype=np.int64)
    if id_variant == "permuted":
        lab = np.random.default_rng(7).permutation(lab)
    lab = lab.reshape(TIED_ROWS, 8)
    for l in TIED_BIG:
        c.add(l, zero_codes(TIED_ROWS), lab[:, l])
    better = zero_codes(30)
    better[:, 0] = 1 + np.arange(30) % 3
    c.add(TIED_BETTER, better)
    for l in TIED_128:
        c.add(l, zero_codes(128))
    c.add(TIED_129, zero_codes(129))
    for l in TIED_SMALL:
        c.add(l, random_codes(rng, 20))
    for l in TIED_RANDOM:
        c.add(l, random_codes(rng, int(rng.integers(0, 61))))
    return c.finish()


def tied_queries(metric, nq, seed=0):
    """Queries for which the tied rows are the best but for list TIED_BETTER's: L2 x = centroid
    + (3, 0, 0, 0, r) (tied distance 9 + |r|^2, better rows 4, 1, 0 + |r|^2); IP x = (1, r)
    (tied similarity A, better rows A + 1...3, every random list's far below)."""
    rng = np.random.default_rng(7100 + seed)
    if metric == IP:
        x = rng.integers(-3, 4, size=(nq, D)).astype(np.float32)
        x[:, 0] = 1
    else:
        x = np.zeros((nq, D), np.float32)
        x[:, 4:] = rng.integers(-2, 3, size=(nq, D - 4))
        x[:, 0] = tied_A(metric) + 3
    return x


def tied_key(metric, xq):
    """The value the search reports for a tied row, per query."""
    if metric == IP:
        return np.full(xq.shape[0], tied_A(metric), np.float32)
    return (9 + (xq[:, 4:].astype(np.float64) ** 2).sum(1)).astype(np.float32)


# ---------------------------------------------------------------- one long list
SINGLE_ROWS = 16384


def single(metric):
    rng = np.random.default_rng(7201 + (metric == IP))
    cent = rng.integers(-3, 4, size=(4, D)).astype(np.float32)
    cent[0] = 0
    cent[0, 0] = tied_A(metric)
    c = Contents(metric, cent, codebook(rng))
    c.add(0, zero_codes(SINGLE_ROWS), np.random.default_rng(8).permutation(SINGLE_ROWS).astype(np.int64))
    for l in (1, 2, 3):
        c.add(l, random_codes(rng, 200))
    return c.finish()


# ---------------------------------------------------------------- inner-product lattice
LAT_SPREAD = 0            # A = 0: sims b + 256 a, every a >= 128 in its own 16-bit bucket
LAT_ONE16 = 1             # A = 2^23: one 16-bit bucket, every a its own 24-bit bucket
LAT_ONE24 = [2, 3, 4]     # A = 2^23, a = 7, b = 0..255 in each: 768 keys in one 24-bit bucket
LAT_FEW = 5               # A = 0, 50 rows
LAT_SIGNS8 = list(range(6, 14))  # A = -58000 - 500 i: sims of both signs
LAT_SIGNS = 14            # A = -45000
LAT_A = {LAT_SPREAD: 0, LAT_ONE16: 2 ** 23, 2: 2 ** 23, 3: 2 ** 23, 4: 2 ** 23, LAT_FEW: 0, LAT_SIGNS: -45000}
LAT_A.update({l: -58000 - 500 * i for i, l in enumerate(LAT_SIGNS8)})


def lattice():
    rng = np.random.default_rng(7301)
    cent = np.zeros((16, D), np.float32)
    for l, a in LAT_A.items():
        cent[l, 0] = a
    c = Contents(IP, cent, codebook(rng, lattice=True))
    row = np.arange(256)

    def ab(a, b):
        codes = zero_codes(len(a))
        codes[:, 0], codes[:, 1] = b, a
        return codes

    c.add(LAT_SPREAD, ab(row, (37 * row) % 256))
    c.add(LAT_ONE16, ab(row, (91 * row) % 256))
    for l in LAT_ONE24:
        c.add(l, ab(np.full(256, 7), row))
    c.add(LAT_FEW, ab(200 + np.arange(50), np.arange(50)))
    for i, l in enumerate(LAT_SIGNS8):
        c.add(l, ab(row, (53 * row + i) % 256))
    c.add(LAT_SIGNS, ab(row, (29 * row) % 256))
    return c.finish()


def lattice_queries(nq, zero=()):
    """x = (1, 0, 0, 0, 1, 0, 0, 0, r): sim = A + b + 256 a (the codebook is zero where r is
    not); the queries listed in `zero` are all zeros (every candidate's sim is 0)."""
    rng = np.random.default_rng(7400)
    x = np.zeros((nq, D), np.float32)
    x[:, 8:] = rng.integers(-3, 4, size=(nq, D - 8))
    x[:, 0] = x[:, 4] = 1
    for q in zero:
        x[q] = 0
    return x


def lattice_sims(c, l):
    """The similarities of list l's rows for a lattice query, from the construction."""
    codes = c.codes[c.list_no == l].astype(np.int64)
    return LAT_A[l] + codes[:, 0] + 256 * codes[:, 1]


# ---------------------------------------------------------------- merge rounds
RS_NLIST = 160
RS_50 = list(range(0, 13))
RS_200 = list(range(13, 24))
RS_256 = list(range(24, 88))
RS_LONG = 88
RS_TINY = list(range(89, 108))
RS_LONG_ROWS = 8192


def rounds(metric):
    rng = np.random.default_rng(7501 + (metric == IP))
    cent = rng.integers(-3, 4, size=(RS_NLIST, D)).astype(np.float32)
    cent[RS_LONG, 0] = 5
    c = Contents(metric, cent, codebook(rng))
    for ls, n in ((RS_50, 50), (RS_200, 200), (RS_256, 256)):
        for l in ls:
            c.add(l, random_codes(rng, n))
    long_codes = zero_codes(RS_LONG_ROWS)
    long_codes[:, 0] = np.arange(RS_LONG_ROWS) % 8  # 8 distinct keys, 256 rows of each per scan wave
    c.add(RS_LONG, long_codes)
    for i, l in enumerate(RS_TINY):
        c.add(l, random_codes(rng, i % 4))
    return c.finish()


def rounds_queries(nq, seed=0):
    rng = np.random.default_rng(7600 + seed)
    x = rng.integers(-3, 4, size=(nq, D)).astype(np.float32)
    x[:, 0] = 1  # (RS_LONG's 8 keys are distinct for both metrics)
    return x


def pad_rows(lists, nprobe):
    """One probe row: the lists, then -1."""
    return np.asarray(list(lists) + [-1] * (nprobe - len(lists)), np.int64)
