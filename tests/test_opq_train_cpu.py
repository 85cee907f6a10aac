"""The host side of the resident OPQ trainer: what needs neither a GPU nor a device."""
import ctypes

import numpy as np
import pytest

from faiss_amd import _lib
from faiss_amd.transform import OPQMatrix, opq_plan, opq_set_chunk_rows


@pytest.mark.parametrize("n,d,d2,rows", [(37, 24, 16, 0), (300, 72, 40, 64), (257, 130, 96, 100), (65536, 768, 384, 0),
                                         (65536, 128, 128, 0)])
def test_plan_covers_the_rows(n, d, d2, rows):
    opq_set_chunk_rows(rows)
    try:
        p = opq_plan(n, d, d2)
    finally:
        opq_set_chunk_rows(0)
    assert p["tiles"] == -(-d // 64) * -(-d2 // 64)
    assert p["chunk_rows"] % 32 == 0 and p["chunks"] == -(-n // p["chunk_rows"])
    if rows:
        assert p["chunk_rows"] == -(-rows // 32) * 32
    else:  # no chunk under 256 rows, about 1024 workgroups
        assert p["chunk_rows"] >= 256 and p["chunks"] * p["tiles"] <= 1024 + p["tiles"]


def test_gpu_is_opt_in():
    assert OPQMatrix().gpu is False and OPQMatrix(32, 4).gpu is False


def test_train_device_rejects_what_is_not_a_cuda_tensor():
    import torch

    opq = OPQMatrix(8, 2)
    x = np.zeros((300, 8), np.float32)
    for bad in (x, torch.from_numpy(x), torch.zeros(300, 9), torch.zeros(300, 8, dtype=torch.float64), x.tolist()):
        with pytest.raises(RuntimeError, match="train_device: x must be a float32 CUDA tensor"):
            opq.train_device(bad)
    assert not opq.is_trained


def test_create_rejects_bad_shapes_before_any_device():
    L, h = _lib.load(), _lib.c_handle()
    for (d, d2, M), word in [((32, 48, 4), b"d2"), ((32, 30, 4), b"multiple"), ((32, 32, 0), b"M must")]:
        assert L.ivfpq_opq_create(d, d2, M, 0, ctypes.byref(h)) != 0
        assert word in L.ivfpq_last_error()
    assert L.ivfpq_opq_free(None) == 0
    assert L.ivfpq_opq_get_plan(0, 8, 8, None, None, None) != 0 and L.ivfpq_opq_set_chunk_rows(-1) != 0
