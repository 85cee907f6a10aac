"""bench.py as a command: the plain run's result line, ``--dump-outputs`` and ``--full``.

Run at a reduced size (smoke()'s index: d = 64, IVF64,PQ16, 20 000 vectors; two
batches of 64 queries, two in flight).  Four timed steps end on batch 1 and on
stream 1's output buffers, so a dump of the wrong batch or buffer differs.

* a plain run prints one JSON line with the headline keys only, for the number
  of steps asked for;
* the dump is what the timed path returned for the last step's batch: equal,
  bit for bit, to a search of that batch on the same index built in this
  process (the data and the GPU training are deterministic), float32 distances
  and labels as float64;
* a second run with the same arguments dumps the same arrays;
* ``--full`` adds the roofline, stage, serial, recall, CPU-baseline and extra
  legs to the same headline, and dumps the same arrays.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import faiss_amd as faiss
from faiss_amd import datasets

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D_, NLIST, M, NB, NT, CENTRES, NITER = 64, 64, 16, 20000, 4000, 100, 5
BATCH, NBATCHES, K, NPROBE, STEPS, WARMUP = 64, 2, 10, 8, 4, 1
SIZE = ["--d", D_, "--nlist", NLIST, "--M", M, "--nb", NB, "--nt", NT, "--centres", CENTRES, "--niter", NITER,
        "--batch", BATCH, "--nbatches", NBATCHES, "--k", K, "--nprobe", NPROBE]
HEADLINE = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "full", "data", "config", "repairs", "stale_reads"}
FULL_ONLY = {"ms_per_step_serial", "roofline", "stages_ms_per_step", "recall", "cpu_baseline", "extra"}


def run_bench(dump, *more):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", STEPS, "--warmup", WARMUP,
           "--dump-outputs", dump, *SIZE, *more]
    p = subprocess.run([str(c) for c in cmd], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0]), np.load(os.path.join(dump, "D.npy")), np.load(os.path.join(dump, "I.npy"))


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return run_bench(str(tmp_path_factory.mktemp("plain")))


def check_headline(j, full):
    assert j["steps"] == STEPS and j["warmup"] == WARMUP and j["full"] is full
    assert j["unit"] == "queries/s" and j["higher_is_better"] is True and j["dtype"] == "f32"
    assert j["ms_per_step"] > 0
    assert j["value"] == pytest.approx(BATCH / (j["ms_per_step"] * 1e-3), rel=1e-9)
    assert j["repairs"] == 0 and j["stale_reads"] == 0


def test_plain_run_prints_the_headline_only(plain):
    j, _, _ = plain
    assert set(j) == HEADLINE
    check_headline(j, False)


def test_dump_is_the_last_timed_steps_result(plain):
    _, D, I = plain
    assert D.dtype == np.float32 and I.dtype == np.float64
    gen = dict(n_centres=CENTRES)
    ix = faiss.index_factory(D_, f"IVF{NLIST},PQ{M}", device=0)
    ix.niter_coarse = ix.niter_pq = NITER
    ix.train(datasets.synthetic_sift_like(NT, D_, seed=4321, **gen))
    ix.add(datasets.synthetic_sift_like(NB, D_, seed=1234, **gen))
    ix.nprobe = NPROBE
    xq = datasets.synthetic_sift_like(NBATCHES * BATCH, D_, seed=123, **gen)
    b = (STEPS - 1) % NBATCHES
    Dr, Ir = ix.search(xq[b * BATCH:(b + 1) * BATCH], K)
    np.testing.assert_array_equal(I, Ir.astype(np.float64))
    np.testing.assert_array_equal(D, Dr)


def test_same_arguments_dump_the_same_arrays(plain, tmp_path):
    _, D, I = plain
    _, D2, I2 = run_bench(str(tmp_path))
    np.testing.assert_array_equal(D2, D)
    np.testing.assert_array_equal(I2, I)


def test_full_adds_its_legs_to_the_same_headline(plain, tmp_path):
    _, D, I = plain
    j, Df, If = run_bench(str(tmp_path), "--full", "--cpu-sample", 64, "--cpu-seconds", 0.05)
    assert set(j) == HEADLINE | FULL_ONLY
    check_headline(j, True)
    assert j["ms_per_step_serial"] > 0 and j["roofline"]["achieved"] > 0 and j["roofline"]["peak_measured"] > 0
    assert set(j["stages_ms_per_step"]) >= {"scan", "lists"}
    assert j["recall"]["queries"] == NBATCHES * BATCH
    assert j["cpu_baseline"]["value"] > 0 and j["cpu_baseline"]["gpu_id_agreement"] == 1.0
    assert j["extra"]["k100_queries_per_s"] > 0 and j["extra"]["host_search_queries_per_s"] > 0
    np.testing.assert_array_equal(Df, D)
    np.testing.assert_array_equal(If, I)
