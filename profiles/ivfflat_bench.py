#!/usr/bin/env python3
"""IndexIVFFlat throughput on one MI355X beside its two bounds, and the paired comparison
with the library's other exact-distance search, IndexFlatL2.search.

What the comparator measures changed with the device-resident flat index: IndexFlatL2.search
no longer is ivfpq_flat_search (brute force with the base uploaded on every call and the full
distance matrix written and selected from -- what profiles/ivfflat_bench.json and DESIGN.md
section 4c recorded) but the fused scan over rows kept in HBM, whose
first call also uploads the rows.  A new run of this script therefore compares IndexIVFFlat
with the resident flat index; profiles/indexflat_bench.py times the stateless call, IVF1,Flat
and the flat index in one job.

    python profiles/ivfflat_bench.py [--out profiles/ivfflat_bench.json] [--nb 1000000]

Shapes: 1024 queries, k = 10, d = 128, clustered data (datasets.synthetic_sift_like):
  ivf1024  IVF1024,Flat, nprobe 16 -- the C2 shape with raw vectors
  ivf1     IVF1,Flat               -- the exact ground truth of compute_ground_truth.py:311
Every GPU step runs in a child process of its own under ``timeout``; the first step that
fails ends the run (nothing else is started on the GPU) and no JSON is written.

Times: ``device_ms`` = device events around whole ``search_device`` calls (coarse
quantizer, planning, scan, merge) after a warm-up, over a window of at least a second.
The comparator takes host buffers only, so each of the three alternating pairs times one
host call of each side with the wall clock (``IndexIVFFlat.search`` against
``IndexFlatL2.search`` of the same queries over the same vectors; both copy the queries
in and the results out; the comparator uploads the base vectors in its first call and keeps
them).  Bounds, from the batch's own probes:
  valu_floor_ms   3 d (rows scanned x queries served) lane-operations (subtract, multiply,
                  add; -ffp-contract=off) over 256 CUs x 128 lanes x 2.4 GHz
  hbm_floor_ms    list bytes fetched once per (row range, group of G pairs) over the HBM
                  read rate measured here by csrc/hbm_stream.hip, as bench.py measures it
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "chameleon-rag-acceleration_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

VALU_LANE_OPS_PER_S = 256 * 128 * 2.4e9  # = the 157.3 TFLOPS fp32 vector peak / 2 (an FMA counts twice)
RANGE_ROWS = 4096                        # kIvfFlatRangeRows
D, NQ, K = 128, 1024, 10
SHAPES = {"ivf1024": dict(nlist=1024, nprobe=16), "ivf1": dict(nlist=1, nprobe=1)}
STEP_TIMEOUT = 540


def timed(fn, torch, min_seconds=1.0):
    """ms per call: two warm-up calls, then a window of at least min_seconds."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    one = max(a.elapsed_time(b), 1e-3)
    reps = int(min(2000, max(3, min_seconds * 1000.0 / one)))
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps, reps


def hbm_read_rate(torch):
    """bytes/s of csrc/hbm_stream.hip's read sweep (1 GiB, best of 10)."""
    import ctypes

    hl = ctypes.CDLL(os.path.join(REPO, "chameleon-rag-acceleration_amd", "lib", "libhbmstream.so"))
    nbytes = 1 << 30
    src = torch.empty(nbytes // 4, dtype=torch.int32, device="cuda").random_(0, 1 << 30)
    dst = torch.empty_like(src)
    sink = torch.empty(1 << 22, dtype=torch.int32, device="cuda")
    cms, rms = ctypes.c_float(0), ctypes.c_float(0)
    rc = hl.hbm_stream_measure(ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()),
                               ctypes.c_int64(nbytes), ctypes.c_void_p(sink.data_ptr()),
                               ctypes.c_int64(sink.numel() * 4), 10,
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream),
                               ctypes.byref(cms), ctypes.byref(rms))
    torch.cuda.synchronize()
    if rc != 0:
        raise RuntimeError("hbm_stream_measure failed")
    return nbytes / (rms.value * 1e-3)


def step_shape(name, nb):
    import numpy as np
    import torch

    import faiss_amd as faiss
    from faiss_amd import datasets

    s = SHAPES[name]
    xb = datasets.synthetic_sift_like(nb, D, seed=1234)
    xq = datasets.synthetic_sift_like(NQ, D, seed=123)
    ix = faiss.index_factory(D, f"IVF{s['nlist']},Flat")
    ix.niter_coarse = 10
    ix.train(datasets.synthetic_sift_like(100_000, D, seed=4321))
    t0 = time.perf_counter()
    ix.add(xb)
    sizes = ix.invlists.list_sizes()
    add_s = time.perf_counter() - t0
    ix.nprobe = s["nprobe"]
    flat = faiss.IndexFlatL2(D)
    flat.add(xb)

    txq = torch.from_numpy(xq).cuda()
    Dd = torch.empty((NQ, K), dtype=torch.float32, device="cuda")
    Id = torch.empty((NQ, K), dtype=torch.int64, device="cuda")
    device_ms, reps = timed(lambda: ix.search_device(txq, K, Dd, Id), torch)

    runs = []
    for _ in range(3):  # alternating pairs, host calls, wall clock
        t0 = time.perf_counter()
        Df, If = flat.search(xq, K)
        t1 = time.perf_counter()
        Dn, In = ix.search(xq, K)
        t2 = time.perf_counter()
        runs.append({"indexflatl2_ms": (t1 - t0) * 1e3, "ivfflat_ms": (t2 - t1) * 1e3,
                     "ratio": (t1 - t0) / (t2 - t1)})
    assert np.array_equal(In, Id.cpu().numpy()) and np.array_equal(Dn, Dd.cpu().numpy())

    # the batch's work, from its own probes
    cq = faiss.IndexFlatL2(D)
    cq.add(ix.centroids())
    probes = cq.search(xq, min(s["nprobe"], s["nlist"]))[1]
    pairs_per_list = np.bincount(probes.reshape(-1), minlength=s["nlist"])
    distances = int((pairs_per_list * sizes).sum())
    G = 8  # pairs per work item at k <= 64
    list_bytes = int((-(-pairs_per_list // G) * sizes).sum()) * 4 * D
    items = int((-(-pairs_per_list // G) * -(-sizes // RANGE_ROWS)).sum())
    read_rate = hbm_read_rate(torch)
    med = sorted(runs, key=lambda r: r["ratio"])[1]
    out = dict(shape=name, d=D, nb=nb, nq=NQ, k=K, nlist=s["nlist"], nprobe=s["nprobe"], add_seconds=add_s,
               imbalance_factor=ix.invlists.imbalance_factor(), largest_list=int(sizes.max()),
               device_ms_per_batch=device_ms, batches_timed=reps, queries_per_s=NQ / device_ms * 1e3,
               distances_computed=distances, fraction_of_brute_force=distances / (NQ * nb), work_items=items,
               valu_floor_ms=3 * D * distances / VALU_LANE_OPS_PER_S * 1e3,
               list_bytes_fetched=list_bytes, hbm_read_bytes_per_s=read_rate,
               hbm_floor_ms=list_bytes / read_rate * 1e3,
               pairs_vs_indexflatl2=runs, median_pair=med,
               faster_than_indexflatl2_in_every_pair=all(r["ivfflat_ms"] < r["indexflatl2_ms"] for r in runs),
               # brute-force ground truth: the comparator's labels
               recall_R1_at_10=datasets.recall_1_at(In, If, ranks=(10,))[10], recall_R_at_10=datasets.recall_at_k(In, If, K),
               labels_equal_brute_force=float((In == If).mean()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ivfflat_bench.json"))
    ap.add_argument("--nb", type=int, default=1_000_000)
    ap.add_argument("--step")
    a = ap.parse_args()
    if a.step:  # child: one GPU step, one JSON line
        print("RESULT " + json.dumps(step_shape(a.step, a.nb)), flush=True)
        return 0
    result = {"nb": a.nb, "valu_lane_ops_per_s": VALU_LANE_OPS_PER_S, "shapes": {}}
    for step in SHAPES:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--step", step,
               "--nb", str(a.nb)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            sys.stderr.write(p.stdout[-4000:])
            sys.stderr.write(f"\nstep {step} failed (exit {p.returncode}); stopping\n")
            return 1
        r = json.loads(lines[-1][7:])
        print(step, json.dumps(r), flush=True)
        result["shapes"][step] = r
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
