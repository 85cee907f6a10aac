#!/usr/bin/env python3
"""GpuIndexFlatL2 with useFloat16 (half rows, v_mfma_f32_16x16x32_f16 scan) beside the fp32
IndexFlatL2 over the same vectors on one MI355X, with both images' bytes and two floors.

    python profiles/indexflat_f16_bench.py [--out profiles/indexflat_f16_bench.json] [--nb 1000000]

Data: clustered vectors from datasets.synthetic_sift_like, 1 M base rows, 1024 queries, L2.
Shapes: d = 128 and d = 768; nq = 1024 at k = 10, 100, 1000; nq = 1 and nq = 16 at k = 64.
One child process per d under ``timeout``; the first step that fails ends the run (nothing else
is started on the GPU; the JSON keeps the steps that finished).

Per shape, three alternating rounds of
  half_device_ms   the half index's search_device: device events around whole calls (query
                   rounding included), a window of at least a second after a warm-up
  fp32_device_ms   IndexFlatL2.search_device over the same vectors, timed the same way
``half_faster_in_every_pair`` compares the two of every round; ``gain_clear_of_spread``: the
slowest half round is faster than the fastest fp32 round and the medians differ by more than
both min-max spreads together.  ``labels_equal_fp32`` is the share of equal labels (the half
index ranks rounded vectors: it is information, not a check).

Floors, computed from rates measured in the same job:
  mfma_floor_ms    2 nq nb d flop (nq rounded up to the plan's query tile) at the rate
                   csrc/mfma_f16_rate.hip reaches with v_mfma_f32_16x16x32_f16
  byte_floor_ms    image bytes x query tiles over the HBM read rate of csrc/hbm_stream.hip
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "chameleon-rag-acceleration_amd"), os.path.join(REPO, "profiles")):
    if p not in sys.path:
        sys.path.insert(0, p)

NQ = 1024
STEP_TIMEOUT = 540
SHAPES = [dict(nq=NQ, k=10), dict(nq=NQ, k=100), dict(nq=NQ, k=1000), dict(nq=1, k=64), dict(nq=16, k=64)]


def mfma_f16_rate(torch):
    """flop/s of v_mfma_f32_16x16x32_f16 over the whole device (best of 5 launches of about 10 ms)."""
    ml = ctypes.CDLL(os.path.join(REPO, "chameleon-rag-acceleration_amd", "lib", "libmfmarate.so"))
    grid, ms, flop = ctypes.c_int(0), ctypes.c_float(0), ctypes.c_double(0)
    args = lambda sink, nbytes: (20000, 5, sink, ctypes.c_int64(nbytes),  # noqa: E731
                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.byref(grid),
                                 ctypes.byref(ms), ctypes.byref(flop))
    if ml.mfma_f16_rate_measure(*args(None, 0)) != 0:
        raise RuntimeError("mfma_f16_rate_measure failed")
    sink = torch.empty(grid.value * 256, dtype=torch.float32, device="cuda")
    rc = ml.mfma_f16_rate_measure(*args(ctypes.c_void_p(sink.data_ptr()), sink.numel() * 4))
    torch.cuda.synchronize()
    if rc != 0:
        raise RuntimeError("mfma_f16_rate_measure failed")
    return flop.value / (ms.value * 1e-3)


def step_d(d, nb):
    import numpy as np
    import torch

    import faiss_amd as faiss
    from faiss_amd import datasets
    from faiss_amd.index import flat_search_plan
    from ivfflat_bench import hbm_read_rate, timed

    xb = datasets.synthetic_sift_like(nb, d, seed=1234)
    xq_all = datasets.synthetic_sift_like(NQ, d, seed=123)
    cfg = faiss.GpuIndexFlatConfig()
    cfg.useFloat16 = True
    half = faiss.GpuIndexFlatL2(faiss.StandardGpuResources(), d, cfg)
    fp32 = faiss.IndexFlatL2(d)
    for ix in (half, fp32):
        for lo in range(0, nb, 50_000):
            ix.add(xb[lo:lo + 50_000])
        ix.search(xq_all[:1], 1)  # the lazy upload
    del xb
    read_rate = hbm_read_rate(torch)
    mfma_rate = mfma_f16_rate(torch)

    results = []
    for s in SHAPES:
        nq, k = s["nq"], s["k"]
        txq = torch.from_numpy(np.ascontiguousarray(xq_all[:nq])).cuda()
        Dh = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        Ih = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        Df, If = torch.empty_like(Dh), torch.empty_like(Ih)
        rounds = []
        for _ in range(3):
            h_ms, h_reps = timed(lambda: half.search_device(txq, k, Dh, Ih), torch)
            f_ms, f_reps = timed(lambda: fp32.search_device(txq, k, Df, If), torch)
            rounds.append(dict(half_device_ms=h_ms, half_calls=h_reps, fp32_device_ms=f_ms, fp32_calls=f_reps))
        plan = flat_search_plan(nq, nb, k)
        tile_q = plan["tile_q"]
        tiles = -(-nq // tile_q)
        hs, fs = sorted(r["half_device_ms"] for r in rounds), sorted(r["fp32_device_ms"] for r in rounds)
        results.append(dict(
            d=d, nb=nb, nq=nq, k=k, metric="l2", plan=plan, rounds=rounds, half_device_ms=hs[1], fp32_device_ms=fs[1],
            half_min_max_ms=[hs[0], hs[2]], fp32_min_max_ms=[fs[0], fs[2]], speedup=fs[1] / hs[1],
            half_faster_in_every_pair=all(r["half_device_ms"] < r["fp32_device_ms"] for r in rounds),
            gain_clear_of_spread=bool(hs[2] < fs[0] and fs[1] - hs[1] > (hs[2] - hs[0]) + (fs[2] - fs[0])),
            labels_equal_fp32=float((Ih == If).float().mean().item()),
            mfma_floor_ms=2.0 * tiles * tile_q * nb * d / mfma_rate * 1e3,
            half_byte_floor_ms=2.0 * nb * d * tiles / read_rate * 1e3,
            fp32_byte_floor_ms=4.0 * nb * d * tiles / read_rate * 1e3))
        print("SHAPE " + json.dumps(results[-1]), flush=True)
    return dict(d=d, nb=nb, hbm_read_bytes_per_s=read_rate, mfma_f16_flops=mfma_rate,
                half_image_bytes=2 * nb * d, fp32_image_bytes=4 * nb * d, shapes=results)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "indexflat_f16_bench.json"))
    ap.add_argument("--nb", type=int, default=1_000_000)
    ap.add_argument("--dims", default="128,768")
    ap.add_argument("--step", type=int)
    a = ap.parse_args()
    if a.step:  # child: one GPU step, one JSON line
        print("RESULT " + json.dumps(step_d(a.step, a.nb)), flush=True)
        return 0
    result = {"nb": a.nb, "nq": NQ, "dims": {}}
    for d in [int(v) for v in a.dims.split(",")]:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--step", str(d),
               "--nb", str(a.nb)]
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        lines, tail = [], []
        for ln in p.stdout:  # a line per finished shape, as it comes
            tail = (tail + [ln])[-60:]
            if ln.startswith("RESULT "):
                lines.append(ln)
            elif ln.startswith("SHAPE "):
                s = json.loads(ln[6:])
                print(f"d={d} nq={s['nq']} k={s['k']}: half {s['half_device_ms']:.3f} ms, fp32 "
                      f"{s['fp32_device_ms']:.3f} ms ({s['speedup']:.2f}x), floors mfma {s['mfma_floor_ms']:.3f} / "
                      f"bytes {s['half_byte_floor_ms']:.3f} ms", flush=True)
        p.wait()
        if p.returncode != 0 or not lines:
            sys.stderr.write("".join(tail))
            sys.stderr.write(f"\nstep d={d} failed (exit {p.returncode}); stopping\n")
            return 1
        result["dims"][str(d)] = json.loads(lines[-1][7:])
        with open(a.out, "w") as f:  # (rewritten after every step: a later step's failure keeps the earlier numbers)
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
