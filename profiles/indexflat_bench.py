#!/usr/bin/env python3
"""IndexFlat (device-resident rows, fused matrix-core top-k scan) on one MI355X beside the two
code paths it is measured against and its two computed floors.

    python profiles/indexflat_bench.py [--out profiles/indexflat_bench.json] [--nb 1000000]

Data: clustered vectors from datasets.synthetic_sift_like, 1 M base rows, 1024 queries.
Shapes: d = 128 and d = 768; k = 10, 100, 1000; L2 and inner product; and nq = 1 and nq = 16
at k = 64 (the index-scanner shape, L2).  One child process per d under ``timeout``; the first
step that fails ends the run (nothing else is started on the GPU; the JSON keeps the steps
that finished).

Per shape, three alternating rounds of
  flat_device_ms      IndexFlat.search_device: device events around whole calls, a window of
                      at least a second after a warm-up
  ivf1_device_ms      IVF1,Flat search_device over the same vectors, timed the same way (the
                      exact search every flat scan here was measured against so far)
  stateless_host_ms   one ivfpq_flat_search host call, wall clock: the path IndexFlatL2.search
                      took before (base uploaded per call, distance matrix written and selected
                      from), as DESIGN.md section 4c timed it
  flat_host_ms        one IndexFlat.search host call, wall clock (queries in, results out)
``faster_than_stateless_in_every_pair`` compares the two host calls of every round.

Floors, computed:
  mfma_floor_ms       2 nq nb d flop at the 155 TF measured for v_mfma_f32_16x16x4_f32
                      (with nq rounded up to the plan's query tile: mfma_floor_tiles_ms)
  byte_floor_ms       base bytes x query tiles (of 64 or 16 queries, the plan's) over the HBM
                      read rate csrc/hbm_stream.hip measures in the same job (every workgroup
                      streams its row range once)
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "chameleon-rag-acceleration_amd"), os.path.join(REPO, "profiles")):
    if p not in sys.path:
        sys.path.insert(0, p)

MFMA_F32_FLOPS = 155e12
NQ = 1024
STEP_TIMEOUT = 1100
IP, L2 = 0, 1


def shapes():
    out = [dict(nq=NQ, k=k, metric=m) for m in (L2, IP) for k in (10, 100, 1000)]
    return out + [dict(nq=1, k=64, metric=L2), dict(nq=16, k=64, metric=L2)]


def step_d(d, nb):
    import numpy as np
    import torch

    import faiss_amd as faiss
    from faiss_amd import _lib, datasets
    from faiss_amd.index import flat_search_plan
    from ivfflat_bench import hbm_read_rate, timed

    xb = datasets.synthetic_sift_like(nb, d, seed=1234)
    xq_all = datasets.synthetic_sift_like(NQ, d, seed=123)
    train = datasets.synthetic_sift_like(20_000, d, seed=4321)
    flat, ivf1 = {}, {}
    t_add = {}
    for m in (L2, IP):
        flat[m] = faiss.IndexFlat(d, m)
        t0 = time.perf_counter()
        for lo in range(0, nb, 50_000):  # beir's buffers
            flat[m].add(xb[lo:lo + 50_000])
        flat[m].search(xq_all[:1], 1)  # the lazy upload
        t_add[m] = time.perf_counter() - t0
        ivf1[m] = faiss.index_factory(d, "IVF1,Flat", m)
        ivf1[m].niter_coarse = 2
        ivf1[m].train(train)
        ivf1[m].add(xb)
    read_rate = hbm_read_rate(torch)
    L = _lib.load()
    f32p, i64p = _lib.c_f32p, _lib.c_i64p

    results = []
    for s in shapes():
        nq, k, m = s["nq"], s["k"], s["metric"]
        xq = np.ascontiguousarray(xq_all[:nq])
        txq = torch.from_numpy(xq).cuda()
        Dd = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        Id = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        Dv, Iv = torch.empty_like(Dd), torch.empty_like(Id)
        Ds, Is = np.empty((nq, k), np.float32), np.empty((nq, k), np.int64)
        rounds = []
        for _ in range(3):
            f_ms, f_reps = timed(lambda: flat[m].search_device(txq, k, Dd, Id), torch)
            v_ms, v_reps = timed(lambda: ivf1[m].search_device(txq, k, Dv, Iv), torch)
            t0 = time.perf_counter()
            _lib.check(L.ivfpq_flat_search(0, d, nb, xb.ctypes.data_as(f32p), nq, xq.ctypes.data_as(f32p), k, m,
                                           Ds.ctypes.data_as(f32p), Is.ctypes.data_as(i64p)))
            t1 = time.perf_counter()
            Dh, Ih = flat[m].search(xq, k)
            t2 = time.perf_counter()
            rounds.append(dict(flat_device_ms=f_ms, flat_calls=f_reps, ivf1_device_ms=v_ms, ivf1_calls=v_reps,
                               stateless_host_ms=(t1 - t0) * 1e3, flat_host_ms=(t2 - t1) * 1e3))
        same_as_stateless = bool(np.array_equal(Ih, Is) and np.array_equal(Dh, Ds)
                                 and np.array_equal(Id.cpu().numpy(), Is) and np.array_equal(Dd.cpu().numpy(), Ds))
        plan = flat_search_plan(nq, nb, k)
        tile_q = plan["tile_q"]
        tiles = -(-nq // tile_q)
        med = lambda key: sorted(r[key] for r in rounds)[1]  # noqa: E731
        results.append(dict(
            d=d, nb=nb, nq=nq, k=k, metric="ip" if m == IP else "l2", plan=plan,
            rounds=rounds, flat_device_ms=med("flat_device_ms"), ivf1_device_ms=med("ivf1_device_ms"),
            stateless_host_ms=med("stateless_host_ms"), flat_host_ms=med("flat_host_ms"),
            faster_than_stateless_in_every_pair=all(r["flat_host_ms"] < r["stateless_host_ms"] for r in rounds),
            faster_than_ivf1_in_every_round=all(r["flat_device_ms"] < r["ivf1_device_ms"] for r in rounds),
            results_equal_stateless=same_as_stateless,
            labels_equal_ivf1=float((Iv.cpu().numpy() == Is).mean()),
            mfma_floor_ms=2.0 * nq * nb * d / MFMA_F32_FLOPS * 1e3,
            mfma_floor_tiles_ms=2.0 * tiles * tile_q * nb * d / MFMA_F32_FLOPS * 1e3,
            byte_floor_ms=4.0 * nb * d * tiles / read_rate * 1e3))
        print("SHAPE " + json.dumps(results[-1]), flush=True)
    return dict(d=d, nb=nb, hbm_read_bytes_per_s=read_rate, add_and_upload_seconds={"l2": t_add[L2], "ip": t_add[IP]},
                shapes=results)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "indexflat_bench.json"))
    ap.add_argument("--nb", type=int, default=1_000_000)
    ap.add_argument("--dims", default="128,768")
    ap.add_argument("--step", type=int)
    a = ap.parse_args()
    if a.step:  # child: one GPU step, one JSON line
        print("RESULT " + json.dumps(step_d(a.step, a.nb)), flush=True)
        return 0
    result = {"nb": a.nb, "nq": NQ, "mfma_f32_flops": MFMA_F32_FLOPS, "dims": {}}
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
                print(f"  done d={d} nq={s['nq']} k={s['k']} {s['metric']}", flush=True)
        p.wait()
        if p.returncode != 0 or not lines:
            sys.stderr.write("".join(tail))
            sys.stderr.write(f"\nstep d={d} failed (exit {p.returncode}); stopping\n")
            return 1
        r = json.loads(lines[-1][7:])
        for s in r["shapes"]:
            print(f"d={d} nq={s['nq']} k={s['k']} {s['metric']}: flat {s['flat_device_ms']:.3f} ms, "
                  f"IVF1,Flat {s['ivf1_device_ms']:.3f} ms, stateless host {s['stateless_host_ms']:.1f} ms, "
                  f"flat host {s['flat_host_ms']:.1f} ms, floors mfma {s['mfma_floor_ms']:.3f} / bytes "
                  f"{s['byte_floor_ms']:.3f} ms", flush=True)
        result["dims"][str(d)] = r
        with open(a.out, "w") as f:  # (rewritten after every step: a later step's failure keeps the earlier numbers)
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
