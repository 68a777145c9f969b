#!/usr/bin/env python
"""Secondary measurement: HDBSCAN (trase_amd.segment.hdbscan) at D = 32 and n = 6000 (2 % of 300k Gaussians: the viewer's
sample), 30 000 and 65 536 rows of seeded unit-normalised blobs, by phase:

  core_ms        trase_hdbscan_core: the k-th neighbour distances             HIP events
  mst_ms         trase_hdbscan_mst: the Boruvka rounds                        HIP events
  host_ms        the one read-back, the key sort and hdbscan_hierarchy        wall clock
  total_ms       segment.hdbscan(...), upload excluded, labels on the device  wall clock
  sklearn_ms     sklearn.cluster.HDBSCAN(algorithm="brute", n_jobs=16) on the same rows on this machine's CPUs, taking turns
                 with ours; null when scikit-learn is not importable, and above --sklearn-max rows (default 6000: its
                 dense n x n float64 matrices take 7 GB apiece at 30 000 rows)

Medians of --reps (default 30; scikit-learn: --sklearn-reps).

    python profiles/bench_hdbscan.py > profiles/hdbscan_bench.json"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trase_amd import segment  # noqa: E402

D, K, EPS = 32, 10, 0.01


def blobs(n, seed):
    g = np.random.default_rng(seed)
    nb = max(6, n // 500)
    c = g.standard_normal((nb, D))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    x = c[g.integers(0, nb, n)] + 0.05 * g.standard_normal((n, D))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def median(v):
    return float(np.median(v)) if len(v) else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--sklearn-reps", type=int, default=5)
    ap.add_argument("--sklearn-max", type=int, default=6000)
    ap.add_argument("--sizes", type=int, nargs="*", default=[6000, 30_000, 65_536])
    args = ap.parse_args()
    try:
        from sklearn.cluster import HDBSCAN
    except ImportError:
        HDBSCAN = None
    dev = torch.device("cuda", 0)
    rows = []
    for n in args.sizes:
        Xh = blobs(n, seed=n)
        X = torch.from_numpy(Xh).to(dev)
        for _ in range(2):
            labels = segment.hdbscan(X, min_cluster_size=K, cluster_selection_epsilon=EPS)
        torch.cuda.synchronize()
        core, mst, host, total, sk = [], [], [], [], []
        sk_every = max(1, args.reps // max(1, args.sklearn_reps))
        for rep in range(args.reps):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            from trase_amd import _lib
            import ctypes as C
            lib = _lib.load()
            sz = C.c_size_t()
            _lib.check(lib.trase_hdbscan_sizes(n, D, K, C.byref(sz)), "hdbscan")
            ws = torch.empty(sz.value, dtype=torch.uint8, device=dev)
            core2 = torch.empty(n, dtype=torch.float32, device=dev)
            out = torch.empty(n + 9, dtype=torch.int64, device=dev)
            st = torch.cuda.current_stream(dev).cuda_stream
            e[0].record()
            _lib.check(lib.trase_hdbscan_core(_lib.ptr(X), n, D, K, _lib.ptr(core2), _lib.ptr(ws), ws.numel(), 0, st), "core")
            e[1].record()
            _lib.check(lib.trase_hdbscan_mst(_lib.ptr(X), n, D, _lib.ptr(core2), _lib.ptr(out), _lib.ptr(out[n:]), _lib.ptr(ws),
                                             ws.numel(), 0, st), "mst")
            e[2].record()
            torch.cuda.synchronize()
            core.append(e[0].elapsed_time(e[1]))
            mst.append(e[1].elapsed_time(e[2]))
            t0 = time.perf_counter()
            edges = segment._mst_edges(out.cpu().numpy(), n)
            segment.hdbscan_hierarchy(edges, n, min_cluster_size=K, cluster_selection_epsilon=EPS)
            host.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            labels = segment.hdbscan(X, min_cluster_size=K, cluster_selection_epsilon=EPS)
            torch.cuda.synchronize()
            total.append((time.perf_counter() - t0) * 1e3)
            if HDBSCAN is not None and n <= args.sklearn_max and rep % sk_every == 0 and len(sk) < args.sklearn_reps:
                t0 = time.perf_counter()
                ref = HDBSCAN(min_cluster_size=K, min_samples=K + 1, cluster_selection_epsilon=EPS, algorithm="brute",
                              n_jobs=16).fit_predict(Xh.astype(np.float64))
                sk.append((time.perf_counter() - t0) * 1e3)
        counts = out[n:].view(torch.int32).cpu().numpy()
        row = {"n": n, "D": D, "min_samples": K, "core_ms": median(core), "mst_ms": median(mst), "host_ms": median(host),
               "total_ms": median(total), "sklearn_ms": median(sk), "sklearn_reps": len(sk), "reps": args.reps,
               "boruvka_rounds": int((counts > 0).sum()) - 1, "clusters": int(labels.max()) + 1,
               "noise": int((labels < 0).sum())}
        if sk:
            row["sklearn_clusters"] = int(ref.max()) + 1
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "results": rows}, indent=1))


if __name__ == "__main__":
    main()
