#!/usr/bin/env python
"""Secondary measurement: the rigid-motion loss with rotation="svd" (torch.svd and its autograd between the two edge kernels) and
rotation="polar" (rigid_fit: the rotation and its closed-form gradient inside one kernel each way), on one cluster of --n points
of the S4 scene with 128 and 16 neighbours.  The two paths take turns in one process, timed with HIP events, medians of --reps
runs after a pre-roll:

  the whole loss, forward + backward, k-NN and graph transpose included (what a training step pays), and its gradients compared
  the k-NN + transpose alone (NeighborGraph.build)
  on a prebuilt graph, forward and backward apart: rigid_fit against edge_moments -> torch.svd -> bmm -> edge_residual
  the fused kernels' own times from the library's profiling scopes, beside the bytes they must move at least once
  bench.py: this tree's library and --parent-lib (the parent commit's build) taking turns, twice each, as fresh child processes; a
  child that fails ends this script at once (no rendering code differs: a control)

    python profiles/bench_rigid.py --parent-lib /path/to/parent/libtrase_rast.so --tests-log LOG > profiles/rigid_bench.json

--tests-log: the output of `pytest tests/test_gpu_rigid.py -s`; the shares of the derived bounds and the distances from float64 it
printed are copied into the result under "tests".
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_neighbors import bench_line  # noqa: E402
from trase_amd import neighbors as nb  # noqa: E402
from trase_amd.rasterizer import profile_enable, profile_report  # noqa: E402
from trase_amd.synthetic import make_scene  # noqa: E402


def alternate(items, reps, warmup=3):
    """items: (setup or None, fn).  Median and minimum HIP-event time in ms of every fn, the items taking turns; setup runs
    untimed before its fn and its result is passed on."""
    def once(setup, fn):
        arg = setup() if setup else None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(arg) if setup else fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)
    for _ in range(warmup):
        for setup, fn in items:
            once(setup, fn)
    times = [[] for _ in items]
    for _ in range(reps):
        for (setup, fn), out in zip(items, times):
            out.append(once(setup, fn))
    return [{"median_ms": round(sorted(t)[len(t) // 2], 4), "min_ms": round(min(t), 4)} for t in times]


def test_records(path):
    """The largest share of a derived bound per quantity, and the whole-loss lines, from the printed output of the GPU tests."""
    shares, lines = {}, {}
    scene = None
    for ln in open(path, errors="replace"):
        ln = ln.strip().lstrip(".")
        if ln.endswith("of the bound"):
            tag = ln.split(":")[-2].strip() if ln.count(":") >= 2 else ln.split(":")[0].strip()
            shares[tag] = max(shares.get(tag, 0.0), float(ln.rsplit(":", 1)[1].split()[0]))
        elif ln.startswith("rigid loss, rotation polar, "):
            scene = ln[len("rigid loss, rotation polar, "):].split(":")[0]
        elif scene and ln.split(":")[0] in ("loss", "gradient to xyz1", "gradient to xyz2") and "polar" in ln:
            lines.setdefault(scene, {})[ln.split(":")[0]] = ln.split(": ", 1)[1]
    return {"largest_share_of_a_derived_bound": shares, "rigid_loss_distance_from_float64": lines}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--skip-bench", action="store_true")
    ap.add_argument("--tests-log", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = a.n
    g = torch.Generator().manual_seed(1)
    xyz = make_scene(300_000, feat_dim=1, seed=3).xyz.to(dev).contiguous()
    p1 = xyz[:n].clone().requires_grad_(True)
    p2 = (xyz[:n] * 1.02 + 0.01 * torch.randn(n, 3, generator=g).to(dev)).requires_grad_(True)
    cid = torch.zeros(n, dtype=torch.long, device=dev)
    res = {"n": n, "reps": a.reps, "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName}
    note = lambda what: print("[bench_rigid]", what, file=sys.stderr, flush=True)          # noqa: E731

    for k in (128, 16):
        note(f"k = {k}")

        def whole(rotation):
            def fn():
                p1.grad = p2.grad = None
                nb.loss_rigid_body_motion_reg_loss(p1, p2, cid, num_neighbors=k, rotation=rotation).backward()
            return fn
        graph = nb.NeighborGraph.build(p1, k)

        def fwd_svd():
            S = nb.edge_moments(p1, p2, graph)
            U, _, V = torch.svd(S)
            return nb.edge_residual(p1, p2, graph, torch.bmm(V, U.transpose(1, 2))).mean()

        def fwd_polar():
            return nb.rigid_fit(p1, p2, graph).mean()

        def bwd(loss):
            p1.grad = p2.grad = None
            loss.backward()
        t = alternate([(None, whole("svd")), (None, whole("polar")), (None, lambda: nb.NeighborGraph.build(p1, k)),
                       (None, fwd_svd), (None, fwd_polar), (fwd_svd, bwd), (fwd_polar, bwd)], a.reps)
        grads = []
        for rotation in ("svd", "polar"):
            whole(rotation)()
            grads.append((p1.grad.clone(), p2.grad.clone()))
        profile_enable(1)
        for _ in range(5):
            bwd(fwd_polar())
        torch.cuda.synchronize()
        scopes = profile_report()
        profile_enable(0)
        res[f"k{k}"] = {
            "whole_loss_fwd_bwd_with_knn": {"svd": t[0], "polar": t[1]}, "knn_and_transpose": t[2],
            "forward_on_a_prebuilt_graph": {"svd": t[3], "polar": t[4]}, "backward_on_a_prebuilt_graph": {"svd": t[5], "polar": t[6]},
            "fused_kernels_from_the_profiling_scopes": {s: scopes[s] for s in ("rigid_fit_fwd", "rigid_fit_bwd") if s in scopes},
            # read or written at least once; the gathers of the neighbour rows come on top and are served by L2
            "bytes_at_least": {"rigid_fit_fwd": n * (24 + 4 * k + 4 + 36 + 64), "rigid_fit_bwd": n * (24 + 8 + 4 * k + 36 + 64 + 4 + 24)},
            "largest_gradient_difference_between_the_paths": [float((grads[0][i] - grads[1][i]).abs().max()) for i in range(2)],
            "largest_gradient": [float(grads[0][i].abs().max()) for i in range(2)]}

    if not a.skip_bench:
        torch.cuda.synchronize()          # a fault of the measurements above raises here, before any child is started
        runs = []
        for turn in range(2):
            note(f"bench.py, turn {turn}")
            runs.append({"tree": bench_line(None)})
            if a.parent_lib:
                runs[-1]["parent"] = bench_line(a.parent_lib)
        res["bench"] = runs
    if a.tests_log:
        res["tests"] = test_records(a.tests_log)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
