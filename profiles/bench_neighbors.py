#!/usr/bin/env python
"""Secondary measurement: the wide k-NN, the transposed graph and the two k-NN graph losses at N = 300 000 points of the S4
scene, each against a torch composition on the same GPU in the same process, the sides taking turns, timed with HIP events,
medians of --reps runs after a pre-roll:

  knn_points, K = 17 / 129 / 256   all N queries, against torch.cdist + topk over chunks of 1024 queries (timed on --cdist-queries
                                   queries and scaled to N: the whole pass takes seconds)
  NeighborGraph.from_idx, k = 128  the radix sort over the targets + the range pass
  loss_reg_3d_feature              forward + backward on a prebuilt graph (k = 16, D = 32) against the reference's statements
                                   (utils/loss_utils.py:146-151) around the same indices
  loss_rigid_body_motion_reg_loss  one cluster of --rigid-n points, 128 neighbours, forward + backward, against the reference's
                                   statements (:197-214) around the same indices; and torch.svd + its backward alone on the
                                   same moment matrices: the share of the loss that stays in torch
  bench.py                         this tree's library and --parent-lib (the parent commit's build) taking turns, twice each, as
                                   fresh child processes under a time limit; a child that ends with a non-zero status or
                                   without a result line ends this script at once: nothing more is started on the card

    python profiles/bench_neighbors.py --parent-lib /path/to/parent/libtrase_rast.so --tests-log LOG > profiles/neighbors_bench.json

--tests-log: the output of `pytest tests/test_gpu_neighbors.py -s`; the distances from float64 that the rigid-loss tests measured
(the kernels, the fp32 compositions, the bar) are copied into the result under "tests".
"""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trase_amd import neighbors as nb  # noqa: E402
from trase_amd.rasterizer import knn_points  # noqa: E402
from trase_amd.synthetic import make_scene  # noqa: E402

N = 300_000


def alternate(fns, reps, warmup=2):
    """Median and minimum HIP-event time in ms of every function, the functions taking turns."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for fn, out in zip(fns, times):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b))
    return [(round(sorted(t)[len(t) // 2], 4), round(min(t), 4)) for t in times]


def cdist_topk(q, cloud, K, chunk=1024):
    out = []
    for lo in range(0, q.shape[0], chunk):
        out.append(torch.cdist(q[lo:lo + chunk], cloud).topk(K, largest=False).indices)
    return torch.cat(out)


def reference_feature_loss(feats, ijs):
    n, k = ijs.shape
    aux = torch.arange(n, device=feats.device).unsqueeze(-1).expand(n, k).reshape(-1)
    s = torch.sigmoid
    kl = s(feats[aux]) * (torch.log(s(feats[aux]) + 1e-10) - torch.log(s(feats[ijs.reshape(-1)]) + 1e-10))
    return kl.mean()


def reference_rigid(p1, p2, ijs):
    n, k = ijs.shape
    aux = torch.arange(n, device=p1.device).unsqueeze(-1).expand(n, k).reshape(-1)
    e1 = (p1[aux] - p1[ijs.reshape(-1)]).reshape(n, k, 3)
    e2 = (p2[aux] - p2[ijs.reshape(-1)]).reshape(n, k, 3)
    S = torch.bmm(e1.transpose(1, 2), e2)
    U, _, V = torch.svd(S)
    R = torch.bmm(V, U.transpose(1, 2))
    return (e1 - torch.bmm(R, e2.transpose(1, 2)).transpose(1, 2)).pow(2).sum(2).sum(1).mean()


def bench_line(lib):
    env = dict(os.environ)
    if lib:
        env["TRASE_RAST_LIB"], env["TRASE_RAST_LIB_AB"] = lib, "1"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "30", "--warmup", "5"],
                         env=env, capture_output=True, text=True, timeout=900)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    if out.returncode != 0 or not lines:
        # a child that failed may have faulted the card: nothing more is started on it, here or by a caller
        sys.stderr.write(out.stderr[-2000:])
        sys.exit(f"[bench_neighbors] bench.py ended with status {out.returncode} and {len(lines)} result lines"
                 f" (library: {lib or 'this tree'}): stopping, nothing further is launched")
    line = json.loads(lines[-1])
    return {k: line[k] for k in ("metric", "value", "unit", "steps", "warmup", "ms_per_step") if k in line}


def rigid_test_records(path):
    """{scene: {quantity: line}} from the printed lines of tests/test_gpu_neighbors.py's rigid-loss tests."""
    out, scene = {}, None
    for ln in open(path, errors="replace"):
        ln = ln.strip().lstrip(".")
        if ln.startswith("rigid loss, "):
            scene = ln[len("rigid loss, "):]
            out[scene] = {}
        elif scene and ln.split(":")[0] in ("loss", "gradient to xyz1", "gradient to xyz2") and "kernels" in ln:
            out[scene][ln.split(":")[0]] = ln.split(": ", 1)[1]
        elif ln.startswith("tiny clusters add"):
            out["tiny clusters"] = ln
        elif ln.startswith("three clusters, 4 neighbours"):
            out["four neighbours, large clusters"] = ln
    return out


def bound_test_records(path):
    """The largest figures among the printed lines of the other tests: the share of a derived bound that the feature loss and
    the edge sums use, and the relative distance error and the near-tie rows of the k-NN on random clouds."""
    share, dist_err, ties, differ = 0.0, 0.0, 0, 0
    for ln in open(path, errors="replace"):
        ln = ln.strip().lstrip(".")
        if ln.endswith("of its bound"):
            share = max(share, float(ln.split(",")[-1].split()[0]))
        elif "largest relative distance error" in ln:
            dist_err = max(dist_err, float(ln.split("largest relative distance error")[1].split()[0]))
        elif ln.startswith("rows with a near-tie at the K-th place"):
            ties = max(ties, int(ln.split(":")[1].split(";")[0]))
            differ = max(differ, int(ln.rsplit(":", 1)[1]))
    return {"largest_share_of_a_derived_bound": share, "knn_random_clouds_largest_relative_distance_error": dist_err,
            "knn_random_clouds_most_near_tie_rows_of_5000": ties, "knn_random_clouds_most_rows_with_another_index_set": differ}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--cdist-queries", type=int, default=8192)
    ap.add_argument("--rigid-n", type=int, default=100_000)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--skip-bench", action="store_true")
    ap.add_argument("--tests-log", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    xyz = make_scene(N, feat_dim=1, seed=3).xyz.to(dev).contiguous()
    res = {"n": N, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "arch": torch.cuda.get_device_properties(0).gcnArchName, "compute_units": torch.cuda.get_device_properties(0).multi_processor_count}
    note = lambda what: print("[bench_neighbors]", what, file=sys.stderr, flush=True)          # noqa: E731

    res["knn"] = {}
    q = xyz[:a.cdist_queries]
    for K in (17, 129, 256):
        note(f"knn K = {K}")
        ours = lambda: knn_points(xyz[None], xyz[None], K=K)                  # noqa: E731
        (t, tmin), = alternate([ours], a.reps)
        (c, cmin), = alternate([lambda: cdist_topk(q, xyz, K)], 5, warmup=1)
        same = (knn_points(q[None], xyz[None], K=K).idx[0].sort(1).values == cdist_topk(q, xyz, K).sort(1).values).all(1)
        res["knn"][f"K{K}"] = {"knn_points_ms": t, "min_ms": tmin, "cdist_topk_ms_for_queries": [a.cdist_queries, c, cmin],
                               "cdist_topk_ms_scaled_to_n": round(c * N / a.cdist_queries, 1),
                               "rows_with_the_same_index_set_as_cdist_topk": [int(same.sum()), int(same.numel())]}

    note("graph reversal")
    idx128 = knn_points(xyz[None], xyz[None], K=129).idx[0][:, 1:].to(torch.int32).contiguous()
    (t, tmin), = alternate([lambda: nb.NeighborGraph.from_idx(idx128)], a.reps)
    res["graph_reverse_k128"] = {"ms": t, "min_ms": tmin, "edges": int(idx128.numel())}

    note("feature loss")
    g = torch.Generator().manual_seed(1)
    D, k = 32, 16
    feats = torch.randn(N, D, generator=g).to(dev).requires_grad_(True)
    graph = nb.NeighborGraph.build(xyz, k)
    ijs = graph.idx.long()

    def ours_feat():
        feats.grad = None
        nb.loss_reg_3d_feature(feats, xyz, k, graph=graph).backward()

    def ref_feat():
        feats.grad = None
        reference_feature_loss(feats, ijs).backward()
    (t, tmin), (r, rmin) = alternate([ours_feat, ref_feat], a.reps)
    ours_feat()
    g_ours = feats.grad.clone()
    ref_feat()
    res["feature_loss"] = {"D": D, "k": k, "fwd_bwd_ms": t, "reference_statements_ms": r, "ratio": round(r / t, 2),
                           "min_ms": [tmin, rmin], "largest_gradient_difference": float((g_ours - feats.grad).abs().max()),
                           "largest_gradient": float(feats.grad.abs().max())}

    note("rigid loss")
    n = a.rigid_n
    p1 = xyz[:n].clone().requires_grad_(True)
    p2 = (xyz[:n] * 1.02 + 0.01 * torch.randn(n, 3, generator=g).to(dev)).requires_grad_(True)
    cid = torch.zeros(n, dtype=torch.long, device=dev)
    rgraph = nb.NeighborGraph.build(p1, 128)
    rij = rgraph.idx.long()
    S = nb.edge_moments(p1, p2, rgraph).detach().requires_grad_(True)

    def ours_rigid():
        p1.grad = p2.grad = None
        nb.loss_rigid_body_motion_reg_loss(p1, p2, cid, num_neighbors=128).backward()

    def ref_rigid():
        p1.grad = p2.grad = None
        reference_rigid(p1, p2, rij).backward()

    def svd_alone():
        S.grad = None
        U, _, V = torch.svd(S)
        torch.bmm(V, U.transpose(1, 2)).sum().backward()

    def knn_alone():
        knn_points(p1.detach()[None], p1.detach()[None], K=129)
    (t, tmin), (r, rmin), (s, smin), (kq, kmin) = alternate([ours_rigid, ref_rigid, svd_alone, knn_alone], a.reps)
    res["rigid_loss"] = {"n": n, "num_neighbors": 128, "fwd_bwd_ms_with_knn": t, "reference_statements_ms_without_knn": r,
                         "torch_svd_fwd_bwd_ms": s, "knn_ms": kq, "svd_share": round(s / t, 3), "min_ms": [tmin, rmin, smin, kmin]}

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
        res["tests"] = {"rigid_loss_distance_from_float64": rigid_test_records(a.tests_log), **bound_test_records(a.tests_log)}
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
