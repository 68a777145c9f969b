#!/usr/bin/env python
"""Secondary measurement: the segmentation stage (gui.py:248-270 K-means, render.py:334-345 query masks) at S4 size,
N = 300k Gaussians with D = 32 features -- the HIP Lloyd loop of trase_amd/segment.py against the float64-checked torch
restatement of kmeans_pytorch 0.3's loop (tests/segment_reference.py: an N x K x D broadcast and K nonzero host syncs per
iteration), both on the same GPU in the same process, alternating, with a fixed iteration count (iter_limit = 30,
tol = 0) so both do equal work; segment_mask at S = 3 against the render.py per-id composition; and the prompt lift
(``lift_votes``: one fused pass over the hash of the points) against the composition of render.py:208-231 around this
repository's ``knn_points`` shim at K = 1, at 300k points and 1080p for prompt masks of 1 %, 10 % and 100 % of the image
(the scene of tests/test_gpu_lift.py), alternating the two.

    python profiles/bench_segment.py                          # one JSON line
    python profiles/bench_segment.py --lift-only              # only the "lift" rows
    python profiles/bench_segment.py --profile-k 16           # only the HIP steps at K = 16 (run under rocprofv3)
    python profiles/bench_segment.py --kernel-stats 16=a.csv --kernel-stats 64=b.csv
        # adds bytes per step over the step kernels' time from `rocprofv3 --kernel-trace --stats` runs of --profile-k

Bytes per step are computed from shapes: X read once (N D 4), ids written (N 4), the block slabs written and read back
(2 G K (D + 1) 4), the centres and the state word (negligible, counted)."""
import argparse
import csv
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import segment_reference as sr  # noqa: E402
from trase_amd import segment  # noqa: E402
from trase_amd.synthetic import make_scene  # noqa: E402

N, D, ITERS = 300_000, 32, 30
THRESHOLD = 0.1          # gui.py's default score_threshold (the synthetic features are not trained: 0.8 selects none)
STEP_KERNELS = ("seg_assign_accum_kernel", "seg_reduce_kernel", "kmeans_finalize_kernel")


def features(dev):
    f = make_scene(N, feat_dim=D, seed=0).gaussian_features.reshape(N, D).to(dev)
    return torch.nn.functional.normalize(f, dim=-1, p=2)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return sorted(out)[len(out) // 2]


def step_loop(X, K):
    centres0 = X[torch.as_tensor(sr.init_indices(N, K, 0), device=X.device)].contiguous()
    ws = torch.empty(segment._kmeans_sizes(N, D, K), dtype=torch.uint8, device=X.device)
    ids = torch.empty(N, dtype=torch.int32, device=X.device)
    state = torch.zeros(4, dtype=torch.int32, device=X.device)

    def run():
        c = centres0.clone()
        state.zero_()
        segment._kmeans_steps(X, c, ids, 0, 0.0, 0, ITERS, state, ws)
    return run


def bytes_per_step(K):
    G = min(256, max(1, (N + 511) // 512))
    return N * D * 4 + N * 4 + 2 * G * K * (D + 1) * 4 + 2 * K * D * 4 + 16


def kernel_us_per_step(path):
    total_ns, calls = 0.0, {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name") or row.get("KernelName") or ""
            for k in STEP_KERNELS:
                if k in name:
                    total_ns += float(row["TotalDurationNs"])
                    calls[k] = calls.get(k, 0) + int(row["Calls"])
    steps = calls.get("kmeans_finalize_kernel", 0)
    return (total_ns / steps / 1e3 if steps else None), steps


def lift_composition(depth, text_mask, view, xyz, cluster_ids_x, threshold):
    """render.py:208-231 as torch ops on the device around the knn_points shim: what a user composed before lift_votes."""
    from pytorch3d.ops import knn_points
    depth = depth.squeeze()
    h, w = depth.shape
    grid_index = torch.stack(torch.meshgrid([torch.arange(h), torch.arange(w)], indexing="ij"), dim=-1).to(depth.device)
    z = view.zfar / (view.zfar - view.znear) * depth[text_mask] - view.zfar * view.znear / (view.zfar - view.znear)
    uvz = torch.cat(((((grid_index[text_mask, :][:, 1] - 0.5) / view.image_width * 2 - 1) * depth[text_mask]).unsqueeze(-1),
                     (((grid_index[text_mask, :][:, 0] - 0.5) / view.image_height * 2 - 1) * depth[text_mask]).unsqueeze(-1),
                     z.unsqueeze(-1), depth[text_mask].unsqueeze(-1)), 1)
    points = uvz @ (torch.inverse(view.full_proj_transform))[:, :3]
    ijs = knn_points(points.unsqueeze(0), xyz.unsqueeze(0), K=1).idx.squeeze(0).squeeze(-1)
    votes = torch.bincount(cluster_ids_x[ijs].int())
    return votes, torch.where(votes > threshold, 1, 0).nonzero()


def lift_rows(dev, reps):
    from tests.test_gpu_lift import K_FULL, _blob, _full_scene
    cam, depth, points, ids, (rr, cc) = _full_scene()
    cam, depth, points, ids = cam.to(dev), depth.to(dev), points.to(dev), ids.to(dev)
    rows = {"n": int(points.shape[0]), "image": [cam.image_width, cam.image_height], "bins": K_FULL}
    for share in (0.01, 0.10, 1.0):
        mask = torch.from_numpy(_blob(rr, cc, share)).to(dev)
        threshold = int(mask.sum()) // (2 * K_FULL)
        fused = lambda: segment.prompt_clusters(depth, mask, cam, points, ids, threshold, num_clusters=K_FULL)   # noqa: E731
        composed = lambda: lift_composition(depth, mask, cam, points, ids.float(), threshold)                    # noqa: E731
        a, (v, b) = fused(), composed()
        torch.cuda.synchronize()
        hip, ref = [], []
        for _ in range(reps):       # alternating
            for fn, out in ((fused, hip), (composed, ref)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                out.append((time.perf_counter() - t0) * 1e3)
        hip_ms, ref_ms = sorted(hip)[len(hip) // 2], sorted(ref)[len(ref) // 2]
        votes = segment.lift_votes(depth, mask, cam, points, ids, num_clusters=K_FULL)
        rows[f"mask_{int(round(share * 100))}pct"] = {
            "prompted_pixels": int(mask.sum()), "lift_votes_ms": round(hip_ms, 4), "torch_render_py_knn_shim_ms": round(ref_ms, 4),
            "speedup": round(ref_ms / hip_ms, 1), "min_ms": [round(min(hip), 4), round(min(ref), 4)],
            "votes_differing_from_composition": int((votes[:v.numel()] != v).sum()),
            "chosen_ids_equal": bool(torch.equal(a, b.flatten()))}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lift-only", action="store_true")
    ap.add_argument("--profile-k", type=int, default=0)
    ap.add_argument("--kernel-stats", action="append", default=[])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    if a.lift_only:
        print(json.dumps({"lift": lift_rows(dev, max(a.reps, 11))}))
        return
    X = features(dev)
    if a.profile_k:
        run = step_loop(X, a.profile_k)
        for _ in range(10):
            run()
        torch.cuda.synchronize()
        return
    res = {"n": N, "d": D, "iter_limit": ITERS}
    for K in (16, 64):
        run = step_loop(X, K)
        step_ms = timed(run, a.reps) / ITERS
        hip, lib = [], []
        for _ in range(a.reps):     # alternating: HIP kmeans call, torch restatement of the library's loop
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ids, c, it = segment.kmeans(X, K, tol=0.0, iter_limit=ITERS, seed=0)
            torch.cuda.synchronize()
            hip.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            l_ids, l_c, l_it = sr.library_kmeans(X, K, tol=0.0, iter_limit=ITERS, seed=0)
            torch.cuda.synchronize()
            lib.append((time.perf_counter() - t0) * 1e3)
        hip_ms, lib_ms = sorted(hip)[len(hip) // 2], sorted(lib)[len(lib) // 2]
        res[f"k{K}"] = {"step_ms": round(step_ms, 4), "kmeans_call_ms": round(hip_ms, 3), "torch_library_loop_ms": round(lib_ms, 3),
                        "speedup": round(lib_ms / hip_ms, 1), "iterations": [it, l_it],
                        "ids_agree_with_torch": round(float((ids == l_ids).double().mean()), 6),
                        "bytes_per_step": bytes_per_step(K)}
    for spec in a.kernel_stats:
        k, path = spec.split("=", 1)
        us, steps = kernel_us_per_step(path)
        e = res[f"k{int(k)}"]
        e["kernel_us_per_step"] = round(us, 2) if us else None
        e["profiled_steps"] = steps
        e["achieved_GBps"] = round(e["bytes_per_step"] / (us * 1e3), 1) if us else None
    # segment_mask at S = 3 against the render.py per-id composition
    ids16, _, _ = segment.kmeans(X, 16, seed=0)
    sel, thr = [1, 5, 9], THRESHOLD
    m_hip = segment.segment_mask(X, ids16, sel, thr)
    m_ref = sr.render_masks_torch(X, ids16, sel, thr)
    t_hip = timed(lambda: segment.segment_mask(X, ids16, sel, thr), 20)
    t_ref = timed(lambda: sr.render_masks_torch(X, ids16, sel, thr), 20)
    res["segment_mask_s3"] = {"score_threshold": thr, "hip_ms": round(t_hip, 4), "torch_render_py_ms": round(t_ref, 4), "speedup": round(t_ref / t_hip, 1),
                              "selected": int(m_hip.sum()), "mask_bits_differing": int((m_hip != m_ref).sum())}
    res["lift"] = lift_rows(dev, max(a.reps, 11))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
