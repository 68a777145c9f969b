#!/usr/bin/env python
"""Secondary measurement: the display stage at S4 size -- N = 300k Gaussians, 1080p, D = 32 features -- each HIP function of
trase_amd/display.py and ``segment.assign_clusters`` against the torch composition of the reference statements it replaces,
both on the same GPU in the same process, alternating, timed with HIP events after a warm-up:

  splat_points at L = 1 and L = 3     render.py:247-260 (the dots) and :247-294 (dots, cluster colours, PCA colours)
  feature_colors                      render.py:52-59 feature3d_to_rgb (QR + SVD through torch.linalg on the device)
  assign_clusters at K = 16 and 256   gui.py:276 + :288-290 with the reference's .cpu() copies, and the same einsum kept on
                                      the device (what a user who only removed the copies would run)

    python profiles/bench_display.py > profiles/display_bench.json
    python profiles/bench_display.py --reps 50

Medians in milliseconds; "per_launch_us" are the profiling scopes of the library around each kernel of one call."""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trase_amd import _lib, display, segment  # noqa: E402
from trase_amd.synthetic import make_scene, orbit_camera  # noqa: E402

N, D, W, H = 300_000, 32, 1920, 1080


def feature3d_to_rgb(x, n_components=3):
    """render.py:52-59."""
    X_center = x - torch.mean(x, axis=0)
    q, r = torch.linalg.qr(X_center)
    U, s, Vt = torch.linalg.svd(r, full_matrices=False)
    x_compress = torch.matmul(U[:, :n_components], torch.diag(s[:n_components]))
    pca_result = torch.matmul(q, x_compress)
    return (pca_result - pca_result.min()) / (pca_result.max() - pca_result.min())


def splat_composition(pts, view, layers, white_background=False):
    """render.py:247-294 for the given colour layers (None: the dots)."""
    cur_pts = torch.cat([pts, torch.ones_like(pts[..., :1])], dim=-1)
    cur_pts2d = cur_pts @ view.full_proj_transform
    cur_pts2d = cur_pts2d[..., :2] / cur_pts2d[..., -1:]
    cur_pts2d = (cur_pts2d + 1) / 2 * torch.tensor([view.image_width, view.image_height]).cuda()
    mask_1 = (cur_pts2d[:, 0] > 0) & (cur_pts2d[:, 0] < view.image_width)
    mask_2 = (cur_pts2d[:, 1] > 0) & (cur_pts2d[:, 1] < view.image_height)
    final_mask = mask_1 & mask_2
    out = []
    for colors in layers:
        size = (3, view.image_height, view.image_width)
        buffer_image = torch.zeros(size=size).cuda() if not white_background else torch.ones(size=size).cuda()
        for c in range(3):
            value = (1 if not white_background else 0) if colors is None else colors[final_mask, c]
            buffer_image[c, (cur_pts2d[final_mask, 1]).type(torch.long), (cur_pts2d[final_mask, 0]).type(torch.long)] = value
        out.append(buffer_image)
    return out


def alternate(fns, reps, warmup=3):
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


def per_launch_us(fn):
    lib = _lib.load()
    buf = ctypes.create_string_buffer(65536)
    fn()
    torch.cuda.synchronize()
    lib.trase_prof_enable(1)
    fn()
    torch.cuda.synchronize()
    lib.trase_prof_report(buf, len(buf))
    lib.trase_prof_enable(0)
    return json.loads(buf.value.decode("utf-8", "replace"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cam = orbit_camera(W, H, angle=0.3, radius=4.0).to(dev)
    scene = make_scene(N, feat_dim=D, seed=3)
    pts = scene.xyz.to(dev)
    feats = scene.gaussian_features.reshape(N, D).to(dev)
    g = torch.Generator().manual_seed(17)
    cluster_colors = torch.rand(16, 3, generator=g)[torch.randint(0, 16, (N,), generator=g)].to(dev)
    pca = display.feature_colors(feats)
    res = {"n": N, "d": D, "image": [W, H], "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    for name, layers in (("splat_l1", [None]), ("splat_l3", [None, cluster_colors, pca])):
        hip = lambda: display.splat_points(pts, cam, layers)                  # noqa: E731
        ref = lambda: splat_composition(pts, cam, layers)                     # noqa: E731
        (h, hmin), (r, rmin) = alternate([hip, ref], a.reps)
        ours, theirs = hip(), ref()
        res[name] = {"splat_points_ms": h, "torch_render_py_ms": r, "ratio": round(r / h, 2), "min_ms": [hmin, rmin],
                     "pixels_differing_from_composition": int(sum((x != y).any(0).sum() for x, y in zip(ours, theirs))),
                     "per_launch": per_launch_us(hip)}
    hip = lambda: display.feature_colors(feats)                               # noqa: E731
    ref = lambda: feature3d_to_rgb(feats)                                     # noqa: E731
    (h, hmin), (r, rmin) = alternate([hip, ref], a.reps)
    res["feature_colors"] = {"feature_colors_ms": h, "torch_feature3d_to_rgb_ms": r, "ratio": round(r / h, 2), "min_ms": [hmin, rmin],
                             "per_launch": per_launch_us(hip)}
    normed = torch.nn.functional.normalize(feats, dim=-1, p=2)
    for K in (16, 256):
        rows = torch.randperm(N, generator=g)[:K].to(dev)
        centres = torch.nn.functional.normalize(normed[rows] + 0.05 * torch.randn(K, D, generator=g).to(dev), dim=-1, p=2)
        centres_cpu = centres.cpu()
        hip = lambda: segment.assign_clusters(feats, centres)                 # noqa: E731
        ref_cpu = lambda: torch.einsum("nc,bc->bn", centres_cpu, torch.nn.functional.normalize(feats, dim=-1, p=2).cpu()).argmax(dim=-1).to(dev)   # noqa: E731
        ref_dev = lambda: torch.einsum("nc,bc->bn", centres, torch.nn.functional.normalize(feats, dim=-1, p=2)).argmax(dim=-1)                     # noqa: E731
        (h, hmin), (rc, rcmin), (rd, rdmin) = alternate([hip, ref_cpu, ref_dev], a.reps)
        res[f"assign_k{K}"] = {"assign_clusters_ms": h, "torch_gui_py_cpu_ms": rc, "torch_einsum_on_device_ms": rd,
                               "ratio_vs_gui_py": round(rc / h, 2), "ratio_vs_device_einsum": round(rd / h, 2),
                               "min_ms": [hmin, rcmin, rdmin], "ids_differing_from_device_einsum": int((hip() != ref_dev()).sum())}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
