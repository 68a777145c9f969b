#!/usr/bin/env python
"""Secondary measurement: the trajectory view and the frame finish at S4 size -- N = 300k Gaussians, 1080p, 512 trajectories
of 32 samples -- each HIP function of trase_amd/trajectory.py against a torch + numpy composition of the same operations,
both on the same GPU in the same process, alternating, timed with HIP events after a pre-roll:

  farthest_point_sample     the sampler as a Python loop of torch operations, one arg-max and one masked assignment per step
                            (the shape of utils/time_utils.py:375-396)
  TrajectoryOverlay.update  gather + torch projection + .cpu() + the line rule in numpy on the host, two images
                            (the shape of gui.py:1169-1191; the host lines are numpy here, not OpenCV)
  present_frame             F.interpolate + permute + clamp + .cpu() + the numpy blends of gui.py:1108-1122, against
                            present_frame + .cpu() (both sides pay the copy of the finished frame)

    python profiles/bench_trajectory.py > profiles/trajectory_bench.json

Medians in milliseconds over --reps runs (the host-side compositions of the overlay run --host-reps times: one takes most
of a second); "per_launch" are the profiling scopes of the library around the launches of one call."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import trajectory_reference as tr  # noqa: E402  (the numpy line rule)
from trase_amd import _lib, trajectory  # noqa: E402
from trase_amd.synthetic import make_scene, orbit_camera  # noqa: E402

N, W, H, GS, SAMP = 300_000, 1920, 1080, 512, 32


def torch_fps(xyz, npoint, start):
    """Farthest-point sampling as a loop of torch operations on the device."""
    n = xyz.shape[0]
    picked = torch.zeros(npoint, dtype=torch.long, device=xyz.device)
    nearest = torch.full((n,), 1e10, device=xyz.device)
    far = torch.tensor(start, device=xyz.device)
    for i in range(npoint):
        picked[i] = far
        d = ((xyz - xyz[far]) ** 2).sum(-1)
        closer = d < nearest
        nearest[closer] = d[closer]
        far = nearest.argmax()
    return picked


def host_overlay(ring, cam, colors):
    """Projection with torch, then the polylines drawn on the host into a colour and an alpha image."""
    pts = torch.cat([ring, torch.ones_like(ring[..., :1])], dim=-1)
    uv = pts @ cam.full_proj_transform
    uv = uv[..., :2] / uv[..., -1:]
    uv = ((uv + 1) / 2 * torch.tensor([cam.image_width, cam.image_height], device=ring.device)).cpu().numpy()
    ok = np.isfinite(uv).all(-1) & (np.abs(uv) < tr.COORD_LIMIT).all(-1)
    px = np.where(ok[..., None], uv, 0).astype(np.int32)
    alpha = np.zeros((cam.image_height, cam.image_width, 3), dtype=np.float32)
    img = np.zeros((cam.image_height, cam.image_width, 3), dtype=np.float32)
    for g in range(ring.shape[1]):
        for s in range(ring.shape[0] - 1):
            if ok[s, g] and ok[s + 1, g]:
                x, y = tr.line_pixels(px[s, g, 0], px[s, g, 1], px[s + 1, g, 0], px[s + 1, g, 1], cam.image_width, cam.image_height)
                alpha[y, x] = 1.0
                img[y, x] = colors[g]
    return np.concatenate([img, alpha[..., :1]], axis=-1)


def host_finish(image, size, control, overlay, tint):
    """gui.py:1085-1122 with the blends in numpy on the host."""
    b = torch.nn.functional.interpolate(image.unsqueeze(0), size=size, mode="bilinear", align_corners=False).squeeze(0)
    b = b.permute(1, 2, 0).contiguous().clamp(0, 1).contiguous().detach().cpu().numpy()
    b = b * (control.sum(axis=-1, keepdims=True) == 0) + control
    b = b * (1 - overlay[..., 3:]) + overlay[..., :3] * overlay[..., 3:]
    b += 0.3 * tint
    return b


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
    ap.add_argument("--host-reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cam = orbit_camera(W, H, angle=0.3, radius=4.0).to(dev)
    xyz = make_scene(N, feat_dim=1, seed=3).xyz.to(dev)
    res = {"n": N, "image": [W, H], "gs_num": GS, "samp_num": SAMP, "reps": a.reps, "host_reps": a.host_reps,
           "device": torch.cuda.get_device_name(0)}

    hip = lambda: trajectory.farthest_point_sample(xyz, GS, start=0)          # noqa: E731
    ref = lambda: torch_fps(xyz, GS, 0)                                       # noqa: E731
    (h, hmin), (r, rmin) = alternate([hip, ref], a.reps)
    res["sampler"] = {"farthest_point_sample_ms": h, "torch_loop_ms": r, "ratio": round(r / h, 2), "min_ms": [hmin, rmin],
                      "rows_differing_from_torch_loop": int((hip() != ref()).sum()), "per_launch": per_launch_us(hip)}

    view = trajectory.TrajectoryOverlay(GS, SAMP)
    rows = view.select(xyz, start=0)
    g = torch.Generator().manual_seed(5)
    walk = torch.cumsum(0.01 * torch.randn(2 * SAMP, GS, 3, generator=g), 0).to(dev)
    frames = []
    for k in range(2 * SAMP):                                                 # the tracked Gaussians drift, the others stay
        f = xyz.clone()
        f[rows] += walk[k]
        frames.append(f)
    colors = trajectory.jet_colors(GS)
    turn = [0]

    def hip():
        turn[0] += 1
        return view.update(frames[turn[0] % len(frames)], cam)
    (h, hmin), = alternate([hip], a.reps, warmup=SAMP)                        # the ring is full when the timing starts
    view.reset()
    for f in frames[:SAMP]:
        view.update(f, cam)
    held = view.coords()
    ref = lambda: host_overlay(torch.cat([held[1:], frames[SAMP][rows][None]]), cam, colors)   # noqa: E731
    (r, rmin), = alternate([ref], a.host_reps, warmup=1)
    ours = view.update(frames[SAMP], cam)
    theirs = torch.from_numpy(ref()).to(dev)
    res["overlay"] = {"update_ms": h, "torch_numpy_host_ms": r, "ratio": round(r / h, 2), "min_ms": [hmin, rmin],
                      "overlay_pixels": int((ours[..., 3] > 0).sum()),
                      "pixels_differing_from_host": int((ours != theirs).any(-1).sum()), "per_launch": per_launch_us(hip)}

    image = torch.rand(3, H // 2, W // 2, generator=g).to(dev)                # a half-size render shown at 1080p
    control = torch.zeros(H, W, 3)
    control[500:510, 900:910] = torch.tensor([1.0, 0.0, 0.0])
    tint = torch.rand(H, W, 3, generator=g)
    control_d, tint_d = control.to(dev), tint.to(dev)
    overlay_h = ours.cpu().numpy()
    for name, img in (("present_resize", image), ("present_same_size", torch.rand(3, H, W, generator=g).to(dev))):
        hip = lambda: trajectory.present_frame(img, size=(H, W), control_overlay=control_d, overlay=ours, tint=tint_d).cpu()   # noqa: E731
        dev_only = lambda: trajectory.present_frame(img, size=(H, W), control_overlay=control_d, overlay=ours, tint=tint_d)  # noqa: E731
        ref = lambda: host_finish(img, (H, W), control.numpy(), overlay_h, tint.numpy())                                      # noqa: E731
        (h, hmin), (d, dmin), (r, rmin) = alternate([hip, dev_only, ref], a.reps)
        gap = float(np.abs(hip().numpy() - ref()).max())
        res[name] = {"present_frame_and_copy_ms": h, "present_frame_on_device_ms": d, "torch_numpy_host_ms": r,
                     "ratio": round(r / h, 2), "min_ms": [hmin, dmin, rmin], "max_abs_difference_from_host": gap,
                     "per_launch": per_launch_us(dev_only)}
    depth = (torch.rand(1, H, W, generator=g) * 7 + 0.2).to(dev)
    hip = lambda: trajectory.present_frame(depth, depth=True)                 # noqa: E731

    def ref():
        b = depth.repeat(3, 1, 1)
        b = (b - b.min()) / (b.max() - b.min() + 1e-20)
        return b.permute(1, 2, 0).contiguous().clamp(0, 1)
    (h, hmin), (r, rmin) = alternate([hip, ref], a.reps)
    res["present_depth"] = {"present_frame_on_device_ms": h, "torch_on_device_ms": r, "ratio": round(r / h, 2), "min_ms": [hmin, rmin],
                            "max_abs_difference": float((hip() - ref()).abs().max()), "per_launch": per_launch_us(hip)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
