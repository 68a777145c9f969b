#!/usr/bin/env python
"""Secondary measurement: the segment output of one frame at S4 size -- N = 300k Gaussians, 1080p, 10 % of the rows selected --
``trase_amd.evaluate.render_segment`` (one fused forward + one launch) against the statements of render.py:344-360 composed
around this repository's ``render()`` (two forwards, about eight torch launches, two host copies with numpy's to8b), both on
the same GPU in the same process, alternating, timed with HIP events after a pre-roll:

  frames        render_segment(frames_u8=True) + one .cpu() of each 8-bit frame     vs the composition as written
  device_only   render_segment() with nothing read back                             vs the composition without to8b
  scored        render_segment(frames_u8=True, scores=, gt_mask=, gt_object=) -- the same pass also fills the frame's record
                and the SSIM launches run; FrameScores.result() is outside the timed region (one read-back per sequence)

    python profiles/bench_evaluate.py > profiles/evaluate_bench.json
    python profiles/bench_evaluate.py --reps 50

Medians (and minima) in milliseconds.  "kernel" is the library's profiling scope around the evaluate launch, with the bytes
that launch has to move and the bandwidth that gives."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trase_amd import _lib  # noqa: E402
from trase_amd.evaluate import FrameScores, render_segment  # noqa: E402
from trase_amd.renderer import render  # noqa: E402
from trase_amd.synthetic import SynthGaussianModel, SynthPipe, make_scene, orbit_camera  # noqa: E402

N, W, H = 300_000, 1920, 1080
to8b = lambda x: (255 * np.clip(x.cpu().numpy(), 0, 1)).astype(np.uint8)          # noqa: E731  (render.py:106)


def composition(cam, pc, pipe, bg, sel, ones, frames=True):
    """render.py:344-360 (black background for the mask pass, the scene's for the object pass)."""
    black = torch.tensor([0, 0, 0], dtype=torch.float32, device="cuda")
    buffer_image = render(cam, pc, pipe, black, 0.0, 0.0, 0.0, False, mask=sel, override_color=ones)["render"]
    buffer_image[buffer_image < 0.5] = 0
    buffer_image[buffer_image != 0] = 1
    inlier_mask = buffer_image.mean(axis=0).bool()
    m8 = to8b(buffer_image).transpose(1, 2, 0) if frames else None
    buffer_image = render(cam, pc, pipe, bg, 0.0, 0.0, 0.0, False, mask=sel)["render"]
    buffer_image[:, ~inlier_mask] = 0
    o8 = to8b(buffer_image).transpose(1, 2, 0) if frames else None
    return inlier_mask, buffer_image, m8, o8


def alternate(fns, reps, warmup=5):
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


def per_launch(fn, reps=10):
    lib = _lib.load()
    buf = ctypes.create_string_buffer(65536)
    fn()
    torch.cuda.synchronize()
    lib.trase_prof_enable(1)
    for _ in range(reps):
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
    pc = SynthGaussianModel(make_scene(N, feat_dim=32, seed=3).to(dev), requires_grad=False)
    pipe = SynthPipe()
    bg = torch.tensor([0.0, 0.0, 0.0], device=dev)
    g = torch.Generator().manual_seed(23)
    sel = (torch.rand(N, generator=g) < 0.10).to(dev)
    ones = torch.ones(N, 3, device=dev)
    res = {"n": N, "selected": int(sel.sum()), "image": [W, H], "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        first = render_segment(cam, pc, pipe, bg, 0.0, 0.0, 0.0, mask=sel, frames_u8=True)
        inlier, cut, m8, o8 = composition(cam, pc, pipe, bg, sel, ones)
        res["mask_fraction"] = round(float(first["pred_mask"].float().mean()), 4)
        res["mask_pixels_differing_from_composition"] = int((first["pred_mask"] != inlier).sum())
        res["object_u8_bytes_differing_from_composition"] = int((first["object_u8"].cpu().numpy() != o8).sum())
        gt_mask = torch.roll(first["pred_mask"], (7, -9), (0, 1)).contiguous()
        gt_object = first["object_u8"].clone()
        scores = FrameScores(1, device=dev)

        def seg_frames():
            o = render_segment(cam, pc, pipe, bg, 0.0, 0.0, 0.0, mask=sel, frames_u8=True)
            return o["object_u8"].cpu(), o["pred_mask_u8"].cpu()

        def seg_scored():
            scores.reset()
            return render_segment(cam, pc, pipe, bg, 0.0, 0.0, 0.0, mask=sel, frames_u8=True, scores=scores, frame=0,
                                  gt_mask=gt_mask, gt_object=gt_object)

        seg_device = lambda: render_segment(cam, pc, pipe, bg, 0.0, 0.0, 0.0, mask=sel)                 # noqa: E731
        one_render = lambda: render(cam, pc, pipe, bg, 0.0, 0.0, 0.0, False, mask=sel)                  # noqa: E731
        ref_frames = lambda: composition(cam, pc, pipe, bg, sel, ones)                                   # noqa: E731
        ref_device = lambda: composition(cam, pc, pipe, bg, sel, ones, frames=False)                     # noqa: E731
        names = ["render_segment_frames", "composition_frames", "render_segment_device_only", "composition_device_only",
                 "render_segment_scored", "one_render_mask"]
        t = alternate([seg_frames, ref_frames, seg_device, ref_device, seg_scored, one_render], a.reps)
        res["ms"] = {k: {"median": v[0], "min": v[1]} for k, v in zip(names, t)}
        res["ratio_frames"] = round(t[1][0] / t[0][0], 2)
        res["ratio_device_only"] = round(t[3][0] / t[2][0], 2)
        px = W * H
        for tag, fn, per_px in (("kernel_frames_u8", lambda: render_segment(cam, pc, pipe, bg, 0.0, 0.0, 0.0, mask=sel, frames_u8=True),
                                 16 + 16 + 1 + 6),                      # 3 planes + T in; 3 planes + alpha, mask bytes, two HWC frames out
                                ("kernel_scored", seg_scored, 16 + 16 + 1 + 6 + 1 + 3 + 24)):   # + gt mask, gt bytes in, the compared pair out
            prof = per_launch(fn)
            ms = prof["evaluate"]["ms"]
            res[tag] = {"ms": round(ms, 5), "bytes": per_px * px, "GBps": round(per_px * px / ms / 1e6, 1),
                        "render_fwd_ms": round(prof.get("render_fwd", {}).get("ms", float("nan")), 5)}
        res["scores_of_the_scored_frame"] = {k: v for k, v in scores.result().items() if not isinstance(v, list)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
