#!/usr/bin/env python
"""Secondary measurement: the FEATURE-state loss head when the SAM masks are smaller than the render (--downsample_mask 2 and 4)
-- a 1080p render, F = 32, 100 masks at 540 x 960 and at 270 x 480, S ~ 5000 sampled pixels, 50 sampled masks, soft mode.

  resized       contrastive_head(full-resolution features, ..., with_norm_reg=True): four bilinear taps per sampled pixel, one
                dense gradient pass (taps + regulariser), forward + backward
  composition   what it replaces: feature_norm_reg(features) + F.interpolate(features, mask size, mode="bilinear") +
                contrastive_head(resized map, ...), forward + backward (torch's upsample backward adds with float atomics)

both on the same GPU in the same process, alternating, timed with HIP events after a pre-roll; medians (and minima) in
milliseconds.  "backward" holds the library's profiling scopes of the new backward: the pair passes (S x S, then per sample), and
the dense pass with the bytes it has to move -- the (32, H, W) gradient written once, the features read once for the regulariser
-- and the bandwidth that gives.

    python profiles/bench_feature_resized.py > profiles/feature_resized_bench.json
"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trase_amd import _lib  # noqa: E402
from trase_amd.feature_head import (check_sampled_counts, contrastive_head, feature_norm_reg, get_sample_pixel_and_mask,  # noqa: E402
                                    mask_stats)

H, W, F, N, S, NM = 1080, 1920, 32, 100, 5000, 50


def scene(h, w, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing="ij")
    cy, cx = torch.randint(0, h, (N,), device=dev, generator=g), torch.randint(0, w, (N,), device=dev, generator=g)
    ry, rx = torch.randint(h // 30, h // 3, (N,), device=dev, generator=g), torch.randint(w // 30, w // 4, (N,), device=dev, generator=g)
    sam = ((yy[None] - cy[:, None, None]).abs() <= ry[:, None, None]) & ((xx[None] - cx[:, None, None]).abs() <= rx[:, None, None])
    base = torch.randn(N, F, device=dev, generator=g)
    big = torch.nn.functional.interpolate(sam.float()[None], size=(H, W), mode="nearest")[0]
    feat = (big.permute(1, 2, 0) @ base).permute(2, 0, 1) * 0.5 + 0.8 * torch.randn(F, H, W, device=dev, generator=g)
    return sam, feat


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
    res = {"render": [H, W], "features": F, "masks": N, "target_samples": S, "sampled_masks": NM, "mode": "soft", "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "cases": {}}
    for h, w in ((540, 960), (270, 480)):
        sam, feat = scene(h, w, dev, seed=h)
        cover, size = mask_stats(sam)
        torch.manual_seed(h)
        sp, sm = get_sample_pixel_and_mask(sam, S, NM, cover_count=cover, rng="cuda")
        f1, f2 = feat.clone().requires_grad_(True), feat.clone().requires_grad_(True)

        def resized():
            lp, ln, _, _, reg = contrastive_head(f1, sam, sp, sm, "soft", 0.75, 0.5, mask_size=size, with_norm_reg=True)
            return torch.autograd.grad(lp + ln + 0.1 * reg, f1)[0], lp.detach(), ln.detach(), reg.detach()

        def composition():
            reg = feature_norm_reg(f2)
            small = torch.nn.functional.interpolate(f2.unsqueeze(0), (h, w), mode="bilinear").squeeze(0)
            lp, ln, _, _ = contrastive_head(small, sam, sp, sm, "soft", 0.75, 0.5, mask_size=size)
            return torch.autograd.grad(lp + ln + 0.1 * reg, f2)[0], lp.detach(), ln.detach(), reg.detach()

        ga, gb = resized(), composition()
        case = {"masks_hw": [h, w], "samples": int(sp.sum()),
                "max_gradient_difference": float((ga[0] - gb[0]).abs().max()), "gradient_max": float(gb[0].abs().max()),
                "loss_difference": [abs(float(x) - float(y)) for x, y in zip(ga[1:], gb[1:])]}
        del ga, gb
        t = alternate([resized, composition], a.reps)
        case["ms"] = {"resized": {"median": t[0][0], "min": t[0][1]}, "composition": {"median": t[1][0], "min": t[1][1]}}
        case["ratio"] = round(t[1][0] / t[0][0], 2)
        prof = per_launch(resized)
        ms = prof["pairhead_spread"]["ms"]
        nbytes = 2 * 4 * F * H * W                           # the gradient written once + the features read once (regulariser)
        case["backward"] = {"dense_pass_ms": round(ms, 5), "dense_pass_bytes": nbytes, "dense_pass_GBps": round(nbytes / ms / 1e6, 1),
                            "pair_passes_ms": round(prof["pairhead_bwd_resized"]["ms"], 5),
                            "forward_ms": round(prof["pairhead_fwd_resized"]["ms"], 5),
                            "featnorm_fwd_ms": round(prof.get("featnorm_fwd", {}).get("ms", float("nan")), 5)}
        res["cases"][f"{h}x{w}"] = case
        check_sampled_counts()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
