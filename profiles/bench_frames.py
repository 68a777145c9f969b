"""The GAUSSIAN-state loss head on an 8-bit ground-truth frame (trase_amd.frames.ByteFrame) against the fp32 tensor, at 1080p.

HIP events around every call, medians of 30 after a pre-roll; the sides of a comparison ALTERNATE inside one process (call by
call), so they see the same clocks and the same neighbours.  Records:

    head             photometric_loss forward + backward on the fp32 tensor (twice: "float" and "float_again", the spread of the
                     float head's own repeated medians), on the ByteFrame, on the ByteFrame with mask_black=True, and the
                     reference's four torch launches of train.py:231-234 followed by the float head
    frame            ByteFrame.from_array and ByteFrame.from_rgba from a host array (upload included) against the host statements
                     of train.py:221-230 (RGBA array -> float64 composite -> bytes -> / 255 -> clamp) plus the fp32 upload; host
                     clock around a synchronise, since most of that work is on the host
    black_mask       frame.black_mask((540, 960)) against upload of the fp32 frame + F.interpolate + sum == 0 (train.py:266-268),
                     and against the same without the upload
    resident_bytes   bytes a resident frame occupies as fp32 and as a ByteFrame

    python profiles/bench_frames.py [--out profiles/frames_bench.json] [--bench-this FILE --bench-parent FILE]

--bench-this / --bench-parent: files holding the JSON lines bench.py printed on this tree and on its parent commit (same machine,
runs taking turns); they are copied into the result as they are.  Prints the result as one JSON line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trase_amd.frames import ByteFrame  # noqa: E402
from trase_amd.losses import photometric_loss  # noqa: E402

REPS, PREROLL = 30, 5
H, W = 1080, 1920


def alternate(fns, reps=REPS, preroll=PREROLL, host=False):
    """median ms of each callable, the callables taking turns; HIP events, or (host=True) a host clock around a synchronise"""
    for _ in range(preroll):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            if host:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3)
            else:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                times[k].append(a.elapsed_time(b))
    return {k: round(statistics.median(v), 4) for k, v in times.items()}, {k: round(max(v) - min(v), 4) for k, v in times.items()}


def scene():
    g = np.random.default_rng(0)
    rgba = g.integers(0, 256, (H, W, 4), dtype=np.uint8)
    rgba[..., 3] = 255
    rgba[200:500, 300:900, 3] = g.integers(0, 256, (300, 600), dtype=np.uint8)      # a translucent region
    rgba[600:900, 1000:1700] = (0, 0, 0, 255)                                        # an opaque black one
    return rgba


def reference_host_frame(rgba, background):
    """the host statements of train.py:221-230 (without the file read and PIL's array round trip), then the upload"""
    norm = rgba / 255.0
    arr = norm[:, :, :3] * norm[:, :, 3:4] + background * (1 - norm[:, :, 3:4])
    as_bytes = np.array(arr * 255.0, dtype=np.byte).view(np.uint8)
    gt = (torch.from_numpy(as_bytes) / 255.0).permute(2, 0, 1)
    return gt.clamp(0.0, 1.0).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_bench.json"))
    ap.add_argument("--bench-this")
    ap.add_argument("--bench-parent")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frames.py measures on the GPU; there is none here")
    rgba = scene()
    rgb = np.ascontiguousarray(rgba[..., :3])
    background = np.zeros(3, dtype=np.float32)
    frame = ByteFrame.from_rgba(rgba, background, device="cuda")
    gt = frame.to_float()
    gt_host = gt.cpu()
    img = torch.rand(3, H, W, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)).requires_grad_(True)

    def head(target, **kw):
        def run():
            img.grad = None
            photometric_loss(img, target, 0.2, **kw).backward()
        return run

    def torch_mask_then_float_head():
        img.grad = None
        black_mask = torch.sum(gt, dim=0) == 0                      # train.py:232-234
        black_mask = black_mask.float()
        image = img * (1 - black_mask) + gt * black_mask
        photometric_loss(image, gt, 0.2).backward()

    res = {"size": [H, W], "reps": REPS, "preroll": PREROLL, "device": torch.cuda.get_device_name(0)}
    med, spread = alternate({"float": head(gt), "bytes": head(frame), "float_again": head(gt), "bytes_mask_black": head(frame, mask_black=True),
                             "torch_mask_then_float": torch_mask_then_float_head})
    res["head_fwd_bwd_ms"] = med
    res["head_fwd_bwd_spread_ms"] = spread
    res["float_head_median_spread_ms"] = round(abs(med["float"] - med["float_again"]), 4)
    res["bytes_minus_float_ms"] = round(med["bytes"] - min(med["float"], med["float_again"]), 4)

    # the results the timed calls produced, once more: bitwise equal
    img.grad = None
    a = photometric_loss(img, gt, 0.2)
    a.backward()
    ga = img.grad.clone()
    img.grad = None
    b = photometric_loss(img, frame, 0.2)
    b.backward()
    res["bytes_equal_float_bitwise"] = bool(torch.equal(a, b) and torch.equal(ga, img.grad))

    med, spread = alternate({"from_array_rgb": lambda: ByteFrame.from_array(rgb, device="cuda"),
                             "from_array_rgba": lambda: ByteFrame.from_array(rgba, device="cuda"),
                             "from_rgba": lambda: ByteFrame.from_rgba(rgba, background, device="cuda"),
                             "reference_host_composite_and_upload": lambda: reference_host_frame(rgba, background),
                             "fp32_upload_only": lambda: gt_host.cuda()}, host=True)
    res["frame_build_wall_ms"] = med
    res["frame_build_spread_ms"] = spread

    size = (540, 960)

    def torch_black(upload):
        def run():
            g = gt_host.cuda() if upload else gt
            r = torch.nn.functional.interpolate(g.unsqueeze(0), size, mode="bilinear").squeeze(0)
            return torch.sum(r, dim=0) == 0
        return run
    med, spread = alternate({"black_mask": lambda: frame.black_mask(size), "upload_interpolate_sum": torch_black(True),
                             "interpolate_sum_resident": torch_black(False), "black_mask_full_size": lambda: frame.black_mask()})
    res["black_mask_540x960_ms"] = med
    res["black_mask_540x960_spread_ms"] = spread
    res["black_mask_equal"] = bool(torch.equal(frame.black_mask(size), torch_black(False)()))

    res["resident_bytes_per_frame"] = {"fp32": gt.numel() * 4, "byteframe": frame.nbytes}
    for key, path in (("bench_this", args.bench_this), ("bench_parent", args.bench_parent)):
        if path:
            lines = [ln for ln in open(path).read().splitlines() if ln.startswith("{")]
            res[key] = [json.loads(ln) for ln in lines]
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
