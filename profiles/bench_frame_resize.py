"""ByteFrame at the camera's resolution (trase_amd.frames: ``resolution=``): Pillow's bicubic resize as one launch, measured.

The method of bench_frames.py: HIP events around every call, medians of 30 after a pre-roll; the sides of a comparison ALTERNATE
inside one process (call by call); builders that upload are timed with a host clock around a synchronise.  Cases:

    2028 x 2704 RGBA -> 1200 x 1600     the multi-view video sets at the default --resolution -1, composited over the background
    1080 x 1920 RGB  ->  540 x  960     -r 2 of a 1080p source

Recorded per case:

    launch_ms            the resize launch alone from a resident source ("resize", and "resize_again": the spread of its own
                         repeated medians), beside frame_pack_kernel at the source size ("pack_source_size": what the parent
                         commit can do with the same bytes) and at the frame's size ("pack_frame_size")
    bytes_moved          what the launch must move -- the source once, the planes once -- and the bandwidth the median implies
    build_wall_ms        from_rgba / from_array with resolution= from a host array (upload included); the same at the source size
                         (today's route followed by nothing: the lower bound of the upload); where PIL imports, the host statements
                         of train.py:221-230 with Pillow's resize, and Pillow's resize alone
    equal_numpy          where tests/resize_reference.py imports: the frame against the numpy restatement, byte for byte

    python profiles/bench_frame_resize.py [--out profiles/frame_resize_bench.json] [--bench-this FILE --bench-parent FILE]

--bench-this / --bench-parent: files holding the JSON lines bench.py printed on this tree and on its parent commit (same machine,
runs taking turns); they are copied into the result as they are.  Prints the result as one JSON line and writes it to --out.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_frames import PREROLL, REPS, alternate  # noqa: E402
from trase_amd.frames import ByteFrame  # noqa: E402

CASES = [("2028x2704_rgba_to_1200x1600", (2028, 2704), 4, (1200, 1600)), ("1080x1920_rgb_to_540x960", (1080, 1920), 3, (540, 960))]


def source(size, channels):
    g = np.random.default_rng(size[0])
    hwc = g.integers(0, 256, size + (channels,), dtype=np.uint8)
    if channels == 4:
        hwc[..., 3] = 255
        hwc[200:500, 300:900, 3] = g.integers(0, 256, (300, 600), dtype=np.uint8)          # a translucent region
    return hwc


def reference_host_frame(Image, rgba, background, resolution):
    """the host statements of train.py:221-230 (without the file read), Pillow's resize included, then the upload"""
    norm = rgba / 255.0
    arr = norm[:, :, :3] * norm[:, :, 3:4] + background * (1 - norm[:, :, 3:4])
    image = Image.fromarray(np.array(arr * 255.0, dtype=np.byte).view(np.uint8), "RGB")
    gt = (torch.from_numpy(np.array(image.resize(resolution))) / 255.0).permute(2, 0, 1)
    return gt.clamp(0.0, 1.0).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_resize_bench.json"))
    ap.add_argument("--bench-this")
    ap.add_argument("--bench-parent")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frame_resize.py measures on the GPU; there is none here")
    try:
        from PIL import Image
    except ImportError:
        Image = None
    try:
        from tests import frames_reference as fr
        from tests import resize_reference as rr
    except ImportError:
        fr = rr = None
    background = np.array([0.2, 0.5, 0.7], dtype=np.float32)
    res = {"reps": REPS, "preroll": PREROLL, "device": torch.cuda.get_device_name(0), "pil": Image is not None, "cases": {}}
    for name, (sH, sW), ch, (H, W) in CASES:
        hwc = source((sH, sW), ch)
        resolution = (W, H)
        dev_src = torch.from_numpy(hwc).cuda()
        dev_small = dev_src[:H, :W].contiguous()
        if ch == 4:
            def build(src, **kw):
                return ByteFrame.from_rgba(src, background, device="cuda", **kw)
        else:
            def build(src, **kw):
                return ByteFrame.from_array(src, device="cuda", **kw)
        case = {"source": [sH, sW, ch], "frame": [H, W]}
        med, spread = alternate({"resize": lambda: build(dev_src, resolution=resolution), "pack_source_size": lambda: build(dev_src),
                                 "resize_again": lambda: build(dev_src, resolution=resolution), "pack_frame_size": lambda: build(dev_small)})
        case["launch_ms"], case["launch_spread_ms"] = med, spread
        moved = hwc.size + 3 * H * ByteFrame.pitch_for(W)
        best = min(med["resize"], med["resize_again"])
        case["bytes_moved"] = {"source": hwc.size, "planes": 3 * H * ByteFrame.pitch_for(W), "implied_GBps": round(moved / best / 1e6, 1)}
        case["resize_over_pack_source_size"] = round(best / med["pack_source_size"], 3)
        fns = {"build_resized": lambda: build(hwc, resolution=resolution), "build_source_size": lambda: build(hwc)}
        if Image is not None:
            rgb = np.ascontiguousarray(hwc[..., :3])
            if ch == 4:
                fns["reference_host_statements"] = lambda: reference_host_frame(Image, hwc, background, resolution)
            pil_image = Image.fromarray(rgb, "RGB")
            fns["pillow_resize_alone"] = lambda: pil_image.resize(resolution)
        med, spread = alternate(fns, host=True)
        case["build_wall_ms"], case["build_wall_spread_ms"] = med, spread
        if rr is not None:
            rgb = fr.composite(hwc, background) if ch == 4 else hwc
            want = torch.from_numpy(fr.planes(rr.resize(rgb, resolution))).cuda()
            case["equal_numpy"] = bool(torch.equal(build(hwc, resolution=resolution).data, want))
        res["cases"][name] = case
    for key, path in (("bench_this", args.bench_this), ("bench_parent", args.bench_parent)):
        if path:
            lines = [ln for ln in open(path).read().splitlines() if ln.startswith("{")]
            res[key] = [json.loads(ln) for ln in lines]
    print(json.dumps(res))
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
