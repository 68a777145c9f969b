"""render_layers against the render() calls it replaces: 300k Gaussians, 1080p, F = 32, forward only.

HIP events around every call, medians of 30 after a pre-roll; the sides of a comparison ALTERNATE inside one process (call by
call), so they see the same clocks and the same neighbours.  Records, for L = 1, 2 and 10 colour tables and under both
capacity policies ("sync": the pair count is read back per forward, the library default; "free": capacity known beforehand):

    one_pass_ms      render_layers(colors=tables[:L])
    calls_ms         render() + L x render(override_color=table) under torch.no_grad() -- render.py:197, :240, :296
    calls_again_ms   the same side once more: the spread of a side's own repeated medians
    frames_u8        both sides with the 8-bit frames: render_layers(frames_u8=True) against the calls followed by the host's
                     to8b of render.py:106 on every image (device -> host copy + numpy), host clock around a synchronise
    pack / finish    the two launches on their own, with the bytes each must move (pack: 12 L + 128 per Gaussian; finish:
                     4 + 24 L per pixel, with the byte frames 12 + 3 (1 + L) more) and the bandwidth that gives
    equal            the layers of the timed calls are bitwise those of render(override_color=)

    python profiles/bench_layers.py [--out profiles/layers_bench.json] [--bench-this FILE --bench-parent FILE]

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
from trase_amd import rasterizer as R  # noqa: E402
from trase_amd.layers import finish_planes, pack_tables, render_layers  # noqa: E402
from trase_amd.renderer import render  # noqa: E402
from trase_amd.synthetic import SynthGaussianModel, SynthPipe, make_scene, orbit_camera  # noqa: E402

REPS, PREROLL = 30, 5
N, W, H, F = 300_000, 1920, 1080, 32
LS = (1, 2, 10)
to8b = lambda x: (255 * np.clip(x.cpu().numpy(), 0, 1)).astype(np.uint8)          # noqa: E731  (render.py:106)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layers_bench.json"))
    ap.add_argument("--bench-this")
    ap.add_argument("--bench-parent")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_layers.py measures on the GPU; there is none here")
    dev = torch.device("cuda", 0)
    pc = SynthGaussianModel(make_scene(N, feat_dim=F, seed=3).to(dev), requires_grad=False)
    cam = orbit_camera(W, H, angle=0.3, radius=4.0).to(dev)
    pipe, bg = SynthPipe(), torch.tensor([0.2, 0.5, 0.7], device=dev)
    g = torch.Generator().manual_seed(4)
    tables = [torch.rand(N, 3, generator=g).to(dev) for _ in range(max(LS))]

    def one_pass(L, u8=False):
        return lambda: render_layers(cam, pc, pipe, bg, 0.0, 0.0, 0.0, colors=tables[:L], frames_u8=u8)

    def calls(L, u8=False):
        def run():
            with torch.no_grad():
                imgs = [render(cam, pc, pipe, bg, 0.0, 0.0, 0.0)["render"]]
                imgs += [render(cam, pc, pipe, bg, 0.0, 0.0, 0.0, override_color=t)["render"] for t in tables[:L]]
                return [to8b(x).transpose(1, 2, 0) for x in imgs] if u8 else imgs
        return run

    res = {"workload": f"{N} Gaussians, {W}x{H}, F={F}, forward only", "reps": REPS, "preroll": PREROLL,
           "device": torch.cuda.get_device_name(0), "policies": {}}
    R.set_sync(True)
    out = one_pass(max(LS))()
    ref = calls(max(LS))()
    res["equal"] = bool(torch.equal(out["render"], ref[0]) and all(torch.equal(a, b) for a, b in zip(out["layers"], ref[1:])))
    capacity = int(R.last_status()[2] * 1.25) + 1024
    for policy in ("sync", "free"):
        R.set_sync(policy == "sync", capacity=0 if policy == "sync" else capacity)
        rec = {}
        for L in LS:
            med, spread = alternate({"one_pass": one_pass(L), "calls": calls(L), "calls_again": calls(L)})
            u8m, _ = alternate({"one_pass": one_pass(L, True), "calls": calls(L, True)}, reps=10, preroll=2, host=True)
            rec[f"L={L}"] = {"one_pass_ms": med["one_pass"], "calls_ms": med["calls"], "calls_again_ms": med["calls_again"],
                             "spread_ms": spread, "saved_ms": round(min(med["calls"], med["calls_again"]) - med["one_pass"], 4),
                             "speedup": round(min(med["calls"], med["calls_again"]) / med["one_pass"], 3),
                             "frames_u8_wall_ms": u8m}
        res["policies"][policy] = rec
    R.set_sync(True)

    # the two launches on their own
    hold = {}
    with torch.no_grad():
        planes = render(cam, pc, pipe, bg, 0.0, 0.0, 0.0, norm_gaussian_features=False, _keep_img=hold)
    image, planes = planes["render"], planes["render_gaussian_features"]
    block = torch.empty(N, 32, device=dev)
    res["launches"] = {}
    for L in LS:
        med, _ = alternate({"pack": lambda: pack_tables(tables[:L], out=block),
                            "finish": lambda: finish_planes(planes, hold["img"], bg, L),
                            "finish_u8": lambda: finish_planes(planes, hold["img"], bg, L, image=image, frames_u8=True)})
        pack_b, fin_b = (12 * L + 128) * N, (4 + 24 * L) * W * H
        fin8_b = fin_b + (12 + 3 * (1 + L)) * W * H
        res["launches"][f"L={L}"] = {
            "pack_ms": med["pack"], "pack_bytes": pack_b, "pack_GBps": round(pack_b / med["pack"] / 1e6, 1),
            "finish_ms": med["finish"], "finish_bytes": fin_b, "finish_GBps": round(fin_b / med["finish"] / 1e6, 1),
            "finish_u8_ms": med["finish_u8"], "finish_u8_bytes": fin8_b, "finish_u8_GBps": round(fin8_b / med["finish_u8"] / 1e6, 1)}
    res["launches"]["note"] = ("event time around one call: launch overhead and (finish_u8) the allocation of the byte frames "
                               "included; the bandwidth is the bytes over that time")
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
