#!/usr/bin/env python
"""Secondary measurement: the VGG16 feature extractor of the style-transfer loop (trase_amd.vgg, csrc/vgg.hip: bf16x3 on the
matrix cores) against the same stack as torch.nn.functional conv2d / relu / max_pool2d in fp32 on the same GPU.  The two
sides take turns in one process, timed with HIP events, medians of --reps runs after a pre-roll (torch's first calls, where
MIOpen picks its kernels, are untimed).  Every part runs as a fresh child process under a time limit of its own; a child that
fails ends the script at once, nothing further is launched.

  (a) forward alone and forward + backward for conv4_1 at 1080 x 1920 and 960 x 1280
  (b) per-layer kernel times from the library's profiling scopes against each layer's FLOP count: achieved bf16 TFLOP/s,
      counting three products per multiply-add
  (c) torch.cuda.max_memory_allocated of one forward + backward on each side
  (d) the style iteration of tests/test_gpu_nnfm.py::test_style_transfer_iteration_config5_size at the S4 size (300 000
      Gaussians, 1920 x 1080) with either extractor
  (e) bench.py on this tree's library and on --parent-lib (the parent commit's build), taking turns twice (no rendering code
      differs: a control)
  tests: the shares of their bars that tests/test_gpu_vgg.py records

    python profiles/bench_vgg.py --parent-lib /path/to/parent/libtrase_rast.so > profiles/vgg_bench.json
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CHANNELS = (3, 64, 64, 128, 128, 256, 256, 256, 512)
POOL_AFTER = (2, 4, 7)
KEYS = ("conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3", "conv4_1")
SIZES = {"1080x1920": (1080, 1920), "960x1280": (960, 1280)}


def layer_flops(H, W):
    """multiply-adds x 2 of every layer's forward at image size (H, W)"""
    out, h, w = {}, H, W
    for l in range(1, 9):
        out[KEYS[l - 1]] = 2 * 9 * CHANNELS[l - 1] * CHANNELS[l] * h * w
        if l in POOL_AFTER:
            h, w = h // 2, w // 2
    return out


def torch_stack(pairs):
    import torch.nn.functional as F

    def fn(x):
        a = x[None]
        for l, (w, b) in enumerate(pairs, start=1):
            a = F.conv2d(a, w, b, padding=1)
            if l < len(pairs):
                a = F.relu(a)
                if l in POOL_AFTER:
                    a = F.max_pool2d(a, 2, 2)
        return a
    return fn


def alternate(fns, reps, warmup=3):
    """median and minimum HIP-event time in ms of every fn, the fns taking turns"""
    import torch

    def once(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)
    for _ in range(warmup):
        for fn in fns:
            once(fn)
    times = [[] for _ in fns]
    for _ in range(reps):
        for fn, out in zip(fns, times):
            out.append(once(fn))
    return [{"median_ms": round(sorted(t)[len(t) // 2], 4), "min_ms": round(min(t), 4)} for t in times]


def part_measure(size, reps):
    """(a), (b), (c) at one size"""
    import torch
    from trase_amd.rasterizer import profile_enable, profile_report
    from trase_amd.vgg import MEAN, STD, VGG16Features, sizes, vgg16_random_weights
    dev = torch.device("cuda", 0)
    H, W = SIZES[size]
    pairs = vgg16_random_weights(1, "conv4_1", device=dev)
    net = VGG16Features(pairs, "conv4_1")
    stack = torch_stack(pairs)
    mean, std = torch.tensor(MEAN, device=dev).view(3, 1, 1), torch.tensor(STD, device=dev).view(3, 1, 1)
    img = torch.rand(3, H, W, device=dev)
    x = img.clone().requires_grad_(True)
    cot = torch.randn(1, 512, H // 8, W // 8, device=dev)

    def hip_fwd():
        with torch.no_grad():
            net(img)

    def torch_fwd():
        with torch.no_grad():
            stack((img - mean) / std)

    def hip_both():
        x.grad = None
        net(x).backward(cot)

    def torch_both():
        x.grad = None
        stack((x - mean) / std).backward(cot)
    t = alternate([hip_fwd, torch_fwd, hip_both, torch_both], reps)
    res = {"size": [H, W], "reps": reps, "forward": {"hip_bf16x3": t[0], "torch_fp32": t[1]},
           "forward_backward": {"hip_bf16x3": t[2], "torch_fp32": t[3]}}
    with torch.no_grad():
        a, b = net(img), stack((img - mean) / std)
    res["largest_difference_of_the_sides"] = {"abs": float((a - b).abs().max()), "largest_value": float(b.abs().max())}
    # (b) the kernels' own times
    profile_enable(1)
    for _ in range(5):
        hip_both()
    torch.cuda.synchronize()
    scopes = profile_report()
    profile_enable(0)
    fl = layer_flops(H, W)
    layers = {}
    for key in KEYS:
        rec = {"gflop": round(fl[key] / 1e9, 2)}
        for side in ("fwd", "bwd"):
            s = scopes.get(f"vgg_{side}_{key}")
            if s:
                rec[f"{side}_ms"] = round(s["ms"], 4)
                if key != "conv1_1":                                   # conv1_1 and its image gradient are fp32 VALU kernels
                    rec[f"{side}_tflops_bf16_three_products"] = round(3 * fl[key] / (s["ms"] * 1e-3) / 1e12, 1)
        layers[key] = rec
    res["layers"] = layers
    res["other_scopes"] = {k: v for k, v in scopes.items() if k.startswith("vgg_") and k[8:] not in KEYS}
    # (c) memory of one forward + backward
    mem = {}
    for name, fn in (("hip_bf16x3", hip_both), ("torch_fp32", torch_both)):
        x.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        mem[name] = int(torch.cuda.max_memory_allocated() - base)
    _, wsf, wsb, saved, _, _, _ = sizes(8, H, W)
    mem["hip_workspace_forward"], mem["hip_workspace_backward"], mem["hip_saved_bits"] = wsf, wsb, saved
    res["peak_bytes_of_forward_backward"] = mem
    res["device"] = torch.cuda.get_device_name(0)
    return res


def part_iteration(reps):
    """(d): render -> extractor -> loss_nnfm_style -> backward -> FusedAdam on the colours, at the S4 size"""
    import torch
    from gaussian_renderer import render
    from trase_amd.losses import loss_nnfm_style
    from trase_amd.optim import FusedAdam
    from trase_amd.synthetic import SynthGaussianModel, SynthPipe, make_scene, orbit_camera
    from trase_amd.vgg import MEAN, STD, VGG16Features, vgg16_random_weights
    dev = torch.device("cuda", 0)
    n, w, h = 300_000, 1920, 1080
    pc = SynthGaussianModel(make_scene(n, feat_dim=32, seed=5).to(dev))
    cam = orbit_camera(w, h, angle=1.1).to(dev)
    bg = torch.zeros(3, device=dev)
    pairs = vgg16_random_weights(1, "conv4_1", device=dev)
    net = VGG16Features(pairs, "conv4_1")
    stack = torch_stack(pairs)
    mean, std = torch.tensor(MEAN, device=dev).view(3, 1, 1), torch.tensor(STD, device=dev).view(3, 1, 1)
    with torch.no_grad():
        style = net(torch.rand(3, h, w, device=dev))[0].reshape(512, -1)
    opt = FusedAdam([{"params": [pc._features_dc], "lr": 0.0025, "name": "f_dc"},
                     {"params": [pc._features_rest], "lr": 0.0025 / 20.0, "name": "f_rest"}], lr=0.0, eps=1e-15)

    def step(extract):
        def fn():
            image = render(cam, pc, SynthPipe(), bg, 0.0, 0.0, 0.0)["render"]
            loss_nnfm_style(extract(image).reshape(512, -1), style).backward()
            opt.step()
            for p in pc.parameters():
                p.grad = None
        return fn
    t = alternate([step(lambda im: net(im)[0]), step(lambda im: stack((im - mean) / std)[0])], reps)
    return {"gaussians": n, "size": [h, w], "reps": reps, "iteration": {"hip_bf16x3": t[0], "torch_fp32": t[1]}}


def part_tests():
    with tempfile.NamedTemporaryFile("r", suffix=".jsonl") as f:
        env = dict(os.environ, TRASE_VGG_RECORD=f.name)
        out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_vgg.py"), "-q", "-m", "gpu",
                              "-p", "no:cacheprovider", "-k", "forward_within or backward_under"], env=env, cwd=ROOT,
                             capture_output=True, text=True, timeout=600)
        recs = [json.loads(ln) for ln in f.read().splitlines() if ln]
    if out.returncode != 0:
        sys.stderr.write(out.stdout[-3000:])
        sys.exit(f"[bench_vgg] the tests ended with status {out.returncode}: stopping")
    res = {}
    for kind in ("forward", "backward"):
        shares = {r["test"]: round(r["share_of_bar"], 4) for r in recs if r["test"].startswith(kind)}
        res[kind] = {"share_of_bar": shares, "largest": max(shares.values()) if shares else None}
    res["summary"] = out.stdout.strip().splitlines()[-1]
    return res


def child(args, limit):
    """run one part of this script as a fresh process under its own time limit; its last line is the part's JSON"""
    print("[bench_vgg]", " ".join(args), file=sys.stderr, flush=True)
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=limit)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    if out.returncode != 0 or not lines:
        sys.stderr.write(out.stderr[-3000:])
        sys.exit(f"[bench_vgg] part {args} ended with status {out.returncode}: stopping, nothing further is launched")
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--skip", default="", help="comma-separated parts to leave out: measure, iteration, bench, tests")
    ap.add_argument("--part", default=None)
    ap.add_argument("--size", default="1080x1920")
    a = ap.parse_args()
    if a.part == "measure":
        print(json.dumps(part_measure(a.size, a.reps)))
        return
    if a.part == "iteration":
        print(json.dumps(part_iteration(a.reps)))
        return
    skip = set(a.skip.split(",")) if a.skip else set()
    res = {"unmeasured": sorted(skip)}
    reps = ["--reps", str(a.reps)]
    if "measure" not in skip:
        for size in SIZES:
            res[size] = child(["--part", "measure", "--size", size] + reps, 600)
    if "iteration" not in skip:
        res["style_iteration_S4"] = child(["--part", "iteration"] + reps, 600)
    if "bench" not in skip:
        from bench_neighbors import bench_line
        runs = []
        for turn in range(2):
            print(f"[bench_vgg] bench.py, turn {turn}", file=sys.stderr, flush=True)
            runs.append({"tree": bench_line(None)})
            if a.parent_lib:
                runs[-1]["parent"] = bench_line(a.parent_lib)
        res["bench"] = runs
    if "tests" not in skip:
        res["tests"] = part_tests()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
