#!/usr/bin/env python
"""Secondary measurement: LPIPS with the VGG16 backbone (trase_amd.lpips, csrc/vgg.hip: bf16x3 convolutions, a float64 head)
against the same computation as torch.nn.functional conv2d / relu / max_pool2d plus the reference's head statements
(lpipsPyTorch/modules/{lpips,utils}.py) in fp32 on the same GPU, seeded weights.  The two sides take turns in one process, timed
with HIP events, medians of --reps runs after a pre-roll (torch's first calls, where MIOpen picks its kernels, are untimed).
Every part runs as a fresh child process under a time limit of its own; a child that fails ends the script at once, nothing
further is launched.

  (a) one pair at 1080 x 1920 and 960 x 1280: both times, the difference of the two results
  (b) per-layer times from the library's profiling scopes (both images of a layer in one scope), with each convolution's achieved
      bf16 TFLOP/s counting three products per multiply-add
  (c) torch.cuda.max_memory_allocated of one call on each side, and the workspace bytes
  (d) bench.py on this tree's library and on --parent-lib (the parent commit's build), taking turns twice in fresh processes (no
      rendering code differs: a control), in the order run
  tests: the shares of their bars that tests/test_gpu_lpips.py records

    python profiles/bench_lpips.py --parent-lib /path/to/parent/libtrase_rast.so > profiles/lpips_bench.json
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

SIZES = {"1080x1920": (1080, 1920), "960x1280": (960, 1280)}


def layer_flops(H, W):
    """multiply-adds x 2 of every layer's forward for ONE image of size (H, W)"""
    from trase_amd.lpips import CHANNELS, KEYS, POOL_AFTER
    out, h, w = {}, H, W
    for l in range(1, 14):
        out[KEYS[l - 1]] = 2 * 9 * CHANNELS[l - 1] * CHANNELS[l] * h * w
        if l in POOL_AFTER:
            h, w = h // 2, w // 2
    return out


def torch_lpips(pairs, lins):
    """the reference's computation with torch's own operators, fp32"""
    import torch
    import torch.nn.functional as F
    from trase_amd.lpips import MEAN, POOL_AFTER, STD, TAP_LAYERS
    dev = pairs[0][0].device
    mean, std = torch.tensor(MEAN, device=dev).view(1, 3, 1, 1), torch.tensor(STD, device=dev).view(1, 3, 1, 1)
    lin4 = [v.view(1, -1, 1, 1) for v in lins]

    def feats(x):
        a, out = (x[None] - mean) / std, []
        for l, (w, b) in enumerate(pairs, start=1):
            a = F.relu(F.conv2d(a, w, b, padding=1))
            if l in TAP_LAYERS:
                out.append(a / (torch.sqrt(torch.sum(a ** 2, dim=1, keepdim=True)) + 1e-10))
            if l in POOL_AFTER:
                a = F.max_pool2d(a, 2, 2)
        return out

    def fn(x, y):
        fx, fy = feats(x), feats(y)
        res = [F.conv2d((p - q) ** 2, l).mean((2, 3), True) for p, q, l in zip(fx, fy, lin4)]
        return torch.sum(torch.cat(res, 0), 0, True)
    return fn


def part_measure(size, reps):
    import torch
    from bench_vgg import alternate
    from trase_amd.lpips import KEYS, LPIPSVGG, TAP_NAMES, lpips_random_weights, sizes
    from trase_amd.rasterizer import profile_enable, profile_report
    dev = torch.device("cuda", 0)
    H, W = SIZES[size]
    pairs, lins = lpips_random_weights(20, device=dev)
    net = LPIPSVGG(pairs, lins)
    ref = torch_lpips(pairs, lins)
    g = torch.Generator().manual_seed(H)
    x = torch.rand(3, H, W, generator=g).to(dev)
    y = (x + 0.1 * torch.rand(3, H, W, generator=g).to(dev)).clamp(0, 1)

    def hip():
        net(x, y)

    def torch_side():
        with torch.no_grad():
            ref(x, y)
    t = alternate([hip, torch_side], reps)
    res = {"size": [H, W], "reps": reps, "pair": {"hip_bf16x3": t[0], "torch_fp32": t[1]}}
    with torch.no_grad():
        a, b = net(x, y), ref(x, y)
        again = net(x, y)
    res["results"] = {"hip_bf16x3": float(a), "torch_fp32": float(b), "difference": abs(float(a) - float(b)),
                      "second_call_same_bits": bool(torch.equal(a, again))}
    profile_enable(1)
    for _ in range(5):
        hip()
    torch.cuda.synchronize()
    scopes = profile_report()
    profile_enable(0)
    fl = layer_flops(H, W)
    layers = {}
    for key in KEYS:
        s = scopes.get(f"lpips_{key}")
        rec = {"gflop_both_images": round(2 * fl[key] / 1e9, 2)}
        if s:
            rec["ms_both_images"] = round(s["ms"], 4)
            if key != "conv1_1":                                        # conv1_1 is an fp32 VALU kernel
                rec["tflops_bf16_three_products"] = round(3 * 2 * fl[key] / (s["ms"] * 1e-3) / 1e12, 1)
        layers[key] = rec
    res["layers"] = layers
    res["heads"] = {n: round(scopes[f"lpips_head_{n}"]["ms"], 4) for n in TAP_NAMES if f"lpips_head_{n}" in scopes}
    res["other_scopes"] = {k: v for k, v in scopes.items() if k in ("lpips_mean", "lpips_pack")}
    mem = {}
    for name, fn in (("hip_bf16x3", hip), ("torch_fp32", torch_side)):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        mem[name] = int(torch.cuda.max_memory_allocated() - base)
    pack_b, ws_b, _ = sizes(H, W)
    mem["hip_workspace"], mem["hip_pack"] = ws_b, pack_b
    res["peak_bytes_of_a_call"] = mem
    res["device"] = torch.cuda.get_device_name(0)
    return res


def part_tests():
    with tempfile.NamedTemporaryFile("r", suffix=".jsonl") as f:
        env = dict(os.environ, TRASE_LPIPS_RECORD=f.name)
        out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_lpips.py"), "-q", "-m", "gpu",
                              "-p", "no:cacheprovider", "-k", "metric_within or fixture_pairs or head_alone"], env=env, cwd=ROOT,
                             capture_output=True, text=True, timeout=600)
        recs = [json.loads(ln) for ln in f.read().splitlines() if ln]
    if out.returncode != 0:
        sys.stderr.write(out.stdout[-3000:])
        sys.exit(f"[bench_lpips] the tests ended with status {out.returncode}: stopping")
    shares = {r["test"]: round(r["share_of_bar"], 4) for r in recs}
    return {"share_of_bar": shares, "largest": max(shares.values()) if shares else None, "summary": out.stdout.strip().splitlines()[-1]}


def child(args, limit):
    """run one part of this script as a fresh process under its own time limit; its last line is the part's JSON"""
    print("[bench_lpips]", " ".join(args), file=sys.stderr, flush=True)
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=limit)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    if out.returncode != 0 or not lines:
        sys.stderr.write(out.stderr[-3000:])
        sys.exit(f"[bench_lpips] part {args} ended with status {out.returncode}: stopping, nothing further is launched")
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--skip", default="", help="comma-separated parts to leave out: measure, bench, tests")
    ap.add_argument("--part", default=None)
    ap.add_argument("--size", default="1080x1920")
    a = ap.parse_args()
    if a.part == "measure":
        print(json.dumps(part_measure(a.size, a.reps)))
        return
    skip = set(a.skip.split(",")) if a.skip else set()
    res = {"unmeasured": sorted(skip)}
    if "measure" not in skip:
        for size in SIZES:
            res[size] = child(["--part", "measure", "--size", size, "--reps", str(a.reps)], 600)
    if "bench" not in skip:
        from bench_neighbors import bench_line
        runs = []
        for turn in range(2):
            print(f"[bench_lpips] bench.py, turn {turn}", file=sys.stderr, flush=True)
            runs.append({"tree": bench_line(None)})
            if a.parent_lib:
                runs[-1]["parent"] = bench_line(a.parent_lib)
        res["bench_in_the_order_run"] = runs
    if "tests" not in skip:
        res["tests"] = part_tests()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
