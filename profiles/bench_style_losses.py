#!/usr/bin/env python
"""Secondary measurement: the image-space losses and the style-statistics node (trase_amd.losses, csrc/style.hip) against the
reference's torch statements (utils/loss_utils.py:33-44, :230-272) in fp32 on the same GPU.  The method of bench_vgg.py: the two
sides take turns in one process, timed with HIP events, medians of --reps runs after a pre-roll.  Every part runs as a fresh
child process under a time limit of its own; a child that fails ends the script at once, nothing further is launched.

  (a) style_statistics_loss forward + backward with all three terms, and with the Gram term alone, on (1, 512, 135, 240) and
      (1, 64, 960, 1280) features, against the same computation as the reference's statements under autograd
  (b) masked_l1_loss, weighted_l1_loss, l2_loss forward + backward at 1080 x 1920 against their torch statements
  (c) the two MFMA kernels' own times from the library's profiling scopes: achieved fp32 TFLOP/s against the 157 TFLOP/s peak
      (the Gram kernel counts the blocks on and above the diagonal only: the work it does)
  (d) bench.py on this tree's library and on --parent-lib (the parent commit's build), taking turns twice (no rendering code
      differs: a control)

    python profiles/bench_style_losses.py --parent-lib /path/to/parent/libtrase_rast.so > profiles/style_losses_bench.json
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SHAPES = {"512x135x240": (512, 135, 240), "64x960x1280": (64, 960, 1280)}
PEAK_FP32_MATRIX_TFLOPS = 157.0
WEIGHTS = {"all_terms": (3e4, 1.5, 0.75), "gram_alone": (3e4, 0.0, 0.0)}


def torch_node(x, s_gram, s_mean, s_std, content, gw, aw, cw):
    """utils/loss_utils.py:230-272 as written there"""
    import torch
    _, c, h, w = x.shape
    loss = 0.0
    if gw:
        f = x.view(c, h * w)
        loss = loss + gw * torch.mean((torch.mm(f, f.t()) - s_gram) ** 2) / (c * h * w)
    if aw:
        mean = torch.mean(x.flatten(2), dim=-1, keepdim=True)
        std = torch.std(x.flatten(2), dim=-1, keepdim=True) + 1e-8
        loss = loss + aw * (torch.nn.functional.mse_loss(mean, s_mean) + torch.nn.functional.mse_loss(std, s_std))
    if cw:
        loss = loss + cw * torch.nn.functional.mse_loss(x, content)
    return loss


def part_node(shape, reps):
    import torch
    from bench_vgg import alternate
    from trase_amd import losses as L
    from trase_amd.rasterizer import profile_enable, profile_report
    dev = torch.device("cuda", 0)
    c, h, w = SHAPES[shape]
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.relu(torch.randn(1, c, h, w, device=dev, generator=g) + 0.3).requires_grad_(True)
    style = torch.relu(torch.randn(1, c, h // 2, w // 2, device=dev, generator=g) * 1.5 + 0.1)
    content = torch.relu(torch.randn(1, c, h, w, device=dev, generator=g) + 0.3)
    T = L.StyleTargets.from_features(style, content)
    s_mean, s_std = T.mean.view(1, c, 1), T.std.view(1, c, 1)
    res = {"shape": [1, c, h, w], "reps": reps, "device": torch.cuda.get_device_name(0)}
    for name, (gw, aw, cw) in WEIGHTS.items():
        def hip():
            x.grad = None
            L.style_statistics_loss(x, T, gram_weight=gw, adain_weight=aw, content_weight=cw).backward()

        def ref():
            x.grad = None
            torch_node(x, T.gram, s_mean, s_std, content, gw, aw, cw).backward()
        t = alternate([hip, ref], reps)
        hip()
        ga = x.grad.clone()
        va = float(L.style_statistics_loss(x, T, gram_weight=gw, adain_weight=aw, content_weight=cw))
        ref()
        vb = float(torch_node(x, T.gram, s_mean, s_std, content, gw, aw, cw))
        res[name] = {"forward_backward": {"hip": t[0], "torch_fp32": t[1]}, "value": {"hip": va, "torch_fp32": vb},
                     "largest_gradient_difference_of_the_sides": {"abs": float((ga - x.grad).abs().max()), "largest_value": float(ga.abs().max())}}
    # (c) the kernels' own times
    profile_enable(1)
    for _ in range(5):
        x.grad = None
        L.style_statistics_loss(x, T, gram_weight=3e4, adain_weight=1.5, content_weight=0.75).backward()
    torch.cuda.synchronize()
    scopes = profile_report()
    profile_enable(0)
    n = h * w
    blocks = -(-c // 32)
    flop = {"gram": 2.0 * 32 * 32 * n * blocks * (blocks + 1) / 2, "style_grad": 2.0 * c * c * n}
    res["kernels"] = {}
    for k in ("gram", "gram_combine", "mean_std", "pixel_loss_fwd", "style_reduce", "style_grad"):
        s = scopes.get(k)
        if s:
            rec = {"ms": round(s["ms"], 4)}
            if k in flop:
                tf = flop[k] / (s["ms"] * 1e-3) / 1e12
                rec.update(gflop=round(flop[k] / 1e9, 2), tflops_fp32=round(tf, 1), share_of_peak=round(tf / PEAK_FP32_MATRIX_TFLOPS, 3))
            res["kernels"][k] = rec
    return res


def part_pixel(reps):
    import torch
    from bench_vgg import alternate
    from trase_amd import losses as L
    dev = torch.device("cuda", 0)
    H, W = 1080, 1920
    x = torch.rand(3, H, W, device=dev).requires_grad_(True)
    gt = torch.rand(3, H, W, device=dev)
    mask = torch.rand(H, W, device=dev) > 0.5
    weight = torch.rand(H, W, device=dev)
    sides = {
        "masked_l1_loss": (lambda: L.masked_l1_loss(x, gt, mask),
                           lambda: (torch.abs(x - gt) * mask.float()[None, :, :].repeat(3, 1, 1)).sum() / mask.float()[None, :, :].repeat(3, 1, 1).sum()),
        "weighted_l1_loss": (lambda: L.weighted_l1_loss(x, gt, weight), lambda: (torch.abs(x - gt) * weight).mean()),
        "l2_loss": (lambda: L.l2_loss(x, gt), lambda: ((x - gt) ** 2).mean()),
    }
    res = {"size": [3, H, W], "reps": reps}
    for name, (hip, ref) in sides.items():
        def run(fn):
            def go():
                x.grad = None
                fn().backward()
            return go
        t = alternate([run(hip), run(ref)], reps)
        res[name] = {"forward_backward": {"hip": t[0], "torch_fp32": t[1]}, "value": {"hip": float(hip()), "torch_fp32": float(ref())}}
    return res


def child(args, limit):
    """run one part of this script as a fresh process under its own time limit; its last line is the part's JSON"""
    print("[bench_style_losses]", " ".join(args), file=sys.stderr, flush=True)
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=limit)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    if out.returncode != 0 or not lines:
        sys.stderr.write(out.stderr[-3000:])
        sys.exit(f"[bench_style_losses] part {args} ended with status {out.returncode}: stopping, nothing further is launched")
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--skip", default="", help="comma-separated parts to leave out: node, pixel, bench")
    ap.add_argument("--part", default=None)
    ap.add_argument("--shape", default="512x135x240")
    a = ap.parse_args()
    if a.part == "node":
        print(json.dumps(part_node(a.shape, a.reps)))
        return
    if a.part == "pixel":
        print(json.dumps(part_pixel(a.reps)))
        return
    skip = set(a.skip.split(",")) if a.skip else set()
    res = {"unmeasured": sorted(skip), "peak_fp32_matrix_tflops": PEAK_FP32_MATRIX_TFLOPS}
    reps = ["--reps", str(a.reps)]
    if "node" not in skip:
        for shape in SHAPES:
            res[shape] = child(["--part", "node", "--shape", shape] + reps, 420)
    if "pixel" not in skip:
        res["pixel_losses_1080p"] = child(["--part", "pixel"] + reps, 300)
    if "bench" not in skip:
        from bench_neighbors import bench_line
        runs = []
        for turn in range(2):
            print(f"[bench_style_losses] bench.py, turn {turn}", file=sys.stderr, flush=True)
            runs.append({"tree": bench_line(None)})
            if a.parent_lib:
                runs[-1]["parent"] = bench_line(a.parent_lib)
        res["bench"] = runs
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
