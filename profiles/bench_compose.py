"""render_composite: the fused compose kernel against the torch composition of the reference's statements, on one GPU.

    python profiles/bench_compose.py [--out profiles/compose_bench.json]

N_bg = 300k, 10 % of a second 300k model selected, 1080p, F = 32, a tensor deformation and a full edit.  Three legs, timed with
HIP events, alternating, medians of 30 after a pre-roll of 10 rounds: the compose launches alone (`compose_models`), the
whole fused `render_composite`, and the torch composition alone (the statements of the reference on activated getters, under
no_grad so that only the forward launches are timed).  Bytes: what the kernel must move, 364 read + 364 written per output row
(+ 8 per gathered row for the index, + 40 per deformed row)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trase_amd import edit  # noqa: E402
from trase_amd.synthetic import SynthGaussianModel, make_scene, orbit_camera  # noqa: E402

N, SHARE, W, H, F = 300_000, 0.10, 1920, 1080, 32
REPS, PREROLL = 30, 10


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "compose_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    bg = SynthGaussianModel(make_scene(N, feat_dim=F, seed=1).to(dev), requires_grad=False)
    dyn = SynthGaussianModel(make_scene(N, feat_dim=F, seed=2).to(dev), requires_grad=False)
    cam = orbit_camera(W, H, angle=0.4).to(dev)
    g = torch.Generator().manual_seed(3)
    d = [(0.01 * torch.randn(N, c, generator=g)).to(dev) for c in (3, 4, 3)]
    mask = (torch.rand(N, generator=g) < SHARE).to(dev)
    rows = torch.nonzero(mask).squeeze(1)
    n_sel = int(rows.shape[0])
    e = edit.rigid_edit(1.5, (0.3, -1.1, 2.0), (0.5, -0.25, 1.0))
    parts = [edit.Part(bg), edit.Part(dyn, d[0], d[1], d[2], rows=rows, edit=e)]
    bgc = torch.zeros(3, device=dev)
    off = torch.tensor([0.5, -0.25, 1.0], device=dev)

    def torch_composition():
        return edit._compose_torch([edit.Part(bg), edit.Part(dyn, d[0], d[1], d[2], rows=mask, edit=e)], dev)

    legs = {
        "compose_kernel_ms": lambda: edit.compose_models(parts),
        "render_composite_ms": lambda: edit.render_composite(cam, bg, dyn, d[0], d[1], d[2], bgc, 1.5, off, (0.3, -1.1, 2.0), 1.0, rows),
        "torch_composition_ms": torch_composition,
    }
    samples = {k: [] for k in legs}
    with torch.no_grad():
        for r in range(PREROLL + REPS):
            for k, fn in legs.items():
                t = timed(fn)
                if r >= PREROLL:
                    samples[k].append(t)
    P = N + n_sel
    nbytes = 2 * 364 * P + (8 + 40) * n_sel
    res = {"N_bg": N, "N_dyn": N, "selected": n_sel, "P": P, "W": W, "H": H, "F": F, "reps": REPS, "preroll": PREROLL,
           "bytes_moved": nbytes, "device": torch.cuda.get_device_name(0)}
    for k, v in samples.items():
        res[k] = round(statistics.median(v), 5)
        res[k.replace("_ms", "_min_ms")] = round(min(v), 5)
        res[k.replace("_ms", "_max_ms")] = round(max(v), 5)
    res["compose_GBps"] = round(nbytes / (res["compose_kernel_ms"] * 1e-3) / 1e9, 1)
    res["torch_over_fused"] = round(res["torch_composition_ms"] / res["compose_kernel_ms"], 2)
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
