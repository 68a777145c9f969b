#!/usr/bin/env python
"""K-steps of the MFMA compositing forward (render_fwd_mf.hip): how many 16-entry steps a launch executes, and in how many of
them the wave still had a live pixel on entry.  Runs the S4 workload (or --gaussians/--width/--height) forward with variant
0x8000 (the counting instantiation, header words 48..49) and prints the counters per view as JSON.  Needs a
`make -C trase_amd/csrc AB=1` build of the library (TRASE_RAST_LIB selects it); add FLAGS+=-DFM_KSTEP_EXIT_=0 for the loop
that tests the wave's pixels once per chunk only."""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trase_amd import rasterizer as R  # noqa: E402
from trase_amd.synthetic import SynthGaussianModel, SynthPipe, make_scene, orbit_camera  # noqa: E402
from gaussian_renderer import render  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--gaussians", type=int, default=300_000)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--scale-mult", type=float, default=0.27)
ap.add_argument("--views", type=int, default=4)
ap.add_argument("--out", default="")
a = ap.parse_args()
dev = torch.device("cuda", 0)
pc = SynthGaussianModel(make_scene(a.gaussians, feat_dim=32, seed=0, scale_mult=a.scale_mult).to(dev))
bg = torch.zeros(3, device=dev)
R.set_sync(True)
R.set_variant(0x8000)     # TRASE_VARIANT_AB_COUNT
tot = {"ksteps_executed": 0, "ksteps_entered_live": 0}
pairs = 0
for k in range(a.views):
    cam = orbit_camera(a.width, a.height, angle=2 * math.pi * k / 16, fid=k / 16).to(dev)
    with torch.no_grad():
        render(cam, pc, SynthPipe(), bg, 0.0, 0.0, 0.0)
    torch.cuda.synchronize()
    hdr = R._Policy.last_geom[:256].view(torch.int32).cpu().tolist()
    tot["ksteps_executed"] += hdr[48] & 0xffffffff
    tot["ksteps_entered_live"] += hdr[49] & 0xffffffff
    pairs += R.last_status()[2]
res = {k: v / a.views for k, v in tot.items()}
res["subtile_pairs"] = pairs / a.views
res["waves"] = 2 * ((a.width + 7) // 8) * ((a.height + 7) // 8)
res["ksteps_per_wave"] = res["ksteps_executed"] / res["waves"]
res["dead_share_of_executed"] = 1.0 - res["ksteps_entered_live"] / max(res["ksteps_executed"], 1)
res["workload"] = f"{a.gaussians} Gaussians {a.width}x{a.height} F=32 scale_mult {a.scale_mult}, {a.views} views"
js = json.dumps(res, indent=1)
print(js)
if a.out:
    open(a.out, "w").write(js)
