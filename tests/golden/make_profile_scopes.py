"""Generates profile_scopes.json: the profiler report's {scope name: count} after one fixed sequence of calls -- the keys and
per-key counts that bench.py and profiles/bench_*.py read.  tests/test_gpu_profile_scopes.py runs the same sequence on the
library under test and asserts the same table, so a change of the host-side launch plumbing cannot rename, merge, split, add
or drop a scope unnoticed.  Regenerate it only from a commit whose scopes are known to be right, never from the code under
test (the table was recorded from the commit before the launch sites were put on TRASE_LAUNCH / TRASE_LAUNCHES).

    python tests/golden/make_profile_scopes.py     (needs a GPU; TRASE_RAST_LIB=<path> selects another build of the library)

The sequence, every call once, with profile_enable(1) and the synchronising capacity policy: the operator path forward +
backward (64 Gaussians, 32 x 32, F = 32), the fused raw path forward + backward on the same scene, knn_points (N = 100, K = 4),
l1_ssim forward + backward on 3 x 16 x 16, feature_colors (trase_feature_gram + trase_feature_project; N = 64, D = 16).  The
smallest shapes at which every stage of both front doors launches: live Gaussians, so that the sort, the scan, the emit and both
compositing directions run, and F = 32, so that the MFMA paths are the ones counted."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

P, W, H, F = 64, 32, 32, 32


def _calls(dev):
    import torch
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from gaussian_renderer import render
    from tests.util import settings_for
    from trase_amd.display import feature_colors
    from trase_amd.losses import l1_ssim
    from trase_amd.rasterizer import knn_points
    from trase_amd.synthetic import SynthGaussianModel, SynthPipe, make_scene, orbit_camera

    g = torch.Generator().manual_seed(0)
    scene = make_scene(P, feat_dim=F, seed=0, scale_mult=0.9)
    cam = orbit_camera(W, H, angle=0.4)
    g_img, g_feat = torch.randn(3, H, W, generator=g).to(dev), torch.randn(F, H, W, generator=g).to(dev)

    # the operator path
    st_cpu = settings_for(cam, bg=(0.1, 0.2, 0.3))
    st = GaussianRasterizationSettings(**{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in st_cpu._asdict().items()})
    leaves = {k: v.to(dev).clone().requires_grad_(True) for k, v in scene.activated().items()}
    m2d = torch.zeros(P, 3, device=dev, requires_grad=True)
    img, _, feats, _ = GaussianRasterizer(raster_settings=st)(
        means3D=leaves["means3D"], means2D=m2d, shs=leaves["shs"], sh_objs=leaves["sh_objs"], opacities=leaves["opacities"],
        scales=leaves["scales"], rotations=leaves["rotations"])
    torch.autograd.backward([img, feats], [g_img, g_feat])

    # the fused raw path, same scene
    pc = SynthGaussianModel(scene.to(dev))
    out = render(cam.to(dev), pc, SynthPipe(), torch.tensor([0.1, 0.2, 0.3], device=dev), 0.0, 0.0, 0.0)
    torch.autograd.backward([out["render"], out["render_gaussian_features"]], [g_img, g_feat])

    pts = torch.randn(1, 100, 3, generator=g).to(dev)
    knn_points(pts, pts, K=4)

    a = torch.rand(3, 16, 16, generator=g).to(dev).requires_grad_(True)
    b = torch.rand(3, 16, 16, generator=g).to(dev)
    l1, ss = l1_ssim(a, b)
    (l1 + ss).backward()

    feature_colors(torch.randn(64, 16, generator=g).to(dev))
    torch.cuda.synchronize(dev)


def collect():
    """-> {scope name: count} of the sequence on the loaded library"""
    import torch
    from trase_amd import rasterizer as R
    dev = torch.device("cuda", 0)
    sync = R._Policy.sync
    R.set_sync(True)
    R.profile_enable(1)
    try:
        _calls(dev)
        rep = R.profile_report()
    finally:
        R.profile_enable(0)
        R.set_sync(sync)
    return {k: int(v["n"]) for k, v in sorted(rep.items())}


def main():
    out = os.path.join(HERE, "profile_scopes.json")
    table = collect()
    with open(out, "w") as f:
        f.write(json.dumps(table, indent=1) + "\n")
    print("wrote", out, os.path.getsize(out), "bytes,", len(table), "scopes,", sum(table.values()), "launch scopes")


if __name__ == "__main__":
    main()
