"""Generates display.npz from the imported reference's render.py: ``feature3d_to_rgb`` (render.py:52-59) and the statements
that draw the three point-cloud images of a frame (render.py:247-287: the projection, the landing masks and the nine
``buffer_image[...] = ...`` assignments) are pulled out of the file with ``ast`` and run on CPU tensors with ``Tensor.cuda``
made a no-op.

    python tests/golden/make_display.py

Scene: a 96 x 64 view of 2400 points -- a cube cloud that overflows the image, so some points land outside and many pixels
take several points, plus 60 points BEHIND the camera whose flipped projection falls inside the image (the reference has no
w > 0 test) -- with 32-d features drawn around 12 cluster centres of decaying per-dimension scale (a clear spectrum),
rounded to multiples of 1/16 so that the archive stays small.  Cluster colours are a random table indexed by the cluster.

The generator refuses to write the file unless
  * every point's pixel bucket (landing or not, column, row) from the reference's all-fp32 coordinates equals the one from
    the float64 restatement (tests/display_reference.py) -- the seed is shifted until it does;
  * the reference's PCA colours, re-signed to the float64 axes, are within 1e-4 of the float64 colours;
  * every point's two best float64 centre scores are at least 1e-4 apart (any fp32 evaluation then gives the same id).

Records the inputs, the reference's colours, axes (rows of its Vt) and three images, the float64 winner map and the float64
centre-assignment ids.  Runs on the CPU only; the archive is written with fixed time stamps, so it regenerates byte for byte.
"""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden import REF  # noqa: E402  (the imported reference checkout)
from make_lift import write_npz  # noqa: E402
from tests import display_reference as dr  # noqa: E402
from trase_amd.synthetic import orbit_camera  # noqa: E402

W, H = 96, 64
N_CLOUD, N_BEHIND, D, K = 2340, 60, 32, 12
SPLAT_NAMES = ("cur_pts", "cur_pts2d", "buffer_image", "mask_1", "mask_2", "final_mask")


def _target(stmt):
    if not isinstance(stmt, ast.Assign):
        return None
    t = stmt.targets[0]
    if isinstance(t, ast.Name):
        return t.id
    if isinstance(t, ast.Subscript) and isinstance(t.value, ast.Name):
        return t.value.id + "[]"
    return None


def load_reference():
    """-> (feature3d_to_rgb, code object of its body without the return, list of code objects of the splat statements with
    the name each assigns)."""
    tree = ast.parse(open(os.path.join(REF, "render.py")).read())
    pca = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "feature3d_to_rgb")
    ns = {"torch": torch}
    exec(compile(ast.Module(body=[pca], type_ignores=[]), "render.py", "exec"), ns)
    pca_body = compile(ast.Module(body=[s for s in pca.body if not isinstance(s, ast.Return)], type_ignores=[]), "render.py", "exec")
    render_set = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "render_set")
    for node in ast.walk(render_set):
        body = getattr(node, "body", None)
        if isinstance(body, list) and any(_target(s) == "cur_pts" for s in body):
            start = next(i for i, s in enumerate(body) if _target(s) == "cur_pts")
            run = []
            for s in body[start:]:
                inner = s.body if isinstance(s, ast.Try) else [s]       # the cluster-colour image sits in a try block
                for t in inner:
                    if _target(t) in SPLAT_NAMES or _target(t) == "buffer_image[]":
                        run.append(t)
                if sum(_target(t) == "buffer_image[]" for t in run) == 9:
                    break
            names = [_target(t) for t in run]
            assert names.count("buffer_image") == 3 and names.count("buffer_image[]") == 9 and names.count("cur_pts2d") == 3, names
            return ns["feature3d_to_rgb"], pca_body, [(n, compile(ast.Module(body=[t], type_ignores=[]), "render.py", "exec"))
                                                      for n, t in zip(names, run)]
    raise RuntimeError("the splat statements were not found in render.py")


def make_scene(seed):
    g = np.random.default_rng(seed)
    cam = orbit_camera(W, H, angle=0.4)
    cloud = g.uniform(-1.6, 1.6, (N_CLOUD, 3))
    eye = cam.camera_center.double().numpy()
    fwd = -eye / np.linalg.norm(eye)
    behind = eye - fwd * g.uniform(0.5, 3.0, (N_BEHIND, 1)) + g.uniform(-0.3, 0.3, (N_BEHIND, 3))
    points = np.concatenate([cloud, behind])
    label = g.integers(0, K, len(points))
    order = g.permutation(len(points))
    points, label = points[order].astype(np.float32), label[order]
    scale = 2.0 * 0.8 ** np.arange(D)
    centres = g.standard_normal((K, D)) * scale
    feats = centres[label] + 0.15 * g.standard_normal((len(points), D)) * scale
    feats = (np.round(feats * 16) / 16).astype(np.float32)
    table = g.uniform(0, 1, (K, 3)).astype(np.float32)
    mean_rows = np.stack([feats[label == k].astype(np.float64).mean(0) for k in range(K)])
    centres_n = (mean_rows / np.linalg.norm(mean_rows, axis=1, keepdims=True)).astype(np.float32)
    return cam, points, feats, table[label], centres_n


def run_reference(feature3d_to_rgb, pca_body, splat, cam, points, feats, cluster_colors, white_background):
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        colors = feature3d_to_rgb(torch.from_numpy(feats))
        pca_ns = {"torch": torch, "x": torch.from_numpy(feats), "n_components": 3}
        exec(pca_body, pca_ns)
        ns = {"torch": torch, "xyz": torch.from_numpy(points), "d_xyz": torch.zeros(len(points), 3), "view": cam,
              "white_background": white_background, "cluster_point_colors": torch.from_numpy(cluster_colors),
              "gaussians_feature_pca": colors}
        images = []
        for name, code in splat:
            if name == "buffer_image" and "buffer_image" in ns:
                images.append(ns["buffer_image"].numpy().copy())
            exec(code, ns)
        images.append(ns["buffer_image"].numpy().copy())
    finally:
        torch.Tensor.cuda = cuda
    assert torch.equal(pca_ns["pca_normalized"], colors)
    return colors.numpy(), pca_ns["Vt"][:3].numpy(), ns["cur_pts2d"].numpy(), images


def main():
    feature3d_to_rgb, pca_body, splat = load_reference()
    for seed in range(100):
        cam, points, feats, cluster_colors, centres = make_scene(seed)
        ref_colors, ref_axes, ref_px, images = run_reference(feature3d_to_rgb, pca_body, splat, cam, points, feats, cluster_colors, False)
        full, _, _ = dr.camera_fields(cam)
        px, py = dr.project(points, full, W, H)
        ok64, col64, row64 = dr.landing(px, py, W, H)
        ok32, col32, row32 = dr.landing(ref_px[:, 0].astype(np.float64), ref_px[:, 1].astype(np.float64), W, H)
        same = np.array_equal(ok64, ok32) and np.array_equal(col64, col32) and np.array_equal(row64, row32)
        print(f"seed {seed}: fp32 and float64 pixel buckets {'agree' if same else 'differ'}")
        if same:
            break
    else:
        raise SystemExit("refusing to write display.npz: no seed gives equal fp32 and float64 pixel buckets")
    assert ref_colors.dtype == np.float32 and ref_px.dtype == np.float32 and len(images) == 3
    o = dr.pca_colors(feats)
    pca_gap = float(np.abs(dr.align_colors(ref_colors, o["raw"]) - o["colors"]).max())
    ev = o["eigenvalues"]
    ids, scores = dr.assign(feats, centres)
    top2 = np.sort(scores, axis=1)[:, -2:]
    margin = float((top2[:, 1] - top2[:, 0]).min())
    winner = dr.winner_map(points, cam)
    p_w = (np.concatenate([points.astype(np.float64), np.ones((len(points), 1))], 1) @ full)[:, 3]
    behind_landing = int((ok64 & (p_w < 0)).sum())
    crowded = int((np.bincount((row64 * W + col64)[ok64], minlength=H * W) > 1).sum())
    print(f"{len(points)} points, {int(ok64.sum())} land on {int((winner >= 0).sum())} pixels ({crowded} take several), "
          f"{behind_landing} land from behind the camera; reference PCA colours vs float64 after sign alignment: max {pca_gap:.3e}; "
          f"top eigenvalues {ev[:4].round(1).tolist()}; smallest top-2 score gap {margin:.3e}")
    if pca_gap > 1e-4:
        raise SystemExit("refusing to write display.npz: the reference's PCA colours are not within 1e-4 of float64")
    if margin < 1e-4:
        raise SystemExit("refusing to write display.npz: a centre assignment is not decided by 1e-4")
    assert behind_landing >= 10 and crowded >= 100 and int((~ok64).sum()) >= 100 and len(np.unique(ids)) == K
    out = os.path.join(HERE, "display.npz")
    write_npz(out, dict(points=points, full_proj_transform=cam.full_proj_transform.numpy(), width=np.int64(W), height=np.int64(H),
                        features=feats, cluster_colors=cluster_colors, centres=centres, ref_colors=ref_colors, ref_axes=ref_axes,
                        ref_dots=images[0], ref_clusters=images[1], ref_pca=images[2], winner=winner.astype(np.int32),
                        ids=ids.astype(np.int32), pca_gap=np.float64(pca_gap)))
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
