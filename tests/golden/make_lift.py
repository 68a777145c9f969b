"""Generates lift.npz from the imported reference's render.py: ``generate_grid_index`` (render.py:46-50) and the statement
run that lifts a text-prompt mask to cluster ids (render.py:208-231, from ``depth = results["depth"]`` to
``text_masked_cls_id = ...``) are pulled out of the file with ``ast`` and run on CPU tensors, with a brute-force fp32
stand-in for ``pytorch3d.ops.knn_points`` and ``Tensor.cuda`` made a no-op.

    python tests/golden/make_lift.py

Scene: a 96 x 64 view of a smooth surface with a nearer rectangular object on it; the cloud holds one point per 2 x 2 pixel
block, un-projected from the block's centre at the surface's depth there and jittered, plus distractor points behind the
surface and one stray point near the camera, in shuffled order.  Every prompted pixel then has its block's point at about
0.7 pixel spacings and the next one at about 1.6, so the reference's all-fp32 result and the float64 restatement (tests/lift_reference.py) must agree on EVERY
index; the generator checks that and refuses to write the file otherwise.  Twelve prompted pixels have depth 0: they all
un-project to one point near the camera, and the stray point is their nearest.

Records the inputs, the reference's fp32 points, indices, votes and chosen ids.  Runs on the CPU only; the archive is
written with fixed time stamps, so it regenerates byte for byte.
"""
import ast
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden import REF  # noqa: E402  (the imported reference checkout)
from tests import lift_reference as lr  # noqa: E402
from trase_amd.synthetic import orbit_camera  # noqa: E402

W, H = 96, 64
THRESHOLD = 100
RUN = ("depth", "grid_index", "z", "uvz", "text_masked_points_in_3D", "knn_obj", "ijs", "text_masked_points_cls",
       "text_masked_cls_id")


def load_reference():
    """-> (generate_grid_index, code object of the statement run)."""
    tree = ast.parse(open(os.path.join(REF, "render.py")).read())
    grid = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "generate_grid_index")
    ns = {"torch": torch}
    exec(compile(ast.Module(body=[grid], type_ignores=[]), "render.py", "exec"), ns)
    render_set = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "render_set")

    def first_target(stmt):
        return stmt.targets[0].id if isinstance(stmt, ast.Assign) and isinstance(stmt.targets[0], ast.Name) else None

    for node in ast.walk(render_set):
        if isinstance(node, ast.If) and any(first_target(s) == "text_masked_points_in_3D" for s in node.body):
            run = [s for s in node.body if first_target(s) in RUN]
            assert [first_target(s) for s in run] == ["depth", "depth", *RUN[1:]], [first_target(s) for s in run]
            return ns["generate_grid_index"], compile(ast.Module(body=run, type_ignores=[]), "render.py", "exec")
    raise RuntimeError("the lift statements were not found in render.py")


def knn_points(p1, p2, K=1):
    """Brute-force fp32 stand-in for pytorch3d.ops.knn_points at K = 1: squared distances summed per axis, first minimum."""
    assert K == 1 and p1.dtype == torch.float32 and p2.dtype == torch.float32
    idx = torch.empty(p1.shape[1], dtype=torch.int64)
    for lo in range(0, p1.shape[1], 256):
        diff = p1[0, lo:lo + 256, None, :] - p2[0, None, :, :]
        idx[lo:lo + 256] = (diff * diff).sum(-1).argmin(dim=1)
    return types.SimpleNamespace(idx=idx.reshape(1, -1, 1), dists=None, knn=None)


def surface_depth(r, c):
    """The rendered depth at continuous pixel coordinates: a smooth far surface and a nearer object over block-aligned
    columns 36..59, rows 20..43."""
    far = 3.6 + 0.5 * np.sin(c / 17.0) + 0.3 * np.cos(r / 11.0)
    obj = 2.6 + 0.1 * np.sin((r + c) / 9.0)
    inside = (c >= 35.5) & (c < 59.5) & (r >= 19.5) & (r < 43.5)
    return np.where(inside, obj, far)


def make_scene(seed=0):
    g = np.random.default_rng(seed)
    cam = orbit_camera(W, H, angle=0.4)
    full, _, _, znear, zfar = lr.camera_fields(cam)
    rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    depth = surface_depth(rr, cc).astype(np.float32)
    # the cloud: one point per 2 x 2 block, from the block's centre, + distractors behind the surface
    br, bc = np.meshgrid(np.arange(0, H, 2) + 0.5, np.arange(0, W, 2) + 0.5, indexing="ij")
    bd = surface_depth(br, bc).reshape(-1)
    zc = zfar / (zfar - znear) * bd - zfar * znear / (zfar - znear)
    uvz = np.stack([((bc.reshape(-1) - 0.5) / W * 2 - 1) * bd, ((br.reshape(-1) - 0.5) / H * 2 - 1) * bd, zc, bd], axis=1)
    lattice = (uvz @ np.linalg.inv(full))[:, :3] + g.uniform(-0.004, 0.004, (len(bd), 3))
    on_object = (bc.reshape(-1) > 35.5) & (bc.reshape(-1) < 59.5) & (br.reshape(-1) > 19.5) & (br.reshape(-1) < 43.5)
    ids = np.where(on_object, 5, (bc.reshape(-1) // 16) % 5).astype(np.int64)
    toward = lattice.mean(0) - cam.camera_center.double().numpy()
    distract = lattice.mean(0) + toward / np.linalg.norm(toward) * 3.0 + g.uniform(-1.0, 1.0, (500, 3))
    # every zero-depth pixel un-projects to the same point; one stray point near it decides their vote
    stray = (np.array([[0.0, 0.0, -zfar * znear / (zfar - znear), 0.0]]) @ np.linalg.inv(full))[:, :3] + [[0.2, 0.1, -0.15]]
    points = np.concatenate([lattice, distract, stray]).astype(np.float32)
    ids = np.concatenate([ids, np.full(500, 6), [4]])
    order = g.permutation(len(points))
    points, ids = points[order], ids[order]
    # the prompt: an ellipse over the object and part of the surface around it, with a few zero-depth holes
    mask = ((rr - 31.0) / 19.0) ** 2 + ((cc - 50.0) / 24.0) ** 2 <= 1.0
    holes = g.choice(np.flatnonzero(mask.reshape(-1)), 12, replace=False)
    depth.reshape(-1)[holes] = 0.0
    return cam, depth, mask, points, ids.astype(np.float32)


def write_npz(path, arrays):
    """An .npz whose bytes depend on the arrays only (numpy stamps the archive members with the current time)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    generate_grid_index, run = load_reference()
    cam, depth, mask, points, ids = make_scene()
    ns = {"torch": torch, "generate_grid_index": generate_grid_index, "ops": types.SimpleNamespace(knn_points=knn_points),
          "results": {"depth": torch.from_numpy(depth).unsqueeze(0)}, "view": cam, "text_mask": torch.from_numpy(mask),
          "xyz": torch.from_numpy(points), "d_xyz": torch.zeros(len(points), 3), "cluster_ids_x": torch.from_numpy(ids),
          "threshold": THRESHOLD}
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        exec(run, ns)
    finally:
        torch.Tensor.cuda = cuda
    ref_points = ns["text_masked_points_in_3D"].numpy()
    ref_index = ns["ijs"].numpy()
    ref_votes = torch.bincount(ns["text_masked_points_cls"]).numpy()
    ref_ids = ns["text_masked_cls_id"].reshape(-1).numpy()
    assert ref_points.dtype == np.float32 and ref_points.shape == (int(mask.sum()), 3)

    o = lr.lift(depth, mask, cam, points, ids, threshold=THRESHOLD)
    gap = float(np.abs(ref_points.astype(np.float64) - o["points"]).max())
    margin = float((o["d2"] - o["d1"]).min())
    differ = int((o["index"] != ref_index).sum())
    print(f"{len(ref_index)} prompted pixels, {len(points)} points; fp32 reference vs float64 points: max {gap:.3e}; "
          f"smallest second-nearest minus nearest distance {margin:.3e}; indices differing: {differ}")
    same_votes = np.array_equal(o["votes"][:len(ref_votes)], ref_votes) and not o["votes"][len(ref_votes):].any()
    if differ or margin < 20 * gap or not same_votes or not np.array_equal(o["chosen"], ref_ids):
        raise SystemExit("refusing to write lift.npz: the reference and the float64 restatement do not agree on every query")
    assert 0 < len(ref_ids) < len(ref_votes) and int((depth[mask] == 0).sum()) == 12
    out = os.path.join(HERE, "lift.npz")
    write_npz(out, dict(depth=depth, prompt_mask=mask, full_proj_transform=cam.full_proj_transform.numpy(),
                        znear=np.float64(cam.znear), zfar=np.float64(cam.zfar), points=points, cluster_ids=ids,
                        threshold=np.int64(THRESHOLD), ref_points=ref_points, ref_index=ref_index.astype(np.int32),
                        ref_votes=ref_votes.astype(np.int64), ref_ids=ref_ids.astype(np.int64)))
    print("wrote", out, os.path.getsize(out), "bytes; votes", ref_votes.tolist(), "chosen", ref_ids.tolist())


if __name__ == "__main__":
    main()
