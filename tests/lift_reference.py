"""Float64 restatement of the prompt lift (trase_amd/segment.py ``lift_votes`` / ``pick``, the lift kernels of
trase_amd/csrc/knn.hip): render.py:208-229 (a text-prompt mask), gui.py:1039-1064 (the same in the viewer) and
gui.py:786-800 (one clicked pixel).

Row-vector convention.  For a prompted pixel at row r, column c with rendered depth d:

    z   = zfar / (zfar - znear) * d - zfar * znear / (zfar - znear)
    uvz = [((c - 0.5) / W * 2 - 1) * d, ((r - 0.5) / H * 2 - 1) * d, z, d]
    p   = (uvz @ inverse(full_proj_transform))[:3]            (no division by the 4th component)

all in float64, the inverse taken in float64 of the camera's matrix as it is stored.  The nearest point of ``points`` to p
(exact, scipy's cKDTree over the float64 copies) gives index j; the vote goes to bin int(cluster_ids[j]); a negative id casts
no vote.  ``chosen`` are the bins with votes > threshold.

A plain numpy module (no HIP library, no torch).
"""
from __future__ import annotations

import numpy as np
from scipy.spatial import cKDTree


def _np64(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def camera_fields(cam):
    """(full_proj_transform float64 (4, 4), W, H, znear, zfar) of anything shaped like the reference's Camera / MiniCam."""
    return _np64(cam.full_proj_transform), int(cam.image_width), int(cam.image_height), float(cam.znear), float(cam.zfar)


def unproject(depth, rows, cols, full_proj, W, H, znear, zfar):
    """float64 points (M, 3) of the pixels (rows[i], cols[i]) of the depth map (H, W)."""
    depth = _np64(depth).reshape(H, W)
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    d = depth[rows, cols]
    z = zfar / (zfar - znear) * d - zfar * znear / (zfar - znear)
    uvz = np.stack([((cols - 0.5) / W * 2 - 1) * d, ((rows - 0.5) / H * 2 - 1) * d, z, d], axis=1)
    return (uvz @ np.linalg.inv(_np64(full_proj)))[:, :3]


def nearest2(queries, points):
    """(d1, d2, i1): float64 distances to the nearest and second-nearest point and the nearest index, for every query.
    With a single point d2 is inf."""
    points = _np64(points)
    k = 2 if len(points) > 1 else 1
    d, i = cKDTree(points).query(_np64(queries), k=k)
    d, i = d.reshape(len(queries), k), i.reshape(len(queries), k)
    d2 = d[:, 1] if k == 2 else np.full(len(queries), np.inf)
    return d[:, 0], d2, i[:, 0].astype(np.int64)


def count_votes(cluster_ids, index, bins=None):
    """bincount of int(cluster_ids[index]) over the non-negative ids; ``bins`` None sizes it from the largest id of ALL
    cluster ids (what ``lift_votes(num_clusters=None)`` does), never smaller than 1."""
    ids = np.asarray(_np64(cluster_ids)).astype(np.int64).reshape(-1)
    if bins is None:
        bins = max(int(ids.max()) + 1, 1) if ids.size else 1
    voted = ids[np.asarray(index, dtype=np.int64)]
    voted = voted[voted >= 0]
    return np.bincount(voted, minlength=bins)[:bins].astype(np.int64)


def lift(depth, prompt_mask, cam, points, cluster_ids, threshold=0, bins=None):
    """-> dict(points (M, 3) float64, d1, d2, index (M,), rows, cols, votes (bins,), chosen) for the prompted pixels in
    row-major order (the order of ``depth[prompt_mask]``)."""
    full, W, H, znear, zfar = camera_fields(cam)
    mask = np.asarray(prompt_mask.detach().cpu().numpy() if hasattr(prompt_mask, "detach") else prompt_mask).reshape(H, W) != 0
    rows, cols = np.nonzero(mask)
    pts = unproject(depth, rows, cols, full, W, H, znear, zfar)
    n = len(_np64(points))
    if n == 0 or len(rows) == 0:
        d1 = d2 = np.zeros(len(rows))
        index = np.full(len(rows), -1, dtype=np.int64)
        votes = count_votes(cluster_ids, index[:0], bins)
    else:
        d1, d2, index = nearest2(pts, points)
        votes = count_votes(cluster_ids, index, bins)
    return dict(points=pts, d1=d1, d2=d2, index=index, rows=rows, cols=cols, votes=votes,
                chosen=np.nonzero(votes > threshold)[0].astype(np.int64))


def index_map(result, H, W):
    """(H, W) int64: the nearest index at every prompted pixel, -1 elsewhere."""
    m = np.full((H, W), -1, dtype=np.int64)
    m[result["rows"], result["cols"]] = result["index"]
    return m
