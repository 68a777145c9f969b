"""Float64 restatement of the display stage (trase_amd/display.py ``splat_points`` / ``feature_colors``, trase_amd/segment.py
``assign_clusters``): render.py:247-294 (the point-cloud images), render.py:52-59 (``feature3d_to_rgb``) and gui.py:276 +
:288-290 (nearest cluster centre by cosine).

Row-vector convention.  For a point (x, y, z):

    p  = [x, y, z, 1] @ full_proj_transform
    px = (p.x / p.w + 1) / 2 * W,   py = (p.y / p.w + 1) / 2 * H

all in float64 from the inputs as stored.  The point lands at column trunc(px), row trunc(py) if 0 < px < W and 0 < py < H;
there is no near-plane or w > 0 test, and a non-finite coordinate lands nowhere.  The winner of a pixel is the HIGHEST point
index landing there (a sequential assignment).

PCA colours: with Xc = X - mean, the reference's ``q @ (U[:, :3] diag(s[:3]))`` equals ``Xc @ V[:, :3]``, V the top
eigenvectors of Xc^T Xc (``numpy.linalg.eigh``); each axis is signed so that its component of largest magnitude is positive;
colours = (Xc @ V - min) / (max - min) with the single global min and max.

Assignment: id = argmax_k <f / |f|, c_k>, ties to the lowest k.

A plain numpy module (no HIP library, no torch).
"""
from __future__ import annotations

import numpy as np


def _np64(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def camera_fields(cam):
    """(full_proj_transform float64 (4, 4), W, H) of anything shaped like the reference's Camera / MiniCam."""
    return _np64(cam.full_proj_transform), int(cam.image_width), int(cam.image_height)


def project(points, full_proj, W, H):
    """-> (px, py) float64 (N,): the continuous pixel coordinates of render.py:247-251."""
    pts = _np64(points).reshape(-1, 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.concatenate([pts, np.ones((len(pts), 1))], axis=1) @ _np64(full_proj)
        px = (p[:, 0] / p[:, 3] + 1) / 2 * W
        py = (p[:, 1] / p[:, 3] + 1) / 2 * H
    return px, py


def landing(px, py, W, H):
    """-> (lands bool (N,), col int64 (N,), row int64 (N,)); col and row are 0 where the point does not land."""
    with np.errstate(invalid="ignore"):
        ok = (px > 0) & (px < W) & (py > 0) & (py < H)
    col = np.where(ok, np.trunc(np.where(ok, px, 0.0)), 0).astype(np.int64)
    row = np.where(ok, np.trunc(np.where(ok, py, 0.0)), 0).astype(np.int64)
    return ok, col, row


def winner_map(points, cam, mask=None):
    """(H, W) int64: the highest index of ``points`` landing in every pixel, -1 where none lands; ``mask`` (N,) bool selects
    the rows that take part."""
    full, W, H = camera_fields(cam)
    px, py = project(points, full, W, H)
    ok, col, row = landing(px, py, W, H)
    if mask is not None:
        ok = ok & (np.asarray(mask.detach().cpu().numpy() if hasattr(mask, "detach") else mask).reshape(-1) != 0)
    win = np.full(H * W, -1, dtype=np.int64)
    idx = np.nonzero(ok)[0]
    np.maximum.at(win, row[idx] * W + col[idx], idx)
    return win.reshape(H, W)


def gather_image(winner, colors, white_background=False):
    """(3, H, W) float32: ``colors[winner]`` at hit pixels (``colors`` None: the dot, 1 on black and 0 on white), the
    background elsewhere."""
    H, W = winner.shape
    bg, dot = (1.0, 0.0) if white_background else (0.0, 1.0)
    img = np.full((3, H, W), bg, dtype=np.float32)
    hit = winner >= 0
    if colors is None:
        img[:, hit] = dot
    else:
        c = np.asarray(colors.detach().cpu().numpy() if hasattr(colors, "detach") else colors, dtype=np.float32)
        img[:, hit] = c[winner[hit]].T
    return img


def fix_signs(axes):
    """Each row's component of largest magnitude made positive."""
    axes = np.array(axes, dtype=np.float64)
    lead = axes[np.arange(axes.shape[0]), np.abs(axes).argmax(axis=1)]
    return axes * np.where(lead < 0, -1.0, 1.0)[:, None]


def pca_colors(features):
    """-> dict(colors (N, 3), raw (N, 3) projections, axes (3, D), mean (D,), eigenvalues descending (D,)), float64."""
    X = _np64(features)
    X = X.reshape(X.shape[0], -1)
    mean = X.mean(axis=0)
    Xc = X - mean
    val, vec = np.linalg.eigh(Xc.T @ Xc)
    order = np.argsort(val)[::-1]
    D = X.shape[1]
    axes = np.zeros((3, D))
    axes[:min(3, D)] = fix_signs(vec[:, order[:3]].T)
    raw = Xc @ axes.T
    with np.errstate(divide="ignore", invalid="ignore"):
        colors = (raw - raw.min()) / (raw.max() - raw.min())
    return dict(colors=colors, raw=raw, axes=axes, mean=mean, eigenvalues=val[order])


def align_colors(colors, raw64):
    """Globally normalised PCA colours re-signed to the float64 axes.  The colours are an increasing affine image a p + b of
    centred projections p, so p is proportional to ``colors - column mean``; every column that correlates negatively with
    the float64 projection ``raw64`` is negated and the result normalised again with its global min and max.  The centred
    projections have zero column means, so the column means of the colours all equal b up to the rounding of the colours
    (averaged over N rows): colours that already agree come back unchanged to that accuracy."""
    q = _np64(colors)
    q = q - q.mean(axis=0)
    q = q * np.where((q * _np64(raw64)).sum(axis=0) < 0, -1.0, 1.0)
    return (q - q.min()) / (q.max() - q.min())


def cosine_scores(features, centres):
    """(N, K) float64: <f_n / |f_n|, c_k>."""
    X = _np64(features)
    X = X.reshape(X.shape[0], -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        Xn = X / np.linalg.norm(X, axis=1, keepdims=True)
    return Xn @ _np64(centres).T


def assign(features, centres):
    """-> (ids int64 (N,), scores (N, K)): the first (lowest k) maximum of every row; a zero row (NaN scores) gets id 0."""
    s = cosine_scores(features, centres)
    return np.argmax(np.nan_to_num(s, nan=0.0), axis=1).astype(np.int64), s
