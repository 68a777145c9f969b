"""numpy restatement of the three rules of trase_amd/csrc/trajectory.hip: the farthest-point sampler in float32, the
trajectory overlay (float64 projection, integer line rule, highest index wins) and the frame finish.  No GPU, no torch
kernels: what the GPU tests compare against, itself checked on the CPU by tests/test_trajectory_reference.py."""
import numpy as np

COORD_LIMIT = float(1 << 20)


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


# ---- sampler -----------------------------------------------------------------------------------------------------------------

def fps(points, npoint, start, mask=None):
    """utils/time_utils.py:375-396 at B = 1 in float32: d = (dx*dx + dy*dy) + dz*dz, every operation rounded to float32,
    running minimum from 1e10 on strict <, arg-max with the lowest row among equals (numpy's argmax).  mask selects the
    candidates; the rows returned index `points`."""
    p = np.ascontiguousarray(_np(points), dtype=np.float32).reshape(-1, 3)
    rows = np.arange(len(p)) if mask is None else np.nonzero(_np(mask).reshape(-1))[0]
    q = p[rows]
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    dist = np.full(len(q), 1e10, dtype=np.float32)
    out = np.empty(npoint, dtype=np.int64)
    far = int(np.nonzero(rows == start)[0][0])
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(npoint):
            out[i] = rows[far]
            dx, dy, dz = x - x[far], y - y[far], z - z[far]
            d = (dx * dx + dy * dy) + dz * dz
            assert d.dtype == np.float32
            np.copyto(dist, d, where=d < dist)
            far = int(np.argmax(dist))
    return out


# ---- overlay -----------------------------------------------------------------------------------------------------------------

def camera_fields(cam):
    return _np(cam.full_proj_transform).astype(np.float64), int(cam.image_width), int(cam.image_height)


def pixels(coords, full, W, H):
    """(..., 3) fp32 world positions -> (ix, iy int64, ok bool): float64 projection, [W, H] scale, truncation toward zero; ok is
    False where a coordinate is non-finite or at least 2^20 in magnitude."""
    c = _np(coords).astype(np.float32).astype(np.float64)
    x, y, z = c[..., 0], c[..., 1], c[..., 2]
    m = full
    with np.errstate(all="ignore"):
        px_h = x * m[0, 0] + y * m[1, 0] + z * m[2, 0] + m[3, 0]
        py_h = x * m[0, 1] + y * m[1, 1] + z * m[2, 1] + m[3, 1]
        w = x * m[0, 3] + y * m[1, 3] + z * m[2, 3] + m[3, 3]
        px = (px_h / w + 1.0) / 2.0 * W
        py = (py_h / w + 1.0) / 2.0 * H
        ok = (np.abs(px) < COORD_LIMIT) & (np.abs(py) < COORD_LIMIT)          # a NaN fails
    ix = np.where(ok, np.trunc(np.where(ok, px, 0.0)), 0).astype(np.int64)
    iy = np.where(ok, np.trunc(np.where(ok, py, 0.0)), 0).astype(np.int64)
    return ix, iy, ok


def line_pixels(ax, ay, bx, by, W, H):
    """The in-image pixels (x, y int64 arrays) of the segment a -> b by the line rule, visiting only the in-image range of
    the major axis."""
    ax, ay, bx, by = int(ax), int(ay), int(bx), int(by)
    dx, dy = abs(bx - ax), abs(by - ay)
    if dx >= dy:
        au, av, bu, bv, du, dv, nu, nv = ax, ay, bx, by, dx, dy, W, H
    else:
        au, av, bu, bv, du, dv, nu, nv = ay, ax, by, bx, dy, dx, H, W
    u = np.arange(max(min(au, bu), 0), min(max(au, bu), nu - 1) + 1, dtype=np.int64)
    if du == 0:
        v = np.full(len(u), av, dtype=np.int64)
    else:
        sign = 1 if bv > av else -1
        v = av + sign * ((2 * np.abs(u - au) * dv + du) // (2 * du))
    keep = (v >= 0) & (v < nv)
    u, v = u[keep], v[keep]
    return (u, v) if dx >= dy else (v, u)


def winner_map(coords, cam):
    """(S, G, 3) positions, oldest first -> (H, W) int64: the highest trajectory index whose polyline passes, -1 elsewhere."""
    full, W, H = camera_fields(cam)
    c = _np(coords)
    S, G = c.shape[0], c.shape[1]
    win = np.full((H, W), -1, dtype=np.int64)
    if S == 0:
        return win
    ix, iy, ok = pixels(c, full, W, H)
    for g in range(G):                                   # ascending: a later trajectory overwrites an earlier one
        pairs = [(0, 0)] if S == 1 else [(s, s + 1) for s in range(S - 1)]
        for a, b in pairs:
            if ok[a, g] and ok[b, g]:
                x, y = line_pixels(ix[a, g], iy[a, g], ix[b, g], iy[b, g], W, H)
                win[y, x] = g
    return win


def overlay_image(win, colors):
    """(H, W) winner map, (G, 3) fp32 colours -> the (H, W, 4) fp32 overlay."""
    colors = _np(colors).astype(np.float32)
    out = np.zeros(win.shape + (4,), dtype=np.float32)
    hit = win >= 0
    out[hit, :3] = colors[win[hit]]
    out[hit, 3] = 1.0
    return out
