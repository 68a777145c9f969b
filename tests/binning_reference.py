"""Plain numpy restatements of the integer stages of trase_amd/csrc/binning.hip that sit between the depth sort and the pair
sort -- the live compaction, the tile scan, the lineage rect count -- of the order every finished sub-tile list must have, and
a float64 membership band for the one decision of the stage that is not an integer algorithm: which borderline 8x8 sub-tiles
a splat reaches.  tests/test_binning_reference.py checks every function against brute force on the CPU;
tests/test_gpu_binning.py compares the kernels with them, array_equal everywhere except the band.  Not a test module.

The membership band
-------------------
For a Gaussian with float32 centre (gx, gy), conic (A, B, C), opacity o and radius r (the device's own values, taken to
float64 without further rounding) and an 8x8 sub-tile, with q(dx, dy) = A dx^2 + 2 B dx dy + C dy^2 and tau = 2 ln(255 o):

  REQUIRED   the sub-tile lies in the Gaussian's 16x16 tile rect (tile_rect, restated in float32: two sums and a division by
             16, exact), in the image and in the strip, and SOME pixel centre (x, y) of the block has q(x - gx, y - gy) <= tau.
             That is the compositing gate itself (alpha = o exp(-q / 2) >= 1 / 255): a list that lacks such a pair changes a pixel.
  FORBIDDEN  the sub-tile lies outside the rect, the image or the strip; or o < 1 / 255; or the float64 minimum of q over the
             CONTINUOUS box of the block's pixel centres, grown by m on each side, exceeds tau_hi.
  FREE       everything else: the kernel may list the pair or not.

Margins, and where they come from.  The kernel (gs_math.h subtile_cull_setup / subtile_row_live) lists a block when the
ellipse q <= tau_k, tau_k = 1.001 tau + 1e-3 in float32, reaches the block's pixel-centre columns inside the row's band of
pixel-centre rows, each side padded by pad = 4e-3 px.  Its float32 roots are what the two widenings cover:
  tau_hi = (1.001 tau + 1e-3) (1 + 1e-3)   the kernel's own threshold and a relative 1e-3 on top: tau_k, the determinant, the
            discriminant A tau_k - det dy^2 and the square root are each a handful of float32 roundings (2^-24 = 6e-8 relative
            each) -- cancellation in det = A C - B^2 amplifies them by the conic's condition number, which the scenes keep below
            1e3: 1e-3 relative covers 6e-8 x 10 roundings x 1e3.
  m = 0.016 px   four times the kernel's documented pad: the pad itself, and the float32 rounding of gx + hi + pad for centres
            within +-2^14 px (ulp 1e-3 px), which is what the remaining 0.012 px are for.
A block whose continuous box lies farther than m outside the ellipse q <= tau_hi can therefore only be listed by a defect.
Both premises are asserted with the band, per scene, by the CPU and the GPU test (band_premises): condition number below 1e3
(the largest is the giant's, 876; every other scene stays below 7) and centres within +-2^14 px.

One defect of that kind was found and fixed with these tests.  subtile_row_live tested the columns of a row against the
unclipped block 8 sx .. 8 sx + 7, although only the pixel centres up to W - 1 exist: in an image whose width is no multiple of 8,
a splat centred right of the last pixel whose left edge fell among the missing columns was counted and emitted for a pair that
no pixel can use (off-edge-9x9: 11 forbidden pairs on the host build, min q over the grown box 11.5 to 24.3 against tau_hi
10.5 to 11.0; off-edge-67x35 likewise).  The band was right and the margins stayed; the row rule now drops a row whose interval
begins right of W - 1.  The scenes off-edge-67x35 and off-edge-9x9 keep the case: splats centred right of and below such an image.
With that, no forbidden pair is listed in any scene, on the host build or on the device.

Not positive definite conics (A <= 0, C <= 0 or A C <= B^2 in float64): the kernel keeps every block of the rect; the band
leaves them free.  None of the scenes has one.

Free-pair share (free / required, must stay <= 2 %; tests/test_binning_reference.py asserts it on the float32-rounded geometry
of oracle/raster_oracle.py, tests/test_gpu_binning.py on the device's own and prints it).  Measured, required / free -- the
device's geometry gave the same counts as the oracle's in every scene, through the cooked entry and the fused render():
  96x64-P1025 24179 / 64 (0.26 %)   96x64-P63 4453 / 3   67x35-P1025 12587 / 36 (0.29 %)   67x35-P63 2101 / 3
  9x9-P63 193 / 0   9x9-P1 4 / 0   8x8-P63 63 / 0   8x8-P1 1 / 0   dense 23678 / 60 (0.25 %)   ties 9794 / 19
  giant 2266 / 26 (1.15 %: one thin slanted splat, the free pairs are blocks its edge crosses between two pixel centres)
  faint-culled 7475 / 10   slot-fallback 79472 / 137 (0.17 %)   off-edge-67x35 2510 / 9 (0.36 %)   off-edge-9x9 216 / 0
  under the tile-row strip (1, 4): 96x64-P1025 18977 / 49, dense 11222 / 26, faint-culled 5866 / 9
"""
from __future__ import annotations

import math

import numpy as np

SC_TILE = 1024                 # depth ranks per workgroup of scan_partial_kernel
EMIT_BIG, EMIT_STAGE = 160, 3072
TILE, SUB = 16, 8
FREE, REQUIRED, FORBIDDEN = 0, 1, 2
PAD_M = 0.016                  # px


# ---- compaction, scan, rect count, order ----------------------------------------------------------------------------------------
def compact_live(tiles: np.ndarray, keys: np.ndarray):
    """-> (live ids ascending, their keys, the ids without a pair ascending, live count)"""
    tiles = np.asarray(tiles)
    live = np.flatnonzero(tiles != 0)
    dead = np.flatnonzero(tiles == 0)
    return live.astype(np.uint32), np.asarray(keys)[live].astype(np.uint32), dead.astype(np.uint32), int(live.size)


def scan_tiles(tiles: np.ndarray, ids_in_rank_order: np.ndarray, n_live: int):
    """-> (inclusive pair offsets per depth rank (uint64, n_live entries), R_eff, the largest count of one rank)"""
    v = np.asarray(tiles)[np.asarray(ids_in_rank_order)[:n_live].astype(np.int64)].astype(np.uint64)
    incl = np.cumsum(v, dtype=np.uint64)
    return incl, int(incl[-1]) if n_live else 0, int(v.max(initial=0))


def scan_device_form(incl: np.ndarray, P: int):
    """What the two scan kernels leave behind for an inclusive scan `incl` of n_live ranks among P: the block-local inclusive
    sums and every block's exclusive prefix (blocks behind the last rank hold the total)."""
    n = incl.shape[0]
    nblocks = (P + SC_TILE - 1) // SC_TILE
    starts = np.arange(nblocks, dtype=np.int64) * SC_TILE
    excl = np.zeros(nblocks, dtype=np.uint64)
    has = starts > 0
    excl[has] = incl[np.minimum(starts[has], n) - 1] if n else 0
    local = incl - excl[np.arange(n) // SC_TILE]
    return local.astype(np.uint32), excl.astype(np.uint32)


def tile_rect(xy: np.ndarray, radii: np.ndarray, gx: int, gy: int):
    """gs_math.h tile_rect in float32 operations -> x0, y0, x1, y1 (int64, half-open, in 16x16 tiles)"""
    xy = np.asarray(xy, dtype=np.float32)
    r = np.asarray(radii).astype(np.float32)
    t, t1 = np.float32(TILE), np.float32(TILE - 1)

    def edge(v, g):
        return np.clip(np.trunc(v / t).astype(np.int64), 0, g)
    px, py = xy[:, 0], xy[:, 1]
    return edge(px - r, gx), edge(py - r, gy), edge(px + r + t1, gx), edge(py + r + t1, gy)


def tile_rect_area(xy: np.ndarray, radii: np.ndarray, gx: int, gy: int) -> int:
    """The lineage pair count HDR_R: the summed rect areas of the Gaussians with a radius."""
    radii = np.asarray(radii)
    has = radii > 0                                             # (the centre of a Gaussian without a radius is undefined)
    x0, y0, x1, y1 = tile_rect(np.asarray(xy, dtype=np.float32)[has], radii[has], gx, gy)
    return int(((x1 - x0) * (y1 - y0)).sum())


def expected_order(depth_bits: np.ndarray, ids: np.ndarray) -> np.ndarray:
    """The ids in depth-rank order: stable ascending sort of the float32 depth bits, ties by Gaussian index."""
    ids = np.sort(np.asarray(ids).astype(np.int64))
    return ids[np.argsort(np.asarray(depth_bits).astype(np.uint32)[ids], kind="stable")]


# ---- the membership band ------------------------------------------------------------------------------------------------------------
def tau_hi(opacity: np.ndarray) -> np.ndarray:
    with np.errstate(divide="ignore", invalid="ignore"):
        tau = 2.0 * np.log(255.0 * np.asarray(opacity, dtype=np.float64))
    return (1.001 * tau + 1e-3) * (1.0 + 1e-3)


def box_min_form(A, B, C, x_lo, x_hi, y_lo, y_hi):
    """float64 minimum of A dx^2 + 2 B dx dy + C dy^2 (positive definite) over the box [x_lo, x_hi] x [y_lo, y_hi] of offsets
    from the centre: 0 when the box holds the centre, else attained on one of the four edges at the clamped edge minimiser."""
    def q(dx, dy):
        return A * dx * dx + 2.0 * B * dx * dy + C * dy * dy
    inside = (x_lo <= 0) & (x_hi >= 0) & (y_lo <= 0) & (y_hi >= 0)
    best = np.full(np.broadcast(A, x_lo, y_lo).shape, np.inf)
    for dx in (x_lo, x_hi):                                 # vertical edges: dy free in [y_lo, y_hi]
        dy = np.clip(-B * dx / C, y_lo, y_hi)
        best = np.minimum(best, q(dx, dy))
    for dy in (y_lo, y_hi):
        dx = np.clip(-B * dy / A, x_lo, x_hi)
        best = np.minimum(best, q(dx, dy))
    return np.where(inside, 0.0, best)


def membership_band(xy, conic_opacity, radii, W: int, H: int, strip=(0, 0), sel=None) -> np.ndarray:
    """(len(sel), T) int8 of FREE / REQUIRED / FORBIDDEN for the Gaussians `sel` (default: all) and every 8x8 sub-tile, row-major.
    xy (P, 2), conic_opacity (P, 4) = A, B, C, o and radii (P,) are the device's float32 / int32 values; strip = (begin, end) rows
    of 16x16 tiles, (0, 0) = the whole image."""
    xy32 = np.asarray(xy, dtype=np.float32)
    radii = np.asarray(radii).astype(np.int64)
    sel = np.arange(xy32.shape[0]) if sel is None else np.asarray(sel, dtype=np.int64)
    co = np.zeros((xy32.shape[0], 4), dtype=np.float64)        # (records of Gaussians outside `sel` may be undefined)
    co[sel] = np.asarray(conic_opacity, dtype=np.float32)[sel]
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    gx8, gy8 = (W + SUB - 1) // SUB, (H + SUB - 1) // SUB
    sy_lo, sy_hi = 0, gy8
    if tuple(strip) != (0, 0):
        sy_lo, sy_hi = min(2 * strip[0], gy8), min(2 * strip[1], gy8)
    out = np.full((sel.size, gx8 * gy8), FORBIDDEN, dtype=np.int8)
    rect = np.zeros((4, xy32.shape[0]), dtype=np.int64)        # (centres of Gaussians outside `sel` may be undefined)
    rect[:, sel] = tile_rect(xy32[sel], np.maximum(radii[sel], 1), gx, gy)
    x0, y0, x1, y1 = rect
    sx = np.arange(gx8)
    sy = np.arange(gy8)
    # pixel centres of every block (clipped to the image), as offsets into one (gy8, 8) / (gx8, 8) table; a clipped-away centre repeats the last one
    px = np.minimum(sx[:, None] * SUB + np.arange(SUB)[None, :], W - 1).astype(np.float64)
    py = np.minimum(sy[:, None] * SUB + np.arange(SUB)[None, :], H - 1).astype(np.float64)
    thi = tau_hi(co[:, 3])
    for k, i in enumerate(sel):
        if radii[i] <= 0:
            continue
        A, B, C, o = co[i]
        cx, cy = float(xy32[i, 0]), float(xy32[i, 1])
        in_rect = ((sx >= 2 * x0[i]) & (sx < 2 * x1[i]))[None, :] & ((sy >= 2 * y0[i]) & (sy < 2 * y1[i]) & (sy >= sy_lo) & (sy < sy_hi))[:, None]
        if not in_rect.any() or not (o >= 1.0 / 255.0):
            continue
        tau = 2.0 * math.log(255.0 * o)
        dx = px - cx                                            # (gx8, 8)
        dy = py - cy                                            # (gy8, 8)
        qq = (A * dx * dx)[None, :, None, :] + (2.0 * B) * dy[:, None, :, None] * dx[None, :, None, :] + (C * dy * dy)[:, None, :, None]
        req = (qq <= tau).any(axis=(2, 3))                      # (gy8, gx8)
        if A > 0 and C > 0 and A * C - B * B > 0:
            bmin = box_min_form(A, B, C, (px[:, 0] - PAD_M - cx)[None, :], (px[:, -1] + PAD_M - cx)[None, :],
                                (py[:, 0] - PAD_M - cy)[:, None], (py[:, -1] + PAD_M - cy)[:, None])
            forb = bmin > thi[i]
        else:
            forb = np.zeros_like(req)
        cls = np.where(req, REQUIRED, np.where(forb, FORBIDDEN, FREE)).astype(np.int8)
        out[k] = np.where(in_rect, cls, FORBIDDEN).reshape(-1)
    return out


def band_premises(xy, conic_opacity, sel) -> tuple:
    """What the margins' error analysis assumes of the Gaussians `sel`: (largest condition number of a conic, largest |centre|)"""
    co = np.asarray(conic_opacity, dtype=np.float32)[sel].astype(np.float64)
    mid = 0.5 * (co[:, 0] + co[:, 2])
    d = np.sqrt(np.maximum(mid * mid - (co[:, 0] * co[:, 2] - co[:, 1] ** 2), 0.0))
    return float(((mid + d) / (mid - d)).max(initial=1.0)), float(np.abs(np.asarray(xy, dtype=np.float32)[sel]).max(initial=0.0))


def band_counts(band: np.ndarray):
    return int((band == REQUIRED).sum()), int((band == FREE).sum())


def describe_pair(i: int, t: int, xy, conic_opacity, radii, W: int, H: int) -> str:
    """The float64 numbers behind the band's answer for Gaussian i and sub-tile t (for a failing membership check)."""
    gx8 = (W + SUB - 1) // SUB
    sx, sy = t % gx8, t // gx8
    A, B, C, o = (float(v) for v in np.asarray(conic_opacity, dtype=np.float32)[i])
    cx, cy = (float(v) for v in np.asarray(xy, dtype=np.float32)[i])
    x_lo, x_hi = sx * SUB - cx, min(sx * SUB + SUB - 1, W - 1) - cx
    y_lo, y_hi = sy * SUB - cy, min(sy * SUB + SUB - 1, H - 1) - cy
    xs, ys = np.arange(x_lo, x_hi + 0.5), np.arange(y_lo, y_hi + 0.5)
    q_pix = float((A * xs[None, :] ** 2 + 2 * B * xs[None, :] * ys[:, None] + C * ys[:, None] ** 2).min())
    pd = A > 0 and C > 0 and A * C - B * B > 0
    q_box = float(box_min_form(A, B, C, x_lo - PAD_M, x_hi + PAD_M, y_lo - PAD_M, y_hi + PAD_M)) if pd else float("nan")
    tau = 2.0 * math.log(255.0 * o) if o > 0 else float("-inf")
    return (f"Gaussian {i} sub-tile {t} (column {sx}, row {sy}): centre ({cx!r}, {cy!r}) conic ({A!r}, {B!r}, {C!r}) opacity {o!r} "
            f"radius {int(np.asarray(radii)[i])}; tau {tau!r} tau_hi {float(tau_hi(np.array([o]))[0])!r}; min q over pixel centres {q_pix!r}, "
            f"over the grown continuous box {q_box!r}")


# ---- the scenes of the finished-list tests --------------------------------------------------------------------------------------------
def _scene(n, w, h, seed, scale_mult=0.9, **cam_kw):
    from trase_amd.synthetic import make_scene, orbit_camera
    return make_scene(n, feat_dim=32, seed=seed, scale_mult=scale_mult), orbit_camera(w, h, angle=0.4, **cam_kw)


def _towards_camera(cam, dist):
    """the point at view depth `dist` on the optical axis (the camera looks at the origin)"""
    import torch
    eye = cam.camera_center.to(torch.float32)
    return eye * (1.0 - dist / float(eye.norm()))


def build_scene(name: str):
    """-> (SynthScene, SynthCamera, notes) on the CPU.  Every edit is to the raw parameters, so that the cooked entry and the
    fused render() see the same scene."""
    import torch
    g = torch.Generator().manual_seed(1234)
    notes = {}
    if name in SMALL:
        w, h, n, seed = SMALL[name]
        scene, cam = _scene(n, w, h, seed)
    elif name == "giant":
        # one slanted, elongated Gaussian over all 70 sub-tile rows of a narrow image, ~5 of its 9 columns in each: the whole-wave
        # path of emit_pairs (more than EMIT_BIG pairs) and its second trip (more than 64 rows)
        scene, cam = _scene(48, 72, 560, seed=5, scale_mult=0.5)
        scene.xyz[7] = 0.0
        scene.scaling[7] = torch.log(torch.tensor([0.4, 12.0, 0.4]))
        scene.rotation[7] = torch.tensor([1.0, 0.0, 0.0, 0.0])
        scene.opacity[7] = 2.0
        notes["giant"] = 7
    elif name == "dense":
        # 128 near, large splats (consecutive depth ranks: whole workgroups of emit_pairs above EMIT_STAGE pairs) among 384 small ones
        scene, cam = _scene(512, 160, 128, seed=6, scale_mult=0.35)
        near = _towards_camera(cam, 1.4)
        idx = torch.arange(3, 512, 4)
        scene.xyz[idx] = near[None, :] + 0.12 * (torch.rand(idx.numel(), 3, generator=g) - 0.5)
        scene.scaling[idx] = math.log(0.1) + 0.3 * (torch.rand(idx.numel(), 3, generator=g) - 0.5)
        scene.opacity[idx] = 1.0 + torch.rand(idx.numel(), 1, generator=g)
        notes["near"] = idx.numpy()
    elif name == "ties":
        # 200 Gaussians with bit-identical means (so depths): the stable order by index, over more than one wave of ranks
        scene, cam = _scene(300, 96, 64, seed=7)
        scene.xyz[50:250] = scene.xyz[50].clone()
        notes["tied"] = np.arange(50, 250)
    elif name == "faint-culled":
        # opacity below 1 / 255 (no pair at all) and every third Gaussian behind the camera
        scene, cam = _scene(400, 96, 64, seed=8)
        scene.opacity[1::5] = -7.0
        scene.opacity[2::25] = -6.0
        behind = cam.camera_center.to(torch.float32) * 1.5
        scene.xyz[0::3] = behind[None, :] + 0.2 * (torch.rand(scene.xyz[0::3].shape, generator=g) - 0.5)
        notes["faint"] = np.concatenate([np.arange(1, 400, 5), np.arange(2, 400, 25)])
        notes["culled"] = np.arange(0, 400, 3)
    elif name == "slot-fallback":
        # 2^18 + 1 Gaussians leave jb = 13 bits for the pair index; Gaussian 11 covers all 2^13 sub-tiles of a 1024 x 512 image:
        # exactly 2^jb pairs, one too many to pack.  All but 40 of the others are behind the camera.
        n = (1 << 18) + 1
        scene, cam = _scene(n, 1024, 512, seed=9, scale_mult=6.0)
        keep = torch.zeros(n, dtype=torch.bool)
        keep[torch.arange(5, n, n // 40)] = True
        keep[11] = True
        behind = cam.camera_center.to(torch.float32) * 1.5
        scene.xyz[~keep] = behind
        scene.xyz[11] = 0.0
        scene.scaling[11] = math.log(30.0)
        scene.opacity[11] = 2.0
        notes["giant"], notes["kept"] = 11, np.flatnonzero(keep.numpy())
    elif name in OFF_EDGE:
        # small splats centred right of and below an image whose size is no multiple of 8: their rect still holds the last column /
        # row of sub-tiles, of which only 3 (1) pixel columns / rows exist -- a pair is required only when the splat reaches those
        w, h, n = OFF_EDGE[name]
        scene, cam = _scene(n, w, h, seed=10)
        k = n // 3
        pix = torch.empty(2 * k, 2)
        pix[:k, 0] = w - 0.5 + 12.0 * torch.rand(k, generator=g)          # right of the last pixel column
        pix[:k, 1] = -3.0 + (h + 14.0) * torch.rand(k, generator=g)       # (the last of them below the image too)
        pix[k:, 0] = -3.0 + (w + 6.0) * torch.rand(k, generator=g)
        pix[k:, 1] = h - 0.5 + 12.0 * torch.rand(k, generator=g)          # below the last pixel row
        depth = 3.0 + 2.0 * torch.rand(2 * k, generator=g)
        tanx, tany = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
        view = torch.stack([((2 * pix[:, 0] + 1) / w - 1) * tanx * depth, ((2 * pix[:, 1] + 1) / h - 1) * tany * depth, depth], 1)
        wvt = cam.world_view_transform.to(torch.float64)                   # row vectors: view = [p, 1] @ wvt
        scene.xyz[:2 * k] = ((view.to(torch.float64) - wvt[3, :3]) @ torch.linalg.inv(wvt[:3, :3])).to(torch.float32)
        sigma_px = 1.0 + 3.0 * torch.rand(2 * k, 1, generator=g)
        focal = w / (2 * tanx)
        scene.scaling[:2 * k] = torch.log(sigma_px * depth[:, None] / focal) + 0.4 * (torch.rand(2 * k, 3, generator=g) - 0.5)
        scene.opacity[:2 * k] = 1.0 + 2.0 * torch.rand(2 * k, 1, generator=g)
        notes["outside"] = np.arange(2 * k)
    else:
        raise KeyError(name)
    return scene, cam, notes


# name -> (W, H, P, seed): P = 1, 63 and 1025 (4 P is then no multiple of 256, and a rank crosses 1024) at the four image sizes
SMALL = {"96x64-P1025": (96, 64, 1025, 1), "96x64-P63": (96, 64, 63, 2), "67x35-P1025": (67, 35, 1025, 3), "67x35-P63": (67, 35, 63, 4),
         "9x9-P63": (9, 9, 63, 12), "9x9-P1": (9, 9, 1, 6), "8x8-P63": (8, 8, 63, 7), "8x8-P1": (8, 8, 1, 8)}
OFF_EDGE = {"off-edge-67x35": (67, 35, 300), "off-edge-9x9": (9, 9, 90)}      # name -> (W, H, P)
SCENES = list(SMALL) + ["giant", "dense", "ties", "faint-culled", "slot-fallback"] + list(OFF_EDGE)
STRIP_SCENES = ["96x64-P1025", "dense", "faint-culled"]      # also run under the tile-row strip (1, 4), with compaction


def oracle_geometry(scene, cam):
    """float32 roundings of the float64 oracle's per-Gaussian geometry (oracle/raster_oracle.py preprocess; oracle/cpu_preprocess.py
    restates the Python routes up to the projected centres and 3D covariances only, not the conics): xy, conic_opacity, radii,
    depth bits."""
    import torch
    from oracle import raster_oracle as ro
    from tests.util import settings_for
    act = scene.activated()
    d = lambda t: t.to(torch.float64)
    geo = ro.preprocess(settings_for(cam), d(act["means3D"]), d(act["shs"]), None, d(act["opacities"]), d(act["scales"]),
                        d(act["rotations"]), None)
    co = torch.cat([geo.conic, d(act["opacities"]).reshape(-1, 1)], dim=1)
    depth = geo.depth.to(torch.float32).numpy().view(np.uint32)
    return geo.xy.to(torch.float32).numpy(), co.to(torch.float32).numpy(), geo.radii.numpy().astype(np.int32), depth

