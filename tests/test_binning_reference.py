"""The numpy references of tests/binning_reference.py against brute force, and the scenes of tests/test_gpu_binning.py against
the conditions their tests rely on: the free pairs of the membership band stay below 2 % of the required ones, the host build of
gs_math.h (tests/hostsim) misses no required pair and keeps no forbidden one, and every scene reaches the path it was built for.
No GPU needed."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import binning_reference as BR


# ---- compaction, scan, order ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 2, 7, 300])
def test_compact_live_against_a_loop(P):
    rng = np.random.default_rng(P)
    for density in (0.0, 0.1, 0.9, 1.0):
        tiles = np.where(rng.random(P) < density, rng.integers(1, 50, size=P), 0).astype(np.uint32)
        keys = rng.integers(0, 1 << 32, size=P, dtype=np.uint64).astype(np.uint32)
        live, lkeys, dead = [], [], []
        for i in range(P):
            if tiles[i]:
                live.append(i)
                lkeys.append(int(keys[i]))
            else:
                dead.append(i)
        got = BR.compact_live(tiles, keys)
        assert got[0].tolist() == live and got[1].tolist() == lkeys and got[2].tolist() == dead and got[3] == len(live)


@pytest.mark.parametrize("P,n_live", [(1, 1), (1, 0), (5, 3), (1024, 1024), (1025, 1025), (2500, 2049), (2500, 0)])
def test_scan_tiles_against_a_loop(P, n_live):
    rng = np.random.default_rng(P + n_live)
    tiles = rng.integers(0, 9, size=P).astype(np.uint32)
    ids = rng.permutation(P).astype(np.uint32)
    incl, r_eff, mx = BR.scan_tiles(tiles, ids, n_live)
    run, want, big = 0, [], 0
    for r in range(n_live):
        run += int(tiles[ids[r]])
        big = max(big, int(tiles[ids[r]]))
        want.append(run)
    assert incl.tolist() == want and r_eff == run and mx == big
    local, excl = BR.scan_device_form(incl, P)
    assert excl.shape[0] == (P + 1023) // 1024
    for b in range(excl.shape[0]):                              # a block's exclusive prefix: the pairs of all ranks before it
        assert int(excl[b]) == (want[min(b * 1024, n_live) - 1] if b and n_live else 0)
    for r in range(n_live):
        assert int(local[r]) + int(excl[r // 1024]) == want[r]


def test_expected_order_is_the_stable_sort_by_bits_then_index():
    rng = np.random.default_rng(3)
    depth = rng.choice(np.array([0.5, 1.0, 1.0000001, 2.0, 77.0], dtype=np.float32), size=400)
    ids = rng.choice(400, size=250, replace=False)
    got = BR.expected_order(depth.view(np.uint32), ids)
    assert got.tolist() == sorted(ids.tolist(), key=lambda i: (int(depth.view(np.uint32)[i]), i))


# ---- the tile rect, against the host build of gs_math.h ------------------------------------------------------------------------------
def _rows_fn(hostsim):
    fn = hostsim.hs_subtile_rows
    fn.restype = C.c_int
    fn.argtypes = [C.c_float] * 6 + [C.c_int] * 3 + [C.POINTER(C.c_int)] * 2 + [C.POINTER(C.c_ubyte), C.c_int, C.POINTER(C.c_int)]
    return fn


def _host_membership(fn, xy, co, radii, i, W, H):
    """-> (row-rule live set, block-rule live set) of Gaussian i as bool (T,) arrays, through hs_subtile_rows' per-block mask"""
    gx8, gy8 = (W + 7) // 8, (H + 7) // 8
    rect = (C.c_int * 4)()
    ob, orow = C.c_int(), C.c_int()
    cap = 4 * ((W + 15) // 16) * ((H + 15) // 16)
    mask = (C.c_ubyte * cap)()
    fn(xy[i, 0], xy[i, 1], co[i, 0], co[i, 1], co[i, 2], co[i, 3], int(radii[i]), W, H, C.byref(ob), C.byref(orow), mask, cap, rect)
    rows, blocks = np.zeros((gy8 + 1, gx8 + 1), dtype=bool), np.zeros((gy8 + 1, gx8 + 1), dtype=bool)
    ncol, nrow = rect[2] - rect[0], rect[3] - rect[1]
    if ncol > 0 and nrow > 0:
        m = np.frombuffer(mask, dtype=np.uint8, count=ncol * nrow).reshape(nrow, ncol)
        y1, x1 = min(rect[3], gy8 + 1), min(rect[2], gx8 + 1)       # (a rect reaches at most one sub-tile past an odd-sized image)
        rows[rect[1]:y1, rect[0]:x1] = (m[:y1 - rect[1], :x1 - rect[0]] & 2) != 0
        blocks[rect[1]:y1, rect[0]:x1] = (m[:y1 - rect[1], :x1 - rect[0]] & 1) != 0
    assert not rows[gy8].any() and not rows[:, gx8].any(), "the host build lists a sub-tile outside the image"
    return rows[:gy8, :gx8].reshape(-1), blocks[:gy8, :gx8].reshape(-1), tuple(rect)


def test_tile_rect_and_area_against_the_host_build(hostsim):
    fn = _rows_fn(hostsim)
    rng = np.random.default_rng(5)
    W, H = 333, 205
    gx, gy = (W + 15) // 16, (H + 15) // 16
    n = 3000
    xy = np.stack([rng.uniform(-80, W + 80, n), rng.uniform(-80, H + 80, n)], 1).astype(np.float32)
    xy[:200] = np.round(xy[:200])                               # on the lattice: quotients at and next to integers
    xy[200:400] = (np.round(xy[200:400] / 16) * 16 + rng.choice([-1e-3, 0.0, 1e-3], size=(200, 2))).astype(np.float32)
    radii = rng.choice([1, 1, 2, 15, 16, 17, 100, 1000], size=n).astype(np.int32)
    x0, y0, x1, y1 = BR.tile_rect(xy, radii, gx, gy)
    co = np.tile(np.array([0.1, 0.0, 0.1, 0.5], dtype=np.float32), (n, 1))
    area = 0
    for i in range(n):
        rect = _host_membership(fn, xy, co, radii, i, W, H)[2]
        assert rect == (2 * x0[i], 2 * y0[i], 2 * x1[i], 2 * y1[i]), (i, xy[i], radii[i])
        area += (rect[2] - rect[0]) * (rect[3] - rect[1]) // 4
    assert BR.tile_rect_area(xy, radii, gx, gy) == area and area > 10000
    dead = radii.copy()
    dead[::2] = 0                                               # radius 0: no rect at all
    assert BR.tile_rect_area(xy, dead, gx, gy) == int(((x1 - x0) * (y1 - y0))[1::2].sum())


# ---- the band ----------------------------------------------------------------------------------------------------------------------
def _random_splats(rng, n, W, H):
    xy = np.stack([rng.uniform(-10, W + 10, n), rng.uniform(-10, H + 10, n)], 1).astype(np.float32)
    co, radii = np.zeros((n, 4), dtype=np.float32), np.zeros(n, dtype=np.int32)
    for i in range(n):
        s1, s2, th = rng.uniform(0.6, 9.0), rng.uniform(0.6, 9.0), rng.uniform(0, np.pi)
        R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        cov = R @ np.diag([s1 * s1, s2 * s2]) @ R.T
        con = np.linalg.inv(cov)
        co[i] = (con[0, 0], con[0, 1], con[1, 1], rng.choice([rng.uniform(0.001, 0.01), rng.uniform(0.01, 1.0)]))
        radii[i] = int(np.ceil(3.0 * max(s1, s2)))
    radii[::9] = 0
    return xy, co, radii


def test_box_minimum_against_dense_sampling():
    rng = np.random.default_rng(7)
    xy, co, _ = _random_splats(rng, 300, 64, 64)
    for i in range(300):
        A, B, Cc = (float(v) for v in co[i, :3])
        x_lo, y_lo = rng.uniform(-20, 15), rng.uniform(-20, 15)
        x_hi, y_hi = x_lo + rng.uniform(0, 8), y_lo + rng.uniform(0, 8)
        got = float(BR.box_min_form(A, B, Cc, x_lo, x_hi, y_lo, y_hi))
        xs, ys = np.linspace(x_lo, x_hi, 161)[None, :], np.linspace(y_lo, y_hi, 161)[:, None]
        if x_lo <= 0 <= x_hi and y_lo <= 0 <= y_hi:
            assert got == 0.0
            continue
        sampled = float((A * xs * xs + 2 * B * xs * ys + Cc * ys * ys).min())
        h = max(x_hi - x_lo, y_hi - y_lo) / 160                 # the sampled minimum lies within a grid step of the true one
        assert got <= sampled * (1 + 1e-12) and sampled - got <= 0.05 * sampled + (A + Cc) * h * h, (i, got, sampled)


@pytest.mark.parametrize("W,H,strip", [(67, 35, (0, 0)), (40, 70, (1, 3)), (9, 9, (0, 0))])
def test_membership_band_against_per_pair_loops(W, H, strip):
    rng = np.random.default_rng(W)
    n = 60
    xy, co, radii = _random_splats(rng, n, W, H)
    band = BR.membership_band(xy, co, radii, W, H, strip)
    sub = BR.membership_band(xy, co, radii, W, H, strip, sel=np.arange(5, 25))
    assert np.array_equal(sub, band[5:25])
    gx, gy, gx8, gy8 = (W + 15) // 16, (H + 15) // 16, (W + 7) // 8, (H + 7) // 8
    x0, y0, x1, y1 = BR.tile_rect(xy, np.maximum(radii, 1), gx, gy)
    sy_lo, sy_hi = (0, gy8) if strip == (0, 0) else (2 * strip[0], min(2 * strip[1], gy8))
    seen = set()
    for i in range(n):
        A, B, Cc, o = (float(v) for v in co[i])
        cx, cy = float(xy[i, 0]), float(xy[i, 1])
        for sy in range(gy8):
            for sx in range(gx8):
                inside = radii[i] > 0 and 2 * x0[i] <= sx < 2 * x1[i] and 2 * y0[i] <= sy < 2 * y1[i] and sy_lo <= sy < sy_hi
                want = BR.FORBIDDEN
                if inside and o >= 1 / 255:
                    tau = 2 * np.log(255 * o)
                    px = [x - cx for x in range(8 * sx, min(8 * sx + 8, W))]
                    py = [y - cy for y in range(8 * sy, min(8 * sy + 8, H))]
                    if any(A * dx * dx + 2 * B * dx * dy + Cc * dy * dy <= tau for dx in px for dy in py):
                        want = BR.REQUIRED
                    else:
                        xs = np.linspace(px[0] - BR.PAD_M, px[-1] + BR.PAD_M, 201)[None, :]
                        ys = np.linspace(py[0] - BR.PAD_M, py[-1] + BR.PAD_M, 201)[:, None]
                        qmin = float((A * xs * xs + 2 * B * xs * ys + Cc * ys * ys).min())
                        thi = float(BR.tau_hi(np.array([o]))[0])
                        if abs(qmin - thi) < 0.03 * thi:        # the sampling cannot decide: either answer but REQUIRED
                            assert band[i, sy * gx8 + sx] != BR.REQUIRED
                            continue
                        want = BR.FORBIDDEN if qmin > thi else BR.FREE
                assert band[i, sy * gx8 + sx] == want, (i, sx, sy, BR.describe_pair(i, sy * gx8 + sx, xy, co, radii, W, H))
                seen.add(want)
    assert {BR.REQUIRED, BR.FORBIDDEN} <= seen


# ---- the scenes -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene_geometry(name):
    scene, cam, notes = BR.build_scene(name)
    return (cam.image_width, cam.image_height, notes) + BR.oracle_geometry(scene, cam)


@pytest.mark.parametrize("name", BR.STRIP_SCENES)
def test_scene_band_share_under_the_strip(name):
    """The 2 % condition again for the scenes that also run under the tile-row strip (1, 4)."""
    W, H, notes, xy, co, radii, depth = _scene_geometry(name)
    sel = np.flatnonzero(radii > 0)
    full = BR.membership_band(xy, co, radii, W, H, sel=sel)
    band = BR.membership_band(xy, co, radii, W, H, strip=(1, 4), sel=sel)
    req, free = BR.band_counts(band)
    print(f"{name} under the strip (1, 4): required {req}, free {free} ({100.0 * free / max(req, 1):.2f} %)")
    assert 0 < req < BR.band_counts(full)[0] and free <= 0.02 * req
    gx8 = (W + 7) // 8
    rows = np.arange(band.shape[1]) // gx8
    inside = (rows >= 2) & (rows < 8)
    assert np.array_equal(band[:, inside], full[:, inside]) and np.all(band[:, ~inside] == BR.FORBIDDEN)


@pytest.mark.parametrize("name", BR.SCENES)
def test_scene_band_share_and_host_build_inside_the_band(name, hostsim):
    """Free pairs at most 2 % of the required ones (a property of the scene and the float64 band alone), and the host build's
    enumerations inside the band: the row rule the kernels count and emit with, block by block through hs_subtile_rows' mask;
    the block rule hs_subtile_enumerate counts, which reports no per-block answer, through its live count (at least the required
    pairs, at most required + free) and its mismatch word."""
    W, H, notes, xy, co, radii, depth = _scene_geometry(name)
    sel = np.flatnonzero(radii > 0)
    band = BR.membership_band(xy, co, radii, W, H, sel=sel)
    req, free = BR.band_counts(band)
    print(f"{name}: {sel.size} of {radii.size} Gaussians live, required {req}, free {free} ({100.0 * free / max(req, 1):.2f} %)")
    assert req > 0 and free <= 0.02 * req
    cond, far = BR.band_premises(xy, co, sel)
    assert cond < 1e3 and far < 2 ** 14, f"the margins' error analysis does not cover this scene: condition {cond:.0f}, centre {far:.0f} px"
    rows_fn = _rows_fn(hostsim)
    enum = hostsim.hs_subtile_enumerate
    enum.restype = C.c_int
    enum.argtypes = [C.c_float] * 6 + [C.c_int] * 3 + [C.POINTER(C.c_int)] * 3
    for k, i in enumerate(sel):
        rows, blocks, _ = _host_membership(rows_fn, xy, co, radii, i, W, H)
        for what, m in (("row rule", rows), ("block rule", blocks)):
            missed, kept = np.flatnonzero(~m & (band[k] == BR.REQUIRED)), np.flatnonzero(m & (band[k] == BR.FORBIDDEN))
            assert missed.size == 0, f"{what} misses a required pair: " + BR.describe_pair(i, missed[0], xy, co, radii, W, H)
            assert kept.size == 0, f"{what} keeps a forbidden pair: " + BR.describe_pair(i, kept[0], xy, co, radii, W, H)
        mm, nf, npr = C.c_int(), C.c_int(), C.c_int()
        live = enum(xy[i, 0], xy[i, 1], co[i, 0], co[i, 1], co[i, 2], co[i, 3], int(radii[i]), W, H, C.byref(mm), C.byref(nf), C.byref(npr))
        r_i, f_i = BR.band_counts(band[k])
        assert mm.value == 0 and live == int(blocks.sum()) and r_i <= live <= r_i + f_i, (i, live, r_i, f_i)


def test_scenes_reach_the_paths_they_were_built_for():
    def pairs(name):
        W, H, notes, xy, co, radii, depth = _scene_geometry(name)
        sel = np.flatnonzero(radii > 0)
        band = BR.membership_band(xy, co, radii, W, H, sel=sel)
        return W, H, notes, sel, band, depth, radii
    # giant: more than EMIT_BIG required pairs, in more than 64 sub-tile rows
    W, H, notes, sel, band, _, _ = pairs("giant")
    assert H >= 544
    g = band[list(sel).index(notes["giant"])] == BR.REQUIRED
    assert g.sum() > BR.EMIT_BIG and g.reshape((H + 7) // 8, -1).any(axis=1).sum() > 64
    # dense: some workgroup of emit_pairs (64 consecutive depth ranks) owns more than EMIT_STAGE pairs, another few enough to stage
    W, H, notes, sel, band, depth, _ = pairs("dense")
    order = BR.expected_order(depth, sel)
    row = {int(i): k for k, i in enumerate(sel)}
    need = np.array([(band[row[int(i)]] == BR.REQUIRED).sum() for i in order])
    most = np.array([(band[row[int(i)]] != BR.FORBIDDEN).sum() for i in order])
    groups = range(0, len(order), 64)
    assert any(need[a:a + 64].sum() > BR.EMIT_STAGE for a in groups) and any(0 < most[a:a + 64].sum() <= BR.EMIT_STAGE for a in groups)
    # ties: 200 live Gaussians with one depth, more than a wave of consecutive ranks
    W, H, notes, sel, band, depth, radii = pairs("ties")
    assert len(set(depth[notes["tied"]].tolist())) == 1 and (radii[notes["tied"]] > 0).all() and len(notes["tied"]) == 200
    # faint-culled: neither kind has a pair; live ones sit between them
    W, H, notes, sel, band, depth, radii = pairs("faint-culled")
    assert (radii[notes["culled"]] == 0).all()
    faint = [list(sel).index(i) for i in notes["faint"] if radii[i] > 0]
    assert len(faint) > 30 and (band[faint] == BR.FORBIDDEN).all()
    # slot-fallback: the giant needs every sub-tile: 2^13 pairs with 13 bits left beside 2^18 + 1 ids
    W, H, notes, sel, band, depth, radii = pairs("slot-fallback")
    assert radii.size == (1 << 18) + 1 and (band[list(sel).index(notes["giant"])] == BR.REQUIRED).sum() == 1 << 13 == band.shape[1]


@pytest.mark.parametrize("name", list(BR.OFF_EDGE))
def test_off_edge_scenes_hold_the_clipped_column_case(name, hostsim):
    """Live splats centred right of the last pixel column and below the last pixel row of an image whose size is no multiple of 8;
    among them some whose rect holds the last column (row) of sub-tiles while the splat ends among the pixels that do not exist:
    forbidden pairs that the row rule of gs_math.h used to list (it tested the unclipped block 8 sx .. 8 sx + 7)."""
    W, H, notes, xy, co, radii, depth = _scene_geometry(name)
    assert W % 8 and H % 8
    gx8, gy8 = (W + 7) // 8, (H + 7) // 8
    out = notes["outside"][radii[notes["outside"]] > 0]
    right, below = out[xy[out, 0] > W - 1], out[xy[out, 1] > H - 1]
    assert right.size >= 10 and below.size >= 10
    x0, y0, x1, y1 = BR.tile_rect(xy, np.maximum(radii, 1), (W + 15) // 16, (H + 15) // 16)
    fn = _rows_fn(hostsim)
    for ids, last, axis in ((right, gx8 - 1, 1), (below, gy8 - 1, 0)):
        band = BR.membership_band(xy, co, radii, W, H, sel=ids).reshape(ids.size, gy8, gx8)
        edge = band[:, :, last] if axis else band[:, last, :]
        in_rect = (2 * x1[ids] > last) if axis else (2 * y1[ids] > last)
        idle = in_rect & ~(edge == BR.REQUIRED).any(axis=1)       # the rect reaches the last column / row, no pixel of it is reached
        reached = in_rect & (edge == BR.REQUIRED).any(axis=1)
        assert idle.sum() >= 3 and reached.sum() >= 3, (name, axis, int(idle.sum()), int(reached.sum()))
        for k in np.flatnonzero(idle):
            rows, blocks, _ = _host_membership(fn, xy, co, radii, int(ids[k]), W, H)
            listed = rows.reshape(gy8, gx8)
            kept = listed[:, last] if axis else listed[last, :]
            forb = (edge[k] == BR.FORBIDDEN)
            assert not (kept & forb).any(), BR.describe_pair(int(ids[k]), int(np.flatnonzero((listed & (band[k] == BR.FORBIDDEN)).reshape(-1))[0]), xy, co, radii, W, H)
