"""The stages of trase_amd/csrc/binning.hip between the depth sort and the pair sort, and the finished sub-tile lists, against
tests/binning_reference.py.  Integer algorithms: every comparison is array_equal, except which borderline sub-tiles a splat
reaches, which is held inside the float64 membership band of that module (required pairs listed, forbidden pairs not).

Scan and compaction run through their test entry points (trase_selftest_compact_live / _scan_tiles: the library's own workspace
layout, filled with 0xCD, so that a word no kernel wrote is seen).  The finished lists come from real forwards -- the cooked
entry and the fused render() -- on the scenes of binning_reference.build_scene, read back with rasterizer.last_sub_tile_lists
together with the device's own geometry, and must satisfy, exactly:
  1 the ranges partition [0, R_eff) in sub-tile row-major order and the sentinel ("trash") list is empty
  2 no id twice in a list                       3 every list ascending in depth rank (stable by Gaussian index)
  4 per Gaussian, lists holding it == tiles[id], the sum == HDR_R_EFF
  5 the packed pair indices of a Gaussian are a permutation of 0 .. tiles[id] - 1
  6 (band) every required pair listed, no forbidden pair listed; free pairs <= 2 % of the required ones
  7 packed lists (staged and direct workgroups of emit_pairs) and slot lists (all direct) hold the same ids
  8 under a tile-row strip the lists are the full image's, restricted to the strip's sub-tile rows
and under a capacity below R_eff: the flag, every range end <= capacity, sub-sequences of the full lists, exactly `capacity`
entries, and one depth rank below which every Gaussian keeps all its pairs and above which none keeps any.

Not covered here: PairBuf::pair_gauss, the id emit_pairs writes beside every slot of a slot list.  last_sub_tile_lists takes a slot
list's ids from slot ownership (the forward fills the id array only as far as it walks a list), so a wrong id in pair_gauss does
not show in check 7; the bit-identity of packed and slot renders in tests/test_gpu_list_values.py is what holds it."""
import functools

import numpy as np
import pytest
import torch

from tests import binning_reference as BR

pytestmark = pytest.mark.gpu

POISON = 0xCDCDCDCD
SLOT_LISTS = 0x100000
SIZES = [1, 3, 1023, 1024, 1025, 4095, 4097, 262144, 262145]      # 262 145: 257 scan blocks, the carry loop of scan_sums_kernel
FAMILIES = ["mostly-zero", "dense-small", "one-giant", "all-zero"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _first_diff(got, want):
    bad = np.flatnonzero(got != want)
    return "equal" if bad.size == 0 else f"{bad.size} words differ, first at {int(bad[0])}: got {int(got[bad[0]])} want {int(want[bad[0]])}"


def _tiles(family, P, rng):
    if family == "mostly-zero":
        return np.where(rng.random(P) < 0.03, rng.integers(1, 400, size=P), 0).astype(np.uint32)
    if family == "dense-small":
        return rng.integers(1, 5, size=P).astype(np.uint32)
    if family == "one-giant":
        t = rng.integers(0, 3, size=P).astype(np.uint32)
        t[rng.integers(0, P)] = 3_000_000
        return t
    return np.zeros(P, dtype=np.uint32)


# ---- compaction -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", SIZES)
def test_compact_live_equals_reference(P):
    from trase_amd.rasterizer import selftest_compact_live
    for fi, family in enumerate(FAMILIES + ["all-live"]):
        rng = np.random.default_rng(1000 * P + fi)
        tiles = _tiles(family, P, rng) if family != "all-live" else np.full(P, 7, dtype=np.uint32)
        keys = rng.integers(0, 1 << 32, size=P, dtype=np.uint64).astype(np.uint32)
        live, lkeys, dead, n = BR.compact_live(tiles, keys)
        ko, io, lo, hdr = selftest_compact_live(_dev(tiles), _dev(keys))
        ko, io, lo = _host(ko), _host(io), _host(lo)
        tag = f"{family} P={P} live={n}"
        assert hdr["length"] == n, f"{tag}: length word {hdr['length']}"
        assert np.array_equal(ko[:n], lkeys), f"{tag}: keys of the live ids: {_first_diff(ko[:n], lkeys)}"
        assert np.array_equal(lo[:n], live), f"{tag}: live_ids: {_first_diff(lo[:n], live)}"
        assert np.array_equal(io[:n], live), f"{tag}: live head of ids_out: {_first_diff(io[:n], live)}"
        assert np.array_equal(io[n:], dead), f"{tag}: dead tail of ids_out: {_first_diff(io[n:], dead)}"
        assert np.all(ko[n:] == POISON) and np.all(lo[n:] == POISON), f"{tag}: a word behind the live count was written"
        assert (hdr["R"], hdr["overflow"], hdr["R_eff"], hdr["pack"]) == (POISON,) * 4, f"{tag}: the compaction touched another header word"


# ---- scan ---------------------------------------------------------------------------------------------------------------------------
GX, GY = 20, 12                 # 16x16 tiles of a 320 x 192 image


def _geometry(P, rng):
    """centres on, beside and far off the image; radii 0, 1 and large"""
    xy = np.stack([rng.uniform(-400, 720, P), rng.uniform(-300, 500, P)], 1).astype(np.float32)
    xy[::5] = np.round(xy[::5])
    radii = rng.choice([0, 1, 1, 9, 40, 1000], size=P).astype(np.int32)
    return xy, radii


def _scan_case(tiles, ids, n_live, xy, radii, cap=0xffffffff, pack_bits=0, overflow_in=0, tag=""):
    from trase_amd.rasterizer import selftest_scan_tiles
    P = tiles.shape[0]
    off, sums, hdr = selftest_scan_tiles(_dev(tiles), _dev(ids), torch.from_numpy(radii).cuda(), torch.from_numpy(xy).cuda(), n_live, cap,
                                         pack_bits, GX, GY, overflow_in)
    off, sums = _host(off), _host(sums)
    n = min(n_live, P)
    incl, r_eff, mx = BR.scan_tiles(tiles, ids, n)
    local, excl = BR.scan_device_form(incl, P)
    tag = f"{tag} P={P} n_live={n_live}"
    assert np.array_equal(off[:n].astype(np.uint64) + sums[np.arange(n) // BR.SC_TILE], incl), \
        f"{tag}: offsets[r] + block_sums[r // 1024]: {_first_diff(off[:n].astype(np.uint64) + sums[np.arange(n) // BR.SC_TILE], incl)}"
    assert np.array_equal(off[:n], local), f"{tag}: block-local offsets: {_first_diff(off[:n], local)}"
    assert np.array_equal(sums, excl), f"{tag}: block prefixes: {_first_diff(sums, excl)}"
    assert np.all(off[n:] == POISON), f"{tag}: an offset behind the live ranks was written"
    assert hdr["R_eff"] == r_eff, f"{tag}: HDR_R_EFF {hdr['R_eff']} want {r_eff}"
    assert hdr["R"] == BR.tile_rect_area(xy, radii, GX, GY), f"{tag}: HDR_R {hdr['R']} want {BR.tile_rect_area(xy, radii, GX, GY)}"
    assert hdr["overflow"] == (overflow_in & 2) | (1 if r_eff > cap else 0), f"{tag}: overflow word {hdr['overflow']} (R_eff {r_eff}, cap {cap}, before {overflow_in})"
    assert hdr["pack"] == (pack_bits if pack_bits > 0 and mx < (1 << pack_bits) else 0), f"{tag}: HDR_PACK {hdr['pack']} (largest count {mx}, pack_bits {pack_bits})"
    assert hdr["length"] == n_live, f"{tag}: the scan changed the length word"
    return r_eff


@pytest.mark.parametrize("P", SIZES)
def test_scan_tiles_equals_reference(P):
    for fi, family in enumerate(FAMILIES):
        rng = np.random.default_rng(77 * P + fi)
        tiles = _tiles(family, P, rng)
        ids = rng.permutation(P).astype(np.uint32)
        xy, radii = _geometry(P, rng)
        for n_live in sorted({P, P - 1, 1, 0}):
            _scan_case(tiles, ids, n_live, xy, radii, pack_bits=(0, 12, 22, 31)[fi], tag=family)


@pytest.mark.parametrize("P", [3, 1025, 4097])
def test_overflow_bit_at_the_capacity(P):
    """Bit 0 exactly when R_eff > cap, with cap = R - 1, R and R + 1; bit 1 (the depth sort's saturated key) survives, a stale bit 0 does not."""
    rng = np.random.default_rng(P)
    tiles = rng.integers(1, 6, size=P).astype(np.uint32)
    ids = rng.permutation(P).astype(np.uint32)
    xy, radii = _geometry(P, rng)
    R = int(tiles.sum())
    for cap in (R - 1, R, R + 1):
        for before in (0, 1, 2, 3):
            assert _scan_case(tiles, ids, P, xy, radii, cap=cap, overflow_in=before, tag=f"cap={cap} before={before}") == R


@pytest.mark.parametrize("jb", [1, 11, 13, 31])
def test_pack_word_at_two_to_the_jb(jb):
    """HDR_PACK = jb while the largest count is 2^jb - 1, 0 at 2^jb, 0 with pack_bits 0 -- wherever the largest count sits: the
    first and the last rank, either side of a block and a wave boundary, a rank the live count just includes or just leaves out."""
    P = 4097
    rng = np.random.default_rng(jb)
    ids = rng.permutation(P).astype(np.uint32)
    xy, radii = _geometry(P, rng)
    for rank in (0, 63, 64, 1023, 1024, 4095, 4096):
        for big, bits in ((2 ** jb - 1, jb), (2 ** jb, jb), (2 ** jb, 0), (2 ** jb - 1, 0)):
            tiles = np.zeros(P, dtype=np.uint32) if big > 1000 else rng.integers(0, min(big, 3), size=P).astype(np.uint32)
            tiles[ids[rank]] = big
            _scan_case(tiles, ids, P, xy, radii, pack_bits=bits, tag=f"largest {big} at rank {rank}")
    tiles = np.zeros(P, dtype=np.uint32)
    tiles[ids[4096]] = 2 ** jb                                  # just outside the live ranks: does not count
    _scan_case(tiles, ids, P - 1, xy, radii, pack_bits=jb, tag="largest behind the live ranks")


# ---- finished lists ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _scene(name):
    scene, cam, notes = BR.build_scene(name)
    dev = torch.device("cuda", 0)
    return scene.to(dev), cam.to(dev), notes


def _forward(name, entry, strip=(0, 0), variant=0):
    """One forward of the scene -> the lists and the device's own geometry, as numpy"""
    from trase_amd import rasterizer as R
    scene, cam, notes = _scene(name)
    P = scene.xyz.shape[0]
    R.set_variant(variant)
    try:
        with R.tile_rows(*strip):
            if entry == "cooked":
                from diff_gaussian_rasterization import GaussianRasterizer
                from tests.util import settings_for
                act = scene.activated()
                out = GaussianRasterizer(settings_for(cam, device=scene.xyz.device))(
                    means3D=act["means3D"], means2D=torch.zeros_like(act["means3D"]), shs=act["shs"], sh_objs=act["sh_objs"],
                    opacities=act["opacities"], scales=act["scales"], rotations=act["rotations"])
                radii = out[1]
            else:
                from gaussian_renderer import render
                from trase_amd.synthetic import SynthGaussianModel, SynthPipe
                out = render(cam, SynthGaussianModel(scene), SynthPipe(), torch.zeros(3, device=scene.xyz.device), 0.0, 0.0, 0.0)
                radii = out["radii"]
        L = R.last_sub_tile_lists(P)
        gv = R.last_geom_view(P)
        geo = {"xy": gv["xy"].cpu().numpy(), "co": gv["conic_opacity"].cpu().numpy(), "tiles": gv["tiles"].cpu().numpy().astype(np.int64),
               "depth": gv["rgb_depth"][:, 3].contiguous().cpu().numpy().view(np.uint32), "radii": radii.cpu().numpy().astype(np.int64)}
    finally:
        R.set_variant(0)
    return {"ranges": L["ranges"].numpy(), "ids": L["ids"].numpy(), "index": None if L["index"] is None else L["index"].numpy(),
            "hdr": L["header"], "geo": geo, "P": P, "W": cam.image_width, "H": cam.image_height, "notes": notes, "strip": strip, "entry": entry}


def _tile_of_position(r, n):
    """Check 1 -> the sub-tile of every list position"""
    ranges, T = r["ranges"], r["ranges"].shape[0] - 1
    geo = r["geo"]
    trash = ranges[T]
    if trash[1] != trash[0]:
        ids = r["ids"][trash[0]:trash[1]]
        recs = "; ".join(f"id {int(i)}: centre {geo['xy'][i].tolist()} conic/opacity {geo['co'][i].tolist()} radius {int(geo['radii'][i])} "
                         f"tiles {int(geo['tiles'][i])}" for i in ids[:4])
        raise AssertionError(f"the sentinel list holds {int(trash[1] - trash[0])} pairs: emit found fewer live sub-tiles than preprocess counted: {recs}")
    assert tuple(trash) == (0, 0)
    start, end = ranges[:T, 0], ranges[:T, 1]
    counts = end - start
    assert np.all(counts >= 0)
    want_start = np.cumsum(counts) - counts
    full = counts > 0
    assert np.array_equal(start[full], want_start[full]), f"ranges are not consecutive in sub-tile order: {_first_diff(start[full], want_start[full])}"
    assert np.all(start[~full] == 0) and np.all(end[~full] == 0), "an empty sub-tile's range is not (0, 0)"
    assert int(counts.sum()) == n, f"the ranges hold {int(counts.sum())} entries, the lists {n}"
    return np.repeat(np.arange(T), counts)


def _rank_of(r):
    geo = r["geo"]
    live = np.flatnonzero(geo["radii"] > 0)
    order = BR.expected_order(geo["depth"], live)
    rank = np.full(r["P"], -1, dtype=np.int64)
    rank[order] = np.arange(order.size)
    return rank, order


def _check_lists(r, band=True):
    """Checks 1-6 on one forward that did not overflow; returns (sub-tile of every position, listed (P_live, T) matrix or None)"""
    hdr, geo, P, W, H = r["hdr"], r["geo"], r["P"], r["W"], r["H"]
    ids, tiles = r["ids"], geo["tiles"]
    assert hdr["overflow"] == 0 and hdr["R_eff"] <= hdr["capacity"] and ids.shape[0] == hdr["R_eff"]
    tile_of = _tile_of_position(r, ids.shape[0])                                                    # 1
    assert np.all(ids < P) and np.all(geo["radii"][ids] > 0), "a culled or out-of-range id is listed"
    key = tile_of * P + ids
    assert np.unique(key).size == key.size, "an id appears twice in one list"                       # 2
    rank, order = _rank_of(r)
    same = np.diff(tile_of) == 0
    bad = np.flatnonzero(same & (np.diff(rank[ids]) <= 0))
    if bad.size:                                                                                    # 3
        p = int(bad[0]) + 1
        t = int(tile_of[p])
        first = int(r["ranges"][t, 0])
        want = np.sort(rank[ids[first:int(r["ranges"][t, 1])]])
        raise AssertionError(f"sub-tile {t}, position {p - first}: id {int(ids[p])}, expected {int(order[want[p - first]])} "
                             f"(depth bits {int(geo['depth'][ids[p]]):#x} after {int(geo['depth'][ids[p - 1]]):#x} of id {int(ids[p - 1])})")
    per_id = np.bincount(ids, minlength=P)
    assert np.array_equal(per_id, tiles), f"lists holding a Gaussian != tiles[id]: {_first_diff(per_id, tiles)}"      # 4
    assert int(tiles.sum()) == hdr["R_eff"]
    jb = hdr["pack"]
    if jb:                                                                                          # 5
        assert int(tiles.max(initial=0)) < (1 << jb)
        o = np.lexsort((r["index"], ids))
        first_of = np.cumsum(tiles) - tiles
        want = np.arange(ids.shape[0]) - first_of[ids[o]]
        assert np.array_equal(r["index"][o], want), f"packed pair indices are no permutation of 0 .. tiles - 1: {_first_diff(r['index'][o], want)}"
    else:
        assert r["index"] is None
    if r["strip"] != (0, 0):
        assert hdr["length"] == int((tiles > 0).sum()), "the length word is not the number of Gaussians with a pair in the strip"
    else:
        assert hdr["length"] == P
    if not band:
        return tile_of
    sel = geo["radii"] > 0                                                                          # 6
    if r["entry"] == "fused" and r["strip"] != (0, 0):
        # the fused preprocess writes no conic for a Gaussian without a pair in the strip: those are held to the band by the full
        # image's lists, which check 8 compares the strip's with
        sel &= tiles > 0
    sel = np.flatnonzero(sel)
    B = BR.membership_band(geo["xy"], geo["co"], geo["radii"], W, H, r["strip"], sel=sel)
    row = np.full(P, -1, dtype=np.int64)
    row[sel] = np.arange(sel.size)
    listed = np.zeros(B.shape, dtype=bool)
    listed[row[ids], tile_of] = True
    req, free = BR.band_counts(B)
    print(f"required {req}, free {free} ({100.0 * free / max(req, 1):.2f} %), listed {ids.shape[0]}, pack {jb}, lineage count {hdr['R']}")
    for what, wrong in (("a required pair is not listed", ~listed & (B == BR.REQUIRED)), ("a forbidden pair is listed", listed & (B == BR.FORBIDDEN))):
        k, t = np.nonzero(wrong)
        assert k.size == 0, f"{what} ({k.size} in all): " + BR.describe_pair(int(sel[k[0]]), int(t[0]), geo["xy"], geo["co"], geo["radii"], W, H)
    cond, far = BR.band_premises(geo["xy"], geo["co"], sel)
    assert cond < 1e3 and far < 2 ** 14, f"the margins' error analysis does not cover this scene: condition {cond:.0f}, centre {far:.0f} px"
    assert free <= 0.02 * req, f"free pairs {free} exceed 2 % of the required {req}: the scene does not pin the lists down"
    assert hdr["R"] == BR.tile_rect_area(geo["xy"], geo["radii"], (W + 15) // 16, (H + 15) // 16)
    return tile_of


def _expected_pack_bits(P):
    lg = 0
    while (1 << lg) < P:
        lg += 1
    return 31 if lg < 1 else 32 - lg


@pytest.mark.parametrize("entry", ["cooked", "fused"])
@pytest.mark.parametrize("name", BR.SCENES)
def test_finished_lists(name, entry):
    r = _forward(name, entry)
    tile_of = _check_lists(r)
    tiles, notes = r["geo"]["tiles"], r["notes"]
    if name == "slot-fallback":          # exactly 2^jb pairs: one too many for the packed form
        assert tiles[notes["giant"]] == 1 << 13 == 1 << _expected_pack_bits(r["P"]) and r["hdr"]["pack"] == 0
    else:
        assert r["hdr"]["pack"] == _expected_pack_bits(r["P"])
    if name == "giant":                  # the whole-wave path of emit_pairs, and its second trip
        rows = np.unique(tile_of[r["ids"] == notes["giant"]] // ((r["W"] + 7) // 8))
        assert tiles[notes["giant"]] > BR.EMIT_BIG and rows.size > 64
    if name == "dense":                  # staged and direct workgroups of emit_pairs in one launch
        _, order = _rank_of(r)
        # the device's ranks: a Gaussian without a pair gets the dead depth key from the preprocess kernels (`(vis && live) ? key :
        # dead`), in a whole-image forward as under a strip, and so sorts behind every Gaussian that has one
        order = order[tiles[order] > 0]
        per_group = np.add.reduceat(tiles[order], np.arange(0, order.size, 64))
        assert (per_group > BR.EMIT_STAGE).any() and ((per_group > 0) & (per_group <= BR.EMIT_STAGE)).any(), per_group
    if name in BR.OFF_EDGE:              # live splats centred right of and below the image, some with a pair in the last column / row, some without
        out = notes["outside"][r["geo"]["radii"][notes["outside"]] > 0]
        xy = r["geo"]["xy"]
        right, below = out[xy[out, 0] > r["W"] - 1], out[xy[out, 1] > r["H"] - 1]
        for ids in (right, below):
            assert ids.size >= 10 and (tiles[ids] > 0).sum() >= 3 and (tiles[ids] == 0).sum() >= 3, (ids.size, tiles[ids])
    if name == "ties":
        assert len(set(r["geo"]["depth"][notes["tied"]].tolist())) == 1 and (tiles[notes["tied"]] > 0).sum() > 64
    if name == "faint-culled":
        assert (tiles[notes["faint"]] == 0).all() and (r["geo"]["radii"][notes["culled"]] == 0).all() and (tiles > 0).sum() > 100
    # 7: slot lists (every workgroup of emit_pairs writes directly) hold the same ids in the same places
    s = _forward(name, entry, variant=SLOT_LISTS)
    assert s["hdr"]["pack"] == 0 and s["index"] is None and s["hdr"]["R_eff"] == r["hdr"]["R_eff"]
    assert np.array_equal(s["ranges"], r["ranges"]), f"slot lists: ranges differ: {_first_diff(s['ranges'].ravel(), r['ranges'].ravel())}"
    assert np.array_equal(s["ids"], r["ids"]), f"slot lists: ids differ: {_first_diff(s['ids'], r['ids'])}"


@pytest.mark.parametrize("entry", ["cooked", "fused"])
@pytest.mark.parametrize("name", BR.STRIP_SCENES)
def test_lists_under_a_tile_row_strip(name, entry):
    """8: tile rows (1, 4), compaction of the live Gaussians included: the full image's lists, restricted to the strip's sub-tile rows."""
    full = _forward(name, entry)
    strip = _forward(name, entry, strip=(1, 4))
    tile_full = _check_lists(full, band=False)
    tile_strip = _check_lists(strip)
    gx8, gy8 = (full["W"] + 7) // 8, (full["H"] + 7) // 8
    lo, hi = 2 * 1 * gx8, min(2 * 4, gy8) * gx8                 # sub-tiles of the strip
    inside = (tile_full >= lo) & (tile_full < hi)
    assert inside.any() and not inside.all()
    assert np.array_equal(tile_strip, tile_full[inside]) and np.array_equal(strip["ids"], full["ids"][inside]), "strip lists differ from the full image's"
    assert strip["hdr"]["length"] < full["hdr"]["length"]


@pytest.mark.parametrize("name,entry", [("96x64-P1025", "cooked"), ("dense", "cooked"), ("giant", "fused")])
def test_lists_when_the_capacity_runs_out(name, entry):
    from trase_amd import rasterizer as R
    full = _forward(name, entry)
    tile_full = _check_lists(full, band=False)
    P, tiles, r_eff = full["P"], full["geo"]["tiles"], full["hdr"]["R_eff"]
    rank, order = _rank_of(full)
    full_keys = tile_full * P + full["ids"]
    for cap in (r_eff - 1, r_eff // 2):
        before = (R._Policy.sync, R._Policy.capacity)
        try:
            R.set_sync(False, capacity=cap)
            o = _forward(name, entry)
        finally:
            R.set_sync(*before)
        hdr, ids = o["hdr"], o["ids"]
        assert hdr["overflow"] & 1 and hdr["R_eff"] == r_eff and hdr["capacity"] == cap
        assert np.array_equal(o["geo"]["tiles"], tiles)
        assert int(o["ranges"].max()) <= cap and ids.shape[0] == cap
        tile_of = _tile_of_position(o, cap)                     # the total is exactly the capacity
        assert np.all(np.isin(tile_of * P + ids, full_keys)), "a pair that the full lists do not hold"
        same = np.diff(tile_of) == 0
        assert np.all(np.diff(rank[ids])[same] > 0), "a list is no sub-sequence of the full list"
        kept = np.bincount(ids, minlength=P)[order]            # per depth rank
        want = tiles[order]
        short = np.flatnonzero(kept < want)
        assert short.size > 0
        r_star = int(short[0])
        assert np.array_equal(kept[:r_star], want[:r_star]) and np.all(kept[r_star + 1:] == 0), \
            f"capacity {cap}: no single depth rank splits kept from dropped (first short rank {r_star})"
        assert int(want[:r_star].sum()) + int(kept[r_star]) == cap
