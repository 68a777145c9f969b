"""The FEATURE-state head on bit-packed SAM masks against the same head on bool masks: 100 masks at 540x960 and 1080x1920.

HIP events around every call, medians of 30 after a pre-roll; the bool and the bit path ALTERNATE inside one process (call by
call), so both see the same clocks and the same neighbours.  Per size:

    mask_stats           bool (N HW bytes) against bits (N HW / 8 bytes), with the bytes per second the bit kernel achieves
                         against what it has to move, N HW / 8 read + 4 HW written
    head                 contrastive_head forward + backward (soft, weights, norm regulariser; ~5000 pixels, ~50 masks)
    pack / unpack        bool bytes <-> stream on the device
    host                 PackedMasks.from_saved + upload against the reference's np.array(list of N HW bools) (train.py:245-249's
                         np.array(bitarray.tolist()); building the list itself is not timed) + upload of the bool array

    python profiles/bench_mask_bits.py [--out profiles/mask_bits_bench.json] [--bench-this FILE --bench-parent FILE]

--bench-this / --bench-parent: files holding the JSON lines bench.py printed on this tree and on its parent commit (same machine,
runs taking turns); they are copied into the result as they are.  Prints the result as one JSON line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trase_amd.feature_head import PackedMasks, contrastive_head, get_sample_pixel_and_mask, mask_stats  # noqa: E402

REPS, PREROLL = 30, 5


def alternate(fns, reps=REPS, preroll=PREROLL):
    """median ms of each callable, HIP events, the callables taking turns"""
    for _ in range(preroll):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: round(statistics.median(v), 4) for k, v in times.items()}, {k: round(max(v) - min(v), 4) for k, v in times.items()}


def scene(N, H, W):
    g = torch.Generator().manual_seed(H)
    sam = torch.zeros(N, H, W, dtype=torch.bool, device="cuda")
    for n in range(N):
        h, w = int(torch.randint(H // 27, H // 2, (1,), generator=g)), int(torch.randint(W // 48, W // 3, (1,), generator=g))
        y0, x0 = int(torch.randint(0, H - h, (1,), generator=g)), int(torch.randint(0, W - w, (1,), generator=g))
        sam[n, y0:y0 + h, x0:x0 + w] = True
    return sam


def one_size(N, H, W):
    HW = H * W
    sam = scene(N, H, W)
    packed = PackedMasks.from_bool(sam)
    assert torch.equal(packed.to_bool(), sam)
    cb, sb = mask_stats(sam)
    cp, sp_ = mask_stats(packed)
    assert torch.equal(cb, cp) and torch.equal(sb, sp_)
    out = {"N": N, "H": H, "W": W, "bool_bytes": N * HW, "stream_bytes": int(packed.bits.numel())}

    med, spread = alternate({"bool": lambda: mask_stats(sam), "bits": lambda: mask_stats(packed)})
    moved = N * HW / 8 + 4 * HW
    out["mask_stats_ms"] = med
    out["mask_stats_spread_ms"] = spread
    out["mask_stats_bits_bytes_moved"] = int(moved)
    out["mask_stats_bits_GBps"] = round(moved / (med["bits"] * 1e-3) / 1e9, 1)
    out["mask_stats_bool_GBps"] = round((N * HW + 4 * HW) / (med["bool"] * 1e-3) / 1e9, 1)

    torch.manual_seed(0)
    feat = torch.randn(32, H, W, device="cuda", requires_grad=True)
    pix, msk = get_sample_pixel_and_mask(packed, 5000, 50, cover_count=cp, rng="cuda")
    out["S"], out["sampled_masks"] = int(pix.sum()), int(msk.sum())

    def head(masks):
        feat.grad = None
        lp, ln, _, _, reg = contrastive_head(feat, masks, pix, msk, "soft", 0.75, 0.5, mask_size=sb, with_norm_reg=True)
        (lp + ln + reg).backward()
    med, spread = alternate({"bool": lambda: head(sam), "bits": lambda: head(packed)})
    out["head_fwd_bwd_ms"], out["head_fwd_bwd_spread_ms"] = med, spread

    med, spread = alternate({"pack": lambda: PackedMasks.from_bool(sam), "unpack": packed.to_bool})
    out["pack_unpack_ms"], out["pack_unpack_spread_ms"] = med, spread

    # the host side of train.py:245-249, once per FEATURE iteration there
    saved = {"masks": packed.bits.cpu().numpy()[:(N * HW + 7) // 8].tobytes(), "N": N, "H": H, "W": W}
    as_list = sam.reshape(-1).cpu().numpy().tolist()
    host = {"from_saved_upload": [], "np_array_of_list_upload": []}
    out["host_reps"] = 3 if N * HW < 100_000_000 else 1          # (a list of 2e8 bools takes ten seconds to convert)
    for _ in range(out["host_reps"]):
        torch.cuda.synchronize(); t = time.perf_counter()
        PackedMasks.from_saved(saved, "cuda")
        torch.cuda.synchronize(); host["from_saved_upload"].append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        torch.from_numpy(np.array(as_list)).reshape(N, H, W).cuda()
        torch.cuda.synchronize(); host["np_array_of_list_upload"].append((time.perf_counter() - t) * 1e3)
    out["host_ms"] = {k: round(statistics.median(v), 3) for k, v in host.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_bits_bench.json"))
    ap.add_argument("--bench-this", default="")
    ap.add_argument("--bench-parent", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mask_bits.py measures on the GPU; none is present")
    res = {"device": torch.cuda.get_device_name(0), "reps": REPS, "preroll": PREROLL,
           "sizes": [one_size(100, 540, 960), one_size(100, 1080, 1920)]}
    for key, path in (("bench_py_this_tree", a.bench_this), ("bench_py_parent", a.bench_parent)):
        if path:
            lines = [ln for ln in open(path).read().splitlines() if ln.startswith("{")]
            res[key] = [json.loads(ln) for ln in lines]          # every run recorded, in the order taken
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
