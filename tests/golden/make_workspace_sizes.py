"""Generates workspace_sizes.json: what every ``trase_*_sizes`` function, ``trase_rast_geom_layout`` and the two VGG16 families'
``trase_vgg_ws_bytes`` / ``trase_lpips_ws_bytes`` of the built library return over a table of shapes.  The table pins the workspace layouts: tests/test_workspace_layout.py asserts that the library
under test returns exactly these integers, so regenerate it only from a commit whose layouts are known to be right.

    python tests/golden/make_workspace_sizes.py          (TRASE_RAST_LIB=<path> selects another build of the library)

The calls need no GPU.  A case is {"args": [...], "rc": status, "out": [...]}: ``args`` are the leading scalar arguments (a
list among them is an int32 input array), ``out`` the integers the function wrote (empty when rc != 0), ``"null_out": true``
marks a call made with null output pointers.  The shapes cross every rule of the layouts: item counts of 0 (where
accepted), 1 and either side of the radix sort's workgroup tile (2048), of its short-sort boundary (16 x 2048 = 32768) and of
the scan partials' 1024; about 2.5 M; feature widths 0, 16 and 32; odd image sizes; point counts across the steps of the KNN
hash's bucket bits; the limits of every segmentation, display and HDBSCAN entry, one step inside and one step outside; every cut of the VGG16
extractor (and 0 and 9) at the smallest image its pools accept, one pixel either side, odd sizes, 1080p and H * W = 2^25 - 4096, 2^25.
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from trase_amd import _lib  # noqa: E402

ALSO = ("trase_rast_geom_layout", "trase_vgg_ws_bytes", "trase_lpips_ws_bytes")     # sizes functions not named *_sizes
OUT_SLOTS = 16          # length of the array handed to an int64* output (trase_compose_sizes writes n_parts + 1 <= 9 of them)


def _ints(obj):
    if isinstance(obj, C.Structure):
        return [int(getattr(obj, f[0])) for f in obj._fields_]
    if isinstance(obj, C.Array):
        return [int(v) for v in obj]
    return [int(obj.value)]


def call(lib, name, args, null_out=False):
    """-> (rc, integers written): calls ``name`` with the scalar ``args`` and fresh (or null) output objects."""
    argtypes = next(a for n, _, a in _lib.SYMBOLS if n == name)
    rest, actual, outs = list(args), [], []
    for t in argtypes:
        if rest and isinstance(rest[0], list):
            actual.append((C.c_int32 * len(rest[0]))(*rest.pop(0)))
        elif rest:
            actual.append(rest.pop(0))
        elif null_out:
            actual.append(None)
        else:
            target = t._type_
            obj = (target * OUT_SLOTS)() if target is C.c_int64 else target()
            outs.append(obj)
            actual.append(obj if target is C.c_int64 else C.byref(obj))
    rc = int(getattr(lib, name)(*actual))
    return rc, ([v for o in outs for v in _ints(o)] if rc == 0 else [])


COUNTS = [1, 1023, 1024, 1025, 2047, 2048, 2049, 3071, 3072, 3073, 32767, 32768, 32769, 2500000, 2500001]
IMAGES = [(1, 1), (7, 9), (127, 83), (801, 799), (1297, 733), (1920, 1080)]


def cases():
    t = {}
    t["trase_rast_sizes"] = ([[p, 127, 83, f, cap] for p in [0] + COUNTS for f in (0, 16, 32) for cap in COUNTS] +
                             [[p, w, h, 32, cap] for (w, h) in IMAGES for (p, cap) in ((0, 1), (1000, 50000), (2049, 32769))] +
                             [[-1, 640, 360, 32, 1], [10, 0, 360, 32, 1], [10, 640, 0, 32, 1], [10, 640, 360, 32, 0]])
    t["trase_rast_geom_layout"] = [[p] for p in [0] + COUNTS + [-1]]
    t["trase_rast_pair_sizes"] = [[p] for p in [0, 512, 513, 16383, 16384, 16385] + COUNTS + [-1]]
    knn = sorted({n for b in (4, 5, 8, 11, 12, 15, 16, 21, 22, 25, 26) for n in ((1 << b) - 1, 1 << b, (1 << b) + 1)} | set(COUNTS))
    t["trase_knn_sizes"] = [[n] for n in [0] + knn + [-1]]
    t["trase_lift_sizes"] = [[n, bins] for n in (0, 1, 2048, 2049, 32769, 2500000) for bins in (0, 1, 4096)] + [[10, 4097], [10, -1], [-1, 8]]
    t["trase_mlp_sizes"] = [[]]
    t["trase_mlp_train_sizes"] = [[n] for n in [0, 31, 32, 33, 255, 256, 257] + COUNTS + [-1]]
    t["trase_loss_sizes"] = ([[c, h, w] for c in (1, 3, 32) for (w, h) in IMAGES] + [[0, 8, 8], [3, 0, 8], [3, 8, 0]])
    t["trase_contrastive_sizes"] = [[s] for s in (1, 31, 32, 33, 63, 64, 65, 1000, 4096, 4097, 0)]
    t["trase_densify_sizes"] = [[p] for p in COUNTS + [(1 << 29) - 1, 1 << 29, 0]]
    t["trase_pairhead_sizes"] = [[s] for s in (1, 63, 64, 65, 1000, 8192, 8193, 0)]
    t["trase_compact_pixels_sizes"] = [[hw] for hw in (1, 4095, 4096, 4097, 127 * 83, 1920 * 1080, 1 << 33, 0)]
    t["trase_featnorm_sizes"] = [[hw] for hw in (1, 127 * 83, 1920 * 1080, 0)]
    t["trase_nnfm_sizes"] = [[64, 1, 1], [64, 255, 256], [128, 256, 257], [192, 257, 255], [512, 4096, 65536 * 32], [256, 99 * 77, 101 * 75],
                             [512, 1000, 65536 * 32 + 1], [32, 10, 10], [576, 10, 10], [100, 10, 10], [64, 0, 10], [64, 10, 0]]
    dims = (1, 8, 9, 16, 17, 32, 33, 64)
    t["trase_kmeans_sizes"] = ([[n, d, k] for d in dims for k in (1, 2, 10, 127, 128) for n in (k, 1000, 65536, 65537, 2500000) if n >= k] +
                               [[127, 32, 128], [1000, 32, 0], [1000, 32, 129], [1000, 0, 10], [1000, 65, 10]])
    t["trase_segment_mask_sizes"] = ([[n, d, s] for d in dims for s in (0, 1, 2, 127, 128) for n in (0, 1, 1000, 65536, 65537, 2500000)] +
                                     [[-1, 32, 4], [1000, 32, -1], [1000, 32, 129], [1000, 0, 4], [1000, 65, 4]])
    t["trase_assign_clusters_sizes"] = [[0, 32, 1], [1000, 1, 4096], [2500000, 64, 10], [1000, 32, 4097], [1000, 32, 0], [1000, 65, 4], [1000, 0, 4], [-1, 32, 4]]
    t["trase_hdbscan_sizes"] = ([[n, d, k] for n in (2, 3, 255, 256, 257, 4095, 4096, 4097, 30000, 65535, 65536) for d in (1, 32, 64)
                                 for k in (1, 15, 16, 17, 64) if k < n] +
                                [[2, 32, 2], [1, 32, 1], [65537, 32, 5], [1000, 0, 5], [1000, 65, 5], [1000, 32, 0], [1000, 32, 65]])
    t["trase_label_centres_sizes"] = ([[n, d, c] for n in (0, 1, 1000, 65536, 2500000) for d in (1, 32, 64) for c in (1, 127, 128, 129, 4096)] +
                                      [[-1, 32, 4], [1000, 0, 4], [1000, 65, 4], [1000, 32, 0], [1000, 32, 4097]])
    t["trase_splat_sizes"] = ([[n, w, h] for n in (0, 1000) for (w, h) in IMAGES] +
                              [[10, 46340, 46340], [10, 46341, 46341], [-1, 8, 8], [10, 0, 8], [10, 8, 0]])
    t["trase_feature_gram_sizes"] = ([[n, d] for n in (2, 255, 256, 257, 65536, 65537, 2500000) for d in dims] + [[1, 32], [1000, 0], [1000, 65]])
    t["trase_compose_sizes"] = [[[5], 1, 32], [[3, 0, 7, 100000], 4, 0], [[1] * 8, 8, 64], [[1] * 8, 9, 32], [[4, -1], 2, 32], [[4], 1, 65],
                                [[4], 0, 32], [[1 << 24, 1 << 24], 2, 32], [[(1 << 24) - 1, 1 << 24], 2, 32]]
    cuts = list(range(8, -1, -1)) + [9]              # a good call first: the null-output row repeats the first row
    pools = lambda k: sum(1 for p in (2, 4, 7) if p < k)
    t["trase_vgg_ws_bytes"] = ([[k, h, w] for (h, w) in ((67, 35), (8, 8), (9, 15), (1080, 1920), (4096, 8191), (4096, 8192)) for k in cuts] +
                               [[k, s, s] for k in cuts for s in ((1 << pools(k)) - 1, 1 << pools(k), (1 << pools(k)) + 1)])
    t["trase_lpips_ws_bytes"] = [[h, w] for (h, w) in ((16, 16), (15, 16), (16, 15), (17, 31), (67, 35), (1080, 1920), (4096, 8191), (4096, 8192))]
    return t


def declared():
    """the functions the table covers, out of the library's symbol list"""
    return sorted(n for n, _, _ in _lib.SYMBOLS if n.endswith("_sizes") or n in ALSO)


def build_table(lib):
    table = {}
    for name, rows in cases().items():
        out = []
        for args in rows:
            rc, ints = call(lib, name, args)
            out.append({"args": args, "rc": rc, "out": ints})
        rc, ints = call(lib, name, rows[0], null_out=True)
        out.append({"args": rows[0], "null_out": True, "rc": rc, "out": ints})
        table[name] = out
    return table


def main():
    lib = _lib.load()
    table = build_table(lib)
    assert sorted(table) == declared(), sorted(set(declared()) ^ set(table))
    out = os.path.join(HERE, "workspace_sizes.json")
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": [\n" + ",\n".join("  " + json.dumps(c) for c in v) + "\n]"
                                   for k, v in sorted(table.items())) + "\n}\n")
    print("wrote", out, os.path.getsize(out), "bytes,", sum(len(v) for v in table.values()), "cases,",
          sum(1 for v in table.values() for c in v if c["rc"] != 0), "of them error returns")


if __name__ == "__main__":
    main()
