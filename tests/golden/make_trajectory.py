"""Generates trajectory.npz: the imported reference's ``farthest_point_sample`` (utils/time_utils.py:375-396, pulled out of
the file with ``ast`` and run on CPU tensors) over small clouds, and matplotlib's jet table as gui.py:1183 quantises it.

    python tests/golden/make_trajectory.py

Clouds: coordinates are multiples of 1/256 in [-2, 2], so every squared distance is a multiple of 2^-16 below 2^6 and
every fp32 product and sum of the sampler is exact -- the sequence then cannot depend on the order or the fusing of the
arithmetic.  "lattice" clouds draw distinct points of the 1/256 grid uniformly, "gauss" clouds round a normal cloud to it.
The generator asserts that no step has a tie at its maximum (the reference's arg-max among equals is torch's choice) and
shifts the seed until none has.  Per cloud: ``torch.manual_seed(seed)``, then the reference's call, whose first index is
its own ``torch.randint`` draw.  One cloud is also sampled through a mask the way gui.py:1160-1161 does it: the reference
runs on ``points[mask]`` and its indices are mapped back through ``arange(N)[mask]``.

Records per cloud the points, the seed, the mask (or none) and the reference's 64 rows; and ``int32(jet(i / max(1, n - 1))[:3]
* 255)`` for n = 1, 2, 7, 512 from matplotlib.  Runs on the CPU only; the archive is written with fixed time stamps.
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
from tests import trajectory_reference as tr  # noqa: E402

NPOINT = 64
CLOUDS = (("lattice", 65, False), ("gauss", 257, False), ("lattice", 1000, True), ("gauss", 5000, False))
JET_SIZES = (1, 2, 7, 512)


def load_reference():
    tree = ast.parse(open(os.path.join(REF, "utils", "time_utils.py")).read())
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "farthest_point_sample")
    ns = {"torch": torch}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "time_utils.py", "exec"), ns)
    return ns["farthest_point_sample"]


def make_cloud(kind, n, seed):
    g = np.random.default_rng(seed)
    if kind == "lattice":
        k = np.unique(g.integers(-512, 513, (2 * n, 3)), axis=0)
        k = k[g.permutation(len(k))[:n]]
    else:
        k = np.clip(np.round(g.standard_normal((n, 3)) * 0.7 * 256), -512, 512)
    assert len(k) == n
    return (k / 256.0).astype(np.float32)


def has_tie(points, rows, mask):
    """Whether a step of the sequence `rows` has more than one candidate at its maximum distance."""
    q = points.astype(np.float64)
    cand = np.ones(len(q), dtype=bool) if mask is None else mask
    dist = np.full(len(q), 1e10)
    for r in rows[:-1]:
        dist = np.minimum(dist, ((q - q[r]) ** 2).sum(-1))
        if int((dist[cand] == dist[cand].max()).sum()) != 1:
            return True
    return False


def main():
    ref_fps = load_reference()
    arrays = {"npoint": np.int64(NPOINT), "count": np.int64(len(CLOUDS))}
    for c, (kind, n, masked) in enumerate(CLOUDS):
        for seed in range(100 * c, 100 * c + 100):
            points = make_cloud(kind, n, seed)
            mask = (np.random.default_rng(seed + 7).uniform(size=n) < 0.6) if masked else None
            torch.manual_seed(seed)
            if masked:
                masked_idx = torch.arange(n)[torch.from_numpy(mask)]
                rows = masked_idx[ref_fps(torch.from_numpy(points)[None, torch.from_numpy(mask)], NPOINT)[0]].numpy()
            else:
                rows = ref_fps(torch.from_numpy(points)[None], NPOINT)[0].numpy()
            if not has_tie(points, rows, mask):
                break
            print(f"cloud {c}: seed {seed} has a tie at a maximum, next seed")
        else:
            raise SystemExit(f"refusing to write trajectory.npz: cloud {c} has a tie at a maximum for every seed")
        mine = tr.fps(points, NPOINT, int(rows[0]), mask=mask)
        print(f"cloud {c}: {kind}, {n} points{', masked' if masked else ''}, seed {seed}, start {int(rows[0])}; the numpy rule "
              f"{'equals' if np.array_equal(mine, rows) else 'DIFFERS from'} the reference's sequence")
        assert np.array_equal(mine, rows) and len(np.unique(rows)) == NPOINT
        arrays[f"points{c}"] = points
        arrays[f"seed{c}"] = np.int64(seed)
        arrays[f"mask{c}"] = mask if masked else np.zeros(0, dtype=bool)
        arrays[f"rows{c}"] = rows.astype(np.int64)
    import matplotlib
    jet = matplotlib.colormaps["jet"]              # what gui.py:1168's cm.get_cmap("jet") returns
    for n in JET_SIZES:
        arrays[f"jet{n}"] = np.array([np.array(jet(i / max(1, float(n - 1)))[:3]) * 255 for i in range(n)], dtype=np.int32)
    out = os.path.join(HERE, "trajectory.npz")
    write_npz(out, arrays)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
