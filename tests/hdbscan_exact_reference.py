"""An exact reference of the device half of HDBSCAN (trase_amd/csrc/hdbscan.hip) on lattice clouds: plain numpy, no GPU.

The kernel's squared distance is the chain  s = fmaf(a_d - b_d, a_d - b_d, s).  On rows X = lo + step * Q with integer Q every
difference is an integer multiple of step, every square and every partial sum an integer multiple of step^2, and while the
largest possible sum stays below 2^24 units all of them are fp32 numbers: the fp32 result equals integer arithmetic in any
order.  ``assert_exact`` checks that premise; every caller states it.

Then the core distances are integers (``core2_units``), the mutual reachability max(core_i, core_j, d_ij) is an integer, and
the device's edge key (weight bits << 32 | min(i, j) << 16 | max(i, j)) is a strict total order on the undirected edges: the
minimum spanning tree is unique and ``mst_keys`` (Prim) must give the key set that the device's Boruvka rounds file."""
import numpy as np

# name -> (step, lo, levels): X = lo + step * Q, Q in [0, levels)
#   coarse: 1/4 in [-8, 8): differences <= 63 units, 64 * 63^2 = 254 016 < 2^24; heavy ties
#   fine: 1/64 in [-4, 4): differences <= 511 units, 64 * 511^2 = 16 711 744 < 2^24; few ties even at D = 64
GRIDS = {"coarse": (0.25, -8.0, 64), "fine": (1.0 / 64, -4.0, 512)}
KINDS = ("volume", "plane", "line", "coincident", "blobs")
EXACT_LIMIT = 1 << 24
NO_EDGE = np.int64(-1)          # ~0 as the device files it in the one slot that keeps no edge


def assert_exact(Q):
    """The premise of every exact comparison: no squared distance between two rows of Q can reach 2^24 units."""
    Q = np.asarray(Q)
    assert Q.dtype == np.int64 and Q.ndim == 2
    span = Q.max(0) - Q.min(0)
    assert int((span * span).sum()) < EXACT_LIMIT, f"squared distances up to {int((span * span).sum())} units are not exact in fp32"


def lattice_points(kind, n, D, grid, seed):
    """-> (Q int64 (n, D), X fp32 (n, D)) with X = lo + step * Q exactly."""
    step, lo, levels = GRIDS[grid]
    g = np.random.default_rng(seed)
    if kind == "volume":
        Q = g.integers(0, levels, (n, D))
    elif kind in ("plane", "line"):                       # all but two coordinates / all but one constant
        Q = np.repeat(g.integers(0, levels, (1, D)), n, axis=0)
        free = g.permutation(D)[:2 if kind == "plane" else 1]
        Q[:, free] = g.integers(0, levels, (n, len(free)))
    elif kind == "coincident":                            # the second half repeats the first half row for row
        h = (n + 1) // 2
        Q = g.integers(0, levels, (h, D))
        Q = np.concatenate([Q, Q[:n - h]])
    elif kind == "blobs":                                 # a few lattice centres plus small lattice offsets
        r = levels // 16
        centres = g.integers(r, levels - r, (4, D))
        Q = centres[g.integers(0, 4, n)] + g.integers(-r, r + 1, (n, D))
    else:
        raise ValueError(kind)
    Q = np.ascontiguousarray(Q, dtype=np.int64)
    assert Q.shape == (n, D) and Q.min() >= 0 and Q.max() < levels
    X = (lo + step * Q.astype(np.float64)).astype(np.float32)
    assert np.array_equal(X.astype(np.float64), lo + step * Q.astype(np.float64))
    return Q, np.ascontiguousarray(X)


def units_to_f32(units, step):
    """units * step^2 as fp32: exact for units < 2^24 and a power-of-two step."""
    u = np.asarray(units, dtype=np.int64)
    assert (u >= 0).all() and (u < EXACT_LIMIT).all()
    w = (u.astype(np.float64) * (step * step)).astype(np.float32)
    assert np.array_equal(w.astype(np.float64), u.astype(np.float64) * (step * step))
    return w


def core2_units(Q, k, block=512):
    """int64 (n,): the k-th smallest squared distance from every row to the OTHER rows (a duplicate is another row), in
    units.  float64 |a|^2 + |b|^2 - 2 a.b is exact for these integers."""
    n = Q.shape[0]
    assert 1 <= k < n
    Qf = Q.astype(np.float64)
    sq = (Qf * Qf).sum(1)
    out = np.empty(n, dtype=np.int64)
    for r0 in range(0, n, block):
        r1 = min(n, r0 + block)
        d = sq[r0:r1, None] + sq[None, :] - 2.0 * (Qf[r0:r1] @ Qf.T)
        d[np.arange(r1 - r0), np.arange(r0, r1)] = np.inf
        out[r0:r1] = np.partition(d, k - 1, axis=1)[:, k - 1].astype(np.int64)
    return out


def edge_keys(weight_units, i, j, step):
    """int64 keys of the edges (i, j) as the device files them: fp32 bits of the weight << 32 | min << 16 | max."""
    bits = units_to_f32(weight_units, step).view(np.uint32).astype(np.int64)
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    return (bits << 32) | (np.minimum(i, j) << 16) | np.maximum(i, j)


def mst_keys(Q, core_units, step):
    """int64 (n - 1,), ascending: the keys of THE minimum spanning tree of the mutual-reachability graph under the key order.
    Prim from row 0: n - 1 steps, each one row of distances; no n x n array."""
    n = Q.shape[0]
    assert 2 <= n <= 65536
    core = np.asarray(core_units, dtype=np.int64)
    Qf = Q.astype(np.float64)
    sq = (Qf * Qf).sum(1)
    idx = np.arange(n, dtype=np.int64)
    big = np.iinfo(np.int64).max
    best = np.full(n, big, dtype=np.int64)
    out = np.empty(n - 1, dtype=np.int64)
    v = 0
    in_tree = np.zeros(n, dtype=bool)
    in_tree[0] = True
    for t in range(n - 1):
        d = (sq + sq[v] - 2.0 * (Qf @ Qf[v])).astype(np.int64)
        w = np.maximum(np.maximum(core, core[v]), d)
        key = edge_keys(w, idx, v, step)
        np.minimum(best, key, out=key)
        best = np.where(in_tree, big, key)
        v = int(np.argmin(best))
        out[t] = best[v]
        in_tree[v] = True
        best[v] = big
    return np.sort(out)


def decode_keys(keys):
    """Sorted keys -> float64 (n - 1, 3) rows (i, j, weight): the float64 square root of the fp32 squared weight."""
    k = np.asarray(keys, dtype=np.int64)
    w2 = (k >> 32).astype(np.uint32).view(np.float32).astype(np.float64)
    return np.stack([((k >> 16) & 0xffff).astype(np.float64), (k & 0xffff).astype(np.float64), np.sqrt(w2)], axis=1)


def key_matrix(Q, core_units, step):
    """int64 (n, n) keys of every pair (the diagonal holds a self edge's key and must be ignored): for the small checks."""
    n = Q.shape[0]
    d = ((Q[:, None, :] - Q[None, :, :]) ** 2).sum(-1)
    core = np.asarray(core_units, dtype=np.int64)
    w = np.maximum(np.maximum(core[:, None], core[None, :]), d)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return edge_keys(w.reshape(-1), i.reshape(-1), j.reshape(-1), step).reshape(n, n), w


# ---- the case plan of tests/test_gpu_hdbscan_exact.py ---------------------------------------------------------------------
DS = (1, 3, 4, 8, 9, 12, 16, 17, 32, 33, 64)             # both sides of every hd_dpad step; D % 4 zero and non-zero
KS = (1, 2, 15, 16, 17, 63, 64)                           # the KC 16 | 64 step and both ends
NS = (2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4000)
N_SPLIT15 = 16385                                         # the smallest n at which hd_splits leaves 16
CLOUDS = (("coarse", "volume"), ("coarse", "plane"), ("coarse", "line"), ("coarse", "coincident"), ("coarse", "blobs"),
          ("fine", "volume"), ("fine", "blobs"))


def _fit_k(k, n):
    """The largest listed k not above the wanted one that the size admits (k < n)."""
    return max(c for c in KS if c <= k and c < n)


def exact_plan():
    """(n, D, k, grid, kind, offset) per case: a covering of DS, KS, NS, CLOUDS and both alignments, not their product.
    ``offset`` is the number of floats X starts behind a 16-byte boundary (0 or 1)."""
    plan = []
    for t in range(45):                                   # 11, 7 and 15 are pairwise coprime: three full rotations of NS
        n = NS[t % len(NS)]
        D = DS[t % len(DS)]
        grid, kind = CLOUDS[(t + t // len(KS)) % len(CLOUDS)]
        plan.append((n, D, _fit_k(KS[t % len(KS)], n), grid, kind, 0))
    plan += [
        (257, 64, 64, "fine", "volume", 0),              # the longest list beside the widest row
        (65, 64, 64, "coarse", "volume", 0),              # k = 64 with small n: every other row is in the list
        (65, 16, 63, "coarse", "blobs", 0),
        (257, 16, 17, "fine", "volume", 0),               # DP = 16 with KC = 64
        (513, 12, 16, "coarse", "volume", 0),             # DP = 16 with KC = 16
        (256, 1, 2, "coarse", "line", 0),                 # a line in one dimension: 64 places for 256 rows
        (1025, 1, 15, "fine", "line", 0),
        (2, 3, 1, "coarse", "coincident", 0),             # two equal rows: the one edge weighs 0
        (512, 8, 1, "coarse", "coincident", 0),           # k = 1 on duplicates: zero core distances, zero weights
        (1023, 33, 1, "fine", "coincident", 0),
        (257, 4, 2, "coarse", "volume", 1),               # X one float behind a 16-byte boundary, D % 4 == 0: hd_load_row's
        (257, 4, 2, "coarse", "volume", 0),               # scalar path for alignment alone, against the aligned run
        (1025, 32, 17, "fine", "blobs", 1),
        (1025, 32, 17, "fine", "blobs", 0),
        (N_SPLIT15, 4, 2, "coarse", "volume", 0),         # 65 row blocks: S = 15, chunk 1152
    ]
    return plan


def case_seed(n, D, k):
    return 100000 * k + 100 * n + D
