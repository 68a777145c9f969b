"""Numpy restatements of trase_amd.neighbors.dense_topk, loss_feature3d and loss_cls_3d (test infrastructure only): the brute-force
selection by the two 64-bit keys, both losses and every gradient in float64, the case plan of the exact GPU tests and the random
scenes of the float64 comparison.

Keys.  With b = the bits of the fp32 squared distance (a NaN becomes 0x7FC00000) the near end is ascending (b << 32) | id and
the far end ascending (~b << 32) | id: smaller / larger distance first, then lower id; NaN ranks above +inf at both.

Distances.  s = fmaf(q_d - p_d, q_d - p_d, s) over d in order.  ``dist2`` evaluates the chain in float64 (or rounds every step to
fp32: the difference is one fp32 operation, the product of two fp32 numbers is exact in float64, and the sum is rounded once
more -- double rounding, which the exact tests never meet because on lattice rows every step is an integer below 2^24).

Bars of the loss tests (tests/test_gpu_dense.py): four times the error of the reference's own fp32 torch statements on the same
inputs and indices, with a floor of 2^-22 times the float64 sum of the absolute terms (``*_abs`` below) for inputs where torch
happens to be exact.  A gradient is held element by element to max(4 * the largest torch error of its group, 2^-22 * the element's
own abs-sum).  The groups: rows at the 1e-8 clamp (a zero row, a row below it) have gradients 1e8 times the others', and
entries with p = 0 gradients 1e10 times the others', so each is measured and held apart -- one largest error over all would be
theirs and hold nothing else.  torch differentiates a row BELOW the clamp differently (its norm stays in the graph: deviation in
INTEGRATION.md), so such a row's torch error is no measure and only the floor and its group's other rows set its bar."""
import numpy as np

U = 2.0 ** -24
NAN_BITS = 0x7FC00000
EPS_COS = 1e-8
EPS_LOG = 1e-10


# ---- distances and the two key orders ---------------------------------------------------------------------------------------
def dist2(q, p, dtype=np.float64):
    """(M, N) squared distances by the chain, every step rounded to `dtype`."""
    q, p = np.asarray(q), np.asarray(p)
    s = np.zeros((len(q), len(p)), dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(q.shape[1]):
            t = (q[:, None, d].astype(dtype) - p[None, :, d].astype(dtype)).astype(np.float64)
            s = (t * t + s.astype(np.float64)).astype(dtype)
    return s


def keys_of(d2):
    """(near keys, far keys) as uint64 of an (M, N) array of squared distances (rounded to fp32 first)."""
    b = np.ascontiguousarray(np.asarray(d2, dtype=np.float32)).view(np.uint32).astype(np.uint64)
    b = np.where(np.isnan(d2), np.uint64(NAN_BITS), b)
    ids = np.arange(b.shape[1], dtype=np.uint64)[None, :]
    return (b << np.uint64(32)) | ids, ((~b & np.uint64(0xFFFFFFFF)) << np.uint64(32)) | ids


def topk_by_keys(d2, k_near, k_far):
    """-> (near_d2 (M, k_near) fp32, near_idx int64, far_d2, far_idx): the k smallest keys of either end, in key order."""
    d32 = np.asarray(d2, dtype=np.float32)
    d32 = np.where(np.isnan(d32), np.uint32(NAN_BITS).view(np.float32), d32)          # the canonical NaN
    out = []
    for keys, k in zip(keys_of(d32), (k_near, k_far)):
        idx = np.argsort(keys, axis=1, kind="stable")[:, :k].astype(np.int64)
        out += [np.take_along_axis(d32, idx, axis=1), idx]
    return tuple(out)


def topk_f64(q, p, k_near, k_far):
    """Float64 selection for the random scenes -> dict(near_idx, far_idx, near_d2, far_d2, near_gap, far_gap, near_at, far_at):
    gap = the float64 difference between the k-th and the (k + 1)-th distance of an end (inf where k == N), at = the larger."""
    d = dist2(np.asarray(q, dtype=np.float64), np.asarray(p, dtype=np.float64))
    order = np.argsort(d, axis=1, kind="stable")
    N = d.shape[1]
    res = {}
    for end, k, o in (("near", k_near, order), ("far", k_far, order[:, ::-1])):
        srt = np.take_along_axis(d, o, axis=1)
        res[end + "_idx"], res[end + "_d2"] = o[:, :k], srt[:, :k]
        if 0 < k < N:
            res[end + "_gap"] = np.abs(srt[:, k] - srt[:, k - 1])
            res[end + "_at"] = np.maximum(srt[:, k], srt[:, k - 1])
        else:
            res[end + "_gap"], res[end + "_at"] = np.full(len(d), np.inf), np.ones(len(d))
    return res


def near_tie_rows(ref, D, k_near, k_far):
    """Rows whose float64 gap at the k-th place of an end in use is at most 4 (D + 1) 2^-24 of the larger distance."""
    tie = np.zeros(len(ref["near_gap"]), dtype=bool)
    for end, k in (("near", k_near), ("far", k_far)):
        if k:
            tie |= ref[end + "_gap"] <= 4 * (D + 1) * U * ref[end + "_at"]
    return tie


# ---- the case plan of the exact GPU tests -------------------------------------------------------------------------------------
# (M, N, D, k_near, k_far, kind, misaligned); kind: self (queries are the points), cross, coincident, nan_query, nan_point
EXACT_CASES = [
    (1, 64, 3, 16, 4, "cross", False),
    (255, 255, 1, 1, 1, "self", False),
    (256, 63, 4, 2, 0, "cross", False),
    (257, 65, 5, 0, 2, "cross", False),
    (600, 1000, 8, 16, 16, "cross", False),
    (257, 1000, 31, 31, 0, "cross", False),
    (300, 300, 32, 0, 31, "self", False),
    (129, 200, 33, 32, 32, "cross", False),
    (65, 64, 63, 32, 0, "cross", False),
    (64, 65, 64, 0, 32, "cross", False),
    (32, 32, 3, 32, 32, "self", False),
    (5, 1, 3, 1, 1, "cross", False),
    (16, 16, 64, 16, 16, "self", False),
    (300, 700, 12, 1, 31, "cross", False),
    (1025, 1025, 16, 2, 1, "self", False),
    (257, 500, 3, 5, 2, "coincident", False),
    (100, 100, 32, 16, 4, "coincident", False),
    (70, 300, 3, 16, 4, "nan_query", False),
    (70, 300, 32, 5, 5, "nan_point", False),
    (257, 1000, 4, 16, 4, "cross", True),
    (130, 130, 32, 5, 0, "self", True),
    (66, 200, 64, 0, 16, "cross", True),
    (131073, 130, 3, 16, 4, "cross", False),
]
EXACT_D = (1, 3, 4, 5, 8, 31, 32, 33, 63, 64)
EXACT_K = (1, 2, 16, 31, 32)


def lattice(rows, D, seed):
    """Integer rows in {-4..4}: every squared distance is an integer <= 64 D <= 4096 < 2^24, exact in fp32 in any order."""
    return np.random.default_rng(seed).integers(-4, 5, size=(rows, D)).astype(np.float32)


def exact_case(case):
    """-> (queries, points) of one plan entry."""
    M, N, D, kn, kf, kind, _ = case
    seed = 7919 * M + 31 * N + D
    p = lattice(N, D, seed)
    if kind in ("self", "coincident") and M == N:
        q = p
    else:
        q = lattice(M, D, seed + 1)
    if kind == "coincident":
        p = np.repeat(p[:1], N, axis=0)
        q = p if M == N else q
    if kind == "nan_query":
        q = q.copy()
        q[M // 2, D // 2] = np.nan
    if kind == "nan_point":
        p = p.copy()
        p[N // 3, 0] = np.nan
    return q, p


# ---- the random scenes of the float64 comparison --------------------------------------------------------------------------------
def random_scenes():
    """name -> (queries, points, k_near, k_far), numpy default_rng(0)."""
    g = np.random.default_rng(0)
    cloud = g.uniform(-1.3, 1.3, (3000, 3)).astype(np.float32)
    unit = g.normal(size=(5000, 32))
    unit = (unit / np.linalg.norm(unit, axis=1, keepdims=True)).astype(np.float32)
    pick = g.permutation(5000)[:800]
    wide = g.normal(size=(3000, 64)).astype(np.float32)
    pick2 = g.permutation(3000)[:257]
    return {"cloud3": (cloud, cloud, 16, 4), "unit32": (unit[pick], unit, 5, 0), "wide64": (wide[pick2], wide, 32, 32)}


# ---- loss_feature3d -----------------------------------------------------------------------------------------------------------
def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def feature3d(f, near_idx, far_idx, lambda_p=1.0, lambda_n=1.0, g_out=1.0):
    """-> dict(loss, grad (rows, D), loss_abs, grad_abs (rows, D)) in float64; ids outside [0, rows) are edges to nowhere."""
    f = np.asarray(f, dtype=np.float64)
    rows, D = f.shape
    n = np.maximum(np.sqrt((f * f).sum(1)), EPS_COS)
    u = f / n[:, None]
    g_u, a_u = np.zeros_like(u), np.zeros_like(u)
    loss = loss_abs = 0.0
    for idx, near, lam in ((near_idx, True, lambda_p), (far_idx, False, lambda_n)):
        idx = np.asarray(idx).astype(np.int64)
        k = idx.shape[1]
        ok = (idx >= 0) & (idx < rows)
        src = np.repeat(np.arange(rows), k).reshape(rows, k)[ok]
        j = idx[ok]
        c = (u[src] * u[j]).sum(1)
        s = _sigmoid(1.0 - c) if near else _sigmoid(c)
        scale = lam / (rows * k)
        loss += scale * s.sum()
        loss_abs += abs(scale) * s.sum()
        w = (-scale if near else scale) * s * (1.0 - s)
        np.add.at(g_u, src, w[:, None] * u[j])
        np.add.at(g_u, j, w[:, None] * u[src])
        np.add.at(a_u, src, np.abs(w)[:, None] * np.abs(u[j]))
        np.add.at(a_u, j, np.abs(w)[:, None] * np.abs(u[src]))
    live = (n > EPS_COS)[:, None]
    grad = np.where(live, (g_u - u * (u * g_u).sum(1, keepdims=True)) / n[:, None], g_u / EPS_COS)
    grad_abs = np.where(live, (a_u + np.abs(u) * (np.abs(u) * a_u).sum(1, keepdims=True)) / n[:, None], a_u / EPS_COS)
    return dict(loss=loss, grad=g_out * grad, loss_abs=loss_abs, grad_abs=abs(g_out) * grad_abs)


# ---- loss_cls_3d --------------------------------------------------------------------------------------------------------------
def cls3d(pred, sample, idx, lambda_val=2.0, g_out=1.0):
    """pred (N, C), sample (S,) rows of pred, idx (S, k) rows of pred -> dict(loss, grad (N, C), loss_abs, grad_abs)."""
    p = np.asarray(pred, dtype=np.float64)
    N, C = p.shape
    sample, idx = np.asarray(sample).astype(np.int64), np.asarray(idx).astype(np.int64)
    S, k = idx.shape
    w = lambda_val / (S * k * C)
    l = np.log(p + EPS_LOG)
    ps, ls = p[sample], l[sample]                                     # (S, C)
    diff = ls[:, None, :] - l[idx]                                    # (S, k, C)
    loss = w * (ps[:, None, :] * diff).sum()
    loss_abs = abs(w) * (np.abs(ps)[:, None, :] * (np.abs(ls)[:, None, :] + np.abs(l[idx]))).sum()
    grad, ga = np.zeros_like(p), np.zeros_like(p)
    direct = diff.sum(1) + k * ps / (ps + EPS_LOG)
    np.add.at(grad, sample, direct)
    np.add.at(ga, sample, (np.abs(ls)[:, None, :] + np.abs(l[idx])).sum(1) + k * np.abs(ps / (ps + EPS_LOG)))
    back = -ps[:, None, :] / (p[idx] + EPS_LOG)                       # (S, k, C)
    np.add.at(grad, idx.reshape(-1), back.reshape(S * k, C))
    np.add.at(ga, idx.reshape(-1), np.abs(back).reshape(S * k, C))
    return dict(loss=loss, grad=g_out * w * grad, loss_abs=loss_abs, grad_abs=abs(g_out * w) * ga)


# ---- the transposed graph with two counts ---------------------------------------------------------------------------------------
def reverse_graph_to(idx, targets):
    """idx (rows, k) into `targets` rows -> (rev_ranges (targets, 2), rev_edges (rows * k)): edge numbers sorted stably by target;
    an id outside [0, targets) sorts behind every row and is in no range (tests/neighbors_reference.py's reverse_graph with the
    target count on its own)."""
    idx = np.asarray(idx).astype(np.int64)
    flat = idx.reshape(-1)
    keys = np.where((flat >= 0) & (flat < targets), flat, targets)
    edges = np.argsort(keys, kind="stable")
    counts = np.bincount(keys, minlength=targets + 1)[:targets]
    end = np.cumsum(counts)
    ranges = np.stack([end - counts, end], axis=1)
    ranges[counts == 0] = 0
    return ranges.astype(np.int32), edges.astype(np.int32)
