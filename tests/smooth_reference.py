"""Float64 statement of the KNN feature smoothing (trase_amd/smooth.py, csrc/smooth.hip), its exact transpose, an fp32
evaluation in the kernels' order, a numpy restatement of ``reverse_adjacency`` and the hand-built graphs of
tests/test_gpu_smooth_edges.py (test infrastructure only).

    out[i] = mean over the selected slots s of n(x[idx[i, sel[s]]]),   n(x) = x / max(||x||, 1e-12)
    dL/dx[j] = J_j^T G_j,  G_j = (1/S) sum of dL/dout[i] over the selected (i, k) with idx[i, k] = j,
    J = (I - n n^T) / ||x|| for ||x|| >= eps and I / eps below (the normalisation is linear there).

The device is held to ``bar``: 4 times the error of the fp32 evaluation on the same input plus one fp32 ulp of the result's
scale (the rule of tests/test_gpu_vgg.py).  The fp32 evaluation follows the kernels -- the forward adds the slots in the order
of ``sel``, the backward adds a node's incoming edges by ascending i*K+k -- but rounds every product and sum on its own where
the device may fuse them."""
import numpy as np
import torch

F = 32
EPS = 1e-12
ULP = 2.0 ** -23
MARGIN = 4.0


# ---- float64 -------------------------------------------------------------------------------------------------------------------
def forward64(x, idx, sel):
    x = np.asarray(x, np.float64).reshape(-1, F)
    n = x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), EPS)
    return n[np.asarray(idx)[:, np.asarray(sel)]].mean(axis=1)


def gathered64(idx, sel, g_out):
    """G_j = (1/S) sum of g_out[i] over the selected (i, k) with idx[i, k] = j"""
    g_out, idx = np.asarray(g_out, np.float64).reshape(-1, F), np.asarray(idx)
    G = np.zeros_like(g_out)
    for s in np.asarray(sel):
        np.add.at(G, idx[:, s], g_out)
    return G / len(sel)


def backward64(x, idx, sel, g_out):
    x = np.asarray(x, np.float64).reshape(-1, F)
    G = gathered64(idx, sel, g_out)
    norm = np.linalg.norm(x, axis=1, keepdims=True)
    n = x / np.maximum(norm, EPS)
    above = (G - n * (n * G).sum(axis=1, keepdims=True)) / np.maximum(norm, EPS)
    return np.where(norm >= EPS, above, G / EPS)


def reverse_adjacency_np(idx):
    """rev_ptr (P + 1,) int32, rev_src (P K,) int32: the flat positions i*K+k of idx, stably sorted by the node they name"""
    idx = np.asarray(idx)
    flat = idx.reshape(-1)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=idx.shape[0]))])
    return ptr.astype(np.int32), np.argsort(flat, kind="stable").astype(np.int32)


# ---- fp32 in the kernels' order ----------------------------------------------------------------------------------------------
def _group8_sum(v):
    """v (P, 8) fp32: the xor-butterfly of group8_sum, every lane's total (P, 8)"""
    lane = np.arange(8)
    for o in (1, 2, 4):
        v = v + v[:, lane ^ o]
    return v


def inv_norm32(x):
    x = np.asarray(x, np.float32).reshape(-1, 8, 4)
    sq = x * x
    n2 = _group8_sum((sq[..., 0] + sq[..., 1]) + (sq[..., 2] + sq[..., 3]))[:, 0]
    return np.float32(1.0) / np.maximum(np.sqrt(n2), np.float32(EPS))


def forward32(x, idx, sel):
    x = np.asarray(x, np.float32).reshape(-1, F)
    idx = np.asarray(idx)
    w = inv_norm32(x)
    acc = np.zeros((idx.shape[0], F), np.float32)
    for s in np.asarray(sel):
        j = idx[:, s]
        acc = acc + x[j] * w[j][:, None]
    return acc * (np.float32(1.0) / np.float32(len(sel)))


def backward32(x, idx, sel, g_out):
    x, g_out = np.asarray(x, np.float32).reshape(-1, F), np.asarray(g_out, np.float32).reshape(-1, F)
    idx = np.asarray(idx)
    P, K = idx.shape
    on = np.zeros(K, bool)
    on[np.asarray(sel)] = True
    G = np.zeros((P, F), np.float32)
    for i in range(P):                                  # ascending i*K+k: every node sees its edges in that order
        for k in np.flatnonzero(on):
            G[idx[i, k]] += g_out[i]
    G = G * (np.float32(1.0) / np.float32(len(sel)))
    w = inv_norm32(x)[:, None]
    p = (x * G).reshape(P, 8, 4)
    dot = _group8_sum((p[..., 0] + p[..., 1]) + (p[..., 2] + p[..., 3]))[:, :1] * w * w
    return np.where(w < np.float32(1.0) / np.float32(EPS), (G - x * dot) * w, G * w)


def bar(emulated, exact, per_row=False):
    """MARGIN times the fp32 evaluation's error plus one ulp of the result's scale -- over the tensor, or row by row"""
    axis = 1 if per_row else None
    return MARGIN * np.abs(emulated - exact).max(axis=axis) + ULP * np.abs(exact).max(axis=axis)


def share(got, emulated, exact, per_row=False, rows=None):
    """largest (device error / bar); where the bar is zero (an exactly zero result) any error is infinite"""
    axis = 1 if per_row else None
    err, b = np.atleast_1d(np.abs(np.asarray(got, np.float64) - exact).max(axis=axis)), np.atleast_1d(bar(emulated, exact, per_row))
    s = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err == 0, 0.0, np.inf))
    if per_row and rows is not None:
        s = s[rows]
    return float(np.max(s))


# ---- graphs ----------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def data(P, seed):
    """features (P, 1, 32) and upstream weights (P, 1, 32), fp32 numpy"""
    g = _gen(seed)
    return torch.randn(P, 1, F, generator=g).numpy(), torch.randn(P, 1, F, generator=g).numpy()


RING_P = (1, 7, 8, 9, 31, 32, 33, 257)                 # eight lanes own a Gaussian, 32 Gaussians make a block


def ring(P):
    i = np.arange(P)[:, None]
    return (i + np.array([[1, 2, P - 1, 3]])) % P, np.array([2, 0, 3])


KS_CASES = ((2, 1), (2, 2), (3, 2), (16, 1), (16, 16), (32, 1), (32, 16), (32, 32))


def ks_graph(K, S, P=67):
    """random targets; sel unsorted; slot 31 is the only selected slot of (32, 1) and one of the slots of (32, 16), (32, 32)"""
    g = _gen(100 * K + S)
    idx = torch.randint(0, P, (P, K), generator=g).numpy()
    if (K, S) == (32, 1):
        sel = np.array([31])
    else:
        perm = torch.randperm(K, generator=g).numpy()
        sel = perm[:S]
        if K == 32 and 31 not in sel:
            sel[S // 2] = 31
    if S >= 2 and (np.diff(sel) > 0).all():
        sel = sel[::-1].copy()
    return idx, sel


def ladder():
    """P = 24, K = 4: node t has in-degree exactly t for t = 0 ... 9 (every remainder of the four-edge loop, and the empty list);
    the other 51 edges go to nodes 10 ... 23.  sel = (2, 0): selected and unselected slots are mixed among the incoming edges."""
    P, K = 24, 4
    g = _gen(7)
    pos = torch.randperm(P * K, generator=g).numpy()
    flat = np.empty(P * K, np.int64)
    at = 0
    for t in range(10):
        flat[pos[at:at + t]] = t
        at += t
    flat[pos[at:]] = 10 + torch.randint(0, P - 10, (P * K - at,), generator=g).numpy()
    return flat.reshape(P, K), np.array([2, 0])


def hub():
    """P = 257, K = 8: every edge points at node 0 (in-degree 2056)"""
    return np.zeros((257, 8), np.int64), np.array([5, 1, 6])


def repeats():
    """P = 9, K = 4: slot 0 is a self-loop, slots 1 and 3 name the same node, all three selected"""
    i = np.arange(9)
    return np.stack([i, (i + 2) % 9, (i + 5) % 9, (i + 2) % 9], axis=1), np.array([3, 1, 0])


NORMS = (0.0, 1e-20, 5e-13, 2e-12, 1e-3)               # exact zero, squares underflow, below eps, just above eps, small


def norm_branches():
    """P = 12, K = 4.  Rows 0 ... 4 have the norms NORMS; output row i < 5 reads node i alone (all four slots), so every branch
    shows in the forward on its own; rows 5 ... 11 mix all nodes, so every node has incoming edges from several rows.
    -> (features (12, 1, 32), upstream weights, idx, sel)"""
    P, K = 12, 4
    g = _gen(21)
    x = torch.randn(P, F, generator=g, dtype=torch.float64)
    for i, n in enumerate(NORMS):
        x[i] = x[i] / x[i].norm() * n
    idx = torch.randint(0, P, (P, K), generator=g).numpy()
    idx[:5] = np.arange(5)[:, None]
    idx[5:10, 1] = np.arange(5)                          # every special node is also read by a mixed row through a selected slot
    w = torch.randn(P, 1, F, generator=g).numpy()
    return x.float().reshape(P, 1, F).numpy(), w, idx, np.array([3, 1])
