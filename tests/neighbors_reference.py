"""Float64 restatements of the k-NN graph, its transpose and the losses of trase_amd/neighbors.py (numpy; the whole rigid loss
with torch float64 for the SVD's autograd; test infrastructure only), and the forward-error bounds the fp32 kernels are held to.

A bound is (fp32 roundings on the longest path) * 2^-24 * (float64 sum of the absolute values of the terms).  u = 2^-24.

Feature loss.  Tables: s = 1 / (1 + exp(-f)) is exp (2), + (1), / (1): relative error 4u.  l = log(s + eps) is + (1), log (2)
  relative to |l|, and the 5u relative error of its argument moves a logarithm by 5u ABSOLUTELY: |dl| <= 2u |l| + 6u, covered by
  8u (|l| + 1).  A term of the value is s_i (l_i - l_j): rounded difference (1), product (1), the table errors (4 on s, 8 on
  each l against |l| + 1), then k sequential additions: (k + 16) u * sum of s_i (|l_i| + |l_j| + 2).  The block and final sums
  are float64.
  Gradient: c [A + (k s - R) / (s + eps)] s (1 - s) with A the k-term sum of differences and R the sum of s over the n_in incoming
  edges.  A: a rounded difference (1) and the table errors (8) on every term, k additions: k + 9.  (k s - R) / (s + eps): the
  product (1), the table error of s (4), n_in additions, the subtraction (1), s + eps (4 + 1), the division (1): n_in + 12.  Their
  sum (1), s (4), 1 - s (1, and the 4u s error of s is 4u s / (1 - s) = 4u e^f relative to 1 - s), the products s (1 - s), [..] * that
  and g * c (3), c as an fp32 number (1): max(k + 9, n_in + 12) + 11 + 4 e^f, covered by (k + n_in + 24 + 4 e^f) u * c *
  [sum_slot (|l_i| + |l_j| + 2) + (k s + R) / (s + eps)] s (1 - s).

Edge moments.  S_ab = sum_slot e1_a e2_b: two rounded differences, one product (the addition may be fused), k additions:
  (k + 3) u sum |e1_a| |e2_b|.  Backward g1 = G (sum e2) - sum_in G_src e2: differences (1), k additions inside sum e2, three
  products and two additions per matrix-vector product, n_in subtractions: (k + n_in + 6) u * [|G| sum_slot |e2| + sum_in |G_src| |e2|];
  g2 the same with G^T and e1.

Edge residual.  v = e1 - R e2: |dv_a| <= 5u m_a with m_a = |e1_a| + sum_b |R_ab| |e2_b| (differences, three products, three
  additions).  r = sum |v|^2: (k + 3) u sum |v|^2 + 10 u sum |v_a| m_a + 25 u^2 sum m_a^2 (the last term is what remains of an
  exactly rigid motion, where v itself is rounding).  Backward, with w = 2 g: g1 = w_i sum v - sum_in w_src v:
  (k + n_in + 4) u * [.. |w| |v| ..] + 5 u [.. |w| m ..];  g2 = -w_i R^T sum v + sum_in w_src R_src^T v: (k + n_in + 8) u * [.. |w| |R|^T |v| ..]
  + 5 u [.. |w| |R|^T m ..];  gR_ab = -w_i sum v_a e2_b: (k + 4) u |w| sum |v_a| |e2_b| + 5 u |w| sum m_a |e2_b|."""
import numpy as np

U = 2.0 ** -24
EPS = 1e-10


# ---- k-NN with the (distance, index) order ------------------------------------------------------------------------------
def knn_lex(p1, p2, K, dtype=np.float64):
    """The K nearest rows of p2 for every row of p1, ascending by (squared distance, index); distances are evaluated as
    dx*dx + dy*dy + dz*dz in `dtype`.  Where p2 has fewer than K rows: index 0, distance 0 (pytorch3d's padding)."""
    p1, p2 = np.asarray(p1, dtype=dtype).reshape(-1, 3), np.asarray(p2, dtype=dtype).reshape(-1, 3)
    n1, n2 = len(p1), len(p2)
    idx, dist = np.zeros((n1, K), dtype=np.int64), np.zeros((n1, K), dtype=dtype)
    have = min(K, n2)
    for lo in range(0, n1, 512):
        d = p1[lo:lo + 512, None, :] - p2[None, :, :]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        order = np.argsort(d2, axis=1, kind="stable")[:, :have]          # stable: ties keep ascending index
        idx[lo:lo + 512, :have] = order
        dist[lo:lo + 512, :have] = np.take_along_axis(d2, order, axis=1)
    return dist, idx


# ---- the transposed graph -----------------------------------------------------------------------------------------------
def reverse_graph(idx):
    """(rev_ranges (N, 2), rev_edges (N * k)): edge numbers sorted stably by target; an id outside [0, N) sorts behind every
    row and is in no range."""
    idx = np.asarray(idx).astype(np.int64)
    N, k = idx.shape
    flat = idx.reshape(-1)
    keys = np.where((flat >= 0) & (flat < N), flat, N)
    edges = np.argsort(keys, kind="stable")
    counts = np.bincount(keys, minlength=N + 1)[:N]
    end = np.cumsum(counts)
    ranges = np.stack([end - counts, end], axis=1)
    ranges[counts == 0] = 0
    return ranges.astype(np.int32), edges.astype(np.int32)


def reverse_brute(idx):
    """For every row the list of edge numbers that point at it, by plain loops."""
    idx = np.asarray(idx)
    N, k = idx.shape
    out = [[] for _ in range(N)]
    for e, t in enumerate(idx.reshape(-1).tolist()):
        if 0 <= t < N:
            out[t].append(e)
    return out


def _valid(idx, N):
    idx = np.asarray(idx).astype(np.int64)
    ok = (idx >= 0) & (idx < N)
    return np.where(ok, idx, 0), ok


def _incoming(idx, N):
    """(src, tgt) of every valid edge."""
    j, ok = _valid(idx, N)
    src = np.repeat(np.arange(N), idx.shape[1]).reshape(idx.shape)
    return src[ok], j[ok]


# ---- loss_reg_3d_feature ------------------------------------------------------------------------------------------------
def feat3d(f, idx, g_out=1.0):
    """-> dict(loss, grad (N, D), loss_bound, grad_bound (N, D)) in float64."""
    f = np.asarray(f, dtype=np.float64)
    N, D = f.shape
    k = idx.shape[1]
    j, ok = _valid(idx, N)
    s = 1.0 / (1.0 + np.exp(-f))
    l = np.log(s + EPS)
    okf = ok[:, :, None].astype(np.float64)
    diff = (l[:, None, :] - l[j]) * okf                          # (N, k, D)
    c = 1.0 / (N * k * D)
    loss = c * (s[:, None, :] * diff).sum()
    absterm = (s[:, None, :] * (np.abs(l)[:, None, :] + np.abs(l)[j] + 2.0) * okf).sum()
    loss_bound = (k + 16) * U * c * absterm
    A = diff.sum(1)
    src, tgt = _incoming(idx, N)
    R = np.zeros_like(s)
    np.add.at(R, tgt, s[src])
    n_in = np.bincount(tgt, minlength=N).astype(np.float64)
    nv = ok.sum(1).astype(np.float64)[:, None]
    grad = g_out * c * (A + (nv * s - R) / (s + EPS)) * s * (1.0 - s)
    T = (((np.abs(l)[:, None, :] + np.abs(l)[j] + 2.0) * okf).sum(1) + (nv * s + R) / (s + EPS)) * s * (1.0 - s)
    grad_bound = (k + n_in[:, None] + 24 + 4 * np.exp(f)) * U * c * abs(g_out) * T
    return dict(loss=loss, grad=grad, loss_bound=loss_bound, grad_bound=grad_bound)


# ---- edge ops ---------------------------------------------------------------------------------------------------------------
def _edges(p, idx):
    p = np.asarray(p, dtype=np.float64)
    j, ok = _valid(idx, len(p))
    return (p[:, None, :] - p[j]) * ok[:, :, None]               # (N, k, 3); an edge to nowhere is a zero edge


def edge_moments(p1, p2, idx):
    """-> (S (N, 3, 3), bound (N, 3, 3))."""
    e1, e2 = _edges(p1, idx), _edges(p2, idx)
    k = idx.shape[1]
    S = np.einsum("nka,nkb->nab", e1, e2)
    bound = (k + 3) * U * np.einsum("nka,nkb->nab", np.abs(e1), np.abs(e2))
    return S, bound


def edge_moments_grad(p1, p2, idx, gS):
    """Cotangent gS (N, 3, 3) -> (g1, g2, bound1, bound2), each (N, 3)."""
    N, k = idx.shape
    e1, e2 = _edges(p1, idx), _edges(p2, idx)
    gS = np.asarray(gS, dtype=np.float64)
    j, ok = _valid(idx, N)
    pe1 = np.einsum("nab,nkb->nka", gS, e2) * ok[:, :, None]      # d / d e1 of every edge
    pe2 = np.einsum("nab,nka->nkb", gS, e1) * ok[:, :, None]
    ae1 = np.einsum("nab,nkb->nka", np.abs(gS), np.abs(e2)) * ok[:, :, None]
    ae2 = np.einsum("nab,nka->nkb", np.abs(gS), np.abs(e1)) * ok[:, :, None]
    n_in = np.bincount(j[ok], minlength=N).astype(np.float64)[:, None]
    out = []
    for pe, ae in ((pe1, ae1), (pe2, ae2)):
        g, a = pe.sum(1), ae.sum(1)
        np.subtract.at(g, j[ok], pe[ok])
        np.add.at(a, j[ok], ae[ok])
        out.append((g, (k + n_in + 6) * U * a))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def edge_residual(p1, p2, idx, R):
    """-> (r (N,), bound (N,))."""
    e1, e2 = _edges(p1, idx), _edges(p2, idx)
    R = np.asarray(R, dtype=np.float64)
    k = idx.shape[1]
    v = e1 - np.einsum("nab,nkb->nka", R, e2)
    m = np.abs(e1) + np.einsum("nab,nkb->nka", np.abs(R), np.abs(e2))
    r = (v * v).sum((1, 2))
    bound = (k + 3) * U * r + 10 * U * (np.abs(v) * m).sum((1, 2)) + 25 * U * U * (m * m).sum((1, 2))
    return r, bound


def edge_residual_grad(p1, p2, idx, R, g):
    """Cotangent g (N,) -> dict(g1, g2, gR, b1, b2, bR)."""
    N, k = idx.shape
    e1, e2 = _edges(p1, idx), _edges(p2, idx)
    R = np.asarray(R, dtype=np.float64)
    w = 2.0 * np.asarray(g, dtype=np.float64)
    j, ok = _valid(idx, N)
    okf = ok[:, :, None]
    v = (e1 - np.einsum("nab,nkb->nka", R, e2)) * okf
    m = (np.abs(e1) + np.einsum("nab,nkb->nka", np.abs(R), np.abs(e2))) * okf
    n_in = np.bincount(j[ok], minlength=N).astype(np.float64)[:, None]
    aw = np.abs(w)[:, None, None]
    # p1
    pe1 = w[:, None, None] * v
    g1, a1, c1 = pe1.sum(1), (aw * np.abs(v)).sum(1), (aw * m).sum(1)
    np.subtract.at(g1, j[ok], pe1[ok]); np.add.at(a1, j[ok], (aw * np.abs(v))[ok]); np.add.at(c1, j[ok], (aw * m)[ok])
    b1 = (k + n_in + 4) * U * a1 + 5 * U * c1
    # p2
    pe2 = -w[:, None, None] * np.einsum("nab,nka->nkb", R, v)
    av2 = aw * np.einsum("nab,nka->nkb", np.abs(R), np.abs(v))
    am2 = aw * np.einsum("nab,nka->nkb", np.abs(R), m)
    g2, a2, c2 = pe2.sum(1), av2.sum(1), am2.sum(1)
    np.subtract.at(g2, j[ok], pe2[ok]); np.add.at(a2, j[ok], av2[ok]); np.add.at(c2, j[ok], am2[ok])
    b2 = (k + n_in + 8) * U * a2 + 5 * U * c2
    # R
    gR = -w[:, None, None] * np.einsum("nka,nkb->nab", v, e2)
    bR = np.abs(w)[:, None, None] * ((k + 4) * U * np.einsum("nka,nkb->nab", np.abs(v), np.abs(e2))
                                     + 5 * U * np.einsum("nka,nkb->nab", m, np.abs(e2)))
    return dict(g1=g1, g2=g2, gR=gR, b1=b1, b2=b2, bR=bR)


# ---- the whole rigid loss (torch float64: the SVD's autograd is torch's own, as in the reference) ------------------------------
def rigid_loss(xyz1, xyz2, cluster_ids, num_neighbors, idx_of=None):
    """-> dict(loss, g1, g2, sigma (list of (n, 3) singular values per cluster), edge_scale): the reference's statements
    restated on float64 tensors with knn_lex for the neighbours (or idx_of(cluster position, p1) -> (n, k) indices)."""
    import torch
    x1 = torch.tensor(np.asarray(xyz1, dtype=np.float64), requires_grad=True)
    x2 = torch.tensor(np.asarray(xyz2, dtype=np.float64), requires_grad=True)
    ids = np.asarray(cluster_ids)
    loss = 0
    sigma, edge_scale = [], 0.0
    uniq = np.unique(ids)
    for pos, c in enumerate(uniq.tolist()):
        sel = torch.from_numpy(ids == c)
        p1, p2 = x1[sel], x2[sel]
        if idx_of is None:
            idx = knn_lex(p1.detach().numpy(), p1.detach().numpy(), num_neighbors + 1)[1][:, 1:]
        else:
            idx = np.asarray(idx_of(pos, p1.detach().numpy())).astype(np.int64)
        j = torch.from_numpy(idx)
        e1, e2 = p1[:, None, :] - p1[j], p2[:, None, :] - p2[j]
        S = torch.bmm(e1.transpose(1, 2), e2)
        Um, sig, V = torch.svd(S)
        Rm = torch.bmm(V, Um.transpose(1, 2))
        res = (e1 - torch.bmm(Rm, e2.transpose(1, 2)).transpose(1, 2)).pow(2).sum(2).sum(1)
        loss = loss + res.mean()
        sigma.append(sig.detach().numpy())
        edge_scale += float((e1.detach() ** 2).sum() + (e2.detach() ** 2).sum()) / len(idx)
    loss = loss / len(uniq)
    loss.backward()
    return dict(loss=float(loss.detach()), g1=x1.grad.numpy(), g2=x2.grad.numpy(), sigma=sigma, edge_scale=edge_scale / len(uniq))


# ---- scenes of the exact k-NN tests -----------------------------------------------------------------------------------------
def grid_cloud(kind, n, step, lo, hi, seed):
    """n points whose coordinates are multiples of `step` in [lo, hi): every difference, product and sum of the squared
    distance is exact in fp32 in any order (see max_grid_distance_units).  kind: volume, plane, line, coincident, blobs."""
    g = np.random.default_rng(seed)
    cells = int(round((hi - lo) / step))
    q = g.integers(0, cells, size=(n, 3))
    if kind == "plane":
        q[:, 2] = cells // 2
    elif kind == "line":
        q[:, 1] = cells // 3
        q[:, 2] = cells // 2
    elif kind == "coincident":
        q[:] = q[0]
    elif kind == "blobs":                                    # two distant blobs: the walk must cross the gap
        w = max(2, cells // 16)
        q = g.integers(0, w, size=(n, 3))
        q[n // 2:] += cells - w
    elif kind != "volume":
        raise ValueError(kind)
    return (lo + q * step).astype(np.float32)


def max_grid_distance_units(lo, hi, step):
    """The largest squared distance between two grid points of [lo, hi)^3, in units of step^2: an integer that must stay
    below 2^24 for fp32 to hold every partial sum exactly."""
    cells = int(round((hi - lo) / step))
    return 3 * (cells - 1) ** 2


# ---- distCUDA2 and the narrow k-NN's edge scenes --------------------------------------------------------------------------------
def dist2_lex(points):
    """simple_knn's distCUDA2: for every row the three smallest squared distances to the OTHER rows (other by index: a copy of
    the point counts, with distance 0), fewer where the cloud has fewer than 4 rows.  -> (their sums in float64, the fp32
    value float32(sum) / float32(3), an IEEE division; the mean of three only from 4 rows on, the sum is always divided by 3)."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    sums = np.zeros(n, dtype=np.float64)
    have = min(3, n - 1)
    for lo in range(0, n, 512):
        d = p[lo:lo + 512, None, :] - p[None, :, :]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        rows = np.arange(len(d2))
        d2[rows, lo + rows] = np.inf                                   # not itself
        if have > 0:
            sums[lo:lo + 512] = np.sort(d2, axis=1)[:, :have].sum(axis=1)
    return sums, sums.astype(np.float32) / np.float32(3)


def axis_line_cloud(n, axis, lo, hi, step, seed, include=()):
    """n distinct points of the lattice `step` on the line along `axis` from lo to hi, both end points among them (rows 0 and
    1), so that the cloud's extent is exactly hi - lo along the axis and exactly 0 along the other two (which sit on lattice
    values inside [lo, hi)).  include: offsets from lo (multiples of step) that must be among the points, e.g. cell faces."""
    g = np.random.default_rng(seed)
    cells = int(round((hi - lo) / step))
    fixed = [0, cells] + [int(round(o / step)) for o in include]
    fixed = list(dict.fromkeys(fixed))
    assert len(fixed) <= n <= cells + 1 and all(0 <= f <= cells for f in fixed)
    rest = np.setdiff1d(np.arange(cells + 1), fixed)
    pos = np.concatenate([fixed, g.choice(rest, n - len(fixed), replace=False)]).astype(np.int64)
    pos[2:] = g.permutation(pos[2:])
    q = np.empty((n, 3), dtype=np.int64)
    q[:, (axis + 1) % 3] = cells // 3
    q[:, (axis + 2) % 3] = cells // 2
    q[:, axis] = pos
    return (lo + q * step).astype(np.float32)


def line_cell_width(n, extent, occ=4.0):
    """The cell width knn_params_kernel gives a collinear cloud of n points: h1 = occ * extent / n in fp32 (one multiply, one
    divide), not below extent / 2^20."""
    h = np.float32(np.float32(occ) * np.float32(extent)) / np.float32(n)
    return np.maximum(h, np.float32(extent) * np.float32(1.0 / 1048576.0))


def line_face_disagreements(n, extent, step, occ=4.0):
    """The lattice offsets x in [0, extent] (x = coordinate - origin, exact in fp32) whose cell as the kernels compute it,
    int(fl(x * fl(1 / h))), is not floor(x / h) in float64, with h = line_cell_width(n, extent): the positions on (or within a
    rounding of) a cell face.  -> (offsets in float64, h)."""
    h = line_cell_width(n, extent, occ)
    inv_h = np.float32(1.0) / h
    x = np.arange(int(round(extent / step)) + 1, dtype=np.float64) * step
    x32 = x.astype(np.float32)
    assert np.array_equal(x32.astype(np.float64), x)
    cell32 = (x32 * inv_h).astype(np.int64)
    cell64 = np.floor(x / float(h)).astype(np.int64)
    return x[cell32 != cell64], h
