"""Losses over a k-NN graph without N x k x ... edge tensors (trase_amd/csrc/neighbors.hip).

The reference's ``loss_reg_3d_feature`` (utils/loss_utils.py:132-152) and ``loss_rigid_body_motion_reg_loss`` (:179-221) call
``pytorch3d.ops.knn_points`` with k + 1 and 129 neighbours and then form ``feats[aux_ids]`` / ``p[aux_ids] - p[ijs]`` tensors of
N x k rows, once more for autograd.  Here the graph is an (N, k) int32 index plus its transpose (``NeighborGraph``), the
forward passes are gather-sums over ``idx`` and the backward passes gather over the transpose for the gradient that flows to
the *neighbour* end of an edge -- no float atomics, so two calls give the same bits.

``edge_moments`` and ``edge_residual`` are the two edge sums of the rigid loss; by default the 3 x 3 SVD between them stays
``torch.svd`` with its own autograd, as in the reference.  ``polar_rotation`` is that rotation as a kernel with its closed-form
gradient (trase_amd/csrc/rigid_math.h), ``rigid_fit`` the three steps in one launch each way, and
``loss_rigid_body_motion_reg_loss(..., rotation="polar")`` the loss over it.

``dense_topk`` (trase_amd/csrc/dense.hip) is the exact all-pairs search at both ends of the distance order that never stores the
M x N matrix; ``loss_feature3d`` (:154-175) and ``loss_cls_3d`` (:89-130) are the two losses of the reference that sit on
``torch.cdist`` + ``topk``, here as gather kernels over its indices."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .rasterizer import _bytes, _stream, knn_points

MAX_FEATURE_DIM = 64
MAX_DENSE_K = 32
MAX_CLASSES = 256


def _dev_index(dev):
    return dev.index if dev.index is not None else torch.cuda.current_device()


def _need_gpu(t, what):
    if t.device.type != "cuda":
        raise RuntimeError(f"{what} runs on the GPU only (there is no CPU path)")


class NeighborGraph:
    """idx (N, k) int32 and its transpose: rev_edges (N * k) holds the edge numbers i * k + slot sorted by the row they point at,
    ascending among the edges of one row; rev_ranges (N, 2) the [begin, end) positions of every row's incoming edges.  An id
    outside [0, N) is an edge to nowhere: it is in no range and contributes to no sum.  With ``num_targets`` the N source rows
    point into that many target rows instead: rev_ranges is (num_targets, 2) and the ids are valid in [0, num_targets)."""

    def __init__(self, idx, rev_ranges, rev_edges):
        self.idx, self.rev_ranges, self.rev_edges = idx, rev_ranges, rev_edges

    @property
    def num_targets(self):
        return self.rev_ranges.shape[0]

    @property
    def N(self):
        return self.idx.shape[0]

    @property
    def k(self):
        return self.idx.shape[1]

    @classmethod
    def from_idx(cls, idx: torch.Tensor, num_targets=None) -> "NeighborGraph":
        _need_gpu(idx, "NeighborGraph")
        if idx.dim() != 2 or idx.shape[1] < 1:
            raise ValueError("NeighborGraph: idx must be (N, k) with k >= 1")
        N, k = idx.shape
        if N * k >= 2 ** 31:
            raise ValueError(f"NeighborGraph: need N * k < 2^31 (got N {N}, k {k})")
        if num_targets is not None and (N < 1 or not 1 <= int(num_targets) < 2 ** 31 - 1):
            raise ValueError(f"NeighborGraph: with num_targets need N >= 1 and 1 <= num_targets < 2^31 - 1 (got N {N}, num_targets {num_targets})")
        if idx.dtype != torch.int32:
            big = torch.iinfo(torch.int32).max
            idx = idx.detach().clamp(-1, big).to(torch.int32)       # what does not fit is out of range either way
        idx = idx.detach().contiguous()
        dev = idx.device
        lib = _lib.load()
        nbytes = C.c_size_t()
        if num_targets is not None:
            T = int(num_targets)
            rev_ranges = torch.empty(T, 2, dtype=torch.int32, device=dev)
            rev_edges = torch.empty(N * k, dtype=torch.int32, device=dev)
            _lib.check(lib.trase_graph_reverse_to_ws_bytes(N, k, T, C.byref(nbytes)), "trase_graph_reverse_to_ws_bytes")
            ws = _bytes(nbytes.value, dev)
            _lib.check(lib.trase_graph_reverse_to(_lib.ptr(idx), N, k, T, _lib.ptr(rev_ranges), _lib.ptr(rev_edges), _lib.ptr(ws),
                                                  ws.numel(), _dev_index(dev), _stream(dev)), "trase_graph_reverse_to")
            return cls(idx, rev_ranges, rev_edges)
        rev_ranges = torch.empty(N, 2, dtype=torch.int32, device=dev)
        rev_edges = torch.empty(N * k, dtype=torch.int32, device=dev)
        _lib.check(lib.trase_graph_reverse_ws_bytes(N, k, C.byref(nbytes)), "trase_graph_reverse_ws_bytes")
        ws = _bytes(nbytes.value, dev)
        _lib.check(lib.trase_graph_reverse(_lib.ptr(idx), N, k, _lib.ptr(rev_ranges), _lib.ptr(rev_edges), _lib.ptr(ws),
                                           ws.numel(), _dev_index(dev), _stream(dev)), "trase_graph_reverse")
        return cls(idx, rev_ranges, rev_edges)

    @classmethod
    def build(cls, points: torch.Tensor, k: int, *, drop_first: bool = True) -> "NeighborGraph":
        """The self-k-NN of ``points`` (N, 3) with K = k + drop_first; drop_first removes column 0 as the reference's
        ``[:, 1:]`` does (with coincident points column 0 is the lowest index among them, not necessarily the point itself)."""
        _need_gpu(points, "NeighborGraph")
        if points.dim() != 2 or points.shape[1] != 3:
            raise ValueError("NeighborGraph.build expects points (N, 3)")
        with torch.no_grad():
            p = points.detach().unsqueeze(0)
            idx = knn_points(p, p, K=int(k) + int(bool(drop_first))).idx[0]
            if drop_first:
                idx = idx[:, 1:]
        return cls.from_idx(idx)


def _f32(t):
    return t.detach().float().contiguous()


class _Feat3D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, graph):
        lib = _lib.load()
        dev = feats.device
        N, D = feats.shape
        f = _f32(feats)
        s_tab, l_tab = torch.empty(N, D, device=dev), torch.empty(N, D, device=dev)
        loss = torch.empty((), device=dev)
        nbytes = C.c_size_t()
        _lib.check(lib.trase_feat3d_ws_bytes(N, D, C.byref(nbytes)), "trase_feat3d_ws_bytes")
        ws = _bytes(nbytes.value, dev)
        _lib.check(lib.trase_feat3d_forward(_lib.ptr(f), _lib.ptr(graph.idx), N, D, graph.k, _lib.ptr(s_tab), _lib.ptr(l_tab),
                                            _lib.ptr(loss), _lib.ptr(ws), ws.numel(), _dev_index(dev), _stream(dev)),
                   "trase_feat3d_forward")
        ctx.save_for_backward(s_tab, l_tab, graph.idx, graph.rev_ranges, graph.rev_edges)
        ctx.meta = (N, D, graph.k, feats.dtype)
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        lib = _lib.load()
        s_tab, l_tab, idx, rev_ranges, rev_edges = ctx.saved_tensors
        N, D, k, dtype = ctx.meta
        dev = s_tab.device
        g = _f32(g_loss).reshape(1)
        g_f = torch.empty(N, D, device=dev)
        _lib.check(lib.trase_feat3d_backward(_lib.ptr(s_tab), _lib.ptr(l_tab), _lib.ptr(idx), _lib.ptr(rev_ranges),
                                             _lib.ptr(rev_edges), N, D, k, _lib.ptr(g), _lib.ptr(g_f), _dev_index(dev),
                                             _stream(dev)), "trase_feat3d_backward")
        return g_f.to(dtype), None


def _check_graph(graph, n, what):
    if not isinstance(graph, NeighborGraph):
        raise TypeError(f"{what}: graph must be a NeighborGraph")
    if graph.N != n:
        raise ValueError(f"{what}: the graph has {graph.N} rows, the input {n}")


def loss_reg_3d_feature(gaussian_feats, gaussian_xyz, k, max_points=-1, *, graph=None):
    """utils/loss_utils.py:132-152: mean over (i, slot, d) of s_i (log(s_i + 1e-10) - log(s_j + 1e-10)), s = sigmoid(feats),
    j the k nearest neighbours of i (column 0 of the k + 1 dropped).  The gradient goes to the features only.  ``graph``: a
    NeighborGraph of the rows actually used (after ``max_points``), to skip the k-NN."""
    _need_gpu(gaussian_feats, "loss_reg_3d_feature")
    if gaussian_feats.dim() != 2 or not 1 <= gaussian_feats.shape[1] <= MAX_FEATURE_DIM:
        raise ValueError(f"loss_reg_3d_feature: features must be (N, D) with 1 <= D <= {MAX_FEATURE_DIM}")
    if gaussian_feats.size(0) > max_points and max_points != -1:
        indices = torch.randperm(gaussian_feats.size(0))[:max_points].to(gaussian_feats.device)
        feats, xyz = gaussian_feats[indices], gaussian_xyz[indices]
    else:
        feats, xyz = gaussian_feats, gaussian_xyz
    if feats.shape[0] < 1:
        raise ValueError("loss_reg_3d_feature: no points")
    if graph is None:
        graph = NeighborGraph.build(xyz, k)
    _check_graph(graph, feats.shape[0], "loss_reg_3d_feature")
    return _Feat3D.apply(feats, graph)


class _EdgeMoments(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p1, p2, graph):
        lib = _lib.load()
        dev = p1.device
        N = p1.shape[0]
        a, b = _f32(p1), _f32(p2)
        S = torch.empty(N, 3, 3, device=dev)
        _lib.check(lib.trase_edge_moments_forward(_lib.ptr(a), _lib.ptr(b), _lib.ptr(graph.idx), N, graph.k, _lib.ptr(S),
                                                  _dev_index(dev), _stream(dev)), "trase_edge_moments_forward")
        ctx.save_for_backward(a, b, graph.idx, graph.rev_ranges, graph.rev_edges)
        ctx.meta = (N, graph.k, p1.dtype, p2.dtype)
        return S

    @staticmethod
    def backward(ctx, gS):
        lib = _lib.load()
        a, b, idx, rev_ranges, rev_edges = ctx.saved_tensors
        N, k, t1, t2 = ctx.meta
        dev = a.device
        g = _f32(gS)
        g1, g2 = torch.empty(N, 3, device=dev), torch.empty(N, 3, device=dev)
        _lib.check(lib.trase_edge_moments_backward(_lib.ptr(a), _lib.ptr(b), _lib.ptr(idx), _lib.ptr(rev_ranges),
                                                   _lib.ptr(rev_edges), N, k, _lib.ptr(g), _lib.ptr(g1), _lib.ptr(g2),
                                                   _dev_index(dev), _stream(dev)), "trase_edge_moments_backward")
        return g1.to(t1), g2.to(t2), None


class _EdgeResidual(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p1, p2, R, graph):
        lib = _lib.load()
        dev = p1.device
        N = p1.shape[0]
        a, b, r = _f32(p1), _f32(p2), _f32(R)
        out = torch.empty(N, device=dev)
        _lib.check(lib.trase_edge_residual_forward(_lib.ptr(a), _lib.ptr(b), _lib.ptr(graph.idx), _lib.ptr(r), N, graph.k,
                                                   _lib.ptr(out), _dev_index(dev), _stream(dev)), "trase_edge_residual_forward")
        ctx.save_for_backward(a, b, r, graph.idx, graph.rev_ranges, graph.rev_edges)
        ctx.meta = (N, graph.k, p1.dtype, p2.dtype, R.dtype)
        return out

    @staticmethod
    def backward(ctx, g_out):
        lib = _lib.load()
        a, b, r, idx, rev_ranges, rev_edges = ctx.saved_tensors
        N, k, t1, t2, tr = ctx.meta
        dev = a.device
        g = _f32(g_out)
        g1, g2, gR = torch.empty(N, 3, device=dev), torch.empty(N, 3, device=dev), torch.empty(N, 3, 3, device=dev)
        _lib.check(lib.trase_edge_residual_backward(_lib.ptr(a), _lib.ptr(b), _lib.ptr(idx), _lib.ptr(rev_ranges),
                                                    _lib.ptr(rev_edges), _lib.ptr(r), N, k, _lib.ptr(g), _lib.ptr(g1),
                                                    _lib.ptr(g2), _lib.ptr(gR), _dev_index(dev), _stream(dev)),
                   "trase_edge_residual_backward")
        return g1.to(t1), g2.to(t2), gR.to(tr), None


def _check_points(p1, p2, what):
    _need_gpu(p1, what)
    if p1.dim() != 2 or p1.shape[1] != 3 or p2.shape != p1.shape or p2.device != p1.device:
        raise ValueError(f"{what}: p1 and p2 must both be (N, 3) on one device")


def edge_moments(p1, p2, graph):
    """S (N, 3, 3) = sum over the slots of e1 e2^T with e = p[i] - p[idx[i, slot]]; differentiable in p1 and p2."""
    _check_points(p1, p2, "edge_moments")
    _check_graph(graph, p1.shape[0], "edge_moments")
    return _EdgeMoments.apply(p1, p2, graph)


def edge_residual(p1, p2, graph, R):
    """(N,) sum over the slots of |e1 - R_i e2|^2; differentiable in p1, p2 and R (N, 3, 3)."""
    _check_points(p1, p2, "edge_residual")
    _check_graph(graph, p1.shape[0], "edge_residual")
    if R.shape != (p1.shape[0], 3, 3) or R.device != p1.device:
        raise ValueError("edge_residual: R must be (N, 3, 3) on the points' device")
    return _EdgeResidual.apply(p1, p2, R, graph)


class _PolarRotation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, S):
        lib = _lib.load()
        dev = S.device
        N = S.shape[0]
        s = _f32(S)
        R = torch.empty(N, 3, 3, device=dev)
        _lib.check(lib.trase_polar3_forward(_lib.ptr(s), N, _lib.ptr(R), _dev_index(dev), _stream(dev)), "trase_polar3_forward")
        ctx.save_for_backward(s, R)
        ctx.dtype = S.dtype
        return R

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gR):
        lib = _lib.load()
        s, R = ctx.saved_tensors
        N = s.shape[0]
        dev = s.device
        g = _f32(gR)
        gS = torch.empty(N, 3, 3, device=dev)
        _lib.check(lib.trase_polar3_backward(_lib.ptr(s), _lib.ptr(R), _lib.ptr(g), N, _lib.ptr(gS), _dev_index(dev), _stream(dev)),
                   "trase_polar3_backward")
        return gS.to(ctx.dtype)


def polar_rotation(S):
    """R (N, 3, 3) = V U^T of S (N, 3, 3) = U Sigma V^T: the orthogonal polar factor of S^T, det R = sign(det S), +1 where det S
    evaluates to 0; a non-finite S gives a NaN R.  Differentiable once, in closed form with the denominators sigma_j + sigma_k
    only; a degenerate row (sigma_2 + sigma_3 <= 12 * 2^-24 |S|_F) gets a zero gradient.  Double backward raises."""
    _need_gpu(S, "polar_rotation")
    if S.dim() != 3 or S.shape[1:] != (3, 3):
        raise ValueError("polar_rotation: S must be (N, 3, 3)")
    return _PolarRotation.apply(S)


class _RigidFit(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p1, p2, graph):
        lib = _lib.load()
        dev = p1.device
        N = p1.shape[0]
        a, b = _f32(p1), _f32(p2)
        out, R = torch.empty(N, device=dev), torch.empty(N, 3, 3, device=dev)
        state = torch.empty(N, _lib.RIGID_STATE_FLOATS, device=dev)
        _lib.check(lib.trase_rigid_fit_forward(_lib.ptr(a), _lib.ptr(b), _lib.ptr(graph.idx), N, graph.k, _lib.ptr(out), _lib.ptr(R),
                                               _lib.ptr(state), _dev_index(dev), _stream(dev)), "trase_rigid_fit_forward")
        ctx.save_for_backward(a, b, R, state, graph.idx, graph.rev_ranges, graph.rev_edges)
        ctx.meta = (N, graph.k, p1.dtype, p2.dtype)
        ctx.mark_non_differentiable(R)
        return out, R

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out, _g_R):
        lib = _lib.load()
        a, b, R, state, idx, rev_ranges, rev_edges = ctx.saved_tensors
        N, k, t1, t2 = ctx.meta
        dev = a.device
        g = _f32(g_out)
        g1, g2 = torch.empty(N, 3, device=dev), torch.empty(N, 3, device=dev)
        _lib.check(lib.trase_rigid_fit_backward(_lib.ptr(a), _lib.ptr(b), _lib.ptr(idx), _lib.ptr(rev_ranges), _lib.ptr(rev_edges),
                                                _lib.ptr(R), _lib.ptr(state), _lib.ptr(g), N, k, _lib.ptr(g1), _lib.ptr(g2),
                                                _dev_index(dev), _stream(dev)), "trase_rigid_fit_backward")
        return g1.to(t1), g2.to(t2), None


def rigid_fit(p1, p2, graph, *, return_rotation=False):
    """(N,) sum over the slots of |e1 - R_i e2|^2 with R_i = polar_rotation(edge_moments(p1, p2, graph))_i, in one launch;
    differentiable (once) in p1 and p2, the dependence of R_i on them included.  return_rotation: also R (N, 3, 3), detached."""
    _check_points(p1, p2, "rigid_fit")
    _check_graph(graph, p1.shape[0], "rigid_fit")
    out, R = _RigidFit.apply(p1, p2, graph)
    return (out, R) if return_rotation else out


def loss_rigid_body_motion_reg_loss(xyz1, xyz2, cluster_ids, num_neighbors=128, max_points=-1, *, rotation="svd"):
    """utils/loss_utils.py:179-221: per cluster, the edges to the num_neighbors nearest points at time 1, the best rotation of
    every point's edge set (SVD of the 3 x 3 moment matrix, R = V U^T) and the mean residual; summed over the clusters and
    divided by their number.  A cluster with fewer points than num_neighbors + 1 gets the k-NN's padding (edges to row 0), as the
    reference would.  One deviation: a cluster whose loss is NaN adds 0 on the device -- no host read, no print.
    rotation: "svd" (the default) is torch.svd and its autograd between the two edge kernels, as the reference has it; "polar"
    is ``rigid_fit``: the same rotation in the kernel with its closed-form gradient, which needs no gap between singular values."""
    if rotation not in ("svd", "polar"):
        raise ValueError(f"loss_rigid_body_motion_reg_loss: rotation must be 'svd' or 'polar' (got {rotation!r})")
    _check_points(xyz1, xyz2, "loss_rigid_body_motion_reg_loss")
    loss = 0
    valid_cluster_ids = torch.unique(cluster_ids)
    for cls in valid_cluster_ids:
        sel = cluster_ids == cls
        p1, p2 = xyz1[sel], xyz2[sel]
        if max_points != -1 and p1.size(0) > max_points:
            indices = torch.randperm(p1.size(0))[:max_points].to(p1.device)
            p1, p2 = p1[indices], p2[indices]
        graph = NeighborGraph.build(p1, num_neighbors)
        if rotation == "polar":
            loss_i = rigid_fit(p1, p2, graph).mean()
        else:
            S_i = edge_moments(p1, p2, graph)
            U_i, _, V_i = torch.svd(S_i)
            R_i = torch.bmm(V_i, U_i.transpose(1, 2))
            loss_i = edge_residual(p1, p2, graph, R_i).mean()
        bad = torch.isnan(loss_i.detach())
        loss = loss + torch.where(bad, torch.zeros_like(loss_i), loss_i)
        # the zero cotangent of a dropped cluster meets NaN on its way back (0 * NaN); the reference leaves such a cluster out
        # of the autograd graph, so its rows get a zero gradient here too
        for p in (p1, p2):
            if p.requires_grad:
                p.register_hook(lambda g, bad=bad: torch.where(bad, torch.zeros_like(g), g))
    return loss / valid_cluster_ids.shape[0]


# ---- the dense search and the two losses over it --------------------------------------------------------------------------------
def _dense_args(queries, points, k_near, k_far, what="dense_topk"):
    for t, name in ((queries, "queries"), (points, "points")):
        if not torch.is_tensor(t) or t.dim() != 2:
            raise ValueError(f"{what}: {name} must be a 2-D tensor")
    if queries.shape[1] != points.shape[1] or not 1 <= points.shape[1] <= MAX_FEATURE_DIM:
        raise ValueError(f"{what}: queries (M, D) and points (N, D) need one D with 1 <= D <= {MAX_FEATURE_DIM}")
    if queries.dtype != torch.float32 or points.dtype != torch.float32:
        raise ValueError(f"{what}: queries and points must be float32")
    k_near, k_far = int(k_near), int(k_far)
    if not (0 <= k_near <= MAX_DENSE_K and 0 <= k_far <= MAX_DENSE_K) or k_near + k_far < 1:
        raise ValueError(f"{what}: need 0 <= k_near, k_far <= {MAX_DENSE_K} and one of them positive (got {k_near}, {k_far})")
    if max(k_near, k_far) > points.shape[0]:
        raise ValueError(f"{what}: k = {max(k_near, k_far)} is larger than the {points.shape[0]} points")
    if queries.shape[0] >= 2 ** 31 or points.shape[0] >= 2 ** 31:
        raise ValueError(f"{what}: need M, N < 2^31")
    if queries.device != points.device:
        raise ValueError(f"{what}: queries and points must be on one device")
    return k_near, k_far


def dense_topk_splits(M, N, D, k_near=0, k_far=0):
    """The number of column ranges S the search of these sizes runs with (S > 1: a merge launch follows the sweep)."""
    nbytes, splits = C.c_size_t(), C.c_int32()
    _lib.check(_lib.load().trase_dense_topk_ws_bytes(M, N, D, k_near, k_far, C.byref(nbytes), C.byref(splits)), "trase_dense_topk_ws_bytes")
    return splits.value


def dense_topk(queries, points, k_near=0, k_far=0):
    """For every row of ``queries`` (M, D) the k_near nearest and the k_far farthest rows of ``points`` (N, D), exactly, without the
    M x N matrix -> (near_d2 (M, k_near) fp32, near_idx (M, k_near) int64, far_d2 (M, k_far), far_idx (M, k_far)).  Squared
    distances are the chain s = fmaf(q_d - p_d, q_d - p_d, s) in dimension order.  Near end: smaller distance first, then lower
    id; far end: larger distance first, then lower id; a NaN distance ranks above +inf (last near, first far).  k > N raises
    ValueError.  Not differentiable."""
    k_near, k_far = _dense_args(queries, points, k_near, k_far)
    _need_gpu(queries, "dense_topk")
    dev = queries.device
    M, D = queries.shape
    N = points.shape[0]
    near_d2, far_d2 = torch.empty(M, k_near, device=dev), torch.empty(M, k_far, device=dev)
    near_idx = torch.empty(M, k_near, dtype=torch.int64, device=dev)
    far_idx = torch.empty(M, k_far, dtype=torch.int64, device=dev)
    if M == 0:
        return near_d2, near_idx, far_d2, far_idx
    q, p = queries.detach().contiguous(), points.detach().contiguous()
    lib = _lib.load()
    nbytes = C.c_size_t()
    _lib.check(lib.trase_dense_topk_ws_bytes(M, N, D, k_near, k_far, C.byref(nbytes), None), "trase_dense_topk_ws_bytes")
    ws = _bytes(nbytes.value, dev)
    _lib.check(lib.trase_dense_topk(_lib.ptr(q), M, _lib.ptr(p), N, D, k_near, k_far,
                                    _lib.ptr(near_d2) if k_near else None, _lib.ptr(near_idx) if k_near else None,
                                    _lib.ptr(far_d2) if k_far else None, _lib.ptr(far_idx) if k_far else None,
                                    _lib.ptr(ws), nbytes.value, _dev_index(dev), _stream(dev)), "trase_dense_topk")
    return near_d2, near_idx, far_d2, far_idx


def _dpad(D):
    return 8 if D <= 8 else 16 if D <= 16 else 32 if D <= 32 else 64


class _Feature3D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, graph, kp, kn, lambda_p, lambda_n):
        lib = _lib.load()
        dev = feats.device
        rows, D = feats.shape
        f = _f32(feats)
        u_tab, nrm = torch.empty(rows, _dpad(D), device=dev), torch.empty(rows, device=dev)
        loss = torch.empty((), device=dev)
        nbytes = C.c_size_t()
        _lib.check(lib.trase_feature3d_ws_bytes(rows, C.byref(nbytes)), "trase_feature3d_ws_bytes")
        ws = _bytes(nbytes.value, dev)
        _lib.check(lib.trase_feature3d_forward(_lib.ptr(f), _lib.ptr(graph.idx), rows, D, kp, kn, lambda_p, lambda_n, _lib.ptr(u_tab),
                                               _lib.ptr(nrm), _lib.ptr(loss), _lib.ptr(ws), ws.numel(), _dev_index(dev), _stream(dev)),
                   "trase_feature3d_forward")
        ctx.save_for_backward(u_tab, nrm, graph.idx, graph.rev_ranges, graph.rev_edges)
        ctx.meta = (rows, D, kp, kn, lambda_p, lambda_n, feats.dtype)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss):
        lib = _lib.load()
        u_tab, nrm, idx, rev_ranges, rev_edges = ctx.saved_tensors
        rows, D, kp, kn, lambda_p, lambda_n, dtype = ctx.meta
        dev = u_tab.device
        g = _f32(g_loss).reshape(1)
        g_f = torch.empty(rows, D, device=dev)
        _lib.check(lib.trase_feature3d_backward(_lib.ptr(u_tab), _lib.ptr(nrm), _lib.ptr(idx), _lib.ptr(rev_ranges), _lib.ptr(rev_edges),
                                                rows, D, kp, kn, lambda_p, lambda_n, _lib.ptr(g), _lib.ptr(g_f), _dev_index(dev),
                                                _stream(dev)), "trase_feature3d_backward")
        return g_f.to(dtype), None, None, None, None, None


def _k_ok(what, name, k):
    if int(k) != k or not 1 <= int(k) <= MAX_DENSE_K:
        raise ValueError(f"{what}: need 1 <= {name} <= {MAX_DENSE_K} (got {k})")
    return int(k)


def loss_feature3d(gaussian_feats, gaussian_xyz, kp=16, kn=4, max_points=10000, lambda_p=1.0, lambda_n=1.0, *, neighbors=None):
    """utils/loss_utils.py:154-175: lambda_p * mean over (i, slot < kp) of sigmoid(1 - cos(f_i, f_j)), j the kp nearest rows of i in
    xyz (the row itself included, as cdist + topk has it), plus lambda_n * mean over (i, slot < kn) of sigmoid(cos(f_i, f_j)), j
    the kn farthest rows; cos(a, b) = (a / max(|a|, 1e-8)) . (b / max(|b|, 1e-8)).  The gradient goes to the features only.
    max_points: an integer is the reference's rule (more rows than that: torch.randperm(N)[:max_points] on the CPU generator);
    None uses every row -- the search never holds the N x N matrix.  neighbors: (near_idx (rows, kp), far_idx (rows, kn)) of the
    rows actually used, to skip the search."""
    what = "loss_feature3d"
    if not torch.is_tensor(gaussian_feats) or gaussian_feats.dim() != 2 or not 1 <= gaussian_feats.shape[1] <= MAX_FEATURE_DIM:
        raise ValueError(f"{what}: features must be (N, D) with 1 <= D <= {MAX_FEATURE_DIM}")
    kp, kn = _k_ok(what, "kp", kp), _k_ok(what, "kn", kn)
    if max_points is not None and (int(max_points) != max_points or max_points < 1):
        raise ValueError(f"{what}: max_points must be a positive integer or None (got {max_points!r})")
    if not torch.is_tensor(gaussian_xyz) or gaussian_xyz.dim() != 2 or gaussian_xyz.shape[0] != gaussian_feats.shape[0] \
            or not 1 <= gaussian_xyz.shape[1] <= MAX_FEATURE_DIM:
        raise ValueError(f"{what}: xyz must be (N, 1..{MAX_FEATURE_DIM}) with the features' N")
    rows = gaussian_feats.shape[0] if max_points is None else min(gaussian_feats.shape[0], int(max_points))
    if rows < 1 or rows >= 2 ** 25:
        raise ValueError(f"{what}: need 1 <= rows < 2^25 (got {rows})")
    if max(kp, kn) > rows:
        raise ValueError(f"{what}: kp = {kp} / kn = {kn} is larger than the {rows} rows")
    if neighbors is not None:
        if len(neighbors) != 2 or tuple(neighbors[0].shape) != (rows, kp) or tuple(neighbors[1].shape) != (rows, kn):
            raise ValueError(f"{what}: neighbors must be (near_idx ({rows}, {kp}), far_idx ({rows}, {kn}))")
    _need_gpu(gaussian_feats, what)
    if max_points is not None and gaussian_feats.size(0) > max_points:
        indices = torch.randperm(gaussian_feats.size(0))[:max_points].to(gaussian_feats.device)
        feats, xyz = gaussian_feats[indices], gaussian_xyz[indices]
    else:
        feats, xyz = gaussian_feats, gaussian_xyz
    if neighbors is None:
        x = _f32(xyz)
        _, near_idx, _, far_idx = dense_topk(x, x, kp, kn)
    else:
        near_idx, far_idx = neighbors
    graph = NeighborGraph.from_idx(torch.cat([near_idx.to(feats.device), far_idx.to(feats.device)], dim=1))
    return _Feature3D.apply(feats, graph, kp, kn, float(lambda_p), float(lambda_n))


class _Cls3D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, preds, sample, graph, sgraph, lambda_val):
        lib = _lib.load()
        dev = preds.device
        N, Cn = preds.shape
        S, k = graph.idx.shape
        p = _f32(preds)
        loss = torch.empty((), device=dev)
        nbytes = C.c_size_t()
        _lib.check(lib.trase_cls3d_ws_bytes(S, Cn, C.byref(nbytes)), "trase_cls3d_ws_bytes")
        ws = _bytes(nbytes.value, dev)
        _lib.check(lib.trase_cls3d_forward(_lib.ptr(p), _lib.ptr(sample), _lib.ptr(graph.idx), S, N, Cn, k, lambda_val, _lib.ptr(loss),
                                           _lib.ptr(ws), ws.numel(), _dev_index(dev), _stream(dev)), "trase_cls3d_forward")
        ctx.save_for_backward(p, sample, graph.idx, graph.rev_ranges, graph.rev_edges, sgraph.rev_ranges, sgraph.rev_edges)
        ctx.meta = (S, N, Cn, k, lambda_val, preds.dtype)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss):
        lib = _lib.load()
        p, sample, idx, rev_ranges, rev_edges, srev_ranges, srev_edges = ctx.saved_tensors
        S, N, Cn, k, lambda_val, dtype = ctx.meta
        dev = p.device
        g = _f32(g_loss).reshape(1)
        g_p = torch.empty(N, Cn, device=dev)
        _lib.check(lib.trase_cls3d_backward(_lib.ptr(p), _lib.ptr(sample), _lib.ptr(idx), _lib.ptr(rev_ranges), _lib.ptr(rev_edges),
                                            _lib.ptr(srev_ranges), _lib.ptr(srev_edges), S, N, Cn, k, lambda_val, _lib.ptr(g),
                                            _lib.ptr(g_p), _dev_index(dev), _stream(dev)), "trase_cls3d_backward")
        return g_p.to(dtype), None, None, None, None


def loss_cls_3d(features, predictions, k=5, lambda_val=2.0, max_points=200000, sample_size=800, *, sample=None):
    """utils/loss_utils.py:89-130: lambda_val / (S k C) * sum over (s, slot, c) of p_s (log(p_s + 1e-10) - log(p_j + 1e-10)) over S
    sampled rows s and their k nearest rows j in FEATURE space (the sampled row itself is slot 0).  More than max_points rows
    are first cut down with torch.randperm(N)[:max_points], the sample is torch.randperm(N)[:sample_size], both on the CPU
    generator as in the reference; ``sample`` (an index tensor into the rows left after max_points) replaces the second draw.
    The gradient goes to ``predictions`` only."""
    what = "loss_cls_3d"
    if not torch.is_tensor(features) or features.dim() != 2 or not 1 <= features.shape[1] <= MAX_FEATURE_DIM:
        raise ValueError(f"{what}: features must be (N, D) with 1 <= D <= {MAX_FEATURE_DIM}")
    if not torch.is_tensor(predictions) or predictions.dim() != 2 or predictions.shape[0] != features.shape[0] \
            or not 1 <= predictions.shape[1] <= MAX_CLASSES:
        raise ValueError(f"{what}: predictions must be (N, C) with the features' N and 1 <= C <= {MAX_CLASSES}")
    k = _k_ok(what, "k", k)
    if int(max_points) != max_points or max_points < 1 or int(sample_size) != sample_size or sample_size < 1:
        raise ValueError(f"{what}: max_points and sample_size must be positive integers")
    N = min(features.shape[0], int(max_points))
    if N < 1 or N * predictions.shape[1] >= 2 ** 31:
        raise ValueError(f"{what}: need N >= 1 and N * C < 2^31 (got N {N}, C {predictions.shape[1]})")
    if k > N:
        raise ValueError(f"{what}: k = {k} is larger than the {N} rows")
    if sample is not None:
        if not torch.is_tensor(sample) or sample.dim() != 1 or sample.numel() < 1 or sample.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{what}: sample must be a non-empty 1-D int32 / int64 index tensor")
    _need_gpu(features, what)
    dev = features.device
    if features.size(0) > max_points:
        indices = torch.randperm(features.size(0))[:max_points].to(dev)
        features, predictions = features[indices], predictions[indices]
    if sample is None:
        sample = torch.randperm(features.size(0))[:sample_size]
    sample = sample.to(dev)
    if int(sample.min()) < 0 or int(sample.max()) >= N:
        raise ValueError(f"{what}: sample holds an index outside [0, {N})")
    f = _f32(features)
    _, idx, _, _ = dense_topk(f[sample.long()], f, k_near=k)
    graph = NeighborGraph.from_idx(idx, num_targets=N)
    sample32 = sample.to(torch.int32).contiguous()
    sgraph = NeighborGraph.from_idx(sample32.reshape(-1, 1), num_targets=N)
    return _Cls3D.apply(predictions, sample32, graph, sgraph, float(lambda_val))
