"""Segmentation after training as HIP kernels (trase_amd/csrc/segment.hip): K-means over the per-Gaussian features and the
query masks built from the clusters.

``kmeans(X, K)`` is ``kmeans_pytorch.kmeans(X, K, distance='euclidean')`` as gui.py:248-270 and gui_standalone.py:685-707
call it (kmeans_pytorch 0.3): numpy draws the K distinct start rows on the host exactly as the library does (so the global
numpy RNG advances the same way), then every Lloyd step runs on the device -- assignment, per-cluster means reduced in a
fixed order, center_shift, the stopping test -- and the host reads the device state word once per ``_BATCH`` steps.
Deliberate deviation: an empty cluster k of iteration i (from 0) is re-seeded with row
``splitmix64(key ^ (i << 32 | k)) mod N`` instead of the library's ``X[torch.randint(N, (1,))]``; ``key`` is ``seed`` when
given, else one draw from torch's default CPU generator (so ``torch.manual_seed`` makes runs repeat).

``segment_mask(features, cluster_ids, segment_ids, score_threshold)`` is render.py:97-105 ``postprocessing`` OR-ed over the
ids as the loop at render.py:334-345 does (also :370-380, gui.py:457-464, :598-607).  It is functional: the reference
normalises the features IN PLACE (``get_gaussian_features`` returns the parameter itself), so its first id of its first
frame takes the query mean from raw features and every later call from normalised ones; callers reproduce that by passing
``F.normalize(features)`` after the first call.

``lift_votes`` / ``prompt_clusters`` / ``pick`` lift a 2D prompt (a mask, or clicked pixels) to the clusters it lands on:
render.py:208-229, gui.py:1039-1064 and gui.py:786-800 as one pass on the device (the lift kernels of
trase_amd/csrc/knn.hip, on top of its spatial hash).  Deliberate deviations: the projection is inverted on the host in
float64 and the un-projection evaluated in float64 (the reference's fp32 ``torch.inverse`` of a znear = 0.01 projection moves
points by up to 4e-4 and with them the nearest index of a fraction of a percent of the pixels), and a negative cluster id
casts no vote where ``torch.bincount`` would raise.

``assign_clusters(features, centres)`` gives every Gaussian the id of its nearest cluster centre by cosine, gui.py:276 +
:288-290 (gui_standalone.py:721-727, the viewer's DBSCAN mode, where the reference copies all features to the host and runs
an N x K x D einsum on the CPU), for clusters that are not K-means ones.

``hdbscan(X, ...)`` / ``density_clusters(features)`` are the viewer's default clustering mode, gui.py:271-301: the core
distances and the minimum spanning tree of the mutual-reachability graph on the device (trase_amd/csrc/hdbscan.hip), the
hierarchy over the n - 1 edges on the host from one read-back (``hdbscan_hierarchy``, plain numpy).  Deliberate deviations:
the centres belong to labels 0..C-1 (the reference's loop is off by one), and among exactly equal weights the spanning tree
follows our edge order.

Only CUDA tensors are accepted: there is no CPU path."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .rasterizer import _stream

_BATCH = 8          # Lloyd steps enqueued per read of the device state word (results do not depend on it)
_MASK64 = (1 << 64) - 1


def _device_index(dev: torch.device) -> int:
    return dev.index if dev.index is not None else torch.cuda.current_device()


def _kmeans_sizes(N: int, D: int, K: int) -> int:
    sz = C.c_size_t()
    _lib.check(_lib.load().trase_kmeans_sizes(N, D, K, C.byref(sz)), "kmeans")
    return sz.value


def _kmeans_steps(X: torch.Tensor, centres: torch.Tensor, ids: torch.Tensor, key: int, tol: float, iter_limit: int,
                  n_steps: int, state: torch.Tensor, ws: torch.Tensor | None = None) -> None:
    """Enqueue ``n_steps`` Lloyd steps on the current stream: ``centres`` (K,D fp32) are updated in place, ``ids`` (N int32)
    receive the assignment of the last step that ran, ``state`` (int32[4]) = {iterations, done, center_shift bits, 0}."""
    N, D = X.shape
    K = centres.shape[0]
    if ws is None:
        ws = torch.empty(_kmeans_sizes(N, D, K), dtype=torch.uint8, device=X.device)
    _lib.check(_lib.load().trase_kmeans_steps(_lib.ptr(X), N, D, K, _lib.ptr(centres), _lib.ptr(ids), int(key) & _MASK64,
                                              float(tol), int(iter_limit), int(n_steps), _lib.ptr(state), _lib.ptr(ws),
                                              ws.numel(), _device_index(X.device), _stream(X.device)), "kmeans")


def kmeans(X: torch.Tensor, num_clusters: int, *, tol: float = 1e-4, iter_limit: int = 0, seed: int | None = None):
    """-> (ids int64 (N,), centres float32 (K, D), iterations), all on X's device."""
    if not torch.is_tensor(X) or X.device.type != "cuda":
        raise RuntimeError("kmeans runs on the GPU only (there is no CPU path)")
    if X.dim() != 2:
        raise ValueError(f"kmeans: X must be (N, D), got {tuple(X.shape)}")
    X = X.detach().float().contiguous()
    N, D = X.shape
    K = int(num_clusters)
    ws = torch.empty(_kmeans_sizes(N, D, K), dtype=torch.uint8, device=X.device)   # validates K, D, N first
    if seed is None:
        indices = np.random.choice(N, K, replace=False)
        key = int(torch.randint(0, 2 ** 62, (1,)).item())
    else:
        np.random.seed(seed)
        indices = np.random.choice(N, K, replace=False)
        key = int(seed)
    centres = X[torch.from_numpy(np.asarray(indices, dtype=np.int64)).to(X.device)].contiguous()
    ids = torch.zeros(N, dtype=torch.int32, device=X.device)
    state = torch.zeros(4, dtype=torch.int32, device=X.device)
    host = torch.empty(4, dtype=torch.int32, pin_memory=True)
    ev = torch.cuda.Event()
    while True:
        _kmeans_steps(X, centres, ids, key, tol, iter_limit, _BATCH, state, ws)
        host.copy_(state, non_blocking=True)
        ev.record(torch.cuda.current_stream(X.device))
        ev.synchronize()
        if int(host[1]):
            break
    return ids.to(torch.int64), centres, int(host[0])


ASSIGN_MAX_CENTRES = 4096      # == LIFT_MAX_BINS: the ids go to lift_votes unchanged


def assign_clusters(features: torch.Tensor, centres: torch.Tensor, *, return_scores: bool = False):
    """-> int64 (N,) ``argmax_k <f_n / |f_n|, c_k>`` on the features' device: gui.py:276 + :288-290.  ``features`` is (N, D) or
    (N, 1, D) fp32, ``centres`` (K, D) on the device or the host, 1 <= K <= 4096, 1 <= D <= 64; the centres are used as given
    (the viewer normalises them at gui.py:286).  Ties go to the lowest k.  A zero feature row gets id 0 (and score 0, its
    norm clamped at 1e-12 as ``F.normalize`` does).  With ``return_scores`` also the winning score, fp32 (N,).  The ids can
    be passed unchanged to ``lift_votes``, ``segment_mask`` and ``display.splat_points``.  Inputs are read, never modified."""
    if not torch.is_tensor(features) or features.device.type != "cuda":
        raise RuntimeError("assign_clusters runs on the GPU only (there is no CPU path)")
    dev = features.device
    if features.dim() == 3 and features.shape[1] == 1:
        features = features.squeeze(1)
    if features.dim() != 2:
        raise ValueError(f"assign_clusters: features must be (N, D) or (N, 1, D), got {tuple(features.shape)}")
    X = features.detach().float().contiguous()
    N, D = X.shape
    centres = torch.as_tensor(centres)
    if centres.dim() != 2 or centres.shape[1] != D:
        raise ValueError(f"assign_clusters: centres must be (K, {D}), got {tuple(centres.shape)}")
    Cn = centres.detach().to(device=dev, dtype=torch.float32).contiguous()
    K = Cn.shape[0]
    lib = _lib.load()
    sz = C.c_size_t()
    _lib.check(lib.trase_assign_clusters_sizes(N, D, K, C.byref(sz)), "assign_clusters")      # validates K, D first
    ws = torch.empty(sz.value, dtype=torch.uint8, device=dev)
    ids = torch.empty(N, dtype=torch.int64, device=dev)
    scores = torch.empty(N, dtype=torch.float32, device=dev) if return_scores else None
    _lib.check(lib.trase_assign_clusters(_lib.ptr(X), N, D, _lib.ptr(Cn), K, _lib.ptr(ids), _lib.ptr(scores),
                                         _lib.ptr(ws) if sz.value else None, ws.numel(), _device_index(dev), _stream(dev)),
               "assign_clusters")
    return (ids, scores) if return_scores else ids


def segment_mask(features: torch.Tensor, cluster_ids: torch.Tensor, segment_ids, score_threshold: float = 0.8) -> torch.Tensor:
    """Boolean (N,) mask of the Gaussians whose cluster is one of ``segment_ids`` and whose fp16 cosine score against that
    cluster's normalised mean feature is >= fp16(score_threshold).  Reads its inputs only."""
    if not torch.is_tensor(features) or features.device.type != "cuda":
        raise RuntimeError("segment_mask runs on the GPU only (there is no CPU path)")
    dev = features.device
    N = features.shape[0]
    X = features.detach().reshape(N, -1).float().contiguous()
    D = X.shape[1]
    ids = cluster_ids.detach().reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
    if ids.numel() != N:
        raise ValueError(f"segment_mask: {ids.numel()} cluster ids for {N} features")
    if torch.is_tensor(segment_ids):
        sel = segment_ids.detach().reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
    else:
        if isinstance(segment_ids, (int, np.integer)):
            segment_ids = [segment_ids]
        sel = torch.tensor([int(s) for s in segment_ids], dtype=torch.int32)
        if sel.numel():
            sel = sel.pin_memory().to(dev, non_blocking=True)
        else:
            sel = sel.to(dev)
    S = int(sel.numel())
    lib = _lib.load()
    sz = C.c_size_t()
    _lib.check(lib.trase_segment_mask_sizes(N, D, S, C.byref(sz)), "segment_mask")
    ws = torch.empty(sz.value, dtype=torch.uint8, device=dev)
    mask = torch.empty(N, dtype=torch.uint8, device=dev)
    thr = float(np.float16(score_threshold))      # as torch rounds a Python float that meets a half tensor
    _lib.check(lib.trase_segment_mask(_lib.ptr(X), N, D, _lib.ptr(ids), _lib.ptr(sel), S, thr, _lib.ptr(mask), _lib.ptr(ws),
                                      ws.numel(), _device_index(dev), _stream(dev)), "segment_mask")
    return mask.view(torch.bool)


# ---- prompt lift: a 2D prompt to cluster votes (render.py:208-229, gui.py:1039-1064; clicked pixels: gui.py:786-800) ---------

LIFT_MAX_BINS = 4096      # the lift kernel's per-block LDS histogram (trase_amd/csrc/knn.hip)


def _lift_call(what, depth, viewpoint_camera, points, *, mask=None, pixels=None, ids=None, bins=0, want_index=False,
               want_points=False):
    """One ``trase_lift_votes`` call -> (votes int32 (bins,) | None, index int32 | None, points fp32 | None)."""
    if not torch.is_tensor(depth) or depth.device.type != "cuda" or not torch.is_tensor(points) or points.device.type != "cuda":
        raise RuntimeError(f"{what} runs on the GPU only (there is no CPU path)")
    dev = depth.device
    W, H = int(viewpoint_camera.image_width), int(viewpoint_camera.image_height)
    if depth.numel() != H * W or depth.dim() not in (2, 3) or tuple(depth.shape[-2:]) != (H, W):
        raise ValueError(f"{what}: depth must be ({H}, {W}) or (1, {H}, {W}), got {tuple(depth.shape)}")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{what}: points must be (N, 3), got {tuple(points.shape)}")
    depth = depth.detach().float().contiguous()
    pts = points.detach().to(dev).float().contiguous()
    N = pts.shape[0]
    # the inverse in float64 of the matrix as stored (one small device-to-host copy unless the camera keeps it on the CPU)
    full = viewpoint_camera.full_proj_transform.detach().to("cpu", torch.float64).numpy()
    if full.shape != (4, 4):
        raise ValueError(f"{what}: full_proj_transform must be (4, 4), got {full.shape}")
    inv = (C.c_double * 16)(*np.linalg.inv(full).reshape(-1).tolist())
    lib = _lib.load()
    sz = C.c_size_t()
    _lib.check(lib.trase_lift_sizes(N, int(bins), C.byref(sz)), what)        # validates bins first
    M = 0
    if mask is not None:
        if not torch.is_tensor(mask) or mask.device.type != "cuda":
            raise RuntimeError(f"{what} runs on the GPU only (there is no CPU path)")
        if mask.numel() != H * W or tuple(mask.shape[-2:]) != (H, W):
            raise ValueError(f"{what}: prompt_mask must be ({H}, {W}), got {tuple(mask.shape)}")
        mask = mask.detach().to(dev)
        mask = (mask if mask.dtype in (torch.bool, torch.uint8) else mask != 0).contiguous().view(torch.uint8)
        n_out = H * W
    else:
        M = n_out = int(pixels.shape[0])
    ws = torch.empty(sz.value, dtype=torch.uint8, device=dev)
    votes = torch.empty(int(bins), dtype=torch.int32, device=dev) if bins else None
    index = torch.empty(n_out, dtype=torch.int32, device=dev) if want_index else None
    out_pts = torch.empty(n_out, 3, dtype=torch.float32, device=dev) if want_points else None
    _lib.check(lib.trase_lift_votes(_lib.ptr(depth), W, H, C.byref(inv), float(viewpoint_camera.znear),
                                    float(viewpoint_camera.zfar), _lib.ptr(mask), _lib.ptr(pixels) if M else None, M,
                                    _lib.ptr(pts) if N else None, N, _lib.ptr(ids) if bins and N else None, int(bins),
                                    _lib.ptr(votes), _lib.ptr(index), _lib.ptr(out_pts), _lib.ptr(ws), ws.numel(),
                                    _device_index(dev), _stream(dev)), what)
    return votes, index, out_pts


def _lift_ids(what, cluster_ids, points, num_clusters):
    ids = cluster_ids.detach().reshape(-1).to(device=points.device, dtype=torch.int32).contiguous()
    if ids.numel() != points.shape[0]:
        raise ValueError(f"{what}: {ids.numel()} cluster ids for {points.shape[0]} points")
    if num_clusters is None:        # as torch.bincount sizes its result: one read-back of the largest id
        bins = max(int(ids.max()) + 1, 1) if ids.numel() else 1
    else:
        bins = int(num_clusters)
    return ids, bins


def lift_votes(depth: torch.Tensor, prompt_mask: torch.Tensor, viewpoint_camera, points: torch.Tensor, cluster_ids: torch.Tensor,
               *, num_clusters: int | None = None, return_index: bool = False, return_points: bool = False):
    """Votes per cluster of a 2D prompt (render.py:208-229, gui.py:1039-1064) in one pass on the device: every pixel of the
    bool / uint8 ``prompt_mask`` (H, W) is un-projected through ``depth`` ((1, H, W) or (H, W), the ``depth`` of ``render()``)
    with the inverse of ``viewpoint_camera.full_proj_transform`` (anything with that, ``image_width``, ``image_height``,
    ``znear``, ``zfar``), its nearest row of ``points`` (N, 3) -- the deformed positions -- is found exactly, and that
    point's cluster id receives one vote.

    -> ``votes`` int64 (bins,), bins = ``num_clusters`` or, when None, the largest id + 1 (one read-back); with
    ``return_index`` also the (H, W) int64 map of nearest indices (-1 where not prompted), with ``return_points`` also the
    (H, W, 3) fp32 un-projected points (0 where not prompted).  At most 4096 bins.  A negative id casts no vote; with
    ``num_clusters`` given, neither does an id >= num_clusters.  Inputs are read, never modified."""
    if not torch.is_tensor(points) or points.device.type != "cuda" or not torch.is_tensor(depth) or depth.device.type != "cuda":
        raise RuntimeError("lift_votes runs on the GPU only (there is no CPU path)")
    ids, bins = _lift_ids("lift_votes", cluster_ids, points, num_clusters)
    H, W = int(viewpoint_camera.image_height), int(viewpoint_camera.image_width)
    votes, index, pts = _lift_call("lift_votes", depth, viewpoint_camera, points, mask=prompt_mask, ids=ids, bins=bins,
                                   want_index=return_index, want_points=return_points)
    votes = votes.to(torch.int64) if votes is not None else torch.zeros(0, dtype=torch.int64, device=depth.device)
    out = (votes,)
    if return_index:
        out += (index.view(H, W).to(torch.int64),)
    if return_points:
        out += (pts.view(H, W, 3),)
    return out[0] if len(out) == 1 else out


def prompt_clusters(depth: torch.Tensor, prompt_mask: torch.Tensor, viewpoint_camera, points: torch.Tensor,
                    cluster_ids: torch.Tensor, threshold, *, num_clusters: int | None = None) -> torch.Tensor:
    """The ids with ``lift_votes(...) > threshold``, ascending, 1-D int64 on the device: what render.py:229-231 prints and
    gui.py:1056-1062 feeds on.  Can be passed straight to ``segment_mask``."""
    votes = lift_votes(depth, prompt_mask, viewpoint_camera, points, cluster_ids, num_clusters=num_clusters)
    return torch.nonzero(votes > threshold).flatten()


def pick(depth: torch.Tensor, pixels, viewpoint_camera, points: torch.Tensor, *, return_points: bool = False):
    """Nearest-point indices, int64 (M,), of the M ``(col, row)`` pixels (an (M, 2) integer tensor, or a sequence of pairs,
    or one pair): the click path of gui.py:786-800.  Pairs given on the host are checked against the image size; a pair
    outside the image in a device tensor gives -1."""
    if not torch.is_tensor(points) or points.device.type != "cuda" or not torch.is_tensor(depth) or depth.device.type != "cuda":
        raise RuntimeError("pick runs on the GPU only (there is no CPU path)")
    dev = depth.device
    W, H = int(viewpoint_camera.image_width), int(viewpoint_camera.image_height)
    if not (torch.is_tensor(pixels) and pixels.device.type == "cuda"):
        host = torch.as_tensor(pixels).reshape(-1, 2).to(torch.int32)
        if host.numel() and (bool((host < 0).any()) or int(host[:, 0].max()) >= W or int(host[:, 1].max()) >= H):
            raise ValueError(f"pick: a pixel lies outside the {W} x {H} image")
        pixels = host.pin_memory().to(dev, non_blocking=True) if host.numel() else host.to(dev)
    if pixels.dim() != 2 or pixels.shape[1] != 2:
        raise ValueError(f"pick: pixels must be (M, 2) (col, row) pairs, got {tuple(pixels.shape)}")
    pixels = pixels.detach().to(torch.int32).contiguous()
    _, index, pts = _lift_call("pick", depth, viewpoint_camera, points, pixels=pixels, want_index=True, want_points=return_points)
    index = index.to(torch.int64)
    return (index, pts) if return_points else index


# ---- HDBSCAN: the viewer's default clustering mode (gui.py:271-301, gui_standalone.py:721-727) --------------------------------

HDBSCAN_MAX_POINTS = 65536      # 16 + 16 index bits in an edge key (trase_amd/csrc/hdbscan.hip)


def hdbscan_hierarchy(edges, n_points: int, *, min_cluster_size: int = 10, cluster_selection_epsilon: float = 0.0,
                      allow_single_cluster: bool = False) -> np.ndarray:
    """Labels, int64 (n_points,), from the n_points - 1 edges ``(i, j, weight)`` of a minimum spanning tree of the
    mutual-reachability graph: the host half of ``hdbscan``, plain numpy, no GPU.  Noise is -1; the clusters are numbered
    0..C-1 by their smallest member index.

    Steps, with the behaviour of the ``hdbscan`` package and of scikit-learn's port: (1) the edges are sorted by weight
    (stably: equal weights keep the order given) and merged into the single-linkage tree by union-find; (2) the tree is
    condensed at ``min_cluster_size``: a split with both sides that large makes two new clusters, otherwise the small side's
    points fall out of the cluster at lambda = 1 / distance; (3) stability of a cluster = sum over what leaves it of
    (lambda - lambda_birth) x size; (4) excess of mass, children before parents: a cluster is kept when its stability is
    at least the sum of its kept descendants'; (5) the root takes no part unless ``allow_single_cluster``; (6) with an
    epsilon, a kept cluster born at a distance below it is replaced by its first ancestor born above it (under the root: the
    last one below it, or the root when a single cluster is allowed); (7) every point takes its nearest kept ancestor."""
    n = int(n_points)
    E = np.asarray(edges, dtype=np.float64).reshape(-1, 3)
    if n < 2 or E.shape[0] != n - 1:
        raise ValueError(f"hdbscan_hierarchy: {n} points need {n - 1} edges, got {E.shape[0]}")
    mcs = int(min_cluster_size)
    if mcs < 2:
        raise ValueError(f"hdbscan_hierarchy: min_cluster_size must be at least 2, got {mcs}")
    eps = float(cluster_selection_epsilon)
    order = np.argsort(E[:, 2], kind="stable")
    ea = E[order, 0].astype(np.int64).tolist()
    eb = E[order, 1].astype(np.int64).tolist()
    ew = E[order, 2].tolist()

    # (1) single linkage: leaves 0..n-1, the k-th merge makes node n + k
    up = list(range(2 * n - 1))
    left = [0] * (n - 1)
    right = [0] * (n - 1)
    size = [1] * n + [0] * (n - 1)

    def find(x):
        r = x
        while up[r] != r:
            r = up[r]
        while up[x] != r:
            up[x], x = r, up[x]
        return r

    for k in range(n - 1):
        ra, rb = find(ea[k]), find(eb[k])
        if ra == rb:
            raise ValueError("hdbscan_hierarchy: the edges do not form a spanning tree")
        node = n + k
        up[ra] = up[rb] = node
        left[k], right[k] = ra, rb
        size[node] = size[ra] + size[rb]

    # the leaves below a node as one slice of `leaves`
    start = [0] * (2 * n - 1)
    for k in range(n - 2, -1, -1):
        node = n + k
        start[left[k]] = start[node]
        start[right[k]] = start[node] + size[left[k]]
    leaves = np.empty(n, dtype=np.int64)
    leaves[np.asarray(start[:n])] = np.arange(n)

    # (2) condensed tree: cluster 0 is the root; a child's id is larger than its parent's
    c_parent, c_birth, c_size = [-1], [0.0], [n]
    p_cluster = np.zeros(n, dtype=np.int64)          # the cluster a point falls out of, and at which lambda
    p_lambda = np.zeros(n, dtype=np.float64)
    todo = [(2 * n - 2, 0)]
    while todo:
        node, c = todo.pop()
        while node >= n:
            k = node - n
            lam = 1.0 / ew[k] if ew[k] > 0.0 else np.inf
            a, b = left[k], right[k]
            big_a, big_b = size[a] >= mcs, size[b] >= mcs
            if big_a and big_b:
                for child in (a, b):
                    c_parent.append(c); c_birth.append(lam); c_size.append(size[child])
                    todo.append((child, len(c_parent) - 1))
                break
            for child, big in ((a, big_a), (b, big_b)):
                if not big:
                    pts = leaves[start[child]:start[child] + size[child]]
                    p_cluster[pts] = c
                    p_lambda[pts] = lam
            if big_a:
                node = a
            elif big_b:
                node = b
            else:
                break
    nc = len(c_parent)
    c_parent = np.asarray(c_parent, dtype=np.int64)
    c_birth = np.asarray(c_birth, dtype=np.float64)
    c_size = np.asarray(c_size, dtype=np.float64)

    # (3) stabilities
    stab = np.zeros(nc, dtype=np.float64)
    np.add.at(stab, p_cluster, p_lambda - c_birth[p_cluster])
    if nc > 1:
        np.add.at(stab, c_parent[1:], (c_birth[1:] - c_birth[c_parent[1:]]) * c_size[1:])
    children = [[] for _ in range(nc)]
    for c in range(1, nc):
        children[c_parent[c]].append(c)

    # (4), (5) excess of mass, children first
    stab = stab.tolist()
    keep = [False] * nc
    for c in range(nc - 1, -1 if allow_single_cluster else 0, -1):
        below = sum(stab[ch] for ch in children[c])
        if below > stab[c]:
            stab[c] = below
        else:
            keep[c] = True
    selected = set()
    stack = [0]
    while stack:                                     # the topmost kept cluster of every branch
        c = stack.pop()
        if keep[c]:
            selected.add(c)
        else:
            stack.extend(children[c])

    # (6) the epsilon rule
    if eps != 0.0 and nc > 1 and selected != {0}:
        merged, done = set(), set()
        for c in sorted(selected):
            if 1.0 / c_birth[c] >= eps:
                merged.add(c)
                continue
            if c in done:
                continue
            top = c
            while True:
                parent = int(c_parent[top])
                if parent == 0:
                    if allow_single_cluster:
                        top = 0
                    break
                top = parent
                if 1.0 / c_birth[top] > eps:
                    break
            merged.add(top)
            stack = list(children[top])
            while stack:
                d = stack.pop()
                done.add(d)
                stack.extend(children[d])
        selected = merged

    # (7) labels: the nearest selected ancestor of the cluster a point fell out of
    owner = np.full(nc, -1, dtype=np.int64)
    for c in range(nc):
        owner[c] = c if c in selected else (owner[c_parent[c]] if c > 0 else -1)
    own = owner[p_cluster]
    if 0 in selected:
        # a single cluster: only the points that stay to the threshold belong to it
        if eps != 0.0:
            threshold = 1.0 / eps
        else:
            from_root = p_lambda[p_cluster == 0]
            threshold = max(from_root.max() if from_root.size else 0.0,
                            max((c_birth[ch] for ch in children[0]), default=0.0))
        own = np.where((own == 0) & (p_lambda < threshold), -1, own)
    labels = np.full(n, -1, dtype=np.int64)
    members = np.nonzero(own >= 0)[0]
    if members.size:
        first = np.full(nc, n, dtype=np.int64)
        np.minimum.at(first, own[members], members)
        ids = np.nonzero(first < n)[0]
        rank = np.empty(nc, dtype=np.int64)
        rank[ids[np.argsort(first[ids], kind="stable")]] = np.arange(ids.size)
        labels[members] = rank[own[members]]
    return labels


def _hdbscan_device(X: torch.Tensor, k: int):
    """The two device passes -> (squared core distances fp32 (n,), int64 (n + 9,): the n edge keys, then the 18 int32
    component counts), on X's device, nothing read back."""
    n, D = X.shape
    lib = _lib.load()
    sz = C.c_size_t()
    _lib.check(lib.trase_hdbscan_sizes(n, D, k, C.byref(sz)), "hdbscan")          # validates n, D, k first
    dev = X.device
    ws = torch.empty(sz.value, dtype=torch.uint8, device=dev)
    core2 = torch.empty(n, dtype=torch.float32, device=dev)
    out = torch.empty(n + 9, dtype=torch.int64, device=dev)                        # n keys, then the 18 counts
    _lib.check(lib.trase_hdbscan_core(_lib.ptr(X), n, D, k, _lib.ptr(core2), _lib.ptr(ws), ws.numel(), _device_index(dev),
                                      _stream(dev)), "hdbscan")
    _lib.check(lib.trase_hdbscan_mst(_lib.ptr(X), n, D, _lib.ptr(core2), _lib.ptr(out), _lib.ptr(out[n:]), _lib.ptr(ws),
                                     ws.numel(), _device_index(dev), _stream(dev)), "hdbscan")
    return core2, out


def _mst_edges(out_host: np.ndarray, n: int) -> np.ndarray:
    """The one read-back of ``_hdbscan_device`` (int64 (n + 9,)) -> float64 (n - 1, 3) rows (i, j, weight), ascending in
    (weight, i, j), i < j."""
    counts = out_host[n:].view(np.int32)
    live = counts[counts > 0]
    if live.size == 0 or live[-1] != 1:
        raise RuntimeError(f"hdbscan: the spanning tree did not close (components per round: {live.tolist()})")
    keys = np.sort(out_host[:n].view(np.uint64))[:n - 1]
    w2 = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32).astype(np.float64)
    if not np.isfinite(w2).all():
        raise ValueError("hdbscan: X has rows that are not finite")
    edges = np.empty((n - 1, 3), dtype=np.float64)
    edges[:, 0] = ((keys >> np.uint64(16)) & np.uint64(0xffff)).astype(np.float64)
    edges[:, 1] = (keys & np.uint64(0xffff)).astype(np.float64)
    edges[:, 2] = np.sqrt(w2)
    return edges


def hdbscan(X: torch.Tensor, *, min_cluster_size: int = 10, min_samples: int | None = None,
            cluster_selection_epsilon: float = 0.0, allow_single_cluster: bool = False, return_mst: bool = False):
    """``hdbscan.HDBSCAN(min_cluster_size, min_samples, cluster_selection_epsilon, allow_single_cluster).fit_predict(X)``
    for the euclidean metric and excess-of-mass selection -> labels int64 (n,) on X's device; noise is -1, the clusters are
    numbered 0..C-1 by their smallest member index.

    ``min_samples`` (None: ``min_cluster_size``) is the package's: the core distance of a row is the distance to its
    ``min_samples``-th nearest OTHER row (scikit-learn counts the row itself: its ``min_samples`` is ours + 1).  The core
    distances and the minimum spanning tree of the mutual-reachability graph are computed on the device in fp32 squared
    distances, ``sum (a_d - b_d)^2`` in dimension order; the n - 1 edges come back in one copy and ``hdbscan_hierarchy`` runs
    on the host.  Among equal weights the tree takes the edge with the lower (min index, max index), where the libraries
    follow their own scan order: partitions can differ from theirs only where distances tie exactly.

    With ``return_mst`` also the (n - 1, 3) float64 edge list ``(i, j, weight)``, i < j, ascending in (weight, i, j), and the
    core distances, float64 (n,), both on X's device: the float64 square roots of the fp32 squared values.
    Limits: 2 <= n <= 65536, 1 <= D <= 64, 1 <= min_samples <= 64, min_samples < n.  Bitwise reproducible."""
    if not torch.is_tensor(X) or X.device.type != "cuda":
        raise RuntimeError("hdbscan runs on the GPU only (there is no CPU path)")
    if X.dim() != 2:
        raise ValueError(f"hdbscan: X must be (n, D), got {tuple(X.shape)}")
    if int(min_cluster_size) < 2:
        raise ValueError(f"hdbscan: min_cluster_size must be at least 2, got {min_cluster_size}")
    X = X.detach().float().contiguous()
    n = X.shape[0]
    k = int(min_cluster_size if min_samples is None else min_samples)
    core2, out = _hdbscan_device(X, k)
    host = torch.empty(n + 9, dtype=torch.int64, pin_memory=True)
    host.copy_(out, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(X.device))
    ev.synchronize()
    edges = _mst_edges(host.numpy(), n)
    labels = hdbscan_hierarchy(edges, n, min_cluster_size=int(min_cluster_size),
                               cluster_selection_epsilon=float(cluster_selection_epsilon),
                               allow_single_cluster=bool(allow_single_cluster))
    labels = torch.from_numpy(labels).to(X.device)
    if return_mst:
        return labels, torch.from_numpy(edges).to(X.device), core2.double().sqrt()
    return labels


def label_centres(X: torch.Tensor, labels: torch.Tensor, num_clusters: int) -> torch.Tensor:
    """-> fp32 (C, D): row c = normalize(mean of the rows of X with label c), gui.py:284-286 without its off-by-one.  A
    label outside [0, C) (noise: -1) belongs to no centre.  1 <= C <= 4096, 1 <= D <= 64."""
    if not torch.is_tensor(X) or X.device.type != "cuda":
        raise RuntimeError("label_centres runs on the GPU only (there is no CPU path)")
    dev = X.device
    X = X.detach().float().contiguous()
    N, D = X.shape
    ids = labels.detach().reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
    if ids.numel() != N:
        raise ValueError(f"label_centres: {ids.numel()} labels for {N} rows")
    Cn = int(num_clusters)
    lib = _lib.load()
    sz = C.c_size_t()
    _lib.check(lib.trase_label_centres_sizes(N, D, Cn, C.byref(sz)), "label_centres")
    ws = torch.empty(sz.value, dtype=torch.uint8, device=dev)
    centres = torch.empty(Cn, D, dtype=torch.float32, device=dev)
    _lib.check(lib.trase_label_centres(_lib.ptr(X), N, D, _lib.ptr(ids), Cn, _lib.ptr(centres), _lib.ptr(ws), ws.numel(),
                                       _device_index(dev), _stream(dev)), "label_centres")
    return centres


def density_clusters(features: torch.Tensor, *, percent: float = 0.02, min_cluster_size: int = 10,
                     cluster_selection_epsilon: float = 0.01, return_sample: bool = False):
    """The viewer's DBSCAN mode, gui.py:274-290, end to end on the device -> (ids int64 (N,), centres fp32 (C, D)).

    The sample is drawn as the reference draws it, ``torch.rand(N) > 1 - percent`` on torch's default CPU generator (so
    ``torch.manual_seed`` reproduces its draw), normalised, clustered by ``hdbscan``; the centres are the normalised means
    of the labelled samples and every Gaussian takes the nearest centre by cosine (``assign_clusters``).  ``features`` is
    (N, D) or (N, 1, D) and is only read.  Deliberate deviation: the reference's centre loop is off by one
    (``cluster_labels == i - 1``: row 0 is the centre of the noise points -- NaN when there are none -- and the last cluster
    gets none); here the centres belong to labels 0..C-1 and noise samples to none.  With ``return_sample`` also the sample's
    indices, int64 (n,), and its labels, int64 (n,).  No cluster found: ValueError."""
    if not torch.is_tensor(features) or features.device.type != "cuda":
        raise RuntimeError("density_clusters runs on the GPU only (there is no CPU path)")
    if features.dim() == 3 and features.shape[1] == 1:
        features = features.squeeze(1)
    if features.dim() != 2:
        raise ValueError(f"density_clusters: features must be (N, D) or (N, 1, D), got {tuple(features.shape)}")
    dev = features.device
    X = features.detach().float()
    index = torch.nonzero(torch.rand(X.shape[0]) > 1 - percent).flatten().to(dev)
    sample = X[index]
    sample = (sample / torch.norm(sample, dim=-1, keepdim=True)).contiguous()
    labels = hdbscan(sample, min_cluster_size=min_cluster_size, cluster_selection_epsilon=cluster_selection_epsilon)
    n_clusters = int(labels.max()) + 1 if labels.numel() else 0
    if n_clusters < 1:
        raise ValueError(f"density_clusters: no cluster among the {sample.shape[0]} sampled rows")
    centres = label_centres(sample, labels, n_clusters)
    ids = assign_clusters(X, centres)
    return (ids, centres, index, labels) if return_sample else (ids, centres)
