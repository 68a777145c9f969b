"""Float64 restatement of the segmentation stage (trase_amd/segment.py, trase_amd/csrc/segment.hip): the K-means loop of
kmeans_pytorch 0.3 (gui.py:248-270) with this project's empty-cluster rule, and the query mask of render.py:97-105 +
render.py:334-345.

* ``lloyd_step`` / ``kmeans_loop``: argmin of the float64 squared distances (ties to the lowest index, as torch.argmin),
  float64 means, center_shift = sum_k |c_k - c_k_prev|, stop when shift^2 < tol or iter_limit is reached.  The returned ids
  are those of the last assignment, made against the centres that iteration started from.
* ``reseed_row``: cluster k empty in iteration i (from 0) takes row splitmix64(key ^ (i << 32 | k)) mod N.
* ``query_mask``: the fp16 scoring of postprocessing -- rows and query normalised, both rounded to fp16, the dot product
  exact (float64 of fp16 operands) then rounded to fp32 and to fp16, compared with fp16(threshold).
* ``library_kmeans`` / ``render_masks_torch``: the library's own torch composition (an N x K x D broadcast per iteration,
  one ``nonzero`` per cluster) and the render.py loop as torch ops, for timing on the same device.

A plain module (no HIP library): it runs on whatever device its tensors live on.
"""
from __future__ import annotations

import numpy as np
import torch

F64 = torch.float64
_M64 = (1 << 64) - 1


def splitmix64(x: int) -> int:
    """splitmix64 output for state x (the golden-ratio increment added first)."""
    z = (x + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def reseed_row(key: int, iteration: int, k: int, n: int) -> int:
    return splitmix64((int(key) & _M64) ^ ((int(iteration) << 32) | int(k))) % n


def init_indices(n: int, k: int, seed=None) -> np.ndarray:
    """kmeans_pytorch's ``initialize``: numpy's global RNG, seeded first when a seed is given."""
    if seed is not None:
        np.random.seed(seed)
    return np.random.choice(n, k, replace=False)


def distances(X: torch.Tensor, C: torch.Tensor) -> torch.Tensor:
    """(N, K) float64 squared distances, in row chunks."""
    X = X.to(F64)
    C = C.to(F64)
    out = torch.empty(X.shape[0], C.shape[0], dtype=F64, device=X.device)
    cc = (C * C).sum(1)
    for a in range(0, X.shape[0], 1 << 16):
        x = X[a:a + (1 << 16)]
        out[a:a + x.shape[0]] = ((x * x).sum(1, keepdim=True) - 2.0 * (x @ C.T) + cc).clamp_min(0.0)
    return out


def assign(X: torch.Tensor, C: torch.Tensor):
    """-> (ids int64, gap) with gap = second-smallest minus smallest squared distance (inf for K = 1)."""
    d = distances(X, C)
    ids = torch.argmin(d, dim=1)
    if C.shape[0] < 2:
        return ids, torch.full_like(d[:, 0], float("inf"))
    two = torch.topk(d, 2, dim=1, largest=False).values
    return ids, two[:, 1] - two[:, 0]


def update(X: torch.Tensor, ids: torch.Tensor, C_prev: torch.Tensor, iteration: int, key: int):
    """float64 centres from an assignment (empty clusters re-seeded) and center_shift against C_prev."""
    X64 = X.to(F64)
    K, D = C_prev.shape
    sums = torch.zeros(K, D, dtype=F64, device=X.device).index_add_(0, ids.to(X.device), X64)
    counts = torch.bincount(ids.to(X.device), minlength=K).to(F64)
    C = sums / counts.clamp_min(1.0)[:, None]
    for k in torch.nonzero(counts == 0).flatten().tolist():
        C[k] = X64[reseed_row(key, iteration, k, X.shape[0])]
    shift = float(torch.sqrt(((C - C_prev.to(F64)) ** 2).sum(1)).sum())
    return C, shift


def lloyd_step(X: torch.Tensor, C: torch.Tensor, iteration: int, key: int):
    """One iteration from centres C -> (ids, gap, new centres, center_shift)."""
    ids, gap = assign(X, C)
    C_new, shift = update(X, ids, C, iteration, key)
    return ids, gap, C_new, shift


def stop(shift: float, iteration_after: int, tol: float, iter_limit: int) -> bool:
    return shift ** 2 < tol or (iter_limit != 0 and iteration_after >= iter_limit)


def kmeans_loop(X: torch.Tensor, indices, key: int, tol: float = 1e-4, iter_limit: int = 0, max_iter: int = 1000):
    """The whole loop from start rows X[indices] -> (ids of the last assignment, centres, iterations)."""
    C = X.to(F64)[torch.as_tensor(np.asarray(indices), dtype=torch.int64, device=X.device)]
    it = 0
    while True:
        ids, _, C, shift = lloyd_step(X, C, it, key)
        it += 1
        if stop(shift, it, tol, iter_limit) or it >= max_iter:
            return ids, C, it


def _f16(v: torch.Tensor) -> torch.Tensor:
    return v.to(torch.float32).to(torch.float16).to(F64)


def query_mask(score_rows: torch.Tensor, query_rows: torch.Tensor, ids: torch.Tensor, segment_ids, threshold: float = 0.8):
    """OR over segment_ids of (ids == id) & (fp16 score >= fp16 threshold) -> (mask bool, fp32-rounded score).

    ``score_rows`` are the features the scores are taken of, ``query_rows`` those the cluster means are taken of (the same
    tensor except for the reference's first call, see trase_amd/segment.py)."""
    f = score_rows.to(F64)
    fn = _f16(f / f.norm(dim=-1, keepdim=True))
    ids = ids.reshape(-1).to(f.device)
    thr = float(np.float16(threshold))
    mask = torch.zeros(f.shape[0], dtype=torch.bool, device=f.device)
    score32 = torch.full((f.shape[0],), float("nan"), dtype=F64, device=f.device)
    for sid in segment_ids:
        pre = ids == int(sid)
        if sid < 0 or not bool(pre.any()):
            continue
        q = query_rows.to(F64)[pre].mean(0)
        qh = _f16(q / q.norm())
        s32 = (fn[pre] @ qh).to(torch.float32).to(F64)
        score32[pre] = s32
        mask[pre] = _f16(s32) >= thr
    return mask, score32


def render_frames(features: torch.Tensor, ids: torch.Tensor, id_lists, threshold: float = 0.8):
    """The render.py:334-345 loop over frames as written, with the in-place normalisation of the features the scores are
    taken of: the first id of the first frame takes its query from the raw rows, every later one from normalised rows."""
    rows = features.to(F64).clone()
    normalised = False
    masks = []
    for segment_ids in id_lists:
        mask = torch.zeros(rows.shape[0], dtype=torch.bool, device=rows.device)
        for sid in segment_ids:
            m, _ = query_mask(rows, rows, ids, [sid], threshold)
            mask |= m
            if not normalised:
                rows = rows / rows.norm(dim=-1, keepdim=True)
                normalised = True
        masks.append(mask)
    return masks


# ---- the library's torch composition, for timing ------------------------------------------------------------------------

def library_kmeans(X: torch.Tensor, num_clusters: int, tol: float = 1e-4, iter_limit: int = 0, seed=None):
    """kmeans_pytorch 0.3's loop on X's device: (N,1,D) - (1,K,D) broadcast, argmin, then per cluster a nonzero +
    index_select + mean (one host sync each); an empty cluster takes a random row."""
    X = X.float()
    indices = init_indices(X.shape[0], num_clusters, seed)
    state = X[indices]
    it = 0
    while True:
        dis = ((X.unsqueeze(1) - state.unsqueeze(0)) ** 2.0).sum(dim=-1).squeeze()
        choice = torch.argmin(dis, dim=1)
        prev = state.clone()
        for index in range(num_clusters):
            sel = torch.nonzero(choice == index).squeeze().to(X.device)
            sel = torch.index_select(X, 0, sel)
            if sel.shape[0] == 0:
                sel = X[torch.randint(len(X), (1,))]
            state[index] = sel.mean(dim=0)
        shift = torch.sum(torch.sqrt(torch.sum((state - prev) ** 2, dim=1)))
        it += 1
        if shift ** 2 < tol:
            break
        if iter_limit != 0 and it >= iter_limit:
            break
    return choice, state, it


def render_masks_torch(features: torch.Tensor, ids: torch.Tensor, segment_ids, threshold: float = 0.8) -> torch.Tensor:
    """render.py's per-id composition as torch ops on the device (on a copy of the features)."""
    f = features.clone()
    out = None
    for sid in segment_ids:
        pre = ids == sid
        q = f[pre].mean(dim=0)
        f /= f.norm(dim=-1, keepdim=True)
        q = q / q.norm()
        scores = (f.half() @ q.half().unsqueeze(-1))[:, 0]
        post = pre & (scores >= threshold)
        out = post if out is None else out | post
    return out
