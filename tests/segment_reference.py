"""Float64 restatement of the segmentation stage (trase_amd/segment.py, trase_amd/csrc/segment.hip): the K-means loop of
kmeans_pytorch 0.3 (gui.py:248-270) with this project's empty-cluster rule, and the query mask of render.py:97-105 +
render.py:334-345.

* ``lloyd_step`` / ``kmeans_loop``: argmin of the float64 squared distances (ties to the lowest index, as torch.argmin),
  float64 means, center_shift = sum_k |c_k - c_k_prev|, stop when shift^2 < tol or iter_limit is reached.  The returned ids
  are those of the last assignment, made against the centres that iteration started from.
* ``reseed_row``: cluster k empty in iteration i (from 0) takes row splitmix64(key ^ (i << 32 | k)) mod N.
* ``query_mask``: the fp16 scoring of postprocessing -- rows and query normalised, both rounded to fp16, the dot product
  exact (float64 of fp16 operands) then rounded to fp32 and to fp16, compared with fp16(threshold).
* ``lattice_rows`` / ``lattice_start`` / ``lattice_step``: one Lloyd step on small-integer rows, where fp32 is exact in any
  order, so the device's ids and centres have one right answer bit for bit; ``SHAPE_PLAN`` lists the (K, D, N) at which
  tests/test_gpu_segment_shapes.py takes that step, ``LOCKSTEP_CASES`` / ``BLOB_CASES`` the real-valued cases of the same file.
* ``library_kmeans`` / ``render_masks_torch``: the library's own torch composition (an N x K x D broadcast per iteration,
  one ``nonzero`` per cluster) and the render.py loop as torch ops, for timing on the same device.

A plain module (no HIP library): it runs on whatever device its tensors live on.
"""
from __future__ import annotations

from typing import NamedTuple

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


# ---- one exact Lloyd step on an integer lattice ----------------------------------------------------------------------------
#
# Rows drawn from {-span..span}^D and start centres that are rows: every product, every partial sum of |c|^2 and x.c and
# |c|^2 - 2 x.c is an integer of magnitude <= 3 * 64 * span^2 < 2^24, so the device's fp32 distances are exact and its argmin
# is THE argmin, ties to the lowest k.  Every per-cluster sum is an integer of magnitude <= N * span < 2^24 (N <= 200 000,
# span = 4), exact in fp32 whatever the order of the additions, and the count is too; sum / count is one correctly rounded
# fp32 division.  Nothing is left to a tolerance but center_shift (a sum of square roots).

def lattice_rows(n: int, d: int, seed: int, span: int = 4) -> torch.Tensor:
    """(n, d) fp32 rows of integers drawn uniformly from {-span..span}."""
    return torch.from_numpy(np.random.default_rng(seed).integers(-span, span + 1, (n, d)).astype(np.float32))


class ShapeCase(NamedTuple):
    K: int
    D: int
    N: int
    dup: bool = False         # start centres K-1 and (K >= 4) 2 repeat centres 0 and 1: tie families, then empty clusters
    offset: bool = False      # also run on a copy of X that starts 4 bytes into its storage (the scalar row loads)

    @property
    def id(self) -> str:
        return f"K{self.K}-D{self.D}-N{self.N}" + ("-dup" if self.dup else "") + ("-offset" if self.offset else "")


def _tail_cases():
    # (K, D) with wacc = 3, 5, 6, 7 accumulating waves, i.e. sub-ranges of 171, 103, 86, 74 rows: one tile of a sub-range
    # - 1, + 0, + 1 rows, and blocks of 512 + r rows (N = 256 (512 + r) - s: second tiles of r rows, r - s in the last block)
    out = []
    for K, D, per in ((128, 64, 171), (80, 64, 103), (72, 64, 86), (64, 64, 74)):
        out += [ShapeCase(K, D, per + e) for e in (-1, 0, 1)]
        out += [ShapeCase(K, D, 256 * 514 - 1), ShapeCase(K, D, 256 * 517 - 2)]
    return out


SHAPE_PLAN = [
    # every D class and K class against the 512-row tile
    ShapeCase(1, 1, 1), ShapeCase(2, 3, 511), ShapeCase(3, 4, 512, offset=True), ShapeCase(3, 8, 513), ShapeCase(2, 9, 1024),
    ShapeCase(3, 12, 1025), ShapeCase(127, 16, 127), ShapeCase(3, 17, 16 * 512 + 1), ShapeCase(4, 20, 16 * 512),
    ShapeCase(127, 31, 1025), ShapeCase(128, 32, 128, offset=True), ShapeCase(2, 33, 513), ShapeCase(3, 36, 511),
    ShapeCase(127, 63, 512), ShapeCase(2, 64, 513, offset=True), ShapeCase(96, 64, 1024), ShapeCase(64, 64, 64),
    # 256 blocks: one full tile each; a second tile of one row and a short last block; chunk = 782
    ShapeCase(128, 64, 131072), ShapeCase(5, 8, 131073), ShapeCase(128, 64, 131073), ShapeCase(1, 64, 200_000),
    ShapeCase(128, 8, 200_000),
    # duplicate start centres in every padded width, and at K = 128
    ShapeCase(8, 5, 600, dup=True), ShapeCase(16, 12, 700, dup=True), ShapeCase(9, 31, 1500, dup=True),
    ShapeCase(128, 64, 1025, dup=True),
] + _tail_cases()


def lattice_start(X: torch.Tensor, case: ShapeCase) -> torch.Tensor:
    """(K, D) start centres for a plan case: K distinct rows of X (all of them, permuted, when N == K), with the duplicates
    ``case.dup`` asks for."""
    g = np.random.default_rng(1000 * case.K + case.D)
    C = X[torch.from_numpy(g.choice(case.N, case.K, replace=False))].clone()
    if case.dup:
        C[case.K - 1] = C[0]
        if case.K >= 4:
            C[2] = C[1]
    return C


def lattice_case(case: ShapeCase):
    """-> (rows, start centres) of a plan case, on the CPU."""
    X = lattice_rows(case.N, case.D, seed=1000 * case.D + case.K)
    return X, lattice_start(X, case)


def lattice_step(X: torch.Tensor, C: torch.Tensor, iteration: int, key: int):
    """One Lloyd step from integer centres C on integer rows X, as fp32 arithmetic must give it whatever its order
    -> (ids int64 (N,), new centres fp32 (K, D), empty bool (K,), center_shift in float64 of those fp32 centres).

    The (N, K) scores |c_k|^2 - 2 x.c_k come from float64 matrix products in row chunks (exact on these integers)."""
    x = X.cpu().double()
    c = C.cpu().double()
    N, K = x.shape[0], c.shape[0]
    assert bool((x == x.round()).all()) and bool((c == c.round()).all()), "lattice_step: integer rows and centres only"
    cc = (c * c).sum(1)
    assert float(3 * torch.maximum((x * x).sum(1).max(), cc.max())) < 2 ** 24
    ids = torch.empty(N, dtype=torch.int64)
    for a in range(0, N, 1 << 16):
        score = cc[None, :] - 2.0 * (x[a:a + (1 << 16)] @ c.T)
        ids[a:a + score.shape[0]] = torch.from_numpy(np.argmin(score.numpy(), axis=1))      # the first of equal minima
    sums = torch.zeros(K, x.shape[1], dtype=F64).index_add_(0, ids, x)
    counts = torch.bincount(ids, minlength=K)
    assert float(sums.abs().max()) < 2 ** 24 and N < 2 ** 24
    empty = counts == 0
    new = torch.from_numpy(sums.numpy().astype(np.float32) / np.maximum(counts.numpy(), 1).astype(np.float32)[:, None])
    for k in torch.nonzero(empty).flatten().tolist():
        new[k] = X.cpu()[reseed_row(key, iteration, k, N)]
    shift = float(torch.sqrt(((new.double() - c) ** 2).sum(1)).sum())
    return ids, new, empty, shift


# ---- real-valued cases away from D = 32 -------------------------------------------------------------------------------------

LOCKSTEP_N, LOCKSTEP_ITERS = 5000, 6
LOCKSTEP_CASES = [(128, 64, True), (127, 63, True), (128, 8, True), (17, 5, True), (2, 3, True), (3, 1, False)]   # K, D, unit rows


def lockstep_rows(K: int, D: int, unit: bool):
    """-> (rows fp32 (LOCKSTEP_N, D) on the CPU, start row indices) of a lockstep case."""
    x = torch.randn(LOCKSTEP_N, D, generator=torch.Generator().manual_seed(1000 * K + D))
    if unit:
        x = torch.nn.functional.normalize(x, dim=-1)
    return x, init_indices(LOCKSTEP_N, K, seed=7)


def near_tie_gap(X: torch.Tensor) -> float:
    """The squared-distance gap below which the fp32 assignment may differ from the float64 one: the device forms
    |c|^2 - 2 x.c from two D-term fmaf chains and one more fma, each with a relative error of at most D 2^-24 on terms
    bounded by M^2 (M the largest row norm, which also bounds every centre); two such distances are compared:
    8 (D + 1) 2^-24 M^2.  1.6e-5 for unit rows at D = 32."""
    M = float(X.double().norm(dim=-1).max())
    return 8.0 * (X.shape[1] + 1) * 2.0 ** -24 * M * M


def near_tie_cap(n: int) -> int:
    """Rows an iteration may leave out of the id comparison as near ties."""
    return max(2, int(1e-3 * n))


BLOB_N = 4000
BLOB_CASES = [(5, 3, 0.05, 3), (128, 64, 0.05, 3)]        # K, D, noise, seed


def blob_rows(n: int, k: int, d: int, noise: float, seed: int):
    """n rows around k unit-norm blob centres; the start rows numpy will draw for ``seed`` lie in k distinct blobs
    -> (rows fp32 on the CPU, blob labels, start row indices)."""
    start = init_indices(n, k, seed)
    g = np.random.default_rng(seed)
    centres = g.standard_normal((k, d))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    labels = g.integers(0, k, n)
    labels[start] = np.arange(k)
    rows = centres[labels] + noise * g.standard_normal((n, d))
    return torch.from_numpy(rows.astype(np.float32)), labels, start


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
