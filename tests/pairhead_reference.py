"""TEST INFRASTRUCTURE ONLY -- float64 statement of the FEATURE-state contrastive pair head (train.py:251-296) with every
discrete quantity the kernels of csrc/pairhead.hip derive on the way, and seeded scenes on which those quantities have one
right answer.

The statement is written from utils/feature_utils.py:28-57 and utils/loss_utils.py:275-406 independently of
oracle/feature_head_oracle.py; tests/test_pairhead_reference.py pins the two against each other and against
tests/golden/feature_head.npz.  Only the pair weights are taken from the oracle (``O.pixel_weights``, float32): that IS the
reference's arithmetic, and the kernel follows it operation by operation.

Lattice features: every pixel's 32 channels hold 16 entries of +-1 and 16 zeros, so |f|^2 = 16, the normalised entries are
+-0.25 and every similarity is a multiple of 1/16 -- exact in float32 in any summation order and identical in float64.  The
thresholds 0.75 and 0.5 lie on the lattice: ties occur by the hundreds, and every strict comparison has one right answer.
"""
import functools
import types

import numpy as np
import torch

from oracle import feature_head_oracle as O

MODES = ("soft", "all", "hard")
MARGIN = 4.0                    # device error / float32-oracle error (tests/test_gpu_mlp_precise.py, test_gpu_vgg.py, the smoothing tests)
LATTICE_HW = (24, 40)
PROBE_HW = (32, 40)
S_EDGES = (2, 3, 31, 32, 33, 63, 64, 65, 255, 256, 257, 320, 513)
# (N, sampled masks, sampled masks with index < 256 or None for a seeded scatter).  257/256: the one mask left out has index 100,
# so rank 255 falls on mask 256; 600/255: 31 sampled masks in the first trip of the rank scan, so ranks 31 and 32 straddle the
# carry and every rank from 31 up lies on a mask with index >= 256; 600/1: rank 0 on a mask with index >= 256.
PROBE_CASES = ((1, 1, None), (7, 7, None), (8, 8, None), (9, 9, None), (31, 31, None), (32, 32, None), (33, 33, None),
               (64, 64, None), (65, 65, None), (255, 255, None), (256, 256, None), (257, 256, 255), (300, 37, None),
               (600, 255, 31), (600, 1, 0))


def f32(x):
    """the float64 value rounded once to float32"""
    return np.float32(float(x))


def ulp32(x):
    """one float32 unit in the last place at magnitude |x| (the smallest normal's for 0)"""
    x = abs(float(x))
    if not np.isfinite(x):
        return float("nan")
    return float(np.spacing(np.float32(max(x, float(np.finfo(np.float32).tiny)))))


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def _lattice_vectors(n, g):
    """n vectors of 32 channels: 16 entries of +-1 at random places, 16 zeros"""
    v = torch.zeros(n, 32)
    for k in range(n):
        idx = torch.randperm(32, generator=g)[:16]
        v[k, idx] = torch.randint(0, 2, (16,), generator=g).float() * 2 - 1
    return v


@functools.lru_cache(maxsize=None)
def lattice_scene(S, N, n_sampled, seed, uncovered=None, nth_plant=0.5):
    """(features (32, H, W), sam_masks (N, H, W), sampled_pixel (H, W), sampled_mask (N,)) on the CPU, H x W = 24 x 40.
    Masks are seeded rectangles; a pixel takes the lattice pattern of its first covering mask (pixels no mask covers share one
    more pattern) with 12 % of its signs flipped.  ``uncovered``: None samples S pixels at random; a fraction q makes exactly
    round(q * S) of the sampled pixels ones that no mask covers.  From S = 31 up one sampled pixel that belongs to no sampled mask
    -- the one with the highest index -- gets a fresh lattice vector whose similarity to every other sampled pixel is <=
    ``nth_plant`` (and, when the search finds one, == nth_plant for at least one): its 'soft' negative column flag is raised by
    its own diagonal entry alone.  Returned tensors are shared: do not modify them."""
    H, W = LATTICE_HW
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    cy, cx = torch.randint(0, H, (N,), generator=g), torch.randint(0, W, (N,), generator=g)
    ry, rx = torch.randint(1, 6, (N,), generator=g), torch.randint(1, 8, (N,), generator=g)
    sam = ((yy[None] - cy[:, None, None]).abs() <= ry[:, None, None]) & ((xx[None] - cx[:, None, None]).abs() <= rx[:, None, None])
    sm = torch.zeros(N, dtype=torch.bool)
    sm[torch.randperm(N, generator=g)[:n_sampled]] = True
    base = _lattice_vectors(N + 1, g)
    covered = sam.any(0)
    first = torch.where(covered, sam.float().argmax(0), torch.full((H, W), N))
    feat = base[first].permute(2, 0, 1).clone()
    feat = torch.where(torch.rand(32, H, W, generator=g) < 0.12, -feat, feat)
    perm = torch.randperm(H * W, generator=g)
    if uncovered is None:
        chosen = perm[:S]
    else:
        n_un = int(round(uncovered * S))
        cov = covered.reshape(-1)[perm]
        chosen = torch.cat([perm[~cov][:n_un], perm[cov][:S - n_un]])
        assert chosen.numel() == S, "not enough pixels of one kind"
    sp = torch.zeros(H * W, dtype=torch.bool)
    sp[chosen] = True
    if S >= 31:
        in_sampled = sam[sm].any(0).reshape(-1)
        cand = torch.nonzero(sp & ~in_sampled).reshape(-1)
        assert cand.numel() > 0, "no sampled pixel outside the sampled masks"
        j = int(cand[-1])
        others = feat.reshape(32, -1)[:, sp & (torch.arange(H * W) != j)].T          # (S - 1, 32)
        best = None
        for _ in range(4000):
            v = _lattice_vectors(1, g)[0]
            sims = others @ v / 16.0
            if float(sims.max()) <= nth_plant:
                best = v if best is None else best
                if float(sims.max()) == nth_plant:
                    best = v
                    break
        assert best is not None, "no lattice vector below the negative threshold against every other sampled pixel"
        feat.reshape(32, -1)[:, j] = best
    return feat.contiguous(), sam.contiguous(), sp.view(H, W), sm


def edge_args(S):
    """lattice_scene arguments of the S-edge scene: 14 masks, 7 of them sampled, seed S.  The two smallest take only covered
    pixels and a seed found by search, so that their one and three pairs are active with distinct, non-zero a."""
    return {2: (2, 14, 7, 20, 0.0), 3: (3, 14, 7, 503, 0.0)}.get(S, (S, 14, 7, S))


def planted_pixel(features, sam_masks, sampled_pixel, sampled_mask):
    """flat index and sample index of lattice_scene's planted pixel (the last sampled pixel outside the sampled masks)"""
    sp = sampled_pixel.reshape(-1)
    cand = torch.nonzero(sp & ~sam_masks[sampled_mask].any(0).reshape(-1)).reshape(-1)
    j = int(cand[-1])
    return j, int(sp[:j].sum())


@functools.lru_cache(maxsize=None)
def probe_scene(N, n_sampled, seed, first_trip=None):
    """Planted pairs on 32 x 40: mask n covers exactly pixels 2n and 2n + 1 of the flattened image and a run of 0..39 pixels in an
    unsampled tail (so the sizes differ); all 2 * min(N, H * W / 2) probe pixels are sampled and every pixel has its own random
    lattice vector.  C then has exactly 2 * n_sampled positive off-diagonal entries, and a lost, aliased or misplaced membership
    bit changes an integer count.  ``first_trip``: how many of the sampled masks have an index below 256 (None: seeded scatter)."""
    H, W = PROBE_HW
    HW = H * W
    g = torch.Generator().manual_seed(seed)
    sam = torch.zeros(N, HW, dtype=torch.bool)
    P = min(N, HW // 2)
    for n in range(P):
        sam[n, 2 * n] = sam[n, 2 * n + 1] = True
    room = HW - 2 * P
    for n in range(N):
        k = int(torch.randint(0, 40, (1,), generator=g))
        if room > 40:
            lo = 2 * P + (n * 7) % (room - 40)
            sam[n, lo:lo + k] = True
    sm = torch.zeros(N, dtype=torch.bool)
    if first_trip is None:
        sm[torch.randperm(N, generator=g)[:n_sampled]] = True
    else:
        lo_n = min(N, 256)
        sm[torch.randperm(lo_n, generator=g)[:first_trip]] = True
        sm[256 + torch.randperm(N - 256, generator=g)[:n_sampled - first_trip]] = True
    feat = _lattice_vectors(HW, g).T.reshape(32, H, W).contiguous()
    sp = torch.zeros(HW, dtype=torch.bool)
    sp[:2 * P] = True
    assert int(sm.sum()) == n_sampled
    return feat, sam.view(N, H, W), sp.view(H, W), sm


@functools.lru_cache(maxsize=None)
def one_mask_scene(S, seed):
    """One sampled mask, every a equal: two masks of the same size, the left and the right half of the image, of which only the
    left one is sampled.  Every pixel is covered by exactly one mask of H * W / 2 pixels, so w_max = 1 and the reference's
    (w - min) / (max - min) is 0 / 0 for every pair; pairs inside the left half are positive, all others negative."""
    H, W = LATTICE_HW
    g = torch.Generator().manual_seed(seed)
    feat = _lattice_vectors(H * W, g).T.reshape(32, H, W).contiguous()
    sp = torch.zeros(H * W, dtype=torch.bool)
    sp[torch.randperm(H * W, generator=g)[:S]] = True
    sam = torch.zeros(2, H, W, dtype=torch.bool)
    sam[0, :, :W // 2] = True
    sam[1, :, W // 2:] = True
    return feat, sam, sp.view(H, W), torch.tensor([True, False])


def upsampled(features):
    """the (32, 2h, 2w) nearest-neighbour x2 image: ATen's bilinear resize of it back to (h, w) (align_corners=False) blends, per
    axis, two taps of one source block with weights 0.5 and 0.5, so it returns ``features`` bit for bit"""
    return features.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2).contiguous()


def spread_x2(grad):
    """what the resized head's gradient must be on upsampled(features): each (32, h, w) entry times 0.25 at its four taps"""
    return (grad * 0.25).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2).contiguous()


# ---- the statement --------------------------------------------------------------------------------------------------------------
def mean_mask_size(sam_masks, sampled_pixel):
    """a: per sampled pixel, the mean size of the masks covering it (utils/feature_utils.py:30-31), float32 like the reference"""
    size = sam_masks.reshape(sam_masks.shape[0], -1).sum(1)
    tot = (sam_masks * size[:, None, None]).sum(0)
    return (tot / (sam_masks.sum(0) + 1e-9))[sampled_pixel]


def weights_from_a(a):
    """the S x S weights as the kernel derives them from a alone (pair_weight of csrc/pairhead.hip), in float32"""
    a = a.float()
    P = a.max() * a.max()
    nz = a[a > 0]
    wmax = torch.clamp(P / (nz.min() * nz.min()), 1.0, None) if nz.numel() else torch.tensor(1.0)
    pm = a[:, None] * a[None, :]
    pm = torch.where(pm == 0, torch.tensor(1e10), pm)
    w = torch.clamp(P / pm, 1.0, None)
    return (w - 1.0) / (wmax - 1.0) * 9.0 + 1.0


def statement(features, sam_masks, sampled_pixel, sampled_mask, mode, pth, nth, use_weights, g_pos=1.0, g_neg=1.0, drop=None):
    """The head in float64.  ``drop`` = (i, j), i < j: the same with that one pair taken out of both masked sums (sensitivity).
    -> namespace: loss_pos, loss_neg, pos_similarity, neg_similarity (float64 tensors), N_pos, N_neg (ints: out8[1], out8[3]),
    colP, colN (bool [S]; None in 'hard', which has no column flags), a (float32 [S]), member (bool [S, sampled masks], column k =
    the k-th sampled mask = bit k), C (bool S x S), C_F, W (float64 S x S), dCF (S x S, d loss / d C_F, upper triangle),
    active (bool [S]: the row takes part in a pair with a non-zero coefficient), grad (32, H, W) float64 and its sampled rows
    ``rows`` (S, 32), fn (S, 32) normalised features, rinv [S], S, n_sampled."""
    assert mode in MODES
    sp, sm = sampled_pixel.bool(), sampled_mask.bool()
    pth, nth = float(np.float32(pth)), float(np.float32(nth))          # the C entry points take the thresholds as float
    x = features.double()[:, sp].T.clone().requires_grad_(True)
    S = x.shape[0]
    fn = torch.nn.functional.normalize(x, dim=-1, p=2)
    CF = fn @ fn.T
    CF.retain_grad()
    member = sam_masks[sm][:, sp].T.contiguous()
    C = (member.double() @ member.double().T) != 0
    W = O.pixel_weights(sam_masks, sp).double() if use_weights else torch.ones(S, S, dtype=torch.float64)
    upper = torch.triu(torch.ones(S, S, dtype=torch.bool), diagonal=1)
    idx = torch.arange(S)
    cf = CF.detach()
    if mode == "hard":
        colP = colN = None
        mP, mN = upper & C & (cf < pth), upper & ~C & (cf > nth)
        N_pos, N_neg = int(mP.sum()), int(mN.sum())
    else:
        colP = (C if mode == "all" else C & (cf < pth)).any(0)          # over ALL rows: the diagonal and the lower triangle count
        colN = (~C if mode == "all" else ~C & (cf > nth)).any(0)
        N_pos, N_neg = int(idx[colP].sum()), int(idx[colN].sum())       # pairs i < j of a flagged column j: j of them
        mP, mN = upper & colP[None, :] & C, upper & colN[None, :] & ~C
    if drop is not None:
        mP, mN = mP.clone(), mN.clone()
        mP[drop] = mN[drop] = False
    zero = CF.sum() * 0.0 + 0.0                     # (+0.0 whatever the sign of the sum)
    # indexed first, multiplied second, like utils/loss_utils.py: an undefined (NaN) weight then reaches the selected pairs only
    loss_pos = (-W[mP] * CF[mP]).sum() / N_pos if N_pos > 0 else zero
    loss_neg = (W[mN] * torch.relu(CF[mN])).sum() / N_neg if N_neg > 0 else zero
    (g_pos * loss_pos + g_neg * loss_neg).backward()
    dCF = CF.grad.clone()
    grad = torch.zeros(32, sp.numel(), dtype=torch.float64)
    grad[:, sp.reshape(-1)] = x.grad.T
    nz = (dCF != 0) | dCF.isnan()
    return types.SimpleNamespace(
        loss_pos=loss_pos.detach(), loss_neg=loss_neg.detach(), pos_similarity=cf[C].mean(), neg_similarity=cf[~C].mean(),
        N_pos=N_pos, N_neg=N_neg, colP=colP, colN=colN, a=mean_mask_size(sam_masks, sp), member=member, C=C, C_F=cf, W=W, dCF=dCF,
        active=nz.any(0) | nz.any(1), grad=grad.view(32, *sp.shape), rows=x.grad.detach().clone(), fn=fn.detach(),
        rinv=1.0 / x.detach().norm(dim=1).clamp_min(1e-12), S=S, n_sampled=int(sm.sum()))


def float32_error(features, sam_masks, sampled_pixel, sampled_mask, mode, pth, nth, use_weights, ref, g_pos=1.0, g_neg=1.0):
    """What the pinned oracle makes of the same inputs in float32 (O.head(dtype=torch.float32) + autograd), against the float64
    statement ``ref``.  -> namespace of absolute errors: loss_pos, loss_neg, pos_similarity, neg_similarity (floats) and rows
    ([S]: per sampled pixel, the largest error over its 32 gradient entries)."""
    f = features.float().clone().requires_grad_(True)
    lp, ln, ps, ns = O.head(f, sam_masks, sampled_pixel, sampled_mask, mode, float(np.float32(pth)), float(np.float32(nth)),
                            use_weights, dtype=torch.float32)
    (g_pos * lp + g_neg * ln).backward()
    rows = f.grad.double()[:, sampled_pixel].T
    return types.SimpleNamespace(
        loss_pos=abs(float(lp.detach()) - float(ref.loss_pos)), loss_neg=abs(float(ln.detach()) - float(ref.loss_neg)),
        pos_similarity=abs(float(ps) - float(ref.pos_similarity)), neg_similarity=abs(float(ns) - float(ref.neg_similarity)),
        rows=(rows - ref.rows).abs().amax(dim=1))


def scalar_bar(err32, value):
    """4 x the float32 oracle's error + one float32 ulp of the quantity"""
    return MARGIN * err32 + ulp32(value)


def row_bars(err32_rows, ref_rows):
    """[S]: per sampled pixel, 4 x the float32 oracle's error on that row + one float32 ulp of the row's largest magnitude"""
    top = ref_rows.abs().amax(dim=1)
    ulp = torch.from_numpy(np.spacing(np.maximum(top.numpy().astype(np.float32), np.finfo(np.float32).tiny)).astype(np.float64))
    return MARGIN * err32_rows + ulp


def row_forward_bounds(ref):
    """[S]: a forward error bound of ph_bwd + ph_scatter for each sampled pixel's gradient row, from the float32 format alone
    (u = 2^-24).  Entry c of d_t = sum_u coef(t, u) f_u[c] is accumulated by serial fmas over chunks of per = ceil(S / 32) pairs
    and the 32 chunk partials are added serially: with T_c = sum_u |coef| |f_u[c]|, |delta d_c| <= (per + 32 + 3) u T_c (3: the
    roundings inside coef = g / N * w).  proj = <f, d> adds sum_c |f_c| |delta d_c| + 7 u sum_c |f_c d_c| (32 products, a five-level
    shuffle tree), and v = r (d - f proj) three more roundings:
        |delta v_c| <= r u T [ (per + 35) + |f|_inf |f|_1 (per + 42) + 3 (1 + |f|_inf |f|_1) ],   T = max_c T_c.
    It is relative to the sum of the pairs' magnitudes, not to the row's own largest entry, which cancellation can make far smaller:
    that is where the kernel's fixed order may lose a few ulp of the row against torch's blocked sums."""
    u, per = 2.0 ** -24, (ref.S + 31) // 32
    c = ref.dCF.abs()
    c = torch.nan_to_num(c + c.T, nan=0.0)
    fa = ref.fn.abs()
    T = (c @ fa).amax(dim=1)
    ff = fa.amax(dim=1) * fa.sum(dim=1)
    return ref.rinv * u * T * ((per + 35) + ff * (per + 42) + 3 * (1 + ff))


@functools.lru_cache(maxsize=None)
def reference(builder, args, mode, pth, nth, use_weights):
    """(scene, statement, float32 error) of ``builder(*args)``, computed once per process and shared: read-only"""
    scene = {"lattice": lattice_scene, "probe": probe_scene, "one_mask": one_mask_scene}[builder](*args)
    ref = statement(*scene, mode, pth, nth, use_weights)
    return scene, ref, float32_error(*scene, mode, pth, nth, use_weights, ref)


def pair_moves(ref):
    """For the sensitivity condition: (move_i, move_j), both S x S -- the largest change among the 32 gradient entries of row i
    (of row j) when the single pair (i, j), i < j, is taken out of the masked sums (statement(..., drop=(i, j))), in closed form:
    row i moves by r_i c_ij (f_j - f_i <f_i, f_j>) and row j by r_j c_ij (f_i - f_j <f_i, f_j>), c = dCF.  Zero where the pair is
    inactive; also zero for an active pair of parallel vectors (<f_i, f_j> = +-1), whose contribution the normalisation projects out."""
    fn, cf = ref.fn, ref.C_F
    c = ref.dCF.abs()
    t_i = (fn[None, :, :] - fn[:, None, :] * cf[:, :, None]).abs().amax(dim=2)          # [i, j]: f_j - f_i <f_i, f_j>
    return ref.rinv[:, None] * c * t_i, ref.rinv[None, :] * c * t_i.T
