"""Float64 statement of the NNFM style loss (trase_amd/csrc/nnfm.hip) and an emulation of its two-candidate short-list.

``reference(f1, f2)``: mean_i min_j (1 - cos(f1_i, f2_j)) in float64 with its analytic gradient with respect to f1, each row's
argmax and the margins to the second and third columns.

``emulate(f1, f2)``: what nnfm.hip computes, as far as a host can know it.  Columns are normalised in fp32
(x * (1 / sqrt(sum x^2))), rounded to bf16, and multiplied in float64; the ``keep`` largest products of a row (ties -> lowest
column) are its short-list, and the float64 cosines of the ORIGINAL data decide inside the list (ties -> lowest column, as
nnfm_finish_kernel).  The device accumulates the products in fp32 in an order of its own and decides with fp32 cosines, so a
row's outcome is only **decided** when

* its second and third emulated products differ by more than ``acc_bound(C) = 2 C 2^-24``: the largest difference between two
  fp32-accumulated sums of C products of unit vectors in any order, so the short-list is the same SET on the device, and
* the float64 cosines of the two listed columns differ by more than ``FP32_MARGIN = 1e-6`` (the project's margin for a
  decision taken in fp32).

Neither the fp32 norm nor its summation order can be reproduced bit for bit, so ``nudge`` moves every element whose
fp32-normalised value lies within 4 fp32 ulps of a bf16 rounding tie by one part in 2^12 of itself until none is left: on such
input the device rounds every element to the same bf16 value as the emulation.

The inputs of tests/test_gpu_nnfm_forms.py are built here (seeded, deterministic, no fixture file) and their premises are
asserted without a GPU by tests/test_nnfm_reference.py."""
import functools

import numpy as np
import torch

FP32_MARGIN = 1e-6            # two cosines further apart than this are told apart by an fp32 evaluation (tests/test_gpu_nnfm.py)
ROW_BAR = 1e-4                # gradient rows: max |got - want| over the row / max |want| over the matrix (tests/test_gpu_nnfm.py)
MAX_EXCLUDED = 0.01           # share of rows that may have a float64 margin <= FP32_MARGIN


def loss_tol(ref_loss):
    """the loss bar of tests/test_gpu_nnfm.py"""
    return 2e-7 * max(1.0, abs(ref_loss)) + 1e-7


def acc_bound(c):
    return 2.0 * c * 2.0 ** -24


# ---- float64 ---------------------------------------------------------------------------------------------------------------
def cosines(f1, f2):
    """(N1, N2) float64 cosines of the columns of f1 (C, N1) and f2 (C, N2)"""
    a, b = np.asarray(f1, np.float64), np.asarray(f2, np.float64)
    return (a / np.linalg.norm(a, axis=0)).T @ (b / np.linalg.norm(b, axis=0))


def grad_toward(f1, f2, cols):
    """d/d f1 of mean_i (1 - cos(f1_i, f2_cols[i])), (C, N1) float64:  -(n2_j - cos n1_i) / (|f1_i| N1)"""
    a, b = np.asarray(f1, np.float64), np.asarray(f2, np.float64)[:, cols]
    na = np.linalg.norm(a, axis=0)
    n1, n2 = a / na, b / np.linalg.norm(b, axis=0)
    cs = (n1 * n2).sum(axis=0)
    return -(n2 - cs * n1) / (na * a.shape[1])


def reference(f1, f2):
    """-> dict(loss, grad (C, N1), argmax (N1,), cos (N1, N2), best (N1,), margin2, margin3 (N1,): best minus the second / third
    largest cosine, +inf where N2 has no such column)"""
    cos = cosines(f1, f2)
    n1, n2 = cos.shape
    order = np.argsort(-cos, axis=1, kind="stable")                 # ties -> lowest column
    arg = order[:, 0]
    best = cos[np.arange(n1), arg]
    srt = np.take_along_axis(cos, order, axis=1)
    margin2 = best - srt[:, 1] if n2 > 1 else np.full(n1, np.inf)
    margin3 = best - srt[:, 2] if n2 > 2 else np.full(n1, np.inf)
    return dict(loss=float((1.0 - best).mean()), grad=grad_toward(f1, f2, arg), argmax=arg, cos=cos, best=best,
                margin2=margin2, margin3=margin3)


# ---- the short-list ----------------------------------------------------------------------------------------------------------
def normalise_fp32(f):
    """columns of f (C, N) times 1 / sqrt(sum x^2), all in fp32 (nnfm_prep_kernel up to the order of the sum)"""
    x = torch.as_tensor(np.asarray(f, np.float32))
    inv = 1.0 / torch.sqrt((x * x).sum(dim=0))
    return x * inv


def near_bf16_tie(v, ulps=4):
    """elements of the fp32 tensor v within `ulps` fp32 ulps of the midpoint of two neighbouring bf16 values"""
    low = v.contiguous().view(torch.int32) & 0xFFFF
    return (low - 0x8000).abs() <= ulps


def nudge(f):
    """f (C, N) fp32 with every element that normalises to within 4 fp32 ulps of a bf16 tie multiplied by 1 + 2^-12, repeated
    until no such element remains"""
    x = np.array(f, np.float32, copy=True)
    for _ in range(64):
        tie = near_bf16_tie(normalise_fp32(x)).numpy()
        if not tie.any():
            return x
        x[tie] *= np.float32(1.0 + 2.0 ** -12)
    raise AssertionError("nudge: elements on a bf16 tie remain")


def bf16_products(f1, f2):
    """(N1, N2) float64 products of the fp32-normalised, bf16-rounded columns"""
    a = normalise_fp32(f1).bfloat16().double().numpy()
    b = normalise_fp32(f2).bfloat16().double().numpy()
    return a.T @ b


def emulate(f1, f2, keep=2):
    """-> dict(pred (N1,): the column the kernel is predicted to match, decided (N1,) bool, deficit (N1,): best float64 cosine
    minus the predicted column's, e: max |product - float64 cosine|, top (N1, <=3): columns by falling product, prod (N1, N2)).
    keep = None short-lists every column."""
    c = np.asarray(f1).shape[0]
    cos = cosines(f1, f2)
    prod = bf16_products(f1, f2)
    n1, n2 = prod.shape
    keep = n2 if keep is None else min(keep, n2)
    rows = np.arange(n1)
    order = np.argsort(-prod, axis=1, kind="stable")                # ties -> lowest column
    cand = order[:, :keep]
    ccos = np.take_along_axis(cos, cand, axis=1)
    # the float64 cosines decide; ties -> lowest column
    pick = np.lexsort((cand.T, -ccos.T), axis=0)[0] if keep > 1 else np.zeros(n1, np.int64)
    pred = cand[rows, pick]
    srt = np.take_along_axis(prod, order, axis=1)
    set_known = (srt[:, keep - 1] - srt[:, keep] > acc_bound(c)) if n2 > keep else np.ones(n1, bool)
    if keep > 1:
        two = np.sort(ccos, axis=1)
        told_apart = two[:, -1] - two[:, -2] > FP32_MARGIN
    else:
        told_apart = np.ones(n1, bool)
    return dict(pred=pred, decided=set_known & told_apart, deficit=cos.max(axis=1) - cos[rows, pred],
                e=float(np.abs(prod - cos).max()), top=order[:, :3], prod=prod)


def follows_float64(f1, f2):
    """(N1,) bool: the float64 argmax is certain to reach the device's short-list -- its emulated product lies more than
    acc_bound(C) above the second largest product of the OTHER columns, so at most one of them can come before it."""
    c = np.asarray(f1).shape[0]
    ref, prod = reference(f1, f2), bf16_products(f1, f2)
    n1, n2 = prod.shape
    if n2 <= 2:
        return np.ones(n1, bool)
    rows = np.arange(n1)
    mine = prod[rows, ref["argmax"]]
    others = prod.copy()
    others[rows, ref["argmax"]] = -np.inf
    second_other = -np.sort(-others, axis=1)[:, 1]
    return mine - second_other > acc_bound(c)


def matched_columns(got, f1, f2):
    """The column each row of the device gradient `got` (C, N1) points at: the j whose float64 gradient has the smallest
    residual max_c |got - grad_j|.  -> (columns (N1,), residuals (N1,) over the scale of the float64 gradient of the argmax)"""
    a, b = np.asarray(f1, np.float64), np.asarray(f2, np.float64)
    got = np.asarray(got, np.float64)
    n1 = a.shape[1]
    na = np.linalg.norm(a, axis=0)
    un1, un2 = a / na, b / np.linalg.norm(b, axis=0)
    cos = un1.T @ un2
    scale = np.abs(grad_toward(f1, f2, cos.argmax(axis=1))).max()
    cols, res = np.zeros(n1, np.int64), np.zeros(n1)
    for i in range(n1):
        g = -(un2 - cos[i][None, :] * un1[:, i:i + 1]) / (na[i] * n1)       # (C, N2)
        r = np.abs(g - got[:, i:i + 1]).max(axis=0)
        cols[i], res[i] = r.argmin(), r.min()
    return cols, res / scale


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def features(c, n, seed, relu):
    x = torch.randn(c, n, generator=_gen(seed))
    return (torch.relu(x + 0.3) if relu else x).numpy()


@functools.lru_cache(maxsize=None)
def plain_case(c, n1, n2, relu, seed=0):
    """Random (or post-ReLU) features on which every row with a float64 margin above FP32_MARGIN follows the float64 neighbour by
    the emulation alone (``follows_float64``), and at most MAX_EXCLUDED of the rows lie below the margin: the first seed of
    seed, seed + 1, ... that meets both.  -> (f1, f2, reference)"""
    for s in range(seed, seed + 32):
        f1 = nudge(features(c, n1, 1000 * s + 7 * c + n1, relu))
        f2 = nudge(features(c, n2, 1000 * s + 7 * c + n2 + 500_000, relu))
        ref = reference(f1, f2)
        clear = ref["margin2"] > FP32_MARGIN
        if (follows_float64(f1, f2) | ~clear).all() and (~clear).mean() <= MAX_EXCLUDED:
            return f1, f2, ref
    raise AssertionError("plain_case: no seed meets the premises")


FORMS = (64, 128, 192, 256, 320, 384, 448, 512)
ROW_EDGES = (1, 31, 32, 33, 127, 128, 129, 255, 256, 257)
COL_EDGES = (1, 2, 3, 31, 32, 33, 63, 64, 65)


@functools.lru_cache(maxsize=None)
def planted_case(c=64, n2=97, runner="lane", seed=3):
    """One row per style column: row i = a positive multiple of the unit column j(i) = i, plus three quarters of the unit
    column r(i), plus small noise (cosines ~0.8 to j, ~0.6 to r, below 0.45 to the others).  r = j +- 32 (the same lane of another
    tile: the lane's own two-entry list) for runner = "lane", r = j +- 1 (a neighbouring lane: the merge across lanes) for
    "merge"; the sign alternates so the runner-up comes both before and after the match.
    -> (f1, f2, j (N1,), r (N1,), reference)"""
    g = _gen(seed + (0 if runner == "lane" else 1))
    f2 = torch.randn(c, n2, generator=g)
    unit = f2 / f2.norm(dim=0)
    j = torch.arange(n2)
    step = 32 if runner == "lane" else 1
    r = torch.where(((j // step) % 2 == 0) & (j + step < n2), j + step, j - step)
    amp = 0.5 + torch.rand(n2, generator=g) * 4.0
    f1 = amp * (unit[:, j] + 0.75 * unit[:, r] + 0.02 * torch.randn(c, n2, generator=g))
    f1, f2 = nudge(f1.numpy()), nudge(f2.numpy())
    return f1, f2, j.numpy(), r.numpy(), reference(f1, f2)


@functools.lru_cache(maxsize=None)
def duplicate_case(c=64, n1=129, n_unique=97, seed=11):
    """f2 holds every column of `unique` twice, interleaved and then shuffled; f1 rows are noisy positive multiples of unique
    columns, so the float64 neighbour is clear of every other DISTINCT column by far more than the bf16 product error (with the
    best column present twice the short-list holds both copies and nothing else).
    -> (f1, f2 (C, 2 n_unique), unique (C, n_unique), copy_of (2 n_unique,), reference on `unique`)"""
    g = _gen(seed)
    unique = torch.relu(torch.randn(c, n_unique, generator=g) + 0.3)
    j = torch.randint(0, n_unique, (n1,), generator=g)
    f1 = (0.5 + 3.0 * torch.rand(n1, generator=g)) * unique[:, j] + 0.1 * torch.randn(c, n1, generator=g).abs()
    unique = nudge(unique.numpy())
    twice = np.repeat(unique, 2, axis=1)                            # interleaved: u0 u0 u1 u1 ...
    perm = torch.randperm(2 * n_unique, generator=g).numpy()
    f1 = nudge(f1.numpy())
    return f1, np.ascontiguousarray(twice[:, perm]), unique, perm // 2, reference(f1, unique)


# near-duplicate style columns: C -> (N1, N2, copies per group, relative perturbation of a copy).  On the CPU (emulation alone) 1e-3
# leaves 96 / 88 / 75 % of the rows decided at C = 64 / 192 / 320 and 46 % at C = 512, where acc_bound(C) = 6.1e-5 swallows more
# of the gaps between the copies' products; 2e-3 there gives 63 % (4e-3 no more, and fewer rows that leave the argmax).
NEAR_DUP = {64: (257, 240, 4, 1e-3), 192: (257, 240, 4, 1e-3), 320: (257, 240, 4, 1e-3), 512: (257, 240, 4, 2e-3)}
NEAR_DUP_ROW_NOISE = 0.3


@functools.lru_cache(maxsize=None)
def near_duplicate_case(c):
    """Post-ReLU features whose style columns come in groups of near-copies (a flat or repeated region of the style image):
    column = base * (1 + p * randn) elementwise, shuffled.  A row of f1 is a base with 30 % elementwise noise (the rendered frame
    resembles the style), so the copies of its group are its nearest columns and their float64 cosines lie far closer together
    than the bf16 product error.  -> (f1, f2, reference, emulation)"""
    n1, n2, copies, p = NEAR_DUP[c]
    g = _gen(100 + c)
    base = torch.relu(torch.randn(c, n2 // copies, generator=g) + 0.3)
    f2 = base.repeat_interleave(copies, dim=1) * (1.0 + p * torch.randn(c, n2, generator=g))
    f2 = f2[:, torch.randperm(n2, generator=g)]
    f1 = base[:, torch.randint(0, n2 // copies, (n1,), generator=g)] * (1.0 + NEAR_DUP_ROW_NOISE * torch.randn(c, n1, generator=g))
    f1, f2 = nudge(f1.numpy()), nudge(f2.numpy())
    return f1, f2, reference(f1, f2), emulate(f1, f2)
