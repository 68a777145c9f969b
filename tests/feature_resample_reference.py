"""TEST INFRASTRUCTURE ONLY -- the bilinear resize the FEATURE-state head takes its sampled columns through
(``torch.nn.functional.interpolate(..., mode="bilinear")``, ``align_corners=False``; train.py:283-284), restated in three parts:

* ``axis_table``: per destination index the two source taps and their fp32 weights, with ATen's coordinate
  ``max(fma(in / out, dst + 0.5, -0.5), 0)``.  The fused product is evaluated as
  ``float32(float64(scale) * float64(dst + 0.5) - 0.5)``: a 24-bit scale times a short integer-and-a-half is exact in float64,
  and so is the subtraction, so the one rounding to float32 is the fma's.  ``fused=False`` rounds the product first (what an
  unfused kernel would compute; kept to show that the tests tell the two apart).
* ``resample64``: ``h0 * (w0 * a + w1 * b) + h1 * (w0 * c + w1 * d)`` in float64 from those fp32 weights, written with
  ``index_select`` so that autograd gives the scatter-form adjoint.
* ``first_count`` / ``adjoint_gather``: the adjoint as a gather from the source side -- per source row (column) the run of
  destinations whose upper tap it is -- the form the HIP backward uses.
"""
import numpy as np
import torch


def axis_table(n_in, n_out, fused=True):
    """(i0, i1 int64; l0, l1 float32) for dst = 0 .. n_out - 1."""
    scale = np.float32(n_in) / np.float32(n_out)
    d = np.arange(n_out, dtype=np.float64) + 0.5
    if fused:
        src = (np.float64(scale) * d - 0.5).astype(np.float32)
    else:
        src = (scale * d.astype(np.float32)).astype(np.float32) - np.float32(0.5)
    src = np.maximum(src, np.float32(0.0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    l0 = (np.float32(1.0) - l1).astype(np.float32)
    return i0, i1, l0, l1


def resample64(f, size, fused=True):
    """(C, Hr, Wr) -> (C, h, w) in float64 (``f`` is converted), on f's device; differentiable in ``f``."""
    h, w = size
    dev = f.device
    y0, y1, h0, h1 = (torch.from_numpy(a).to(dev) for a in axis_table(f.shape[1], h, fused))
    x0, x1, w0, w1 = (torch.from_numpy(a).to(dev) for a in axis_table(f.shape[2], w, fused))
    h0, h1, w0, w1 = h0.double()[None, :, None], h1.double()[None, :, None], w0.double(), w1.double()
    f = f.double()
    top, bot = f.index_select(1, y0), f.index_select(1, y1)
    a, b = top.index_select(2, x0), top.index_select(2, x1)
    c, d = bot.index_select(2, x0), bot.index_select(2, x1)
    return h0 * (w0 * a + w1 * b) + h1 * (w0 * c + w1 * d)


def first_count(n_in, n_out):
    """Per source index i: the first destination whose upper tap i0 is i, and how many there are (i0 is monotone)."""
    i0 = axis_table(n_in, n_out)[0]
    assert bool(np.all(np.diff(i0) >= 0))
    first = np.searchsorted(i0, np.arange(n_in), side="left")
    count = np.searchsorted(i0, np.arange(n_in), side="right") - first
    return first, count


def _axis_contributors(n_in, n_out):
    """Per source index the destinations it is a tap of, padded to the longest run: (dst [n_in, K] int64, weight [n_in, K]
    float64, 0 in the padding), in the fixed order lower-tap run (i0 == i - 1, weight l1), then upper-tap run (i0 == i, weight
    l0 -- and l1 as well where the clamp put both taps on i)."""
    i0, i1, l0, l1 = axis_table(n_in, n_out)
    first, count = first_count(n_in, n_out)
    rows = []
    for i in range(n_in):
        row = []
        if i > 0:
            row += [(d, float(l1[d])) for d in range(first[i - 1], first[i - 1] + count[i - 1])]
        for d in range(first[i], first[i] + count[i]):
            row.append((d, float(l0[d]) + float(l1[d]) if i1[d] == i0[d] else float(l0[d])))
        rows.append(row)
    K = max(1, max(len(r) for r in rows))
    dst, wt = np.zeros((n_in, K), dtype=np.int64), np.zeros((n_in, K))
    for i, row in enumerate(rows):
        for k, (d, x) in enumerate(row):
            dst[i, k], wt[i, k] = d, x
    return dst, wt


def adjoint_gather(g, in_size, sampled=None):
    """Adjoint of ``resample64`` applied to the (C, h, w) float64 cotangent ``g`` (numpy), gathered per source pixel through
    the first / count tables; with ``sampled`` (h, w bool) only those destinations contribute.  Returns (C, Hr, Wr) float64:
    out[:, Y, X] = sum over the row contributors (dy, hy) of Y and the column contributors (dx, wx) of X of hy * wx * g[:, dy, dx]."""
    Hr, Wr = in_size
    g = np.asarray(g, dtype=np.float64)
    if sampled is not None:
        g = g * np.asarray(sampled, dtype=np.float64)[None]
    dy, hy = _axis_contributors(Hr, g.shape[1])
    dx, wx = _axis_contributors(Wr, g.shape[2])
    rows = np.einsum("yk,cykw->cyw", hy, g[:, dy, :])               # (C, Hr, w)
    return np.einsum("xk,cyxk->cyx", wx, rows[:, :, dx])            # (C, Hr, Wr)
