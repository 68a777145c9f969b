"""Float64 restatement of the composition behind ``render_composite`` (numpy, test infrastructure only), and the forward-error
bounds every fp32 evaluation of it -- the reference's torch ops, the torch helpers of trase_amd/edit.py, the HIP kernel -- is
held to.

A bound is (fp32 roundings in the expression + 2 per library transcendental) * 2^-24 * (sum of the absolute values of the
terms):
  means      8: x + d (1), * s (1), three products R_ij * . (1 each on its term, 1 more for a rounded R_ij), two sums (2),
                + t (1) -- the longest chain through one term is 7, "about 8";   scale  sum_j |R_ij| |s (x + d)_j| + |t_i|
  rotations 16: normalise (4 products, 3 sums, sqrt, reciprocal, product: each below one rounding of a unit vector), + d (1),
                the Hamilton product (4 products, 3 sums per component, q_edit itself rounded), the second normalise;
                scale  max(1, |rot|): 1 for a renormalised quaternion, the norm of normalize(q) + d when the rotation is skipped
  scales     4: exp (2), + d (1), * s (1);                                        scale  |s| (exp(x) + |d|)
  opacity    4: exp (2), 1 + . (1), 1 / . (1), all on values <= 1;                scale  1"""
import numpy as np

U = 2.0 ** -24
MEANS_ROUNDINGS, ROT_ROUNDINGS, SCALES_ROUNDINGS, OPACITY_ROUNDINGS = 8, 16, 4, 4


def rot_x(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], dtype=np.float64)


def rot_y(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=np.float64)


def rot_z(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float64)


def euler_matrix(angles):
    x, y, z = (float(a) for a in angles)
    return rot_x(x) @ rot_y(y) @ rot_z(z)


def quat_to_rotmat(q):
    """R(q), q = (r, x, y, z) (utils/general_utils.py:122-154 without its normalisation)."""
    r, x, y, z = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
                     [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                     [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]])


def qvec(R):
    """The unit quaternion (r, x, y, z), r >= 0, with R(q) = R: closed form through the largest of the four squared
    components (Shepperd) -- independent of the eigenvector form the code under test uses."""
    R = np.asarray(R, dtype=np.float64)
    t = np.array([1 + R[0, 0] + R[1, 1] + R[2, 2], 1 + R[0, 0] - R[1, 1] - R[2, 2],
                  1 - R[0, 0] + R[1, 1] - R[2, 2], 1 - R[0, 0] - R[1, 1] + R[2, 2]])
    k = int(t.argmax())
    if k == 0:
        q = np.array([t[0], R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    elif k == 1:
        q = np.array([R[2, 1] - R[1, 2], t[1], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]])
    elif k == 2:
        q = np.array([R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], t[2], R[1, 2] + R[2, 1]])
    else:
        q = np.array([R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], t[3]])
    q = q / np.linalg.norm(q)
    return -q if q[0] < 0 else q


def hamilton(a, b):
    """a (x) b, components (r, x, y, z), broadcasting over leading axes."""
    w1, x1, y1, z1 = (a[..., k] for k in range(4))
    w0, x0, y0, z0 = (b[..., k] for k in range(4))
    return np.stack([w1 * w0 - x1 * x0 - y1 * y0 - z1 * z0, w1 * x0 + x1 * w0 + y1 * z0 - z1 * y0,
                     w1 * y0 - x1 * z0 + y1 * w0 + z1 * x0, w1 * z0 + x1 * y0 - y1 * x0 + z1 * w0], axis=-1)


def make_edit(scale_factor=1.0, angles=(0.0, 0.0, 0.0), offsets=(0.0, 0.0, 0.0), R=None):
    """angles: the fp32 (or float) values as given; R: a rotation matrix given instead of angles (rotate_by_matrix)."""
    zero = R is None and all(float(a) == 0.0 for a in angles)
    R = euler_matrix(angles) if R is None else np.asarray(R, dtype=np.float64)
    return dict(s=float(scale_factor), R=R, q=qvec(R), t=np.asarray(offsets, dtype=np.float64).reshape(3), zero=zero)


def edit_activated(means, rots, scales, edit):
    """The reference's ``transform`` on float64 copies of activated tensors -> (means, rots, scales, bounds dict)."""
    m, q, sc = (np.asarray(a, dtype=np.float64) for a in (means, rots, scales))
    R = np.eye(3) if edit["zero"] else edit["R"]
    ms = m * edit["s"]
    out_m = ms @ R.T + edit["t"]
    out_sc = sc * edit["s"]
    if edit["zero"]:
        out_q = q
    else:
        p = hamilton(edit["q"][None, :], q)
        out_q = p / np.linalg.norm(p, axis=-1, keepdims=True)
    b = dict(means=MEANS_ROUNDINGS * U * (np.abs(ms) @ np.abs(R).T + np.abs(edit["t"])),
             scales=(SCALES_ROUNDINGS - 2) * U * np.abs(out_sc),        # no exp here: the table's 2 roundings
             rots=ROT_ROUNDINGS * U * np.maximum(1.0, np.linalg.norm(out_q, axis=-1, keepdims=True)) * np.ones_like(out_q))
    return out_m, out_q, out_sc, b


def compose_part(model, d_xyz=None, d_rotation=None, d_scaling=None, rows=None, edit=None):
    """model: dict of the raw fp32 arrays xyz, scaling, rotation, opacity, features_dc, features_rest, gaussian_features.
    -> (dict means, scales, rots, opac, shs, objs in float64; dict of bounds for means, scales, rots, opac)."""
    f = lambda a: np.asarray(a, dtype=np.float64)
    n = model["xyz"].shape[0]
    z = lambda c: np.zeros((n, c))
    dx, dq, ds = (z(c) if d is None else f(d) for d, c in ((d_xyz, 3), (d_rotation, 4), (d_scaling, 3)))
    means = f(model["xyz"]) + dx
    ex = np.exp(f(model["scaling"]))
    scales = ex + ds
    scales_abs = ex + np.abs(ds)
    r = f(model["rotation"])
    rots = r / np.maximum(np.linalg.norm(r, axis=-1, keepdims=True), 1e-12) + dq
    opac = 1.0 / (1.0 + np.exp(-f(model["opacity"])))
    shs = np.concatenate([f(model["features_dc"]), f(model["features_rest"])], axis=1)
    objs = f(model["gaussian_features"])
    if rows is not None:
        rows = np.asarray(rows)
        rows = np.nonzero(rows)[0] if rows.dtype == np.bool_ else rows
        means, scales, scales_abs, rots, opac, shs, objs = (a[rows] for a in (means, scales, scales_abs, rots, opac, shs, objs))
    e = edit if edit is not None else make_edit()
    means, rots, scales, b = edit_activated(means, rots, scales, e)
    b["scales"] = SCALES_ROUNDINGS * U * abs(e["s"]) * scales_abs
    b["opac"] = OPACITY_ROUNDINGS * U * np.ones_like(opac)
    return dict(means=means, scales=scales, rots=rots, opac=opac, shs=shs, objs=objs), b


def compose(parts):
    """parts: list of keyword dicts of ``compose_part`` -> (outputs, bounds, offsets), rows of the parts one after the other."""
    outs, bounds, offsets = [], [], [0]
    for p in parts:
        o, b = compose_part(**p)
        outs.append(o)
        bounds.append(b)
        offsets.append(offsets[-1] + o["means"].shape[0])
    cat = lambda ds: {k: np.concatenate([d[k] for d in ds], axis=0) for k in ds[0]}
    return cat(outs), cat(bounds), offsets


def worst(value, exact, bound):
    """max over entries of |value - exact| / bound (<= 1 passes) and the largest absolute difference."""
    err = np.abs(np.asarray(value, dtype=np.float64) - exact)
    return float((err / bound).max()), float(err.max())
