"""Generates compose.npz from the imported reference's gaussian_renderer/__init__.py: the nine rigid-edit helpers
(``rotmat2qvec``, ``rx``, ``ry``, ``rz``, ``rescale``, ``rotate_by_euler_angles``, ``rotate_by_matrix``, ``translation``,
``transform``, :158-249) and the statements of ``render_composite`` between the rasterizer's construction and its call
(:287-312: the getters, the deformation, the six boolean gathers, ``transform``, the six ``torch.cat``) are pulled out of
the file with ``ast`` and run on CPU fp32 tensors.

    python tests/golden/make_compose.py

Scene: a background model of 600 Gaussians and a dynamic model of 1600 (trase_amd.synthetic, F = 8, SH and feature values
rounded to multiples of 1/16 so that the archive stays small) with a tensor deformation of the dynamic model.  Cases:
  edit    ``transform`` of the deformed dynamic model: scale 1.5, angles (0.3, -1.1, 2.0), offset (0.5, -0.25, 1.0), and the
          outputs of every helper on the way;
  zero    ``transform`` with all angles exactly zero (scale 0.75, offset (-0.5, 0.125, 2.0)): the early return;
  masked  the ``render_composite`` statements with a 60 % mask and the edit of the first case: all six tensors.

The generator refuses to write the file if any reference output is outside its forward-error bound around the float64
restatement (tests/compose_reference.py).  Runs on the CPU only; the archive regenerates byte for byte.
"""
import ast
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden import REF  # noqa: E402  (the imported reference checkout)
from make_lift import write_npz  # noqa: E402
from tests import compose_reference as cr  # noqa: E402
from trase_amd.synthetic import SynthGaussianModel, make_scene  # noqa: E402

HELPERS = ("rotmat2qvec", "rx", "ry", "rz", "rescale", "rotate_by_euler_angles", "rotate_by_matrix", "translation", "transform")
N_BG, N_DYN, F = 600, 1600, 8
EDIT = dict(scale=1.5, angles=(0.3, -1.1, 2.0), offset=(0.5, -0.25, 1.0))
ZERO = dict(scale=0.75, angles=(0.0, 0.0, 0.0), offset=(-0.5, 0.125, 2.0))
RAW = ("xyz", "scaling", "rotation", "opacity", "features_dc", "features_rest", "gaussian_features")


def load_reference():
    """-> (namespace holding the nine helpers, code object of render_composite's composition statements)."""
    tree = ast.parse(open(os.path.join(REF, "gaussian_renderer", "__init__.py")).read())
    funcs = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}
    ns = {"torch": torch}
    exec(compile(ast.Module(body=[funcs[h] for h in HELPERS], type_ignores=[]), "gaussian_renderer/__init__.py", "exec"), ns)
    body = funcs["render_composite"].body

    def assigns(stmt, name):
        if not isinstance(stmt, ast.Assign):
            return False
        t = stmt.targets[0]
        names = [e.id for e in t.elts] if isinstance(t, ast.Tuple) else ([t.id] if isinstance(t, ast.Name) else [])
        return name in names

    first = next(i for i, s in enumerate(body) if assigns(s, "means3D_final"))
    last = max(i for i, s in enumerate(body) if assigns(s, "shs_obj_final"))
    assert 0 < first < last
    return ns, compile(ast.Module(body=body[first:last + 1], type_ignores=[]), "gaussian_renderer/__init__.py", "exec")


def quantised(scene):
    q = lambda t: torch.round(t * 16) / 16
    scene.features_dc, scene.features_rest, scene.gaussian_features = q(scene.features_dc), q(scene.features_rest), q(scene.gaussian_features)
    return scene


def raw_of(pc):
    return {k: getattr(pc, "_" + k).detach().numpy() for k in RAW}


def main():
    warnings.simplefilter("ignore")            # the reference re-wraps tensors with torch.tensor(): a UserWarning per call
    ns, composite = load_reference()
    bg = SynthGaussianModel(quantised(make_scene(N_BG, feat_dim=F, seed=11, scale_mult=0.8)), requires_grad=False)
    dyn = SynthGaussianModel(quantised(make_scene(N_DYN, feat_dim=F, seed=12, scale_mult=0.8)), requires_grad=False)
    g = torch.Generator().manual_seed(13)
    d_xyz, d_rot, d_sc = (0.02 * torch.randn(N_DYN, c, generator=g) for c in (3, 4, 3))
    mask = torch.rand(N_DYN, generator=g) < 0.6
    T = lambda v: torch.tensor(v, dtype=torch.float32)
    angles = [T(a) for a in EDIT["angles"]]
    out = dict(mask=mask.numpy(), d_xyz=d_xyz.numpy(), d_rotation=d_rot.numpy(), d_scaling=d_sc.numpy(),
               edit_scale=np.float64(EDIT["scale"]), edit_angles=np.array(EDIT["angles"], dtype=np.float32),
               edit_offset=np.array(EDIT["offset"], dtype=np.float32), zero_scale=np.float64(ZERO["scale"]),
               zero_offset=np.array(ZERO["offset"], dtype=np.float32))
    out.update({"bg_" + k: v for k, v in raw_of(bg).items()})
    out.update({"dyn_" + k: v for k, v in raw_of(dyn).items()})

    # the deformed, activated dynamic model: what the helpers act on
    means_in, rots_in, scales_in = dyn.get_xyz + d_xyz, dyn.get_rotation + d_rot, dyn.get_scaling + d_sc
    out.update(means_in=means_in.numpy(), rots_in=rots_in.numpy(), scales_in=scales_in.numpy())
    checks = []

    # every helper by itself
    Rx, Ry, Rz = ns["rx"](angles[0]), ns["ry"](angles[1]), ns["rz"](angles[2])
    R32 = torch.tensor(Rx @ Ry @ Rz, dtype=torch.float32)
    q32 = ns["rotmat2qvec"](R32)
    out.update(rx=Rx.numpy(), ry=Ry.numpy(), rz=Rz.numpy(), R=R32.numpy(), q=q32.numpy())
    for axis, got in zip("xyz", (Rx, Ry, Rz)):                 # one transcendental per entry: 2 roundings of a value <= 1
        a = float(np.float32(EDIT["angles"]["xyz".index(axis)]))
        checks.append(("r" + axis, *cr.worst(got.numpy(), getattr(cr, "rot_" + axis)(a), 2 * cr.U * np.ones((3, 3)))))
    checks.append(("rotmat2qvec", *cr.worst(q32.numpy(), cr.qvec(R32.numpy()), cr.ROT_ROUNDINGS * cr.U * np.ones(4))))
    rs_m, rs_s = ns["rescale"](means_in[:64].clone(), scales_in[:64].clone(), EDIT["scale"])
    tr_m = ns["translation"](means_in[:64].clone(), T(EDIT["offset"]))
    out.update(rescale_means=rs_m.numpy(), rescale_scales=rs_s.numpy(), translation_means=tr_m.numpy())
    mm, mq = ns["rotate_by_matrix"](means_in.clone(), rots_in.clone(), R32)
    em, eq = ns["rotate_by_euler_angles"](means_in.clone(), rots_in.clone(), angles)
    assert torch.equal(mm, em) and torch.equal(mq, eq)
    out.update(matrix_means=mm.numpy(), matrix_rots=mq.numpy())
    e_rot = cr.make_edit(1.0, R=R32.numpy())
    xm, xq, _, b = cr.edit_activated(means_in.numpy(), rots_in.numpy(), scales_in.numpy(), e_rot)
    checks += [("rotate_by_matrix means", *cr.worst(mm.numpy(), xm, b["means"])), ("rotate_by_matrix rots", *cr.worst(mq.numpy(), xq, b["rots"]))]

    # transform: the edit and the zero-angle case
    for tag, spec in (("edit", EDIT), ("zero", ZERO)):
        tm, tq, ts = ns["transform"](means_in.clone(), rots_in.clone(), scales_in.clone(), spec["scale"], T(spec["offset"]),
                                     [T(a) for a in spec["angles"]])
        out.update({f"{tag}_means": tm.numpy(), f"{tag}_rots": tq.numpy(), f"{tag}_scales": ts.numpy()})
        e = cr.make_edit(spec["scale"], np.array(spec["angles"], dtype=np.float32), np.array(spec["offset"], dtype=np.float32))
        xm, xq, xs, b = cr.edit_activated(means_in.numpy(), rots_in.numpy(), scales_in.numpy(), e)
        checks += [(f"{tag} means", *cr.worst(tm.numpy(), xm, b["means"])), (f"{tag} rots", *cr.worst(tq.numpy(), xq, b["rots"])),
                   (f"{tag} scales", *cr.worst(ts.numpy(), xs, b["scales"]))]
        if tag == "zero":
            assert torch.equal(tq, rots_in)                    # the early return: not renormalised

    # the masked composite: render_composite's own statements
    cns = dict(ns, background_gaussian=bg, dynamic_gaussian=dyn, d_xyz=d_xyz, d_rotation=d_rot, d_scaling=d_sc, mask=mask,
               scales_bias=EDIT["scale"], motion_bias=T(EDIT["offset"]), rotation_bias=angles)
    exec(composite, cns)
    names = dict(means="means3D_final", scales="scales_final", rots="rotations_final", opac="opacity_final", shs="shs_final",
                 objs="shs_obj_final")
    for k, v in names.items():
        out["masked_" + k] = cns[v].detach().numpy()
    e = cr.make_edit(EDIT["scale"], np.array(EDIT["angles"], dtype=np.float32), np.array(EDIT["offset"], dtype=np.float32))
    x, b, offsets = cr.compose([dict(model=raw_of(bg)), dict(model=raw_of(dyn), d_xyz=d_xyz.numpy(), d_rotation=d_rot.numpy(),
                                                              d_scaling=d_sc.numpy(), rows=mask.numpy(), edit=e)])
    assert offsets == [0, N_BG, N_BG + int(mask.sum())] and out["masked_means"].shape[0] == offsets[-1]
    for k in ("means", "scales", "rots", "opac"):
        checks.append((f"masked {k}", *cr.worst(out["masked_" + k], x[k], b[k])))
    assert np.array_equal(out["masked_shs"], x["shs"]) and np.array_equal(out["masked_objs"], x["objs"])

    bad = False
    for name, ratio, err in checks:
        print(f"{name:28s} reference fp32 vs float64: max error {err:.3e}, {ratio:.3f} of its bound")
        bad |= not ratio <= 1.0
    if bad:
        raise SystemExit("refusing to write compose.npz: a reference output is outside its forward-error bound")
    assert all(v.dtype != np.float64 or v.ndim == 0 for v in out.values())
    path = os.path.join(HERE, "compose.npz")
    write_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
