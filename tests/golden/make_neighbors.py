"""Generates neighbors.npz from the imported reference's utils/loss_utils.py: ``loss_reg_3d_feature`` (:132-152) and
``loss_rigid_body_motion_reg_loss`` (:179-221) are pulled out of the file with ``ast`` and run on CPU tensors, in fp32 and in
float64, with a brute-force stand-in for ``pytorch3d.ops.knn_points`` that orders by (squared distance, index).

    python tests/golden/make_neighbors.py

Cases:
  feat    N = 300, D = 8, k = 5: the feature loss on a random cloud
  rigid2  two clusters of 140 and 160 points (ids 3 and 7), 128 neighbours, a random deformation of a rotated copy of an
          anisotropic cloud (the generator checks that the singular values of every S_i are at least 1e-2 apart, relative)
  rigid1  one cluster of 100 points, 128 neighbours: fewer points than K = 129, so the k-NN pads with edges to row 0

Records the inputs, the neighbour indices the stand-in returned ([:, 1:] applied), the losses and the autograd gradients of both
precisions.  The generator checks the float64 results against tests/neighbors_reference.py to 1e-12 relative and refuses to
write the file otherwise.  Runs on the CPU only; the archive is written with fixed time stamps, so it regenerates byte for byte.
"""
import ast
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden import REF  # noqa: E402  (the imported reference checkout)
from make_lift import write_npz  # noqa: E402
from tests import neighbors_reference as nr  # noqa: E402

NAMES = ("loss_reg_3d_feature", "loss_rigid_body_motion_reg_loss")


class Knn:
    """Stand-in for pytorch3d.ops.knn_points (self-queries, batch 1): brute force in the tensors' own precision, rows ascending
    by (squared distance, index), index 0 / distance 0 where the cloud has fewer than K points.  Keeps every index it returned."""

    def __init__(self):
        self.calls = []

    def knn_points(self, p1, p2, K=1):
        a, b = p1[0].detach().numpy(), p2[0].detach().numpy()
        dist, idx = nr.knn_lex(a, b, K, dtype=a.dtype)
        self.calls.append(idx)
        return types.SimpleNamespace(idx=torch.from_numpy(idx)[None], dists=torch.from_numpy(dist)[None], knn=None)


def load_reference(knn):
    tree = ast.parse(open(os.path.join(REF, "utils", "loss_utils.py")).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in NAMES]
    assert sorted(n.name for n in body) == sorted(NAMES)
    ns = {"torch": torch, "sigmoid": torch.sigmoid, "ops": knn}
    exec(compile(ast.Module(body=body, type_ignores=[]), "loss_utils.py", "exec"), ns)
    return ns[NAMES[0]], ns[NAMES[1]]


def rotation(axis, angle):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def scenes(seed=0):
    g = np.random.default_rng(seed)
    feat = dict(feats=g.normal(0.0, 1.5, (300, 8)).astype(np.float32), xyz=g.uniform(-1, 1, (300, 3)).astype(np.float32))
    out = {"feat": feat}
    for name, sizes, ids in (("rigid2", (140, 160), (3, 7)), ("rigid1", (100,), (0,))):
        n = sum(sizes)
        x1 = g.uniform(-1, 1, (n, 3)) * np.array([1.0, 0.6, 0.3])     # anisotropic: the singular values of every S_i stay apart
        cid = np.concatenate([np.full(s, i) for s, i in zip(sizes, ids)])
        order = g.permutation(n)
        x1, cid = x1[order], cid[order]
        x2 = x1 @ rotation((1, 2, 3), 0.7).T + 0.3 + 0.15 * g.normal(size=(n, 3))
        out[name] = dict(xyz1=x1.astype(np.float32), xyz2=x2.astype(np.float32), cluster_ids=cid.astype(np.int64))
    return out


def run(fn, knn, arrays, dtype, grads, **kw):
    knn.calls.clear()
    ts = {k: torch.tensor(v.astype(dtype) if v.dtype.kind == "f" else v, requires_grad=k in grads) for k, v in arrays.items()}
    loss = fn(*ts.values(), **kw)
    loss.backward()
    return loss.detach().numpy(), {k: ts[k].grad.numpy() for k in grads}, [c[:, 1:].copy() for c in knn.calls]


def close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
    print(f"  {what}: restatement vs reference float64, relative {err:.2e}")
    if not err <= 1e-12:
        raise SystemExit("refusing to write neighbors.npz: the float64 restatement does not reproduce the reference")


def main():
    knn = Knn()
    feat_loss, rigid_loss = load_reference(knn)
    sc = scenes()
    out = {}
    # ---- the feature loss
    a = sc["feat"]
    for tag, dt in (("f32", np.float32), ("f64", np.float64)):
        loss, gr, idx = run(feat_loss, knn, dict(gaussian_feats=a["feats"], gaussian_xyz=a["xyz"]), dt, ("gaussian_feats",), k=5)
        out[f"feat_loss_{tag}"], out[f"feat_grad_{tag}"], out[f"feat_idx_{tag}"] = loss, gr["gaussian_feats"], idx[0].astype(np.int32)
    assert np.array_equal(out["feat_idx_f32"], out["feat_idx_f64"]), "the fp32 and float64 neighbours differ: pick another seed"
    out["feat_feats"], out["feat_xyz"] = a["feats"], a["xyz"]
    r = nr.feat3d(a["feats"], out["feat_idx_f64"])
    close(r["loss"], out["feat_loss_f64"], "feature loss")
    close(r["grad"], out["feat_grad_f64"], "feature gradient")
    assert np.array_equal(nr.knn_lex(a["xyz"], a["xyz"], 6)[1][:, 1:], out["feat_idx_f64"])
    # ---- the rigid loss
    for name in ("rigid2", "rigid1"):
        a = sc[name]
        for tag, dt in (("f32", np.float32), ("f64", np.float64)):
            loss, gr, idx = run(rigid_loss, knn, a, dt, ("xyz1", "xyz2"), num_neighbors=128)
            out[f"{name}_loss_{tag}"], out[f"{name}_g1_{tag}"], out[f"{name}_g2_{tag}"] = loss, gr["xyz1"], gr["xyz2"]
            for c, ix in enumerate(idx):
                out[f"{name}_idx{c}_{tag}"] = ix.astype(np.int32)
        for c in range(len(idx)):
            assert np.array_equal(out[f"{name}_idx{c}_f32"], out[f"{name}_idx{c}_f64"]), "fp32 and float64 neighbours differ"
        for k, v in a.items():
            out[f"{name}_{k}"] = v
        r = nr.rigid_loss(a["xyz1"], a["xyz2"], a["cluster_ids"], 128)
        gap = min(float((np.minimum(sg[:, 0] - sg[:, 1], sg[:, 1] - sg[:, 2]) / sg[:, 0]).min()) for sg in r["sigma"])
        print(f"  {name}: singular values of every S_i at least {gap:.3e} apart, relative")
        if gap < 1e-2:
            raise SystemExit("refusing to write neighbors.npz: the SVD's gradient is ill-conditioned in this scene")
        close(r["loss"], out[f"{name}_loss_f64"], f"{name} loss")
        close(r["g1"], out[f"{name}_g1_f64"], f"{name} gradient to xyz1")
        close(r["g2"], out[f"{name}_g2_f64"], f"{name} gradient to xyz2")
        # the edge sums on their own, on the first cluster's float64 data
        sel = a["cluster_ids"] == np.unique(a["cluster_ids"])[0]
        ix = out[f"{name}_idx0_f64"]
        p1, p2 = torch.tensor(a["xyz1"][sel].astype(np.float64)), torch.tensor(a["xyz2"][sel].astype(np.float64))
        j = torch.from_numpy(ix.astype(np.int64))
        e1, e2 = p1[:, None] - p1[j], p2[:, None] - p2[j]
        S = torch.bmm(e1.transpose(1, 2), e2)
        close(nr.edge_moments(p1.numpy(), p2.numpy(), ix)[0], S.numpy(), f"{name} moments")
        Um, _, V = torch.svd(S)
        Rm = torch.bmm(V, Um.transpose(1, 2))
        res = (e1 - torch.bmm(Rm, e2.transpose(1, 2)).transpose(1, 2)).pow(2).sum(2).sum(1)
        close(nr.edge_residual(p1.numpy(), p2.numpy(), ix, Rm.numpy())[0], res.numpy(), f"{name} residual")
        out[f"{name}_S0_f64"], out[f"{name}_R0_f64"], out[f"{name}_res0_f64"] = S.numpy(), Rm.numpy(), res.numpy()
    path = os.path.join(HERE, "neighbors.npz")
    write_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes;", {k: float(v) for k, v in out.items() if "loss" in k})


if __name__ == "__main__":
    main()
