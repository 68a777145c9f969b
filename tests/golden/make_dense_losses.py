"""Generates dense_losses.npz from the imported reference's utils/loss_utils.py: ``loss_feature3d`` (:154-175) and ``loss_cls_3d``
(:89-130) are pulled out of the file with ``ast`` and run on CPU tensors, in fp32 and in float64.

    python tests/golden/make_dense_losses.py

Cases (N <= max_points in both, so the only draw is loss_cls_3d's sample, recorded):
  f3d   N = 300, D = 8, kp = 16, kn = 4, lambda_p = 1, lambda_n = 1 on a random cloud in +-1
  cls   N = 500 rows of 32-d unit features, C = 16 softmax predictions, k = 5, 100 sampled rows (torch.manual_seed(5))

Records the inputs, the sample, the neighbour indices (float64 selection of tests/dense_reference.py), the losses and the autograd
gradients of both precisions.  The generator refuses to write unless the float64 results equal the restatement of
tests/dense_reference.py to 1e-12 relative -- which also proves that the reference chose the same neighbours -- and unless the
fp32 ``cdist`` + ``topk`` picks the same neighbour sets, so that the fp32 results count as the same sum in another precision.
Runs on the CPU only; the archive is written with fixed time stamps, so it regenerates byte for byte."""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden import REF  # noqa: E402  (the imported reference checkout)
from make_lift import write_npz  # noqa: E402
from tests import dense_reference as dr  # noqa: E402

NAMES = ("loss_feature3d", "loss_cls_3d")
CLS_SEED = 5


def load_reference():
    tree = ast.parse(open(os.path.join(REF, "utils", "loss_utils.py")).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in NAMES]
    assert sorted(n.name for n in body) == sorted(NAMES)
    ns = {"torch": torch, "sigmoid": torch.sigmoid, "cosine_similarity": torch.nn.functional.cosine_similarity}
    exec(compile(ast.Module(body=body, type_ignores=[]), "loss_utils.py", "exec"), ns)
    return ns[NAMES[0]], ns[NAMES[1]]


def scenes(seed=0):
    g = np.random.default_rng(seed)
    f3d = dict(feats=g.normal(0.0, 1.0, (300, 8)).astype(np.float32), xyz=g.uniform(-1, 1, (300, 3)).astype(np.float32))
    feat = g.normal(size=(500, 32))
    feat = (feat / np.linalg.norm(feat, axis=1, keepdims=True)).astype(np.float32)
    logits = g.normal(0.0, 2.0, (500, 16))
    pred = np.exp(logits) / np.exp(logits).sum(1, keepdims=True)
    return f3d, dict(features=feat, predictions=pred.astype(np.float32))


def close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
    print(f"  {what}: restatement vs reference float64, relative {err:.2e}")
    if not err <= 1e-12:
        raise SystemExit("refusing to write dense_losses.npz: the float64 restatement does not reproduce the reference")


def same_sets(a, b, what):
    if not np.array_equal(np.sort(np.asarray(a), axis=1), np.sort(np.asarray(b), axis=1)):
        raise SystemExit(f"refusing to write dense_losses.npz: {what}: fp32 cdist + topk picks other neighbours; use another seed")


def main():
    feature3d, cls3d = load_reference()
    a, b = scenes()
    out = {}
    # ---- loss_feature3d
    ref = dr.topk_f64(a["xyz"], a["xyz"], 16, 4)
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        f = torch.tensor(a["feats"], dtype=dt, requires_grad=True)
        x = torch.tensor(a["xyz"], dtype=dt)
        loss = feature3d(f, x)
        loss.backward()
        out[f"f3d_loss_{tag}"], out[f"f3d_grad_{tag}"] = loss.detach().numpy(), f.grad.numpy()
        d = torch.cdist(x, x)
        same_sets(d.topk(16, largest=False)[1].numpy(), ref["near_idx"], f"f3d near, {tag}")
        same_sets(d.topk(4, largest=True)[1].numpy(), ref["far_idx"], f"f3d far, {tag}")
    out["f3d_feats"], out["f3d_xyz"] = a["feats"], a["xyz"]
    out["f3d_near_idx"], out["f3d_far_idx"] = ref["near_idx"].astype(np.int32), ref["far_idx"].astype(np.int32)
    r = dr.feature3d(a["feats"], ref["near_idx"], ref["far_idx"])
    close(r["loss"], out["f3d_loss_f64"], "loss_feature3d")
    close(r["grad"], out["f3d_grad_f64"], "loss_feature3d gradient")
    # ---- loss_cls_3d
    torch.manual_seed(CLS_SEED)
    sample = torch.randperm(500)[:100].numpy()
    ref = dr.topk_f64(b["features"][sample], b["features"], 5, 0)
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        ft = torch.tensor(b["features"], dtype=dt)
        p = torch.tensor(b["predictions"], dtype=dt, requires_grad=True)
        torch.manual_seed(CLS_SEED)
        loss = cls3d(ft, p, sample_size=100)
        loss.backward()
        out[f"cls_loss_{tag}"], out[f"cls_grad_{tag}"] = loss.detach().numpy(), p.grad.numpy()
        same_sets(torch.cdist(ft[sample], ft).topk(5, largest=False)[1].numpy(), ref["near_idx"], f"cls, {tag}")
    out["cls_features"], out["cls_predictions"] = b["features"], b["predictions"]
    out["cls_sample"], out["cls_idx"] = sample.astype(np.int32), ref["near_idx"].astype(np.int32)
    r = dr.cls3d(b["predictions"], sample, ref["near_idx"])
    close(r["loss"], out["cls_loss_f64"], "loss_cls_3d")
    close(r["grad"], out["cls_grad_f64"], "loss_cls_3d gradient")
    path = os.path.join(HERE, "dense_losses.npz")
    write_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes;", {k: float(v) for k, v in out.items() if "loss" in k})


if __name__ == "__main__":
    main()
