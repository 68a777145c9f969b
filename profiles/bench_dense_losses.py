#!/usr/bin/env python
"""Secondary measurement: the dense top-k search and the two losses over it, each against a torch composition on the same GPU in
the same process, the sides taking turns, timed with HIP events, medians of --reps runs after a pre-roll:

  dense_topk 10 000 x 10 000 x 3, 16 near + 4 far      against torch.cdist + two topk (the reference's statements)
  dense_topk 800 x 200 000 x 32, 5 near                against torch.cdist + topk
  dense_topk 300 000 x 300 000 x 3, 16 near + 4 far    against torch.cdist + two topk over chunks of 1024 queries, timed on
                                                       --cdist-queries queries and scaled to N (the whole pass takes seconds)
  loss_feature3d, 10 000 rows, D = 32                  forward + backward, search included, against the reference's statements
                                                       (utils/loss_utils.py:162-175)
  loss_cls_3d, 200 000 rows, D = 32, C = 16, 800 rows  forward + backward, search included, against the reference's statements
                                                       (:112-130) on the same sample
  loss_feature3d(max_points=None), 300 000 rows        forward + backward; torch has no counterpart (a 360 GB matrix): the scaled
                                                       chunked search above stands beside it
  bench.py                                             this tree's library and --parent-lib (the parent commit's build) taking
                                                       turns, twice each, as fresh child processes under a time limit; a child that
                                                       ends with a non-zero status or without a result line ends this script at once

    python profiles/bench_dense_losses.py --parent-lib /path/to/parent/libtrase_rast.so --tests-log LOG > profiles/dense_losses_bench.json

--tests-log: the output of `pytest tests/test_gpu_dense.py -s`; the shares of the bar that the loss tests measured and the figures
of the random-cloud tests are copied into the result under "tests".
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_neighbors import alternate, bench_line  # noqa: E402
from trase_amd import neighbors as nb  # noqa: E402
from trase_amd.synthetic import make_scene  # noqa: E402

N = 300_000


def cdist_both_ends(q, cloud, kn, kf, chunk=1024):
    near, far = [], []
    for lo in range(0, q.shape[0], chunk):
        d = torch.cdist(q[lo:lo + chunk], cloud)
        if kn:
            near.append(d.topk(kn, largest=False).indices)
        if kf:
            far.append(d.topk(kf, largest=True).indices)
    return (torch.cat(near) if kn else None), (torch.cat(far) if kf else None)


def same_rows(a, b):
    return [int((a.sort(1).values == b.sort(1).values).all(1).sum()), int(a.shape[0])]


def reference_feature3d(feats, xyz, kp=16, kn=4, lambda_p=1.0, lambda_n=1.0):
    from torch.nn.functional import cosine_similarity
    n = feats.shape[0]
    dists = torch.cdist(xyz, xyz)
    _, nn_indices = dists.topk(kp, largest=False)
    _, fn_indices = dists.topk(kn, largest=True)
    an = torch.arange(n, device=feats.device).unsqueeze(-1).expand(n, kp).reshape(-1)
    af = torch.arange(n, device=feats.device).unsqueeze(-1).expand(n, kn).reshape(-1)
    near = lambda_p * torch.sigmoid(1 - cosine_similarity(feats[an, :], feats[nn_indices.reshape(-1), :], dim=1)).mean()
    far = lambda_n * torch.sigmoid(cosine_similarity(feats[af, :], feats[fn_indices.reshape(-1), :], dim=1)).mean()
    return near + far


def reference_cls3d(features, predictions, sample, k=5, lambda_val=2.0):
    sp = predictions[sample]
    dists = torch.cdist(features[sample], features)
    _, ni = dists.topk(k, largest=False)
    kl = sp.unsqueeze(1) * (torch.log(sp.unsqueeze(1) + 1e-10) - torch.log(predictions[ni] + 1e-10))
    return lambda_val * (kl.sum(dim=-1).mean() / predictions.size(1))


def test_records(path):
    """The largest figures among the printed lines of tests/test_gpu_dense.py."""
    out = {"largest_share_of_the_bar": {"value": 0.0, "gradient": 0.0}, "random_clouds": {}, "every_row": None}
    for ln in open(path, errors="replace"):
        ln = ln.strip().lstrip(".")
        if ln.endswith("of the bar"):
            kind = ln.split()[0]
            if kind in out["largest_share_of_the_bar"]:
                out["largest_share_of_the_bar"][kind] = max(out["largest_share_of_the_bar"][kind], float(ln.split(",")[-1].split()[0]))
        elif "largest relative distance error" in ln:
            out["random_clouds"][ln.split(":")[0]] = ln.split(": ", 1)[1]
        elif ln.startswith("65 537 rows"):
            out["every_row"] = ln
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--cdist-queries", type=int, default=8192)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--skip-bench", action="store_true")
    ap.add_argument("--tests-log", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    props = torch.cuda.get_device_properties(0)
    res = {"n": N, "reps": a.reps, "device": torch.cuda.get_device_name(0), "arch": props.gcnArchName,
           "compute_units": props.multi_processor_count}
    note = lambda what: print("[bench_dense_losses]", what, file=sys.stderr, flush=True)          # noqa: E731
    g = torch.Generator().manual_seed(1)
    xyz = make_scene(N, feat_dim=1, seed=3).xyz.to(dev).contiguous()
    feats = torch.nn.functional.normalize(torch.randn(N, 32, generator=g), dim=1).to(dev)

    res["dense_topk"] = {}
    note("dense_topk 10 000 x 10 000 x 3")
    x10 = xyz[:10_000].contiguous()
    (t, tmin), (c, cmin) = alternate([lambda: nb.dense_topk(x10, x10, 16, 4), lambda: cdist_both_ends(x10, x10, 16, 4, chunk=10_000)], a.reps)
    got, ref = nb.dense_topk(x10, x10, 16, 4), cdist_both_ends(x10, x10, 16, 4, chunk=10_000)
    res["dense_topk"]["10000x10000x3_16near_4far"] = {
        "ms": t, "cdist_topk_ms": c, "ratio": round(c / t, 2), "min_ms": [tmin, cmin], "splits": nb.dense_topk_splits(10_000, 10_000, 3, 16, 4),
        "rows_with_the_same_index_sets_as_cdist_topk": [same_rows(got[1], ref[0]), same_rows(got[3], ref[1])]}

    note("dense_topk 800 x 200 000 x 32")
    f200 = feats[:200_000].contiguous()
    sample = torch.randperm(200_000, generator=g)[:800].to(dev)
    q800 = f200[sample].contiguous()
    (t, tmin), (c, cmin) = alternate([lambda: nb.dense_topk(q800, f200, 5), lambda: cdist_both_ends(q800, f200, 5, 0)], a.reps)
    got, ref = nb.dense_topk(q800, f200, 5), cdist_both_ends(q800, f200, 5, 0)
    res["dense_topk"]["800x200000x32_5near"] = {
        "ms": t, "cdist_topk_ms": c, "ratio": round(c / t, 2), "min_ms": [tmin, cmin], "splits": nb.dense_topk_splits(800, 200_000, 32, 5, 0),
        "rows_with_the_same_index_set_as_cdist_topk": same_rows(got[1], ref[0])}

    note("dense_topk 300 000 x 300 000 x 3")
    q = xyz[:a.cdist_queries]
    (t, tmin), = alternate([lambda: nb.dense_topk(xyz, xyz, 16, 4)], a.reps, warmup=1)
    (c, cmin), = alternate([lambda: cdist_both_ends(q, xyz, 16, 4)], 5, warmup=1)
    got, ref = nb.dense_topk(q, xyz, 16, 4), cdist_both_ends(q, xyz, 16, 4)
    res["dense_topk"]["300000x300000x3_16near_4far"] = {
        "ms": t, "min_ms": tmin, "pairs_per_second": round(N * N / (t * 1e-3), 0), "splits": nb.dense_topk_splits(N, N, 3, 16, 4),
        "cdist_topk_ms_for_queries": [a.cdist_queries, c, cmin], "cdist_topk_ms_scaled_to_n": round(c * N / a.cdist_queries, 1),
        "rows_with_the_same_index_sets_as_cdist_topk": [same_rows(got[1], ref[0]), same_rows(got[3], ref[1])]}

    note("loss_feature3d, 10 000 rows")
    f10 = feats[:10_000].clone().requires_grad_(True)

    def ours_f3d():
        f10.grad = None
        nb.loss_feature3d(f10, x10).backward()

    def ref_f3d():
        f10.grad = None
        reference_feature3d(f10, x10).backward()
    (t, tmin), (r, rmin) = alternate([ours_f3d, ref_f3d], a.reps)
    ours_f3d()
    g_ours = f10.grad.clone()
    ref_f3d()
    res["loss_feature3d"] = {"rows": 10_000, "D": 32, "kp": 16, "kn": 4, "fwd_bwd_ms": t, "reference_statements_ms": r,
                             "ratio": round(r / t, 2), "min_ms": [tmin, rmin],
                             "largest_gradient_difference": float((g_ours - f10.grad).abs().max()),
                             "largest_gradient": float(f10.grad.abs().max())}

    note("loss_cls_3d, 200 000 rows")
    pred = torch.softmax(2.0 * torch.randn(200_000, 16, generator=g), dim=1).to(dev).requires_grad_(True)

    def ours_cls():
        pred.grad = None
        nb.loss_cls_3d(f200, pred, sample=sample).backward()

    def ref_cls():
        pred.grad = None
        reference_cls3d(f200, pred, sample).backward()
    (t, tmin), (r, rmin) = alternate([ours_cls, ref_cls], a.reps)
    ours_cls()
    g_ours = pred.grad.clone()
    ref_cls()
    res["loss_cls_3d"] = {"rows": 200_000, "D": 32, "C": 16, "k": 5, "sample_size": 800, "fwd_bwd_ms": t, "reference_statements_ms": r,
                          "ratio": round(r / t, 2), "min_ms": [tmin, rmin],
                          "largest_gradient_difference": float((g_ours - pred.grad).abs().max()),
                          "largest_gradient": float(pred.grad.abs().max())}

    note("loss_feature3d on every row")
    fall = feats.clone().requires_grad_(True)

    def ours_all():
        fall.grad = None
        nb.loss_feature3d(fall, xyz, max_points=None).backward()
    near, far = nb.dense_topk(xyz, xyz, 16, 4)[1::2]

    def ours_all_given():
        fall.grad = None
        nb.loss_feature3d(fall, xyz, max_points=None, neighbors=(near, far)).backward()
    (t, tmin), (s, smin) = alternate([ours_all, ours_all_given], a.reps, warmup=1)
    res["loss_feature3d_every_row"] = {"rows": N, "D": 32, "fwd_bwd_ms": t, "fwd_bwd_ms_with_given_neighbours": s, "min_ms": [tmin, smin],
                                       "torch": "no counterpart: cdist(xyz, xyz) is 360 GB; see cdist_topk_ms_scaled_to_n above"}

    if not a.skip_bench:
        torch.cuda.synchronize()          # a fault of the measurements above raises here, before any child is started
        runs = []
        for turn in range(2):
            note(f"bench.py, turn {turn}")
            runs.append({"tree": bench_line(None)})
            if a.parent_lib:
                runs[-1]["parent"] = bench_line(a.parent_lib)
        res["bench"] = runs
    if a.tests_log:
        res["tests"] = test_records(a.tests_log)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
