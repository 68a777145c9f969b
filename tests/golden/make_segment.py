"""Generates segment.npz from the imported reference's render.py (``postprocessing``, render.py:97-105, pulled out with
``ast``) driven the way the loop at render.py:334-345 drives it: for every id of a list, the query is the mean of the
current feature rows of the cluster and ``postprocessing`` normalises the feature tensor IN PLACE, the masks OR-ed over the
ids.  Two id lists over two "frames" on one copy of the features, as written -- so the first id of the first frame takes
its query from raw features and every later call from normalised ones.

    python tests/golden/make_segment.py

Records the features, the float cluster ids (as scene/gaussian_model.py:383-386 holds them), the four masks and the fp16
scores of every call.  Runs on the CPU only.
"""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF  # noqa: E402  (the imported reference checkout)

N, D, K = 4096, 32, 8
ID_LISTS = ([2, 5], [0, 3, 7])
FRAMES = 2
THRESHOLD = 0.8


def load_postprocessing():
    src = open(os.path.join(REF, "render.py")).read()
    fn = next(n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "postprocessing")
    ns = {"torch": torch}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "render.py", "exec"), ns)
    return ns["postprocessing"]


def make_features(seed=0):
    g = np.random.default_rng(seed)
    centres = g.standard_normal((K, D))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    labels = g.integers(0, K, N)
    sigma = g.uniform(0.04, 0.3, (N, 1))                  # cosine to the centre spread around the 0.8 threshold
    rows = centres[labels] + sigma * g.standard_normal((N, D))
    rows *= g.uniform(0.3, 3.0, (N, 1))                   # raw (unnormalised) features: the first call sees their mean
    return rows.astype(np.float32), labels


def main():
    postprocessing = load_postprocessing()
    feats, labels = make_features()
    param = torch.from_numpy(feats.copy()).unsqueeze(1)   # (N, 1, D): get_gaussian_features returns this tensor itself
    cluster_ids = torch.from_numpy(labels.astype(np.float32))
    masks, scores = [], []
    for _ in range(FRAMES):
        for segment_ids in ID_LISTS:
            segmented_mask = None
            for sid in segment_ids:
                pre_mask = (cluster_ids == sid)
                f = param.squeeze(1)
                q = param.squeeze(1)[pre_mask].mean(dim=0)
                qn = q / q.norm()          # the scores the call computes, recorded alongside (postprocessing returns the mask only)
                fn = f / f.norm(dim=-1, keepdim=True)
                scores.append((fn.half() @ qn.half().unsqueeze(-1))[:, 0].numpy())
                filtered_mask = postprocessing(f, q, score_threshold=THRESHOLD)
                post_mask = pre_mask & filtered_mask
                segmented_mask = post_mask if segmented_mask is None else segmented_mask | post_mask
            masks.append(segmented_mask.numpy())
    out = os.path.join(HERE, "segment.npz")
    np.savez_compressed(out, features=feats, cluster_ids=labels.astype(np.float32),
                        id_lists=np.array([l + [-1] * (3 - len(l)) for l in ID_LISTS], dtype=np.int32),
                        frames=np.int32(FRAMES), threshold=np.float64(THRESHOLD), masks=np.stack(masks),
                        scores=np.stack(scores).astype(np.float16))
    print("wrote", out, os.path.getsize(out), "bytes; mask sizes", [int(m.sum()) for m in masks])


if __name__ == "__main__":
    main()
