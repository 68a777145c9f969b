#!/usr/bin/env python
"""The deformation MLP's inference forward at N Gaussians in its two precisions against the wrapped torch fp32 network:
``deform_forward(precision="bf16")``, ``deform_forward(precision="bf16x3")`` (split-bf16 operands, trase_amd/csrc/mlp_split.hip)
and ``net(x, t)``.  The three paths take turns in one process; every figure is the median of 30 HIP-event timings after a
pre-roll.  Also records the error table of tests/test_gpu_mlp_precise.py (every case at its largest size, and the image-level
figures) and, when given, the result lines of bench.py on this tree and on the parent commit (several files each: runs that
took turns; ``tree`` / ``parent`` are the last of them, ``views_per_s_taking_turns`` lists them all).

    python profiles/bench_mlp_precise.py [--n 300000] [--bench-tree FILE ...] [--bench-parent FILE ...] [--out profiles/mlp_precise.json]

Exits 1 when the split forward is not faster than the torch fp32 network: the mode then has no reason to exist."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trase_amd.deform import deform_forward  # noqa: E402
from trase_amd.synthetic import SynthDeformNetwork  # noqa: E402

ROUNDS, PREROLL = 30, 10


def last_json_line(path):
    if not path:
        return None
    for line in reversed(open(path).read().splitlines()):
        line = line.strip()
        if line.startswith("{"):
            return json.loads(line)
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=300_000)
    ap.add_argument("--bench-tree", nargs="*", default=[], help="files holding bench.py's result line on this tree, in run order")
    ap.add_argument("--bench-parent", nargs="*", default=[], help="files holding bench.py's result line on the parent commit")
    ap.add_argument("--no-error-table", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "mlp_precise.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    net = SynthDeformNetwork().to(dev)
    n = args.n
    x = (torch.rand(n, 3, device=dev) * 2 - 1) * 1.3
    t = torch.tensor([[0.4]], device=dev).expand(n, -1)
    tc = t.contiguous()
    params = dict(net.state_dict())
    paths = {"bf16": lambda: deform_forward(params, x, t),
             "bf16x3": lambda: deform_forward(params, x, t, precision="bf16x3"),
             "torch_fp32": lambda: net(x, tc)}
    ms = {k: [] for k in paths}
    with torch.no_grad():
        for r in range(PREROLL + ROUNDS):
            for k, fn in paths.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if r >= PREROLL:
                    ms[k].append(e0.elapsed_time(e1))
        outs = {k: fn() for k, fn in paths.items()}
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {"n": n, "rounds": ROUNDS, "preroll": PREROLL,
           "call_ms_median": {k: round(v, 4) for k, v in med.items()},
           "call_ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
           "bf16x3_over_bf16": round(med["bf16x3"] / med["bf16"], 3),
           "torch_fp32_over_bf16x3": round(med["torch_fp32"] / med["bf16x3"], 3),
           "split_faster_than_torch_fp32": med["bf16x3"] < med["torch_fp32"],
           "max_abs_d_xyz_vs_torch_fp32": {k: float((outs[k][0] - outs["torch_fp32"][0]).abs().max()) for k in ("bf16", "bf16x3")}}
    if not args.no_error_table:
        from tests import test_gpu_mlp_precise as T
        table = {}
        for case in T.CASES:
            figs, _ = T.measure_case(*case, max(T.SIZES), dev)
            table["/".join(str(c) for c in case)] = figs
        out["error_table"] = {"factor": T.FACTOR, "rows": max(T.SIZES), "unit": "max|float64| of the output", "cases": table}
        out["image_level"] = T.measure_image(dev)
    lines = {"tree": [last_json_line(f) for f in args.bench_tree], "parent": [last_json_line(f) for f in args.bench_parent]}
    out["bench_py"] = {"tree": lines["tree"][-1] if lines["tree"] else None, "parent": lines["parent"][-1] if lines["parent"] else None,
                       "views_per_s_taking_turns": {k: [ln["value"] for ln in v if ln] for k, v in lines.items()}}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("n", "call_ms_median", "bf16x3_over_bf16", "torch_fp32_over_bf16x3",
                                          "split_faster_than_torch_fp32")}))
    if not out["split_faster_than_torch_fp32"]:
        print("the split forward is NOT faster than the torch fp32 network: the mode has no reason to exist", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
