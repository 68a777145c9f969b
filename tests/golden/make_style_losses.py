"""Generates style_losses.npz from the imported reference's own functions (utils/loss_utils.py): masked_l1_loss, weighted_l1_loss,
l2_loss (:33-44), calc_mean_std (:230-238), gram_matrix (:240-249), cal_adain_style_loss (:251-262), cal_style_loss (:264-269)
and cal_mse_content_loss (:271-272), evaluated in float64 on seeded inputs, with their autograd gradients.  Data only.

    python tests/golden/make_style_losses.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402

STYLE_WEIGHT = 2.5


def main():
    import_reference()
    from utils import loss_utils as lu
    g = torch.Generator().manual_seed(20240)
    out = {}

    def leaf(t):
        return t.clone().requires_grad_(True)

    def record(name, fn, x, *rest):
        xl = leaf(x)
        v = fn(xl, *rest)
        v.backward()
        out[name], out[name + "_grad"] = v.detach().numpy(), xl.grad.numpy()

    # images (3, 10, 11): fp32-representable values held in float64, so the GPU sees the same numbers
    img = torch.rand(3, 10, 11, generator=g).double()
    gt = torch.rand(3, 10, 11, generator=g).double()
    mask_bool = torch.rand(10, 11, generator=g) > 0.4
    # (masked_l1_loss converts its mask with .float() and sums it in fp32: eighths keep that sum exact, so the value is a float64 one)
    mask_float = (torch.round(torch.rand(10, 11, generator=g) * 8) / 8).double()
    weight_hw = torch.rand(10, 11, generator=g).double()
    weight_chw = torch.rand(3, 10, 11, generator=g).double()
    out.update(img=img.numpy(), gt=gt.numpy(), mask_bool=mask_bool.numpy(), mask_float=mask_float.numpy(), weight_hw=weight_hw.numpy(),
               weight_chw=weight_chw.numpy())
    record("masked_bool", lu.masked_l1_loss, img, gt, mask_bool)
    record("masked_float", lu.masked_l1_loss, img, gt, mask_float)
    record("weighted_hw", lu.weighted_l1_loss, img, gt, weight_hw)
    record("weighted_chw", lu.weighted_l1_loss, img, gt, weight_chw)
    record("l2", lu.l2_loss, img, gt)

    # features: post-ReLU-like, with a channel offset so that the means matter
    for tag, (c, h, w, hs, ws_) in {"f8": (8, 5, 7, 4, 9), "f64": (64, 3, 4, 5, 3)}.items():
        x = torch.relu(torch.randn(1, c, h, w, generator=g) + 0.3).double()
        style = torch.relu(torch.randn(1, c, hs, ws_, generator=g) * 1.5 + 0.1).double()      # another spatial size
        content = torch.relu(torch.randn(1, c, h, w, generator=g) + 0.3).double()
        out.update({f"{tag}_x": x.numpy(), f"{tag}_style": style.numpy(), f"{tag}_content": content.numpy()})
        mean, std = lu.calc_mean_std(x)
        out.update({f"{tag}_mean": mean.numpy(), f"{tag}_std": std.numpy(), f"{tag}_gram": lu.gram_matrix(x).numpy()})
        # gradients of the two non-scalar functions under fixed seeded cotangents
        # (the Gram cotangent is the rank-one u v^T: two vectors instead of a matrix in the file)
        cm, cs = torch.randn(1, c, 1, generator=g).double(), torch.randn(1, c, 1, generator=g).double()
        cu, cv = torch.randn(c, generator=g).double(), torch.randn(c, generator=g).double()
        cg = torch.outer(cu, cv)
        out.update({f"{tag}_cot_mean": cm.numpy(), f"{tag}_cot_std": cs.numpy(), f"{tag}_cot_gram_u": cu.numpy(), f"{tag}_cot_gram_v": cv.numpy()})
        record(f"{tag}_mean_std_dot", lambda t: sum((a * b).sum() for a, b in zip(lu.calc_mean_std(t), (cm, cs))), x)
        record(f"{tag}_gram_dot", lambda t: (lu.gram_matrix(t) * cg).sum(), x)
        record(f"{tag}_adain", lu.cal_adain_style_loss, x, style)
        record(f"{tag}_style_loss", lu.cal_style_loss, x, style, STYLE_WEIGHT)
        record(f"{tag}_content_loss", lu.cal_mse_content_loss, x, content)
    out["style_weight"] = np.float64(STYLE_WEIGHT)
    # inputs and cotangents are fp32 values: stored as such (lossless), the results stay float64
    for k in list(out):
        if out[k].dtype == np.float64 and (k in ("img", "gt", "mask_float", "weight_hw", "weight_chw") or k.endswith(("_x", "_style", "_content"))
                                           or "_cot_" in k):
            assert np.array_equal(out[k].astype(np.float32).astype(np.float64), out[k]), k
            out[k] = out[k].astype(np.float32)
    path = os.path.join(HERE, "style_losses.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
