"""Generates feature_resized.npz: the FEATURE-state head of the imported reference as train.py:280-296 composes it when the
SAM masks are smaller than the render (``--downsample_mask``), run on the CPU.

    python tests/golden/make_feature_resized.py

A (32, 67, 35) feature image and 12 masks at 33 x 17 (67 // 2, 35 // 2: a non-integral ratio on both axes).  The reference's own
steps, in its order: the norm regulariser on the image as rendered (train.py:280-281), ``torch.nn.functional.interpolate(...,
sam_masks.shape[-2:], mode='bilinear')`` (:283), then ``get_pixel_mask_correspondence_matrix``,
``get_features_correspondence_matrix``, ``get_pixel_weights`` (utils/feature_utils.py) and the soft / all / hard pair losses
(utils/loss_utils.py), and the two mean similarities (:295-296).  Recorded: the inputs, the fixed ``sampled_pixel`` /
``sampled_mask``, per mode both losses, for the soft mode the fp32 gradient of their sum with respect to the FULL-resolution
features, the similarities, and the regulariser.  The archive holds data only and is written with fixed time stamps.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402  (the imported reference checkout)
from make_lift import write_npz  # noqa: E402

N, HR, WR, H, W = 12, 67, 35, 33, 17


def main():
    import_reference()
    from utils.feature_utils import (get_features_correspondence_matrix, get_pixel_mask_correspondence_matrix, get_pixel_weights)
    from utils.loss_utils import negative_pixel_pair_loss, positive_pixel_pair_loss
    torch.manual_seed(21)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    sam = torch.zeros(N, H, W, dtype=torch.bool)
    for k in range(N):                                      # overlapping boxes and discs, some pixels uncovered
        cy, cx = int(torch.randint(0, H, (1,))), int(torch.randint(0, W, (1,)))
        ry, rx = int(torch.randint(3, 12, (1,))), int(torch.randint(2, 7, (1,)))
        if k % 2:
            sam[k] = ((yy - cy).abs() <= ry) & ((xx - cx).abs() <= rx)
        else:
            sam[k] = ((yy - cy).float() / ry) ** 2 + ((xx - cx).float() / rx) ** 2 <= 1.0
    base = torch.randn(N, 32)
    big = torch.nn.functional.interpolate(sam.float()[None], size=(HR, WR), mode="nearest")[0]
    feat = (big.permute(1, 2, 0) @ base).permute(2, 0, 1) * 0.7 + 0.6 * torch.randn(32, HR, WR)
    sampled_pixel = (torch.rand(H, W) < 0.3) & (sam.sum(dim=0) != 0)
    sampled_pixel[H - 1, W - 1] = bool(sam[:, H - 1, W - 1].any())          # the corner whose taps end at the last row and column
    sampled_mask = torch.rand(N) < 0.6
    out = {"sam_masks": sam.numpy(), "features": feat.numpy(), "sampled_pixel": sampled_pixel.numpy(),
           "sampled_mask": sampled_mask.numpy(), "positive_th": 0.75, "negative_th": 0.5}
    Cm = get_pixel_mask_correspondence_matrix(sam, sampled_pixel, sampled_mask)
    Wm = get_pixel_weights(sam, sampled_pixel)
    for mode in ("soft", "all", "hard"):
        fr = feat.clone().requires_grad_(True)
        small = torch.nn.functional.interpolate(fr.unsqueeze(0), sam.shape[-2:], mode="bilinear").squeeze(0)      # train.py:283
        CFm = get_features_correspondence_matrix(small, sampled_pixel)
        lp = positive_pixel_pair_loss[mode](C=Cm, C_F=CFm, positive_th=0.75, weights=Wm)
        ln = negative_pixel_pair_loss[mode](C=Cm, C_F=CFm, negative_th=0.5, weights=Wm)
        (lp + ln).backward()
        out[f"{mode}_loss_pos"], out[f"{mode}_loss_neg"] = float(lp.detach()), float(ln.detach())
        if mode == "soft":                                  # (one dense gradient keeps the archive at a few hundred KB)
            out["soft_grad"] = fr.grad.numpy()
    with torch.no_grad():
        out["pos_similarity"] = float(CFm[Cm == 1].mean())  # train.py:295-296
        out["neg_similarity"] = float(CFm[Cm == 0].mean())
    out["reg"] = float((1 - feat.norm(dim=0, p=2).mean()) ** 2)             # train.py:280-281, before the resize
    print("S =", int(sampled_pixel.sum()), "sampled masks =", int(sampled_mask.sum()),
          {k: round(v, 6) for k, v in out.items() if isinstance(v, float)})
    path = os.path.join(HERE, "feature_resized.npz")
    write_npz(path, out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
