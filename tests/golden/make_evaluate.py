"""Generates evaluate.npz from the imported reference: ``compute_iou`` and ``compute_acc`` of metrics_segmentation.py
(:33-48) and ``psnr`` of utils/image_utils.py (:17-19) are IMPORTED (with the ``sys.modules`` stubs of make_golden.py plus
stand-ins for the packages metrics_segmentation.py imports at its top and never uses in these functions) and called on
seeded 24 x 20 masks and 8-bit image pairs.

    python tests/golden/make_evaluate.py

Mask cases (prediction, ground truth), all (20, 24) bool: random, empty prediction, empty union, identical, full.
Image cases, (3, 20, 24) uint8: random, identical (PSNR inf), one 8-bit step apart everywhere, a cut-out-like pair.
``psnr`` is called as metrics_segmentation.py:144 calls it -- on ``byte / 255`` tensors with a leading batch axis -- once on
float64 tensors (``psnr``: what the float64 scores are compared with) and once on fp32 tensors as ``to_tensor`` makes them
(``psnr_f32``).  Runs on the CPU only; the archive regenerates byte for byte.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden import _stub, import_reference  # noqa: E402
from make_lift import write_npz  # noqa: E402

W, H = 24, 20


def load_reference():
    import_reference()
    for name in ("PIL", "PIL.Image", "torchvision.transforms", "torchvision.transforms.functional", "lpipsPyTorch", "tqdm"):
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                _stub(name)
    sys.modules["PIL"].Image = getattr(sys.modules["PIL"], "Image", sys.modules["PIL.Image"])
    if not hasattr(sys.modules["lpipsPyTorch"], "lpips"):
        sys.modules["lpipsPyTorch"].lpips = None
    if not hasattr(sys.modules["tqdm"], "tqdm"):
        sys.modules["tqdm"].tqdm = None
    import metrics_segmentation as ms
    from utils.image_utils import psnr
    return ms.compute_iou, ms.compute_acc, psnr


def main():
    compute_iou, compute_acc, psnr = load_reference()
    g = np.random.default_rng(20)
    rnd = lambda p: g.random((H, W)) < p
    blob = np.zeros((H, W), dtype=bool)
    blob[5:15, 6:19] = True
    masks = [(rnd(0.5), rnd(0.4)), (np.zeros((H, W), dtype=bool), rnd(0.3)), (np.zeros((H, W), dtype=bool), np.zeros((H, W), dtype=bool)),
             (blob, blob.copy()), (np.ones((H, W), dtype=bool), np.ones((H, W), dtype=bool)), (blob, np.roll(blob, (2, -3), (0, 1)))]
    pred = np.stack([m[0] for m in masks])
    gt = np.stack([m[1] for m in masks])
    iou = np.array([float(compute_iou(p, q)) for p, q in masks], dtype=np.float64)
    acc = np.array([float(compute_acc(p, q)) for p, q in masks], dtype=np.float64)

    a = g.integers(0, 256, (3, H, W), dtype=np.uint8)
    b = g.integers(0, 256, (3, H, W), dtype=np.uint8)
    step = g.integers(0, 255, (3, H, W), dtype=np.uint8)
    cut = (a * blob[None]).astype(np.uint8)
    noisy = np.clip(cut.astype(np.int64) + g.integers(-6, 7, cut.shape), 0, 255).astype(np.uint8)
    images = [(a, b), (a, a.copy()), (step, (step + 1).astype(np.uint8)), (cut, noisy)]
    img = np.stack([p[0] for p in images])
    img_gt = np.stack([p[1] for p in images])

    def ref_psnr(x, y, dtype):
        tx = (torch.from_numpy(x).to(dtype) / 255).unsqueeze(0)
        ty = (torch.from_numpy(y).to(dtype) / 255).unsqueeze(0)
        return float(psnr(tx, ty).reshape(-1)[0])

    ps64 = np.array([ref_psnr(x, y, torch.float64) for x, y in images], dtype=np.float64)
    ps32 = np.array([ref_psnr(x, y, torch.float32) for x, y in images], dtype=np.float64)
    assert np.isinf(ps64[1]) and np.isinf(ps32[1]) and iou[1] == 0.0 and iou[2] == 0.0 and acc[2] == 1.0 and iou[3] == 1.0
    for name, v in (("IoU", iou), ("ACC", acc), ("PSNR float64", ps64), ("PSNR fp32", ps32)):
        print(f"{name:14s}", v.tolist())
    path = os.path.join(HERE, "evaluate.npz")
    write_npz(path, dict(pred=pred, gt=gt, iou=iou, acc=acc, image=img, image_gt=img_gt, psnr=ps64, psnr_f32=ps32))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
