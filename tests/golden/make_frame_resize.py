"""Generates frame_resize.npz: one small opaque RGBA image taken through the reference's own on-the-fly ground-truth statements
(train.py:221-229) with ``PILtoTorch`` (utils/general_utils.py:22-28, imported from the reference checkout) at three camera
resolutions, and the sizes the reference's ``loadCam`` statements (utils/camera_utils.py:30-48) compute for a list of cameras.

    python tests/golden/make_frame_resize.py

The image is 67 x 35 (H x W) with alpha 255 everywhere, so train.py:227-228 takes the RGB branch and Pillow resizes an RGB image
(with alpha below 255 somewhere it would resize premultiplied RGBA values, which ``ByteFrame`` does not follow).
It holds random colours, a 0 / 255 checkerboard patch (the bicubic overshoot reaches both clamps) and constant patches.  The
resolutions (W, H): (17, 33) and (13, 20) shrink both axes by about 2 and 3, (70, 134) doubles both.  Per background and
resolution the archive keeps the fp32 frame after train.py:230's clamp.

As in make_frames.py one statement differs from train.py: ``Image.fromarray`` of current Pillow refuses the int8 array, so it is
passed as ``.view(np.uint8)`` -- the same bytes.  Runs on the CPU only; the archive is written with fixed time stamps.
"""
import os
import sys
import textwrap
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden import REF  # noqa: E402  (the imported reference checkout)
from make_lift import write_npz  # noqa: E402
from tests import frames_reference as fr  # noqa: E402
from tests import resize_reference as rr  # noqa: E402

H, W = 67, 35
RESOLUTIONS = [(17, 33), (13, 20), (70, 134)]                       # (W, H), as PILtoTorch takes them
BACKGROUNDS = (("bg0", (0.0, 0.0, 0.0)), ("bg1", (1.0, 1.0, 1.0)), ("bgc", (0.2, 0.5, 0.7)))
# (orig_w, orig_h, --resolution, resolution_scale): the multi-view video sets at the default, 2704 x 2028 at every setting, widths
# whose half, quarter or eighth ends in .5 (round goes to even), and sizes where int() cuts a fraction
CAMERAS = [(2704, 2028, r, 1.0) for r in (-1, 1, 2, 4, 8, 800)] + \
          [(2560, 1920, -1, 1.0), (2048, 1088, -1, 1.0), (1600, 1200, -1, 1.0), (1601, 901, -1, 1.0), (1352, 1014, -1, 1.0),
           (1001, 751, 2, 1.0), (1003, 753, 2, 1.0), (1002, 750, 4, 1.0), (1006, 754, 4, 1.0), (1004, 1012, 8, 1.0), (1917, 1075, 1, 1.0),
           (2704, 2028, -1, 2.0), (2704, 2028, 2, 2.0), (1001, 751, 1, 2.0), (1920, 1080, 640, 1.0), (1920, 1080, 1000, 1.0),
           (1920, 1080, 333, 1.0), (800, 800, -1, 1.0), (800, 800, 3, 1.0)]


def make_image():
    g = np.random.default_rng(28)
    rgba = g.integers(0, 256, (H, W, 4), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    board = (((yy // 2 + xx // 2) & 1) * 255).astype(np.uint8)
    rgba[8:40, 4:30, :3] = board[8:40, 4:30, None]                  # 2 x 2 squares of 0 and 255
    rgba[44:54, 0:12, :3] = 255
    rgba[56:67, 20:35, :3] = 0
    rgba[..., 3] = 255
    return rgba


def reference_frame(im_data, background, resolution):
    """Runs train.py:222-229 -- read from the reference checkout, not restated here -- on the array of :221, on the CPU."""
    sys.path.insert(0, REF)
    from utils.general_utils import PILtoTorch
    lines = open(os.path.join(REF, "train.py")).read().split("\n")[221:229]
    code = textwrap.dedent("\n".join(lines))
    assert code.startswith("norm_data = im_data / 255.0") and code.count("dtype=np.byte)") == 2
    code = code.replace("dtype=np.byte)", "dtype=np.byte).view(np.uint8)")          # (Pillow >= 12 refuses the int8 array itself)
    ns = {"np": np, "Image": Image, "PILtoTorch": PILtoTorch, "im_data": im_data, "background": background,
          "viewpoint_cam": types.SimpleNamespace(image_width=resolution[0], image_height=resolution[1])}
    exec(compile(code, "train.py", "exec"), ns)
    assert ns["arr"].shape == (H, W, 3)                                              # alpha is 1 everywhere: the RGB variant
    return ns["gt_image"].clamp(0.0, 1.0)


def reference_sizes():
    """Runs utils/camera_utils.py:30-48 (the size computation of loadCam) for every entry of CAMERAS."""
    lines = open(os.path.join(REF, "utils", "camera_utils.py")).read().split("\n")[29:48]
    code = textwrap.dedent("\n".join(lines))
    assert code.startswith("orig_w, orig_h = cam_info.image.size") and code.rstrip().endswith("int(orig_h / scale))")
    out = []
    for w, h, resolution, resolution_scale in CAMERAS:
        ns = {"args": types.SimpleNamespace(resolution=resolution), "resolution_scale": resolution_scale, "WARNED": True,
              "cam_info": types.SimpleNamespace(image=types.SimpleNamespace(size=(w, h)))}
        exec(compile(code, "camera_utils.py", "exec"), ns)
        out.append(ns["resolution"])
    return out


def main():
    rgba = make_image()
    arrays = {"rgba": rgba}
    for name, value in BACKGROUNDS:
        background = torch.tensor(value, dtype=torch.float32)
        for res in RESOLUTIONS:
            frame = reference_frame(rgba, background, res)
            assert frame.dtype == torch.float32 and tuple(frame.shape) == (3, res[1], res[0])
            mine = rr.resize(fr.composite(rgba, background.numpy()), res)
            same = np.array_equal(fr.to_float(mine).transpose(2, 0, 1), frame.numpy())
            print(f"{name} {res}: the numpy restatement {'equals' if same else 'DIFFERS from'} the reference's frame; "
                  f"bytes {int(mine.min())}..{int(mine.max())}")
            assert same
            arrays[f"frame_{name}_{res[0]}x{res[1]}"] = frame.numpy()
    sizes = reference_sizes()
    for cam, size in zip(CAMERAS, sizes):
        mine = rr.camera_resolution(*cam)
        print(cam, "->", size, "" if tuple(mine) == tuple(size) else f"restatement DIFFERS: {mine}")
        assert tuple(mine) == tuple(size)
    arrays["cameras"] = np.array([c[:3] for c in CAMERAS], dtype=np.int64)
    arrays["camera_scales"] = np.array([c[3] for c in CAMERAS], dtype=np.float64)
    arrays["camera_sizes"] = np.array(sizes, dtype=np.int64)
    out = os.path.join(HERE, "frame_resize.npz")
    write_npz(out, arrays)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
