"""Generates frames.npz: one small RGBA image taken through the reference's own on-the-fly ground-truth statements
(train.py:221-229) and its ``PILtoTorch`` (utils/general_utils.py:22-28, imported from the reference checkout), for the
backgrounds 0 and 1.

    python tests/golden/make_frames.py

The image is 67 x 35 (H x W) RGBA with random colours and alphas, a patch that is black and opaque (it stays black over any
background), a patch that is black and transparent (it takes the background), and an opaque patch (its colours must come
through unchanged).  Per background the archive keeps the bytes the reference hands to PIL and the fp32 frame PILtoTorch
returns from them; alpha is below 1 somewhere, so both are the 4-channel variant of train.py:224-226 and the consumers use
the first three channels (utils/camera_utils.py:51).

One statement differs from train.py:226: ``Image.fromarray`` of current Pillow refuses the int8 array that older Pillow
reinterpreted as bytes, so the array is passed as ``.view(np.uint8)`` -- the same bytes.  Runs on the CPU only; the archive is
written with fixed time stamps.
"""
import os
import sys

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden import REF  # noqa: E402  (the imported reference checkout)
from make_lift import write_npz  # noqa: E402
from tests import frames_reference as fr  # noqa: E402

H, W = 67, 35


def make_image():
    g = np.random.default_rng(20)
    rgba = g.integers(0, 256, (H, W, 4), dtype=np.uint8)
    rgba[10:40, 5:20, :3] = 0
    rgba[10:40, 5:20, 3] = 255            # black and opaque: black over any background (rows 30..39 cross the 32-row tile edge)
    rgba[50:60, 20:33] = 0                # black and transparent: the background shows
    rgba[0:8, 25:35, 3] = 255             # opaque: the colours come through unchanged
    rgba[3, 30, :3] = (0, 0, 7)           # zero in two channels only: not black
    return rgba


def reference_frame(im_data, background):
    """Runs train.py:222-229 -- read from the reference checkout, not restated here -- on the array of :221, on the CPU.
    Returns the bytes handed to PIL (recomputed from the statements' own ``arr``) and the frame after :230's clamp."""
    import textwrap
    import types
    sys.path.insert(0, REF)
    from utils.general_utils import PILtoTorch
    lines = open(os.path.join(REF, "train.py")).read().split("\n")[221:229]
    code = textwrap.dedent("\n".join(lines))
    assert code.startswith("norm_data = im_data / 255.0") and code.count("dtype=np.byte)") == 2
    code = code.replace("dtype=np.byte)", "dtype=np.byte).view(np.uint8)")          # (Pillow >= 12 refuses the int8 array itself)
    ns = {"np": np, "Image": Image, "PILtoTorch": PILtoTorch, "im_data": im_data, "background": background,
          "viewpoint_cam": types.SimpleNamespace(image_width=W, image_height=H)}
    exec(compile(code, "train.py", "exec"), ns)
    assert ns["arr"].shape == (H, W, 4)                                              # alpha < 1 somewhere: the RGBA variant
    as_bytes = np.array(ns["arr"] * 255.0, dtype=np.byte).view(np.uint8)
    return as_bytes, ns["gt_image"].clamp(0.0, 1.0)


def main():
    rgba = make_image()
    arrays = {"rgba": rgba}
    for name, value in (("bg0", 0.0), ("bg1", 1.0)):
        background = torch.tensor([value] * 3, dtype=torch.float32)
        as_bytes, frame = reference_frame(rgba, background)
        assert frame.dtype == torch.float32 and tuple(frame.shape) == (4, H, W)
        mine = fr.composite(rgba, background.numpy())
        same = np.array_equal(mine, as_bytes[..., :3])
        exact = np.array_equal(fr.to_float(as_bytes).transpose(2, 0, 1), frame.numpy())
        print(f"{name}: the numpy composite {'equals' if same else 'DIFFERS from'} the reference's bytes; "
              f"float32(b) / 255 {'equals' if exact else 'DIFFERS from'} PILtoTorch's frame")
        assert same and exact
        assert np.array_equal(as_bytes[0:8, 25:35, :3], rgba[0:8, 25:35, :3])          # the opaque patch keeps its values
        arrays[f"bytes_{name}"] = as_bytes
        arrays[f"frame_{name}"] = frame.numpy()
    out = os.path.join(HERE, "frames.npz")
    write_npz(out, arrays)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
