"""Drop-in for the reference's ``gaussian_renderer`` package (``from gaussian_renderer import render`` at
train.py:24, train_style_transfer_nnfm.py:24, render.py:25, gui.py:23): put this repository BEFORE the
reference checkout on PYTHONPATH and the training / rendering scripts run unmodified on the fused
MI355X path.  ``render_composite`` and its rigid-edit helpers (gaussian_renderer/__init__.py:158-331 of the reference)
are trase_amd/edit.py's."""
from trase_amd.renderer import render  # noqa: F401
from trase_amd.layers import render_layers  # noqa: F401
from trase_amd.edit import (render_composite, rescale, rotate_by_euler_angles, rotate_by_matrix, rotmat2qvec,  # noqa: F401
                            rx, ry, rz, transform, translation)

try:   # render.py:30 imports GaussianModel through this module; available when run inside the reference tree
    from scene.gaussian_model import GaussianModel  # noqa: F401
except Exception:   # pragma: no cover
    pass

__all__ = ["render", "render_layers", "render_composite", "rotmat2qvec", "rx", "ry", "rz", "rescale", "rotate_by_euler_angles",
           "rotate_by_matrix", "translation", "transform"]
