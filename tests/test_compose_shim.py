"""The shim exports the reference's editing entry point and its nine helpers, and every helper reproduces the outputs the
reference's own functions wrote into tests/golden/compose.npz, on CPU tensors, within the forward-error bounds of
tests/compose_reference.py."""
import numpy as np
import torch

from tests import compose_reference as cr
from tests.test_compose_reference import _inside, edit_of, fixture

T = torch.from_numpy


def test_the_reference_names_import_from_the_shim():
    from gaussian_renderer import (render_composite, transform, rotmat2qvec, rx, ry, rz, rescale,  # noqa: F401
                                   rotate_by_euler_angles, rotate_by_matrix, translation)
    import inspect
    assert list(inspect.signature(render_composite).parameters)[:12] == [
        "viewpoint_camera", "background_gaussian", "dynamic_gaussian", "d_xyz", "d_rotation", "d_scaling", "bg_color",
        "scales_bias", "motion_bias", "rotation_bias", "scaling_modifier", "mask"]
    assert list(inspect.signature(transform).parameters) == ["means3d", "rotations", "scales", "scale_factor", "offsets",
                                                             "rotation_angles"]
    assert list(inspect.signature(rotate_by_matrix).parameters) == ["means3d", "rotations", "rotation_matrix", "keep_sh_degree"]


def test_axis_rotations_and_quaternion_match_the_fixture():
    from gaussian_renderer import rotmat2qvec, rx, ry, rz
    z = fixture()
    one = 2 * cr.U * np.ones((3, 3))                     # one transcendental per entry, values <= 1
    for k, f in enumerate((rx, ry, rz)):
        name = "r" + "xyz"[k]
        for theta in (torch.tensor(z["edit_angles"][k]), float(z["edit_angles"][k])):       # tensor, and (deviation) a float
            got = f(theta)
            assert got.dtype == torch.float32 and tuple(got.shape) == (3, 3)
            _inside(name, got.numpy(), z[name].astype(np.float64), one)
    q = rotmat2qvec(T(z["R"]))
    assert q.dtype == torch.float32 and float(q[0]) >= 0
    _inside("rotmat2qvec", q.numpy(), z["q"].astype(np.float64), cr.ROT_ROUNDINGS * cr.U * np.ones(4))


def test_rescale_translation_and_rotations_match_the_fixture():
    from gaussian_renderer import rescale, rotate_by_euler_angles, rotate_by_matrix, translation
    z = fixture()
    m, s = rescale(T(z["means_in"][:64].copy()), T(z["scales_in"][:64].copy()), float(z["edit_scale"]))
    assert np.array_equal(m.numpy(), z["rescale_means"]) and np.array_equal(s.numpy(), z["rescale_scales"])   # one rounding each
    moved = translation(T(z["means_in"][:64].copy()), T(z["edit_offset"]))
    assert np.array_equal(moved.numpy(), z["translation_means"])
    e = cr.make_edit(1.0, R=z["R"])
    _, _, _, b = cr.edit_activated(z["means_in"], z["rots_in"], z["scales_in"], e)
    for name, got in (("rotate_by_matrix", rotate_by_matrix(T(z["means_in"].copy()), T(z["rots_in"].copy()), T(z["R"]))),
                      ("rotate_by_euler_angles", rotate_by_euler_angles(T(z["means_in"].copy()), T(z["rots_in"].copy()),
                                                                        [torch.tensor(a) for a in z["edit_angles"]]))):
        _inside(name + " means", got[0].numpy(), z["matrix_means"].astype(np.float64), b["means"])   # 8 roundings
        _inside(name + " rots", got[1].numpy(), z["matrix_rots"].astype(np.float64), b["rots"])      # 16 roundings
    same = rotate_by_euler_angles(T(z["means_in"]), T(z["rots_in"]), (0.0, 0.0, 0.0))
    assert same[0].data_ptr() == T(z["means_in"]).data_ptr() or np.array_equal(same[0].numpy(), z["means_in"])
    assert np.array_equal(same[1].numpy(), z["rots_in"])


def test_transform_matches_the_fixture():
    from gaussian_renderer import transform
    z = fixture()
    for tag, scale, offset, angles in (("edit", float(z["edit_scale"]), z["edit_offset"], z["edit_angles"]),
                                       ("zero", float(z["zero_scale"]), z["zero_offset"], np.zeros(3, dtype=np.float32))):
        _, _, _, b = cr.edit_activated(z["means_in"], z["rots_in"], z["scales_in"], edit_of(z, tag))
        m, q, s = transform(T(z["means_in"].copy()), T(z["rots_in"].copy()), T(z["scales_in"].copy()), scale, T(offset),
                            [torch.tensor(a) for a in angles])
        _inside(f"{tag} means", m.numpy(), z[f"{tag}_means"].astype(np.float64), b["means"])      # 8 roundings
        _inside(f"{tag} rots", q.numpy(), z[f"{tag}_rots"].astype(np.float64), b["rots"])         # 16 roundings
        _inside(f"{tag} scales", s.numpy(), z[f"{tag}_scales"].astype(np.float64), b["scales"])   # 2 roundings
    assert np.array_equal(q.numpy(), z["rots_in"])               # zero angles: returned as given


def test_rigid_edit_record():
    from trase_amd.edit import quat_to_rotmat64, rigid_edit
    z = fixture()
    e = rigid_edit(float(z["edit_scale"]), [torch.tensor(a) for a in z["edit_angles"]], T(z["edit_offset"]))
    assert not e.zero_angles and e.R.dtype == np.float32 and e.q.dtype == np.float32 and e.q[0] >= 0
    assert float(np.abs(quat_to_rotmat64(e.q64) - e.R64).max()) < 4e-15     # R(q_edit) reproduces R
    assert float(np.abs(e.R64 - cr.euler_matrix(z["edit_angles"])).max()) < 1e-15
    assert float(np.abs(e.q64 - cr.qvec(e.R64)).max()) < 1e-15              # eigenvector form against the closed form
    assert np.array_equal(e.R, e.R64.astype(np.float32)) and np.array_equal(e.q, e.q64.astype(np.float32))   # rounded once
    assert float(np.abs(e.R - z["R"]).max()) <= 2 ** -23                    # the reference's fp32 R: one rounding of an entry away
    f = rigid_edit(2.0, (0.0, 0.0, 0.0), (1.0, 2.0, 3.0))
    assert f.zero_angles and rigid_edit(1.0, (0.0, 1e-30, 0.0)).zero_angles is False


def test_cpu_tensors_and_bad_part_lists_are_rejected():
    import ctypes as C
    import pytest
    from trase_amd import _lib
    from trase_amd.edit import Part, compose_models
    from trase_amd.synthetic import SynthGaussianModel, make_scene
    pc = SynthGaussianModel(make_scene(16, feat_dim=8, seed=0), requires_grad=False)
    with pytest.raises(RuntimeError, match="GPU only"):
        compose_models([Part(pc)])
    with pytest.raises(ValueError, match="1 to 8 parts"):
        compose_models([])
    with pytest.raises(ValueError, match="mask entries"):
        Part(pc, rows=torch.ones(15, dtype=torch.bool))
    lib = _lib.load()
    offsets = (C.c_int64 * 9)()
    assert lib.trase_compose_sizes((C.c_int32 * 2)(600, 950), 2, 32, offsets) == 0 and list(offsets[:3]) == [0, 600, 1550]
    assert lib.trase_compose_sizes((C.c_int32 * 9)(), 9, 32, offsets) != 0 and b"parts" in lib.trase_last_error()
    assert lib.trase_compose_sizes((C.c_int32 * 1)(-1), 1, 32, offsets) != 0
    assert lib.trase_compose_sizes((C.c_int32 * 1)(5), 1, 65, offsets) != 0
