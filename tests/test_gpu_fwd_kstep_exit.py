"""The MFMA forward (render_fwd_mf.hip) leaves the K-step loop of a 64-entry chunk at the first 16-entry step its wave enters
without a live pixel.  The skipped steps have all-zero weights, so nothing may move: maps, final_T, n_contrib (checked through
the backward, which reads both) and bit-reproducibility.

Scenes: a stack of N wide Gaussians (sigma = 150 px on a 16x8 or 12x10 image) centred just above the image at distinct depths, one
opacity for the whole stack, so alpha is the opacity to within 0.5 % at every pixel and the stop rule T (1 - alpha) < 1e-4 fires
at a list position the opacity chooses: in K-step 0, 1, 2, 3 of the first chunk, inside the second chunk, or never (list
exhausted).  N = 150 (> 128, 150 = 9 * 16 + 6).  Two more cases centre a stack of sigma_y = 12 px Gaussians 22 px above
(below) the image, so that the rows of wave 0 finish one to two chunks before (after) the rows of wave 1.  The float64 oracle
must place every pixel's finishing entry where the case intends -- asserted in every case before any comparison.

Bars: against the oracle, the helpers and bars of tests/test_gpu_parity.py (maps 1e-4, gradients rtol 1e-3 + 1e-5 of scale).
Default forward against the packed-FP32 forward (TRASE_VARIANT_VALU_FORWARD), maps and the gradients of the default backward
run after each: test_gpu_parity.py has no map comparison between the two formulations; its rule wherever the MFMA and the
packed-FP32 formulation of one computation meet is 2e-5 of the tensor's scale (+ 1e-9), and 2e-5 is also its per-pixel bar
between two routes to the same maps.  The same rule is used here: both forwards blend the same entries with fp32 weights; the
bf16-split contraction (three products per term) is exact to ~2^-16 of each term and the weights sum to at most 1.

K-step 0 is reached with opacity 0.85 (four entries blended), not with 0.98 .. 0.99 (two): dL/dalpha carries a factor
1 / (1 - alpha), 50 at 0.98, which multiplies the ~1e-5 rounding of the MFMA backward's bf16-split contractions; with only two
Gaussians receiving a gradient the relative L2 error of means2D against the oracle was measured at 2.1e-4 (bar 2e-4; 2.4e-5 with
the packed-FP32 backward; the same figures whichever forward ran, and outputs bit-identical to the kernel without the exit).  That
is the conditioning of the backward at alpha -> 0.99, not something a forward can move; 1 - alpha >= 0.1 keeps the factor <= 10."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

FOCAL_MULT = 50.0        # focal = 50 W: world-space sigmas of 0.56..0.94 at depth 3..5 on a 16 px wide image
SIGMA_PX = 150.1         # (3 sigma = 450.3: no radius sits on its ceil())
N_STACK = 150
NAMES = ["means3D", "means2D", "opacities", "scales", "rotations", "shs", "sh_objs"]

# name: (W, H, N, opacity, (image row of the stack's centre, sigma_y in px), expectation)
#   expectation ("kstep", k): every pixel finishes in global K-step k (entry index // 16; 4 K-steps per chunk)
#               ("never",):    no pixel finishes, n_contrib = N
#               ("waves", first): the rows of wave `first` of the sub-tile finish at least one chunk before the other wave's
WIDE = (-6.0, SIGMA_PX)  # isotropic, centred 6 px above row 0: no pixel within float32 rounding of the centre (the gate power <= 0)
CASES = {
    "kstep0": (16, 8, N_STACK, 0.85, WIDE, ("kstep", 0)),       # (not 0.98 .. 0.99: see the module docstring)
    "kstep1": (16, 8, N_STACK, 0.35, WIDE, ("kstep", 1)),
    "kstep2": (16, 8, N_STACK, 0.20, WIDE, ("kstep", 2)),
    "kstep3": (16, 8, N_STACK, 0.155, WIDE, ("kstep", 3)),
    "chunk1": (16, 8, N_STACK, 0.10, WIDE, ("kstep", 5)),
    "never": (16, 8, N_STACK, 0.05, WIDE, ("never",)),
    "ragged": (12, 10, N_STACK, 0.155, WIDE, ("kstep", 3)),
    "wave0_first": (16, 8, 182, 0.99, (-22.0, 12.0), ("waves", 0)),
    "wave1_first": (16, 8, 182, 0.99, (7.0 + 22.0, 12.0), ("waves", 1)),
}


def stack_case(w, h, n, opacity, centre):
    """Activated inputs (CPU) and camera.  The camera sits at (0, 0, 4) looking down -z: view x = world x, view y = -world y,
    view depth = 4 - world z; pixel = (W / 2 - 0.5 + focal x_v / z, H / 2 - 0.5 + focal y_v / z)."""
    from trase_amd.synthetic import orbit_camera
    cam = orbit_camera(w, h, angle=0.0, radius=4.0, elevation=0.0, focal_mult=FOCAL_MULT)
    focal = FOCAL_MULT * w
    g = torch.Generator().manual_seed(n + w)
    z = torch.linspace(3.0, 5.0, n, dtype=torch.float64)             # distinct depths, 0.013 apart
    means = torch.zeros(n, 3, dtype=torch.float64)
    means[:, 2] = 4.0 - z
    scales = (SIGMA_PX * z / focal)[:, None].repeat(1, 3)            # the same 150.1 px (radius 451) at every depth
    cy, sigma_y = centre
    means[:, 1] = -(cy - h / 2 + 0.5) * z / focal
    scales[:, 1] = sigma_y * z / focal
    rot = torch.zeros(n, 4)
    rot[:, 0] = 1.0
    shs = torch.zeros(n, 16, 3)
    shs[:, 0] = (torch.rand(n, 3, generator=g) - 0.5) / 0.28209479177387814
    f = torch.rand(n, 1, 32, generator=g) - 0.5
    act = dict(means3D=means.float(), scales=scales.float(), rotations=rot, opacities=torch.full((n, 1), opacity), shs=shs,
               sh_objs=f / (f.norm(dim=2, keepdim=True) + 1e-9))
    return act, cam


def check_finishing_places(name, o):
    """The oracle's n_contrib is the number of blended entries: the pixel is finished by entry index n_contrib."""
    w, h, n, _, _, want = CASES[name]
    nc = o.n_contrib
    assert not bool(o.fragile.any()), f"{name}: {int(o.fragile.sum())} pixels sit on a gate"
    if want[0] == "never":
        assert bool((nc == n).all()), (name, nc.unique().tolist())
    elif want[0] == "kstep":
        assert bool((nc < n).all()) and bool((nc // 16 == want[1]).all()), (name, nc.unique().tolist())
    else:
        first, other = (nc[0:4], nc[4:8]) if want[1] == 0 else (nc[4:8], nc[0:4])
        assert bool((nc < n).all()), (name, nc.unique().tolist())
        # a whole chunk earlier, and in the chunk both still walk the first wave is done K-steps before any row of the other
        assert int(first.max()) // 64 < int(other.max()) // 64, (name, int(first.max()), int(other.max()))
        assert int(first.max()) // 16 < int(other.min()) // 16, (name, int(first.max()), int(other.min()))


@functools.lru_cache(maxsize=None)
def run_case(name):
    """One case, computed once and shared (read-only) by the tests: the oracle with its gradients, then on the GPU the default
    forward twice and the packed-FP32 forward once, each followed by the default backward."""
    from tests import test_gpu_parity as T
    from tests.util import settings_for
    from trase_amd import rasterizer as R
    w, h, n, opacity, centre, _ = CASES[name]
    act, cam = stack_case(w, h, n, opacity, centre)
    st = settings_for(cam, bg=(0.1, 0.25, 0.4))
    gen = torch.Generator().manual_seed(17)
    gi, gf = torch.randn(3, h, w, generator=gen), torch.randn(32, h, w, generator=gen)
    runs = {}
    v0 = R._Policy.variant
    try:
        for tag, bit in (("mfma", 0), ("mfma2", 0), ("valu", 0x2000)):
            R.set_variant(v0 | bit)
            out, leaves = T._gpu_call(act, st)
            if tag == "mfma":
                o, ol = T._oracle_call(act, st, gpu=out)             # adopts the device view of the forward that just ran
            runs[tag] = (out, leaves)
    finally:
        R.set_variant(v0)
    check_finishing_places(name, o)
    assert int(o.geom.valid.sum()) == n
    gi, gf = T._masked(gi, o), T._masked(gf, o)
    (o.image * gi.double()).sum().add((o.feats * gf.double()).sum()).backward()
    for tag, (out, leaves) in runs.items():
        torch.autograd.backward([out[0], out[2]], [gi.cuda(), gf.cuda()])
    return runs, o, ol


@pytest.mark.parametrize("name", list(CASES))
def test_maps_and_gradients_against_the_oracle(name):
    from tests import test_gpu_parity as T
    runs, o, ol = run_case(name)
    out, leaves = runs["mfma"]
    T._check_maps(out, o)
    T._check_grads(leaves, ol, o, NAMES)


@pytest.mark.parametrize("name", list(CASES))
def test_default_forward_against_packed_fp32_forward(name):
    runs, _, _ = run_case(name)
    (a_out, a_leaves), (b_out, b_leaves) = runs["mfma"], runs["valu"]
    assert torch.equal(a_out[1], b_out[1])
    pairs = [("image", a_out[0], b_out[0]), ("feats", a_out[2], b_out[2]), ("depth", a_out[3], b_out[3])]
    pairs += [(k, a_leaves[k].grad, b_leaves[k].grad) for k in NAMES]
    worst = []
    for k, a, b in pairs:
        scale, d = float(b.detach().abs().max()), float((a.detach() - b.detach()).abs().max())
        print(f"{name} {k}: max abs diff {d:.3e}, scale {scale:.3e}, ratio {d / max(scale, 1e-30):.3e}")
        if not d <= 2e-5 * max(scale, 1e-12) + 1e-9:
            worst.append((k, d, scale))
    assert not worst, worst


@pytest.mark.parametrize("name", list(CASES))
def test_two_runs_are_bit_identical(name):
    runs, _, _ = run_case(name)
    (a_out, a_leaves), (b_out, b_leaves) = runs["mfma"], runs["mfma2"]
    for a, b in zip(a_out, b_out):
        assert torch.equal(a, b)
    for k in NAMES:
        assert torch.equal(a_leaves[k].grad, b_leaves[k].grad), k
