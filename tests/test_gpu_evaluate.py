"""render_segment, the evaluate kernel and FrameScores on the GPU against the float64 oracle, the two-pass composition of
render.py:344-360 run through this repository's render(), and the numpy restatement (tests/evaluate_reference.py).

Scenes: tests.util.small_case at 96 x 64 (400 Gaussians, seed 0), 80 x 48 (600, seed 3) and 67 x 35 (400, seed 0: plane size
and row length no multiples of 4, so every access is scalar), selection ``means3D[:, 0] < -0.4``.  Mask comparisons leave
out the pixels whose oracle alpha lies within 1e-3 of the threshold (at most 0.5 % of the image).  The oracle of a scene is
computed once per module and only read.

Each comparison prints its figure before it asserts."""
import numpy as np
import pytest
import torch

from tests import evaluate_reference as er

pytestmark = pytest.mark.gpu

SCENES = {"96x64": dict(n=400, w=96, h=64, seed=0), "80x48": dict(n=600, w=80, h=48, seed=3), "67x35": dict(n=400, w=67, h=35, seed=0)}
BAND = 1e-3


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def cases(dev):
    """name -> dict(pc, cam, pipe, sel (device bool), oracle of the selected subset, seeded ground truths)."""
    from oracle import raster_oracle as ro
    from tests.util import settings_for, small_case
    from trase_amd.synthetic import SynthGaussianModel, SynthPipe, make_scene
    out = {}
    for name, c in SCENES.items():
        act, cam = small_case(**c)
        scene = make_scene(c["n"], feat_dim=32, seed=c["seed"], scale_mult=0.9)         # the raw parameters small_case activates
        assert all(torch.equal(v, act[k]) for k, v in scene.activated().items())
        sel = act["means3D"][:, 0] < -0.4
        o = ro.rasterize(settings_for(cam), act["means3D"][sel], None, shs=act["shs"][sel], sh_objs=act["sh_objs"][sel],
                         opacities=act["opacities"][sel], scales=act["scales"][sel], rotations=act["rotations"][sel])
        alpha = (1.0 - o.final_T).numpy()
        clear = np.abs(alpha - 0.5) >= BAND
        assert (~clear).mean() <= 0.005, name
        mask = alpha >= 0.5
        g = np.random.default_rng(c["seed"] + 100)
        gt_mask = mask.copy()
        gt_mask[c["h"] // 4:c["h"] // 4 + 17, c["w"] // 3:c["w"] // 3 + 23] ^= True               # a block flipped
        gt_mask = np.roll(gt_mask, (2, -3), (0, 1))                                             # and shifted
        obj = np.where(mask[None], o.image.numpy(), 0.0)
        gt_obj = er.save8b(np.clip(obj + g.normal(0.0, 0.03, obj.shape), 0.0, 1.0).astype(np.float32))
        out[name] = dict(pc=SynthGaussianModel(scene.to(dev), requires_grad=False), cam=cam.to(dev), pipe=SynthPipe(),
                         sel=sel.to(dev), o=o, alpha=alpha, clear=clear, mask=mask, gt_mask=gt_mask, gt_obj=gt_obj,
                         frac=float(mask.mean()))
    return out


def _segment(c, dev, **kw):
    from trase_amd.evaluate import render_segment
    bg = torch.tensor([0.1, 0.2, 0.3] if not kw.get("white_background") else [1.0, 1.0, 1.0], device=dev)
    return render_segment(c["cam"], c["pc"], c["pipe"], bg, 0.0, 0.0, 0.0, mask=c["sel"], **kw)


def _render(c, dev, bg=(0.1, 0.2, 0.3), **kw):
    from trase_amd.renderer import render
    with torch.no_grad():
        return render(c["cam"], c["pc"], c["pipe"], torch.tensor(bg, device=dev), 0.0, 0.0, 0.0, mask=c["sel"], **kw)


def test_scenes_are_the_ones_the_masks_were_sized_on(cases):
    assert abs(cases["96x64"]["frac"] - 0.62) < 0.01 and abs(cases["80x48"]["frac"] - 0.60) < 0.01
    assert int((~cases["96x64"]["clear"]).sum()) == 1 and int((~cases["80x48"]["clear"]).sum()) == 1


@pytest.mark.parametrize("name", sorted(SCENES))
@pytest.mark.parametrize("white", [False, True])
def test_outputs_against_the_oracle_and_the_two_pass_composition(cases, dev, name, white):
    from tests.test_gpu_parity import MAP_ATOL              # the bar of a scene's image map against the oracle
    c = cases[name]
    out = _segment(c, dev, white_background=white, frames_u8=True)
    H, W = c["alpha"].shape
    assert out["object"].shape == (3, H, W) and out["pred_mask"].dtype == torch.bool and out["object_u8"].shape == (H, W, 3)
    alpha = out["alpha"].cpu().numpy()
    ok = ~c["o"].fragile.numpy()
    err = np.abs(alpha.astype(np.float64) - c["alpha"])[ok].max()
    print(f"{name}: alpha vs the oracle's 1 - final_T: max abs error {err:.3e} on {int(ok.sum())} of {ok.size} pixels")
    assert err < MAP_ATOL
    # the mask: the oracle's, and the reference's two statements over an all-ones render on black, outside the band
    pred = out["pred_mask"].cpu().numpy()
    buf = _render(c, dev, bg=(0.0, 0.0, 0.0), override_color=torch.ones(c["sel"].numel(), 3, device=dev))["render"].clone()
    buf[buf < 0.5] = 0
    buf[buf != 0] = 1
    inlier = buf.mean(axis=0).bool().cpu().numpy()
    clear = c["clear"]
    assert np.array_equal(pred[clear], c["mask"][clear]) and np.array_equal(pred[clear], inlier[clear])
    assert np.array_equal(pred, alpha >= np.float32(0.5))
    # the cut-out: the bits of render(mask=) inside, exactly the background value outside
    bg = (1.0, 1.0, 1.0) if white else (0.1, 0.2, 0.3)
    img = _render(c, dev, bg=bg)["render"].cpu().numpy()
    obj = out["object"].cpu().numpy()
    assert np.array_equal(obj[:, pred].view(np.uint32), img[:, pred].view(np.uint32))
    assert (obj[:, ~pred] == (1.0 if white else 0.0)).all() and (~pred).any() and pred.any()
    # the 8-bit frames: to8b of the read-back fp32 outputs
    assert np.array_equal(out["object_u8"].cpu().numpy(), np.ascontiguousarray(er.to8b(obj).transpose(1, 2, 0)))
    assert np.array_equal(out["pred_mask_u8"].cpu().numpy(), np.repeat((pred * np.uint8(255))[:, :, None], 3, axis=2))


def _gt_variants(c, dev):
    """The same object image as (H,W,3) uint8, (3,H,W) uint8 and (3,H,W) fp32 (byte / 255: quantises back to the byte)."""
    g = c["gt_obj"]
    return [torch.from_numpy(np.ascontiguousarray(g.transpose(1, 2, 0))).to(dev), torch.from_numpy(g).to(dev),
            torch.from_numpy(g.astype(np.float32) / np.float32(255)).to(dev)]


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scores_three_frames_in_their_slots(cases, dev, name):
    from trase_amd.evaluate import FrameScores
    from trase_amd.losses import ssim
    c = cases[name]
    fs = FrameScores(4, device=dev)
    gts = _gt_variants(c, dev)
    gm = [torch.from_numpy(c["gt_mask"]).to(dev), torch.from_numpy(c["gt_mask"].astype(np.uint8) * 7).to(dev),
          torch.from_numpy(np.roll(c["gt_mask"], 5, 1)).to(dev)]
    outs = {}
    for k, slot in enumerate((2, 0, 1)):
        outs[slot] = (_segment(c, dev, scores=fs, frame=slot, gt_mask=gm[k], gt_object=gts[k]), gm[k], gts[k])
    records = fs.records.cpu().numpy()
    r = fs.result()                                             # one read-back for the three frames
    assert r["IOU"][3] is None and r["PSNR_frames"][3] is None and not records[3].any()
    for slot, (out, gmask, gobj) in outs.items():
        obj, pred = out["object"].cpu().numpy(), out["pred_mask"].cpu().numpy()
        g = gobj.cpu().numpy()
        rec, _ = er.frame_record(pred_mask=pred, gt_mask=gmask.cpu().numpy(), obj=obj, gt_object=g)
        assert np.array_equal(records[slot, :6], rec[:6]), (slot, records[slot], rec)
        iou, acc, psnr = er.scores(rec)
        for got, want in ((r["IOU"][slot], iou), (r["ACC"][slot], acc), (r["PSNR_frames"][slot], psnr)):
            assert abs(got - want) <= 1e-12 * abs(want), (slot, got, want)
        print(f"{name} slot {slot}: IoU {iou:.4f} ACC {acc:.4f} PSNR {psnr:.3f} dB")
        assert 0.0 < iou < 1.0 and 0.0 < psnr < 100.0
        po, pg = er.compared_pair(obj, c["gt_obj"])
        direct = float(ssim(torch.from_numpy(po).to(dev), torch.from_numpy(pg).to(dev)))
        assert r["SSIM_frames"][slot] == direct and 0.0 < direct < 1.0, (slot, r["SSIM_frames"][slot], direct)
    assert r["mIOU"] == float(np.mean([r["IOU"][s] for s in range(3)])) and r["SSIM"] == float(np.mean(r["SSIM_frames"][:3]))


def test_empty_selection(cases, dev):
    from trase_amd.evaluate import FrameScores
    c = dict(cases["96x64"])
    c["sel"] = torch.zeros_like(c["sel"])
    fs = FrameScores(1, device=dev)
    H, W = c["alpha"].shape
    out = _segment(c, dev, scores=fs, frame=0, gt_mask=torch.zeros(H, W, dtype=torch.bool, device=dev))
    assert not out["pred_mask"].any() and float(out["alpha"].abs().max()) == 0.0 and float(out["object"].abs().max()) == 0.0
    r = fs.result()
    assert r["IOU"] == [0.0] and r["ACC"] == [1.0] and r["PSNR"] is None
    assert fs.records.cpu().tolist()[0][:4] == [0, 0, H * W, H * W]


def _synthetic(H, W, seed, dev, all_inside=False):
    g = np.random.default_rng(seed)
    image = g.uniform(-0.1, 1.1, (3, H, W)).astype(np.float32)
    T = np.zeros((H, W), dtype=np.float32) if all_inside else g.uniform(0.0, 1.0, (H, W)).astype(np.float32)
    T[g.random((H, W)) < 0.01] = 0.5                         # alpha exactly at the threshold: inside
    image[:, 3 % H, 5 % W] = np.nan                          # a NaN colour, and a NaN transmittance
    T[7 % H, 11 % W] = np.nan
    gt_mask = g.random((H, W)) < 0.5
    gt_obj = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return image, T, gt_mask, gt_obj


@pytest.mark.parametrize("shape,all_inside", [((1080, 1920), False), ((1080, 1920), True), ((1000, 2304), False),
                                              ((34, 66), False), ((35, 67), False), ((1, 3), False)])
def test_kernel_alone_counts_are_exact(dev, shape, all_inside):
    """1920 x 1080: the headline size; 2304 x 1000: more quads than one sweep of the capped grid; 66 x 34: rows alternate
    between the 16-byte and the scalar path, with a 2-pixel tail; 67 x 35: all scalar; 3 x 1: less than one quad."""
    from trase_amd.evaluate import FrameScores, segment_frame
    H, W = shape
    image, T, gt_mask, gt_obj = _synthetic(H, W, 7, dev, all_inside)
    fs, fu = FrameScores(2, device=dev, ssim=False), FrameScores(2, device=dev, quantize=False, ssim=False)
    ti, tT, tm, tg = (torch.from_numpy(a).to(dev) for a in (image, T, gt_mask, gt_obj))
    out = segment_frame(ti, tT, frames_u8=True, scores=fs, frame=1, gt_mask=tm, gt_object=tg)
    segment_frame(ti, tT, scores=fu, frame=0, gt_mask=tm, gt_object=tg)
    want = er.segment_output(image, T)
    for k, v in want.items():
        got = out[k].cpu().numpy()
        assert got.dtype == v.dtype and np.array_equal(got, v, equal_nan=(v.dtype == np.float32)), k
    if all_inside:
        assert int(want["pred_mask"].sum()) == H * W - 1                 # all but the NaN transmittance
    rec, _ = er.frame_record(pred_mask=want["pred_mask"], gt_mask=gt_mask, obj=want["object"], gt_object=gt_obj)
    assert np.array_equal(fs.records.cpu().numpy()[1, :6], rec[:6]) and not fs.records[0].any()
    # the unquantised sum: float64 per workgroup, workgroups in order.  n non-negative terms: a sum in any order is within
    # (n - 1) 2^-53 (relative) of the exact one, so two orders agree to 2 n 2^-53
    finite = np.isfinite(want["object"])
    gt_f = (gt_obj.transpose(2, 0, 1).astype(np.float32) / np.float32(255)).astype(np.float64)       # to_tensor's fp32 division
    d = np.where(finite, want["object"].astype(np.float64) - gt_f, 0.0)
    got_parts = fu.buffer.cpu().numpy()[0, 8:].view(np.float64)
    if finite.all():
        sse = float(np.sum(d * d))
        print(f"{W}x{H}: unquantised squared error {float(np.sum(got_parts)):.17g} against numpy's {sse:.17g}")
        assert abs(float(np.sum(got_parts)) - sse) <= 2.0 * d.size * 2.0 ** -53 * sse
    else:
        assert np.isnan(got_parts).sum() == 1                            # the NaN colour poisons its workgroup's slot only
    assert np.array_equal(fu.records.cpu().numpy()[0, :4], rec[:4]) and fu.records.cpu().numpy()[0, 4] == 0


def test_stand_alone_entry_points(cases, dev):
    from trase_amd.evaluate import FrameScores, image_scores, segment_scores
    c = cases["67x35"]
    fs = FrameScores(2, device=dev)
    g = np.random.default_rng(5)
    pred = g.random(c["mask"].shape) < 0.4
    image = g.uniform(0, 1, (3,) + c["mask"].shape).astype(np.float32)
    segment_scores(torch.from_numpy(pred).to(dev), torch.from_numpy(c["gt_mask"]).to(dev), fs, 1)
    image_scores(torch.from_numpy(image).to(dev), torch.from_numpy(c["gt_obj"]).to(dev), fs, 1)
    rec, _ = er.frame_record(pred_mask=pred, gt_mask=c["gt_mask"], obj=image, gt_object=c["gt_obj"])
    assert np.array_equal(fs.records.cpu().numpy()[1, :6], rec[:6])
    r = fs.result()
    assert r["IOU"][0] is None and abs(r["PSNR_frames"][1] - er.scores(rec)[2]) <= 1e-12 * er.scores(rec)[2]
    assert 0.0 < r["SSIM_frames"][1] < 1.0


def test_two_identical_calls_are_bitwise_identical(cases, dev):
    from trase_amd.evaluate import FrameScores
    c = cases["80x48"]
    runs = []
    for _ in range(2):
        fs, fu = FrameScores(1, device=dev), FrameScores(1, device=dev, quantize=False)
        gm, go = torch.from_numpy(c["gt_mask"]).to(dev), _gt_variants(c, dev)[2]
        out = _segment(c, dev, frames_u8=True, scores=fs, frame=0, gt_mask=gm, gt_object=go)
        _segment(c, dev, scores=fu, frame=0, gt_mask=gm, gt_object=go)
        runs.append([out[k].cpu().numpy().copy() for k in sorted(out)] + [fs.buffer.cpu().numpy(), fu.buffer.cpu().numpy()])
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()
    assert runs[0][-1][0, 8:].view(np.float64).sum() > 0


def test_render_under_no_grad_is_undisturbed(cases, dev):
    c = cases["96x64"]
    before = _render(c, dev)
    _segment(c, dev, frames_u8=True)
    after = _render(c, dev)
    for k in ("render", "render_gaussian_features", "depth", "radii"):
        assert torch.equal(before[k], after[k]), k
    assert before["radii"].shape[0] == int(c["sel"].sum())
