"""The scores of trase_amd.evaluate against the imported reference's own functions (tests/golden/evaluate.npz, written by
tests/golden/make_evaluate.py from metrics_segmentation.py's compute_iou / compute_acc and utils/image_utils.psnr), and the
two 8-bit quantisers of the numpy restatement against numpy / torch evaluating the reference's expressions.  No GPU."""
import math
import os

import numpy as np
import pytest
import torch

import trase_amd.evaluate as ev
from tests import evaluate_reference as er

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "evaluate.npz"))
N_MASKS, N_IMAGES = len(G["iou"]), len(G["psnr"])
# psnr_f32 is the reference's fp32 evaluation: the squared differences and their mean carry a few fp32 roundings (relative
# 2^-24 each; 20 / ln 10 = 8.7 dB per unit of relative error of the mse's root) and the result is rounded to fp32 near
# 48 dB (half an ulp: 1.9e-6)
PSNR_F32_TOL = 1e-5


def _same_psnr(got, want, tol):
    return (math.isinf(want) and got == want) or abs(got - want) <= tol


def test_fixture_holds_the_edge_cases():
    assert not G["pred"][1].any() and G["gt"][1].any()                              # an empty prediction
    assert not (G["pred"][2] | G["gt"][2]).any() and G["iou"][2] == 0.0             # an empty union -> IoU 0
    assert np.array_equal(G["image"][1], G["image_gt"][1]) and np.isinf(G["psnr"][1])
    assert np.array_equal(G["image"][2].astype(int) + 1, G["image_gt"][2].astype(int))


def test_restatement_reproduces_the_reference_scores():
    for i in range(N_MASKS):
        rec, _ = er.frame_record(pred_mask=G["pred"][i], gt_mask=G["gt"][i])
        iou, acc, _ = er.scores(rec)
        assert iou == G["iou"][i] and acc == G["acc"][i], i
    for i in range(N_IMAGES):
        rec, _ = er.frame_record(obj=G["image"][i].astype(np.float32) / np.float32(255), gt_object=G["image_gt"][i])
        assert _same_psnr(er.scores(rec)[2], float(G["psnr"][i]), 1e-6), i
        assert _same_psnr(er.scores(rec)[2], float(G["psnr_f32"][i]), PSNR_F32_TOL), i


def test_frame_scores_result_from_host_built_records():
    n = max(N_MASKS, N_IMAGES)
    fs = ev.FrameScores(n, device="cpu")
    for i in range(N_MASKS):
        fs.records[i] += torch.from_numpy(er.frame_record(pred_mask=G["pred"][i], gt_mask=G["gt"][i])[0])
    for i in range(N_IMAGES):
        rec, _ = er.frame_record(obj=G["image"][i].astype(np.float32) / np.float32(255), gt_object=G["image_gt"][i].transpose(1, 2, 0))
        fs.records[i] += torch.from_numpy(rec)
    r = fs.result()
    assert r["IOU"] == G["iou"].tolist() and r["ACC"] == G["acc"].tolist()           # exactly
    for i in range(N_IMAGES):
        assert _same_psnr(r["PSNR_frames"][i], float(G["psnr"][i]), 1e-6), i
    assert r["PSNR_frames"][N_IMAGES:] == [None] * (n - N_IMAGES)
    assert r["mIOU"] == float(np.mean(G["iou"])) and r["mACC"] == float(np.mean(G["acc"]))
    assert math.isinf(r["PSNR"])                                                     # a mean over an identical pair, as torch's


def test_unquantised_records_and_empty_slots():
    fs = ev.FrameScores(3, device="cpu", quantize=False, ssim=False)
    a = G["image"][3].astype(np.float32) / np.float32(255)
    rec, sse = er.frame_record(obj=a, gt_object=G["image_gt"][3], quantize=False)
    fs.records[1] += torch.from_numpy(rec)
    fs.buffer[1, ev.RECORD_WORDS:ev.RECORD_WORDS + 2] = torch.tensor([0.75 * sse, 0.25 * sse], dtype=torch.float64).view(torch.int64)
    r = fs.result()
    assert r["IOU"] == [None] * 3 and r["mIOU"] is None and r["SSIM"] is None
    assert r["PSNR_frames"][0] is None and abs(r["PSNR_frames"][1] - float(G["psnr"][3])) <= 1e-6


def _grid():
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    one = np.float32(1.0)
    parts = [k, np.nextafter(k, np.float32(2.0)), np.nextafter(k, np.float32(-2.0)),
             (np.arange(256, dtype=np.float32) + np.float32(0.5)) / np.float32(255),
             np.array([0.0, -0.0, 1.0, -0.25, 1.5, 7.0, -3.0, 0.5, 1e-8, np.nextafter(one, np.float32(2.0)), 254.5 / 255, 0.002], dtype=np.float32)]
    return np.concatenate(parts).astype(np.float32)


def test_quantisers_are_bit_equal_to_the_reference_expressions():
    x = _grid()
    assert (x == 0).any() and (x == 1).any() and (x < 0).any() and (x > 1).any()
    assert np.array_equal(er.to8b(x), (255 * np.clip(x, 0, 1)).astype(np.uint8))                       # render.py:106
    t = torch.from_numpy(x.copy())
    assert np.array_equal(er.save8b(x), t.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).numpy())   # torchvision save_image
    assert er.to8b(np.float32(np.nan)) == 0 and er.save8b(np.float32(np.nan)) == 0
    # the two rules differ: to8b truncates, save_image rounds
    assert er.to8b(np.float32(0.002)) == 0 and er.save8b(np.float32(0.002)) == 1


def test_cpu_tensors_are_refused():
    fs = ev.FrameScores(1, device="cpu")
    with pytest.raises(RuntimeError, match="GPU only"):
        ev.segment_scores(torch.zeros(4, 4, dtype=torch.bool), torch.zeros(4, 4, dtype=torch.bool), fs, 0)
    with pytest.raises(RuntimeError, match="GPU only"):
        ev.image_scores(torch.zeros(3, 4, 4), torch.zeros(3, 4, 4), fs, 0)
