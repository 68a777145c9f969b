"""CPU references for LPIPS with the VGG16 backbone (trase_amd/lpips.py, csrc/vgg.hip); torch on the CPU, no GPU.  The 8-layer
pieces come from tests/vgg_reference.py; this file extends them to the 13 convolutions up to relu5_3 and adds the head.

* ``forward_f64``: what the reference computes (lpipsPyTorch/modules/{lpips,networks,utils}.py), in float64:
  ``z = (x - mean) / std``, VGG16 ``features`` to module 30, the taps relu1_2 relu2_2 relu3_3 relu4_3 relu5_3 (before the pool
  that follows), ``t / (sqrt(sum_c t^2) + 1e-10)``, per pixel ``sum_c lin_c (a_c - b_c)^2``, spatial mean, sum over the five.
* ``forward_emulated``: the device's arithmetic -- the fp32 normalisation ``(x - mean) * (1 / std)``, conv1_1 as its fp32 chain,
  every later layer on split operands with float64 sums rounded to fp32 once (``products=3``; ``products=1``: the one-product
  bf16 variant), the taps as ``hi + lo`` (``products=1``: ``hi``), the head in float64 rounded to fp32 once per pixel
  (``head_device``), the layer mean in float64.
* ``lattice_taps``: the int64 statement of the five taps for integer data, with the two premises of an exact fp32 device result
  asserted on the data: split operands below 2^16 and sum |w| max|a| below 2^24.

The head's error bound (``head_bound``).  The device forms, per pixel and in float64 (u = 2^-53), na = sum a_c^2, ra = 1 / (sqrt(na)
+ 1e-10), p_c = a_c ra (likewise q_c), d = sum_c lin_c (p_c - q_c)^2, and rounds d to fp32 once.  p_c and q_c are at most 1 and
carry a relative error of a few u each (sum, root, reciprocal, product), so p_c - q_c is off by at most 8 u absolutely and its
square by at most 16 u |p_c - q_c| + 64 u^2; with L = sum lin_c and Cauchy-Schwarz the weighted sum is off by at most
16 u sqrt(L d) + 64 u^2 L, plus (C + 3) u d for its own C roundings.  A float64 reference of another order carries as much, hence
the factor 2; the one fp32 rounding adds 2^-24 d (2^-149 where d is subnormal):
    |map - d| <= 2^-24 d + 2 (16 u sqrt(L d) + 64 u^2 L + (C + 3) u d) + 2^-149.
The layer mean of n fp32 map values: 256 chunks of 256 ceil(n / 65536) elements; in a chunk thread t sums elements t, t + 256, ..
(ceil(n / 65536) terms) and a tree of 8 levels joins the 256 threads; another tree of 8 levels joins the 256 chunks; one division:
relative error at most (ceil(n / 65536) + 17) u (``mean_bound``), the terms being non-negative."""
import functools
import math

import torch

from tests import vgg_reference as R

KEYS = R.KEYS + ("conv4_2", "conv4_3", "conv5_1", "conv5_2", "conv5_3")
CHANNELS = R.CHANNELS + (512,) * 5
POOL_AFTER = R.POOL_AFTER + (10,)
TAP_LAYERS = (2, 4, 7, 10, 13)
TAP_CHANNELS = (64, 128, 256, 512, 512)
FEATURE_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
MEAN = (-.030, -.088, -.188)
STD = (.458, .448, .450)
EPS = 1e-10
U64 = 2.0 ** -53


def _advance(z, l):
    a = torch.relu(z)
    if l in POOL_AFTER:
        a, _ = R.pool_decide(a)
    return a


def normalise_reference(img):
    """z_score of networks.py in float64: the buffers are fp32 tensors, the division is a division"""
    m = torch.tensor(MEAN, dtype=torch.float32).double().view(3, 1, 1)
    s = torch.tensor(STD, dtype=torch.float32).double().view(3, 1, 1)
    return (img.double() - m) / s


def taps_f64(pairs, img):
    """the five taps (C, h, w) of one image in float64"""
    x = normalise_reference(img)
    taps = []
    for l, (w, b) in enumerate(pairs, start=1):
        z = R._conv(x, w.double(), b.double())
        if l in TAP_LAYERS:
            taps.append(torch.relu(z))
        x = _advance(z, l)
    return taps


def head_f64(a, b, lin):
    """(C, h, w) float64 taps -> the (h, w) float64 map, as the reference states it"""
    a, b = a.double(), b.double()
    pa = a / (torch.sqrt((a * a).sum(0, keepdim=True)) + EPS)
    pb = b / (torch.sqrt((b * b).sum(0, keepdim=True)) + EPS)
    return (lin.double().view(-1, 1, 1) * (pa - pb) ** 2).sum(0)


def head_device(a, b, lin):
    """the device's head on fp32 taps: float64 with the reciprocal multiplied, rounded to fp32 once per pixel"""
    a, b = a.float().double(), b.float().double()
    ra = 1.0 / (torch.sqrt((a * a).sum(0, keepdim=True)) + EPS)
    rb = 1.0 / (torch.sqrt((b * b).sum(0, keepdim=True)) + EPS)
    return (lin.float().double().view(-1, 1, 1) * (a * ra - b * rb) ** 2).sum(0).float()


def head_bound(d, lin):
    """the bound of the module docstring on |map - d| per pixel, d the float64 map"""
    L, C = float(lin.double().sum()), lin.numel()
    d = d.double()
    return 2.0 ** -24 * d + 2.0 * (16 * U64 * torch.sqrt(L * d) + 64 * U64 * U64 * L + (C + 3) * U64 * d) + 2.0 ** -149


def mean_bound(n):
    """relative error of the device's float64 mean of n non-negative fp32 values"""
    return (math.ceil(n / 65536) + 17) * U64


def _result(taps_x, taps_y, maps):
    layers = torch.stack([m.double().mean() for m in maps])
    total = layers[0]
    for v in layers[1:]:
        total = total + v
    return {"taps_x": taps_x, "taps_y": taps_y, "maps": maps, "layers": layers, "total": total}


def forward_f64(pairs, lins, x, y):
    tx, ty = taps_f64(pairs, x), taps_f64(pairs, y)
    return _result(tx, ty, [head_f64(a, b, lin) for a, b, lin in zip(tx, ty, lins)])


def taps_emulated(pairs, img, products=3):
    """the five taps the device's head reads, as fp32"""
    x = R.normalise_fp32(img, MEAN, STD)
    taps = []
    for l, (w, b) in enumerate(pairs, start=1):
        w = w.float()
        if l == 1:
            z = R.conv1_fp32_chain(x, w, b.float())
        else:
            a_hi, a_lo = R.split(x)
            w_hi, w_lo = R.split(w)
            if products == 3:
                z = R._conv(a_hi.double(), w_hi.double() + w_lo.double(), b.double()) + R._conv(a_lo.double(), w_hi.double())
            else:
                z = R._conv(a_hi.double(), w_hi.double(), b.double())
        z = z.float()
        if l in TAP_LAYERS:
            hi, lo = R.split(torch.relu(z))
            taps.append(hi + lo if products == 3 else hi)
        x = _advance(z, l)
    return taps


def forward_emulated(pairs, lins, x, y, products=3):
    tx, ty = taps_emulated(pairs, x, products), taps_emulated(pairs, y, products)
    return _result(tx, ty, [head_device(a, b, lin) for a, b, lin in zip(tx, ty, lins)])


def map_err(m, ref):
    """max|m - ref| / max|ref|: the measure of every bar"""
    return float((m.double() - ref.double()).abs().max() / ref.double().abs().max())


# ---- lattice data ----------------------------------------------------------------------------------------------------------
def lattice_weights(seed, dense=()):
    """integer weights of the 13 layers: layers 1 .. 8 are vgg_reference.lattice_weights'; a sparse layer of 9 .. 13 has ONE
    weight of +1 per output channel (input channel and tap scattered with the output channel) and so cannot grow the stack's
    magnitudes; a dense layer draws every weight from {-1, 0, 1}, three in four of them 0.  Biases from {-1, 0, 1}."""
    pairs = R.lattice_weights(seed, 8, dense=tuple(l for l in dense if l <= 8))
    g = torch.Generator().manual_seed(int(seed) + 13)
    for l in range(9, 14):
        cin = cout = 512
        if l in dense:
            w = torch.randint(-1, 2, (cout, cin, 3, 3), generator=g).float() * (torch.randint(0, 4, (cout, cin, 3, 3), generator=g) == 0)
        else:
            w = torch.zeros(cout, cin, 3, 3)
            co = torch.arange(cout)
            ci = (co * 5 + 3 + l) % cin
            tap = (co + co // 9 + l) % 9
            w[co, ci, tap // 3, tap % 3] = 1.0
        b = torch.randint(-1, 2, (cout,), generator=g).float()
        pairs.append((w, b))
    return pairs


def lattice_taps(pairs, img):
    """int64 taps of integer data, premises asserted: every split activation below 2^16, every weight a small integer (its lo
    part is 0), every output's sum |w| max|a| below 2^24"""
    x = R._exact_int(img.double(), "image")
    taps = []
    for l, (w, b) in enumerate(pairs, start=1):
        wi, bi = R._exact_int(w.double(), "weights"), R._exact_int(b.double(), "bias")
        assert int(wi.abs().max()) <= 128, "weights must be small integers: their bf16 lo part is 0"
        amax = int(x.abs().max())
        if l > 1:
            assert amax < 2 ** 16, f"layer {l}: a split activation of magnitude {amax} >= 2^16"
        bound = int(wi.abs().sum(dim=(1, 2, 3)).max()) * amax + int(bi.abs().max())
        assert bound < 2 ** 24, f"layer {l}: sum |w| max|a| = {bound} >= 2^24"
        z = R._exact_int(R._conv(x.double(), wi.double(), bi.double()), f"z_{l}")
        if l in TAP_LAYERS:
            t = torch.relu(z)
            assert int(t.max()) < 2 ** 16, f"tap of layer {l}: a value >= 2^16 is not hi + lo exactly"
            taps.append(t)
        x = _advance(z, l)
    return taps


LATTICE_DENSE = {(16, 16): (9, 12), (17, 31): (10, 13), (32, 48): (9, 11), (67, 35): (10, 12), (33, 65): (11, 13),
                 (240, 272): (11,), (272, 256): (12,)}       # one dense layer: a second takes these sizes' maxima past 2^16


@functools.lru_cache(maxsize=None)
def lattice_case(H, W):
    """(weights, image x, image y, int64 taps of x, of y) of the exact tests; two of layers 9 .. 13 dense per size"""
    pairs = lattice_weights(500 + H, dense=LATTICE_DENSE[(H, W)])
    x, y = R.lattice_image(600 + H * 1000 + W, H, W), R.lattice_image(700 + H * 1000 + W, H, W)
    return pairs, x, y, lattice_taps(pairs, x), lattice_taps(pairs, y)


# ---- real-valued cases -----------------------------------------------------------------------------------------------------
def weights(seed):
    from trase_amd.lpips import lpips_random_weights
    return lpips_random_weights(seed)


def image_pair(kind, H, W, seed):
    """[0, 1] image pairs: 'independent'; 'quantised' (an image and floor(255 x + 0.5) / 255 of it); 'patch' (a copy with one
    16 x 16 patch redrawn)"""
    g = torch.Generator().manual_seed(int(seed))
    x = torch.rand(3, H, W, generator=g)
    if kind == "independent":
        return x, torch.rand(3, H, W, generator=g)
    if kind == "quantised":
        return x, torch.floor(255.0 * x + 0.5) / 255.0
    assert kind == "patch"
    y = x.clone()
    y[:, H // 2 - 8:H // 2 + 8, W // 2 - 8:W // 2 + 8] = torch.rand(3, 16, 16, generator=g)
    return x, y


CASE_SEED = 20                    # the fixture's seed: one weight set for every real-valued test


def total_bar(emu, f64):
    """sum_l mean_p |map_emulated - map_f64|: the emulation's error of the total without cancellation between pixels (a scalar's
    own error can be small by accident)"""
    return sum(float((a.double() - b.double()).abs().mean()) for a, b in zip(emu["maps"], f64["maps"]))


@functools.lru_cache(maxsize=None)
def _case_weights():
    return weights(CASE_SEED)


@functools.lru_cache(maxsize=None)
def real_case(kind, H, W):
    """{"x", "y", "f64", "emu3", "emu1"} of a seeded [0, 1] pair; computed once and shared, never modified"""
    pairs, lins = _case_weights()
    x, y = image_pair(kind, H, W, seed=H * 1000 + W)
    return {"x": x, "y": y, "f64": forward_f64(pairs, lins, x, y), "emu3": forward_emulated(pairs, lins, x, y, 3),
            "emu1": forward_emulated(pairs, lins, x, y, 1)}


def checksums(pairs, lins):
    """per weight tensor (float64 sum, float64 sum of squares): names a drifting generator as that"""
    out = []
    for w, b in pairs:
        out += [[float(w.double().sum()), float((w.double() ** 2).sum())], [float(b.double().sum()), float((b.double() ** 2).sum())]]
    for v in lins:
        out.append([float(v.double().sum()), float((v.double() ** 2).sum())])
    return torch.tensor(out, dtype=torch.float64)
