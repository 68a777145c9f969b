"""CPU references for the VGG16 feature extractor (trase_amd/vgg.py, csrc/vgg.hip); torch on the CPU, no GPU.

* ``forward_f64`` / ``backward_f64``: the network in float64.  The backward takes the DECISIONS (ReLU bits, pool choices) as
  inputs, so a device gradient can be compared under the device's own decisions.
* ``forward_emulated`` / ``backward_emulated``: the kernels' split arithmetic -- every matrix operand as hi = bf16(v),
  lo = bf16(v - hi); per layer the three partial convolutions hi.hi + hi.lo + lo.hi summed in float64 and rounded to fp32 once
  (``products=3``), or the one-product bf16 variant hi.hi (``products=1``) for comparison.  conv1_1 and its image gradient are
  fp32 on the device: conv1_1 is emulated as its chain of fp32 fused multiply-adds, the image gradient as a float64 sum.
* ``lattice_forward`` / ``lattice_backward``: the int64 statement for integer data.  Integer images, integer weights and
  integer cotangents have one right answer whatever the summation order as long as every partial sum stays below 2^24 (fp32)
  and every split operand below 2^16 (hi + lo exact); both premises are ASSERTED here, in int64, on the data at hand.

Layers are 1-based: layer l is the l-th convolution (conv1_1 .. conv4_1).  Decisions: ``{l: ("relu", bits)}`` with bits
(C, H, W) bool, or ``{l: ("pool", idx, pos)}`` with idx (C, H/2, W/2) in 0..3 -- the window position in ATen's scan order
(row, column; update on strict >) -- and pos = the pooled maximum is positive."""
import functools

import torch
import torch.nn.functional as F

KEYS = ("conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3", "conv4_1")
CHANNELS = (3, 64, 64, 128, 128, 256, 256, 256, 512)
POOL_AFTER = (2, 4, 7)
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)

# the MFMA kernel's tile constants (csrc/vgg.hip): a workgroup owns VG_TILE x VG_TILE pixels and VG_NB output channels; a
# wave owns 4 rows of the tile as two groups of 2 rows x 16 columns
VG_TILE = 16
VG_NB = 64


def split(v):
    """fp32 tensor -> (hi, lo) as fp32 tensors holding bf16 values, both rounded to nearest even"""
    v = v.float()
    hi = v.bfloat16().float()
    lo = (v - hi).bfloat16().float()
    return hi, lo


def normalise_fp32(img, mean=MEAN, std=STD):
    """what conv1_1 reads: (x - mean) * (1 / std), every step rounded to fp32"""
    m = torch.tensor(mean, dtype=torch.float32).view(3, 1, 1)
    inv = (1.0 / torch.tensor(std, dtype=torch.float32)).view(3, 1, 1)
    return (img.float() - m) * inv


def inv_std_fp32(std=STD):
    return (1.0 / torch.tensor(std, dtype=torch.float32)).view(3, 1, 1)


def pool_decide(a):
    """2x2 floor pool of (C, H, W) by ATen's rule: scan (row, column), update on strict >.  -> (max, idx)"""
    C, H, W = a.shape
    h, w = H // 2, W // 2
    win = [a[:, dy:2 * h:2, dx:2 * w:2] for dy in (0, 1) for dx in (0, 1)]
    best = win[0].clone()
    idx = torch.zeros(C, h, w, dtype=torch.int64)
    for i in (1, 2, 3):
        upd = win[i] > best
        best = torch.where(upd, win[i], best)
        idx = torch.where(upd, torch.full_like(idx, i), idx)
    return best, idx


def unpool(g, idx, pos, H, W):
    """scatter the pooled cotangent (C, h, w) to (C, H, W): position idx of each window where pos, zeros elsewhere"""
    C, h, w = g.shape
    out = torch.zeros(C, H, W, dtype=g.dtype)
    for i in range(4):
        dy, dx = i // 2, i % 2
        out[:, dy:2 * h:2, dx:2 * w:2] = torch.where((idx == i) & pos, g, torch.zeros_like(g))
    return out


def decisions_from(zs):
    """decisions of layers 1 .. len(zs) out of their pre-ReLU outputs zs[l - 1] (C, H, W)"""
    dec = {}
    for l, z in enumerate(zs, start=1):
        if l in POOL_AFTER:
            best, idx = pool_decide(torch.relu(z))
            dec[l] = ("pool", idx, best > 0)
        else:
            dec[l] = ("relu", z > 0)
    return dec


def _conv(x, w, b=None):
    return F.conv2d(x.unsqueeze(0), w, b, padding=1)[0]


def _conv_t(g, w):
    return F.conv_transpose2d(g.unsqueeze(0), w, None, padding=1)[0]


def _advance(z, l):
    """the activation layer l + 1 reads, out of layer l's pre-ReLU output"""
    a = torch.relu(z)
    if l in POOL_AFTER:
        a, _ = pool_decide(a)
    return a


def forward_f64(pairs, img, normalize=True):
    """[z_1 .. z_k] in float64 (pre-ReLU outputs, (C, H, W)); the input is the fp32-normalised image the device reads"""
    x = (normalise_fp32(img) if normalize else img.float()).double()
    zs = []
    for l, (w, b) in enumerate(pairs, start=1):
        z = _conv(x, w.double(), b.double())
        zs.append(z)
        x = _advance(z, l)
    return zs


def forward_emulated(pairs, img, normalize=True, products=3):
    """[z_1 .. z_k] as fp32 values (held in fp32 tensors): the device's arithmetic with float64 sums, rounded once per layer"""
    x = normalise_fp32(img) if normalize else img.float()
    zs = []
    for l, (w, b) in enumerate(pairs, start=1):
        w = w.float()
        if l == 1:
            z = conv1_fp32_chain(x, w, b.float())
        else:
            a_hi, a_lo = split(x)
            w_hi, w_lo = split(w)
            if products == 3:      # hi.hi + hi.lo and lo.hi: w_hi + w_lo is exact in float64, so two convolutions state three
                z = _conv(a_hi.double(), w_hi.double() + w_lo.double(), b.double()) + _conv(a_lo.double(), w_hi.double())
            else:
                z = _conv(a_hi.double(), w_hi.double(), b.double())
        z = z.float()
        zs.append(z)
        x = _advance(z, l)
    return zs


def conv1_fp32_chain(x, w, b):
    """conv1_1 as the device evaluates it: one fp32 fused multiply-add per term, bias first, terms in (channel, row, column)
    order.  A product of two fp32 values is exact in float64; the sum is rounded to fp32 after every term."""
    _, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1)).double()
    z = b.view(-1, 1, 1).expand(-1, H, W).float()
    for ci in range(3):
        for ky in range(3):
            for kx in range(3):
                z = (z.double() + xp[ci, ky:ky + H, kx:kx + W][None] * w[:, ci, ky, kx].double().view(-1, 1, 1)).float()
    return z


def _mask(g, dec, H, W):
    if dec[0] == "pool":
        return unpool(g, dec[1], dec[2], H, W)
    return g * dec[1].to(g.dtype)


def backward_f64(pairs, cot, dec, normalize=True):
    """gradient to the image (3, H, W), float64, of <cot, z_k> under the given decisions of layers 1 .. k - 1"""
    g = cot.double()
    for l in range(len(pairs), 1, -1):
        ga = _conv_t(g, pairs[l - 1][0].double())
        H, W = dec["shape"][l - 1]
        g = _mask(ga, dec[l - 1], H, W)
    d_img = _conv_t(g, pairs[0][0].double())
    return d_img * inv_std_fp32().double() if normalize else d_img


def backward_emulated(pairs, cot, dec, normalize=True, products=3):
    """the device's backward: cotangents split before every MFMA convolution, float64 sums rounded to fp32 once per layer"""
    g = cot.float()
    for l in range(len(pairs), 1, -1):
        w = pairs[l - 1][0].float()
        g_hi, g_lo = split(g)
        w_hi, w_lo = split(w)
        if products == 3:
            ga = _conv_t(g_hi.double(), w_hi.double() + w_lo.double()) + _conv_t(g_lo.double(), w_hi.double())
        else:
            ga = _conv_t(g_hi.double(), w_hi.double())
        d = dec[l - 1]
        H, W = dec["shape"][l - 1]
        g = _mask(ga.float(), d, H, W)
    g_hi, g_lo = split(g)
    d_img = _conv_t(g_hi.double() + g_lo.double(), pairs[0][0].double())
    if normalize:
        d_img = d_img.float() * inv_std_fp32()
    return d_img.float()


def with_shapes(dec, H, W):
    """add the full-resolution shape of every layer's output to a decision dict (the unpool needs it where H or W is odd)"""
    dec = dict(dec)
    shapes = {}
    h, w = H, W
    for l in range(1, len(KEYS) + 1):
        shapes[l] = (h, w)
        if l in POOL_AFTER:
            h, w = h // 2, w // 2
    dec["shape"] = shapes
    return dec


def rel_err(a, ref):
    """max|a - ref| / max|ref|"""
    return float((a.double() - ref.double()).abs().max() / ref.double().abs().max())


def flip_shares(dec_a, dec_b):
    """(share of ReLU units whose bit differs, share of LIVE pooled units -- positive in either -- whose decision differs)"""
    relu_n = relu_d = pool_n = pool_d = 0
    for l, d in dec_a.items():
        if l == "shape" or l not in dec_b:
            continue
        e = dec_b[l]
        if d[0] == "relu":
            relu_n += d[1].numel()
            relu_d += int((d[1] != e[1]).sum())
        else:
            live = d[2] | e[2]
            pool_n += int(live.sum())
            pool_d += int((live & ((d[2] != e[2]) | (d[1] != e[1]))).sum())
    return relu_d / max(relu_n, 1), pool_d / max(pool_n, 1)


# ---- the size plan of the exact GPU tests ------------------------------------------------------------------------------------
IMAGE_SIZES = ((8, 8), (9, 15), (24, 40), (67, 35), (44, 52), (256, 320))                       # (H, W) of the image, every key
TILE_SIZES = ((VG_TILE - 1, VG_TILE + 1), (VG_TILE, VG_TILE), (VG_TILE + 1, VG_TILE - 1),   # one tile -1 / 0 / +1 pixels
              (2 * VG_TILE + 1, 2 * VG_TILE + 1))                                      # two tiles + 1


def pools_before(k):
    return sum(1 for p in POOL_AFTER if p < k)


def exact_sizes(k):
    """image sizes of the exact tests of the network cut at layer k: the common sizes, and the tile-edge sizes stated at the
    resolution layer k's convolution runs at (the image is 2^p times as large behind p pools)"""
    p = pools_before(k)
    return list(IMAGE_SIZES) + [(h << p, w << p) for h, w in TILE_SIZES]


# ---- lattice data ----------------------------------------------------------------------------------------------------------
def lattice_weights(seed, k, dense=()):
    """integer weights of layers 1 .. k.  Layer 1 and the layers in ``dense`` draw every weight from {-2 .. 2}; every other
    layer has two weights of +-1 per output channel (input channel and tap scattered with the output channel), sparse enough
    that the sums of a deep stack stay below 2^24.  Biases from {-1, 0, 1}."""
    g = torch.Generator().manual_seed(int(seed))
    pairs = []
    for l in range(1, k + 1):
        cin, cout = CHANNELS[l - 1], CHANNELS[l]
        if l == 1 or l in dense:
            w = torch.randint(-2, 3, (cout, cin, 3, 3), generator=g).float()
        else:
            w = torch.zeros(cout, cin, 3, 3)
            co = torch.arange(cout)
            for mul, add, tmul, tadd in ((5, 3, 1, 0), (11, 7, 7, 4)):
                ci = (co * mul + add + l) % cin
                tap = (co * tmul + tadd + co // 9) % 9
                sign = torch.randint(0, 2, (cout,), generator=g).float() * 2 - 1
                w[co, ci, tap // 3, tap % 3] += sign
        b = torch.randint(-1, 2, (cout,), generator=g).float()
        pairs.append((w, b))
    return pairs


def lattice_image(seed, H, W):
    g = torch.Generator().manual_seed(int(seed))
    return torch.randint(0, 8, (3, H, W), generator=g).float()


def lattice_cotangent(seed, C, h, w):
    g = torch.Generator().manual_seed(int(seed))
    return torch.randint(-1, 2, (C, h, w), generator=g).float()


def _exact_int(t, what):
    """float64 tensor of integers -> int64, the float64 arithmetic that produced it having been exact"""
    i = t.round().to(torch.int64)
    assert bool((i.double() == t).all()) and int(i.abs().max()) < 2 ** 52, f"{what}: not integers"
    return i


def lattice_forward(pairs, img):
    """int64 [z_1 .. z_k] of integer data, with the premises of an exact fp32 device result asserted:
    every split activation below 2^16, every weight a small integer (lo = 0), every output's sum |w| max|a| below 2^24.
    (The convolutions run in float64, exact far beyond these magnitudes; the results are checked to be integers.)"""
    x = _exact_int(img.double(), "image")
    zs = []
    for l, (w, b) in enumerate(pairs, start=1):
        wi, bi = _exact_int(w.double(), "weights"), _exact_int(b.double(), "bias")
        assert int(wi.abs().max()) <= 128, "weights must be small integers: their bf16 lo part is 0"
        amax = int(x.abs().max())
        if l > 1:
            assert amax < 2 ** 16, f"layer {l}: a split activation of magnitude {amax} >= 2^16"
        bound = int(wi.abs().sum(dim=(1, 2, 3)).max()) * amax + int(bi.abs().max())
        assert bound < 2 ** 24, f"layer {l}: sum |w| max|a| = {bound} >= 2^24"
        z = _exact_int(_conv(x.double(), wi.double(), bi.double()), f"z_{l}")
        zs.append(z)
        x = _advance(z, l)
    return zs


def lattice_backward(pairs, cot, dec):
    """int64 gradient to the image of integer data under the given decisions (normalize=False), premises asserted as above"""
    g = _exact_int(cot.double(), "cotangent")
    for l in range(len(pairs), 0, -1):
        wi = _exact_int(pairs[l - 1][0].double(), "weights")
        gmax = int(g.abs().max())
        assert gmax < 2 ** 16, f"layer {l}: a split cotangent of magnitude {gmax} >= 2^16"
        bound = int(wi.abs().sum(dim=(0, 2, 3)).max()) * gmax
        assert bound < 2 ** 24, f"layer {l} backward: sum |w| max|g| = {bound} >= 2^24"
        ga = _exact_int(_conv_t(g.double(), wi.double()), f"g_{l}")
        if l == 1:
            return ga
        H, W = dec["shape"][l - 1]
        g = _mask(ga, dec[l - 1], H, W)


@functools.lru_cache(maxsize=None)
def lattice_case(k, dense, H, W):
    """the exact tests' case: (weights, image, int64 z_k, cotangent, int64 image gradient) of the network cut at layer k with
    the layers in ``dense`` dense, premises asserted; computed once and shared"""
    pairs = lattice_weights(100 + k, k, dense=dense)
    img = lattice_image(200 + H * 1000 + W, H, W)
    zs = lattice_forward(pairs, img)
    dec = with_shapes(decisions_from(zs[:-1]), H, W)
    cot = lattice_cotangent(300 + k, *zs[-1].shape)
    return pairs, img, zs[-1], cot, lattice_backward(pairs, cot, dec)
