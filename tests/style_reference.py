"""What csrc/style.hip is held to (tests/test_style_reference.py without a GPU, tests/test_gpu_style_losses.py with one):
  * float64 statements of the eight functions of utils/loss_utils.py (:33-44, :230-272) and of their closed-form gradients;
  * the fp32 term-by-term restatement of the pixel losses and their gradients, in the kernels' operation order;
  * the kernels' tiling constants (restated, not imported: a change of the kernel has to be made twice) and the plans derived
    from them: workgroups of the pixel pass, slices of the statistics, tiles / chains / slices of the Gram kernel;
  * the emulation of the statistics' summation order in float64, and the error bounds of the MFMA kernels."""
import numpy as np

# ---- constants of csrc/style.hip ---------------------------------------------------------------------------------------------------
PX_WG_MAX, PX_WG_MIN_ELEMS = 512, 1024
ST_SLICES, ST_SLICE_MIN = 64, 4096
GR_TILE, GR_KT, GR_CHAIN, GR_SLICE_BUDGET, MFMA_BLOCK = 128, 32, 1024, 400, 32
GD_PER = 1024                       # elements of G - S per workgroup of the difference pass
STYLE_MAX_C = 512
U = 2.0 ** -24                      # unit roundoff of fp32


def gamma(m):
    """Higham's gamma_m for fp32: the relative error bound of an m-term recursive sum of exactly formed... products"""
    return m * U / (1.0 - m * U)


def px_blocks(n):
    return min(PX_WG_MAX, -(-n // PX_WG_MIN_ELEMS))


def st_slices(n):
    return min(ST_SLICES, -(-n // ST_SLICE_MIN))


def gram_tiles(C):
    t = -(-C // GR_TILE)
    return t * (t + 1) // 2


def gram_slice_cap(C):
    return max(1, GR_SLICE_BUDGET // gram_tiles(C))


def gram_plan(C, n):
    """(tiles, chains, chains per slice, slices) of the Gram kernel"""
    nchain = -(-n // GR_CHAIN)
    s0 = min(nchain, gram_slice_cap(C))
    cps = -(-nchain // s0)
    return gram_tiles(C), nchain, cps, -(-nchain // cps)


def gram_ws_bytes(C, n):
    """the float64 chain sums: 16384 per tile and slice"""
    t, _, _, s = gram_plan(C, n)
    return t * s * 16384 * 8


# ---- float64 statements ---------------------------------------------------------------------------------------------------------------
def masked_l1(x, gt, mask):
    m = np.broadcast_to(np.asarray(mask, np.float64)[None], x.shape)
    den = m.sum()
    return float((np.abs(x - gt) * m).sum() / den) if den != 0 else 0.0


def masked_l1_grad(x, gt, mask):
    m = np.broadcast_to(np.asarray(mask, np.float64)[None], x.shape)
    den = m.sum()
    return np.sign(x - gt) * m / den if den != 0 else np.zeros_like(x)


def weighted_l1(x, gt, w):
    return float((np.abs(x - gt) * np.broadcast_to(w, x.shape)).mean())


def weighted_l1_grad(x, gt, w):
    return np.sign(x - gt) * np.broadcast_to(w, x.shape) / x.size


def l2(x, y):
    return float(((x - y) ** 2).mean())


def l2_grad(x, y):
    return 2.0 * (x - y) / x.size


def mean_std(x2, eps=1e-8):
    """x2 (C, n) -> (mean, unbiased std + eps), two passes"""
    mu = x2.mean(axis=1)
    sd = np.sqrt(((x2 - mu[:, None]) ** 2).sum(axis=1) / (x2.shape[1] - 1))
    return mu, sd + eps


def mean_std_grad(x2, g_mean, g_std):
    """gradient of <g_mean, mean> + <g_std, std>; a channel of zero variance takes nothing from the std"""
    n = x2.shape[1]
    mu = x2.mean(axis=1)
    dev = x2 - mu[:, None]
    sd = np.sqrt((dev ** 2).sum(axis=1) / (n - 1))
    b = np.divide(g_std, (n - 1) * sd, out=np.zeros_like(sd), where=sd > 0)
    return g_mean[:, None] / n + b[:, None] * dev


def gram(x2):
    return x2 @ x2.T


def gram_grad(x2, g_gram):
    return (g_gram + g_gram.T) @ x2


def adain(x2, s_mean, s_std, eps=1e-8):
    mu, sd = mean_std(x2, eps)
    return float(((mu - s_mean) ** 2).mean() + ((sd - s_std) ** 2).mean())


def adain_grad(x2, s_mean, s_std, eps=1e-8):
    mu, sd = mean_std(x2, eps)
    c = x2.shape[0]
    return mean_std_grad(x2, 2.0 * (mu - s_mean) / c, 2.0 * (sd - s_std) / c)


def style_loss(x2, s_gram, weight):
    c, n = x2.shape
    return float(weight * ((gram(x2) - s_gram) ** 2).mean() / (c * n))


def style_loss_grad(x2, s_gram, weight):
    c, n = x2.shape
    d = 2.0 * weight / (c * c) / (c * n) * (gram(x2) - s_gram)
    return 2.0 * d @ x2


def node(x2, s_gram=None, s_mean=None, s_std=None, content=None, gw=0.0, aw=0.0, cw=0.0):
    """(total, gram, adain, content) of style_statistics_loss, every term weighted"""
    lg = style_loss(x2, s_gram, gw) if gw else 0.0
    la = aw * adain(x2, s_mean, s_std) if aw else 0.0
    lc = cw * l2(x2, content) if cw else 0.0
    return lg + la + lc, lg, la, lc


def node_grad(x2, s_gram=None, s_mean=None, s_std=None, content=None, gw=0.0, aw=0.0, cw=0.0):
    g = np.zeros_like(x2)
    if gw:
        g = g + style_loss_grad(x2, s_gram, gw)
    if aw:
        g = g + aw * adain_grad(x2, s_mean, s_std)
    if cw:
        g = g + cw * l2_grad(x2, content)
    return g


def grad_gemm(D, a, b, c, x2, y):
    """the backward launch on its own: 2 D x + a + b * x + c (x - y), every part optional"""
    g = np.zeros_like(x2)
    if D is not None:
        g = g + 2.0 * (D @ x2)
    if a is not None:
        g = g + a[:, None] + b[:, None] * x2
    if y is not None:
        g = g + c * (x2 - y)
    return g


def grad_gemm_abs(D, a, b, c, x2, y):
    """the sum of the absolute values of the terms of grad_gemm: what gamma_(C + 4) multiplies"""
    g = np.zeros_like(x2)
    if D is not None:
        g = g + 2.0 * (np.abs(D) @ np.abs(x2))
    if a is not None:
        g = g + np.abs(a)[:, None] + np.abs(b[:, None] * x2)
    if y is not None:
        g = g + np.abs(c * (x2 - y))
    return g


# ---- fp32 restatement of the pixel losses: the kernels' terms and gradients, operation by operation ---------------------------------------
F32 = np.float32
MASKED, WEIGHTED, L2 = 0, 1, 2


def byte_gt(planes_u8):
    """(3, H, W) bytes -> what the kernels read: the exact fp32 quotient"""
    return planes_u8.astype(F32) / F32(255.0)


def pixel_terms(kind, x, gt, aux=None):
    """(fp32 terms, float64 denominator).  aux: the mask (H, W) as float32 values, or the weight broadcastable to x"""
    x, gt = np.asarray(x, F32), np.asarray(gt, F32)
    d = x - gt
    if kind == L2:
        return d * d, float(x.size)
    a = np.broadcast_to(np.asarray(aux, F32), x.shape)
    terms = np.abs(d) * a
    return terms, (float(a.astype(np.float64).sum()) if kind == MASKED else float(x.size))


def pixel_value(kind, x, gt, aux=None):
    """the float64 sum of the fp32 terms over the denominator, rounded once (the kernel is within one ulp: its float64 sum has
    another order)"""
    terms, den = pixel_terms(kind, x, gt, aux)
    return F32(terms.astype(np.float64).sum() / den) if den != 0 else F32(0)


def pixel_grad(kind, x, gt, aux=None, g=1.0):
    """s = g * float(1 / denominator); l2: (2 s) * (x - gt); masked / weighted: sign(x - gt) * (aux * s), sign(0) = 0"""
    x, gt = np.asarray(x, F32), np.asarray(gt, F32)
    _, den = pixel_terms(kind, x, gt, aux)
    inv = F32(1.0 / den) if den != 0 else F32(0)
    s = F32(g) * inv
    d = x - gt
    if kind == L2:
        return (F32(2.0) * s) * d
    ms = np.broadcast_to(np.asarray(aux, F32), x.shape) * s
    return np.where(d > 0, ms, np.where(d < 0, -ms, F32(0))).astype(F32)


# ---- the statistics' summation order, emulated in float64 --------------------------------------------------------------------------------
def _block_sum(v):
    """what a workgroup of 256 threads does with the float64 values v of its slice: thread t adds v[t], v[t + 256], ... in order,
    then the halving tree"""
    pad = (-len(v)) % 256
    rows = np.concatenate([v, np.zeros(pad)]).reshape(-1, 256)
    acc = np.zeros(256)
    for r in rows:
        acc = acc + r
    o = 128
    while o:
        acc[:o] = acc[:o] + acc[o:2 * o]
        o //= 2
    return acc[0]


def emulated_mean_sd(row):
    """(float64 mean, float64 unbiased standard deviation before eps) of one channel exactly as the two passes sum it"""
    n = len(row)
    ss = st_slices(n)
    per = -(-n // ss)
    v = row.astype(np.float64)
    s = 0.0
    for k in range(ss):
        s += _block_sum(v[k * per:(k + 1) * per])
    mean = s / n
    m2 = 0.0
    for k in range(ss):
        d = v[k * per:(k + 1) * per] - mean
        m2 += _block_sum(d * d)
    return mean, np.sqrt(m2 / (n - 1))


# ---- the GPU test's case plans -------------------------------------------------------------------------------------------------------------
PIXEL_SHAPES = [(3, 1, 1), (3, 5, 7), (1, 31, 33), (3, 64, 65), (3, 33, 257)]
GRAM_C = [1, 31, 32, 33, 64, 65, 127, 128, 129, 512]
# n: 1 2 3 | the staging tile GR_KT - 1 / 0 / + 1 | one chain - 1 / 0 / + 1 | two slices + 1
GRAM_N = [1, 2, 3, GR_KT - 1, GR_KT, GR_KT + 1, GR_CHAIN - 1, GR_CHAIN, GR_CHAIN + 1, 2 * GR_CHAIN + 1]
GRAM_CASES = [(c, n) for c in GRAM_C for n in GRAM_N if c <= 129 or n in (3, GR_KT + 1, GR_CHAIN + 1, 2 * GR_CHAIN + 1)]
# the slice cap: more chains than slices, so a slice adds several chain results in its registers -- at one tile (cap 400), at the
# three tiles of C = 129 (cap 133) and at the 10 tiles of C = 512 (cap 40)
GRAM_CAP_CASES = [(31, GR_SLICE_BUDGET * GR_CHAIN + 1), (129, (GR_SLICE_BUDGET // 3) * GR_CHAIN + GR_CHAIN + 7), (512, 41 * GR_CHAIN + 5)]
STATS_C = [1, 3, 64, 512]
STATS_N = [2, 3, 255, 256, 257, 32400]
NODE_SHAPES = [(64, 8, 8), (128, 9, 15), (256, 33, 17), (512, 34, 60)]
LATTICE = 3                       # lattice rows take values in {-3 .. 3}


def lattice_rows(C, n, seed):
    return np.random.default_rng(seed).integers(-LATTICE, LATTICE + 1, size=(C, n)).astype(np.float64)


def gram_bound(x2):
    """|G - G64|[i][j] <= gamma_m * sum_k |x_ik x_jk|, m = chain length + 1: a chain is an m - 1 term fp32 recursive sum of exact
    products (one rounding per accumulation, <= gamma_(m-1)); the float64 combination and the final rounding add one more u"""
    a = np.abs(x2)
    return gamma(GR_CHAIN + 1) * (a @ a.T)
