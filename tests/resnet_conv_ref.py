"""float64 references of ResNet-18's convolution GEMMs (csrc/pconv.hip, pwgrad.hip, pwgrad_ring.hip, stem_rows.hip, and igemm.hip /
wgrad.hip on a products = 0 handle) in the engine's layouts, the conv table at any input size, the operands of every case of
tests/test_resnet_conv_gpu.py, and the mutated references that tests/test_resnet_conv_ref_cpu.py uses to show that the comparisons
have teeth.  Host only.

Forward, data gradient and weight gradient go through F.conv2d and autograd in double; everything is linear in each operand, so a
call on absolute values yields the sum of |terms| the rounding bounds need.  A second, explicit tap-by-tap forward / weight gradient
(`taps_fwd`, `taps_wgrad`: pinned to the first by the CPU test) exists because the geometric mutants are mutations of its gather.

Operand families.
dyadic   _vals / _wts / _coef of tests/test_eff_kernels_gpu.py: multiples of 1/2 in [-2, 2] times {0, +-1/2, +-1, +-2}.  ResNet-18
         contracts up to K = 4608 terms over up to 19200 pixels per group, where dense dyadic weights would push the sum of squares
         of a statistics tile past 2^24 units of 1/16: a keep-mask (0 is a member of the weight set) leaves about DY_TERMS
         nonzero weights per contraction, in random positions, different per output channel.
random   standard normal.
planes3x activations (dy for the backward ops) = a dyadic value + [-3, 3] 2^-10 + [-3, 3] 2^-18: all three bf16 planes nonzero; the
         other operand holds one plane and is sparse -- weights from {+-1/2, +-1, +-2} with at most P3_W nonzeros per output channel
         AND per input channel (forward and data gradient contract over different axes), x of the weight gradient with at most P3_PIX
         nonzero pixels per channel.  Every term is a multiple of 2^-19 and sum|terms| < 32 = 2^24 units: every partial sum in any
         order is an fp32 number, and every product has a one-plane factor, so six products, nine products and the fp32 pipe all
         form it exactly.
planes3w the roles swapped: dense three-plane weights (through set_state: k_split_weights_bm and the data-gradient packs make their
         planes), one-plane activations on a lattice of one site per k x k window with at most P3_SITE / P3_SITE_DY nonzero channels;
         for the weight gradient x is dense three-plane and dy has at most P3_PIX nonzero pixels per channel."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import eff_ref as R
from tests.bn_ref import planes_of
from tests.conv_ref import dot_bound, epilogue, epilogue_bound, exact_terms, stats_bound  # noqa: F401  (the GPU and CPU tests take them from here)
from tests.test_kernels_gpu import conv_names

U = R.U
bn_stats = R.bn_stats
INFO_KEYS = ("cin", "cout", "k", "stride", "pad", "hin", "win", "hout", "wout", "cin_p", "Kw", "kw_p", "cout_p")
FAMILIES = ("dyadic", "random", "planes3x", "planes3w")
EXACT = ("dyadic", "planes3x", "planes3w")
# name: (H, W, imgs, groups, max_images of the handle)
SHAPES = {"S1": (32, 224, 4, 2, 4), "S2": (224, 32, 4, 2, 4), "S3": (96, 160, 5, 1, 5), "S4a": (32, 32, 1, 1, 3), "S4b": (32, 32, 3, 1, 3)}
DY_TERMS = 256          # nonzero dyadic weights per contraction (see above)
P3_W, P3_PIX, P3_SITE, P3_SITE_DY = 3, 6, 6, 3
P3_UNIT = 2.0 ** -19
P3_SET = np.array([0.5, -0.5, 1.0, -1.0, 2.0, -2.0])
STAT_TILE = 512         # no kernel folds more pixels than this into one statistics partial (pconv / igemm 256, stem_rows 448)


# ---- the convolutions of ResNet-18 -------------------------------------------------------------------------------------------------
def r18_convs(H, W):
    """[info] in the engine's conv order (conv_names()): fm_debug_conv_info's dict + name.  The stem is the packed form: the framed
    NHWC3 image, kernel rows of kw_p * cin_p = 24 floats (tap kw = 7 is a zero slot), 7 rows = 168 padded to Kw = 176"""
    out = []

    def add(name, cin, cout, k, s, h, w):
        stem = cin == 3
        pad = k // 2
        ho, wo = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
        out.append(dict(name=name, cin=cin, cout=cout, k=k, stride=s, pad=pad, hin=h, win=w, hout=ho, wout=wo, cin_p=cin,
                        Kw=176 if stem else k * k * cin, kw_p=8 if stem else k, cout_p=cout))
        return ho, wo

    h, w = add("conv1", 3, 64, 7, 2, H, W)
    h, w = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1           # the 3x3 / stride-2 / pad-1 max-pool
    cin = 64
    for li, width in enumerate((64, 128, 256, 512), start=1):
        for b in range(2):
            p = f"layer{li}.{b}"
            s = 2 if (li > 1 and b == 0) else 1
            h2, w2 = add(p + ".conv1", cin, width, 3, s, h, w)
            add(p + ".conv2", width, width, 3, 1, h2, w2)
            if s != 1 or cin != width:
                add(p + ".downsample.0", cin, width, 1, s, h, w)
            h, w, cin = h2, w2, width
    assert [c["name"] for c in out] == conv_names()
    return out


def block_convs(convs, block):
    """(conv1, downsample) indices of stride-2 basic block `block` (2, 4, 6)"""
    idx = {c["name"]: i for i, c in enumerate(convs)}
    p = f"layer{block // 2 + 1}.{block % 2}"
    return idx[p + ".conv1"], idx[p + ".downsample.0"]


# ---- float64 references (F.conv2d + autograd), engine layouts -----------------------------------------------------------------------
def _nchw(a):
    return torch.from_numpy(np.array(a, np.float64)).permute(0, 3, 1, 2).contiguous()


def _wt(w):
    return torch.from_numpy(np.array(w, np.float64))


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous().numpy()


def fwd(x, w, c):
    """x [N][hin][win][cin], w OIHW -> y [N][hout][wout][cout]"""
    return _nhwc(F.conv2d(_nchw(x), _wt(w), None, c["stride"], c["pad"]))


def dgrad(dy, w, c):
    """dy [N][hout][wout][cout] -> dx [N][hin][win][cin] (every parity class)"""
    x = torch.zeros((dy.shape[0], c["cin"], c["hin"], c["win"]), dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, _wt(w), None, c["stride"], c["pad"])
    (g,) = torch.autograd.grad(y, x, _nchw(dy))
    return _nhwc(g)


def written(dx, c):
    """the part of dx a conv's own data gradient writes: everything, except for a stride-2 1x1 conv, whose only parity class is
    (0, 0) (the block's 3x3 conv writes the rest)"""
    return dx[:, ::2, ::2] if (c["k"] == 1 and c["stride"] == 2) else dx


def engine_dw(g_oihw, c):
    """OIHW weight gradient -> the engine's [cout][k][kw_p][cin_p] padded to [cout][Kw]"""
    g = np.asarray(g_oihw, np.float64).transpose(0, 2, 3, 1)                      # O, kh, kw, I
    out = np.zeros((c["cout"], c["k"], c["kw_p"], c["cin_p"]), np.float64)
    out[:, :, :c["k"], :c["cin"]] = g
    flat = np.zeros((c["cout"], c["Kw"]), np.float64)
    flat[:, :c["k"] * c["kw_p"] * c["cin_p"]] = out.reshape(c["cout"], -1)
    return flat


def wgrad(x, dy, c):
    """-> dw [cout][Kw] (engine layout; zero tap slots and pad columns are 0)"""
    w = torch.zeros((c["cout"], c["cin"], c["k"], c["k"]), dtype=torch.float64, requires_grad=True)
    y = F.conv2d(_nchw(x), w, None, c["stride"], c["pad"])
    (g,) = torch.autograd.grad(y, w, _nchw(dy))
    return engine_dw(g.numpy(), c)


def block_dgrad(dy1, dyd, w1, wd, c1, cd):
    """dx of a stride-2 block: dgrad(conv1; dy1) + dgrad(downsample; dyd)"""
    return dgrad(dy1, w1, c1) + dgrad(dyd, wd, cd)


def class_taps(c):
    """[hin][win]: the kernel taps that reach an input pixel in the data gradient (those of its parity class): the terms of its
    dot product are these x cout"""
    def axis(n):
        i = np.arange(n)[:, None]
        return (((i + c["pad"] - np.arange(c["k"])[None, :]) % c["stride"]) == 0).sum(1)
    return axis(c["hin"])[:, None] * axis(c["win"])[None, :]


def dgrad_K(c):
    return (class_taps(c) * c["cout"])[None, :, :, None]


def stats_stored(y):
    """what fm_debug_conv hands back for exact tile partials: the float64 sum of the tiles, rounded once to fp32"""
    return lambda groups: bn_stats(y, groups).astype(np.float32).astype(np.float64)


def stats_tiles_exact(y, groups, unit):
    """the precondition of bit-exact statistics: over any STAT_TILE consecutive pixels of a group the sums of |y| (unit) and of
    y^2 (unit^2) stay below 2^24 units, so every tile partial is an fp32 number in any order (the fold over tiles runs in double)"""
    g = R.group_rows(np.abs(y), groups)
    for t, u in ((g, unit), (g * g, unit * unit)):
        if not np.array_equal(np.round(t / u), t / u):
            return False
        cs = np.concatenate([np.zeros_like(t[:, :1]), np.cumsum(t, 1)], 1)
        n = min(STAT_TILE, t.shape[1])
        if (cs[:, n:] - cs[:, :-n]).max() / u >= 2 ** 24:
            return False
    return True


# ---- explicit tap-by-tap forms: the base of the geometric mutants ---------------------------------------------------------------------
def _gather(x, ih, iw, mode):
    """x [N][H][W][C] at rows ih [Ho][1] and columns iw [1][Wo] -> [N][Ho][Wo][C], zero where the tap leaves the image.
    mode "true"; "row_wrap": the column is not checked -- a left / right neighbour outside the row is the adjacent row's end pixel
    (flat index inside the image); "img_wrap": the row is not checked -- a top / bottom neighbour outside the image is the adjacent
    image's row (flat index inside the batch)"""
    N, H, W, C = x.shape
    ih, iw = np.broadcast_arrays(ih, iw)
    if mode == "true":
        ok = (ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)
        return np.where(ok[None, :, :, None], x[:, np.clip(ih, 0, H - 1), np.clip(iw, 0, W - 1)], 0.0)
    if mode == "row_wrap":
        flat = ih * W + iw
        ok = (ih >= 0) & (ih < H) & (flat >= 0) & (flat < H * W)
        return np.where(ok[None, :, :, None], x.reshape(N, H * W, C)[:, np.clip(flat, 0, H * W - 1)], 0.0)
    assert mode == "img_wrap"
    flat = (np.arange(N)[:, None, None] * H + ih[None]) * W + iw[None]
    ok = (iw >= 0) & (iw < W) & (flat >= 0) & (flat < N * H * W)
    return np.where(ok[..., None], x.reshape(N * H * W, C)[np.clip(flat, 0, N * H * W - 1)], 0.0)


def _tap_rows(c):
    return np.arange(c["hout"])[:, None] * c["stride"] - c["pad"], np.arange(c["wout"])[None, :] * c["stride"] - c["pad"]


def taps_fwd(x, w, c, mode="true"):
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    ih0, iw0 = _tap_rows(c)
    wt = np.ascontiguousarray(w.transpose(2, 3, 1, 0))                          # [kh][kw][cin][cout]
    y = np.zeros((x.shape[0] * c["hout"] * c["wout"], c["cout"]))
    for kh in range(c["k"]):
        for kw in range(c["k"]):
            y += _gather(x, ih0 + kh, iw0 + kw, mode).reshape(-1, c["cin"]) @ wt[kh, kw]
    return y.reshape(x.shape[0], c["hout"], c["wout"], c["cout"])


def taps_wgrad(x, dy, c, mode="true"):
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    ih0, iw0 = _tap_rows(c)
    g = np.zeros((c["cout"], c["cin"], c["k"], c["k"]))
    d2 = dy.reshape(-1, c["cout"])
    for kh in range(c["k"]):
        for kw in range(c["k"]):
            g[:, :, kh, kw] = d2.T @ _gather(x, ih0 + kh, iw0 + kw, mode).reshape(-1, c["cin"])
    return engine_dw(g, c)


# ---- mutated references: what a subtly wrong kernel would compute (CPU test only) -----------------------------------------------------
def _swapped(c):
    return dict(c, hin=c["win"], win=c["hin"], hout=c["wout"], wout=c["hout"])


def mut_row_wrap(x, w, c):
    """forward whose left / right neighbours come from the adjacent row instead of zero"""
    return taps_fwd(x, w, c, "row_wrap")


def mut_img_wrap(x, w, c):
    """forward whose top / bottom neighbours come from the adjacent image instead of zero"""
    return taps_fwd(x, w, c, "img_wrap")


def mut_hw_swap(x, w, c):
    """forward that decodes pixel indices with H and W exchanged: the same memory read as a [W][H] map"""
    N = x.shape[0]
    y = fwd(np.asarray(x).reshape(N, c["win"], c["hin"], c["cin"]), w, _swapped(c))
    return y.reshape(N, c["hout"], c["wout"], c["cout"])


def mut_class_shift(dx):
    """data gradient of a stride-2 conv whose parity class (1, 1) lands one pixel to the right (cyclically)"""
    dx = np.array(dx, np.float64)
    dx[:, 1::2, 1::2] = np.roll(dx[:, 1::2, 1::2], 1, axis=2)
    return dx


def mut_drop_last_pixel(t, groups):
    """a copy of an NHWC tensor with the last pixel of every group zeroed: sums over pixels (weight gradient with groups = 1,
    statistics) lose it"""
    t = np.array(t, np.float64)
    g = t.reshape(groups, -1, t.shape[-1])
    g[:, -1] = 0.0
    return g.reshape(t.shape)


def mut_group_boundary(y, groups):
    """statistics whose first group ends one image late: [groups][2][C]"""
    y = np.asarray(y, np.float64)
    ipg = y.shape[0] // groups
    cuts = [0] + [ipg * g + 1 for g in range(1, groups)] + [y.shape[0]]
    parts = [y[a:b].reshape(-1, y.shape[-1]) for a, b in zip(cuts[:-1], cuts[1:])]
    return np.stack([np.stack([p.sum(0), (p * p).sum(0)]) for p in parts])


def mut_ring_pad(x, dy, c):
    """weight gradient of the ring form whose padding position behind a row's last pixel counts as a pixel: the right neighbour of
    column W - 1 is the next row's first pixel instead of zero"""
    return taps_wgrad(x, dy, c, "row_wrap")


def drop_plane(a, which):
    """a copy of fp32-valued `a` without its m (1) or l (2) bf16 plane"""
    planes = planes_of(np.asarray(a, np.float32))
    return np.asarray(a, np.float64) - planes[which].astype(np.float64)


GEOMETRIC = ("row_wrap", "img_wrap", "hw_swap", "class_shift", "wgrad_last_pixel", "stats_last_pixel", "group_boundary", "ring_pad")


def reachable(mutant, shape, c):
    """can a kernel make this mistake on conv c at this shape at all (would the mutated reference differ from the true one)?"""
    H, W, imgs, groups, _ = SHAPES[shape]
    k3s1 = c["k"] == 3 and c["stride"] == 1
    if mutant in ("row_wrap", "ring_pad"):      # needs a neighbouring row
        return k3s1 and c["hin"] > 1 and (mutant == "row_wrap" or 28 <= c["win"] <= 62)
    if mutant == "img_wrap":
        return k3s1 and imgs > 1
    if mutant == "hw_swap":
        return c["hin"] != c["win"] and c["k"] == 3
    if mutant == "class_shift":
        return c["stride"] == 2 and c["k"] == 3 and c["win"] >= 4 and c["hin"] >= 2
    if mutant == "group_boundary":
        return groups > 1
    return True


# ---- operands -------------------------------------------------------------------------------------------------------------------------
def _three_planes(rs, shape):
    return rs.randint(-4, 5, shape) / 2.0 + rs.randint(-3, 4, shape) * 2.0 ** -10 + rs.randint(-3, 4, shape) * 2.0 ** -18


def _sparse_weights(rs, shape):
    """OIHW from P3_SET with at most P3_W nonzeros per output channel and per input channel: P3_W rounds of a partial matching of
    output to input channels, one random tap each"""
    cout, cin, k, _ = shape
    w = np.zeros(shape)
    n = min(cout, cin)
    for _ in range(P3_W):
        o, i = rs.permutation(cout)[:n], rs.permutation(cin)[:n]
        w[o, i, rs.randint(0, k, n), rs.randint(0, k, n)] = rs.choice(P3_SET, n)
    return w


def _lattice(rs, shape, step, per_site):
    """NHWC from P3_SET, nonzero only at one site per step x step cell (a random offset per image) and there in at most `per_site`
    channels: any step x step window holds at most per_site nonzeros"""
    N, H, W, C = shape
    t = np.zeros(shape)
    for n in range(N):
        oh, ow = rs.randint(0, step), rs.randint(0, step)
        hs, ws = np.arange(oh, H, step), np.arange(ow, W, step)
        if not len(hs) or not len(ws):
            hs, ws = np.arange(H)[:1], np.arange(W)[:1]
        for h in hs:
            for w_ in ws:
                ch = rs.permutation(C)[:per_site]
                t[n, h, w_, ch] = rs.choice(P3_SET, len(ch))
    return t


def _sparse_pixels(rs, shape):
    """NHWC from P3_SET with at most P3_PIX nonzero pixels per channel"""
    N, H, W, C = shape
    t = np.zeros((N * H * W, C))
    for ch in range(C):
        p = rs.randint(0, N * H * W, P3_PIX)
        t[p, ch] = rs.choice(P3_SET, P3_PIX)
    return t.reshape(shape)


def model_weights(gen, family, seed=5151):
    """{conv name: OIHW float64 (fp32 values)} of the 20 convs"""
    rs = np.random.RandomState(seed + FAMILIES.index(family))
    out = {}
    for c in r18_convs(32, 32):
        shape = (c["cout"], c["cin"], c["k"], c["k"])
        if family == "planes3x":
            w = _sparse_weights(rs, shape)
        elif family == "planes3w":
            w = _three_planes(rs, shape)
        else:
            w = gen._wts(family, rs, (int(np.prod(shape)),)).reshape(shape)
            if family == "dyadic":
                K = c["cin"] * c["k"] * c["k"]
                w = w * (rs.random_sample(shape) < min(1.0, DY_TERMS / K))
        out[c["name"]] = w.astype(np.float32).astype(np.float64)
    return out


def state_dict(gen, family):
    """a ResNet-18 state_dict (spec.init_state) with the family's conv weights"""
    from fedmlp_amd import spec
    flat, cnt = spec.init_state("Resnet18", 5, 1037)
    sd = spec.flat_to_state_dict("Resnet18", 5, flat, cnt)
    for name, w in model_weights(gen, family).items():
        assert sd[name + ".weight"].shape == w.shape
        sd[name + ".weight"] = w.astype(np.float32)
    return sd


def operands(gen, family, shape, ci, c):
    """x, dy of the forward / data gradient and xw, dyw of the weight gradient of conv ci at a shape"""
    imgs = SHAPES[shape][2]
    rs = np.random.RandomState(20000 + 1000 * list(SHAPES).index(shape) + 10 * ci + FAMILIES.index(family))
    xs, ys = (imgs, c["hin"], c["win"], c["cin"]), (imgs, c["hout"], c["wout"], c["cout"])
    if family == "planes3x":
        x, dy = _three_planes(rs, xs), _three_planes(rs, ys)
        return dict(x=x, dy=dy, xw=_sparse_pixels(rs, xs), dyw=dy)
    if family == "planes3w":
        x, dy = _lattice(rs, xs, c["k"], P3_SITE), _lattice(rs, ys, c["k"], P3_SITE_DY)
        return dict(x=x, dy=dy, xw=_three_planes(rs, xs), dyw=_sparse_pixels(rs, ys))
    x, dy = gen._vals(family, rs, xs, False), gen._vals(family, rs, ys, False)
    return dict(x=x, dy=dy, xw=x, dyw=dy)


def unit(family):
    return 0.25 if family == "dyadic" else P3_UNIT


def sweep_reference(gen, family, shape, ci, weights):
    """operands and float64 results of the three ops of conv ci at a shape: y / ya (sum of |terms|), dx / dxa over the pixels the
    conv's own data gradient writes, dw / dwa"""
    H, W = SHAPES[shape][:2]
    c = r18_convs(H, W)[ci]
    w = weights[c["name"]]
    o = operands(gen, family, shape, ci, c)
    o.update(c=c, w=w)
    o["y"], o["ya"] = fwd(o["x"], w, c), fwd(np.abs(o["x"]), np.abs(w), c)
    o["dx"], o["dxa"] = written(dgrad(o["dy"], w, c), c), written(dgrad(np.abs(o["dy"]), np.abs(w), c), c)
    o["dxK"] = written(np.broadcast_to(dgrad_K(c), (1, c["hin"], c["win"], 1)), c)
    o["dw"], o["dwa"] = wgrad(o["xw"], o["dyw"], c), wgrad(np.abs(o["xw"]), np.abs(o["dyw"]), c)
    return o


def sweep_exact(o, family, groups):
    """the exactness preconditions of a sweep case of an exact family, on its own data"""
    u = unit(family)
    ok = exact_terms(o["ya"], u) and exact_terms(o["dxa"], u) and exact_terms(o["dwa"], u)
    return ok and (family != "dyadic" or stats_tiles_exact(o["y"], groups, u))


def block_reference(gen, family, shape, block, weights):
    """dy1, dyd and the float64 dx / dxa / K of fm_debug_block_dgrad for stride-2 block `block`"""
    H, W, imgs = SHAPES[shape][:3]
    convs = r18_convs(H, W)
    i1, id_ = block_convs(convs, block)
    c1, cd = convs[i1], convs[id_]
    w1, wd = weights[c1["name"]], weights[cd["name"]]
    dy1, dyd = operands(gen, family, shape, i1, c1)["dy"], operands(gen, family, shape, id_, cd)["dy"]
    return dict(c1=c1, cd=cd, dy1=dy1, dyd=dyd, dx=block_dgrad(dy1, dyd, w1, wd, c1, cd),
                dxa=block_dgrad(np.abs(dy1), np.abs(dyd), np.abs(w1), np.abs(wd), c1, cd), K=dgrad_K(c1) + dgrad_K(cd))


# ---- the planes eval epilogue -----------------------------------------------------------------------------------------------------------
# (conv name, relu, residual form, outputs): the five forms forward_eval hands conv_fwd in planes mode
EPILOGUE_CASES = (("layer1.0.conv1", 1, None, "planes"), ("layer1.0.conv2", 1, "planes", "both"), ("layer2.0.downsample.0", 0, None, "f32"),
                  ("layer2.0.conv2", 0, "f32", "planes"), ("layer4.1.conv2", 0, "planes", "f32"))
EPILOGUE_SHAPES = ("S1", "S3", "S4a", "S4b")


def epilogue_operands(gen, family, shape, ci, c, with_res):
    imgs = SHAPES[shape][2]
    rs = np.random.RandomState(40000 + 1000 * list(SHAPES).index(shape) + 10 * ci + (family == "random"))
    scale, shift = gen._coef(family, rs, (c["cout"],)), gen._coef(family, rs, (c["cout"],))
    res = gen._vals(family, rs, (imgs, c["hout"], c["wout"], c["cout"]), False) if with_res else None
    return scale, shift, res
