"""float64 restatements of the convolution GEMMs of an fp32 EfficientNet-B0 engine (csrc/conv1x1.hip, igemm.hip, wgrad.hip) on the
engine's own padded arrays: NHWC activations with cin_p / cout_p channels, weights [cout_p][k][kw_p][cin_p] (pad rows, pad taps and
pad channels zero).  tests/test_conv_ref_cpu.py pins every function to F.conv2d + autograd in float64;
tests/test_eff_conv_f32_gpu.py holds the kernels to them.  Everything is linear algebra on what it is given, so calling a function
on absolute values yields the sum of |terms| that the rounding bounds need.

Also here, because the CPU test and the GPU test must agree on them: the table of the 33 convolutions at an input size (what
fm_debug_conv_info reports), which kernel arm a convolution takes (the `takes` conditions of the launchers restated), the operands of
every case (drawn by the generators of tests/test_eff_kernels_gpu.py, handed in as `gen`), the error bounds, and the mutated
references that show the comparator has teeth."""
import numpy as np

from fedmlp_amd import spec
from tests import eff_ref as R

U = R.U
IMGS, GROUPS, SIDE = 6, 2, 96          # the shapes of tests/test_eff_conv_f32_gpu.py: maps of 48, 24, 12, 6, 3; HW = 9 at the end


def r16(c):
    return (c + 15) // 16 * 16


# ---- the convolutions of EfficientNet-B0 --------------------------------------------------------------------------------------------
def b0_convs(H=SIDE, W=SIDE):
    """[info] in the engine's conv order (stem, per block expand? + project, head); info = fm_debug_conv_info's dict + name (the
    state_dict key of the weight) + role"""
    out = []

    def add(name, role, cin, cout, k, s, h, w):
        stem = cin == 3
        cin_p, kw_p = (4, 4) if stem else (r16(cin), k)
        out.append(dict(name=name, role=role, cin=cin, cout=cout, k=k, stride=s, pad=R.same_pad(h, k, s) if stem else 0, hin=h, win=w,
                        hout=R.out_size(h, s), wout=R.out_size(w, s), cin_p=cin_p, Kw=k * kw_p * cin_p, kw_p=kw_p, cout_p=r16(cout)))
        return out[-1]["hout"], out[-1]["wout"]

    h, w = add("_conv_stem.weight", "stem", 3, 32, 3, 2, H, W)
    for i, (k, s, e, cin, cout) in enumerate(spec.b0_blocks()):
        if e != 1:
            add(f"_blocks.{i}._expand_conv.weight", "expand", cin, cin * e, 1, 1, h, w)
        h, w = R.out_size(h, s), R.out_size(w, s)
        add(f"_blocks.{i}._project_conv.weight", "project", cin * e, cout, 1, 1, h, w)
    add("_conv_head.weight", "head", 320, 1280, 1, 1, h, w)
    return out


INFO_KEYS = ("cin", "cout", "k", "stride", "pad", "hin", "win", "hout", "wout", "cin_p", "Kw", "kw_p", "cout_p")


# ---- which kernel a convolution takes (conv1x1_stream_takes, launch_wgrad_skinny restated) ---------------------------------------
def stream_takes(K, M):
    """conv1x1_stream_takes for a stride-1 1x1 GEMM of K input and M output channels"""
    return K <= 256 and K % 16 == 0


def fwd_arm(c):
    """("stem",) | ("stream", M, K) | ("igemm", M, K)"""
    if c["cin"] == 3:
        return ("stem",)
    return ("stream" if stream_takes(c["cin_p"], c["cout_p"]) else "igemm", c["cout_p"], c["cin_p"])


def dgrad_arm(c):
    """the data gradient is the 1x1 GEMM with the transposed weights: M = cin_p rows, K = cout_p (the stem's has kernels of its own,
    csrc/stem_dgrad.hip, covered by tests/test_input_grad_gpu.py)"""
    if c["cin"] == 3:
        return ("stem",)
    return ("stream" if stream_takes(c["cout_p"], c["cin_p"]) else "igemm", c["cin_p"], c["cout_p"])


def wgrad_arm(c):
    """("skinny", CC, swap, gathered) | ("generic",): the skinny kernels take min(cout_p, Kw) <= 128; CC = 16-column groups of the
    small side, swap = the large operand is x"""
    S = min(c["cout_p"], c["Kw"])
    if S > 128:
        return ("generic",)
    return ("skinny", min((S + 15) // 16, 8), c["Kw"] > c["cout_p"], c["cin"] == 3)


def stream_sp(K, products):
    """the product form the streaming kernel runs: the split forms while the weight planes fit (K <= 192)"""
    return products if K <= 192 else 0


# ---- weights -----------------------------------------------------------------------------------------------------------------------------
def weight_matrix(w_oihw, c):
    """OIHW [cout][cin][k][k] -> the engine's [cout_p][k][kw_p][cin_p] (zeros in every pad slot)"""
    w = np.asarray(w_oihw, np.float64)
    out = np.zeros((c["cout_p"], c["k"], c["kw_p"], c["cin_p"]), np.float64)
    out[:c["cout"], :, :c["k"], :c["cin"]] = w.transpose(0, 2, 3, 1)
    return out


# ---- pointwise (1x1, stride 1) ----------------------------------------------------------------------------------------------------------
def pw_fwd(x, w):
    """x [N][H][W][cin_p], w [cout_p][cin_p] -> y [N][H][W][cout_p]"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64).reshape(-1, x.shape[-1])
    return x @ w.T


def pw_dgrad(dy, w):
    """dy [N][H][W][cout_p] -> dx [N][H][W][cin_p]"""
    dy = np.asarray(dy, np.float64)
    return dy @ np.asarray(w, np.float64).reshape(dy.shape[-1], -1)


def pw_wgrad(x, dy):
    """-> dw [cout_p][cin_p]"""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    return dy.reshape(-1, dy.shape[-1]).T @ x.reshape(-1, x.shape[-1])


# ---- the 3x3 stride-2 stem with TF-"same" padding ------------------------------------------------------------------------------------------
def _stem_frame(x, c):
    N, H, W, C = x.shape
    k, s, pt, pl = c["k"], c["stride"], R.same_pad(c["hin"], c["k"], c["stride"]), R.same_pad(c["win"], c["k"], c["stride"])
    xp = np.zeros((N, (c["hout"] - 1) * s + k + pt, (c["wout"] - 1) * s + k + pl, C), np.float64)
    xp[:, pt:pt + H, pl:pl + W] = x
    return xp


def stem_fwd(x, w, c):
    """x [N][H][W][cin_p = 4], w [cout_p][k][kw_p][cin_p] -> y [N][Ho][Wo][cout_p]; the pad tap kw = k and the pad channel carry zero
    weights, so whatever x holds there does not count"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64).reshape(c["cout_p"], c["k"], c["kw_p"], c["cin_p"])
    xp, s, Ho, Wo = _stem_frame(x, c), c["stride"], c["hout"], c["wout"]
    y = np.zeros((x.shape[0], Ho, Wo, c["cout_p"]), np.float64)
    for kh in range(c["k"]):
        for kw in range(c["k"]):
            y += xp[:, kh:kh + (Ho - 1) * s + 1:s, kw:kw + (Wo - 1) * s + 1:s] @ w[:, kh, kw].T
    return y


def stem_wgrad(x, dy, c):
    """-> dw [cout_p][k][kw_p][cin_p]; the pad tap stays 0"""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    xp, s, Ho, Wo = _stem_frame(x, c), c["stride"], c["hout"], c["wout"]
    dw = np.zeros((c["cout_p"], c["k"], c["kw_p"], c["cin_p"]), np.float64)
    d2 = dy.reshape(-1, c["cout_p"])
    for kh in range(c["k"]):
        for kw in range(c["k"]):
            dw[:, kh, kw] = d2.T @ xp[:, kh:kh + (Ho - 1) * s + 1:s, kw:kw + (Wo - 1) * s + 1:s].reshape(-1, c["cin_p"])
    return dw


def conv_fwd(x, w, c):
    return stem_fwd(x, w, c) if c["cin"] == 3 else pw_fwd(x, w)


def conv_wgrad(x, dy, c):
    """-> [cout_p][Kw]"""
    return (stem_wgrad(x, dy, c) if c["cin"] == 3 else pw_wgrad(x, dy)).reshape(c["cout_p"], c["Kw"])


# ---- operand prologue and eval epilogue -----------------------------------------------------------------------------------------------------
def per_pixel(v, x):
    """per-image [N][C] or per-group [groups][C] vector -> broadcastable over x [N][H][W][C] (image i in group i // (N / groups))"""
    v = np.asarray(v, np.float64)
    return np.repeat(v, x.shape[0] // v.shape[0], axis=0)[:, None, None, :]


def prologue(x, gate, psc=None, psh=None):
    """the operand of the streaming kernel: x gate[img], or swish(x psc[g] + psh[g]) gate[img]"""
    x = np.asarray(x, np.float64)
    if psc is not None:
        x = R.swish(x * per_pixel(psc, x) + per_pixel(psh, x))
    return x * per_pixel(gate, x)


def epilogue(y, scale, shift, res=None, a=0):
    """act(y scale + shift + res)"""
    v = np.asarray(y, np.float64) * np.asarray(scale, np.float64) + np.asarray(shift, np.float64)
    if res is not None:
        v = v + np.asarray(res, np.float64)
    return R.act(v, a)


# ---- bounds (u = 2^-24; csrc/split3.h) -------------------------------------------------------------------------------------------------------
def dot_bound(K, abs_sum):
    """a K-term dot product in any of the product forms, accumulated in fp32 in any order and in any number of partial sums that
    are then added (wgrad splits, stream-K partial tiles: n/s + s + 1 <= n + 2 roundings for s >= 1 partial sums of n/s terms), is
    within (K + 2) u sum|a b| of the float64 value"""
    return (K + 2) * U * np.asarray(abs_sum, np.float64)


def stats_bound(y_stored, groups):
    """bounds [groups][2][C] of the fused (sum, sumsq) against the float64 sums of the stored output: n additions and the final
    rounding of the folded tiles, (n + 1) u sum|y|; the square adds one rounding per term, (n + 2) u sum y^2"""
    g = R.group_rows(np.abs(y_stored), groups)
    n = g.shape[1]
    return np.stack([(n + 1) * U * g.sum(1), (n + 2) * U * (g * g).sum(1)], 1)


def prologue_bound(gen, x, gate, psc, psh, w):
    """bound of a pointwise forward whose operand a is formed on load: (K + 2) u sum|a w| + sum |w| da.  Gate only: a = x gate is one
    rounding, da = u |a|.  Affine form: v = x psc + psh carries gen._affine_err, swish(v) gen._swish_err(v, dv) (hardware exp and
    rcp), the gate one more rounding: da = swish_err |gate| + u |a|"""
    a = prologue(x, gate, psc, psh)
    da = U * np.abs(a)
    if psc is not None:
        x = np.asarray(x, np.float64)
        sc, sh = per_pixel(psc, x), per_pixel(psh, x)
        da = da + gen._swish_err(x * sc + sh, gen._affine_err(x, sc, sh)) * np.abs(per_pixel(gate, x))
    aw = np.abs(np.asarray(w, np.float64)).reshape(-1, a.shape[-1])
    return dot_bound(a.shape[-1], pw_fwd(np.abs(a), aw)) + pw_fwd(da, aw)


def epilogue_bound(gen, y, dy, scale, shift, res=None, a=0):
    """bound of act(y scale + shift + res) given the bound dy of y: the affine part rounds twice (gen._affine_err), the residual
    addition once, relu is 1-Lipschitz, swish goes through gen._swish_err"""
    y, scale, shift = np.asarray(y, np.float64), np.asarray(scale, np.float64), np.asarray(shift, np.float64)
    v = y * scale + shift
    dv = dy * np.abs(scale) + gen._affine_err(y, scale, shift)
    if res is not None:
        v = v + np.asarray(res, np.float64)
        dv = dv + U * np.abs(v)
    return gen._swish_err(v, dv) if a == 2 else dv


def exact_terms(abs_sum, unit):
    """the dyadic precondition: every term is a multiple of `unit` and sum|terms| < 2^24 units, so that every partial sum in any
    order is an fp32 number (`abs_sum` = that sum of |terms| per output element)"""
    t = np.asarray(abs_sum, np.float64) / unit
    return bool(np.array_equal(np.round(t), t) and (t.max() if t.size else 0.0) < 2 ** 24)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------
def model_weights(gen, family, seed=4242):
    """a state_dict whose conv weights come from the family's weight generator (DYW in the dyadic family, standard normal in the
    random one), everything else from spec.init_state"""
    flat, cnt = spec.init_state("Efficient_b0", 5, 3)
    sd = spec.flat_to_state_dict("Efficient_b0", 5, flat, cnt)
    rs = np.random.RandomState(seed)
    for c in b0_convs():
        shape = sd[c["name"]].shape
        sd[c["name"]] = gen._wts(family, rs, (int(np.prod(shape)),)).reshape(shape).astype(np.float32)
    return sd


def _padded(gen, family, rs, shape, real, zero_pad):
    """an NHWC operand whose pad channels are zero (weight gradient) or finite and non-zero (forward, data gradient: zero weight
    columns must hide them)"""
    t = gen._vals(family, rs, shape, False)
    if shape[-1] > real:
        t[..., real:] = 0.0 if zero_pad else (1.5 if family == "dyadic" else 3.25)
    return t


def operands(gen, family, c, ci, imgs=IMGS):
    """x, dy for the forward / data gradient (pad channels loud) and xz, dyz for the weight gradient (pad channels zero)"""
    rs = np.random.RandomState(7000 + 10 * ci + (family == "random"))
    xs, ys = (imgs, c["hin"], c["win"], c["cin_p"]), (imgs, c["hout"], c["wout"], c["cout_p"])
    x, dy = _padded(gen, family, rs, xs, c["cin"], False), _padded(gen, family, rs, ys, c["cout"], False)
    xz, dyz = x.copy(), dy.copy()
    xz[..., c["cin"]:] = 0.0
    dyz[..., c["cout"]:] = 0.0
    return dict(x=x, dy=dy, xz=xz, dyz=dyz)


def sweep_reference(gen, family, ci, sd, convs=None):
    """operands and float64 results of the three ops of conv ci: y (+ its sum of |terms| ya), dx / dxa (not for the stem), dw / dwa"""
    c = (convs or b0_convs())[ci]
    w = weight_matrix(sd[c["name"]], c)
    o = operands(gen, family, c, ci)
    o.update(c=c, w=w.reshape(c["cout_p"], c["Kw"]))
    o["y"], o["ya"] = conv_fwd(o["x"], w, c), conv_fwd(np.abs(o["x"]), np.abs(w), c)
    if c["cin"] != 3:
        o["dx"], o["dxa"] = pw_dgrad(o["dy"], w), pw_dgrad(np.abs(o["dy"]), np.abs(w))
    o["dw"], o["dwa"] = conv_wgrad(o["xz"], o["dyz"], c), conv_wgrad(np.abs(o["xz"]), np.abs(o["dyz"]), c)
    return o


def sweep_exact(o):
    """the dyadic precondition of a sweep case on its own data: products are multiples of 1/4, squares of outputs of 1/16"""
    ok = exact_terms(o["ya"], 0.25) and exact_terms(o["dwa"], 0.25) and ("dxa" not in o or exact_terms(o["dxa"], 0.25))
    st = R.bn_stats(np.abs(o["y"]), GROUPS)
    return ok and exact_terms(st[:, 0], 0.25) and exact_terms(st[:, 1], 1.0 / 16)


def prologue_operands(gen, family, c, ci, groups, imgs=IMGS, zero_affine=False):
    """gate [imgs][cin_p] (different per image), psc / psh [groups][cin_p] (different per group; zero_affine: the dyadic entry of
    the affine form, psc = psh = 0)"""
    rs = np.random.RandomState(9000 + 10 * ci + groups)
    gate = gen._coef(family, rs, (imgs, c["cin_p"]))
    gate[:, 0] = (np.arange(imgs) % 3 + 1) * (0.25 if family == "dyadic" else 0.37)      # no two neighbouring images alike
    psc, psh = gen._coef(family, rs, (groups, c["cin_p"])), gen._coef(family, rs, (groups, c["cin_p"]))
    if zero_affine:
        psc, psh = np.zeros_like(psc), np.zeros_like(psh)
    elif groups > 1:
        psc[1] = psc[0] + (0.5 if family == "dyadic" else 0.61)
    return gate, psc, psh


def epilogue_operands(gen, family, c, ci, act, res, imgs=IMGS):
    """scale, shift [cout_p] and res [imgs][hout][wout][cout_p] | None of an eval epilogue.  Dyadic: act 2 enters at scale = shift = 0
    (swish(0) = 0 exactly), act 0 / 1 with DYC coefficients"""
    rs = np.random.RandomState(11000 + 10 * ci + act)
    scale, shift = gen._coef(family, rs, (c["cout_p"],)), gen._coef(family, rs, (c["cout_p"],))
    if family == "dyadic" and act == 2:
        scale, shift = np.zeros_like(scale), np.zeros_like(shift)
    r = gen._vals(family, rs, (imgs, c["hout"], c["wout"], c["cout_p"]), False) if res else None
    return scale, shift, r


def epilogue_cases(convs=None):
    """(conv index, act, res) of the eval-epilogue test: swish with scale / shift on the stem, one expand conv and the head; scale /
    shift / res without activation on one streaming and one igemm project conv"""
    convs = convs or b0_convs()
    idx = {c["name"]: i for i, c in enumerate(convs)}
    return [(0, 2, False), (idx["_blocks.1._expand_conv.weight"], 2, False), (len(convs) - 1, 2, False),
            (idx["_blocks.2._project_conv.weight"], 0, True), (idx["_blocks.7._project_conv.weight"], 0, True)]


def prologue_convs(convs=None):
    """indices of the convs test 3 runs: the project convs with cin_p 32, 96, 144, 240 (HW = 2304, 576, 144, 36) and every
    stream-eligible 1x1 conv on the 6x6 and 3x3 maps"""
    convs = convs or b0_convs()
    want = {(32, 48), (96, 24), (144, 12), (240, 6)}
    out = []
    for i, c in enumerate(convs):
        if c["k"] != 1 or not stream_takes(c["cin_p"], c["cout_p"]):
            continue
        if (c["role"] == "project" and (c["cin_p"], c["hout"]) in want) or c["hout"] in (6, 3):
            out.append(i)
    return out


# ---- mutated references: what a subtly wrong kernel would compute ------------------------------------------------------------------------------
def mut_gate_next_image(x, gate, psc=None, psh=None):
    """the last pixel of every image takes the NEXT image's gate (the last image: the first one's)"""
    a = prologue(x, gate, psc, psh)
    b = prologue(x, np.roll(np.asarray(gate, np.float64), -1, axis=0), psc, psh)
    a[:, -1, -1] = b[:, -1, -1]
    return a


def mut_group0_affine(x, gate, psc, psh):
    """group 1 reads psc / psh of group 0"""
    psc, psh = np.array(psc, np.float64), np.array(psh, np.float64)
    psc[1:], psh[1:] = psc[0], psh[0]
    return prologue(x, gate, psc, psh)


def mut_drop_last_chunk(w, dgrad=False):
    """the weights [cout_p][Kw] as a GEMM sees them that skips the last 16-k chunk of its K (forward: the last 16 columns; data
    gradient, K = cout_p: the last 16 rows)"""
    w = np.array(w, np.float64)
    if dgrad:
        w[-16:] = 0.0
    else:
        w[:, -16:] = 0.0
    return w


def mut_drop_last_pixel(t, groups):
    """a copy of an NHWC tensor with the last pixel of every group zeroed: sums over pixels (weight gradient, statistics) lose it"""
    t = np.array(t, np.float64)
    g = t.reshape(groups, -1, t.shape[-1])
    g[:, -1] = 0.0
    return g.reshape(t.shape)


def mut_row_shift(y, cout):
    """output row cout - 1 written to row cout (dropped when there is no such row); row cout - 1 keeps the value 0"""
    y = np.array(y, np.float64)
    if cout < y.shape[-1]:
        y[..., cout] = y[..., cout - 1]
    y[..., cout - 1] = 0.0
    return y
