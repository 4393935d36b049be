"""float64 restatement of the bf16 pointwise GEMM family of an EfficientNet-B0 engine with bf16 storage (csrc/pwconv_bf16.hip: the
streaming kernel pw_conv_bf16_kernel, the LDS-tiled pw_gemm_bf16_kernel, the block and wave weight-gradient kernels, the fused
expand / project backward kernels) and of the two fp32 fused twins (projbwd_f32.hip, expbwd_f32.hip), on the engine's own padded
arrays.  Built on tests/conv_ref.py (the conv table, pw_fwd / pw_dgrad / pw_wgrad / stem_fwd / stem_wgrad, prologue / epilogue, the
fp32 bounds, the mutators) and tests/eff_ref.py (bf16 words, swish); tests/test_pw_bf16_ref_cpu.py pins what is new here to torch
float64, tests/test_pw_bf16_gpu.py holds the kernels to it.

THE bf16 MODEL OF AN OPERAND.  Activations and gradients are bf16 numbers (the generators round to bf16).  A weight is the fp32
master rounded to nearest even onto bf16 (launch_cast_weights; `weights`): the reference multiplies by the rounded weight, so the
cast is part of the statement, not of the error.  A product of two bf16 numbers is exact in fp32, only the additions of a dot
product round: conv_ref.dot_bound, (K + 2) u sum|a b|, holds as it stands (it assumes round-to-nearest accumulation in the matrix
pipe; on the MI355X every fp32 output stayed below it -- the plain weight gradients at 0.04 of it -- so no measured factor replaces
K + 2: pw_bf16_parity.json).  An operand FORMED on load (x gate, swish(x psc + psh) gate; d y_e, d a_s, a_s inside the fused kernels) is computed in fp32
and re-rounded to bf16 before the MFMA.  The reference keeps it unrounded in float64 and carries the kernel's deviation as a bound
da = (fp32 error of forming it) + half a bf16 ulp of (|a| + that error), which enters the following sum as sum |other operand| da
(`formed`, `pro_bound`, `pro_wgrad_bound`): rigorous whichever way a near-tie rounds.  A bf16 store adds half a bf16 ulp of
|value| + bound (tests/test_eff_kernels_gpu.py: _check(..., bf=True)).  The fp32 twins form nothing in bf16: the same functions
with bf = False drop the half-ulp terms and read the fp32 master weights.

Train statistics are taken from the fp32 ACCUMULATORS of the GEMM (both kernels: s1 += acc, s2 += acc * acc before the bf16 store), so
their reference is the float64 (sum, sumsq) of the unrounded float64 output and `acc_stats_bound` carries each accumulator's own
dot-product bound through the sums.

Also here: the launch predicates of pwconv_bf16.hip restated (`conv_arm`, `wgrad_arm`, `exp_bwd_arm`, `proj_bwd_arm`), the forms the
model's graphs launch (`model_arms`), the operands of every case, and the mutated references for the bf16-specific ways to be wrong."""
import numpy as np

from tests import conv_ref as CR
from tests import eff_ref as R

U = R.U
IMGS, GROUPS = CR.IMGS, CR.GROUPS
SIDES = (96, 64)                    # the two square bf16 handles; the stem also runs at 96 x 64
STEM_HW = (96, 64)


def hb(x):
    return R.half_ulp_bf16(x)


def is_bf16(a):
    """every element is a bf16 number"""
    u = np.ascontiguousarray(np.asarray(a, np.float64).astype(np.float32)).view(np.uint32)
    return bool(np.array_equal(np.asarray(a, np.float64).astype(np.float32).astype(np.float64), np.asarray(a, np.float64))
                and not (u & 0xFFFF).any())


# ---- weights and operands -----------------------------------------------------------------------------------------------------------------
def weights(sd, c, bf=True):
    """[cout_p][Kw] as the kernels read them: the bf16 shadow of the fp32 master (bf) or the master itself (the fp32 twins)"""
    w = CR.weight_matrix(sd[c["name"]], c).reshape(c["cout_p"], c["Kw"])
    return R.bf16_round(w) if bf else w


def _padded(gen, family, rs, shape, real, bf=True):
    """an NHWC tensor of bf16 numbers whose pad channels are finite and non-zero (zero weight columns must hide them)"""
    t = gen._vals(family, rs, shape, bf)
    if shape[-1] > real:
        t[..., real:] = 1.5 if family == "dyadic" else 3.25
    return t


def nchw_to_nhwc4(x):
    """the stem's fp32 NCHW batch [N][3][H][W] as conv_ref.stem_fwd wants it: NHWC with a zero fourth channel"""
    x = np.asarray(x, np.float64)
    out = np.zeros((x.shape[0], x.shape[2], x.shape[3], 4), np.float64)
    out[..., :3] = x.transpose(0, 2, 3, 1)
    return out


def operands(gen, family, c, ci, imgs=IMGS, bf=True):
    """x, dy (pad channels loud) and xz, dyz (pad channels zero, for the weight gradient); the stem's x is the NCHW batch `xn`
    and its NHWC4 view"""
    rs = np.random.RandomState(17000 + 10 * ci + (family == "random") + 3 * c["hin"])
    ys = (imgs, c["hout"], c["wout"], c["cout_p"])
    if c["cin"] == 3:
        xn = gen._vals(family, rs, (imgs, 3, c["hin"], c["win"]), bf)
        x = nchw_to_nhwc4(xn)
    else:
        xn, x = None, _padded(gen, family, rs, (imgs, c["hin"], c["win"], c["cin_p"]), c["cin"], bf)
    dy = _padded(gen, family, rs, ys, c["cout"], bf)
    xz, dyz = x.copy(), dy.copy()
    xz[..., c["cin"]:] = 0.0
    dyz[..., c["cout"]:] = 0.0
    o = dict(x=x, dy=dy, xz=xz, dyz=dyz)
    if xn is not None:
        o["xn"] = xn
    return o


def sweep_reference(gen, family, ci, sd, convs, imgs=IMGS):
    """operands and float64 results of the three ops of conv ci on the bf16 shadow weights: y / ya, dx / dxa and the residual r of
    the data gradient (not for the stem), dw / dwa"""
    c = convs[ci]
    w = weights(sd, c)
    o = operands(gen, family, c, ci, imgs)
    o.update(c=c, w=w)
    o["y"], o["ya"] = CR.conv_fwd(o["x"], w, c), CR.conv_fwd(np.abs(o["x"]), np.abs(w), c)
    if c["cin"] != 3:
        o["dx"], o["dxa"] = CR.pw_dgrad(o["dy"], w), CR.pw_dgrad(np.abs(o["dy"]), np.abs(w))
        rs = np.random.RandomState(18000 + ci)
        o["r"] = gen._vals(family, rs, o["dx"].shape, True)
    o["dw"], o["dwa"] = CR.conv_wgrad(o["xz"], o["dyz"], c), CR.conv_wgrad(np.abs(o["xz"]), np.abs(o["dyz"]), c)
    return o


def sweep_exact(o, groups=GROUPS):
    """the dyadic precondition of a sweep case on its own data: every operand and weight a bf16 number, every sum exact in fp32"""
    ok = all(is_bf16(o[k]) for k in ("x", "dy", "w")) and CR.exact_terms(o["ya"], 0.25) and CR.exact_terms(o["dwa"], 0.25)
    if "dxa" in o:
        ok = ok and is_bf16(o["r"]) and CR.exact_terms(o["dxa"] + np.abs(o["r"]), 0.25)
    st = R.bn_stats(np.abs(o["y"]), groups)
    return ok and CR.exact_terms(st[:, 0], 0.25) and CR.exact_terms(st[:, 1], 1.0 / 16)


# ---- bounds ----------------------------------------------------------------------------------------------------------------------------------
def acc_stats_bound(y, b, groups):
    """[groups][2][C]: the fused (sum, sumsq) of accumulators within b of y, against the float64 sums of y: the accumulators' own
    deviation, sum b and sum (2 |y| b + b^2), plus the summation of what is summed ((n + 1) u sum|acc|, (n + 2) u sum acc^2 as
    conv_ref.stats_bound counts them)"""
    ya, b = R.group_rows(np.abs(y), groups), R.group_rows(np.broadcast_to(b, np.shape(y)), groups)
    n, m = ya.shape[1], ya + b
    return np.stack([b.sum(1) + (n + 1) * U * m.sum(1), (2 * ya * b + b * b).sum(1) + (n + 2) * U * (m * m).sum(1)], 1)


def residual_bound(v, b):
    """a value within b of its reference plus an exactly converted residual, v = the float64 sum: one more rounding"""
    return b + U * (np.abs(v) + b)


def formed(a, e, bf=True):
    """bound of an operand formed in fp32 within e of the float64 value a and then (bf) re-rounded to bf16"""
    e = np.broadcast_to(np.asarray(e, np.float64), np.shape(a))
    return e + hb(np.abs(a) + e) if bf else e + 0.0


def pro_operand(gen, x, gate, psc=None, psh=None, bf=True):
    """(a, da): the operand of a launch with a prologue in float64, and the bound of the kernel's bf16 operand against it.  Gate
    only: one fp32 rounding of x gate.  Affine form: v = x psc + psh (gen._affine_err), swish (gen._swish_err: hardware exp and
    rcp), times the gate, one more rounding"""
    a = CR.prologue(x, gate, psc, psh)
    e = U * np.abs(a)
    if psc is not None:
        x = np.asarray(x, np.float64)
        sc, sh = CR.per_pixel(psc, x), CR.per_pixel(psh, x)
        e = e + gen._swish_err(x * sc + sh, gen._affine_err(x, sc, sh)) * np.abs(CR.per_pixel(gate, x))
    return a, formed(a, e, bf)


def pro_bound(a, da, w):
    """forward on a formed operand: (K + 2) u sum (|a| + da) |w| + sum |w| da"""
    aw = np.abs(np.asarray(w, np.float64)).reshape(-1, a.shape[-1])
    return CR.dot_bound(a.shape[-1], CR.pw_fwd(np.abs(a) + da, aw)) + CR.pw_fwd(da, aw)


def pro_wgrad_bound(a, da, dy):
    """weight gradient dy^T a on a formed operand, n = pixels"""
    n = int(np.prod(a.shape[:-1]))
    return CR.dot_bound(n, CR.pw_wgrad(np.abs(a) + da, np.abs(dy))) + CR.pw_wgrad(da, np.abs(dy))


# ---- the fused backward kernels -------------------------------------------------------------------------------------------------------------------
def _pp(v, t):
    """per-group [groups][C] or per-image [imgs][C] vector -> per pixel of t [imgs][HW][C]"""
    v = np.asarray(v, np.float64)
    return np.repeat(v, t.shape[0] // v.shape[0], axis=0)[:, None, :]


def exp_bwd(da, ye, x, w, bn, res=None):
    """fm_debug_exp_bwd: da, ye [imgs][HW][L], x, res [imgs][HW][S], w [L][S], bn [5][groups][L] = ca, cb, cc, scale, shift ->
    (d y_e [imgs][HW][L] unrounded, dx [imgs][HW][S], dw [L][S])"""
    da, ye, x, w = (np.asarray(t, np.float64) for t in (da, ye, x, w))
    ca, cb, cc, sc, sh = (_pp(v, ye) for v in bn)
    dye = ca * (da * R.swish_grad(ye * sc + sh)) + cb * ye + cc
    dx = dye @ w
    if res is not None:
        dx = dx + np.asarray(res, np.float64)
    return dye, dx, CR.pw_wgrad(x, dye)


def exp_bwd_bounds(gen, da, ye, x, w, bn, res=None, bf=True):
    """(bound of dx before the store, bound of dw).  d y_e in fp32: d = da swish'(v) carries gen._swish_grad_err at v within
    gen._affine_err and one rounding; ca d + cb y + cc 3 u (|ca d| + |cb y| + |cc|) (two products, two sums, as
    test_bnact_bwd_apply counts them); then (bf) the bf16 re-rounding (`formed`).  dx = sum_l dye w: (L + 2) u sum (|dye| + d) |w| + sum
    |w| d, the residual addition one more rounding.  dw = sum_pix dye x likewise with n = pixels"""
    da, ye, x, w = (np.asarray(t, np.float64) for t in (da, ye, x, w))
    ca, cb, cc, sc, sh = (_pp(v, ye) for v in bn)
    v = ye * sc + sh
    sg = R.swish_grad(v)
    d = da * sg
    ed = np.abs(da) * gen._swish_grad_err(v, gen._affine_err(ye, sc, sh)) + U * np.abs(d)
    dye = ca * d + cb * ye + cc
    dl = formed(dye, np.abs(ca) * ed + 3 * U * (np.abs(ca * d) + np.abs(cb * ye) + np.abs(cc)), bf)
    L = ye.shape[-1]
    bx = CR.dot_bound(L, (np.abs(dye) + dl) @ np.abs(w)) + dl @ np.abs(w)
    if res is not None:
        bx = residual_bound(dye @ w + np.asarray(res, np.float64), bx)
    n = int(np.prod(ye.shape[:-1]))
    bw = CR.dot_bound(n, CR.pw_wgrad(np.abs(x), np.abs(dye) + dl)) + CR.pw_wgrad(np.abs(x), dl)
    return bx, bw


def proj_bwd(dyp, yd, w, bn, gate, ds=None, hw_div=None):
    """fm_debug_proj_bwd: dyp [imgs][HW][S], yd [imgs][HW][L], w [S][L], bn [7][groups][L] = scale, shift, mean, istd, ca, cb, cc,
    gate / ds [imgs][L] -> dict(das = dyp w unrounded, a_s, pool5 [imgs][5][L], dw [S][L], dyd (with ds)); hw_div: the divisor of
    ds (the image's pixel count; another value is the mutation)"""
    dyp, yd, w, gate = (np.asarray(t, np.float64) for t in (dyp, yd, w, gate))
    sc, sh, mean, istd, ca, cb, cc = (_pp(v, yd) for v in bn)
    das = dyp @ w
    v = yd * sc + sh
    ad, sg, xh = R.swish(v), R.swish_grad(v), (yd - mean) * istd
    out = dict(das=das, a_s=ad * gate[:, None, :])
    out["pool5"] = np.stack([(das * ad).sum(1), (das * sg).sum(1), (das * sg * xh).sum(1), sg.sum(1), (sg * xh).sum(1)], 1)
    out["dw"] = CR.pw_wgrad(out["a_s"], dyp)
    if ds is not None:
        d = das * gate[:, None, :] + np.asarray(ds, np.float64)[:, None, :] / (hw_div or yd.shape[1])
        out["dyd"] = ca * (d * sg) + cb * yd + cc
    return out


def proj_bwd_bounds(gen, dyp, yd, w, bn, gate, ds=None, bf=True):
    """dict(pool5, dw, dyd): d a_s = dyp w is within dd = `formed`((S + 2) u sum|dyp w|) of the float64 product; v, swish, swish'
    as in exp_bwd_bounds; xhat = (y - mean) istd two roundings.  Every term of the five sums carries the errors of its factors and
    one rounding per product; a sum over the HW pixels of an image, in records that are added afterwards, (HW + 2) u sum|terms|.
    a_s = swish(v) gate: one more rounding, then `formed`; dw as pro_wgrad_bound.  dyd: d = das gate + ds / HW (roundings of 1 / HW, the
    two products, the sum), times swish', then ca d + cb y + cc as above"""
    dyp, yd, w, gate = (np.asarray(t, np.float64) for t in (dyp, yd, w, gate))
    sc, sh, mean, istd, ca, cb, cc = (_pp(v, yd) for v in bn)
    S, HW = dyp.shape[-1], yd.shape[1]
    das = dyp @ w
    dd = formed(das, CR.dot_bound(S, np.abs(dyp) @ np.abs(w)), bf)
    dm = np.abs(das) + dd
    v = yd * sc + sh
    dv = gen._affine_err(yd, sc, sh)
    ad, sg, xh = R.swish(v), R.swish_grad(v), (yd - mean) * istd
    e_ad, e_sg, e_xh = gen._swish_err(v, dv), gen._swish_grad_err(v, dv), 2 * U * np.abs(xh)
    t1, e1 = das * sg, dd * np.abs(sg) + dm * e_sg + U * dm * (np.abs(sg) + e_sg)
    terms = [(das * ad, dd * np.abs(ad) + dm * e_ad + U * dm * (np.abs(ad) + e_ad)), (t1, e1),
             (t1 * xh, e1 * np.abs(xh) + (np.abs(t1) + e1) * e_xh + U * (np.abs(t1) + e1) * np.abs(xh) * (1 + 2 * U)),
             (sg, e_sg), (sg * xh, e_sg * np.abs(xh) + (np.abs(sg) + e_sg) * e_xh + U * (np.abs(sg) + e_sg) * np.abs(xh) * (1 + 2 * U))]
    out = dict(pool5=np.stack([e.sum(1) + (HW + 2) * U * (np.abs(t) + e).sum(1) for t, e in terms], 1))
    g = np.abs(gate)[:, None, :]
    a_s = ad * gate[:, None, :]
    das_ = formed(a_s, e_ad * g + U * (np.abs(a_s) + e_ad * g), bf)
    out["dw"] = pro_wgrad_bound(a_s, das_, dyp)
    if ds is not None:
        dsv = np.asarray(ds, np.float64)[:, None, :] / HW
        d = das * gate[:, None, :] + dsv
        ed = dd * g + U * dm * g + 2 * U * np.abs(dsv) + U * (dm * g + np.abs(dsv))
        t, et = d * sg, ed * np.abs(sg) + (np.abs(d) + ed) * e_sg + U * (np.abs(d) + ed) * (np.abs(sg) + e_sg)
        out["dyd"] = np.abs(ca) * et + 3 * U * (np.abs(ca) * (np.abs(t) + et) + np.abs(cb * yd) + np.abs(cc))
    return out


def fused_operands(gen, family, kind, c, ci, groups, imgs=IMGS, bf=True, linear=False):
    """operands of a fused-backward case.  kind "exp": da, ye [imgs][HW][L], x, res [imgs][HW][S], bn [5][groups][L]; kind "proj": dyp
    [imgs][HW][S] (pad channels zero, as the engine's), yd [imgs][HW][L], bn [7][groups][L], gate, ds [imgs][L].  Coefficients differ per
    group and gates per image.  linear (the dyadic entry): scale = shift = 0 and ca = 0, so that whatever the hardware's sigmoid
    returns is multiplied by an exact zero and every remaining operation is exact"""
    rs = np.random.RandomState(23000 + 10 * ci + groups + 5 * c["hout"] + (family == "random"))
    HW = c["hout"] * c["wout"]
    big, small = (c["cout_p"], c["cin_p"]) if kind == "exp" else (c["cin_p"], c["cout_p"])
    vec = lambda n: gen._coef(family, rs, (n, groups, big))
    o = {}
    if kind == "exp":
        o["da"], o["ye"] = gen._vals(family, rs, (imgs, HW, big), bf), gen._vals(family, rs, (imgs, HW, big), bf)
        o["x"], o["res"] = gen._vals(family, rs, (imgs, HW, small), bf), gen._vals(family, rs, (imgs, HW, small), bf)
        o["x"][..., c["cin"]:] = 0.0
        bn = vec(5)
        if linear:
            bn[0], bn[3], bn[4] = 0.0, 0.0, 0.0
    else:
        o["dyp"], o["yd"] = gen._vals(family, rs, (imgs, HW, small), bf), gen._vals(family, rs, (imgs, HW, big), bf)
        o["dyp"][..., c["cout"]:] = 0.0
        bn = vec(7)
        if family == "random":
            bn[3] = np.abs(bn[3]) + 0.5                      # istd
        if linear:
            bn[0], bn[1], bn[4] = 0.0, 0.0, 0.0
        o["gate"], o["ds"] = gen._coef(family, rs, (imgs, big)), gen._coef(family, rs, (imgs, big))
        o["gate"][:, 0] = (np.arange(imgs) % 3 + 1) * (0.25 if family == "dyadic" else 0.37)
    if groups > 1 and not linear:
        bn[:, 1] = bn[:, 0] + (0.5 if family == "dyadic" else 0.61) * (1 + np.arange(bn.shape[0]))[:, None]
    o["bn"] = bn
    return o


# ---- launch predicates of pwconv_bf16.hip, restated ---------------------------------------------------------------------------------------------------
def pw_gemm_takes(M, K, pro, plain, HW):
    if M % 16 or K % 16:
        return False
    return (K >= 240 and M <= 128 and HW >= 32) if pro else (plain and K >= 64)


def pw_rt(K):
    return 4 if K <= 1152 else 2


def pw_ppb(npix, groups, M, K):
    MT = 16 * pw_rt(K)
    tiles_m = (M + MT - 1) // MT
    ppb = max(npix * groups * tiles_m // 2048, 16 * MT)
    ppb = min(max(ppb, 128), 4096)
    return (ppb + 31) // 32 * 32


def _remap(nby):
    """which branches of the XCD block-id remap a launch of nby pixel ranges runs"""
    full = nby // 8 * 8
    return tuple(n for n, on in (("full", full > 0), ("rem", nby > full)) if on)


def conv_arm(M, K, npix, groups, HW, mode, pro=0):
    """launch_pw_conv for a GEMM of M output rows and K terms over `groups` groups of npix pixels; mode 0 plain store / 1 statistics /
    2 eval epilogue, pro 0 / 1 gate / 2 affine + gate.
    ("gemm", BM, mode, pro, K % 64, nrt of the last M-tile, tiles_m, remap) | ("stream", (RT, P, KB, NW), mode, pro > 0, K % 32 == 16,
    nrt of the last M-tile, tiles_m, remap)"""
    if pw_gemm_takes(M, K, pro > 0, mode == 0, HW):
        BM = 64 if M <= 64 else 128
        tm, nblk = (M + BM - 1) // BM, (npix + 127) // 128
        return ("gemm", BM, mode, pro, K % 64, (M - (tm - 1) * BM) // 16, tm, _remap(nblk * groups))
    RT = pw_rt(K)
    MT = 16 * RT
    ppb = pw_ppb(npix, groups, M, K)
    nblk, tm = (npix + ppb - 1) // ppb, (M + MT - 1) // MT
    form = (4, 4, 2, 4) if RT == 4 and K <= 64 else ((4, 2, 4, 8) if RT == 4 and K > 640 else ((4, 2, 4, 4) if RT == 4 else (2, 2, 4, 4)))
    return ("stream", form, mode, pro > 0, K % 32 == 16, (M - (tm - 1) * MT) // 16, tm, _remap(nblk * groups))


def wgrad_arm(M, K, pro=False):
    """launch_pw_wgrad: ("wave", nrt, cc, pro) | ("block", CC, swap, pro) | None (S > 320: refused)"""
    L, S = max(M, K), min(M, K)
    if S > 320 or S % 16 or L % 16:
        return None
    nrt, cc = L // 16, S // 16
    if ((nrt, cc) in ((2, 1), (6, 1), (6, 2), (9, 2))) and (not pro or nrt == 2):
        return ("wave", nrt, cc, pro)
    return ("block", next((v for v in (1, 2, 3, 5, 7, 12, 20) if v >= cc), 20), K > M, pro)


def exp_bwd_arm(L, S, npix, pix_per_group, groups, bf=True):
    """launch_pw_exp_bwd / launch_pw_exp_bwd_f32: ("exp_bwd", nrt, cc) | None"""
    nrt, cc, q = L // 16, S // 16, 32 if bf else 16
    shape = ((nrt, cc) in ((6, 1), (9, 2))) if bf else (nrt in (6, 9) and cc in (1, 2))
    if not shape or L % 16 or S % 16 or pix_per_group % q or npix % q or not 1 <= groups <= 2:
        return None
    return ("exp_bwd", nrt, cc)


def proj_bwd_nch(L, S, imgs, HW, bf=True):
    """pw_proj_bwd_nch / pw_proj_bwd_f32_nch: pooling records per image, 0 = shape not handled"""
    ls = 32 if L == 32 else (48 if L % 48 == 0 else 0)
    if not ls or L // ls > (5 if bf else 3) or S not in (16, 32, 48) or imgs < 1 or HW % 16:
        return 0
    return max(1, min(min(16, (HW + 31) // 32), (2048 + imgs - 1) // imgs))


def proj_bwd_arm(L, S, imgs, HW, bf=True):
    """("proj_bwd", NLT = slice / 16, CS = S / 16, slices, ragged last tile) | None; both phases are instantiated for each"""
    if not proj_bwd_nch(L, S, imgs, HW, bf):
        return None
    ls = 32 if L == 32 else 48
    return ("proj_bwd", ls // 16, S // 16, L // ls, HW % 32 != 0)


def fuses_gate(c):
    """fuse_for (bf16): the project convs whose operand prologue the engine fuses, pw_tiles_m(cout_p, cin_p) <= 2"""
    if c["role"] != "project":
        return False
    M, K = c["cout_p"], c["cin_p"]
    return ((M + 127) // 128 if (K >= 240 and M <= 128) else (M + 16 * pw_rt(K) - 1) // (16 * pw_rt(K))) <= 2


def model_arms(convs, imgs, groups):
    """every (conv index, op, arm) the graphs of a bf16 engine can launch on `convs` with imgs images: the train forward (statistics,
    `groups` views; the fused project convs with the affine prologue), the eval forward (one group; the fused project convs with
    the gate), the data gradient, the weight gradient (the fused project convs with the affine prologue; each of these also without the
    prologue, as the engine runs them when it materialises a_s), and the fused backward kernels where their launchers take the shape.  A fused backward replaces the separate launches only where it is taken, and
    whether it is depends on the input size: the separate ones are listed for every conv"""
    out = []
    for i, c in enumerate(convs):
        M, K, HW = c["cout_p"], c["Kw"] if c["cin"] == 3 else c["cin_p"], c["hout"] * c["wout"]
        for fg in ((True, False) if fuses_gate(c) else (False,)):       # (FM_FUSE_GATE=0: a_s materialised, no prologue anywhere)
            out.append((i, "train", conv_arm(M, K, imgs // groups * HW, groups, HW, 1, 2 if fg else 0)))
            out.append((i, "eval", conv_arm(M, K, imgs * HW, 1, HW, 2, 1 if fg else 0)))
            out.append((i, "wgrad", wgrad_arm(M, K, fg)))
        if c["cin"] == 3:
            continue
        out.append((i, "dgrad", conv_arm(K, M, imgs * HW, 1, HW, 0)))
        if c["role"] == "expand" and M in (96, 144) and K <= 32:
            a = exp_bwd_arm(M, K, imgs * HW, imgs // groups * HW, groups)
            if a:
                out.append((i, "exp_bwd", a))
        if c["role"] == "project":
            a = proj_bwd_arm(K, M, imgs, HW)
            if a:
                out.append((i, "proj_bwd", a))
    return out


def tile_row_to_channel(r, i, npairs):
    return 32 * (r >> 1) + 8 * (i >> 2) + 4 * (r & 1) + (i & 3) if r < 2 * npairs else 16 * r + i


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------------
def short(c):
    return c["name"].replace("_blocks.", "b").replace("._expand_conv.weight", ".exp").replace("._project_conv.weight", ".proj") \
        .replace("_conv_stem.weight", "stem").replace("_conv_head.weight", "head")


def index(convs):
    return {short(c): i for i, c in enumerate(convs)}


def epilogue_operands(gen, family, c, ci, act, res, imgs=IMGS):
    """conv_ref.epilogue_operands with the residual as the engine holds it: bf16 numbers"""
    scale, shift, r = CR.epilogue_operands(gen, family, c, ci, act, res, imgs)
    return scale, shift, (None if r is None else R.bf16_round(r))


def epilogue_cases(convs):
    """(conv index, act, res, gate) on the 96 x 96 handle: swish with scale / shift on the stem, a streaming expand conv with K <= 64
    and the head; scale / shift / res without activation on a streaming project conv (K = 144) and a K > 640 project conv (the
    8-wave form); gate prologue + scale / shift / res on a K >= 240, M <= 128 project conv at HW = 36 (pw_gemm <128, 2, 1>) and on
    block 0's project conv (K = 32: the streaming <4, 4, 2> form with PRO, MODE 2)"""
    ix = index(convs)
    return [(0, 2, False, False), (ix["b1.exp"], 2, False, False), (len(convs) - 1, 2, False, False), (ix["b2.proj"], 0, True, False),
            (ix["b10.proj"], 0, True, False), (ix["b6.proj"], 0, True, True), (ix["b0.proj"], 0, True, True)]


def epilogue_cases_64(convs):
    """on the 64 x 64 handle: the same gate + scale / shift / res form at HW = 16 < 32 (streaming PRO, MODE 2: K = 240 in the 4-wave
    and K = 672 in the 8-wave form) and at HW = 64 (pw_gemm <64, 2, 1>, M = 48)"""
    ix = index(convs)
    return [(ix["b6.proj"], 0, True, True), (ix["b9.proj"], 0, True, True), (ix["b4.proj"], 0, True, True)]


def prologue_convs(convs):
    """every project conv whose prologue the engine fuses (blocks 0-10)"""
    return [i for i, c in enumerate(convs) if fuses_gate(c)]


def exp_bwd_convs(convs):
    """the expand convs of shape (96, 16) and (144, 32): blocks 1 and 2 (block 3's has the shape and the map of block 2's)"""
    ix = index(convs)
    return [ix["b1.exp"], ix["b2.exp"]]


def proj_bwd_convs(convs, bf=True):
    """one project conv per shape pw_proj_bwd_nch / pw_proj_bwd_f32_nch accept: (32, 16), (96, 32), (144, 32), (144, 48), (240, 48; bf16)"""
    ix = index(convs)
    return [ix[n] for n in ("b0.proj", "b1.proj", "b2.proj", "b3.proj") + (("b4.proj",) if bf else ())]


# ---- mutated references: the bf16-specific ways to be wrong ------------------------------------------------------------------------------------------------
def mut_stats_of_stored(y, groups):
    """the statistics of the bf16-ROUNDED output instead of the accumulators"""
    return R.bn_stats(R.bf16_round(y), groups)


def mut_unpermute(y, MT=64):
    """the two row tiles of every full pair of an M-tile stored without tile_row_to_channel: position 16 r + i of the tile holds the
    value of channel tile_row_to_channel(r, i)"""
    y = np.array(y, np.float64)
    M = y.shape[-1]
    out = y.copy()
    for m0 in range(0, M, MT):
        nrt = min(MT, M - m0) // 16
        for r in range(nrt):
            for i in range(16):
                out[..., m0 + 16 * r + i] = y[..., m0 + tile_row_to_channel(r, i, nrt // 2)]
    return out


def mut_gate_next_image(x, gate, psc=None, psh=None, last=3):
    """the last `last` pixels of every image take the next image's gate row"""
    a = CR.prologue(x, gate, psc, psh).reshape(x.shape[0], -1, x.shape[-1])
    b = CR.prologue(x, np.roll(np.asarray(gate, np.float64), -1, axis=0), psc, psh).reshape(a.shape)
    a[:, -last:] = b[:, -last:]
    return a.reshape(x.shape)
