"""tests/resnet_conv_ref.py (the float64 yardstick of tests/test_resnet_conv_gpu.py) pinned to F.conv2d + autograd in float64 at the
four shapes of the GPU file, the exactness preconditions of the dyadic and planes3 families asserted on the data the GPU test uses,
and the comparisons shown to have teeth: every geometric mutant is rejected by bit equality in the dyadic family and by the random
family's bound, every plane mutant by bit equality in the planes3 family -- while it stays inside the random bound, which is why
that family exists.  No GPU."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import resnet_conv_ref as RR
from tests import test_eff_kernels_gpu as GEN          # the operand generators (no GPU at import)

TOL = 1e-12
SHAPES = list(RR.SHAPES)
# (K + 2) u sum|a b| grows as K^2 u: from K ~ 1 / sqrt(u) = 4096 on, a worst-case bound is wider than ONE term of the sum.  The two
# mutants that lose a single term are therefore asserted against the random bound where the sum has at most this many terms, and
# against bit equality in the dyadic family everywhere.
RESOLVE_K = 2048


def _close(name, got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = max(1.0, float(np.abs(want).max()))
    assert np.abs(got - want).max() <= TOL * scale, (name, float(np.abs(got - want).max()))


def _beyond(got, want, bound):
    """the comparator of the GPU test (`_within`): is any element further from `want` than its bound?"""
    return bool((np.abs(np.asarray(got, np.float64) - want) > bound).any())


def _differs(got, want):
    """the comparator of the exact families (`_bits`): any element with different fp32 bits"""
    return not np.array_equal(np.asarray(got, np.float64).astype(np.float32), np.asarray(want, np.float64).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _w(family):
    return RR.model_weights(GEN, family)


@functools.lru_cache(maxsize=48)
def _case(family, shape, ci):
    return RR.sweep_reference(GEN, family, shape, ci, _w(family))


def test_conv_table():
    """20 convs in conv_names() order; the packed stem; the maps the GPU file's shape table promises"""
    maps = {"S1": [(8, 56), (4, 28), (2, 14), (1, 7)], "S2": [(56, 8), (28, 4), (14, 2), (7, 1)], "S3": [(24, 40), (12, 20), (6, 10), (3, 5)],
            "S4a": [(8, 8), (4, 4), (2, 2), (1, 1)]}
    for shape, want in maps.items():
        H, W, imgs, groups, _ = RR.SHAPES[shape]
        convs = RR.r18_convs(H, W)
        assert len(convs) == 20 and set(convs[0]) == set(RR.INFO_KEYS) | {"name"}
        s = convs[0]
        assert (s["cin_p"], s["kw_p"], s["Kw"], s["k"], s["stride"], s["pad"], s["hout"], s["wout"]) == (3, 8, 176, 7, 2, 3, H // 2, W // 2)
        got = []
        for c in convs[1:]:
            assert c["cin_p"] == c["cin"] and c["cout_p"] == c["cout"] and c["kw_p"] == c["k"] and c["Kw"] == c["k"] ** 2 * c["cin"]
            if (c["hout"], c["wout"]) not in got:
                got.append((c["hout"], c["wout"]))
        assert got == want, (shape, got)
        assert [imgs // groups * h * w for h, w in want] == {"S1": [896, 224, 56, 14], "S2": [896, 224, 56, 14], "S3": [4800, 1200, 300, 75],
                                                               "S4a": [64, 16, 4, 1]}[shape]
    assert RR.r18_convs(32, 224)[0]["wout"] == 112 and RR.block_convs(RR.r18_convs(32, 32), 2) == (5, 7)
    assert [RR.block_convs(RR.r18_convs(32, 32), b) for b in (4, 6)] == [(10, 12), (15, 17)]


@pytest.mark.parametrize("shape", SHAPES)
def test_references_against_conv2d(shape):
    """every reference function and the explicit tap forms against F.conv2d + backward() in float64 on NCHW tensors, the engine
    layouts restated here with F.pad as tests/test_kernels_gpu.py does"""
    H, W, imgs = RR.SHAPES[shape][:3]
    convs = RR.r18_convs(H, W)
    rs = np.random.RandomState(17)
    grads = {}
    for ci, c in enumerate(convs):
        w = rs.standard_normal((c["cout"], c["cin"], c["k"], c["k"]))
        x, dy = rs.standard_normal((imgs, c["hin"], c["win"], c["cin"])), rs.standard_normal((imgs, c["hout"], c["wout"], c["cout"]))
        xt = torch.tensor(x).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        wt = torch.tensor(w, requires_grad=True)
        y = F.conv2d(xt, wt, None, c["stride"], c["pad"])
        assert tuple(y.shape) == (imgs, c["cout"], c["hout"], c["wout"])
        y.backward(torch.tensor(dy).permute(0, 3, 1, 2))
        _close("fwd", RR.fwd(x, w, c), y.detach().permute(0, 2, 3, 1).numpy())
        _close("taps_fwd", RR.taps_fwd(x, w, c), y.detach().permute(0, 2, 3, 1).numpy())
        dx = xt.grad.permute(0, 2, 3, 1).numpy()
        grads[ci] = (dy, w, dx)
        dgr = RR.dgrad(dy, w, c)
        _close("dgrad", dgr, dx)
        want = dx[:, ::2, ::2] if (c["k"] == 1 and c["stride"] == 2) else dx
        _close("written", RR.written(dgr, c), want)
        g = F.pad(wt.grad.permute(0, 2, 3, 1), (0, c["cin_p"] - c["cin"], 0, c["kw_p"] - c["k"])).reshape(c["cout"], -1)
        g = F.pad(g, (0, c["Kw"] - g.shape[1])).numpy()
        dw = RR.wgrad(x, dy, c)
        _close("wgrad", dw, g)
        _close("taps_wgrad", RR.taps_wgrad(x, dy, c), g)
        if ci == 0:         # the zero tap slot kw = 7 of every kernel row and the 8 pad columns
            g4 = dw[:, :168].reshape(64, 7, 8, 3)
            assert not g4[:, :, 7].any() and g4[:, :, :7].all() and not dw[:, 168:].any()
        # the terms of a data-gradient dot product: all-ones operands count them (fewer at the borders, where taps leave the map)
        ones, K = RR.dgrad(np.ones_like(dy), np.ones_like(w), c), np.broadcast_to(RR.dgrad_K(c), (imgs, c["hin"], c["win"], c["cin"]))
        assert (ones <= K).all() and np.array_equal(ones[:, 4:-4, 4:-4], K[:, 4:-4, 4:-4]), c["name"]
    for b in (2, 4, 6):
        i1, id_ = RR.block_convs(convs, b)
        assert convs[i1]["stride"] == 2 and convs[id_]["k"] == 1 and convs[i1]["hin"] == convs[id_]["hin"]
        _close("block", RR.block_dgrad(grads[i1][0], grads[id_][0], grads[i1][1], grads[id_][1], convs[i1], convs[id_]),
               grads[i1][2] + grads[id_][2])


def test_plane_families_have_three_planes():
    """the planes3 operands do exercise the m and l planes, and their one-plane partners hold one plane"""
    rs = np.random.RandomState(3)
    h, m, l = RR.planes_of(RR._three_planes(rs, (4000,)).astype(np.float32))
    # (the 2^-18 part stays in l whenever it is odd or the 2^-10 part leaves it no room in m: about 4 values in 10)
    assert np.count_nonzero(m) > 3000 and np.count_nonzero(l) > 1200
    for t in (RR._sparse_weights(rs, (64, 64, 3, 3)), RR._lattice(rs, (2, 8, 56, 64), 3, 6), RR._sparse_pixels(rs, (2, 8, 56, 64))):
        h, m, l = RR.planes_of(t.astype(np.float32))
        assert np.count_nonzero(t) and not m.any() and not l.any()
    w = RR._sparse_weights(rs, (128, 64, 3, 3))
    assert (np.count_nonzero(w, axis=(1, 2, 3)) <= RR.P3_W).all() and (np.count_nonzero(w, axis=(0, 2, 3)) <= RR.P3_W).all()


@pytest.mark.parametrize("family", RR.EXACT)
@pytest.mark.parametrize("shape", SHAPES)
def test_exactness_preconditions(shape, family):
    """every (shape, conv, op) of the GPU sweep, every block and (dyadic) every epilogue case: all terms are multiples of the family's
    unit and sum|terms| < 2^24 units; the dyadic statistics over any tile of pixels likewise"""
    H, W, imgs, groups, _ = RR.SHAPES[shape]
    convs = RR.r18_convs(H, W)
    for ci in range(20):
        assert RR.sweep_exact(_case(family, shape, ci), family, groups), (shape, family, convs[ci]["name"])
    for b in (2, 4, 6):
        assert RR.exact_terms(RR.block_reference(GEN, family, shape, b, _w(family))["dxa"], RR.unit(family)), (shape, family, b)
    if family == "dyadic" and shape in RR.EPILOGUE_SHAPES:
        idx = {c["name"]: i for i, c in enumerate(convs)}
        for name, relu, res_form, outs in RR.EPILOGUE_CASES:
            ci = idx[name]
            o = _case(family, shape, ci)
            scale, shift, res = RR.epilogue_operands(GEN, family, shape, ci, o["c"], res_form is not None)
            terms = o["ya"] * np.abs(scale) + np.abs(shift) + (np.abs(res) if res is not None else 0.0)
            assert RR.exact_terms(terms, 1.0 / 16), (shape, name)


def _one_term(mutant, o, shape):
    c, (imgs, groups) = o["c"], RR.SHAPES[shape][2:4]
    if mutant == "wgrad_last_pixel":
        return imgs * c["hout"] * c["wout"]
    if mutant == "stats_last_pixel":
        return imgs // groups * c["hout"] * c["wout"]
    return 0


def _mutate(mutant, o, shape):
    """[(mutated, true, random-family bound)] of one geometric mutant on one case"""
    c, w = o["c"], o["w"]
    imgs, groups = RR.SHAPES[shape][2:4]
    if mutant in ("row_wrap", "img_wrap", "hw_swap"):
        f = {"row_wrap": RR.mut_row_wrap, "img_wrap": RR.mut_img_wrap, "hw_swap": RR.mut_hw_swap}[mutant]
        return [(f(o["x"], w, c), o["y"], RR.dot_bound(c["Kw"], o["ya"]))]
    if mutant == "class_shift":
        return [(RR.mut_class_shift(o["dx"]), o["dx"], RR.dot_bound(o["dxK"], o["dxa"]))]
    if mutant == "wgrad_last_pixel":
        return [(RR.wgrad(o["xw"], RR.mut_drop_last_pixel(o["dyw"], 1), c), o["dw"], RR.dot_bound(imgs * c["hout"] * c["wout"], o["dwa"]))]
    if mutant == "ring_pad":
        return [(RR.mut_ring_pad(o["xw"], o["dyw"], c), o["dw"], RR.dot_bound(imgs * c["hout"] * c["wout"], o["dwa"]))]
    true, bound = RR.bn_stats(o["y"], groups), RR.stats_bound(o["y"], groups)
    mut = RR.bn_stats(RR.mut_drop_last_pixel(o["y"], groups), groups) if mutant == "stats_last_pixel" else RR.mut_group_boundary(o["y"], groups)
    return [(mut[:, k], true[:, k], bound[:, k]) for k in (0, 1)]


@pytest.mark.parametrize("mutant", RR.GEOMETRIC)
@pytest.mark.parametrize("shape", SHAPES)
def test_geometric_mutants_are_rejected(shape, mutant):
    """on every conv of the shape where the mistake can be made at all: the mutated reference differs in bits from the true one in
    the dyadic family and lies outside the random family's bound (the single-term mutants: where the sum has <= RESOLVE_K terms --
    every shape has such convs)"""
    H, W = RR.SHAPES[shape][:2]
    cis = [ci for ci, c in enumerate(RR.r18_convs(H, W)) if RR.reachable(mutant, shape, c)]
    if mutant == "hw_swap":
        assert bool(cis) == (H != W)
    if mutant == "group_boundary":
        assert bool(cis) == (RR.SHAPES[shape][3] > 1)
    if mutant == "img_wrap":
        assert bool(cis) == (RR.SHAPES[shape][2] > 1)
    if mutant == "ring_pad":
        assert bool(cis) == (shape in ("S1", "S3"))
    if mutant in ("row_wrap", "class_shift", "wgrad_last_pixel", "stats_last_pixel"):
        assert cis
    resolved = 0
    for ci in cis:
        for mut, true, _ in _mutate(mutant, _case("dyadic", shape, ci), shape):
            assert _differs(mut, true), (shape, mutant, ci, "dyadic")
        o = _case("random", shape, ci)
        if _one_term(mutant, o, shape) > RESOLVE_K:
            continue
        resolved += 1
        for mut, true, bound in _mutate(mutant, o, shape):
            assert _beyond(mut, true, bound), (shape, mutant, ci, "random")
    assert resolved or not cis


@pytest.mark.parametrize("which", (1, 2), ids=["m", "l"])
@pytest.mark.parametrize("operand", ("x", "w"))
@pytest.mark.parametrize("shape", ("S1", "S3", "S4b"))
def test_plane_mutants(shape, operand, which):
    """a forward / data gradient / weight gradient that loses the m or the l plane of its three-plane operand (x, dy: the planes3x
    arm; the weights, and x of the weight gradient: the planes3w arm) differs in bits from the true reference -- and with random
    operands stays inside (K + 2) u sum|a b|, so only the planes3 family can see it: a lost l plane is an error of about
    2^-17 / sqrt(K) of sum|a b| against the bound's (K + 2) 2^-24, inside from K = 576 on (asserted).  A lost m plane is 2^-9 / sqrt(K) of
    sum|a b|: it meets the bound near K = 1024 and, on the small maps used here (few taps inside the image, so few real terms),
    still sticks out of it at K = 4608 -- nothing is asserted about it in the random family"""
    H, W, imgs = RR.SHAPES[shape][:3]
    family = "planes3x" if operand == "x" else "planes3w"
    for ci in (1, 6, 11, 16, 7):        # one 3x3 conv per width and a 1x1 downsample
        o = _case(family, shape, ci)
        c, w = o["c"], o["w"]
        if operand == "x":
            muts = [(RR.fwd(RR.drop_plane(o["x"], which), w, c), o["y"]),
                    (RR.written(RR.dgrad(RR.drop_plane(o["dy"], which), w, c), c), o["dx"]),
                    (RR.wgrad(o["xw"], RR.drop_plane(o["dyw"], which), c), o["dw"])]
        else:
            wm = RR.drop_plane(w, which)
            muts = [(RR.fwd(o["x"], wm, c), o["y"]), (RR.written(RR.dgrad(o["dy"], wm, c), c), o["dx"]),
                    (RR.wgrad(RR.drop_plane(o["xw"], which), o["dyw"], c), o["dw"])]
        for k, (mut, true) in enumerate(muts):
            assert _differs(mut, true), (shape, operand, which, c["name"], k)
        # the same loss on random operands against the random bound
        r = _case("random", shape, ci)
        w = r["w"]
        if operand == "x":
            muts = [(RR.fwd(RR.drop_plane(r["x"], which), w, c), r["y"], RR.dot_bound(c["Kw"], r["ya"]), c["Kw"]),
                    (RR.wgrad(r["xw"], RR.drop_plane(r["dyw"], which), c), r["dw"], RR.dot_bound(imgs * c["hout"] * c["wout"], r["dwa"]),
                     imgs * c["hout"] * c["wout"])]
        else:
            muts = [(RR.fwd(r["x"], RR.drop_plane(w, which), c), r["y"], RR.dot_bound(c["Kw"], r["ya"]), c["Kw"])]
        for mut, true, bound, K in muts:
            if which == 2 and K >= 576:
                assert not _beyond(mut, true, bound), (shape, operand, which, c["name"], K)
