"""The grouped data gradient of ResNet-18's stride-2 residual blocks on a real MI355X: ONE launch of the per-tap planes kernel
walks a job table (four parity classes of the 3x3 conv; the 1x1 downsample's gradient as extra K-steps of class (0,0)) --
against torch CPU autograd of conv3x3s2(x) + conv1x1s2(x), through the C ABI (fm_debug_block_dgrad).

Sizes: fm_create takes input sizes that are multiples of 32 only, so the input of every stride-2 conv is even (H / 4, H / 8,
H / 16): a size whose parity classes differ in their grids (72 -> 9 x 9 into layer3.0) is refused at fm_create and cannot be
tested through the engine."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fedmlp_amd import spec

pytestmark = pytest.mark.gpu

# (basic block, conv1, downsample) of layer2.0 / layer3.0 / layer4.0
BLOCKS = [(2, 5, 7), (4, 10, 12), (6, 15, 17)]


def _names():
    from tests.test_kernels_gpu import conv_names
    return conv_names()


def _nhwc(x_nchw):
    return x_nchw.permute(0, 2, 3, 1).contiguous()


def _operands(e, sd, blk, imgs, seed, dtype=torch.float32):
    """seeded dy1, dyd and the wanted dx = d/dx [sum(conv1(x) * dy1) + sum(downsample(x) * dyd)] in `dtype` on the CPU"""
    b, c1, ds = blk
    i1, i2 = e.debug_conv_info(c1), e.debug_conv_info(ds)
    assert (i1["k"], i1["stride"], i2["k"], i2["stride"]) == (3, 2, 1, 2)
    assert (i1["hout"], i1["wout"], i1["cout"]) == (i2["hout"], i2["wout"], i2["cout"])
    g = torch.Generator().manual_seed(seed)
    dy1 = torch.randn((imgs, i1["cout"], i1["hout"], i1["wout"]), generator=g)
    dyd = torch.randn((imgs, i2["cout"], i2["hout"], i2["wout"]), generator=g)
    w1 = torch.from_numpy(sd[_names()[c1] + ".weight"]).to(dtype)
    w2 = torch.from_numpy(sd[_names()[ds] + ".weight"]).to(dtype)
    x = torch.zeros((imgs, i1["cin"], i1["hin"], i1["win"]), dtype=dtype, requires_grad=True)
    y = (F.conv2d(x, w1, None, 2, 1) * dy1.to(dtype)).sum() + (F.conv2d(x, w2, None, 2, 0) * dyd.to(dtype)).sum()
    y.backward()
    return dy1, dyd, x.grad, i1


def _grouped(e, blk, dy1, dyd, info, imgs):
    dev = e.device
    dx = torch.full((imgs, info["hin"], info["win"], info["cin"]), float("nan"), device=dev)     # every element must be written
    e.debug_block_dgrad(blk[0], _nhwc(dy1).to(dev), _nhwc(dyd).to(dev), dx, imgs)
    return dx.cpu()


def check_block(e, sd, blk, imgs, seed):
    """_check_conv's data-gradient bound (tests/test_kernels_gpu.py): rtol 1e-4, atol 2e-5 x max|want|; and two calls on the
    same operands are bit-identical"""
    dy1, dyd, want, info = _operands(e, sd, blk, imgs, seed)
    got = _grouped(e, blk, dy1, dyd, info, imgs)
    again = _grouped(e, blk, dy1, dyd, info, imgs)
    scale = want.abs().max().item()
    err = (got.permute(0, 3, 1, 2) - want).abs().max().item()
    print(f"block {blk[0]} imgs {imgs} hin {info['hin']}: max|err| {err:.3e}, max|want| {scale:.3e}")
    np.testing.assert_allclose(got.permute(0, 3, 1, 2).numpy(), want.numpy(), rtol=1e-4, atol=2e-5 * scale,
                               err_msg=f"grouped dgrad of block {blk[0]}")
    assert torch.equal(got, again), "two grouped calls on the same operands differ"


@pytest.fixture(scope="module")
def eng64():
    from fedmlp_amd.engine import Engine
    e = Engine("Resnet18", 5, 64, 64, 8)
    flat, cnt = spec.init_state("Resnet18", 5, 1037)
    e.set_state(flat, cnt)
    yield e, spec.flat_to_state_dict("Resnet18", 5, flat, cnt)
    e.close()


@pytest.fixture(scope="module")
def eng224_forms():
    from fedmlp_amd.engine import Engine
    flat, cnt = spec.init_state("Resnet18", 5, 7)
    engs = {}
    for sp in (0, 9, 6):
        engs[sp] = Engine("Resnet18", 5, 224, 224, 4, products=sp)
        engs[sp].set_state(flat, cnt)
    yield engs, spec.flat_to_state_dict("Resnet18", 5, flat, cnt)
    for e in engs.values():
        e.close()


@pytest.mark.parametrize("blk", BLOCKS)
def test_grouped_dgrad_64(eng64, blk):
    e, sd = eng64
    assert e.planes
    check_block(e, sd, blk, imgs=6, seed=500 + blk[0])


@pytest.mark.parametrize("blk", BLOCKS)
def test_grouped_dgrad_224(eng224_forms, blk):
    engs, sd = eng224_forms
    for sp in (6, 9):
        check_block(engs[sp], sd, blk, imgs=3, seed=600 + blk[0])


@pytest.mark.parametrize("blk", BLOCKS)
def test_grouped_dgrad_is_fp32_accurate(eng224_forms, blk):
    """test_split_products_are_fp32_accurate's criterion: relative L2 error against float64 <= 1.25 x the error of the
    products = 0 handle (fp32 matrix pipe, its two conv_dgrad calls) on the same operands, and < 2e-6; SP = 6 and 9."""
    engs, sd = eng224_forms
    imgs = 3
    dy1, dyd, want, info = _operands(engs[0], sd, blk, imgs, 700 + blk[0], torch.float64)
    errs = {}
    for sp in (0, 9, 6):
        assert engs[sp].products == sp
        got = _grouped(engs[sp], blk, dy1, dyd, info, imgs).permute(0, 3, 1, 2).double()
        errs[sp] = ((got - want).norm() / want.norm()).item()
    print(f"block {blk[0]} relative L2 error vs float64: {errs}")
    for sp in (9, 6):
        assert errs[sp] <= 1.25 * errs[0] + 1e-9, (sp, errs)
        assert errs[sp] < 2e-6, (sp, errs)


def test_grouped_dgrad_forced_splits():
    """the same under forced grids (FM_IGEMM_BLOCKS is read once per process: a child each): ranges that cut tiles of every
    job, ranges that span jobs, more blocks than CUs asked for"""
    code = (
        "import sys; sys.path.insert(0, '.');"
        "import tests.test_pconv_group_gpu as T; from fedmlp_amd.engine import Engine; from fedmlp_amd import spec;"
        "e = Engine('Resnet18', 5, 64, 64, 8); flat, cnt = spec.init_state('Resnet18', 5, 1037);"
        "e.set_state(flat, cnt); sd = spec.flat_to_state_dict('Resnet18', 5, flat, cnt);"
        "[T.check_block(e, sd, b, 6, 800 + b[0]) for b in T.BLOCKS]; e.close();"
        "e = Engine('Resnet18', 5, 224, 224, 4); flat, cnt = spec.init_state('Resnet18', 5, 7);"
        "e.set_state(flat, cnt); sd = spec.flat_to_state_dict('Resnet18', 5, flat, cnt);"
        "[T.check_block(e, sd, b, 3, 900 + b[0]) for b in T.BLOCKS]; e.close(); print('ok')")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for nb in ("7", "61", "509"):
        env = dict(os.environ, FM_IGEMM_BLOCKS=nb)
        # (subprocess.run kills the child when the timeout expires; three children stay below the suite's 420-s bound per test)
        r = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "ok" in r.stdout, f"FM_IGEMM_BLOCKS={nb}: {r.stdout[-2000:]} {r.stderr[-3000:]}"
