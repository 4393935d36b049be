"""The RSCFed aggregation on the GPU (utils/FedAvg.py:16-49): fm_state_dist (the per-entry terms of model_dist), fm_fed_w
(Fed_w with double weights) and fedavg.rscfed_device, against numpy mirrors of the reference's arithmetic and the host drop-ins
that tests/test_rscfed_cpu.py pins on the reference.

Client states are built with POISONED padding: the engine's arena is first filled with per-client random values, then
fm_set_state writes the real elements and zeroes the padding inside the conv matrices; the gaps between matrices keep that
client's garbage.  A kernel that counts anything but state_dict elements fails the norm bounds.

Bounds: every norm within 2 fp32 ulps of sqrt(sum(float64(fp32 difference)^2)) formed on the host (the kernel's fp64 sums are
off by < 1e-9 relative whatever their order; the square root and one rounding to fp32 make <= 1 ulp; 2 allows for a host
sqrt / rounding tie on the other side).  Fed_w is bit-exact."""
import numpy as np
import pytest
import torch

from fedmlp_amd import fedavg, spec

pytestmark = pytest.mark.gpu

C_, HW = 5, 64
FOLD_MAX = 16
LENS = [5000, 4999, 37, 5000, 1, 2500, 5000, 123]          # test_fedavg_fold_of_eight_clients_into_the_engine_state's
DMA = [[0, 1, 2], [3, 4, 5], [6, 7, 0], [2, 4, 7]]
K_, M_ = 3, 4


class Clients:
    """n clients of `model`: device states with poisoned gaps, their state_dict-order host arrays and counters."""

    def __init__(self, eng, model, n, seed):
        self.eng, self.model = eng, model
        base, _ = spec.init_state(model, C_, 1037)
        rs = np.random.RandomState(seed)
        g = torch.Generator(device=eng.device).manual_seed(seed)
        self.states, self.flats, self.cnts = [], [], []
        for _ in range(n):
            st = eng.state_tensor()
            st.copy_(3.0 * torch.randn(st.shape, device=eng.device, generator=g) + 1.0)          # the poison
            flat = (base * (1.0 + 0.01 * rs.standard_normal(base.size))).astype(np.float32)
            cnt = rs.randint(0, 4, size=eng.ni).astype(np.int64)         # keeps model_dist / n of order 1 at n = 1
            eng.set_state(flat, cnt)
            self.states.append(eng.state_tensor().clone())
            self.flats.append(flat)
            self.cnts.append(cnt)
        self.names, self.slices = [], []
        off = 0
        for key, shape, dt in spec.entries(model, C_):
            if dt == "f32":
                n_el = int(np.prod(shape))
                self.names.append(key)
                self.slices.append(slice(off, off + n_el))
                off += n_el

    def state_dict(self, i):
        return spec.flat_to_state_dict(self.model, C_, self.flats[i], self.cnts[i])

    def want_norms(self, a, b):
        d = (a - b).astype(np.float32).astype(np.float64)
        return np.array([np.sqrt(np.dot(d[s], d[s])) for s in self.slices])

    def check_norms(self, got, a, b, what):
        want = self.want_norms(a, b)
        w32 = want.astype(np.float32)
        err = np.abs(got.astype(np.float64) - want)
        bad = err > 2.0 * np.spacing(w32).astype(np.float64)
        assert not bad.any(), (what, [(self.names[j], float(got[j]), float(want[j])) for j in np.nonzero(bad)[0][:5]])
        return want


def mean32(arrs):
    acc = arrs[0].copy()
    for a in arrs[1:]:
        acc = acc + a
    return acc / np.float32(len(arrs))


def fold32(arrs, wts):
    acc = arrs[0] * np.float32(wts[0])
    for a, w in zip(arrs[1:], wts[1:]):
        acc = acc + a * np.float32(w)
    return acc / np.float32(sum(wts))


@pytest.fixture(scope="module")
def eng():
    from fedmlp_amd.engine import Engine
    e = Engine("Resnet18", C_, HW, HW, 16)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cl(eng):
    return Clients(eng, "Resnet18", 8, 7)


def _named(cl, got, want, names):
    for nm in names:
        j = cl.names.index(nm)
        assert want[j] > 0 and abs(float(got[j]) - want[j]) <= 2 * float(np.spacing(np.float32(want[j]))), (nm, got[j], want[j])


SMALL = ["fc.bias", "bn1.weight", "bn1.running_var", "layer1.0.bn1.weight"]


def test_state_dist_against_an_explicit_reference(eng, cl):
    got = eng.state_dist(cl.states[:3], ref=cl.states[3]).cpu().numpy()
    assert got.shape == (3, len(cl.names)) and len(cl.names) == eng.n_float_entries == 102
    for k in range(3):
        want = cl.check_norms(got[k], cl.flats[k], cl.flats[3], f"client {k}")
        _named(cl, got[k], want, SMALL)
    assert cl.slices[cl.names.index("fc.bias")].stop - cl.slices[cl.names.index("fc.bias")].start == 5


def test_state_dist_against_the_group_mean(eng, cl):
    got = eng.state_dist(cl.states[:3]).cpu().numpy()
    b = mean32(cl.flats[:3])
    for k in range(3):
        want = cl.check_norms(got[k], cl.flats[k], b, f"client {k}")
        _named(cl, got[k], want, SMALL)
    # the poison is really there: over the whole arena the states differ far more than over the state_dict elements
    raw = float((cl.states[0] - cl.states[1]).double().norm())
    assert raw > 2 * float(np.sqrt(np.sum(cl.want_norms(cl.flats[0], cl.flats[1]) ** 2)))


def test_state_dist_limits(eng, cl):
    a = eng.state_dist(cl.states[:3])
    b = eng.state_dist(cl.states[:3])
    assert torch.equal(a, b)                                             # deterministic: no atomics
    one = eng.state_dist(cl.states[4:5], ref=cl.states[5]).cpu().numpy()
    cl.check_norms(one[0], cl.flats[4], cl.flats[5], "K = 1")
    assert float(eng.state_dist(cl.states[4:5]).abs().max()) == 0.0      # a state is its own mean
    ids = [i % 3 for i in range(FOLD_MAX)]
    got = eng.state_dist([cl.states[i] for i in ids]).cpu().numpy()      # K = FM_FOLD_MAX: the wide instantiation
    m = mean32([cl.flats[i] for i in ids])
    for k in range(3):
        cl.check_norms(got[k], cl.flats[k], m, f"K = 16, client {k}")
    np.testing.assert_array_equal(got[3:6], got[0:3])
    with pytest.raises(Exception):
        eng.state_dist([cl.states[i % 3] for i in range(FOLD_MAX + 1)])
    with pytest.raises(Exception):
        eng.state_dist(cl.states[:3], n_entries=len(cl.names) + 1)
    with pytest.raises(Exception):
        eng.state_dist(cl.states[:3], n_entries=len(cl.names) + eng.ni)


WTS = [0.2604923103919594, 0.8050278270130223, 0.5486993038355893, 0.014041700164018955]


def test_fed_w_is_bit_exact_over_the_whole_arena(eng, cl):
    assert np.float32(sum(WTS)) != np.float32(sum(float(np.float32(w)) for w in WTS))     # the divisors really differ
    hs = [s.cpu().numpy() for s in cl.states[:4]]
    want = fold32(hs, WTS)
    out = torch.empty_like(cl.states[0])
    eng.fed_w(cl.states[:4], WTS, out)
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    dst = cl.states[1].clone()                                           # out = an input
    eng.fed_w([cl.states[0], dst, cl.states[2], cl.states[3]], WTS, dst)
    np.testing.assert_array_equal(dst.cpu().numpy(), want)
    with pytest.raises(Exception):
        eng.fed_w([cl.states[i % 3] for i in range(FOLD_MAX + 1)], [1.0] * (FOLD_MAX + 1), out)


def test_fed_w_into_the_engine_state_rebuilds_derived_buffers(eng, cl):
    g = torch.Generator(device=eng.device).manual_seed(2)
    x = torch.randn((4, 3, HW, HW), device=eng.device, generator=g)
    eng.set_state(cl.flats[0], cl.cnts[0])
    eng.forward_eval(x)                                                  # derived buffers built for the old state
    eng.fed_w(cl.states[:4], WTS)                                        # out = the engine's state
    want = fold32([s.cpu().numpy() for s in cl.states[:4]], WTS)
    np.testing.assert_array_equal(eng.state_tensor().cpu().numpy(), want)
    f1, z1 = eng.forward_eval(x)
    flat, cnt = eng.get_state()
    eng.set_state(flat, cnt)
    f2, z2 = eng.forward_eval(x)
    assert torch.equal(z1, z2) and torch.equal(f1, f2)
    np.testing.assert_array_equal(flat, fold32(cl.flats[:4], WTS))


@pytest.fixture(scope="module")
def host_rscfed(cl):
    sds = [cl.state_dict(i) for i in range(8)]
    groups = []
    for ids in DMA:
        w_avg = fedavg.Fed_w([sds[i] for i in ids], [1] * K_)
        dists = [fedavg.model_dist(sds[i], w_avg) for i in ids]
        groups.append((dists, fedavg._rscfed_weights(ids, LENS, dists)))
    out = fedavg.RSCFed(DMA, sds, K_, LENS, M_)
    return groups, out


def _flat_of(cl, sd):
    fl = np.concatenate([sd[k].numpy().reshape(-1) for k in cl.names])
    cnt = np.array([float(v) for k, v in sd.items() if k.endswith("num_batches_tracked")])
    return fl, cnt


def test_rscfed_device_matches_the_host_aggregation(eng, cl, host_rscfed):
    """The weights differ from the host's only through norms that agree to ~1e-7 relative, entering as exp(-0.01 d / n) with
    d / n of order 1 (a few tens at n = 1): they move by less than an fp32 ulp, so the float entries agree to rtol 1e-6."""
    groups, want_sd = host_rscfed
    assert max(d / LENS[i] for ids, (dists, _) in zip(DMA, groups) for i, d in zip(ids, dists)) < 100
    want, want_cnt = _flat_of(cl, want_sd)
    st, cnt = fedavg.rscfed_device(eng, cl.states, np.stack(cl.cnts), DMA, LENS)
    assert cnt.dtype == np.float32 and cnt.shape == (eng.ni,)
    eng.state_tensor().copy_(st)
    got, _ = eng.get_state()
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=0)
    np.testing.assert_allclose(cnt, want_cnt, rtol=1e-6)
    np.testing.assert_array_equal(np.trunc(cnt), np.trunc(want_cnt))
    # the dispatch of the drop-in: DeviceState clients take the same path
    ds = [fedavg.DeviceState(eng, s, c) for s, c in zip(cl.states, cl.cnts)]
    res = fedavg.RSCFed(DMA, ds, K_, LENS, M_)
    assert isinstance(res, fedavg.DeviceState) and torch.equal(res.tensor, st)
    np.testing.assert_array_equal(res.counters, cnt)


def test_fed_w_with_the_hosts_weights_is_bit_exact(eng, cl, host_rscfed):
    groups, want_sd = host_rscfed
    want, _ = _flat_of(cl, want_sd)
    subs = []
    for ids, (_, wts) in zip(DMA, groups):
        subs.append(eng.fed_w([cl.states[i] for i in ids], wts, torch.empty_like(cl.states[0])))
    eng.fed_w(subs, [1] * M_)
    got, _ = eng.get_state()
    np.testing.assert_array_equal(got, want)


def test_efficientnet_b0_state_dist_and_fed_w():
    """EfficientNet-B0's entry table is built by other code: channel padding to 16 in every matrix, depthwise and
    squeeze-excite weights as their own layouts, odd-sized bias vectors."""
    from fedmlp_amd.engine import Engine
    e = Engine("Efficient_b0", C_, HW, HW, 8)
    try:
        c = Clients(e, "Efficient_b0", 4, 11)
        assert len(c.names) == e.n_float_entries
        got = e.state_dist(c.states[:3]).cpu().numpy()
        b = mean32(c.flats[:3])
        for k in range(3):
            c.check_norms(got[k], c.flats[k], b, f"mean, client {k}")
        got = e.state_dist(c.states[:3], ref=c.states[3]).cpu().numpy()
        for k in range(3):
            want = c.check_norms(got[k], c.flats[k], c.flats[3], f"ref, client {k}")
            for nm in ("_fc.bias", "_blocks.0._se_reduce.weight", "_blocks.0._depthwise_conv.weight", "_conv_stem.weight"):
                j = c.names.index(nm)
                assert want[j] > 0, nm
        assert torch.equal(e.state_dist(c.states[:3]), e.state_dist(c.states[:3]))
        out = torch.empty_like(c.states[0])
        e.fed_w(c.states, WTS, out)
        np.testing.assert_array_equal(out.cpu().numpy(), fold32([s.cpu().numpy() for s in c.states], WTS))
        e.state_tensor().copy_(out)
        flat, _ = e.get_state()
        np.testing.assert_array_equal(flat, fold32(c.flats, WTS))
    finally:
        e.close()
