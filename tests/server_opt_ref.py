"""The server optimizers' rule (include/fedmlp_hip_server.h) restated in numpy: np.float32 scalars and arrays only, one rounded
operation per line.  Written from the header's statement, independently of fedmlp_amd/server_opt.py.

    step(rule, x, a, m, v, lr, beta1, beta2, tau) -> (x', m', v')        v, v' None for "avgm"
    init(rule, n, tau)                            -> (m, v) of a fresh install

x, a, m, v: float32 arrays of one shape (the parameters only: buffers are the caller's business, x' = a there)."""
import numpy as np

F = np.float32
RULES = ("avgm", "adagrad", "adam", "yogi")


def init(rule, n, tau):
    m = np.zeros(n, F)
    if rule == "avgm":
        return m, None
    t = F(tau)
    return m, np.full(n, t * t, F)


def step(rule, x, a, m, v, lr, beta1, beta2=0.0, tau=0.0):
    assert rule in RULES
    for arr in (x, a, m) + (() if rule == "avgm" else (v,)):
        assert arr.dtype == F
    lr, b1, b2, tau = F(lr), F(beta1), F(beta2), F(tau)
    d = a - x
    if rule == "avgm":
        t = b1 * m
        m = t + d
        t = lr * m
        return x + t, m, None
    omb1 = F(1.0) - b1
    omb2 = F(1.0) - b2
    t = b1 * m
    u = omb1 * d
    m = t + u
    q = d * d
    if rule == "adagrad":
        v = v + q
    elif rule == "adam":
        t = b2 * v
        u = omb2 * q
        v = t + u
    else:
        w = v - q
        s = np.where(w > 0, F(1.0), np.where(w < 0, F(-1.0), F(0.0))).astype(F)
        u = omb2 * q
        u = u * s
        v = v - u
    r = np.sqrt(v)
    r = r + tau
    t = lr * m
    t = t / r
    out = x + t
    assert out.dtype == F and m.dtype == F and v.dtype == F
    return out, m, v


def delta_norm(x, a):
    """float64 norm of the fp32 differences"""
    d = (a - x).astype(np.float64)
    return float(np.sqrt(np.sum(d * d)))
