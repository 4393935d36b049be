"""numpy restatement of the client-drift correction (include/fedmlp_hip_drift.h, fedmlp_amd/csrc/drift.hip), operation for
operation, and of SCAFFOLD's bookkeeping (fedmlp_amd/drift.py).  Every array operation below is one IEEE operation per element in
the arrays' dtype: with float32 inputs it is the kernel's arithmetic (each product and each sum rounded on its own), with float64
inputs it is the exact-enough form the property tests use."""
import numpy as np


def correct(g, p=None, a=None, mu=0.0, s=None):
    """r = g; mu != 0: d = p - a, m = mu * d, r = r + m; shift: r = r + s"""
    g = np.asarray(g)
    dt = g.dtype.type
    r = g.copy()
    if mu != 0.0:
        d = np.asarray(p, g.dtype) - np.asarray(a, g.dtype)
        m = dt(mu) * d
        r = r + m
    if s is not None:
        r = r + np.asarray(s, g.dtype)
    return r


def track(S, g):
    """S = S + g, the raw gradient"""
    return np.asarray(S) + np.asarray(g, np.asarray(S).dtype)


def mean(S, K):
    """S / (float)K, one division per element; zeros when no step was taken"""
    S = np.asarray(S)
    return np.zeros_like(S) if K == 0 else S / S.dtype.type(K)


def option_ii(c_i, c, x, y, K, eta):
    """SCAFFOLD's option II for the new client control variate: c_i - c + (x - y) / (K eta)"""
    return c_i - c + (x - y) / (K * eta)


class ScaffoldRef:
    """fedmlp_amd.drift.Scaffold's state on the host: c_global, c_local[i]; shift / end / server_update in the arrays' dtype"""

    def __init__(self, n_params, n_clients, dtype=np.float32):
        self.n_clients = n_clients
        self.c_global = np.zeros(n_params, dtype)
        self.c_local = {}

    def _local(self, i):
        return self.c_local.setdefault(i, np.zeros_like(self.c_global))

    def shift(self, i):
        return self.c_global - self._local(i)

    def end(self, i, mean_grad):
        new = np.asarray(mean_grad, self.c_global.dtype)
        delta = new - self._local(i)
        self.c_local[i] = new
        return delta

    def server_update(self, deltas):
        total = np.zeros_like(self.c_global)
        for d in deltas:
            total = total + d
        self.c_global = self.c_global + total / self.c_global.dtype.type(self.n_clients)
        return self.c_global
