"""Aggregation: the reference's utils/FedAvg.py surface + its RCCL form.

Two forms of the same arithmetic:
  * FedAvg / FedAvg_tao / FedAvg_proto / FedAvg_rela -- drop-ins with the reference signatures
    (utils/FedAvg.py:7-14, 51-70, 72-93, 95-103) for a single-process driver that holds
    every client's state_dict on the host, as main.py:216-234 does.  Host glue:
    left-to-right weighted mean, same order as the reference.
  * Fed_w / model_dist / RSCFed -- the `--exp RSCFed` aggregation (utils/FedAvg.py:16-49, main.py:213-214): host drop-ins
    with the reference's signatures and roundings, and rscfed_device, the same aggregation over engine-layout device
    states (fm_state_dist + fm_fed_w), which RSCFed itself takes when it is handed DeviceState clients.
  * fedavg_allreduce / tao_allreduce / proto_allreduce -- one client per GPU:
    each rank pre-scales its device-resident state by n_i/sum(n) (HIP kernel) and
    the sum is an RCCL all-reduce over xGMI (torch.distributed backend "nccl");
    on CPU test rigs the same code runs over gloo tensors.
"""
import copy
import logging
import math
from collections import OrderedDict

import numpy as np
import torch


def _np(v):
    return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)


def FedAvg(w, dict_len):
    """utils/FedAvg.py:7-14: sample-count weighted mean of EVERY state_dict entry,
    accumulated left to right in the entry's dtype; the int64 counter becomes
    float through the true division (and is truncated again on load)."""
    out = OrderedDict()
    for k in w[0].keys():
        acc = _np(w[0][k]) * dict_len[0]
        for i in range(1, len(w)):
            acc = acc + _np(w[i][k]) * dict_len[i]
        if np.issubdtype(acc.dtype, np.integer):
            acc = (acc / float(sum(dict_len))).astype(np.float32)
        else:
            acc = (acc / np.float32(sum(dict_len))).astype(np.float32)
        out[k] = torch.from_numpy(np.ascontiguousarray(acc))
    return out


def _is_int(a):
    return np.issubdtype(np.asarray(a).dtype, np.integer)


def Fed_w(w, weight):
    """utils/FedAvg.py:16-23: ((w0*wt0 + w1*wt1) + ...) / sum(weight), left to right in fp32.  A Python-float weight is
    rounded to fp32 once (torch's tensor * scalar), every product and sum is rounded separately, and the divisor is
    float32(sum(weight)) with Python's sum (in double for float weights).  An int64 entry (num_batches_tracked) stays
    integer under int weights until the true division makes it fp32, and is fp32 from the first product under float ones."""
    ints = all(isinstance(x, (int, np.integer)) for x in weight)
    tot = np.float32(sum(weight))
    out = OrderedDict()
    for k in w[0].keys():
        vs = [_np(wi[k]) for wi in w]
        if _is_int(vs[0]) and ints:
            acc = vs[0] * int(weight[0])
            for i in range(1, len(w)):
                acc = acc + vs[i] * int(weight[i])
            acc = acc.astype(np.float32)
        else:
            acc = vs[0].astype(np.float32) * np.float32(weight[0])
            for i in range(1, len(w)):
                acc = acc + vs[i].astype(np.float32) * np.float32(weight[i])
        out[k] = torch.from_numpy(np.ascontiguousarray((acc / tot).astype(np.float32)))
    return out


def _entry_norm(a, b):
    """|| a - b ||_2 as fm_state_dist forms it: the difference in fp32 (torch's), squares and sum in fp64, one rounding."""
    d = (np.asarray(a).astype(np.float32) - np.asarray(b).astype(np.float32)).astype(np.float64).reshape(-1)
    return np.float32(np.sqrt(np.dot(d, d)))


def _dist_sum(terms):
    """model_dist's accumulation: dist_total is an fp32 tensor, every term is added in turn."""
    tot = np.float32(0.0)
    for t in terms:
        tot = np.float32(tot + np.float32(t))
    return float(tot)


def _dist_rows(terms):
    """_dist_sum of every row of an fp32 [rows, terms] array: add.accumulate is r[i] = r[i - 1] + t[i], each sum rounded to
    fp32, the same left-to-right chain."""
    return [float(v) for v in np.add.accumulate(np.asarray(terms, dtype=np.float32), axis=1, dtype=np.float32)[:, -1]]


def model_dist(w_1, w_2):
    """utils/FedAvg.py:43-49: the fp32 sum over keys, in key order, of norm(w_1[k] - w_2[k]); int64 entries take part as
    fp32 values.  (torch.norm sums its squares in fp32 in an order of its own; here they are summed in fp64, so the two
    agree to fp32 rounding, not bit for bit.)"""
    assert w_1.keys() == w_2.keys(), "Error: cannot compute distance between dict with different keys"
    return _dist_sum(_entry_norm(_np(w_1[k]), _np(w_2[k])) for k in w_1)


def _rscfed_weights(ids, dict_len, dists):
    """utils/FedAvg.py:29-38 in double: a = n_id / N_group, b = exp(-0.01 * dist / n_id)."""
    n_total = 0
    for i in ids:
        n_total += dict_len[i]
    return [dict_len[i] / n_total * math.exp((-0.01) * (d / dict_len[i])) for i, d in zip(ids, dists)]


class DeviceState:
    """One client's result kept on the GPU: the engine-layout state (`engine.state_tensor().clone()`) and its
    num_batches_tracked counters.  RSCFed takes the device path when every client is one of these."""

    def __init__(self, engine, tensor, counters):
        self.engine, self.tensor = engine, tensor
        self.counters = np.asarray(counters)

    @classmethod
    def capture(cls, engine):
        return cls(engine, engine.state_tensor().clone(), engine.counters())


def rscfed_device(engine, states, counters, DMA, dict_len):
    """RSCFed (utils/FedAvg.py:25-41) over engine-layout device states, one tensor per client, and their [n_clients, ni]
    int64 counters.  Per group: one fm_state_dist against the group's own mean (never stored), ONE device-to-host read (the
    [K, n_entries] norms), the weights on the host in double -- each distance the fp32 sum, in key order, of a row of norms
    and of the counters' terms |float32(nbt_id) - mean_nbt| -- and one fm_fed_w; then a final fm_fed_w with [1]*M.
    Returns (device state, float counters [ni]); the counters are truncated on load as for FedAvg."""
    from . import spec
    M = len(DMA)
    assert 1 <= M <= 16, "rscfed_device: the final fold takes at most FM_FOLD_MAX = 16 groups"
    counters = np.asarray(counters)
    is_f32 = np.array([dt == "f32" for _, _, dt in spec.entries(engine.model, engine.n_classes)])
    subs = [torch.empty_like(states[0]) for _ in range(M)]
    sub_cnt = []
    for g, group in enumerate(DMA):
        ids = list(group)
        K = len(ids)
        sel = [states[i] for i in ids]
        cnt = counters[ids].astype(np.int64)                              # [K, ni]
        mean_cnt = cnt.sum(axis=0).astype(np.float32) / np.float32(K)     # Fed_w(.., [1]*K) of an int64 entry
        terms = np.empty((K, is_f32.size), np.float32)                    # model_dist's terms in key order
        terms[:, ~is_f32] = np.abs(cnt.astype(np.float32) - mean_cnt[None, :])
        terms[:, is_f32] = engine.state_dist(sel).cpu().numpy()           # the group's one device-to-host read
        dists = _dist_rows(terms)
        wts = _rscfed_weights(ids, dict_len, dists)
        engine.fed_w(sel, wts, subs[g])
        acc = cnt[0].astype(np.float32) * np.float32(wts[0])
        for r in range(1, K):
            acc = acc + cnt[r].astype(np.float32) * np.float32(wts[r])
        sub_cnt.append((acc / np.float32(sum(wts))).astype(np.float32))
    out = torch.empty_like(states[0])
    engine.fed_w(subs, [1] * M, out)
    acc = sub_cnt[0] * np.float32(1)
    for g in range(1, M):
        acc = acc + sub_cnt[g] * np.float32(1)
    return out, (acc / np.float32(M)).astype(np.float32)


def RSCFed(DMA, w_locals, K, dict_len, M):
    """utils/FedAvg.py:25-41 (main.py:213-214).  state_dicts: the host path, the reference's arithmetic.  DeviceState
    clients of one engine: rscfed_device, and the result is a DeviceState with float counters."""
    if len(w_locals) and all(isinstance(w, DeviceState) for w in w_locals):
        eng = w_locals[0].engine
        assert all(w.engine is eng for w in w_locals), "RSCFed: the device states belong to different engines"
        assert all(len(g) == K for g in DMA) and len(DMA) == M
        st, cnt = rscfed_device(eng, [w.tensor for w in w_locals], np.stack([w.counters for w in w_locals]), DMA, dict_len)
        return DeviceState(eng, st, cnt)
    w_sub = []
    for group in DMA:
        w_select = [w_locals[i] for i in group]
        w_avg = Fed_w(w_select, [1] * K)
        dists = [model_dist(w_locals[i], w_avg) for i in group]
        w_sub.append(Fed_w(w_select, _rscfed_weights(group, dict_len, dists)))
    return Fed_w(w_sub, [1] * M)


def FedAvg_tao(t, weight, class_active_client_list=None):
    """utils/FedAvg.py:51-70."""
    C = len(t[0])
    out = np.array([0.] * C)
    if class_active_client_list is None:
        for i, tao in enumerate(t):
            out += np.asarray(tao) * float(weight[i])
        return out / float(sum(weight))
    for cls, clients in enumerate(class_active_client_list):
        if len(clients) == 0:
            out[cls] = 1.
            continue
        wsum = 0.
        for i, tao in enumerate(t):
            if i in clients:
                out[cls] += tao[cls] * float(weight[i])
                wsum += float(weight[i])
        out[cls] = out[cls] / wsum
    return out


def FedAvg_proto(Prototypes, weight, class_active_client_list):
    """utils/FedAvg.py:72-93 (a class with no active client yields NaN rows)."""
    P = [torch.as_tensor(_np(p)) for p in Prototypes]
    out = torch.zeros((len(P[0]), len(P[0][0])))
    for cls, clients in enumerate(class_active_client_list):
        a0 = torch.zeros_like(P[0][0])
        a1 = torch.zeros_like(P[0][0])
        for cid in clients:
            a0 = P[cid][2 * cls] * weight[cid] + a0
            a1 = P[cid][2 * cls + 1] * weight[cid] + a1
        den = np.sum(np.array(weight)[clients])
        out[2 * cls] = a0 / den
        out[2 * cls + 1] = a1 / den
    return out


def FedAvg_rela(Prototypes, weight, class_active_client_list):
    """utils/FedAvg.py:95-103 (main.py:247, 251): row cls of the result is the weighted mean of the clients' relation-matrix
    rows over the clients that annotate cls, accumulated in the listed order as `row * weight + acc` in fp32 and divided by
    numpy's sum of their weights: the reference's operations on host tensors, bit for bit.  A class nobody annotates yields a
    NaN row (0 / 0) as there."""
    P = [torch.as_tensor(_np(p)) for p in Prototypes]
    out = torch.zeros((len(P[0]), len(P[0][0])))
    for cls, clients in enumerate(class_active_client_list):
        acc = torch.zeros_like(P[0][0])
        for cid in clients:
            acc = P[cid][cls] * weight[cid] + acc
        acc = acc / np.sum(np.array(weight)[clients])
        out[cls] = acc
    return out


# ---- one client per GPU: RCCL --------------------------------------------------------
_log = logging.getLogger("fedmlp_amd.fedavg")
_warned_fallback = False


def _dist():
    import torch.distributed as dist
    return dist if (dist.is_available() and dist.is_initialized()) else None


def allreduce_weighted_(tensor, w):
    """tensor <- sum_ranks(w_rank * tensor_rank), in place (tensor on any device)."""
    tensor.mul_(w)
    d = _dist()
    if d is not None and d.get_world_size() > 1:
        d.all_reduce(tensor, op=d.ReduceOp.SUM)
    return tensor


def trunc_counters(cnt_float):
    """float num_batches_tracked means -> the int64 counters load_state_dict leaves (utils/FedAvg.py:13): truncated, the 1e-9
    keeping a mean that rounded just below its integer"""
    return np.trunc(np.asarray(cnt_float, np.float64) + 1e-9).astype(np.int64)


def gather_dicts(dist, mine):
    """{client: value} of this rank -> the merged dict of every rank, on every rank (all_gather_object); dist None: one rank,
    the identity"""
    if dist is None:
        return mine
    parts = [None] * dist.get_world_size()
    dist.all_gather_object(parts, mine)
    return {k: v for part in parts for k, v in part.items()}


def comm_init(engine):
    """Create the library's own RCCL communicator (fm_comm_init) over the ranks of the current
    torch.distributed job: rank 0 draws the ncclUniqueId, torch.distributed only carries those
    128 bytes.  Returns the communicator's rank count."""
    d = _dist()
    if d is None or d.get_world_size() == 1:
        return 1
    # Every rank must end up on the SAME path (library communicator or torch.distributed fallback), so failures are
    # agreed on: rank 0 ships None when it cannot draw an id, and after fm_comm_init the ranks take the minimum of
    # their success flags; if any rank failed, those that succeeded drop their communicator and all of them raise.
    # (0) non-collective preflight, agreed on before any rank enters ncclCommInitRank: a rank that cannot load librccl
    # would otherwise leave its peers blocked inside the collective init, never reaching the agreement below
    pre = None
    try:
        engine.comm_preflight()
    except Exception as ex:                                  # noqa: BLE001
        pre = ex
    ok0 = torch.tensor([0 if pre is not None else 1], dtype=torch.int32, device=engine.device)
    d.all_reduce(ok0, op=d.ReduceOp.MIN)
    if int(ok0.item()) == 0:
        raise RuntimeError(f"fm_comm_preflight failed on at least one rank ({pre})")
    box = [None]
    if d.get_rank() == 0:
        try:
            box = [engine.comm_unique_id()]
        except Exception:                                    # noqa: BLE001
            box = [None]
    d.broadcast_object_list(box, src=0)
    if box[0] is None:
        raise RuntimeError("fm_comm_unique_id failed on rank 0")
    err = None
    try:
        engine.comm_init(box[0], d.get_rank(), d.get_world_size())
    except Exception as ex:                                  # noqa: BLE001
        err = ex
    ok = torch.tensor([0 if err is not None else 1], dtype=torch.int32, device=engine.device)
    d.all_reduce(ok, op=d.ReduceOp.MIN)
    if int(ok.item()) == 0:
        if err is None:
            engine.comm_destroy()
        raise RuntimeError(f"fm_comm_init failed on at least one rank ({err})")
    return engine.comm_size()


def fedavg_allreduce(engine, w):
    """FedAvg of the device-resident model over all ranks: state <- sum_i w_i state_i with
    w_i = n_i / sum(n).  With a library communicator (comm_init) the pre-scale, the
    ncclAllReduce of the arena and the counter mean all run inside the C ABI on the engine's
    stream (fm_fedavg_allreduce); otherwise the sum goes through torch.distributed."""
    if engine.comm_size() >= 1:
        engine.fedavg_allreduce(float(w))
        return engine.state_tensor()
    d = _dist()
    engine.state_scale(float(w))
    st = engine.state_tensor()
    if d is not None and d.get_world_size() > 1:
        global _warned_fallback
        if not _warned_fallback:
            # a caller that skipped comm_init (or whose comm_init failed) gets a DIFFERENT path from the one bench.py / driver.py
            # insist on: say so once
            _warned_fallback = True
            _log.warning("fedavg_allreduce: no library RCCL communicator (fm_comm_init was not called or failed): the all-reduce "
                         "of the state goes through torch.distributed (%s) instead of fm_fedavg_allreduce", d.get_backend())
        d.all_reduce(st, op=d.ReduceOp.SUM)
        engine.state_tensor()                 # marks the engine's derived buffers (BN folds, weight packs) stale
        cnt = torch.from_numpy(engine.counters().astype(np.float64) * float(w)).to(st.device)
        d.all_reduce(cnt, op=d.ReduceOp.SUM)
        engine.counters(np.trunc(cnt.cpu().numpy() + 1e-9).astype(np.int64))
    return st


def state_agreement(engine):
    """After a FedAvg every rank must hold the SAME state (utils/FedAvg.py:7-14 hands one w_glob to every client, main.py:216-222).
    Three checksums of the device arena -- the sum of its bit patterns as integers (any flipped bit moves it), the float64 sum and
    the float64 sum of magnitudes -- are compared across ranks with ONE extra all-reduce: returns (agree, worst) where worst is the
    largest difference between the ranks' checksums, relative to the magnitude sum.  A world of one agrees by definition.
    The first multi-GPU run of bench.py / driver.py is therefore also a correctness run of the RCCL path."""
    d = _dist()
    if d is None or d.get_world_size() <= 1:
        return True, 0.0
    st = engine.state_tensor()
    bits = st.view(torch.int32).to(torch.int64).sum().to(torch.float64)
    s1 = st.to(torch.float64).sum()
    s2 = st.to(torch.float64).abs().sum()
    v = torch.stack([bits, s1, s2, -bits, -s1, -s2])
    d.all_reduce(v, op=d.ReduceOp.MAX)                 # max(x) and max(-x) = -min(x) in one collective
    v = v.cpu().numpy()
    spread = v[:3] + v[3:]                             # max - min of each checksum over the ranks
    scale = max(abs(float(v[2])), 1e-30)
    worst = float(max(spread[1], spread[2]) / scale)
    return bool(spread[0] == 0.0 and spread[1] == 0.0 and spread[2] == 0.0), worst


def tao_allreduce(t, n_i, is_negative_client_mask, device="cpu", engine=None):
    """FedAvg_tao over ranks: t[C] local, mask[c] = 1 if this client has class c missing
    (it is in class_negative_client_list[c], main.py:206-210, 223)."""
    if engine is not None and engine.comm_size() >= 1:
        return engine.fedavg_tao(t, n_i, is_negative_client_mask)
    m = np.asarray(is_negative_client_mask, dtype=np.float64)
    buf = torch.from_numpy(np.concatenate([np.asarray(t, np.float64) * n_i * m, n_i * m])).to(device)
    d = _dist()
    if d is not None and d.get_world_size() > 1:
        d.all_reduce(buf, op=d.ReduceOp.SUM)
    buf = buf.cpu().numpy()
    C = len(m)
    num, den = buf[:C], buf[C:]
    return np.where(den == 0, 1.0, num / np.where(den == 0, 1.0, den))


def proto_allreduce(proto, n_i, is_active_client_mask, device="cpu", engine=None):
    """FedAvg_proto over ranks: proto[2C,D] local, mask[c] = 1 if this client annotates c."""
    if engine is not None and engine.comm_size() >= 1:
        return torch.from_numpy(engine.fedavg_proto(_np(proto), n_i, is_active_client_mask))
    m = np.repeat(np.asarray(is_active_client_mask, dtype=np.float32), 2)[:, None]
    P = np.asarray(_np(proto), dtype=np.float32) * (np.float32(n_i) * m)     # NaN rows of an active class propagate
    num = torch.from_numpy(np.where(m > 0, P, 0.0).astype(np.float32)).to(device)
    den = torch.from_numpy((np.float32(n_i) * m[:, 0]).astype(np.float32)).to(device)
    d = _dist()
    if d is not None and d.get_world_size() > 1:
        d.all_reduce(num, op=d.ReduceOp.SUM)
        d.all_reduce(den, op=d.ReduceOp.SUM)
    with np.errstate(invalid="ignore", divide="ignore"):
        return torch.from_numpy(num.cpu().numpy() / den.cpu().numpy()[:, None])   # 0/0 -> NaN


# ---- CBAFed's host arithmetic (main.py:273-316) ---------------------------------------
def cbafed_tao(class_num_lists, data_nums):
    """main.py:289-300: pt = sum_clients class_num_list / sum_clients data_num (fp32 tensors, as there), the unbiased
    standard deviation of pt over the classes, tao = clip(pt + 0.45 - std, 0.55, 0.95).  -> (pt, tao), fp32 tensors [C]."""
    c_num = torch.zeros(len(class_num_lists[0]))
    d_num = 0
    for cn, dn in zip(class_num_lists, data_nums):
        c_num += torch.as_tensor(cn, dtype=torch.float32)
        d_num += dn
    pt = c_num / d_num
    avg_pt = pt.sum() / len(pt)
    std_pt = torch.sqrt((1 / (len(pt) - 1)) * (((pt - avg_pt) ** 2).sum()))
    tao = pt + 0.45 - std_pt
    tao = torch.where(tao > 0.95, 0.95, tao)
    tao = torch.where(tao < 0.55, 0.55, tao)
    return pt, tao


def cbafed_blend(rnd, warmup):
    """The residual blend of main.py:274-288 (warm-up) and :301-316 (stage 2) at round `rnd`:
    -> (w_new, w_res, store): the round's global model is w_new * FedAvg + w_res * res (w_res = 0: the plain FedAvg, res
    not read), and store says whether it then becomes the new res.  Warm-up: every 5th round blends 0.2 / 0.8, round 0
    only stores; stage 2: every 5th round after its first blends 0.5 / 0.5, the first (rnd == warmup) only stores."""
    k, w = (rnd, 0.2) if rnd < warmup else (rnd - warmup, 0.5)
    if k % 5 != 0:
        return 1.0, 0.0, False
    if k == 0:
        return 1.0, 0.0, True
    return w, 1.0 - w, True


# ---- RoFL's server step (main.py:98-99, 253-268) ----------------------------------------
def rofl_centroids(f_G, f_locals):
    """The global centroids after a round: per row r, w_i = cos(f_G[r], f_k_i[r]) (torch's CosineSimilarity), then
    f_G[r] <- sum_i w_i f_k_i[r] / sum_i w_i, a zero weight sum dividing by 1.  The weights may be negative, as in the
    reference.  fp32 torch tensors [2C, D] on one device; f_G is not modified."""
    sim = torch.nn.CosineSimilarity(dim=1)
    f_G = torch.as_tensor(f_G, dtype=torch.float32)
    tmp = torch.zeros_like(f_G)
    w_sum = torch.zeros((f_G.shape[0], 1), dtype=torch.float32, device=f_G.device)
    for f in f_locals:
        f = torch.as_tensor(f, dtype=torch.float32).to(f_G.device)
        w = sim(f_G, f).reshape(-1, 1)
        w_sum = w_sum + w
        tmp = tmp + w * f
    return tmp / torch.where(w_sum == 0, torch.ones_like(w_sum), w_sum)


def consistency_weight(rnd, begin, end):
    """get_current_consistency_weight(rnd, args.begin, args.end) (utils/FedNoRo.py:72-81): the
    sigmoid ramp-up main.py:127-128 multiplies by args.a to get train_FedNoRo's weight_kd."""
    cur = float(np.clip(rnd, begin, end))
    phase = 1.0 - (cur - begin) / (end - begin)
    return float(np.exp(-5.0 * phase * phase))
