"""Python handle over the C-ABI engine (include/fedmlp_hip.h).

torch is used for device memory and streams only (tensor.data_ptr() crosses the
ABI); all arithmetic on the path runs in the HIP library.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib, spec

MODEL_IDS = {"Resnet18": 0, "Efficient_b0": 1}
PRECISION_IDS = {"fp32": 0, "bf16": 1}
# fm_config.reserved[2]: None = the library default (six products unless FM_MFMA_SPLIT says otherwise), 0 = fp32 matrix pipe,
# 9 = all nine partial products, 6 = exactly six (an explicit request is not subject to the environment override)
PRODUCT_FORMS = {None: 0, 6: 3, 0: 1, 9: 2}


def _ptr(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous() and t.dtype in (torch.float32, torch.int32, torch.bfloat16), \
        (t.device, t.dtype, t.is_contiguous())
    return C.c_void_p(t.data_ptr())


def _cargs(args):
    return [_ptr(a) if torch.is_tensor(a) else a for a in args]


class RoflHeads:
    """The RoFL client's wrappers (include/fedmlp_hip_rofl.h), a base of Engine.  They go through Engine._step / Engine._head
    like every fused step and head, so a step bumps serial and weights_version and a head bumps serial."""

    def _rofl_args(self, item, B, centroids, pseudo):
        """-> (item, centroids, pseudo, N) as the C arguments.  centroids None passes a null pointer (the library refuses it)"""
        n, D = self.n_classes, self.feature_dim
        if tuple(item.shape) != (B,) or item.dtype != torch.int32 or not item.is_contiguous() or not item.is_cuda:
            raise ValueError(f"rofl: item must be a contiguous int32 [{B}] device tensor")
        if centroids is not None and (tuple(centroids.shape) != (2 * n, D) or centroids.dtype != torch.float32
                                      or not centroids.is_contiguous() or not centroids.is_cuda):
            raise ValueError(f"rofl: centroids must be a contiguous float32 [{2 * n}, {D}] device tensor")
        if pseudo.dim() != 2 or pseudo.shape[1] != n or pseudo.dtype != torch.uint8 or not pseudo.is_contiguous() \
                or not pseudo.is_cuda:
            raise ValueError(f"rofl: pseudo must be a contiguous uint8 [N, {n}] device tensor")
        return item, centroids, C.c_void_p(pseudo.data_ptr()), C.c_int64(pseudo.shape[0])

    def step_rofl(self, x, y, item, n_keep, pos_weight, lambda_cen_eff, lambda_e, write_labels, centroids, pseudo, loss_out):
        """train_RoFL's step (utils/local_training.py:516-574) fused: train forward, loss_rofl's head on the engine's logits and
        pooled feature, backward, Adam.  centroids [2C,D] float32 and pseudo [N,C] uint8 are DEVICE tensors of the caller's (the
        client's f_k and the round's pseudo-label table): the step reads and updates both, with no host read"""
        it, ce, ps, N = self._rofl_args(item, x.shape[0], centroids, pseudo)
        self._step(self.lib.fm_step_rofl, x.shape[0], x, y, it, x.shape[0], int(n_keep), _lib.fvec(pos_weight, self.n_classes),
                   C.c_float(lambda_cen_eff), C.c_float(lambda_e), int(bool(write_labels)), ce, ps, N, loss_out)

    def loss_rofl(self, z, feat, y, item, n_keep, pos_weight, lambda_cen_eff, lambda_e, write_labels, centroids, pseudo,
                  keep=None):
        """RoFL's head on caller tensors: z, y [B,C], feat [B,D] (forward_train's feature), item int32 [B]; see step_rofl.
        keep (optional int32 [B] device tensor) receives bit 0 = kept, bit 1 = mask"""
        B = y.shape[0]
        if tuple(feat.shape) != (B, self.feature_dim) or feat.dtype != torch.float32 or not feat.is_contiguous():
            raise ValueError(f"loss_rofl: feat must be a contiguous float32 [{B}, {self.feature_dim}] tensor")
        if keep is not None and (tuple(keep.shape) != (B,) or keep.dtype != torch.int32 or not keep.is_contiguous()):
            raise ValueError(f"loss_rofl: keep must be a contiguous int32 [{B}] tensor")
        it, ce, ps, N = self._rofl_args(item, B, centroids, pseudo)
        return self._head(self.lib.fm_loss_rofl, 1, z, y, None, z, feat, y, it, B, int(n_keep),
                          _lib.fvec(pos_weight, self.n_classes), C.c_float(lambda_cen_eff), C.c_float(lambda_e),
                          int(bool(write_labels)), ce, ps, N, tail=(keep,))


class Engine(RoflHeads):
    """One per process/GPU. Owns the device-resident model state, optimiser
    moments, teacher snapshot and activation workspaces for `max_images`."""

    def __init__(self, model, n_classes, in_h, in_w, max_images, device=None, precision="fp32", streams=0, products=None):
        """streams: fm_config.reserved[1] -- 0 the engine forks its side stream for the frozen teacher and the weight
        gradients (default, bit-identical to one stream), 1 one stream (per-kernel profiling), 2 teacher only.
        products: fm_config.reserved[2] -- how the fp32 conv GEMMs form their products, fixed for the handle: None = library
        default (six exact bf16 partial products per fp32 product on the bf16 matrix pipe), 0 = fp32 matrix pipe, 6, 9."""
        if not torch.cuda.is_available():
            raise RuntimeError("fedmlp_amd.Engine needs a GPU (no CPU fallback)")
        self.lib = _lib.load()
        self.model, self.n_classes = model, int(n_classes)
        self.in_h, self.in_w, self.max_images = int(in_h), int(in_w), int(max_images)
        if device is None:                       # the rank's own GPU, never a hard-coded cuda:0
            from .launch import default_device
            device = default_device()
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        self.precision = precision
        if precision != "fp32" and model != "Efficient_b0":
            raise ValueError("precision 'bf16' is built for Efficient_b0 only (BASELINE configs[4])")
        # the engine enqueues on torch's CURRENT stream of this device (0 = the null stream when it is the default one),
        # so its kernels are ordered with the torch ops around the calls
        self.stream = torch.cuda.current_stream(self.device).cuda_stream
        self.streams = int(streams)
        cfg = _lib.FmConfig(MODEL_IDS[model], self.n_classes, self.in_h, self.in_w,
                            self.max_images, (C.c_int32 * 3)(PRECISION_IDS[precision], self.streams,
                                                             PRODUCT_FORMS[products]),
                            C.c_void_p(self.stream) if self.stream else None)
        h = C.c_void_p()
        _lib.check(self.lib.fm_create(C.byref(cfg), C.byref(h)))
        self.h = h
        nf, ni = C.c_int64(), C.c_int64()
        _lib.check(self.lib.fm_state_sizes(self.h, C.byref(nf), C.byref(ni)))
        self.nf, self.ni = nf.value, ni.value
        assert (self.nf, self.ni) == spec.sizes(model, self.n_classes), \
            "engine and fedmlp_amd.spec disagree on the state_dict layout"
        self.feature_dim = spec.FEATURE_DIM[model]
        # what fm_create actually set up (it keeps one stream when the second buffer set does not fit in free memory)
        self.stream_mode = int(self.lib.fm_stream_mode(self.h))
        self.products = int(self.lib.fm_products(self.h))      # 0 fp32 matrix pipe, 6 / 9 bf16 partial products
        self.planes = bool(self.lib.fm_planes_mode(self.h))    # conv GEMMs read bf16 planes written by the producing kernels
        # Efficient_b0: draw drop-connect / dropout multipliers before every train step, like the
        # reference's model does inside net(images) in train mode.  Parity tests switch it off and
        # install their own draws with set_stochastic().
        self.stochastic = model == "Efficient_b0"
        self.stochastic_generator = None
        # serial: bumped by every call that enqueues work -- any of them may overwrite the activations a train-mode forward
        # saved (fm_forward_eval writes the feature the backward reads), so an autograd node whose forward is no longer the
        # engine's last call recomputes it (model.HipNet).  weights_version: bumped by every call that may change the
        # resident weights (steps, optimizer, set_state, FedAvg, a torch write through state_tensor()).
        self.serial = 0
        self.weights_version = 0

    def _enqueue(self, weights=False):
        self.serial += 1
        if weights:
            self.weights_version += 1

    def close(self):
        if getattr(self, "h", None):
            self.lib.fm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- EfficientNet-B0 training-time randomness ---------------------------------
    def set_stochastic(self, drop_connect=None, dropout=None):
        """Multipliers for the NEXT train steps (kept until replaced; None = no drop).
        drop_connect: cuda fp32 [16, imgs]; dropout: cuda fp32 [imgs, 1280] (include/fedmlp_hip.h)."""
        self._dc = None if drop_connect is None else drop_connect.contiguous().float()
        self._dr = None if dropout is None else dropout.contiguous().float()
        _lib.check(self.lib.fm_set_stochastic(self.h, _ptr(self._dc), _ptr(self._dr)))

    def draw_stochastic(self, imgs, generator=None):
        """One draw with efficientnet-pytorch's formulas (drop_connect_rate 0.2 scaled by
        idx/16, dropout 0.2) on the engine's device, installed for the next train step."""
        if self.model != "Efficient_b0":
            return
        dev = self.device
        u = torch.rand((16, imgs), device=dev, generator=generator)
        keep = 1.0 - 0.2 * torch.arange(16, device=dev, dtype=torch.float32).view(16, 1) / 16.0
        dc = torch.floor(keep + u) / keep
        dr = (torch.rand((imgs, 1280), device=dev, generator=generator) >= 0.2).float() / 0.8
        self.set_stochastic(dc, dr)

    # ---- state -----------------------------------------------------------------
    def set_state(self, flat, counters):
        flat = np.ascontiguousarray(flat, dtype=np.float32)
        counters = np.ascontiguousarray(counters, dtype=np.int64)
        assert flat.size == self.nf and counters.size == self.ni
        self._enqueue(weights=True)
        _lib.check(self.lib.fm_set_state(self.h, flat.ctypes.data_as(C.c_void_p),
                                         counters.ctypes.data_as(C.c_void_p)))

    def get_state(self):
        flat = np.empty(self.nf, np.float32)
        counters = np.empty(self.ni, np.int64)
        _lib.check(self.lib.fm_get_state(self.h, flat.ctypes.data_as(C.c_void_p),
                                         counters.ctypes.data_as(C.c_void_p)))
        return flat, counters

    def state_tensor(self):
        """torch view of the engine-layout device state (for the RCCL all-reduce)."""
        p, n = C.c_void_p(), C.c_int64()
        self._enqueue(weights=True)              # the caller may write the state through the view
        _lib.check(self.lib.fm_state_device(self.h, C.byref(p), C.byref(n)))
        return _device_view(p.value, n.value, self.device)

    def counters(self, new=None):
        c = np.zeros(self.ni, np.int64) if new is None else np.ascontiguousarray(new, dtype=np.int64)
        if new is not None:
            self._enqueue(weights=True)          # the counters are part of the resident state
        _lib.check(self.lib.fm_counters(self.h, c.ctypes.data_as(C.c_void_p), int(new is not None)))
        return c

    def state_scale(self, w):
        self._enqueue(weights=True)
        _lib.check(self.lib.fm_state_scale(self.h, C.c_float(w)))

    def fedavg_fold(self, states, dict_len, out=None):
        """FedAvg (utils/FedAvg.py:7-14) of K engine-layout device states on this GPU, reference order and roundings.
        states: list of cuda fp32 tensors of state_tensor()'s length; out: destination (default: the engine's own state)."""
        K = len(states)
        assert K == len(dict_len) and K >= 1
        for t in states:
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == self.state_tensor().numel()
        ptrs = (C.c_void_p * K)(*[t.data_ptr() for t in states])
        dst = self.state_tensor() if out is None else out
        self._check_stream()
        self._enqueue(weights=True)
        _lib.check(self.lib.fm_fedavg_fold(self.h, ptrs, _lib.fvec(dict_len, K), K, _ptr(dst)))
        return dst

    def _state_ptrs(self, states):
        K = len(states)
        assert K >= 1
        if getattr(self, "_ns", None) is None:
            self._ns = self.state_tensor().numel()
        for t in states:
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == self._ns
        return (C.c_void_p * K)(*[t.data_ptr() for t in states])

    def fed_w(self, states, weights, out=None):
        """Fed_w (utils/FedAvg.py:16-23) of K engine-layout device states: the fold with Python-float weights, each rounded
        to fp32 once, divided by float32(sum of the double weights).  out: destination (default: the engine's own state)."""
        K = len(states)
        assert K == len(weights)
        ptrs = self._state_ptrs(states)
        dst = self.state_tensor() if out is None else out
        assert dst.is_cuda and dst.dtype == torch.float32 and dst.is_contiguous() and dst.numel() == states[0].numel()
        self._check_stream()
        self._enqueue(weights=True)
        w = (C.c_double * K)(*[float(v) for v in weights])
        _lib.check(self.lib.fm_fed_w(self.h, ptrs, w, K, _ptr(dst)))
        return dst

    @property
    def n_float_entries(self):
        """fp32 entries of the state_dict (the columns of state_dist)."""
        if getattr(self, "_nfe", None) is None:
            self._nfe = sum(1 for _, _, dt in spec.entries(self.model, self.n_classes) if dt == "f32")
        return self._nfe

    def state_dist(self, states, ref=None, n_entries=None):
        """The terms of model_dist (utils/FedAvg.py:43-49) on the device: a cuda fp32 tensor [K, n_float_entries] of the L2
        norms of (states[k] - ref) per fp32 state_dict entry, in state_dict order, over the real elements of the engine
        layout only.  ref None: the states' own Fed_w(states, [1]*K) mean, formed in registers."""
        K = len(states)
        ptrs = self._state_ptrs(states)
        if ref is not None:
            assert ref.is_cuda and ref.dtype == torch.float32 and ref.is_contiguous() and ref.numel() == states[0].numel()
        ne = self.n_float_entries if n_entries is None else int(n_entries)
        norms = torch.empty((K, ne), device=self.device, dtype=torch.float32)
        self._check_stream()
        self._enqueue()
        _lib.check(self.lib.fm_state_dist(self.h, ptrs, K, _ptr(ref), _ptr(norms), ne))
        return norms

    def _check_stream(self):
        """The engine enqueues on the stream that was torch's current one when it was built (fm_config.stream is fixed for
        the handle's life: its workspaces are ordered on that stream).  A call made under another torch.cuda.stream(...)
        would race with the producers of its inputs, so it is refused."""
        cur = torch.cuda.current_stream(self.device).cuda_stream
        if cur != self.stream:
            raise RuntimeError(f"fedmlp_amd.Engine was built on stream {self.stream:#x} but torch's current stream is "
                               f"{cur:#x}: call the engine under the stream it was created on")

    def teacher_snapshot(self):
        self._enqueue()
        _lib.check(self.lib.fm_teacher_snapshot(self.h))

    def adam_reset(self, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-4):
        hp = _lib.FmAdam(lr, betas[0], betas[1], eps, weight_decay)
        self._enqueue()
        _lib.check(self.lib.fm_adam_reset(self.h, C.byref(hp)))

    def sync(self):
        _lib.check(self.lib.fm_sync(self.h))

    # ---- forward / steps -----------------------------------------------------------
    def forward_eval(self, x, teacher=False):
        B = x.shape[0]
        feat = torch.empty((B, self.feature_dim), device=self.device, dtype=torch.float32)
        logits = torch.empty((B, self.n_classes), device=self.device, dtype=torch.float32)
        return self.forward_eval_into(x, feat, logits, teacher)

    def forward_eval_into(self, x, feat, logits, teacher=False):
        """net(x) in eval mode into caller-owned [B,D] / [B,C] device buffers (no allocation)."""
        self._check_stream()
        self._enqueue()
        _lib.check(self.lib.fm_forward_eval(self.h, _ptr(x), x.shape[0], int(teacher), _ptr(feat), _ptr(logits)))
        return feat, logits

    # ---- RCCL inside the C-ABI library (utils/FedAvg.py:7-14, 51-93 across ranks) ---------
    def comm_preflight(self):
        """librccl loadable and complete on THIS rank (local; fm_comm_init is the collective step)."""
        _lib.check(self.lib.fm_comm_preflight())

    def comm_unique_id(self):
        buf = (C.c_uint8 * _lib.FM_COMM_ID_BYTES)()
        _lib.check(self.lib.fm_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, unique_id, rank, world):
        buf = (C.c_uint8 * _lib.FM_COMM_ID_BYTES)(*unique_id)
        _lib.check(self.lib.fm_comm_init(self.h, buf, int(rank), int(world)))

    def comm_destroy(self):
        _lib.check(self.lib.fm_comm_destroy(self.h))

    def comm_size(self):
        return int(self.lib.fm_comm_size(self.h))

    def fedavg_allreduce(self, w):
        """state <- sum_ranks w_rank * state_rank on the engine stream (ncclAllReduce in the library)."""
        self._enqueue(weights=True)
        _lib.check(self.lib.fm_fedavg_allreduce(self.h, C.c_float(w)))

    def fedavg_tao(self, t, n_i, negative_mask):
        n = self.n_classes
        tt = (C.c_double * n)(*[float(v) for v in t])
        out = (C.c_double * n)()
        _lib.check(self.lib.fm_fedavg_tao(self.h, tt, C.c_double(float(n_i)), _lib.fvec(negative_mask, n), out))
        return np.array(out[:], dtype=np.float64)

    def fedavg_proto(self, proto, n_i, active_mask):
        n, D = self.n_classes, self.feature_dim
        p = np.ascontiguousarray(proto, dtype=np.float32).reshape(2 * n, D)
        out = np.empty((2 * n, D), np.float32)
        _lib.check(self.lib.fm_fedavg_proto(self.h, p.ctypes.data_as(C.c_void_p), C.c_double(float(n_i)),
                                            _lib.fvec(active_mask, n), out.ctypes.data_as(C.c_void_p)))
        return out

    def _draw(self, imgs):
        if self.stochastic:
            self.draw_stochastic(imgs, self.stochastic_generator)

    def _step(self, fn, imgs, *args):
        """A fused step: fn is the caller's own self.lib.fm_step_*, imgs the images its forward draws stochastic depth for, args
        the C arguments (tensors as they are)"""
        self._check_stream()
        self._enqueue(weights=True)
        self._draw(imgs)
        _lib.check(fn(self.h, *_cargs(args)))

    def step_bce(self, x, y, pos_weight, bs_norm, loss_out):
        self._step(self.lib.fm_step_bce, x.shape[0], x, y, x.shape[0], _lib.fvec(pos_weight, self.n_classes),
                   int(bs_norm), loss_out)

    def step_stage1(self, x1, x2, y, active_mask, annotation_num, bs_norm, loss_out):
        self._step(self.lib.fm_step_stage1, 2 * x1.shape[0], x1, x2, y, x1.shape[0],
                   _lib.fvec(active_mask, self.n_classes), int(annotation_num), int(bs_norm), loss_out)

    def step_stage2(self, x, y, distill, loss_out):
        self._step(self.lib.fm_step_stage2, x.shape[0], x, y, distill, x.shape[0], loss_out)

    def step_fixmatch(self, xw, xs, y, pos_weight, pos_weight_unk, active_mask, annotation_num,
                      bs_norm, loss_out):
        n = self.n_classes
        self._step(self.lib.fm_step_fixmatch, 2 * xw.shape[0], xw, xs, y, xw.shape[0], _lib.fvec(pos_weight, n),
                   _lib.fvec(pos_weight_unk, n), _lib.fvec(active_mask, n), int(annotation_num), int(bs_norm), loss_out)

    def step_fedlsr(self, x1, x2, y, pos_weight, mix1, beta, loss_out):
        """train_FedLSR's step (utils/local_training.py:1294-1319) fused: two-view forward, loss_fedlsr's head, backward, Adam"""
        self._step(self.lib.fm_step_fedlsr, 2 * x1.shape[0], x1, x2, y, x1.shape[0],
                   _lib.fvec(pos_weight, self.n_classes), C.c_float(mix1), C.c_float(beta), loss_out)

    def step_rscfed(self, x1, x2, y, pos_weight, active_mask, annotation_num, bs_norm, w_teacher, w_student, loss_out):
        """train_RSCFed's step (utils/local_training.py:733-759) fused: teacher-slot eval forward of x2, train forward of x1,
        loss_rscfed's head, backward, Adam, then teacher = w_teacher teacher + w_student student over every state entry"""
        n = self.n_classes
        self._step(self.lib.fm_step_rscfed, x1.shape[0], x1, x2, y, x1.shape[0], _lib.fvec(pos_weight, n),
                   _lib.fvec(active_mask, n), int(annotation_num), int(bs_norm), C.c_float(w_teacher), C.c_float(w_student),
                   loss_out)

    def step_fednoro(self, x, y, active_mask, w_kd, loss_out):
        """train_FedNoRo's warm-up step (:143-160) fused: frozen teacher's eval forward and the train forward of the same x,
        loss_lakd's head, backward, Adam"""
        self._step(self.lib.fm_step_fednoro, x.shape[0], x, y, x.shape[0], _lib.fvec(active_mask, self.n_classes),
                   C.c_float(w_kd), loss_out)

    def _cbafed_args(self, tao, pos_weight, counts):
        """-> (tao, pos_weight, counts) as the C arguments"""
        n = self.n_classes
        if tuple(pos_weight.shape) != (n,) or pos_weight.dtype != torch.float32 or not pos_weight.is_contiguous() \
                or not pos_weight.is_cuda:
            raise ValueError(f"cbafed: pos_weight must be a contiguous float32 [{n}] device tensor")
        if counts is not None and (tuple(counts.shape) != (n + 1,) or counts.dtype != torch.int64
                                   or not counts.is_contiguous() or not counts.is_cuda):
            raise ValueError(f"cbafed: counts must be a contiguous int64 [{n + 1}] device tensor")
        if tao is not None and counts is None:
            raise ValueError("cbafed: stage 2 (tao given) needs counts")
        return (None if tao is None else _lib.fvec(tao, n), _ptr(pos_weight),
                None if counts is None else C.c_void_p(counts.data_ptr()))

    def step_cbafed(self, x, y, active_mask, annotation_num, bs_norm, tao, pos_weight, counts, loss_out):
        """train_CBAFed's step (:247-269, 303-340) fused.  tao None: warm-up.  pos_weight [C] float32 and counts [C+1] int64 are
        DEVICE tensors of the caller's: stage 2 rewrites the missing classes' weights and adds to the counts, with no host read"""
        t, pw, cn = self._cbafed_args(tao, pos_weight, counts)
        self._step(self.lib.fm_step_cbafed, x.shape[0], x, y, x.shape[0], _lib.fvec(active_mask, self.n_classes),
                   int(annotation_num), int(bs_norm), t, pw, cn, loss_out)

    # ---- the loss heads alone, on caller logits: two-view z [2B,C] (forward_train's layout; FedLSR, FedIRM) or single-view
    # z [B,C] (RSCFed, FedNoRo, CBAFed) -> (dz like z, loss [1]) ----------------------------------------------------------
    def _head(self, fn, views, z, y, zt, *args, tail=()):
        """fn is the caller's own self.lib.fm_loss_*; its C arguments are args (tensors as they are), then dz and loss (then
        tail, for a head with outputs behind them)"""
        self._check_stream()
        self._enqueue()
        B, n = y.shape[0], self.n_classes
        ts = [(z, views * B), (y, B)] + ([] if zt is None else [(zt, B)])
        shapes = all(tuple(t.shape) == (rows, n) for t, rows in ts)
        plain = all(t.dtype == torch.float32 and t.is_contiguous() for t, _ in ts)
        if views == 1 and not (shapes and plain):
            raise ValueError(f"single-view head: contiguous float32 [B, {n}] tensors are required")
        if not shapes:
            raise ValueError(f"two-view head: z must be [2B, C] and y [B, C], got {tuple(z.shape)} and {tuple(y.shape)}")
        if not plain:
            raise ValueError("two-view head: contiguous float32 tensors are required")
        dz, loss = torch.empty_like(z), torch.empty(1, device=z.device, dtype=torch.float32)
        _lib.check(fn(self.h, *_cargs(args), _ptr(dz), _ptr(loss), *_cargs(tail)))
        return dz, loss

    def _rel_arg(self, t, what):
        if t is None:
            return None
        n = self.n_classes
        if tuple(t.shape) != (n, n) or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"{what} must be a contiguous float32 [{n}, {n}] device tensor")
        return t

    def loss_fedlsr(self, z, y, pos_weight, mix1, beta):
        return self._head(self.lib.fm_loss_fedlsr, 2, z, y, None, z, y, _lib.fvec(pos_weight, self.n_classes),
                          C.c_float(mix1), C.c_float(beta), y.shape[0])

    def loss_fedirm_sup(self, z, y, pos_weight, active_mask, annotation_num, bs_norm, rel_acc=None):
        """rel_acc [C,C] (optional) += get_confuse_matrix(z[:B], y)"""
        n = self.n_classes
        return self._head(self.lib.fm_loss_fedirm_sup, 2, z, y, None, z, y, _lib.fvec(pos_weight, n),
                          _lib.fvec(active_mask, n), int(annotation_num), int(bs_norm), y.shape[0],
                          self._rel_arg(rel_acc, "rel_acc"))

    def loss_fedirm_rel(self, z, zt, y, pos_weight, active_mask, annotation_num, bs_norm, cw, target, rel_acc=None):
        """zt [B,C]: the EMA model's logits on view 2; target [C,C]: the aggregated relation matrix (device)"""
        B, n = y.shape[0], self.n_classes
        if tuple(zt.shape) != (B, n) or zt.dtype != torch.float32 or not zt.is_contiguous():
            raise ValueError(f"loss_fedirm_rel: zt must be a contiguous float32 [{B}, {n}] tensor")
        return self._head(self.lib.fm_loss_fedirm_rel, 2, z, y, None, z, zt, y, _lib.fvec(pos_weight, n),
                          _lib.fvec(active_mask, n), int(annotation_num), int(bs_norm), C.c_float(cw),
                          self._rel_arg(target, "target"), B, self._rel_arg(rel_acc, "rel_acc"))

    def loss_rscfed(self, z, zt, y, pos_weight, active_mask, annotation_num, bs_norm):
        n = self.n_classes
        return self._head(self.lib.fm_loss_rscfed, 1, z, y, zt, z, zt, y, _lib.fvec(pos_weight, n),
                          _lib.fvec(active_mask, n), int(annotation_num), int(bs_norm), y.shape[0])

    def loss_lakd(self, z, zt, y, active_mask, w_kd):
        return self._head(self.lib.fm_loss_lakd, 1, z, y, zt, z, zt, y, _lib.fvec(active_mask, self.n_classes),
                          C.c_float(w_kd), y.shape[0])

    def loss_cbafed(self, z, y, active_mask, annotation_num, bs_norm, tao, pos_weight, counts=None):
        """tao None: warm-up (pos_weight read, counts untouched); else stage 2 (see step_cbafed)"""
        t, pw, cn = self._cbafed_args(tao, pos_weight, counts)
        return self._head(self.lib.fm_loss_cbafed, 1, z, y, None, z, y, _lib.fvec(active_mask, self.n_classes),
                          int(annotation_num), int(bs_norm), t, y.shape[0], pw, cn)

    # ---- prototypes / tagging ------------------------------------------------------
    # ---- generic split step (rank-4 baselines: loss head computed by the host mirror) -----------
    def forward_train(self, x1, x2=None):
        self._check_stream()
        self._enqueue()
        views = 1 if x2 is None else 2
        B = x1.shape[0]
        self._draw(views * B)
        feat = torch.empty((views * B, self.feature_dim), device=self.device, dtype=torch.float32)
        logits = torch.empty((views * B, self.n_classes), device=self.device, dtype=torch.float32)
        _lib.check(self.lib.fm_forward_train(self.h, _ptr(x1), _ptr(x2), B, _ptr(feat), _ptr(logits)))
        self._pending_rows, self._pending_B = views * B, B
        return feat, logits

    def backward_step(self, dlogits):
        self._check_stream()
        self._enqueue(weights=True)
        _lib.check(self.lib.fm_backward_step(self.h, _ptr(dlogits.contiguous().float())))

    # ---- autograd path: backward into the gradient accumulator, optimizer step apart (model.HipNet, optim.Adam) -----
    def forward_recompute(self, x1, x2=None):
        """The train-mode forward of x1 (and x2) again, for a following backward_grads: same saved tensors, BN running
        statistics and counters untouched, no outputs.  The caller installs the draws of the original forward."""
        self._check_stream()
        self._enqueue()
        _lib.check(self.lib.fm_forward_recompute(self.h, _ptr(x1), _ptr(x2), x1.shape[0]))
        self._pending_rows, self._pending_B = (1 if x2 is None else 2) * x1.shape[0], x1.shape[0]

    def backward_grads(self, dlogits=None, dfeat=None, dx=None):
        """Backward of the pending forward_train / forward_recompute from d loss / d logits [views*B, C] and d loss / d feature
        [views*B, D] (None = zero); the parameter gradients are added to the engine's accumulator, no optimizer step.
        dx: a contiguous fp32 device tensor shaped like x1 (or a pair, one per view, either entry None) that receives d loss /
        d image of that view -- written, not accumulated (fm_backward_grads_x).  None: no input gradient is computed."""
        self._check_stream()
        self._enqueue()
        dz = None if dlogits is None else dlogits.detach().contiguous().float()
        df = None if dfeat is None else dfeat.detach().contiguous().float()
        rows = getattr(self, "_pending_rows", 0)
        if dz is not None and tuple(dz.shape) != (rows, self.n_classes):
            raise ValueError(f"backward_grads: dlogits {tuple(dz.shape)}, the pending forward's logits are {(rows, self.n_classes)}")
        if df is not None and tuple(df.shape) != (rows, self.feature_dim):
            raise ValueError(f"backward_grads: dfeat {tuple(df.shape)}, the pending forward's feature is {(rows, self.feature_dim)}")
        if dx is None:
            _lib.check(self.lib.fm_backward_grads(self.h, _ptr(dz), _ptr(df)))
            return
        dxs = list(dx) if isinstance(dx, (tuple, list)) else [dx]
        dxs += [None] * (2 - len(dxs))
        if len(dxs) != 2:
            raise ValueError("backward_grads: dx is one tensor or a pair of tensors")
        want = (getattr(self, "_pending_B", 0), 3, self.in_h, self.in_w)
        for t in dxs:
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda
                                  or t.device.index != torch.cuda.current_device() or tuple(t.shape) != want):
                raise ValueError(f"backward_grads: dx must be a contiguous fp32 {want} tensor on {self.device}")
        _lib.check(self.lib.fm_backward_grads_x(self.h, _ptr(dz), _ptr(df), _ptr(dxs[0]), _ptr(dxs[1])))

    def zero_grad(self):
        _lib.check(self.lib.fm_zero_grad(self.h))

    def eval_metrics(self, scores, labels, threshold=0.5, ap=True, auc=True, counts=True):
        """globaltest's per-class metrics on the device (fm_eval_metrics): scores, labels contiguous fp32 [N, C] device
        tensors -> (ap [C] fp64, auc [C] fp64, counts [C, 4] int64 {tp, npos, npred, tn} with pred = score > threshold) as
        device tensors; enqueued, not synchronised.  ap / auc / counts False: that output is not computed and comes back as
        None (counts alone skips the ranking passes)."""
        for name, t in (("scores", scores), ("labels", labels)):
            if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda
                    or t.device.index != torch.cuda.current_device() or t.dim() != 2):
                raise ValueError(f"eval_metrics: {name} must be a contiguous fp32 [N, C] tensor on {self.device}")
        if scores.shape != labels.shape:
            raise ValueError(f"eval_metrics: scores {tuple(scores.shape)} and labels {tuple(labels.shape)} differ")
        N, Cn = int(scores.shape[0]), int(scores.shape[1])
        if not (1 <= Cn <= _lib.FM_MAX_CLASSES and 1 <= N <= 1 << 22):
            raise ValueError(f"eval_metrics: N = {N}, C = {Cn}: 1 <= C <= {_lib.FM_MAX_CLASSES}, 1 <= N <= 2^22")
        self._check_stream()
        self._enqueue()
        o_ap = torch.empty(Cn, device=self.device, dtype=torch.float64) if ap else None
        o_auc = torch.empty(Cn, device=self.device, dtype=torch.float64) if auc else None
        o_cnt = torch.empty((Cn, 4), device=self.device, dtype=torch.int64) if counts else None
        vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
        _lib.check(self.lib.fm_eval_metrics(self.h, vp(scores), vp(labels), N, Cn, float(threshold), vp(o_ap), vp(o_auc),
                                            vp(o_cnt)))
        return o_ap, o_auc, o_cnt

    def bn_freeze(self, on=True):
        """Frozen BatchNorm statistics for the NEXT forward_train / forward_recompute (kept until changed): every BatchNorm
        applies its running statistics, which -- like the num_batches_tracked counters -- stay as they are.  A backward runs
        in the mode of the forward it belongs to, whatever the flag is by then.  The fused step_* ignore the flag."""
        _lib.check(self.lib.fm_bn_freeze(self.h, int(bool(on))))

    @property
    def bn_frozen(self):
        return bool(self.lib.fm_bn_frozen(self.h))

    def adam_step(self, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        """torch.optim.Adam (coupled L2) over the accumulator with the engine's moments (adam_reset zeroes them)."""
        self._check_stream()
        self._enqueue(weights=True)
        hp = _lib.FmAdam(lr, betas[0], betas[1], eps, weight_decay)
        _lib.check(self.lib.fm_adam_step(self.h, C.byref(hp)))

    def grads(self):
        """The accumulator in state_dict order (conv weights OIHW, BN running statistics as zeros) as a cuda fp32 tensor
        of get_state()'s float length; enqueued, not synchronised."""
        self._check_stream()
        self._enqueue()
        out = torch.empty(self.nf, device=self.device, dtype=torch.float32)
        _lib.check(self.lib.fm_get_grads(self.h, _ptr(out)))
        return out

    # ---- SGD, AdamW, clipping, optimizer state (fedmlp_amd.optim) ----------------------------------------
    def sgd_reset(self, lr=0.0, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
        """A fresh torch.optim.SGD: the handle's moment arenas and step count zeroed (what adam_reset does)."""
        hp = _lib.FmSgd(lr, momentum, dampening, weight_decay, int(bool(nesterov)))
        self._enqueue()
        _lib.check(self.lib.fm_sgd_reset(self.h, C.byref(hp)))

    def sgd_step(self, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
        """torch.optim.SGD over the accumulator; the momentum buffer is the engine's first moment arena."""
        self._check_stream()
        self._enqueue(weights=True)
        hp = _lib.FmSgd(lr, momentum, dampening, weight_decay, int(bool(nesterov)))
        _lib.check(self.lib.fm_sgd_step(self.h, C.byref(hp)))

    def adamw_step(self, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        """torch.optim.AdamW (decoupled weight decay) over the accumulator with the engine's moments."""
        self._check_stream()
        self._enqueue(weights=True)
        hp = _lib.FmAdam(lr, betas[0], betas[1], eps, weight_decay)
        _lib.check(self.lib.fm_adamw_step(self.h, C.byref(hp)))

    # ---- per-layer requires_grad, optimizer parameter groups (model.HipNet.requires_grad_, fedmlp_amd.optim) --------------
    def _entry_array(self, values, what):
        a = np.ascontiguousarray(values, dtype=np.int32).reshape(-1)
        n = len(spec.entries(self.model, self.n_classes))
        if a.size != n:
            raise ValueError(f"{what}: {a.size} values, the state has {n} entries")
        return a, n

    def set_trainable(self, flags):
        """requires_grad of every parameter: one flag per state_dict entry in spec.entries order (buffers' slots are ignored).
        Read by the NEXT forward_train / forward_recompute -- a backward runs under the mask of the forward it belongs to --
        and by the grouped optimizer steps.  Under a non-default mask the fused step_* raise."""
        a, n = self._entry_array(flags, "set_trainable")
        _lib.check(self.lib.fm_set_trainable(self.h, a.ctypes.data_as(C.c_void_p), n))

    def get_trainable(self):
        n = len(spec.entries(self.model, self.n_classes))
        a = np.empty(n, np.int32)
        _lib.check(self.lib.fm_get_trainable(self.h, a.ctypes.data_as(C.c_void_p), n))
        return a

    def optim_groups(self, group_of_entry, n_groups):
        """The parameter group (0 .. n_groups - 1, -1 = not optimized) of every state_dict entry; n_groups = 0 clears the table."""
        if not n_groups:
            _lib.check(self.lib.fm_optim_groups(self.h, None, 0, 0))
            return
        a, n = self._entry_array(group_of_entry, "optim_groups")
        _lib.check(self.lib.fm_optim_groups(self.h, a.ctypes.data_as(C.c_void_p), n, int(n_groups)))

    def _step_groups(self, fn, struct, rows):
        self._check_stream()
        self._enqueue(weights=True)
        hp = (struct * len(rows))(*[struct(*r) for r in rows])
        _lib.check(fn(self.h, hp, len(rows)))

    def adam_step_groups(self, hps):
        """adam_step with one (lr, betas, eps, weight_decay) per group of the installed optim_groups table."""
        self._step_groups(self.lib.fm_adam_step_groups, _lib.FmAdam, [(lr, b[0], b[1], eps, wd) for lr, b, eps, wd in hps])

    def adamw_step_groups(self, hps):
        self._step_groups(self.lib.fm_adamw_step_groups, _lib.FmAdam, [(lr, b[0], b[1], eps, wd) for lr, b, eps, wd in hps])

    def sgd_step_groups(self, hps):
        """sgd_step with one (lr, momentum, dampening, weight_decay, nesterov) per group."""
        self._step_groups(self.lib.fm_sgd_step_groups, _lib.FmSgd, [(lr, m, d, wd, int(bool(n))) for lr, m, d, wd, n in hps])

    def grad_norm(self):
        """L2 norm of the accumulator as a 0-dim cuda fp32 tensor (0 when it is empty); enqueued, not synchronised."""
        self._check_stream()
        self._enqueue()
        out = torch.empty((), device=self.device, dtype=torch.float32)
        _lib.check(self.lib.fm_grad_norm(self.h, _ptr(out)))
        return out

    def clip_grad_norm(self, max_norm):
        """accumulator *= min(1, max_norm / (norm + 1e-6)); returns the norm before clipping as a 0-dim cuda tensor."""
        self._check_stream()
        self._enqueue()
        out = torch.empty((), device=self.device, dtype=torch.float32)
        _lib.check(self.lib.fm_clip_grad_norm(self.h, C.c_float(max_norm), _ptr(out)))
        return out

    def clip_grad_value(self, clip_value):
        """accumulator = clamp(accumulator, -clip_value, clip_value)"""
        self._check_stream()
        self._enqueue()
        _lib.check(self.lib.fm_clip_grad_value(self.h, C.c_float(clip_value)))

    def optim_state(self):
        """(step, m, v): the step count and the two moment arenas as flat cuda fp32 tensors in grads() layout."""
        self._check_stream()
        self._enqueue()
        m = torch.empty(self.nf, device=self.device, dtype=torch.float32)
        v = torch.empty(self.nf, device=self.device, dtype=torch.float32)
        step = C.c_int64()
        _lib.check(self.lib.fm_optim_get_state(self.h, _ptr(m), _ptr(v), C.byref(step)))
        return step.value, m, v

    def set_optim_state(self, step, m, v=None):
        """The inverse of optim_state(); v None (SGD) zeroes the second arena.  m / v: nf floats in grads() layout."""
        self._check_stream()
        ts = []
        for t in (m, v):
            if t is not None:
                t = torch.as_tensor(t, dtype=torch.float32).to(self.device).contiguous().reshape(-1)
                if t.numel() != self.nf:
                    raise ValueError(f"set_optim_state: a state tensor has {t.numel()} elements, the engine's layout has {self.nf}")
            ts.append(t)
        self._enqueue()
        # enqueued on torch's current stream (_check_stream), so the caching allocator may take the staging tensors back at once
        _lib.check(self.lib.fm_optim_set_state(self.h, _ptr(ts[0]), _ptr(ts[1]), int(step)))

    def teacher_axpby(self, w_teacher, w_student):
        self._enqueue()
        _lib.check(self.lib.fm_teacher_axpby(self.h, C.c_float(w_teacher), C.c_float(w_student)))

    def teacher_ema_params(self, alpha):
        """update_ema_variables (utils/local_training.py:62-65) over the parameters only: running statistics and counters stay"""
        self._enqueue()
        _lib.check(self.lib.fm_teacher_ema_params(self.h, C.c_double(float(alpha))))

    def teacher_swap(self):
        self._enqueue(weights=True)
        _lib.check(self.lib.fm_teacher_swap(self.h))

    def proto_reset(self):
        self._enqueue()
        _lib.check(self.lib.fm_proto_reset(self.h))

    def proto_accumulate(self, feat, logits, labels, active_mask, negative_mask, L, U):
        n = self.n_classes
        self._enqueue()
        _lib.check(self.lib.fm_proto_accumulate(self.h, _ptr(feat), _ptr(logits), _ptr(labels),
                                                feat.shape[0], _lib.fvec(active_mask, n),
                                                _lib.fvec(negative_mask, n), C.c_float(L),
                                                C.c_float(U)))

    def proto_finalize(self, zero_guard, n_local, active_mask):
        proto = np.empty((2 * self.n_classes, self.feature_dim), np.float32)
        t = np.empty(self.n_classes, np.float64)
        self._enqueue()
        _lib.check(self.lib.fm_proto_finalize(self.h, int(zero_guard), int(n_local),
                                              _lib.fvec(active_mask, self.n_classes),
                                              proto.ctypes.data_as(C.c_void_p),
                                              t.ctypes.data_as(C.c_void_p)))
        return t, proto

    def cos_tag(self, feat, proto, classes):
        N = feat.shape[0]
        sim = torch.empty((len(classes), N), device=self.device, dtype=torch.float32)
        if len(classes) and N:
            self._enqueue()
            cls = (C.c_int32 * len(classes))(*[int(c) for c in classes])
            _lib.check(self.lib.fm_cos_tag(self.h, _ptr(feat), N, _ptr(proto), cls, len(classes),
                                           _ptr(sim)))
        return sim

    def select_topk(self, sim_row, clean_thr, noise_thr):
        N = sim_row.shape[0]
        cap = max(N, 1)
        top, bot = (C.c_int32 * cap)(), (C.c_int32 * cap)()
        nt, nb = C.c_int32(), C.c_int32()
        self._enqueue()
        _lib.check(self.lib.fm_select_topk(self.h, _ptr(sim_row), N, float(clean_thr),
                                           float(noise_thr), cap, top, C.byref(nt), bot,
                                           C.byref(nb)))
        return list(top[:nt.value]), list(bot[:nb.value])

    def select_topk_rows(self, sims, pools, clean_thr, noise_thr):
        """Every class of a round at once: sims [n_cls, N] (cos_tag's output), pools[k] = the positions of class k's pool inside
        its similarity row, in pool order (None = every row).  -> [(top, bot)] per class, as positions INSIDE the pool.  One
        launch pair and one device-to-host read (fm_select_topk_rows)."""
        n_cls, N = int(sims.shape[0]), int(sims.shape[1])
        if n_cls == 0:
            return []
        sizes = [N if p is None else len(p) for p in pools]
        whole = all(p is None for p in pools)
        stride = max(max(sizes), 1)
        rows = None
        if not whole:
            flat = np.zeros((n_cls, stride), dtype=np.int32)
            for k, p in enumerate(pools):
                flat[k, :sizes[k]] = np.arange(N, dtype=np.int32) if p is None else np.asarray(p, dtype=np.int32)
            rows = flat.ctypes.data_as(C.POINTER(C.c_int32))
            self._keep = flat
        cap = int(max(clean_thr, noise_thr, 0.0) * max(sizes)) + 1
        pn = (C.c_int32 * n_cls)(*sizes)
        top, bot = (C.c_int32 * (n_cls * cap))(), (C.c_int32 * (n_cls * cap))()
        nt, nb = (C.c_int32 * n_cls)(), (C.c_int32 * n_cls)()
        self._enqueue()
        _lib.check(self.lib.fm_select_topk_rows(self.h, _ptr(sims), N, n_cls, rows, pn, stride, float(clean_thr),
                                                float(noise_thr), cap, top, nt, bot, nb))
        return [(list(top[k * cap:k * cap + nt[k]]), list(bot[k * cap:k * cap + nb[k]])) for k in range(n_cls)]

    # ---- input pipeline ---------------------------------------------------------------
    def augment(self, cache_u8, idx, params, mean, std):
        """uint8 cache [N,3,H,W] + sample indices [B] (int32) + fixed-point affine/flip records [B,8] (int32,
        fedmlp_amd.augment.fixed_point_params) -> fp32 NCHW batch."""
        B = idx.shape[0]
        out = torch.empty((B, 3, self.in_h, self.in_w), device=self.device, dtype=torch.float32)
        assert cache_u8.is_cuda and cache_u8.dtype == torch.uint8 and cache_u8.is_contiguous()
        assert params.dtype == torch.int32 and params.shape == (B, 8)
        self._enqueue()
        _lib.check(self.lib.fm_augment(self.h, C.c_void_p(cache_u8.data_ptr()), _ptr(idx), _ptr(params), B,
                                       _lib.fvec(mean, 3), _lib.fvec(std, 3), _ptr(out)))
        return out

    def augment_strong(self, cache_u8, idx, params, strong, mean, std):
        """the FixMatch strong view: augment()'s arguments plus the [B,20] int32 records of
        fedmlp_amd.augment.draw_strong (two RandAugmentMC op slots and the cutout corners) -> fp32 NCHW batch."""
        B = idx.shape[0]
        out = torch.empty((B, 3, self.in_h, self.in_w), device=self.device, dtype=torch.float32)
        assert cache_u8.is_cuda and cache_u8.dtype == torch.uint8 and cache_u8.is_contiguous()
        assert params.dtype == torch.int32 and params.shape == (B, 8)
        assert strong.dtype == torch.int32 and strong.shape == (B, 20) and strong.is_contiguous()
        self._enqueue()
        _lib.check(self.lib.fm_augment_strong(self.h, C.c_void_p(cache_u8.data_ptr()), _ptr(idx), _ptr(params), _ptr(strong),
                                              B, _lib.fvec(mean, 3), _lib.fvec(std, 3), _ptr(out)))
        return out

    # ---- measurement ------------------------------------------------------------------
    def profile_enable(self, on):
        _lib.check(self.lib.fm_profile_enable(self.h, int(on)))

    def profile_read(self, family):
        n, ms, fl = C.c_int64(), C.c_double(), C.c_double()
        _lib.check(self.lib.fm_profile_read(self.h, family, C.byref(n), C.byref(ms), C.byref(fl)))
        return n.value, ms.value, fl.value

    def profile_ops(self, enable, read=True):
        """[(label, calls, total_ms)] of the ops timed since the last read (EfficientNet-B0 graph)."""
        buf = C.create_string_buffer(1 << 16) if read else None
        _lib.check(self.lib.fm_profile_ops(self.h, int(enable), buf, (1 << 16) if read else 0))
        rows = []
        if read:
            for line in buf.value.decode().splitlines():
                lab, n, ms = line.split("\t")
                rows.append((lab, int(n), float(ms)))
        return rows

    # ---- kernel-level test hooks ----------------------------------------------------------
    def debug_conv_info(self, conv):
        info = (C.c_int32 * 16)()
        _lib.check(self.lib.fm_debug_conv_info(self.h, conv, info))
        keys = ("cin", "cout", "k", "stride", "pad", "hin", "win", "hout", "wout", "cin_p", "Kw", "kw_p", "cout_p")
        return dict(zip(keys, list(info)))

    def debug_stem_masks(self, imgs, groups):
        """(relu mask [imgs, H/2, W/2, 64] bool, max-pool argmax code [imgs, H/4, W/4, 64] uint8) of the last train-mode forward's
        stem (fm_debug_stem_masks)"""
        H2, W2 = self.in_h // 2, self.in_w // 2
        bits = np.empty((imgs, H2, W2, 8), np.uint8)
        code = np.empty((imgs, H2 // 2, W2 // 2, 64), np.uint8)
        _lib.check(self.lib.fm_debug_stem_masks(self.h, imgs, groups, bits.ctypes.data_as(C.c_void_p),
                                                code.ctypes.data_as(C.c_void_p)))
        return np.unpackbits(bits, axis=-1, bitorder="little").astype(bool), code

    def debug_get_grads(self):
        flat = np.empty(self.nf, np.float32)
        _lib.check(self.lib.fm_debug_get_grads(self.h, flat.ctypes.data_as(C.c_void_p)))
        return flat

    WAIT_KINDS = ("side_begin", "side_guard", "side_join", "ev_in", "ev_t")     # FM_WAIT_* of fedmlp_hip_debug.h, in order

    def debug_lane_delay(self, lane, at, micros):
        """Arm one delay of `micros` us at delay point `at` of lane 0 (main) / 1 (side); restarts the point and wait counts
        (fm_debug_lane_delay).  micros = 0 only counts."""
        _lib.check(self.lib.fm_debug_lane_delay(self.h, int(lane), int(at), int(micros)))

    def debug_lane_points(self, disarm=False):
        """Since the last debug_lane_delay: {"points": (main, side), "fired": bool, "waits" / "skipped": {kind: count}}."""
        o = (C.c_int64 * 16)()
        _lib.check(self.lib.fm_debug_lane_points(self.h, o, int(bool(disarm))))
        n = len(self.WAIT_KINDS)
        return {"points": (int(o[0]), int(o[1])), "fired": bool(o[2]),
                "waits": {k: int(o[3 + i]) for i, k in enumerate(self.WAIT_KINDS)},
                "skipped": {k: int(o[3 + n + i]) for i, k in enumerate(self.WAIT_KINDS)}}

    def debug_drop_wait(self, kind, on=True):
        """Skip (on) / keep the cross-lane wait of one kind (a name of WAIT_KINDS or its index): fm_debug_drop_wait."""
        which = self.WAIT_KINDS.index(kind) if isinstance(kind, str) else int(kind)
        _lib.check(self.lib.fm_debug_drop_wait(self.h, which, int(bool(on))))

    def debug_optim_arena(self, which):
        """torch view of a raw engine-layout arena of the optimizers: 0 / 1 the moments, 2 the gradient accumulator, 3 the
        gradients of the last backward."""
        p, n = C.c_void_p(), C.c_int64()
        _lib.check(self.lib.fm_debug_optim_arena(self.h, int(which), C.byref(p), C.byref(n)))
        return _device_view(p.value, n.value, self.device)

    def debug_entry_spans(self):
        """int64 [n_entries, 2]: (arena offset, span floats) of every state_dict entry, (-1, 0) for buffers."""
        n = len(spec.entries(self.model, self.n_classes))
        a = np.empty((n, 2), np.int64)
        _lib.check(self.lib.fm_debug_entry_spans(self.h, a.ctypes.data_as(C.c_void_p), n))
        return a

    def debug_pw(self, op, conv, x, dy, out, imgs, groups=1, psc=None, psh=None, gate=None, stats=None):
        self._enqueue()
        _lib.check(self.lib.fm_debug_pw(self.h, op, conv, _ptr(x), _ptr(dy), _ptr(out), imgs, groups, _ptr(psc),
                                        _ptr(psh), _ptr(gate), _ptr(stats)))

    def debug_pw_fwd(self, conv, x, out, imgs, groups=1, scale=None, shift=None, res=None, act=0, psc=None, psh=None, gate=None,
                     stats=None):
        """one 1x1 convolution (x bf16) or the stem (x = the fp32 NCHW batch) of a bf16 handle through conv_fwd, with the eval
        epilogue, the operand prologue or the train statistics (fm_debug_pw_fwd)"""
        self._enqueue()
        _lib.check(self.lib.fm_debug_pw_fwd(self.h, conv, _ptr(x), _ptr(out), imgs, groups, _ptr(scale), _ptr(shift), _ptr(res),
                                            int(act), _ptr(psc), _ptr(psh), _ptr(gate), _ptr(stats)))

    def debug_proj_bwd(self, conv, phase, dyp, yd, bn, gate, ds, imgs, groups, out, pool5=None):
        self._enqueue()
        _lib.check(self.lib.fm_debug_proj_bwd(self.h, conv, phase, _ptr(dyp), _ptr(yd), _ptr(bn), _ptr(gate), _ptr(ds), imgs,
                                              groups, _ptr(out), _ptr(pool5)))

    def debug_exp_bwd(self, conv, da, ye, x, res, bn, imgs, groups, dx, dw):
        self._enqueue()
        _lib.check(self.lib.fm_debug_exp_bwd(self.h, conv, _ptr(da), _ptr(ye), _ptr(x), _ptr(res), _ptr(bn), imgs, groups,
                                             _ptr(dx), _ptr(dw)))

    def debug_activation(self, kind, block, imgs):
        """post-ReLU activation kept by the last train-mode forward, as an NCHW numpy array"""
        dims = (C.c_int32 * 4)()
        _lib.check(self.lib.fm_debug_activation(self.h, kind, block, imgs, None, dims))
        out = np.empty(tuple(dims), np.float32)
        _lib.check(self.lib.fm_debug_activation(self.h, kind, block, imgs, out.ctypes.data_as(C.c_void_p), dims))
        return np.ascontiguousarray(out.transpose(0, 3, 1, 2))

    def debug_num_convs(self):
        return self.lib.fm_debug_num_convs(self.h)

    def debug_conv(self, op, conv, x, dy, out, imgs, groups=1, stats=None):
        self._enqueue()
        _lib.check(self.lib.fm_debug_conv(self.h, op, conv, _ptr(x), _ptr(dy), _ptr(out), imgs, groups,
                                          _ptr(stats)))

    def debug_conv_fwd(self, conv, x, out, imgs, groups=1, scale=None, shift=None, res=None, act=0, psc=None, psh=None,
                       gate=None, stats=None):
        """one convolution forward with the eval epilogue (scale, shift, res, act), the operand prologue of the streaming 1x1
        kernel (gate, psc, psh) or the train statistics (fm_debug_conv_fwd: the three forms the engine's graphs use)"""
        self._enqueue()
        _lib.check(self.lib.fm_debug_conv_fwd(self.h, conv, _ptr(x), _ptr(out), imgs, groups, _ptr(scale), _ptr(shift),
                                              _ptr(res), int(act), _ptr(psc), _ptr(psh), _ptr(gate), _ptr(stats)))

    def debug_conv_planes(self, conv, xp, imgs, scale, shift, res=None, resp=None, relu=0, out=None, outp=None):
        """one convolution as forward_eval runs it in planes mode (fm_debug_conv_planes): operand, residual and output as
        block-major bf16 planes (int16 device tensors) and / or fp32"""
        def words(t):
            assert t is None or (t.is_cuda and t.is_contiguous() and t.dtype == torch.int16), "planes are int16 device tensors"
            return None if t is None else C.c_void_p(t.data_ptr())
        self._enqueue()
        _lib.check(self.lib.fm_debug_conv_planes(self.h, conv, words(xp), imgs, _ptr(scale), _ptr(shift), _ptr(res), words(resp),
                                                 int(relu), _ptr(out), words(outp)))

    # arm codes of fm_debug_conv_arm (include/fedmlp_hip_debug.h), in the header's order
    CONV_ARMS = ("igemm", "igemm_stem", "stem_rows", "pconv_ts", "pconv_tap", "pwgrad", "pwgrad_ring", "wgrad_generic",
                 "wgrad_skinny", "stem_dgrad")

    def debug_conv_arm(self, op, conv, imgs):
        """the launcher fm_debug_conv(op, conv) takes for `imgs` images: a name of CONV_ARMS (host-side query, no launch)"""
        rc = self.lib.fm_debug_conv_arm(self.h, op, conv, imgs)
        if rc < 0:
            _lib.check(rc)
        return self.CONV_ARMS[rc]

    def debug_block_dgrad(self, block, dy1, dyd, dx, imgs):
        """input gradient of stride-2 basic block `block` from the gradients of its conv1 / downsample outputs (fp32 NHWC)"""
        self._enqueue()
        _lib.check(self.lib.fm_debug_block_dgrad(self.h, block, _ptr(dy1), _ptr(dyd), _ptr(dx), imgs))

    # op codes of fm_debug_ew (include/fedmlp_hip_debug.h), in the header's order
    EW_OPS = ("split_planes", "planes_to_f32", "bn_finalize", "bn_finalize_frozen", "bn_eval_affine", "bn_apply",
              "bn_apply_planes", "stem_pool", "stem_pool_planes", "stem_pool_bwd", "stem_pool_bn_reduce", "stem_pool_bn_apply",
              "bn_bwd_reduce", "bn_bwd_finalize", "bn_bwd_apply", "bn_bwd_apply_planes")

    def debug_ew(self, op, ptrs, dims, scalars=()):
        """one BatchNorm / stem-pool / plane-writer launcher on caller tensors (fm_debug_ew): op = a name of EW_OPS, ptrs =
        contiguous device tensors of any dtype in the header's operand order (None = absent), dims / scalars as documented there"""
        assert len(ptrs) <= 12 and len(dims) <= 5 and len(scalars) <= 2, (len(ptrs), len(dims), len(scalars))
        for t in ptrs:
            assert t is None or (t.is_cuda and t.is_contiguous()), op
        p = (C.c_void_p * 12)(*[None if t is None else t.data_ptr() for t in ptrs])
        d = (C.c_int32 * 5)(*[int(v) for v in dims])
        _lib.check(self.lib.fm_debug_ew(self.h, self.EW_OPS.index(op), p, d, _lib.fvec(list(scalars) + [0.0] * (2 - len(scalars)))))

    # op codes of fm_debug_eff (include/fedmlp_hip_debug.h), in the header's order
    EFF_OPS = ("dw_fwd", "dw_dgrad", "dw_wgrad", "se_fwd", "se_scale", "se_bwd_bn1", "se_wgrad", "bnact_apply", "chan_reduce",
               "bnact_bwd_apply")

    def debug_eff_ws(self, op, dims):
        """floats of each workspace / result of one fm_debug_eff op at these dimensions (fm_debug_eff_ws), in the header's order"""
        assert len(dims) <= 13, len(dims)
        d = (C.c_int32 * 13)(*[int(v) for v in dims])
        n = (C.c_int64 * 4)()
        _lib.check(self.lib.fm_debug_eff_ws(self.EFF_OPS.index(op), d, n))
        return list(n)

    def debug_eff(self, op, ptrs, dims, scalars=()):
        """one depthwise / squeeze-excite / BN+activation launcher of the EfficientNet-B0 path on caller tensors (fm_debug_eff): op = a name of
        EFF_OPS, ptrs = contiguous device tensors of any dtype in the header's operand order (None = absent), dims as documented
        there.  Returns the launcher's "request served" flag (False for the launchers that return nothing)."""
        assert len(ptrs) <= 15 and len(dims) <= 13 and len(scalars) <= 1, (len(ptrs), len(dims), len(scalars))
        for t in ptrs:
            assert t is None or (t.is_cuda and t.is_contiguous()), op
        served = C.c_int32(-1)
        p = (C.c_void_p * 16)(*([None if t is None else t.data_ptr() for t in ptrs] + [None] * (15 - len(ptrs))
                                + [C.addressof(served)]))
        d = (C.c_int32 * 13)(*[int(v) for v in dims])
        _lib.check(self.lib.fm_debug_eff(self.h, self.EFF_OPS.index(op), p, d, _lib.fvec(list(scalars) + [0.0] * (1 - len(scalars)))))
        return served.value == 1

    # op codes of fm_debug_head (include/fedmlp_hip_debug.h), in the header's order
    HEAD_OPS = ("avgpool", "fc_fwd", "fc_bwd", "loss_bce", "loss_stage1", "loss_stage2", "loss_fixmatch")

    def debug_head(self, op, ptrs, dims, scalars=()):
        """one classifier-head / loss launcher on caller tensors (fm_debug_head): op = a name of HEAD_OPS, ptrs = contiguous device
        tensors in the header's operand order (None = absent); a per-class HOST vector (pos_w, pos_wu, active) is given as a list
        of floats.  dims / scalars as documented there."""
        assert len(ptrs) <= 8 and len(dims) <= 5 and len(scalars) <= 2, (len(ptrs), len(dims), len(scalars))
        keep, raw = [], []
        for t in ptrs:
            if t is None:
                raw.append(None)
            elif isinstance(t, (list, tuple)):
                keep.append(_lib.fvec(t))
                raw.append(C.addressof(keep[-1]))
            else:
                assert t.is_cuda and t.is_contiguous(), op
                raw.append(t.data_ptr())
        p = (C.c_void_p * 8)(*(raw + [None] * (8 - len(raw))))
        d = (C.c_int32 * 5)(*[int(v) for v in dims])
        _lib.check(self.lib.fm_debug_head(self.h, self.HEAD_OPS.index(op), p, d, _lib.fvec(list(scalars) + [0.0] * (2 - len(scalars)))))


class _CudaArrayView:
    """Minimal __cuda_array_interface__ carrier so torch can alias engine memory."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (ptr, False),
                                         "version": 2, "strides": None}


def _device_view(ptr, n, device):
    return torch.as_tensor(_CudaArrayView(ptr, n), device=device)


_ENGINES = {}


def get_engine(model, n_classes, in_h, in_w, max_images, device=None, precision="fp32"):
    """Process-wide engine cache (engines own GBs of workspace; the reference's
    cheap deepcopy(net) objects map onto ONE engine whose state is swapped)."""
    if device is None:
        from .launch import default_device
        device = default_device()
    key = (model, int(n_classes), int(in_h), int(in_w), str(device), precision)
    e = _ENGINES.get(key)
    if e is None or e.max_images < max_images:
        if e is not None:
            # a larger workspace replaces the engine: first pull the resident net's device-only
            # trained state to its host copy (and unbind it), or it would be lost with the handle
            owner = getattr(e, "_owner", None)
            if owner is not None:
                owner._pull()
                owner._engine = None
            e._owner = None
            e.close()
        e = Engine(model, n_classes, in_h, in_w, max_images, device, precision)
        _ENGINES[key] = e
    return e


def release_engines():
    """Close every cached engine (pulling a resident net's trained state to its host copy first).  The next
    get_engine() builds a fresh one -- which is also when the library's per-engine environment switches are read."""
    for key, e in list(_ENGINES.items()):
        owner = getattr(e, "_owner", None)
        if owner is not None:
            owner._pull()
            owner._engine = None
        e._owner = None
        e.close()
        del _ENGINES[key]
