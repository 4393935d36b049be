#!/usr/bin/env python3
"""Thin FL driver: the FedMLP / FedAVG / FedAVG+FixMatch / FedLSR / FedIRM / RSCFed / FedNoRo / CBAFed rows of the
reference's main.py (main.py:106-319, with the 'FeMLP' typos normalised) on the HIP engine, one process
per GPU, clients dealt round-robin over the ranks, aggregation as RCCL all-reduces
(fedmlp_amd/fedavg.py).  Data is synthetic and HBM-resident (the reference's datasets and
ImageNet weights are not available offline).  main() sets the process up; run_rounds() is the loop over rounds, which asks
the row's object (fedmlp_amd/rows.py, one class per --exp value) for everything that differs between the rows.

  python -m fedmlp_amd.driver --gpus 8 --exp FedMLP --n_clients 8 --rounds_warmup 4 --rounds_FedMLP_stage1 2
  python -m fedmlp_amd.driver --exp FedIRM --rounds_warmup 4 --rounds_FedIRM_sup 2
(with --gpus N > 1 and no torchrun environment the driver starts its N ranks itself, fedmlp_amd/launch.py)
"""
import argparse
import json
import os
import time

import numpy as np
import torch

from fedmlp_amd.rows import ROWS, RSCFED_K, RSCFED_M         # noqa: F401  (tests read RSCFED_M / RSCFED_K from here)


def build_parser():
    """the driver's flags, before any are parsed (fedmlp_amd/driver_rofl.py starts from the same parser)"""
    p = argparse.ArgumentParser()      # flag names/defaults follow utils/options.py:4-81
    p.add_argument("--exp", default="FedMLP", choices=[e for e in ROWS if e != "RoFL"])      # RoFL: fedmlp_amd.driver_rofl
    p.add_argument("--model", default="Resnet18")
    p.add_argument("--seed", type=int, default=1037)
    p.add_argument("--batch_size", type=int, default=32)
    p.add_argument("--base_lr", type=float, default=3e-5)
    p.add_argument("--annotation_num", type=int, default=1)
    p.add_argument("--n_clients", type=int, default=8)            # utils/options.py:34
    p.add_argument("--n_classes", type=int, default=8)            # utils/options.py:36
    p.add_argument("--local_ep", type=int, default=1)
    p.add_argument("--rounds_warmup", type=int, default=500)      # utils/options.py:42
    p.add_argument("--rounds_FedMLP_stage1", type=int, default=50)    # utils/options.py:46
    p.add_argument("--t_w", type=int, default=40)                 # utils/options.py:67 (FedLSR: rounds of the beta warm-up)
    p.add_argument("--rounds_FedIRM_sup", type=int, default=20)   # utils/options.py:69
    p.add_argument("--consistency", type=float, default=1)        # utils/options.py:70
    p.add_argument("--consistency_rampup", type=float, default=30)    # utils/options.py:71
    p.add_argument("--ema_decay", type=float, default=0.99)       # utils/options.py:72
    p.add_argument("--rounds_FedNoRo_warmup", type=int, default=500)  # utils/options.py:74
    p.add_argument("--begin", type=int, default=10)               # utils/options.py:75 (FedNoRo: ramp-up begin)
    p.add_argument("--end", type=int, default=499)                # utils/options.py:76
    p.add_argument("--a", type=float, default=0.8)                # utils/options.py:77
    p.add_argument("--rounds_CBAFed_warmup", type=int, default=50)    # utils/options.py:79
    p.add_argument("--forget_rate", type=float, default=0.2)      # utils/options.py:53 (RoFL; constant: main.py's schedule is applied nowhere)
    p.add_argument("--T_pl", type=int, default=100)               # utils/options.py:55 (RoFL: rounds before the global-guided pseudo labels)
    p.add_argument("--lambda_cen", type=float, default=1.0)       # utils/options.py:56
    p.add_argument("--lambda_e", type=float, default=0.8)         # utils/options.py:57
    p.add_argument("--U", type=float, default=0.7)
    p.add_argument("--L", type=float, default=0.3)
    p.add_argument("--clean_threshold", type=float, default=0.005)
    p.add_argument("--noise_threshold", type=float, default=0.01)
    p.add_argument("--feature_dim", type=int, default=0, help="0 = the model's own (512 ResNet-18, 1280 Efficient_b0)")
    p.add_argument("--n_local", type=int, default=512, help="samples per client (5000 for ICH)")
    p.add_argument("--hw", type=int, default=224)
    p.add_argument("--gpus", type=int, default=1, help="ranks = GPUs; clients are dealt round-robin over them")
    p.add_argument("--precision", default="fp32", choices=["fp32", "bf16"], help="bf16: Efficient_b0 only")
    p.add_argument("--streams", type=int, default=0, help="engine stream mode (fm_config.reserved[1]): 0 default, 1 one stream")
    p.add_argument("--pretrained", type=int, default=1,
                   help="utils/options.py:26: ImageNet checkpoint through build_model (a warning and the from-scratch init "
                        "when no checkpoint file is on this machine)")
    p.add_argument("--pretrained_path", default=None)
    p.add_argument("--init_ckpt", default=None, help="torch.save(state_dict) file to start from (main.py:361-367)")
    p.add_argument("--save_every", type=int, default=0, help="save netglob.state_dict() every N rounds (main.py:237)")
    p.add_argument("--save_dir", default=".")
    p.add_argument("--augment", type=int, default=0,
                   help="1: uint8 HBM cache + per-sample RandomAffine/HFlip/Normalize kernel (dataset/dataset.py:40-53); "
                        "2: the same with the FixMatch pair (:63-77): image_aug_2 is weak + RandAugmentMC(2, 10) + cutout")
    p.add_argument("--eval_every", type=int, default=0,
                   help="globaltest of the new global model every K rounds (main.py:322-357 uses 10), the forward dealt over "
                        "the ranks and the metrics from fm_eval_metrics; 0 = never")
    p.add_argument("--n_test", type=int, default=1024, help="samples of the synthetic test set (--eval_every)")
    p.add_argument("--prox_mu", type=float, default=0.0,
                   help="FedProx: mu of the proximal term mu/2 |w - w_glob|^2 in every local step (fedmlp_amd/drift.py); 0 = off")
    p.add_argument("--scaffold", type=int, default=0, choices=[0, 1],
                   help="1: SCAFFOLD control variates in every local step (fedmlp_amd/drift.py)")
    p.add_argument("--server_opt", default="none", choices=["none", "avgm", "adagrad", "adam", "yogi"],
                   help="server optimizer on the aggregated model (fedmlp_amd/server_opt.py): FedAvgM, FedAdagrad, FedAdam, FedYogi")
    p.add_argument("--server_lr", type=float, default=None, help="default: the class's own (1.0 avgm, 1e-2 the adaptive rules)")
    p.add_argument("--server_beta1", type=float, default=None, help="momentum of avgm; default 0.9")
    p.add_argument("--server_beta2", type=float, default=None, help="adam, yogi; default 0.99")
    p.add_argument("--server_tau", type=float, default=None, help="adagrad, adam, yogi; default 1e-3")
    p.add_argument("--init_server_opt", default=None,
                   help="a server_opt_{rnd}.pth of --save_every to resume the server optimizer from; its hyper-parameters are "
                        "taken, and a --server_* flag that contradicts them is refused")
    return p


DRIFT_EXPS = tuple(e for e, row in ROWS.items() if row.trains_with_drift)     # the trainers that install LocalUpdate.drift


def check_drift_flags(p, args):
    """--prox_mu / --scaffold: one of them at most, and only with the trainers that install a correction"""
    if not (args.prox_mu >= 0.0 and args.prox_mu != float("inf")):
        p.error("--prox_mu must be finite and >= 0")
    if args.prox_mu > 0 and args.scaffold:
        p.error("--prox_mu and --scaffold are two client-drift corrections: give one of them")
    if (args.prox_mu > 0 or args.scaffold) and args.exp not in DRIFT_EXPS:
        p.error(f"--prox_mu / --scaffold are built for --exp {', '.join(DRIFT_EXPS)} (got {args.exp})")


SERVER_OWN_EXPS = ("RSCFed", "CBAFed")                  # rows whose aggregation is server arithmetic of its own


def check_server_flags(p, args):
    """--server_opt and its hyper-parameters: not with the rows that have server arithmetic of their own, values the rule accepts"""
    given = [f for f in ("server_lr", "server_beta1", "server_beta2", "server_tau", "init_server_opt") if getattr(args, f) is not None]
    if args.server_opt == "none":
        if given:
            p.error(f"--{given[0]} needs --server_opt")
        return
    if args.exp in SERVER_OWN_EXPS:
        p.error(f"--server_opt is not built for --exp {' / '.join(SERVER_OWN_EXPS)}, whose aggregation has server arithmetic of "
                f"its own (got {args.exp})")
    from fedmlp_amd import server_opt
    try:
        server_opt.make(args.server_opt, args.server_lr, args.server_beta1, args.server_beta2, args.server_tau)
    except ValueError as ex:
        p.error(f"--server_opt {args.server_opt}: {ex}")


def args_parser(argv=None):
    p = build_parser()
    args = p.parse_args(argv)
    check_drift_flags(p, args)
    check_server_flags(p, args)
    if args.exp == "RSCFed" and args.n_clients < RSCFED_K:
        p.error(f"--exp RSCFed draws groups of {RSCFED_K} clients (main.py:116-119): --n_clients must be >= {RSCFED_K}")
    if args.exp == "FedNoRo" and args.rounds_warmup > args.rounds_FedNoRo_warmup:
        p.error("--exp FedNoRo: --rounds_warmup may not exceed --rounds_FedNoRo_warmup (after its warm-up the reference "
                "trains and aggregates nothing, main.py:140-148, 269-272)")
    return args


def gather_client_states(eng, states, counters, n_clients, rank, world, dist):
    """Every client's engine-layout state and counters on every rank: client c lives on rank c % world, so slot j of the
    all-gather carries the clients j * world .. j * world + world - 1 (a rank without a client in the slot sends zeros)."""
    like = eng.state_tensor()
    out_s, out_c = [None] * n_clients, [None] * n_clients
    for j in range((n_clients + world - 1) // world):
        c = j * world + rank
        parts = [torch.empty_like(like) for _ in range(world)]
        dist.all_gather(parts, states[c] if c < n_clients else torch.zeros_like(like))
        cnts = [None] * world
        dist.all_gather_object(cnts, counters.get(c))
        for r in range(world):
            if j * world + r < n_clients:
                out_s[j * world + r], out_c[j * world + r] = parts[r], np.asarray(cnts[r])
    return out_s, out_c


def AugmentedDeviceDataset(n, C, hw, seed, device, strong=False):
    """synthetic uint8 images behind fedmlp_amd.augment.AugmentedDataset (uint8 HBM cache + fm_augment; strong=True:
    the FixMatch pair, whose second view goes through fm_augment_strong)"""
    from fedmlp_amd.augment import AugmentedDataset
    rs = np.random.RandomState(seed)
    imgs = rs.randint(0, 256, size=(n, 3, hw, hw)).astype(np.uint8)
    targets = (rs.uniform(size=(n, C)) < 0.15).astype(np.float32)
    return AugmentedDataset(imgs, targets, train=True, generator=torch.Generator().manual_seed(seed), strong=strong)


class DeviceDataset:
    """dataset/all_dataset.py:64-83 contract on synthetic data kept in HBM."""

    def __init__(self, n, C, hw, seed, device):
        g = torch.Generator(device=device).manual_seed(seed)
        self.targets = (torch.rand((n, C), device=device, generator=g) < 0.15).float().cpu().numpy()
        x1 = torch.randn((n, 3, hw, hw), device=device, generator=g)
        self._v = {"image": x1, "image_aug_1": x1,
                   "image_aug_2": x1 + 0.1 * torch.randn((n, 3, hw, hw), device=device, generator=g)}

    def __len__(self):
        return len(self.targets)

    def __getitem__(self, i):
        return {k: v[i] for k, v in self._v.items()} | {"target": self.targets[i].copy(), "index": i}

    def device_views(self, device):
        return self._v


class ShardedTestSet:
    """The synthetic test set of --eval_every: generated in fixed blocks of `bs` rows, block b from the seed (seed, b), so
    the data does not depend on the world size; the labels of every block are kept on the host (they are small), the images
    of the blocks b % world == rank in HBM.  With world = 1 it is a whole dataset (globaltest takes it)."""

    def __init__(self, n, C, hw, seed, bs, rank, world, device, p_pos=0.3):
        self.bs, self.rank, self.world = int(bs), rank, world
        self.blocks, targets = {}, []
        for b, i in enumerate(range(0, n, self.bs)):
            rows = min(self.bs, n - i)
            g = torch.Generator().manual_seed(int(seed) * 1000003 + b)
            targets.append((torch.rand((rows, C), generator=g) < p_pos).float().numpy())
            if b % world == rank:
                gd = torch.Generator(device=device).manual_seed(int(seed) * 1000003 + b)
                self.blocks[b] = torch.randn((rows, 3, hw, hw), device=device, generator=gd)
        self.targets = np.concatenate(targets, 0)

    def __len__(self):
        return len(self.targets)

    def block_of(self, rows):
        """the images of the consecutive rows `rows`, which are one of this rank's blocks"""
        x = self.blocks[rows[0] // self.bs]
        assert rows[0] % self.bs == 0 and len(rows) == x.shape[0]
        return x

    def __getitem__(self, i):
        return {"image": self.blocks[i // self.bs][i % self.bs], "target": self.targets[i].copy(), "index": i}

    def device_views(self, device):
        assert self.world == 1, "a shard is not a whole dataset"
        if getattr(self, "_v", None) is None:
            self._v = {"image": torch.cat([self.blocks[b] for b in sorted(self.blocks)], 0)}
        return self._v


def evaluate_sharded(net, eng, test, C, rank, world, dev):
    """globaltest of the engine's resident model on a ShardedTestSet: every rank forwards its blocks, one all-reduce
    completes the [n, C] probabilities, fm_eval_metrics ranks them -> main.py:326-331's seven numbers as floats."""
    from fedmlp_amd.evaluations import multilabel_metrics_device, sharded_probs
    was = net.training
    net.eval()
    probs = sharded_probs(lambda rows: net(test.block_of(rows))[1], len(test), C, rank, world, test.bs, dev)
    net.train(was)
    targets = torch.from_numpy(np.ascontiguousarray(test.targets, dtype=np.float32)).to(dev)
    return {k: float(v) for k, v in multilabel_metrics_device(eng, targets, probs).items()}


class RoundAccumulator:
    """One round's aggregation (main.py:216-234: FedAvg, FedAvg_tao, FedAvg_proto) split over ranks.  A rank that trains
    several clients folds them first -- state and counters with the weights n_c / sum(n), tao / prototype numerators
    with n_c per class the client misses / annotates -- then every sum over ranks is ONE all-reduce
    (fedmlp_amd/fedavg.py: the library's RCCL communicator, or torch.distributed).  With one rank it reproduces the
    reference's single-process loop; the world-2 gloo test pins both against utils/FedAvg.py's surface."""

    def __init__(self, state_like, n_counters, C, D, n_total):
        self.acc = torch.zeros_like(state_like)
        self.acc_cnt = np.zeros(n_counters, np.float64)
        self.C, self.n_total = C, float(n_total)
        self.t = np.zeros(C); self.tn = np.zeros(C)              # FedAvg_tao numerators / weights of this rank
        self.p = torch.zeros((2 * C, D)); self.pn = np.zeros(C)  # FedAvg_proto numerators / weights

    def add(self, n_c, state, counters, active_class_list, t=None, proto=None):
        """t, proto: what a prototype pass of train_FedMLP returned for this client (else None)"""
        w = n_c / self.n_total
        self.acc.add_(state, alpha=w)                            # FedAvg numerator (utils/FedAvg.py:9-13)
        self.acc_cnt += w * np.asarray(counters, np.float64)
        if t is not None:
            neg = np.array([0.0 if k in active_class_list else 1.0 for k in range(self.C)])
            act = 1.0 - neg
            self.t += np.asarray(t) * n_c * neg; self.tn += n_c * neg
            pa = np.repeat(act, 2)
            self.p += torch.where(torch.from_numpy(pa > 0)[:, None], torch.as_tensor(proto) * n_c, torch.zeros(()))
            self.pn += n_c * act

    def reduce(self, eng, dev, with_tao_proto, scale=1.0):
        """-> (global num_batches_tracked counters, tao or None, Prototype or None); the averaged state is in the engine.
        scale: a factor common to every rank applied to the sums (CBAFed's 1 / sum(data_num)); cnt_float keeps the
        counters' means before their truncation."""
        from fedmlp_amd.fedavg import fedavg_allreduce, tao_allreduce, proto_allreduce, state_agreement, trunc_counters
        eng.state_tensor().copy_(self.acc)
        eng.counters(np.zeros(len(self.acc_cnt), np.int64))      # the counters are reduced as float64 below
        fedavg_allreduce(eng, scale)                             # fm_fedavg_allreduce: ncclAllReduce of the state arena
        agree, worst = state_agreement(eng)                      # every rank starts the next round from the same w_glob
        if not agree:
            raise RuntimeError(f"the ranks' states differ after the FedAvg all-reduce (checksum spread {worst:.3e})")
        self.cnt_float = rank_sum(self.acc_cnt, dev) * scale
        cnt = trunc_counters(self.cnt_float)
        eng.counters(cnt)
        if not with_tao_proto:
            return cnt, None, None
        # FedAvg_tao / FedAvg_proto (utils/FedAvg.py:51-93): this rank enters with its folded clients' means and, per
        # class, the weight sum(n_c) of its clients that miss / annotate the class
        with np.errstate(invalid="ignore", divide="ignore"):
            t_rank = np.where(self.tn > 0, self.t / np.where(self.tn > 0, self.tn, 1.0), 0.0)
            p_rank = self.p.numpy() / np.repeat(np.where(self.pn > 0, self.pn, 1.0), 2)[:, None].astype(np.float32)
        tao = tao_allreduce(t_rank, 1.0, self.tn, device=dev, engine=eng)
        proto = proto_allreduce(p_rank, 1.0, self.pn, device=dev, engine=eng)
        return cnt, tao, proto


def main(args=None, module="fedmlp_amd.driver"):
    """args: a parsed namespace (default: args_parser() of the command line); module: what a multi-GPU run starts per rank"""
    if args is None:
        args = args_parser()
    from fedmlp_amd.launch import launched_by_torchrun, spawn_ranks
    if args.gpus > 1 and not launched_by_torchrun():
        import sys
        sys.exit(spawn_ranks(module, sys.argv[1:], args.gpus, module=True))
    rank = int(os.environ.get("RANK", "0")); world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # every RNG the flow draws from (batch orders: torch; class draws: random; numpy) is seeded like main.py seeds its
    # process, offset by the rank: a run is reproducible bit for bit
    import random
    random.seed(args.seed + rank); np.random.seed(args.seed + rank)
    torch.manual_seed(args.seed + rank); torch.cuda.manual_seed_all(args.seed + rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=dev)
    from fedmlp_amd import spec
    from fedmlp_amd.engine import Engine
    from fedmlp_amd.model import ResidentNet, build_model
    from fedmlp_amd.local_training import LocalUpdate
    from fedmlp_amd.fedavg import comm_init

    C = args.n_classes
    args.feature_dim = args.feature_dim or spec.FEATURE_DIM[args.model]
    eng = Engine(args.model, C, args.hw, args.hw, 4 * args.batch_size, device=str(dev), precision=args.precision,
                 streams=args.streams)
    try:
        comm_init(eng)                                    # the library's own RCCL communicator (C ABI)
    except Exception as ex:                               # noqa: BLE001  (then torch.distributed carries the sums)
        print(f"[driver] fm_comm_init failed ({ex}); using torch.distributed all_reduce", flush=True)
    # netglob = build_model(args) (main.py:73): from-scratch init, an ImageNet checkpoint, or --init_ckpt
    host = build_model(args)
    if args.init_ckpt:
        host.load_state_dict(torch.load(args.init_ckpt, map_location="cpu"))
    host._pull()
    eng.set_state(host.flat, host.counters)
    net = ResidentNet(eng)

    mine = [c for c in range(args.n_clients) if c % world == rank]
    n_all = [args.n_local] * args.n_clients
    row = ROWS[args.exp](args, eng, n_all, rank, world, dist, dev)
    clients = {}
    for c in mine:                                       # client c annotates class c mod C
        if args.augment:
            ds = AugmentedDeviceDataset(args.n_local, C, args.hw, args.seed + 1000 * c, dev, strong=args.augment == 2)
        else:
            ds = DeviceDataset(args.n_local, C, args.hw, args.seed + 1000 * c, dev)
        pos = [np.where(ds.targets[:, k] == 1)[0] for k in range(C)]
        a = argparse.Namespace(**vars(args))
        ema = build_model(args) if row.client_ema else None          # the client's own EMA model
        clients[c] = LocalUpdate(a, c % C, ds, list(range(args.n_local)), pos, pos, active_class_list=[c % C], teacher_neg=ema)
    # client-drift correction (fedmlp_amd/drift.py), installed by the trainers of DRIFT_EXPS around their local steps
    scaffold = None
    if args.scaffold:
        from fedmlp_amd.drift import Scaffold
        scaffold = Scaffold(eng.nf, args.n_clients, dev)
        for c in mine:
            clients[c].drift = scaffold.client(c)
    elif args.prox_mu > 0:
        from fedmlp_amd.drift import FedProx
        for c in mine:
            clients[c].drift = FedProx(args.prox_mu)
    test = None
    if args.eval_every > 0:                              # its own seed: no client's data (seed + 1000 c) is the test set
        test = ShardedTestSet(args.n_test, C, args.hw, args.seed + 500, 4 * args.batch_size, rank, world, dev)
    # server optimizer (fedmlp_amd/server_opt.py): one launch on the aggregated model per round, the same on every rank
    server = None
    if args.server_opt != "none":
        from fedmlp_amd import server_opt
        server = server_opt.make(args.server_opt, args.server_lr, args.server_beta1, args.server_beta2, args.server_tau)
        if args.init_server_opt:                          # the file's hyper-parameters win: a flag that says otherwise is refused
            saved = torch.load(args.init_server_opt, map_location="cpu")
            asked = server.hyper()
            for flag, key in (("server_lr", "lr"), ("server_beta1", "beta1"), ("server_beta2", "beta2"), ("server_tau", "tau")):
                if getattr(args, flag) is not None and asked[key] != float(saved["hyper"][key]):
                    raise SystemExit(f"--{flag} {getattr(args, flag)} contradicts {args.init_server_opt}, which was saved with "
                                     f"{key} = {saved['hyper'][key]}: drop the flag or start a fresh optimizer")
            server.load_state_dict(saved)
        server.begin(eng)
    log = run_rounds(args, row, eng, net, clients, rank, world, dev, test=test, scaffold=scaffold, server=server)
    if server is not None:
        server.end(eng)
    if dist is not None:
        dist.barrier(); dist.destroy_process_group()
    return log


def run_rounds(args, row, eng, net, clients, rank, world, dev, test=None, scaffold=None, server=None):
    """The loop over rounds (main.py:106-357) for one row (fedmlp_amd/rows.py) on this rank's clients {c: LocalUpdate}, from the
    global model the engine holds -> the per-round records (rank 0 prints them).  Nothing here needs a GPU of its own: with
    stand-ins for the engine and the clients it runs on the CPU.  server: a fedmlp_amd.server_opt optimizer installed on the
    engine (or None): its step turns the round's aggregate into the new global model."""
    sync = torch.cuda.synchronize if torch.device(dev).type == "cuda" else (lambda: None)
    C = args.n_classes
    glob = eng.state_tensor().clone()                     # netglob, replicated on every rank
    glob_cnt = eng.counters().copy()                      # its num_batches_tracked counters
    log = []
    for rnd in range(args.rounds_warmup):
        t0 = time.perf_counter()
        acc = RoundAccumulator(glob, len(glob_cnt), C, args.feature_dim, row.fedavg_total(rnd))
        losses = []
        row.begin_round(rnd)
        for c, loc in clients.items():
            eng.state_tensor().copy_(glob)                # net = deepcopy(netglob)  (main.py:181-184)
            eng.counters(glob_cnt)
            ret = row.train(rnd, c, loc, net)
            losses.append(float(ret[1]))
            row.contribute(rnd, acc, c, loc, ret)
        # aggregation (main.py:213-319): every sum over clients is an RCCL all-reduce in the library
        glob_cnt = row.aggregate(rnd, acc)
        delta_norm = None
        if server is not None:                            # x' from the pseudo-gradient aggregate - glob; every rank the same bits
            from fedmlp_amd.fedavg import state_agreement
            delta_norm = server.step(eng, glob)
            agree, worst = state_agreement(eng)
            if not agree:
                raise RuntimeError(f"the ranks' states differ after the server optimizer's step (checksum spread {worst:.3e})")
        glob.copy_(eng.state_tensor())
        if scaffold is not None:                          # c += sum_i delta c_i / n_clients; the models went through FedAvg above
            scaffold.server_update()
        row.end_round(rnd)
        metrics = None
        if test is not None and (rnd + 1) % args.eval_every == 0:     # globaltest of the new netglob (main.py:322-331)
            sync()
            t1 = time.perf_counter()
            metrics = evaluate_sharded(net, eng, test, C, rank, world, dev)
            eval_sec = time.perf_counter() - t1
        sync()
        dt = time.perf_counter() - t0
        rec = {"round": rnd, "sec": round(dt, 3), "mean_loss": float(np.mean(losses)) if losses else None,
               "samples_per_sec_per_gpu": round(len(clients) * args.n_local / dt, 1)}
        if metrics is not None:
            rec["test"] = metrics
            rec["eval_sec"] = round(eval_sec, 3)
        if scaffold is not None:
            rec["scaffold"] = {"c_norm": float(scaffold.c_global.double().norm())}
        elif args.prox_mu > 0:
            rec["prox_mu"] = args.prox_mu
        if server is not None:
            rec["server_opt"] = {"rule": server.rule, "step": int(server.steps), "delta_norm": float(delta_norm)}
        if rank == 0:
            print(json.dumps(rec), flush=True)
            if args.save_every and (rnd + 1) % args.save_every == 0:     # torch.save(netglob.state_dict(), ...) main.py:237
                torch.save(net.state_dict(), os.path.join(args.save_dir, f"model_{rnd}.pth"))
                if server is not None:
                    torch.save(server.state_dict(), os.path.join(args.save_dir, f"server_opt_{rnd}.pth"))
        log.append(rec)
    return log


def rscfed_round(eng, DMA, states, counters, n_all, rank, world, dist):
    """main.py:213-215 on the device: RSCFed (utils/FedAvg.py:25-41) over every client's engine-layout state.  One rank: the
    clients' DeviceStates through fedavg.RSCFed.  More ranks: the states are all-gathered and every rank runs the same
    rscfed_device, so all of them hold the same global model (checked).  The float counters are truncated on load.
    Leaves the result in the engine; -> its int64 counters."""
    from fedmlp_amd import fedavg
    n_clients = len(n_all)
    if dist is None:
        w_locals = [fedavg.DeviceState(eng, states[c], counters[c]) for c in range(n_clients)]
        agg = fedavg.RSCFed(DMA, w_locals, RSCFED_K, n_all, RSCFED_M)
        st, cnt_f = agg.tensor, agg.counters
    else:
        all_s, all_c = gather_client_states(eng, states, counters, n_clients, rank, world, dist)
        st, cnt_f = fedavg.rscfed_device(eng, all_s, np.stack(all_c), DMA, n_all)
    eng.state_tensor().copy_(st)
    cnt = fedavg.trunc_counters(cnt_f)
    eng.counters(cnt)
    agree, worst = fedavg.state_agreement(eng)
    if not agree:
        raise RuntimeError(f"the ranks' states differ after the RSCFed aggregation (checksum spread {worst:.3e})")
    return cnt


def rank_sum(x, dev):
    """float64 sum of a small host vector over the ranks"""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return np.asarray(x, np.float64)
    t = torch.from_numpy(np.asarray(x, np.float64)).to(dev)
    dist.all_reduce(t)
    return t.cpu().numpy()


if __name__ == "__main__":
    main()
