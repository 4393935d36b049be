"""The rows of the reference's main.py (:106-319) as objects: one class per --exp value, each holding what its row carries from
round to round and from training to aggregation.  fedmlp_amd.driver.run_rounds asks a row, per round,

  begin_round(rnd)                 the round's draws, before any client trains
  train(rnd, c, loc, net) -> ret   the row's one LocalUpdate.train_* call for client c
  fedavg_total(rnd)                the denominator of the round's FedAvg weights
  contribute(rnd, acc, c, loc, ret)  client c's trained state (in the engine) into the round's RoundAccumulator
  aggregate(rnd, acc) -> counters  the new global model into the engine
  end_round(rnd)                   what the row derives from the clients' returns once the global model stands

and Row itself is plain FedAvg of every client by n_all[c].  ROWS maps the --exp strings to the classes; the parser's choices and
DRIFT_EXPS are read from it.  fedavg.* and driver.rscfed_round are looked up when called (tests wrap them)."""
import random

import torch

from fedmlp_amd import fedavg

RSCFED_M, RSCFED_K = 10, 6         # main.py:115-116: M groups of K clients per round


class Row:
    trains_with_drift = False      # its trainer installs LocalUpdate.drift (--prox_mu / --scaffold)
    client_ema = False             # every client gets its own build_model(args) as teacher_neg

    def __init__(self, args, eng, n_all, rank, world, dist, dev):
        self.args, self.eng, self.n_all = args, eng, n_all
        self.rank, self.world, self.dist, self.dev = rank, world, dist, dev
        self.n_clients = len(n_all)

    def begin_round(self, rnd):
        pass

    def train(self, rnd, c, loc, net):
        raise NotImplementedError

    def fedavg_total(self, rnd):
        return float(sum(self.n_all))

    def contribute(self, rnd, acc, c, loc, ret):
        acc.add(self.n_all[c], self.eng.state_tensor(), self.eng.counters(), loc.active_class_list)

    def aggregate(self, rnd, acc):
        return acc.reduce(self.eng, self.dev, with_tao_proto=False)[0]

    def end_round(self, rnd):
        pass


class FedAVG(Row):
    trains_with_drift = True

    def train(self, rnd, c, loc, net):
        return loc.train(rnd, net, None)


class FixMatch(Row):
    trains_with_drift = True

    def train(self, rnd, c, loc, net):
        return loc.train_FixMatch(rnd, net)


class FedMLP(Row):
    trains_with_drift = True

    def __init__(self, *a):
        super().__init__(*a)
        self.S1 = self.args.rounds_FedMLP_stage1
        self.tao, self.Prototype = [0] * self.args.n_classes, None

    def train(self, rnd, c, loc, net):
        if rnd < self.S1 - 1:
            return loc.train_FedMLP(rnd, self.tao, self.Prototype, None, None, None, net=net)
        return loc.train_FedMLP(rnd, self.tao, self.Prototype, None, loc.negative_class_list, loc.active_class_list, net=net)

    def contribute(self, rnd, acc, c, loc, ret):
        t, proto = (ret[6], ret[7]) if rnd >= self.S1 - 1 else (None, None)    # a prototype pass returns (..., t, proto)
        acc.add(self.n_all[c], self.eng.state_tensor(), self.eng.counters(), loc.active_class_list, t, proto)

    def aggregate(self, rnd, acc):
        cnt, tao, proto = acc.reduce(self.eng, self.dev, with_tao_proto=rnd >= self.S1 - 1)
        if tao is not None:                                        # read by the next round's clients
            self.tao, self.Prototype = tao, proto
        return cnt


class FedLSR(Row):
    def train(self, rnd, c, loc, net):                             # main.py:161-163
        return loc.train_FedLSR(rnd, net)


class FedIRM(Row):
    client_ema = True              # main.py hands LocalUpdate a teacher_neg (:31, 393-395)

    def __init__(self, *a):
        super().__init__(*a)
        self.SI, self.Prototype = self.args.rounds_FedIRM_sup, None
        C = self.args.n_classes
        # main.py:200-208: class k is annotated by the clients c with c mod C == k (every rank knows the whole assignment)
        self.class_active_client_list = [[c for c in range(self.n_clients) if c % C == k] for k in range(C)]

    def begin_round(self, rnd):
        self.relas = {}                                            # client -> its relation matrix (host), main.py:192-193

    def train(self, rnd, c, loc, net):                             # main.py:169-177
        if rnd < self.SI - 1:
            return loc.train_FedIRM(rnd, self.Prototype, None, None, None, net=net)
        ret = loc.train_FedIRM(rnd, self.Prototype, None, loc.negative_class_list, loc.active_class_list, net=net)
        self.relas[c] = ret[6].detach().cpu()
        return ret

    def end_round(self, rnd):                                      # main.py:245-251: FedAvg_rela with lam = 1
        if rnd < self.SI - 1:
            return
        relas = fedavg.gather_dicts(self.dist, self.relas)         # C x C floats per client, folded on every rank alike
        rela = fedavg.FedAvg_rela([relas[c] for c in range(self.n_clients)], self.n_all, self.class_active_client_list)
        if rnd == self.SI - 1:
            self.Prototype = rela
        else:
            lam = 1.0
            self.Prototype = (1 - lam) * self.Prototype + lam * rela


class RSCFed(Row):
    client_ema = True              # main.py:164-166: train_RSCFed blends into the client's own teacher_neg

    def __init__(self, *a):
        super().__init__(*a)
        # ONE generator seeded without the rank offset and stepped alike on every rank: the same DMA everywhere
        self.rng = random.Random(self.args.seed)

    def begin_round(self, rnd):                                    # main.py:114-121
        self.DMA = [self.rng.sample(range(self.n_clients), RSCFED_K) for _ in range(RSCFED_M)]
        self.states, self.counters = {}, {}                        # client -> device state / counters

    def train(self, rnd, c, loc, net):
        return loc.train_RSCFed(rnd, net)

    def contribute(self, rnd, acc, c, loc, ret):
        self.states[c], self.counters[c] = self.eng.state_tensor().clone(), self.eng.counters().copy()

    def aggregate(self, rnd, acc):                                 # main.py:213-215
        from fedmlp_amd import driver
        return driver.rscfed_round(self.eng, self.DMA, self.states, self.counters, self.n_all, self.rank, self.world, self.dist)


class FedNoRo(Row):
    def begin_round(self, rnd):                                    # main.py:127-128
        self.weight_kd = fedavg.consistency_weight(rnd, self.args.begin, self.args.end) * self.args.a

    def train(self, rnd, c, loc, net):                             # main.py:140-144
        return loc.train_FedNoRo(c, rnd, net, None, weight_kd=self.weight_kd)


class CBAFed(Row):
    def __init__(self, *a):
        super().__init__(*a)
        self.WC = self.args.rounds_CBAFed_warmup
        self.pt = self.tao = None                                  # main.py:289-300
        self.res = self.res_cnt = None                             # the last blended model (w_glob_res) and its float counters

    def begin_round(self, rnd):
        self.counts = {}                                           # client -> (class_num_list, data_num)

    def train(self, rnd, c, loc, net):                             # main.py:149-157
        ret = loc.train_CBAFed(rnd, net) if rnd < self.WC else loc.train_CBAFed(rnd, net, pt=self.pt, tao=self.tao)
        self.counts[c] = (ret[6].clone(), int(ret[7]))
        return ret

    # stage 2: FedAvg weights data_num_c / sum(data_num), main.py:302.  The sum is known only after every client trained:
    # accumulate with the raw data_num, scale the all-reduce by 1 / sum
    def fedavg_total(self, rnd):
        return super().fedavg_total(rnd) if rnd < self.WC else 1.0

    def contribute(self, rnd, acc, c, loc, ret):
        n_c = self.n_all[c] if rnd < self.WC else self.counts[c][1]
        acc.add(n_c, self.eng.state_tensor(), self.eng.counters(), loc.active_class_list)

    def aggregate(self, rnd, acc):
        eng = self.eng
        self.counts = fedavg.gather_dicts(self.dist, self.counts)  # every client's class_num_list / data_num on every rank
        scale = 1.0 if rnd < self.WC else 1.0 / float(sum(self.counts[c][1] for c in range(self.n_clients)))
        cnt = acc.reduce(eng, self.dev, with_tao_proto=False, scale=scale)[0]
        w_new, w_res, store = fedavg.cbafed_blend(rnd, self.WC)    # main.py:274-288, 303-316
        cnt_f = acc.cnt_float
        if w_res != 0.0:
            # two rounded products, then their sum: the reference's 0.2 * w + 0.8 * res (no fused multiply-add)
            eng.state_tensor().mul_(w_new).add_(self.res * w_res)
            cnt_f = w_new * cnt_f + w_res * self.res_cnt           # the counters follow the blend in float ...
            cnt = fedavg.trunc_counters(cnt_f)                     # ... and are truncated on load
            eng.counters(cnt)
        if store:
            self.res, self.res_cnt = eng.state_tensor().clone(), cnt_f
        return cnt

    def end_round(self, rnd):                                      # main.py:289-300
        if rnd >= self.WC - 1:
            order = range(self.n_clients)
            self.pt, self.tao = fedavg.cbafed_tao([self.counts[c][0] for c in order], [self.counts[c][1] for c in order])


class RoFL(Row):
    def __init__(self, *a):
        super().__init__(*a)
        # the global centroids (main.py:99) from a CPU generator seeded without the rank offset: the same f_G on every rank
        self.f_G = torch.randn((2 * self.args.n_classes, self.args.feature_dim),
                               generator=torch.Generator().manual_seed(self.args.seed))

    def begin_round(self, rnd):
        self.f_locals = {}                                         # client -> its centroids f_k (host)

    def train(self, rnd, c, loc, net):                             # main.py:167-168
        ret = loc.train_RoFL(net, self.f_G, rnd)
        self.f_locals[c] = ret[2]
        return ret

    def end_round(self, rnd):                                      # main.py:253-268: the centroids' cosine-weighted fold
        f_locals = fedavg.gather_dicts(self.dist, self.f_locals)   # 2C x D floats per client, folded on every rank alike
        self.f_G = fedavg.rofl_centroids(self.f_G, [f_locals[c] for c in range(self.n_clients)])


# RoFL is the branch main.py keeps commented out: fedmlp_amd.driver's parser leaves it out, fedmlp_amd.driver_rofl is its command
ROWS = {"FedAVG": FedAVG, "FedAVG+FixMatch": FixMatch, "FedMLP": FedMLP, "FedLSR": FedLSR, "FedIRM": FedIRM, "RSCFed": RSCFed,
        "FedNoRo": FedNoRo, "CBAFed": CBAFed, "RoFL": RoFL}
