#!/usr/bin/env python3
"""Known answers for RoFL, produced by THE REFERENCE'S OWN LocalUpdate.get_small_loss_samples, RFLloss and train_RoFL
(utils/local_training.py:466-626) on the CPU, with `.cuda()` made the identity as make_golden.py does.  The methods are called on
an instance made without the constructor and given the attributes they read.
  * the two functions on fixed float64 inputs, B = 8, C = 5 (the class count train_RoFL hard-codes in its mask), D = 16: the
    kept rows and the mutated loss_w; RFLloss at an epoch inside the lambda_cen ramp and at one past T_pl;
  * one whole train_RoFL call each at epoch 0 and at epoch = T_pl (with a given f_G): 20 samples in batches of 8, 8 and 4, a
    stand-in net (12 inputs -> tanh(Linear) feature of 16 -> Linear logits) whose initial weights are recorded; per-step losses
    (RFLloss's return values), the pseudo-label table after every step, the final f_k and the final weights.
The inputs keep the small-loss boundary away from a tie (the functions': asserted here; the trainer's boundaries and centroid
votes: tests/test_rofl_cpu.py asserts their margins in float64).
Writes tests/golden/rofl_kat.npz.
usage: python tests/golden/make_rofl_golden.py /path/to/reference"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_irm_lsr_golden import import_with_stubs      # noqa: E402

B, C, D, DIN, N = 8, 5, 16, 12, 20
ACTIVE = [2]
LOSS_W = [2.5, 1.5, 3.0, 1.25, 2.0]
T_PL, LAMBDA_CEN, LAMBDA_E, FORGET, LR = 4, 1.0, 0.8, 0.2, 1e-3


def args():
    return types.SimpleNamespace(n_classes=C, feature_dim=D, device="cpu", batch_size=B, local_ep=1, forget_rate=FORGET,
                                 T_pl=T_PL, lambda_cen=LAMBDA_CEN, lambda_e=LAMBDA_E, annotation_num=len(ACTIVE))


class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.body = torch.nn.Linear(DIN, D)
        self.fc = torch.nn.Linear(D, C)

    def forward(self, x):
        f = torch.tanh(self.body(x))
        return f, self.fc(f)


def function_inputs():
    rs = np.random.RandomState(466)
    z = rs.uniform(-4, 4, (B, C))
    y = (rs.rand(B, C) < 0.4).astype(np.float64)
    feat = rs.standard_normal((B, D))
    f_k = rs.standard_normal((2 * C, D))
    mask = np.array([1, 0, 1, 1, 0, 1, 0, 1], np.float64)
    new = (rs.rand(B, C) < 0.5).astype(np.float64)
    return z, y, feat, f_k, mask, new


def train_inputs():
    rs = np.random.RandomState(583)
    x = rs.standard_normal((N, DIN)).astype(np.float32)
    y = (rs.rand(N, C) < 0.4).astype(np.float32)
    f_G = rs.standard_normal((2 * C, D)).astype(np.float32)
    return x, y, f_G


def main():
    ref = sys.argv[1]
    sys.path.insert(0, ref)
    torch.set_num_threads(1)
    torch.Tensor.cuda = lambda self, *a, **k: self
    LT = import_with_stubs("utils.local_training")
    t = torch.from_numpy
    out = {}

    # ---- the two functions, float64 ----
    z, y, feat, f_k, mask, new = function_inputs()
    lu = LT.LocalUpdate.__new__(LT.LocalUpdate)
    lu.args = args()
    lu.loss_w = list(LOSS_W)
    neg = [c for c in range(C) if c not in ACTIVE]
    idx, lw = lu.get_small_loss_samples(t(z), t(y), FORGET, neg)
    assert lw is lu.loss_w and idx.numel() == int((1 - FORGET) * B)
    w = torch.tensor(lw, dtype=torch.float64)
    key = torch.nn.functional.binary_cross_entropy_with_logits(t(z), t(y), pos_weight=w, reduction="none").sum(1).sort().values
    assert float(key[idx.numel()] - key[idx.numel() - 1]) > 1e-3 * float(key[idx.numel()])
    out.update(fn_z=z, fn_y=y, fn_feat=feat, fn_fk=f_k, fn_mask=mask, fn_new=new, fn_loss_w_in=np.asarray(LOSS_W),
               fn_kept=np.sort(idx.numpy()).astype(np.int64), fn_loss_w_out=np.asarray(lw, np.float64))
    for name, epoch in (("ramp", 3), ("flat", T_PL + 2)):
        val = lu.RFLloss(t(z), t(y), t(feat), t(f_k), t(mask), idx, t(new)[idx], lw, epoch)
        assert val.dtype == torch.float64
        out["fn_rfl_" + name] = val.numpy()
        out["fn_epoch_" + name] = np.int64(epoch)

    # ---- train_RoFL, fp32 like the real loop ----
    x, yt, f_G = train_inputs()
    torch.manual_seed(11)
    net0 = Net()
    out.update(tr_x=x, tr_y=yt, tr_fG=f_G, **{"tr_w0_" + k: v.numpy().copy() for k, v in net0.state_dict().items()})
    order = list(range(N))
    batches = [order[i:i + B] for i in range(0, N, B)]
    act = [torch.tensor([c] * B) for c in ACTIVE]
    for name, epoch in (("e0", 0), ("eT", T_PL)):
        net = Net()
        net.load_state_dict(net0.state_dict())
        lu = LT.LocalUpdate.__new__(LT.LocalUpdate)
        lu.args = args()
        lu.loss_w = list(LOSS_W)
        lu.lr = LR
        lu.dataset = order
        lu.ldr_train = [({"image": t(x[b]), "target": t(yt[b])}, torch.tensor(b), act) for b in batches]
        losses, tables = [], []
        inner = lu.RFLloss

        def spy(*a, inner=inner, losses=losses, tables=tables):
            r = inner(*a)
            losses.append(float(r.detach()))
            tables.append(sys._getframe(1).f_locals["pseudo_labels"].clone().numpy())
            return r
        lu.RFLloss = spy
        sd, mean, fk = lu.train_RoFL(net, t(f_G.copy()), epoch)
        assert len(losses) == len(batches) and abs(mean - sum(losses) / len(losses)) < 1e-12
        tab = np.stack(tables)
        assert set(np.unique(tab)) <= {0.0, 1.0}
        out.update({f"tr_{name}_epoch": np.int64(epoch), f"tr_{name}_losses": np.asarray(losses, np.float64),
                    f"tr_{name}_tables": tab.astype(np.uint8), f"tr_{name}_fk": fk.detach().numpy(),
                    f"tr_{name}_loss_w": np.asarray(lu.loss_w, np.float64)})
        out.update({f"tr_{name}_w_{k}": v.numpy().copy() for k, v in sd.items()})
    path = os.path.join(HERE, "rofl_kat.npz")
    np.savez(path, **out)
    print("wrote rofl_kat.npz:", os.path.getsize(path), "bytes; kept =", out["fn_kept"].tolist(),
          "losses e0 =", out["tr_e0_losses"].tolist())


if __name__ == "__main__":
    main()
