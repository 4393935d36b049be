"""Per-step time of the RoFL step two ways, with the plain BCE step beside them, ResNet-18 at bs 128 x 224^2, stream mode 0 by
default, measured alternately in one process:
  rofl_split   Engine.forward_train(x), the head in torch the way a user of the split path would write it today -- per-sample
               losses sorted on the host (numpy argsort of loss.cpu()), Python loops over the kept samples x classes for the
               centroid votes (a cosine and an argmax per class, torch.equal per sample), the loss with autograd, loops again
               for the centroid sums -- then Engine.backward_step
  rofl_fused   Engine.step_rofl (fm_step_rofl): one call, no host read
  bce          Engine.step_bce: the plain one-view fused step, the yardstick
and `head`: Engine.loss_rofl alone (its three launches) on saved logits and features, device events around `--steps` calls.
Device events around `--steps` steps after `--warmup`, repeated `--reps` times alternating the arms; prints one JSON line (median
and spread of the repetitions, ms per step) and, with --out, writes it to that file.  --arms a,b runs only those."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fedmlp_amd import spec  # noqa: E402
from fedmlp_amd.engine import Engine  # noqa: E402

ARMS = ("rofl_split", "rofl_fused", "bce", "head")


def torch_head(z, feat, y, item, n_keep, pw, lam_cen, lam_e, write_labels, f_k, pseudo):
    """-> (loss, dz, new f_k); pseudo (float [N, C]) is updated in place.  Host sort and Python loops, on purpose."""
    B, C = y.shape
    D = feat.shape[1]
    sim = torch.nn.CosineSimilarity(dim=1)
    zl = z.detach().requires_grad_(True)
    w = torch.tensor(pw, device=z.device)
    per_row = torch.nn.functional.binary_cross_entropy_with_logits(zl, y, pos_weight=w, reduction="none").sum(1)
    kept = torch.from_numpy(np.argsort(per_row.detach().cpu().numpy(), kind="stable")[:n_keep]).to(z.device)     # host read
    vote = torch.zeros((B, C), device=z.device)
    mask = torch.zeros(B, device=z.device)
    for i in kept:
        for c in range(C):
            vote[i, c] = torch.argmax(sim(f_k[2 * c:2 * c + 2], feat[i].reshape(1, D)))
        if torch.equal(vote[i], y[i]):
            mask[i] = 1
    if write_labels:
        for i in kept:
            pseudo[item[i]] = y[i]
    m = mask[kept].unsqueeze(1)
    new = m * y[kept] + (1 - m) * pseudo[item[kept].long()]
    L_c = torch.nn.functional.binary_cross_entropy_with_logits(zl[kept], new, pos_weight=w)
    L_cen = 0.0
    for c in range(C):
        own = f_k[(2 * c + y[kept, c]).long()]
        L_cen = L_cen + (mask[kept] * ((feat[kept] - own) ** 2).sum(1)).sum() / (n_keep * D)
    L_cen = L_cen / C
    zk = zl[kept]
    L_e = (torch.nn.functional.softplus(zk) - zk * torch.sigmoid(zk)).sum() / (n_keep * C)
    loss = L_c + lam_cen * L_cen + lam_e * L_e
    (dz,) = torch.autograd.grad(loss, zl)
    fh = torch.zeros_like(f_k)
    cnt = torch.zeros((2 * C, 1), device=z.device)
    for i in kept:
        for c in range(C):
            r = 2 * c + int(y[i, c])                                                          # host read
            fh[r] += feat[i]
            cnt[r] += 1
    fh = fh / torch.where(cnt == 0, torch.ones_like(cnt), cnt)
    s2 = sim(f_k, fh).reshape(-1, 1) ** 2
    return loss.detach(), dz, (1 - s2) * f_k + s2 * fh


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--streams", type=int, default=0)
    ap.add_argument("--model", choices=["Resnet18", "Efficient_b0"], default="Resnet18")
    ap.add_argument("--arms", default="", help="comma list of arms to run (default: all)")
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rofl_time: needs a GPU")
    B, C, hw = a.batch, a.classes, a.hw
    eng = Engine(a.model, C, hw, hw, B, streams=a.streams)
    eng.stochastic = False
    eng.set_state(*spec.init_state(a.model, C, 1037))
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn((B, 3, hw, hw), device="cuda", generator=g)
    y = (torch.rand((B, C), device="cuda", generator=g) < 0.3).float()
    pw = [2.0] + [5.0] * (C - 1)
    n_keep = int((1 - 0.2) * B)
    N = 4 * B
    item = torch.randperm(N, device="cuda", generator=g)[:B].to(torch.int32)
    f0 = torch.randn((2 * C, eng.feature_dim), device="cuda", generator=g)
    p0 = (torch.rand((N, C), device="cuda", generator=g) < 0.5)
    st = {"f_split": f0.clone(), "p_split": p0.float(), "f_fused": f0.clone(), "p_fused": p0.to(torch.uint8),
          "f_head": f0.clone(), "p_head": p0.to(torch.uint8)}
    lo = torch.zeros(1, device="cuda")
    lam_cen, lam_e = 0.5, 0.8
    feat_s, z_s = (t.clone() for t in eng.forward_train(x))

    def rofl_split():
        feat, z = eng.forward_train(x)
        _, dz, st["f_split"] = torch_head(z, feat, y, item, n_keep, pw, lam_cen, lam_e, True, st["f_split"], st["p_split"])
        eng.backward_step(dz)

    def rofl_fused():
        eng.step_rofl(x, y, item, n_keep, pw, lam_cen, lam_e, True, st["f_fused"], st["p_fused"], lo)

    def bce():
        eng.step_bce(x, y, pw, B, lo)

    def head():
        eng.loss_rofl(z_s, feat_s, y, item, n_keep, pw, lam_cen, lam_e, True, st["f_head"], st["p_head"])

    fns = {"rofl_split": rofl_split, "rofl_fused": rofl_fused, "bce": bce, "head": head}
    arms = {k: fns[k] for k in (a.arms.split(",") if a.arms else ARMS)}
    times = {k: [] for k in arms}

    def prepare():
        eng.adam_reset(3e-5, (0.9, 0.999), 1e-8, 5e-4)      # every arm starts its window from a fresh optimizer

    for fn in arms.values():
        prepare()
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for k, fn in arms.items():
            prepare()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.steps):
                fn()
            t1.record()
            t1.synchronize()
            times[k].append(t0.elapsed_time(t1) / a.steps)
    out = {"model": a.model, "batch": B, "hw": hw, "classes": C, "n_keep": n_keep, "steps": a.steps, "reps": a.reps,
           "stream_mode": int(eng.lib.fm_stream_mode(eng.h))}
    for k in ARMS:
        v = times.get(k)
        out[k + "_ms"] = round(float(np.median(v)), 4) if v else None
        out[k + "_spread_ms"] = round(float(max(v) - min(v)), 4) if v else None
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
