"""RoFL (train_RoFL, RFLloss, get_small_loss_samples, the server's centroid fold) restated on torch tensors of any float dtype.

Written from the description of the method, generalised to any number of classes; pinned to the reference's own functions
at C = 5 by tests/golden/rofl_kat.npz (tests/test_rofl_cpu.py).  float64: the exact side of the GPU tests; float32: the
"torch-CPU fp32" yardstick of their bound.  The two stated deviations from the reference's arithmetic are the engine's too: the
entropy is softplus(z) - z sigmoid(z) (finite where fp32 p log p is NaN), and ties of the small-loss sort go to the lower row.
"""
import torch
import torch.nn.functional as F


def n_keep(forget_rate, B):
    """num_remember: Python double arithmetic, truncated"""
    return int((1 - forget_rate) * B)


def cosine(a, b):
    """row-wise a.b / (|a| |b|); exactly 0 where a norm is 0"""
    dot = (a * b).sum(-1)
    den = (a * a).sum(-1).sqrt() * (b * b).sum(-1).sqrt()
    return torch.where(den == 0, torch.zeros_like(dot), dot / torch.where(den == 0, torch.ones_like(den), den))


def row_loss(z, y, w):
    return F.binary_cross_entropy_with_logits(z, y, pos_weight=w, reduction="none").sum(1)


def kept_rows(loss, n):
    """bool [B]: the n rows of smallest loss; ties to the lower row, NaN last (torch's stable sort orders NaN above everything)"""
    keep = torch.zeros(loss.shape[0], dtype=torch.bool)
    keep[torch.sort(loss.detach(), stable=True).indices[:n]] = True
    return keep


def cos_table(feat, f_k):
    """[B, 2C]: cos(f_k[r], feat_i)"""
    return cosine(f_k[None, :, :], feat[:, None, :])


def votes(feat, f_k):
    """[B, C] in {0, 1}: argmax over (cos with f_k[2c], cos with f_k[2c + 1]); a tie gives 0"""
    t = cos_table(feat, f_k)
    return (t[:, 1::2] > t[:, 0::2]).to(feat.dtype)


def entropy(z):
    """binary entropy of sigmoid(z), formed from the logit: softplus(z) - z sigmoid(z)"""
    return F.softplus(z) - z * torch.sigmoid(z)


def rfl_loss(z, y, feat, f_k, mask, keep, new, w, lam_cen, lam_e):
    """RFLloss: keep, mask bool [B]; new [B, C] (read on the kept rows); lam_cen is the effective weight"""
    C, D = y.shape[1], feat.shape[1]
    n = int(keep.sum())
    kz = z[keep]
    L_c = F.binary_cross_entropy_with_logits(kz, new[keep], pos_weight=w, reduction="sum") / (n * C)
    own = f_k[2 * torch.arange(C)[None, :] + y.long()]                       # [B, C, D]: the centroid of the row's own label
    d2 = ((feat[:, None, :] - own) ** 2).sum(2)                              # [B, C]
    L_cen = (d2.sum(1) * (mask & keep).to(feat.dtype)).sum() / (n * D) / C
    L_e = entropy(kz).sum() / (n * C)
    return L_c + lam_cen * L_cen + lam_e * L_e


def head(z, feat, y, item, n, w, lam_cen, lam_e, write_labels, f_k, pseudo):
    """One batch (B.2 - B.6, B.8).  z may require grad; feat, f_k are constants.  pseudo: uint8 [N, C], not modified.
    -> dict: loss (differentiable in z), dz (the stated formula), keep, mask (bool [B]), pseudo (new table), f_k (new)"""
    B, C = y.shape
    item = item.long()
    feat, f_k = feat.detach(), f_k.detach()
    keep = kept_rows(row_loss(z, y, w), n)
    mask = keep & (votes(feat, f_k) == y).all(1)
    pseudo = pseudo.clone()
    if write_labels:
        pseudo[item[keep]] = y[keep].to(pseudo.dtype)
    new = torch.where(mask[:, None], y, pseudo[item].to(y.dtype))
    loss = rfl_loss(z, y, feat, f_k, mask, keep, new, w, lam_cen, lam_e)
    with torch.no_grad():
        zd = z.detach()
        p = torch.sigmoid(zd)
        q = torch.sigmoid(-zd)
        dz = ((1 - new) - (1 + (w - 1) * new) * q - lam_e * zd * p * q) / (n * C)
        dz = torch.where(keep[:, None], dz, torch.zeros_like(dz))
        f_new = centroid_update(feat, y, keep, f_k)
    return {"loss": loss, "dz": dz, "keep": keep, "mask": mask, "pseudo": pseudo, "f_k": f_new}


def centroid_update(feat, y, keep, f_k):
    """B.8: fh[2c + y_ic] = the kept rows' mean feature (a zero count divides by 1), s = cos(f_k, fh), the blend"""
    B, C = y.shape
    sel = torch.zeros((2 * C, B), dtype=feat.dtype)
    rows = torch.nonzero(keep).flatten()
    for c in range(C):
        sel[2 * c + y[rows, c].long(), rows] = 1
    cnt = sel.sum(1, keepdim=True)
    fh = (sel @ feat) / torch.where(cnt == 0, torch.ones_like(cnt), cnt)
    s2 = (cosine(f_k, fh) ** 2)[:, None]
    return (1 - s2) * f_k + s2 * fh


def margins(z, feat, y, n, w, f_k, every_row=False):
    """How far the batch's discrete decisions are from a tie, in float64: (the smallest |cos_0 - cos_1| over the kept rows'
    votes -- over every row's with every_row --, the gap of the per-row loss across the keep boundary relative to the loss
    above it; inf when every row is kept)"""
    z, feat, y, w, f_k = (t.detach().double() for t in (z, feat, y, w, f_k))
    loss = row_loss(z, y, w)
    keep = kept_rows(loss, n)
    t = cos_table(feat, f_k)
    vote = float((t[:, 1::2] - t[:, 0::2]).abs()[torch.ones_like(keep) if every_row else keep].min())
    srt = torch.sort(loss).values
    gap = float("inf") if n >= len(srt) else float((srt[n] - srt[n - 1]) / srt[n].abs())
    return vote, gap


def lambda_cen_eff(lambda_cen, epoch, T_pl):
    return (lambda_cen * epoch) / T_pl if epoch < T_pl else lambda_cen


def round_start(feat, logits, labels):
    """Part A over the whole local set: (pseudo uint8 [N, C], f_k [2C, D] of epoch 0: label-wise mean features, every class,
    a zero count dividing by 1)"""
    C = labels.shape[1]
    pseudo = (torch.sigmoid(logits) > 0.5).to(torch.uint8)
    f_k = torch.zeros((2 * C, feat.shape[1]), dtype=feat.dtype)
    for c in range(C):
        for t in (0, 1):
            rows = labels[:, c] == t
            f_k[2 * c + t] = feat[rows].sum(0) / max(int(rows.sum()), 1)
    return pseudo, f_k


def server_centroids(f_G, f_locals):
    """Part C: w_i = cos(f_G, f_k_i) per row; f_G <- sum_i w_i f_k_i / sum_i w_i, a zero sum dividing by 1 (the weights may
    be negative)"""
    num = torch.zeros_like(f_G)
    den = torch.zeros(f_G.shape[0], dtype=f_G.dtype)
    for f in f_locals:
        w = cosine(f_G, f)
        num = num + w[:, None] * f
        den = den + w
    return num / torch.where(den == 0, torch.ones_like(den), den)[:, None]


def train_round(net, optimizer, batches, f_G, epoch, loss_w, active, a):
    """train_RoFL on a torch net returning (feature, logits).  batches: list of (x, y, item) of ONE pass in loader order, used
    for part A and for each of a.local_ep training passes; item: positions in the round's label table.  loss_w: the client's
    list, mutated like the reference's.  A batch with n_keep < 1 is skipped.
    -> (per-step losses, f_k, [pseudo table after each step], [margins() of each step])"""
    C = a.n_classes
    for c in range(C):
        if c not in active:
            loss_w[c] = 5.0
    net.eval()
    with torch.no_grad():
        outs = [net(x) for x, _, _ in batches]
    items = torch.cat([it for _, _, it in batches]).long()
    feat = torch.cat([o[0] for o in outs])
    pseudo0, f0 = round_start(feat, torch.cat([o[1] for o in outs]), torch.cat([y for _, y, _ in batches]))
    pseudo = torch.zeros((int(items.max()) + 1, C), dtype=torch.uint8)
    pseudo[items] = pseudo0
    f_k = f0 if epoch == 0 else f_G.clone().to(feat.dtype)
    net.train()
    w = torch.tensor(loss_w, dtype=feat.dtype)
    lam = lambda_cen_eff(a.lambda_cen, epoch, a.T_pl)
    losses, tables, margin = [], [], []
    for _ in range(a.local_ep):
        for x, y, it in batches:
            n = n_keep(a.forget_rate, x.shape[0])
            if n < 1:
                continue
            optimizer.zero_grad()
            f, z = net(x)
            margin.append(margins(z, f, y, n, w, f_k))
            r = head(z, f.detach(), y, it, n, w, lam, a.lambda_e, epoch < a.T_pl, f_k, pseudo)
            r["loss"].backward()
            optimizer.step()
            f_k, pseudo = r["f_k"], r["pseudo"]
            losses.append(float(r["loss"].detach()))
            tables.append(pseudo.clone())
    return losses, f_k, tables, margin
