"""globaltest / classtest / valloss drop-ins (reference: utils/evaluations.py:15-133, utils/valloss_cal.py,
utils/multilabel_metrixs.py).

The eval-mode forward over the test set runs on the HIP engine (batches of 4*batch_size like
:18); the metrics are small host-side numpy restatements: per-class average precision and ROC
AUC follow scikit-learn's definitions (the reference calls average_precision_score / roc_curve
+ auc, :41-49, :60-66), BACC / R / P / F1 / Hamming follow utils/multilabel_metrixs.py.  With device_metrics=True the
sigmoids stay on the device and the same numbers come from the engine's fm_eval_metrics kernels (csrc/metrics.hip).
"""
import numpy as np
import torch


def average_precision(y_true, score):
    """sklearn.metrics.average_precision_score for one binary column:
    AP = sum_n (R_n - R_{n-1}) P_n over the distinct score thresholds, descending."""
    y_true = np.asarray(y_true, dtype=np.float64)
    score = np.asarray(score, dtype=np.float64)
    order = np.argsort(-score, kind="mergesort")
    y, s = y_true[order], score[order]
    distinct = np.where(np.diff(s))[0]
    idx = np.r_[distinct, y.size - 1]
    tps = np.cumsum(y)[idx]
    fps = 1 + idx - tps
    precision = tps / (tps + fps)
    recall = tps / tps[-1] if tps[-1] > 0 else np.full_like(tps, np.nan)
    return float(np.sum(np.diff(np.r_[0.0, recall]) * precision))


def roc_auc(y_true, score):
    """auc(roc_curve(y, score)) -- trapezoid under the ROC of the distinct thresholds."""
    y_true = np.asarray(y_true, dtype=np.float64)
    score = np.asarray(score, dtype=np.float64)
    order = np.argsort(-score, kind="mergesort")
    y, s = y_true[order], score[order]
    idx = np.r_[np.where(np.diff(s))[0], y.size - 1]
    tps = np.r_[0.0, np.cumsum(y)[idx]]
    fps = np.r_[0.0, (1 + idx) - np.cumsum(y)[idx]]
    tpr, fpr = tps / tps[-1], fps / fps[-1]
    return float((np.trapezoid if hasattr(np, "trapezoid") else np.trapz)(tpr, fpr))


def count_metrics(tp, npos, npred, tn, n):
    """BACC, R, F1, P, hamming_loss (utils/multilabel_metrixs.py, all classes) from the four per-class count vectors
    tp = #(y & pred), npos = #y, npred = #pred, tn = #(~y & ~pred) over n samples: the one expression the host and the
    device path share."""
    tp, npos, npred, tn = (np.asarray(v).astype(np.float64) for v in (tp, npos, npred, tn))
    C = tp.shape[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        recall1 = tp / npos
        recall0 = tn / (n - npos)
        R = float(np.sum(recall1) / C)
        bacc = float(np.sum((recall0 + recall1) / 2) / C)
        F1 = float(np.sum(2 * tp / (npos + npred)) / C)
        # Precision skips classes without predictions but still divides by C (multilabel_metrixs.py:57-64)
        P = float(np.sum(np.where(npred > 0, tp / np.where(npred > 0, npred, 1), 0.0)) / C)
    # a sample differs from its prediction in n - tp - tn places: fn + fp = (npos - tp) + (npred - tp) = n - tn - tp
    hamming = float((npos + npred - 2 * tp).sum() / (n * C))
    return {"BACC": bacc, "R": R, "F1": F1, "P": P, "hamming_loss": hamming}


def multilabel_metrics(all_labels, all_probs, threshold=0.5):
    """mAP, BACC, R, F1, auc, P, hamming_loss exactly as globaltest assembles them."""
    y = np.asarray(all_labels)
    p = np.asarray(all_probs)
    pred = p > threshold
    C = y.shape[1]
    aps = [average_precision(y[:, c], p[:, c]) for c in range(C)]
    yt = y.astype(bool)
    m = count_metrics(np.logical_and(yt, pred).sum(0), yt.sum(0), pred.sum(0), (~np.logical_or(yt, pred)).sum(0), y.shape[0])
    auroc = float(np.mean([roc_auc(y[:, c], p[:, c]) for c in range(C)]))
    return {"mAP": torch.tensor(aps).mean(), "BACC": m["BACC"], "R": m["R"], "F1": m["F1"], "auc": auroc, "P": m["P"],
            "hamming_loss": m["hamming_loss"]}


def multilabel_metrics_device(engine, labels_dev, probs_dev, threshold=0.5):
    """multilabel_metrics with the ranking and the counts on the device (fm_eval_metrics): the same dict.  ONE device-to-host
    read, of 6 C 8-byte values (AP, AUC as fp64 and the four int64 counts per class)."""
    ap, auc, counts = engine.eval_metrics(probs_dev, labels_dev, threshold)
    C = int(ap.shape[0])
    # one buffer, one copy: the fp64 values travel as their bit patterns
    host = torch.cat([ap.view(torch.int64), auc.view(torch.int64), counts.reshape(-1)]).cpu().numpy()
    aps, aucs = host[:C].view(np.float64), host[C:2 * C].view(np.float64)
    cnt = host[2 * C:].reshape(C, 4)
    m = count_metrics(cnt[:, 0], cnt[:, 1], cnt[:, 2], cnt[:, 3], int(probs_dev.shape[0]))
    return {"mAP": torch.tensor(aps.tolist()).mean(), "BACC": m["BACC"], "R": m["R"], "F1": m["F1"],
            "auc": float(np.mean(aucs)), "P": m["P"], "hamming_loss": m["hamming_loss"]}


def class_metrics(labels, preds, classid):
    """BACC, R, F1, P of ONE class: the `classid` branches of utils/multilabel_metrixs.py:21-71.  No zero guards: a class
    without positives, negatives or predictions gives the NaN / inf the reference's divisions give."""
    y = np.asarray(labels)[:, classid].astype(bool)
    p = np.asarray(preds)[:, classid].astype(bool)
    return class_count_metrics(np.logical_and(y, p).sum(), y.sum(), p.sum(), (~np.logical_or(y, p)).sum(), y.size)


def class_count_metrics(tp, npos, npred, tn, n):
    """class_metrics from the class's four counts (what the device path reads back)"""
    tp, npos, npred, tn = (np.float64(v) for v in (tp, npos, npred, tn))
    with np.errstate(invalid="ignore", divide="ignore"):
        recall1 = tp / npos
        recall0 = tn / (np.float64(n) - npos)
        return {"BACC": float((recall0 + recall1) / 2), "R": float(recall1), "F1": float((2 * tp) / (npos + npred)),
                "P": float(tp / npred)}


def _hw(ds):
    s = ds[0]["image"]
    return int(s.shape[-2]), int(s.shape[-1])


def _batch_images(net, test_dataset, views, idx, bs):
    """the eval batch of the consecutive rows `idx` (at most bs of them) on the device"""
    if hasattr(test_dataset, "device_batch"):
        return test_dataset.device_batch(net.bind(*_hw(test_dataset), bs), "image", idx)
    if views is not None and "image" in views:
        return views["image"][idx[0]:idx[0] + len(idx)]
    return torch.stack([torch.as_tensor(test_dataset[j]["image"], dtype=torch.float32) for j in idx])


def _host_probs(net, test_dataset, args):
    """sigmoid(logits) of the whole test set as a host fp32 [N, C] array (batches of 4 * batch_size, one read per batch)"""
    net.eval()
    n = len(test_dataset)
    bs = args.batch_size * 4
    from .launch import default_device
    views = test_dataset.device_views(default_device()) if hasattr(test_dataset, "device_views") else None
    probs = []
    for i in range(0, n, bs):
        idx = list(range(i, min(n, i + bs)))
        _, logits = net(_batch_images(net, test_dataset, views, idx, bs))
        z = logits.cpu().numpy().astype(np.float32)
        probs.append((1.0 / (1.0 + np.exp(-z.astype(np.float32)))).astype(np.float32))
    all_probs = np.concatenate(probs, 0)
    assert all_probs.shape == (n, args.n_classes)
    return all_probs


def sharded_probs(forward, n, C, rank, world, bs, device):
    """sigmoid(logits) of n rows as a device fp32 [n, C] tensor, the forward dealt over the ranks: rank r forwards the fixed
    blocks b of bs consecutive rows with b % world == r (`forward(rows)` returns their logits) and writes their sigmoids into
    a zero tensor; ONE sum all-reduce (torch.distributed, if initialised) completes it on every rank.  Every row is written
    by one rank and adding zeros is exact: bit-identical to the one-rank result.  Nothing here synchronises with the host."""
    probs = torch.zeros((n, C), device=device, dtype=torch.float32)
    for b, i in enumerate(range(0, n, bs)):
        if b % world != rank:
            continue
        rows = list(range(i, min(n, i + bs)))
        torch.sigmoid(forward(rows).detach().float(), out=probs[i:i + len(rows)])
    if world > 1:
        import torch.distributed as dist
        assert dist.is_available() and dist.is_initialized() and dist.get_world_size() == world
        dist.all_reduce(probs)
    return probs


def _rank_world():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def _device_probs(net, test_dataset, args):
    """(probs [N, C], targets [N, C]) on the engine's device: the rank-sharded eval forward, no host read"""
    net.eval()
    n = len(test_dataset)
    bs = args.batch_size * 4
    from .launch import default_device
    dev = default_device()
    views = test_dataset.device_views(dev) if hasattr(test_dataset, "device_views") else None
    rank, world = _rank_world()
    probs = sharded_probs(lambda rows: net(_batch_images(net, test_dataset, views, rows, bs))[1], n, args.n_classes, rank,
                          world, bs, dev)
    targets = torch.as_tensor(np.ascontiguousarray(np.array(test_dataset.targets), dtype=np.float32)).to(probs.device)
    return probs, targets


def _engine_of(net, test_dataset, args):
    """the engine the eval forward of `net` runs on (a rank whose shard is empty has not called it yet)"""
    eng = getattr(net, "_engine", None)
    if eng is None or not eng.h:
        eng = net.bind(*_hw(test_dataset), max(net.default_max_images, args.batch_size * 4))
    return eng


def globaltest(net, test_dataset, args, device_metrics=False):
    """utils/evaluations.py:15-73 with the forward on the HIP engine.  device_metrics=True: the sigmoids stay in a device
    [N, C] tensor (no read inside the loop; the forward is dealt over the ranks of an initialised torch.distributed group)
    and the metrics come from fm_eval_metrics with one small read at the end."""
    if device_metrics:
        probs, targets = _device_probs(net, test_dataset, args)
        return multilabel_metrics_device(_engine_of(net, test_dataset, args), targets, probs)
    return multilabel_metrics(np.array(test_dataset.targets), _host_probs(net, test_dataset, args))


def classtest(net, test_dataset, args, classid, device_metrics=False):
    """utils/evaluations.py:89-133: BACC, R, F1, P of class `classid` at the 0.5 threshold.  device_metrics=True: the counts
    come from fm_eval_metrics (no ranking pass)."""
    if device_metrics:
        probs, targets = _device_probs(net, test_dataset, args)
        _, _, counts = _engine_of(net, test_dataset, args).eval_metrics(probs, targets, 0.5, ap=False, auc=False)
        tp, npos, npred, tn = (int(v) for v in counts[classid].cpu().numpy())
        return class_count_metrics(tp, npos, npred, tn, len(test_dataset))
    return class_metrics(np.array(test_dataset.targets), _host_probs(net, test_dataset, args) > 0.5, classid)


def valloss_from_logits(logits, targets, order, bs):
    """The arithmetic of utils/valloss_cal.py:30-41 on the logits of the first n = len(order) samples: batches of bs in
    `order`, each BCEWithLogitsLoss(pos_weight = n / class_sum) with mean reduction, the mean of the batch means."""
    n = len(order)
    targets = torch.as_tensor(targets, dtype=torch.float32, device=logits.device)[:n]
    class_sum = np.zeros(targets.shape[1])
    for row in targets.cpu().numpy():                    # get_num_of_each_class: a float64 running sum, row by row
        class_sum += row
    loss_w = [n / i for i in class_sum.tolist()]         # a class without a positive raises, as in the reference
    crit = torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor(loss_w).to(logits.device))
    order = torch.as_tensor(order, dtype=torch.int64, device=logits.device)
    batch_loss = [crit(logits[order[i:i + bs]], targets[order[i:i + bs]]).item() for i in range(0, n, bs)]
    return np.array(batch_loss).mean()


def valloss(net, test_dataset, args):
    """utils/valloss_cal.py:15-43: the weighted BCE of the first int(0.1 N) test samples, drawn in SubsetRandomSampler's
    order (one torch.randperm(n) from the global generator), with the forward on the HIP engine."""
    net.eval()
    n = int(len(test_dataset) * 0.1)
    bs = args.batch_size * 4
    order = torch.randperm(n).tolist()
    from .launch import default_device
    views = test_dataset.device_views(default_device()) if hasattr(test_dataset, "device_views") else None
    logits = None
    for i in range(0, n, bs):
        idx = list(range(i, min(n, i + bs)))
        _, z = net(_batch_images(net, test_dataset, views, idx, bs))
        if logits is None:
            logits = torch.empty((n, z.shape[1]), device=z.device, dtype=torch.float32)
        logits[i:i + len(idx)] = z.detach()
    return valloss_from_logits(logits, np.array(test_dataset.targets)[:n], order, bs)
