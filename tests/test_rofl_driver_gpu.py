"""The RoFL row (main.py:98-99, 167-168, 253-268; fedmlp_amd.driver_rofl, the driver's round loop with exp = "RoFL") end to end on
one GPU, in-process like tests/test_baseline_driver_gpu.py:
two rounds of eight clients.  After each round the global model is FedAvg of the clients' host state_dicts, and the f_G handed to
the next round's clients is fedavg.rofl_centroids of the previous f_G and the clients' returned centroids; the first f_G is the
CPU generator's draw for args.seed.  The multi-rank gather of the centroids needs more than one GPU and is not covered here."""
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_driver_rofl(monkeypatch):
    from fedmlp_amd import driver, driver_rofl, fedavg
    from fedmlp_amd.local_training import LocalUpdate
    trained, folds = [], []
    real_train, real_fold = LocalUpdate.train_RoFL, fedavg.rofl_centroids

    def spy_train(self, net, f_G, epoch):
        out = real_train(self, net, f_G, epoch)
        trained.append({"epoch": epoch, "client": self.client_id, "f_G": f_G.clone(), "f_k": out[2].clone(), "net": net,
                        "sd": {k: v.clone() for k, v in net.state_dict().items()}})
        return out

    def spy_fold(f_G, f_locals):
        out = real_fold(f_G, f_locals)
        # called behind the round's FedAvg: the engine holds the new global model
        folds.append({"f_G": f_G.clone(), "f_locals": [f.clone() for f in f_locals], "out": out.clone(),
                      "glob": {k: v.clone() for k, v in trained[-1]["net"].state_dict().items()}})
        return out
    monkeypatch.setattr(LocalUpdate, "train_RoFL", spy_train)
    monkeypatch.setattr(fedavg, "rofl_centroids", spy_fold)
    old = sys.argv
    sys.argv = ["driver_rofl", "--rounds_warmup", "2", "--n_local", "64", "--hw", "64", "--pretrained", "0"]
    try:
        log = driver_rofl.main()
    finally:
        sys.argv = old
    with pytest.raises(SystemExit):
        driver.args_parser(["--exp", "RoFL"])                   # the driver's own parser lists the reference's live rows only
    assert len(log) == 2 and all(np.isfinite(r["mean_loss"]) for r in log)
    assert len(trained) == 16 and len(folds) == 2
    assert [t["epoch"] for t in trained] == [0] * 8 + [1] * 8                  # the round number is train_RoFL's epoch
    f_G0 = torch.randn((16, 512), generator=torch.Generator().manual_seed(1037))
    for rnd in range(2):
        clients = trained[8 * rnd:8 * rnd + 8]
        fold = folds[rnd]
        f_in = f_G0 if rnd == 0 else folds[0]["out"]
        assert all(torch.equal(t["f_G"], f_in) for t in clients) and torch.equal(fold["f_G"], f_in)
        assert all(torch.equal(a, t["f_k"]) for a, t in zip(fold["f_locals"], clients))       # every client's, in client order
        assert torch.equal(fold["out"], real_fold(f_in, [t["f_k"] for t in clients]))
        assert bool(torch.isfinite(fold["out"]).all()) and not torch.equal(fold["out"], f_in)
        # FedAvg on the host copies (utils/FedAvg.py:7-14, equal shares): eight fp32 terms folded in another order than the
        # device's weighted accumulation -- 1e-5 relative, and 1e-7 where the terms cancel
        want = fedavg.FedAvg([t["sd"] for t in clients], [64] * 8)
        for k, v in want.items():
            g = fold["glob"][k]
            if "num_batches" in k:
                assert int(g) == int(v), k
            else:
                np.testing.assert_allclose(g.numpy(), v.numpy(), rtol=1e-5, atol=1e-7, err_msg=k)
    assert not torch.equal(trained[0]["f_k"], trained[1]["f_k"])
