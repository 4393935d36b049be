"""torch.optim.Adam for a HipNet / ResidentNet (utils/local_training.py builds a fresh torch.optim.Adam every round).

The weights, the Adam moments and the step count live in the HIP engine the net is bound to, and the gradients are the
engine's accumulator that loss.backward() through a train-mode ``net(x)`` fills (model.HipNet).  So the optimizer takes
the net, not ``net.parameters()``:

    opt = Adam(net, lr=args.base_lr, betas=(0.9, 0.999), weight_decay=5e-4)
    net.train(); feat, logits = net(x); loss = head(feat, logits)
    opt.zero_grad(); loss.backward(); opt.step()

Arithmetic: torch.optim.Adam's single-tensor update with coupled L2 weight decay (fm_adam_step).
"""


class Adam:
    def __init__(self, net, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        if lr < 0.0 or eps < 0.0 or weight_decay < 0.0 or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Adam: invalid hyper-parameters lr={lr} betas={betas} eps={eps} weight_decay={weight_decay}")
        self.net = net
        self.defaults = {"lr": lr, "betas": tuple(betas), "eps": eps, "weight_decay": weight_decay}
        # read on every step, so a caller may change lr between steps (param_groups[0]["lr"] = ...)
        self.param_groups = [dict(self.defaults)]
        # a fresh torch.optim.Adam: zero moments and step count.  The moments belong to the engine; a net that is not bound
        # yet gets them reset at its first step
        self._engine = None
        eng = net._bound_engine()
        if eng is not None:
            self._reset(eng)

    def _reset(self, eng):
        g = self.param_groups[0]
        eng.adam_reset(g["lr"], g["betas"], g["eps"], g["weight_decay"])
        self._engine = eng

    def zero_grad(self, set_to_none=True):
        self.net.zero_grad()

    def step(self):
        eng = self.net._bound_engine()
        if eng is None:
            raise RuntimeError("Adam.step: the engine does not hold this optimizer's net (another net was bound to it since "
                               "the backward, or the net never ran); the Adam moments belong to the engine")
        if self._engine is not eng:
            self._reset(eng)
        if getattr(eng, "_grad_owner", None) is not self.net:
            return                      # no gradients: torch.optim.Adam skips parameters whose .grad is None
        g = self.param_groups[0]
        eng.adam_step(g["lr"], g["betas"], g["eps"], g["weight_decay"])
        self.net.mark_trained()
