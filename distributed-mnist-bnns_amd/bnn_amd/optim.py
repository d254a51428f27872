"""Latent-weight update.

The reference's protocol around ``torch.optim.Adam`` (mnist-dist2.py:91, :131-137)::

    for p in model.parameters():            # restore the latent weight
        if hasattr(p, 'org'): p.data.copy_(p.org)
    optimizer.step()
    for p in model.parameters():            # clamp it and keep it as the new latent
        if hasattr(p, 'org'): p.org.copy_(p.data.clamp_(-1, 1))

``org_protocol_step`` is that loop, for models running with ``org_protocol = True``.
``LatentAdam`` is the fused form for models whose Parameters hold the latent weights directly
(``org_protocol = False``): one libbnn kernel per tensor does Adam (torch's formula) and the clamp
of the parameters the reference clamps, with an optional gradient scale (1/world_size when the
gradient exchange summed instead of averaged).  For a binarized layer's weight the same kernel
also rewrites the next forward's packed ternary operands (bnn_adam_clamp_pack), replacing the
per-forward sign-pack of the weight.

With ``device_step`` (a ``functional.DeviceStep``) the step is graph-capturable: the bias
corrections come from a device table indexed by the device step counter (bit-identical to the
per-launch values), and the counter is advanced on the device after the last update.

``LatentSGD`` is the same fusion around ``torch.optim.SGD``, the optimizer of the reference's ConvNet
scripts (mnist.py, mnist-dist.py, mnist-mixed.py) and DDP demos (mnist-distributed-BNNS2.py): momentum,
dampening, weight decay and Nesterov as torch computes them, the clamp, and the re-pack of a binarized
layer's weight in one pass (bnn_sgd_clamp_pack).

``LatentBop`` is the binary optimizer of Helwegen et al. (NeurIPS 2019; larq's Bop) for the binarized weights
-- no latent weight, a moving average of the gradient, a flip where it exceeds a threshold against the
weight -- fused with the same re-pack (bnn_bop_pack), and ``LatentAdam`` for every other parameter.
"""
import os

import torch

from . import functional as BF

# Side streams for the binarized weights' Adam + pack launches (bnn_adam_clamp_pack): the k-th such
# launch of a step runs on stream k mod (1 + ADAM_STREAMS), 0 = the caller's, each forked from the
# caller's stream just before its launch and joined back after the last.  Every launch touches only
# its own tensors, so the results are bit-identical.  Measured, off by default (0 = one stream): at
# 2 the captured graphs' parallel branches made config 3's step 0.76-0.81 ms against 0.69 and the
# 192-wide net's 0.42 against 0.25; the wide step did not move (profiles/r06_af_adam_streams_ab.txt).
ADAM_STREAMS = int(os.environ.get("BNN_ADAM_STREAMS", "0"))


def org_protocol_step(model, optimizer):
    """mnist-dist2.py:131-137 verbatim in behaviour."""
    params = list(model.parameters())
    for p in params:
        if hasattr(p, "org"):
            p.data.copy_(p.org)
    optimizer.step()
    for p in params:
        if hasattr(p, "org"):
            p.org.copy_(p.data.clamp_(-1, 1))


class LatentAdam(torch.optim.Optimizer):
    """Adam (torch defaults) fused with clamp(-1, 1) for the parameters in ``clamp_params``."""

    SCHEDULE_STEPS = 1 << 20      # device-step table length (8 MiB per parameter group)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, clamp_params=(),
                 grad_scale=1.0, device_step=None):
        defaults = dict(lr=lr, betas=betas, eps=eps)
        super().__init__(params, defaults)
        self._clamp = {id(p) for p in clamp_params}
        self.grad_scale = grad_scale
        self.device_step = device_step
        self._sched = {}              # group index -> (device table, (lr, betas) it was built for)
        self._sides = {}              # device -> side streams (ADAM_STREAMS)

    def _side_streams(self, device):
        ss = self._sides.get(device)
        if ss is None:
            ss = [torch.cuda.Stream(device=device) for _ in range(ADAM_STREAMS)]
            self._sides[device] = ss
        return ss

    def _schedule(self, gi, group, step, device, build):
        """Device table for this group covering the device counter's steps: entry c holds the bias
        corrections of Adam step (step at table build) + c - (counter at build).  ``build``: make
        one if the cached table is missing or was built for another lr / betas; else None."""
        ds = self.device_step
        key = (group["lr"], tuple(group["betas"]))
        ent = self._sched.get(gi)
        if ent is None or ent[1] != key:
            if not build:
                return None
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("LatentAdam: build the device schedule (build_schedules) before capturing")
            first = step - ds.steps
            if first < 1:
                raise RuntimeError("LatentAdam: device step counter ahead of the optimizer's steps")
            tab = BF.adam_schedule(group["lr"], *group["betas"], first, ds.steps + self.SCHEDULE_STEPS, device)
            ent = (tab, key)
            self._sched[gi] = ent
        if ds.steps >= ent[0].shape[0]:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("LatentAdam: device-step schedule exhausted")
            return None             # eager: per-launch bias corrections
        return ent[0]

    def build_schedules(self):
        """(Re)build every group's device table for its current lr / betas, between steps -- before
        a HIP-graph capture (graph.GraphedStep calls it)."""
        ds = self.device_step
        if ds is None:
            return
        for gi, group in enumerate(self.param_groups):
            steps = {self.state[p]["step"] for p in group["params"] if self.state.get(p)}
            if not steps:
                continue
            if len(steps) != 1:
                raise RuntimeError("LatentAdam: device_step needs every parameter of a group stepped together")
            self._sched.pop(gi, None)
            self._schedule(gi, group, steps.pop() + 1, group["params"][0].device, build=True)

    def _own_update(self, p, group):
        """A subclass's own update of ``p`` (LatentBop); True: done, Adam skips it.  Such a parameter still
        keeps a ``"step"`` in its state, for the uniform-step logic above and build_schedules."""
        return False

    def schedule_limit(self):
        """Device counter value at which the first device table runs out (None: no table)."""
        lens = [ent[0].shape[0] for ent in self._sched.values()]
        return min(lens) if lens else None

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        ds = self.device_step
        capturing = ds is not None and torch.cuda.is_current_stream_capturing()
        npack = 0
        joined = {}                   # id(side stream) -> stream to join back into the caller's
        for gi, group in enumerate(self.param_groups):
            b1, b2 = group["betas"]
            sched = None
            small = []                # plain Adam + clamp tensors: one multi-tensor launch per 16
            live = [p for p in group["params"] if p.grad is not None]
            steps = {self.state[p]["step"] if self.state.get(p) else 0 for p in live}
            uniform = len(steps) == 1 and len(live) == len(group["params"])
            if ds is not None and live and not uniform and capturing:
                # one table per group is indexed by the shared device counter
                raise RuntimeError("LatentAdam: a captured device step needs every parameter of a group to "
                                   "get a gradient on every step")
            if ds is not None and live and uniform:
                # the table of this lr: built on the group's first step (or by build_schedules before
                # a capture); an eager step at another lr (the trainer's lr-quirk epochs) -- or an
                # eager step where some parameter got no gradient -- uses the per-launch bias
                # corrections (bit-identical) instead of a table
                sched = self._schedule(gi, group, steps.pop() + 1, live[0].device,
                                       build=gi not in self._sched)
                if sched is None and capturing:
                    raise RuntimeError("LatentAdam: no device schedule for this lr (build_schedules before capturing)")
            for p in live:
                if self._own_update(p, group):
                    continue
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["step"] += 1
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                args = (g, st["exp_avg"], st["exp_avg_sq"], st["step"], group["lr"], b1, b2, group["eps"],
                        self.grad_scale, id(p) in self._clamp)
                kw = dict(sched=sched, ctr=ds.ctr) if sched is not None else {}
                # a binarized layer's weight also gets its next-forward ternary operands rewritten in
                # the same pass (bnn_adam_clamp_pack); anything else: plain fused Adam + clamp
                side = None
                if ADAM_STREAMS > 0 and p.is_cuda and p.dim() == 2 and getattr(p, "_bnn_pack", None) is not None:
                    j = npack % (ADAM_STREAMS + 1)
                    npack += 1
                    if j > 0:
                        side = self._side_streams(p.device)[j - 1]
                if side is None:
                    done = BF.adam_clamp_pack_(p, *args, **kw)
                else:
                    main = torch.cuda.current_stream(p.device)
                    side.wait_stream(main)       # the gradient, the state and the counter are ready
                    with torch.cuda.stream(side):
                        done = BF.adam_clamp_pack_(p, *args, **kw)
                    if done:
                        joined[id(side)] = (side, main)
                        if g is not p.grad:
                            g.record_stream(side)
                if not done:
                    small.append((p, g, st["exp_avg"], st["exp_avg_sq"], st["step"], id(p) in self._clamp))
            if small:
                BF.adam_clamp_multi_(small, group["lr"], b1, b2, group["eps"], self.grad_scale,
                                     sched=sched, ctr=ds.ctr if sched is not None else None)
        for side, main in joined.values():
            main.wait_stream(side)
        if ds is not None:
            ds.advance()
        return loss


class LatentSGD(torch.optim.Optimizer):
    """``torch.optim.SGD`` (momentum, dampening, weight decay, Nesterov) fused with clamp(-1, 1) for the
    parameters in ``clamp_params``; bit-identical to torch's CPU fp32 step followed by ``clamp_``.

    State is torch's: ``momentum_buffer`` per parameter, allocated on the parameter's first step and
    absent when momentum is 0, so a ``torch.optim.SGD`` state_dict loads.  ``maximize`` is not built.

    With ``device_step`` the step advances the device counter after the last update (dropout and
    stochastic-binarization seeds move) and can be captured by ``graph.GraphedStep``: nothing in the
    update depends on the step count, so there is no device table.  A parameter's first step
    allocates its buffer and cannot be captured (GraphedStep's warm-up runs it eagerly).  lr and the
    other hyper-parameters are passed to the kernels by value: a captured step keeps the values of
    its capture, and a changed lr needs a recapture, as with LatentAdam.
    """

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False,
                 clamp_params=(), grad_scale=1.0, device_step=None):
        # torch.optim.SGD's own checks and messages
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                        nesterov=nesterov, maximize=False)
        super().__init__(params, defaults)
        self._clamp = {id(p) for p in clamp_params}
        self.grad_scale = grad_scale
        self.device_step = device_step

    @staticmethod
    def _refuse_maximize(groups):
        if any(g.get("maximize", False) for g in groups):
            raise ValueError("LatentSGD: maximize=True is not supported")

    def add_param_group(self, param_group):
        self._refuse_maximize([param_group])
        super().add_param_group(param_group)

    def load_state_dict(self, state_dict):
        self._refuse_maximize(state_dict["param_groups"])
        super().load_state_dict(state_dict)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        ds = self.device_step
        capturing = torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()
        self._refuse_maximize(self.param_groups)
        for group in self.param_groups:
            mu = group["momentum"]
            hyper = dict(momentum=mu, dampening=group["dampening"], weight_decay=group["weight_decay"],
                         nesterov=group["nesterov"], grad_scale=self.grad_scale)
            small = []                # plain SGD + clamp tensors: one multi-tensor launch per 16
            for p in group["params"]:
                if p.grad is None:
                    continue
                buf, first = None, False
                if mu != 0:
                    buf = (self.state.get(p) or {}).get("momentum_buffer")
                    if buf is None:
                        if capturing:
                            raise RuntimeError("LatentSGD: a captured step cannot be a parameter's first (it "
                                               "allocates the momentum buffer); run one eager step before capturing")
                        buf = torch.empty_like(p, memory_format=torch.contiguous_format)
                        self.state[p]["momentum_buffer"] = buf
                        first = True
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                clamp = id(p) in self._clamp
                # a binarized layer's weight also gets its next-forward ternary operands rewritten in the
                # same pass (bnn_sgd_clamp_pack); anything else: plain fused SGD + clamp
                if not BF.sgd_clamp_pack_(p, g, buf, group["lr"], first=first, clamp=clamp, **hyper):
                    small.append((p, g, buf, first, clamp))
            if small:
                BF.sgd_clamp_multi_(small, group["lr"], **hyper)
        if ds is not None:
            ds.advance()
        return loss


class LatentBop(LatentAdam):
    """Bop (Helwegen et al., "Latent Weights Do Not Exist: Rethinking Binarized Neural Network
    Optimization", NeurIPS 2019; larq's Bop) for the parameters in ``bop_params`` -- the binarized layers'
    weights, ``nets.binary_weights(model)`` -- and ``LatentAdam`` (lr, betas, eps, ``clamp_params``, the
    device-step table) through the same launches for every other parameter.

    A Bop weight is +-1, not a latent number: its state is ``bop_m``, the moving average of its gradient
    with rate ``gamma``, and it flips where that average exceeds ``threshold`` and has the weight's sign.
    The first step binarizes whatever the Parameter holds.  A 2-D weight with live packed operands gets
    them rewritten by the same pass (bnn_bop_pack); anything else -- the conv weights -- takes the flat
    pass (bnn_bop).  ``gamma`` and ``threshold`` are per param group and travel in the ``state_dict``; the
    defaults are larq's, starting points rather than values tuned for these nets.

    Every pass also counts the weights it flipped into the parameter's ``flips`` state, on the device;
    ``flip_counts`` reads them: the flip ratio flips / (numel * steps) is what gamma and threshold are
    tuned by.  Nothing in the Bop update depends on the step count, so a captured step replays it as it
    is; a parameter's first step allocates its state and cannot be captured.
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, gamma=1e-4, threshold=1e-8, bop_params=(),
                 clamp_params=(), grad_scale=1.0, device_step=None):
        super().__init__(params, lr=lr, betas=betas, eps=eps, clamp_params=clamp_params, grad_scale=grad_scale,
                         device_step=device_step)
        self._bop = {id(p) for p in bop_params}
        for group in self.param_groups:
            group.setdefault("gamma", gamma)
            group.setdefault("threshold", threshold)
            self._check_hyper(group)
        self.defaults.update(gamma=gamma, threshold=threshold)

    @staticmethod
    def _check_hyper(group):
        gamma, threshold = group["gamma"], group["threshold"]
        if not 0.0 < gamma <= 1.0:
            raise ValueError(f"Invalid gamma value: {gamma} (Bop's averaging rate lies in (0, 1])")
        if not threshold >= 0.0:
            raise ValueError(f"Invalid threshold value: {threshold} (Bop's flip threshold is not negative)")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)        # gamma / threshold: the defaults unless given
        if "gamma" in self.defaults:                # (the base constructor adds groups before they exist)
            self._check_hyper(self.param_groups[-1])

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            self._check_hyper(group)
        # torch casts every state tensor to the parameter's dtype; the counters are int64 and exact.  Saved
        # parameter ids are positions in the groups' order, as state_dict() numbers them.
        saved = state_dict["state"]
        ids = [i for g in state_dict["param_groups"] for i in g["params"]]
        ps = [p for g in self.param_groups for p in g["params"]]
        for i, p in zip(ids, ps):
            if i in saved and "flips" in saved[i]:
                self.state[p]["flips"] = saved[i]["flips"].to(device=p.device, dtype=torch.int64).clone()

    @torch.no_grad()
    def step(self, closure=None):
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            for group in self.param_groups:
                for p in group["params"]:
                    if id(p) in self._bop and p.grad is not None and "bop_m" not in self.state.get(p, {}):
                        raise RuntimeError("LatentBop: a captured step cannot be a parameter's first (it allocates "
                                           "the gradient average and the flip counter); run one eager step before "
                                           "capturing")
        return super().step(closure)

    def _own_update(self, p, group):
        if id(p) not in self._bop:
            return False
        st = self.state[p]
        if "bop_m" not in st:
            st["step"] = 0
            st["bop_m"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["flips"] = torch.zeros((1,), dtype=torch.int64, device=p.device)
            st["flips_since"] = 0           # the step count at the last flip_counts(reset=True)
        st["step"] += 1
        g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
        args = (g, st["bop_m"], group["gamma"], group["threshold"], self.grad_scale, st["flips"])
        if not BF.bop_pack_(p, *args):
            BF.bop_(p, *args)
        return True

    def flip_counts(self, reset=False):
        """{parameter: (flips, numel, steps)} of every Bop parameter that has stepped: the weights flipped
        over its ``steps`` steps since the last reset (flip ratio = flips / (numel * steps)).  One host read
        for all of them together."""
        items = [(p, self.state[p]) for group in self.param_groups for p in group["params"]
                 if "flips" in self.state.get(p, {})]
        if not items:
            return {}
        counts = torch.cat([st["flips"] for _, st in items]).tolist()
        out = {p: (int(c), p.numel(), st["step"] - st.get("flips_since", 0)) for (p, st), c in zip(items, counts)}
        if reset:
            for _, st in items:
                st["flips"].zero_()
                st["flips_since"] = st["step"]
        return out
