"""Optimizer side of the hot path: timm's decay / no-decay parameter grouping (timm 0.4.12
optim_factory.add_weight_decay, call site main_pretrain.py:253) and AdamW(betas=(0.9, 0.95)) (:254) as ONE fused
HIP launch over the parameter arena (ecamp_adamw_grouped), which also refreshes the bf16 shadow weights."""
import collections
import math
import os

import torch

from . import hip_ops as ops
from .streams import held

# How many (micro-)steps the host may queue ahead of the GPU.  The host queues a step in ~15 ms, the GPU runs it in ~36: unbounded, the
# host's lead grows by 20 ms per step, and every tensor a side stream reads (record_stream: the weight-gradient stream's x and dy, i.e.
# most saved activations, ~10 GB per step) is only returned to the caching allocator when the GPU gets there -- round 6's bench record
# showed 250-570 hipMalloc calls and 27-60 GB of reserve growth inside 20 timed steps, and steps of 2x the median when such a burst met
# a small lead (BENCH_r05's 40.7 ms mean).  Two steps in flight keep the GPU fed through a host hiccup of ~70 ms and reach their steady state within a 5-step warm-up
# (three: +35 ms of slack, but the lead is still growing when the driver's timed region starts).  0 = unbounded (the old behaviour).
MAX_STEPS_IN_FLIGHT = int(os.environ.get("ECAMP_MAX_STEPS_IN_FLIGHT", "2"))
# ... and fewer than that (never fewer than one) while the tensors held for the side streams (streams.Held: ~21 GB per step at B = 256) pass this
MAX_HELD_BYTES = int(float(os.environ.get("ECAMP_MAX_HELD_GB", "96")) * 2 ** 30)


def add_weight_decay(model, weight_decay=1e-5, skip_list=()):
    """1-D tensors and names ending in '.bias' get no decay; everything else (incl. the 3-D cls/mask tokens and the
    embedding tables) is decayed.  Returns [no_decay group, decay group] like timm."""
    decay, no_decay = [], []
    for name, param in model.named_parameters():
        if not param.requires_grad:
            continue
        if len(param.shape) == 1 or name.endswith(".bias") or name in skip_list:
            no_decay.append(param)
        else:
            decay.append(param)
    return [{"params": no_decay, "weight_decay": 0.0}, {"params": decay, "weight_decay": weight_decay}]


class _FlatOptimizer(torch.optim.Optimizer):
    """What the two fused optimizers share: at most 8 groups over ONE parameter arena (and, where `_TAIL_OK`, one arena.FlatTail), bound
    on first use with a block table per space (arena.FlatSpace.block_table); pacing; `zero_grad` / `flush_grads`; and the checkpoint
    packing of torch.optim, driven by three hooks: `_state_head`, `_state_views`, `_accept_state`."""
    _TAIL_OK = False

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        if len(self.param_groups) > 8:
            raise ValueError("%s supports at most 8 param groups" % type(self).__name__)
        self._arena = self._tail = None
        self._inflight = collections.deque()

    def pace(self):
        """Called where a (micro-)step ends: records an event on the compute stream and blocks the host until the step
        MAX_STEPS_IN_FLIGHT back has finished on the GPU (see MAX_STEPS_IN_FLIGHT).  No device-wide synchronisation."""
        if not torch.cuda.is_available():
            return
        held.seal()   # tensors the second streams read during this step: held until the GPU is past here (streams.Held)
        if MAX_STEPS_IN_FLIGHT <= 0:
            return
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        self._inflight.append(ev)
        while len(self._inflight) > MAX_STEPS_IN_FLIGHT or (len(self._inflight) > 1 and held.bytes > MAX_HELD_BYTES):
            self._inflight.popleft().synchronize()
            held.reap()
        held.reap()   # the step that wait was for is complete: its held tensors go back to the allocator now

    @property
    def arena(self):
        """The parameter arena this optimizer updates (bound on first use); `arena.reducer` is the data-parallel reducer, if any."""
        return self._bind()

    def _bind(self):
        if self._arena is not None:
            return self._arena
        who = type(self).__name__
        arena = tail = None
        for g in self.param_groups:
            for p in g["params"]:
                a, t = getattr(p, "_ecamp_arena", None), getattr(p, "_ecamp_tail", None) if self._TAIL_OK else None
                if a is None and t is None:
                    raise RuntimeError(who + ": parameter is not in an ecamp_amd arena -- call model.prepare() (or run one forward) after "
                                       "model.to('cuda') and before the first optimizer.step()")
                if a is not None:
                    arena = arena or a
                    if a is not arena:
                        raise RuntimeError(who + ": parameters from different arenas")
                else:
                    tail = tail or t
                    if t is not tail:
                        raise RuntimeError(who + ": parameters from different arenas (two tail buffers)")
        self._bound(arena, tail)
        self._table = arena.block_table(self.param_groups).to(arena.device)
        self._tail_table = tail.block_table(self.param_groups).to(tail.device) if tail is not None else None
        self._arena, self._tail = arena, tail
        return arena

    def zero_grad(self, set_to_none=False):
        """p.grad stay views of the gradient arena / the tail buffer (set_to_none would detach them).  After the first step this is LAZY for
        weight matrices: biases / LayerNorm / embedding gradients are zeroed now, a weight matrix keeps its old values until the next
        backward pass OVERWRITES it (its first weight-gradient GEMM runs with beta = 0), or until `flush_grads()` / `step()` find
        it untouched and zero it.  Read p.grad after backward, not between zero_grad() and backward.  ECAMP_LAZY_ZERO_GRAD=0 restores
        the plain memset."""
        self._bind().zero_grad()
        if self._tail is not None:
            self._tail.zero_grad()

    def flush_grads(self):
        """Make every p.grad consistent (zero the weight gradients no GEMM has written since zero_grad())."""
        self._bind().flush_fresh()

    # -- checkpoint format compatible with torch.optim (misc.py:295-338) ----------------------------------------
    def state_dict(self):
        self._bind()
        head = self._state_head()
        state, packed_groups, idx = {}, [], 0
        for g in self.param_groups:
            ids = []
            for p in g["params"]:
                if head is not None and not getattr(p, "_ecamp_unused", False):
                    state[idx] = {**{k: v.clone() for k, v in head.items()}, **{k: v.clone() for k, v in self._state_views(p).items()}}
                ids.append(idx)
                idx += 1
            packed_groups.append({**{k: v for k, v in g.items() if k != "params"}, "params": ids})
        return {"state": state, "param_groups": packed_groups}

    def load_state_dict(self, sd):
        self._bind()
        idx = 0
        for g, sg in zip(self.param_groups, sd["param_groups"]):
            for k, v in sg.items():
                if k != "params":
                    g[k] = v
            for p in g["params"]:
                st = sd["state"].get(idx, sd["state"].get(str(idx)))
                if st is not None and self._accept_state(st):
                    for k, v in self._state_views(p).items():
                        v.copy_(st[k])
                idx += 1


class FusedAdamW(_FlatOptimizer):
    """torch.optim.AdamW semantics (decoupled decay, bias correction, eps outside the sqrt) on the flat arenas.
    `param_groups` behave as usual (lr schedulers write `group['lr']`); parameters whose gradient never arrives in
    the reference (`_ecamp_unused`, the BERT pooler) are skipped entirely, exactly as torch skips `grad is None`."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        b = {tuple(g["betas"]) for g in self.param_groups}
        e = {g["eps"] for g in self.param_groups}
        if len(b) != 1 or len(e) != 1:
            raise ValueError("all groups must share betas and eps")
        self._step = 0
        self._step_dev = None       # f32[1] on the device: the count of steps actually taken when a loss scaler decides skips there (`ctl`)
        self.grad_scale = 1.0
        self.bucketwise_steps = 0   # optimizer steps that ran bucket by bucket behind the gradient all-reduces

    def _bound(self, arena, tail):
        self._m = ops.zeros((arena.total,), arena.device)
        self._v = ops.zeros((arena.total,), arena.device)

    @property
    def steps_taken(self):
        """Optimizer steps applied so far (a step skipped by the dynamic loss scaler does not count; reading it waits for the device)."""
        if self._step_dev is not None:
            self._step = int(self._step_dev.item())
        return self._step

    def step_counter(self):
        """The device-side step count (created from the host's on first use): ecamp_loss_scale_update advances it only on clean steps."""
        if self._step_dev is None:
            self._step_dev = torch.full((1,), float(self._step), device=self._bind().device, dtype=torch.float32)
        return self._step_dev

    def _launch(self, A, lo, hi, grad_sumsq, ctl=None):
        g0 = self.param_groups[0]
        ops.adamw_grouped(A.flat_p[lo:hi], A.flat_g[lo:hi], self._m[lo:hi], self._v[lo:hi], A.flat_p16[lo:hi] if A.flat_p16 is not None else None,
                          self._table[lo // 64:hi // 64], [g["lr"] for g in self.param_groups], [g["weight_decay"] for g in self.param_groups],
                          g0["betas"][0], g0["betas"][1], g0["eps"], max(self._step, 1), self.grad_scale, grad_sumsq, ctl)

    @torch.no_grad()
    def step(self, closure=None, grad_sumsq=None, ctl=None):
        """`ctl` (device f32[4], hip_ops.loss_scale_update): the gradient scale, the bias corrections and whether this step happens at all
        are read on the device; the step count then lives in `step_counter()`."""
        loss = closure() if closure is not None else None
        A = self._bind()
        events = None
        if A.reducer is not None:
            A.reducer.assert_reduced()   # loud failure instead of a silent step on un-reduced gradients
            events = A.reducer.take_bucket_events()
        if ctl is None:
            if self._step_dev is not None:      # back from device-decided steps to host-counted ones
                self._step, self._step_dev = self.steps_taken, None
            self._step += 1
        if events and not A._fresh:
            # data parallel, lazy join (GradReducer.lazy): one slice of the fused kernel per gradient bucket, each behind its own
            # all-reduce, in the order the collectives were issued -- the update of the early buckets runs while the last ones
            # are still on the links
            cur = torch.cuda.current_stream()
            for lo, hi, ev in events:
                cur.wait_event(ev)
                self._launch(A, lo, hi, grad_sumsq, ctl)
            self.bucketwise_steps += 1
        else:
            for _, _, ev in events or ():    # (a module did not run this window: zero its weights only behind every collective)
                torch.cuda.current_stream().wait_event(ev)
            A.flush_fresh()
            self._launch(A, 0, A.total, grad_sumsq, ctl)
        A.version += 1   # the bf16 shadows changed: the fp8-forward mode re-quantises its weight copies on next use
        self.pace()
        return loss

    def covers(self, parameters):
        """True when the tensors of `parameters` that carry a gradient are exactly the ones this optimizer updates: then
        `step_with_grad_norm()` equals the reference's get_grad_norm_(parameters) followed by step()."""
        own = {id(p) for g in self.param_groups for p in g["params"] if p.grad is not None}
        given = {id(p) for p in parameters if p.grad is not None}
        return len(own) > 0 and given == own

    @torch.no_grad()
    def step_with_grad_norm(self):
        """One pass over the gradient arena: the update AND sum(g^2) of what it consumed (util/misc.py:280-292 computes the norm in
        a separate pass over 733 MB just before the step).  -> 0-d tensor, the global L2 gradient norm before the update."""
        A = self._bind()
        s = ops.zeros((1,), A.device)
        self.step(grad_sumsq=s)
        return s.sqrt().reshape(())

    def _state_head(self):
        """The leading entries of every parameter's state, None before the first step."""
        self._step = self.steps_taken
        return {"step": torch.tensor(float(self._step))} if self._step > 0 else None

    def _state_views(self, p):
        o, n = self._arena.span(p)
        return {"exp_avg": self._m[o:o + n].view(p.shape), "exp_avg_sq": self._v[o:o + n].view(p.shape)}

    def _accept_state(self, st):
        self._step, self._step_dev = int(float(st["step"])), None
        return True


class FusedSGD(_FlatOptimizer):
    """torch.optim.SGD(momentum, dampening 0, no Nesterov, weight decay added to the gradient) behind
    torch.nn.utils.clip_grad_norm_(max_grad_norm) -- train.py:377-384,458 of the reference's Fine-tuning/Classification -- as fused HIP
    launches over the parameter arena: `ecamp_sumsq_grouped` leaves one partial sum of squares per workgroup, `ecamp_sgd_grouped` adds them
    in every workgroup, forms the clip coefficient and updates parameters, momentum and the 16-bit shadows.  Parameters outside the arena
    must sit in ONE arena.FlatTail (ECAMPClassifier's fc_norm and head): a second pair of launches updates them with the same partials,
    hence the same norm and coefficient.  Nothing is read back: `last_norm` is the global gradient norm as a device scalar.
    max_grad_norm <= 0: no clipping."""
    _TAIL_OK = True

    def __init__(self, params, lr=1e-3, momentum=0.9, weight_decay=0.0, max_grad_norm=0.0):
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=False))
        if len({g["momentum"] for g in self.param_groups}) != 1:
            raise ValueError("all groups must share momentum")
        if any(g.get("dampening", 0) != 0 or g.get("nesterov", False) for g in self.param_groups):
            raise ValueError("FusedSGD implements dampening 0 without Nesterov momentum only")
        self.max_grad_norm = float(max_grad_norm)
        self.grad_scale = 1.0
        self.last_norm = None       # f32[1] on the device after a step: the global norm of the (un-scaled) gradients before clipping
        self._steps = 0

    def _bound(self, arena, tail):
        if arena is None:
            raise RuntimeError("FusedSGD: no parameter of a model's arena among the groups (the tail buffer alone is not supported)")
        if arena.reducer is not None:
            raise RuntimeError("FusedSGD: data-parallel fine-tuning is not implemented")
        self._buf = ops.zeros((arena.total,), arena.device)
        self._slots = (ops.sumsq_grouped_slots(arena.total), ops.sumsq_grouped_slots(tail.total) if tail is not None else 0)
        self._partials = ops.zeros((sum(self._slots),), arena.device)
        self.last_norm = ops.zeros((1,), arena.device)

    @torch.no_grad()
    def step(self, closure=None, ctl=None):
        """`ctl` (device f32[4], hip_ops.loss_scale_update): the gradient scale and whether this step happens at all are read on the device."""
        loss = closure() if closure is not None else None
        self._step(ctl, None)
        return loss

    @torch.no_grad()
    def step_scaled(self, scaler):
        """The step under an `SGDLossScaler` whose scale multiplied the loss: between the sums of squares and the updates ONE
        `ecamp_sgd_scale_update` launch decides from the partials whether the scaled gradients overflowed, writes the `ctl` both updates
        read (1 / scale; a skip leaves parameters, momentum, shadows and the tail alone), `last_norm` (the norm of the un-scaled
        gradients; inf / nan on a skipped step) and the scaler's next state.  Nothing is read back, and the step count advances whether or
        not the device skipped -- as the reference's scheduler and global_step do around apex (train.py:462-465)."""
        self._step(None, scaler)

    def _step(self, ctl, scaler):
        A, T = self._bind(), self._tail
        A.flush_fresh()
        lrs = [g["lr"] for g in self.param_groups]
        wds = [g["weight_decay"] for g in self.param_groups]
        mom = self.param_groups[0]["momentum"]
        n0, n1 = self._slots
        ops.sumsq_grouped(A.flat_g, self._table, self._partials)
        if T is not None:
            ops.sumsq_grouped(T.flat_g, self._tail_table, self._partials[n0:])
        norm_out = self.last_norm
        if scaler is not None:   # (a skipped sgd_grouped writes no norm: the scaler's launch does, with the same bits on a clean step)
            ctl, norm_out = scaler.update(self._partials, n0 + n1, self.last_norm), None
        ops.sgd_grouped(A.flat_p, A.flat_g, self._buf, A.flat_p16, self._table, lrs, wds, mom, self.max_grad_norm, self._partials, n0 + n1,
                        self.grad_scale, ctl, norm_out)
        if T is not None:
            ops.sgd_grouped(T.flat_p, T.flat_g, T.flat_buf, None, self._tail_table, lrs, wds, mom, self.max_grad_norm, self._partials, n0 + n1,
                            self.grad_scale, ctl, None)
        self._steps += 1
        A.version += 1   # the 16-bit shadows changed
        self.pace()

    def _state_head(self):
        return {} if self._steps > 0 else None

    def _state_views(self, p):
        space, buf = (self._arena, self._buf) if id(p) in self._arena.index else (self._tail, self._tail.flat_buf)
        o, n = space.span(p)
        return {"momentum_buffer": buf[o:o + n].view(p.shape)}

    def _accept_state(self, st):
        if st.get("momentum_buffer") is None:   # (torch.optim.SGD keeps None until its first step)
            return False
        self._steps = max(self._steps, 1)
        return True


class SGDLossScaler:
    """apex's dynamic loss scaling (LossScaler.update_scale under `amp.initialize(opt_level="O2")`, the reference's `--fp16` recipe:
    Fine-tuning/Classification/train.py:398 starts it at 2^20) for `FusedSGD.step_scaled`, with the decision on the device:

        scaler.scale_loss(loss).backward();  optimizer.step_scaled(scaler)

    state = {scale, clean steps since the last change, steps skipped in total, steps skipped in a row}.  A step whose scaled gradients
    are not finite is skipped and the scale multiplied by `backoff`; after `window` clean steps in a row the scale grows by `growth`, up to
    `max_scale`.  `window=0` is a static scale (it never moves; a non-finite step is still skipped, where apex's static mode would step
    into the NaNs).  The state moves to the device on first use (ecamp_sgd_scale_update keeps it there) and no step reads it back:
    `scale`, `skipped_steps`, `skipped_in_a_row`, `clean_steps` and `last_found_inf` wait for the device only when asked.  `host_update`
    is the same rule on the host, for a state that has not moved to the device."""

    def __init__(self, init_scale=2.0 ** 20, growth=2.0, backoff=0.5, window=2000, max_scale=2.0 ** 24):
        if not init_scale > 0 or not growth >= 1 or not 0 < backoff <= 1 or int(window) != window or window < 0 or not max_scale > 0:
            raise ValueError("SGDLossScaler: init_scale > 0, growth >= 1, 0 < backoff <= 1, an integer window >= 0 and max_scale > 0 are required")
        self.growth, self.backoff, self.window, self.max_scale = float(growth), float(backoff), int(window), float(max_scale)
        self.init_scale = float(init_scale)
        self._host = [self.init_scale, 0.0, 0.0, 0.0]
        self._found = False
        self._dev = self._ctl = None

    @staticmethod
    def rule(state, found, growth, backoff, window, max_scale):
        """One update of [scale, clean, skipped, skipped in a row] in f32 arithmetic, as the kernel's thread 0 applies it -> the new list."""
        import numpy as np
        f = np.float32
        scale, clean, skipped, row = (f(v) for v in state)
        if found:
            with np.errstate(under="ignore"):
                return [float(scale * f(backoff) if window != 0 else scale), 0.0, float(skipped + f(1)), float(row + f(1))]
        clean = clean + f(1)
        if clean == f(window):
            with np.errstate(over="ignore"):
                return [float(min(f(max_scale), scale * f(growth))), 0.0, float(skipped), 0.0]
        return [float(scale), float(clean), float(skipped), 0.0]

    def host_update(self, found):
        """The rule on the host copy of the state -> the new scale."""
        if self._dev is not None:
            raise RuntimeError("SGDLossScaler.host_update: the state lives on the device (ecamp_sgd_scale_update moves it)")
        self._host = self.rule(self._host, bool(found), self.growth, self.backoff, self.window, self.max_scale)
        self._found = bool(found)
        return self._host[0]

    def state(self, device=None):
        """The device f32[4] (created from the host copy on first use, on `device`)."""
        if self._dev is None:
            if device is None:
                raise RuntimeError("SGDLossScaler: no device state yet (scale_loss / FusedSGD.step_scaled create it)")
            self._dev = torch.tensor(self._host, device=device, dtype=torch.float32)
            self._ctl = torch.tensor([1.0 / self._host[0], 0.0, 0.0, 0.0], device=device, dtype=torch.float32)
        return self._dev

    @property
    def ctl(self):
        """The device f32[4] the last update wrote for `ecamp_sgd_grouped`: {1 / scale of that step, skipped, 0, 0}."""
        return self._ctl

    def scale_loss(self, loss):
        """loss * scale, the scale read on the device."""
        return loss * self.state(loss.device)[0]

    def update(self, partials, npart, norm_out=None):
        """One `ecamp_sgd_scale_update` over `partials[0:npart]` (sums of squares of the scaled gradients) -> `ctl`."""
        state = self.state(partials.device)
        ops.sgd_scale_update(partials, npart, state, self._ctl, norm_out, self.growth, self.backoff, self.window, self.max_scale)
        return self._ctl

    def _read(self):
        if self._dev is not None:
            self._host = [float(v) for v in self._dev.tolist()]
            self._found = bool(self._ctl[1].item() != 0)
        return self._host

    scale = property(lambda self: self._read()[0])
    clean_steps = property(lambda self: int(self._read()[1]))
    skipped_steps = property(lambda self: int(self._read()[2]))
    skipped_in_a_row = property(lambda self: int(self._read()[3]))

    @property
    def last_found_inf(self):
        self._read()
        return self._found

    def describe(self):
        """The rule in words, from the constructor's arguments alone (the driver's opening line)."""
        def num(v):   # 1048576 (2^20), not 1.04858e+06
            m, e = math.frexp(v)
            return "%d (2^%d)" % (v, e - 1) if m == 0.5 and v >= 1 else "%g" % v

        if self.window == 0:
            return "a static loss scale of %s (a step whose gradients are not finite is skipped)" % num(self.init_scale)
        return ("a dynamic loss scale from %s: x %g and the step skipped when the scaled gradients are not finite, x %g after %d clean steps "
                "in a row, at most %s" % (num(self.init_scale), self.backoff, self.growth, self.window, num(self.max_scale)))
