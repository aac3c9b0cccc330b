"""Optimizer face for the engine (reference: torch.optim.Adam in model/model.py:39-40,54-55).

The gradients are produced by the engine's fused forward+backward (`EngineUNet.train_step`, called from
`GaussianDiffusion.p_losses`); this object owns Adam's moments as two arena-shaped buffers and applies
the update with one fused kernel over the whole parameter arena (sr3_adam_step) -- or, with the EMA of the weights
enabled (config train.ema_scheduler.enabled), sr3_adam_ema_step: the same pass with the EMA arena as one more stream.

Two engine keys of config train.optimizer sit between the gradients and that kernel, both off unless set: `accumulate` (K calls of
`step` make one optimizer step on the in-order fp32 sum of their gradients: sr3_grad_accumulate) and `clip_grad_norm` (the gradient is
scaled to that global L2 norm on the device, and a non-finite norm skips the update: sr3_grad_norm, sr3_adam_ema_step_scaled).
"""
import ctypes as C

import torch

from . import lib as L


def warmup_lr(lr, step, warmup_steps):
    """Linear warm-up (config train.optimizer.warmup_steps): the learning rate of the 1-based optimizer step `step`,
    lr * min(1, step / warmup_steps) as a Python float; warmup_steps = 0: lr."""
    return lr if warmup_steps <= 0 else lr * min(1.0, step / warmup_steps)


def ema_mode(step, step_start_ema, update_ema_every):
    """What the 1-based optimizer step `step` does to the EMA of the weights (sr3_adam_ema_step's ema_mode): 0 nothing (not an
    update step), 1 copy the new weights (before step_start_ema), 2 move towards them by 1 - ema_decay."""
    if step % update_ema_every != 0:
        return 0
    return 1 if step < step_start_ema else 2


def accumulate_schedule(micro, accumulate):
    """(first, last) of the 0-based micro-batch `micro` (calls of `step` since the run or the resume began) under config
    train.optimizer.accumulate = K: `first` starts a new sum (acc = g instead of acc += g), `last` closes it -- the optimizer
    step is taken.  K = 1: every micro-batch is both."""
    k = micro % accumulate
    return k == 0, k == accumulate - 1


def check_accumulate(value):
    """config train.optimizer.accumulate: an integer >= 1 (absent / None: 1)."""
    if value is None:
        return 1
    if isinstance(value, bool) or not isinstance(value, int) or value < 1:
        raise ValueError('train.optimizer.accumulate must be an integer >= 1 (got %r)' % (value,))
    return value


def check_clip_grad_norm(value):
    """config train.optimizer.clip_grad_norm: a number > 0, or absent / None (no clipping)."""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not value > 0:
        raise ValueError('train.optimizer.clip_grad_norm must be a number > 0 or null (got %r)' % (value,))
    return float(value)


class EngineAdam(object):
    def __init__(self, netG, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, warmup_steps=0, ema=None, accumulate=None, clip_grad_norm=None):
        """`ema`: None (no EMA: `step` is the plain sr3_adam_step call) or a dict with step_start_ema, update_ema_every and
        ema_decay (config train.ema_scheduler with `enabled`); the EMA tensor itself belongs to the UNet (EngineUNet.ema_arena).
        Neither setting is part of state_dict(): both come from the config, and the step count they depend on is Adam's.
        `accumulate` (K >= 1) / `clip_grad_norm` (c > 0 or None): see `step`; with both off nothing below allocates or launches
        anything new.  Neither is in state_dict() either, nor is a partial sum: a resumed run starts a fresh accumulation."""
        self.netG = netG
        self.accumulate = check_accumulate(accumulate)
        self.clip_grad_norm = check_clip_grad_norm(clip_grad_norm)
        netG.denoise_fn.accumulate = self.accumulate      # the training step scales its gradients by 1 / K (EngineUNet.train_step)
        self.micro_count = 0          # calls of `step` (micro-batches); `step_count` counts optimizer steps
        self.grad_acc = None          # accumulate > 1: the running sum, arena-shaped
        self.norm4 = None             # clip_grad_norm: device floats {norm, coef, finite flag, 0} of the last optimizer step
        self._norm_scratch = None
        self.defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0, amsgrad=False)
        self.warmup_steps = int(warmup_steps)
        if self.warmup_steps < 0:
            raise ValueError('warmup_steps must be >= 0 (got %d)' % self.warmup_steps)
        self.ema = None
        if ema is not None:
            self.ema = dict(step_start_ema=int(ema['step_start_ema']), update_ema_every=int(ema['update_ema_every']),
                            ema_decay=float(ema['ema_decay']))
            if self.ema['update_ema_every'] < 1 or not 0.0 <= self.ema['ema_decay'] < 1.0:
                raise ValueError('ema_scheduler: update_ema_every >= 1 and 0 <= ema_decay < 1 are required (got %s)' % self.ema)
        self.step_count = 0
        self.exp_avg = None
        self.exp_avg_sq = None

    def zero_grad(self):
        pass                        # every gradient is overwritten by the next train_step

    def _moments(self, arena):
        if self.exp_avg is None or self.exp_avg.device != arena.device:
            self.exp_avg = torch.zeros_like(arena) if self.exp_avg is None else self.exp_avg.to(arena.device)
            self.exp_avg_sq = torch.zeros_like(arena) if self.exp_avg_sq is None else self.exp_avg_sq.to(arena.device)

    def last_grad_norm(self):
        """0-dim device tensor: the global gradient norm (before clipping) of the last optimizer step taken; None without
        clip_grad_norm or before the first such step."""
        return None if self.norm4 is None else self.norm4[0]

    def _gradient(self, un, stream):
        """accumulate / clip_grad_norm: fold this micro-batch into the sum and, on the last one of K, return the gradient the
        optimizer step applies (None before that), its norm / coef / flag in `norm4` when clipping is on.  Data parallel with
        K > 1: the accumulated arena is all-reduced here, once per optimizer step, before the norm -- every rank gets the same coef."""
        lib = L.load()
        g = un.grad_arena
        n, K, clip = g.numel(), self.accumulate, self.clip_grad_norm
        scratch, nbytes = None, 0
        if clip is not None:
            if self._norm_scratch is None or self._norm_scratch.device != g.device:
                self._norm_scratch = torch.empty(int(lib.sr3_grad_norm_scratch_bytes(n)), dtype=torch.uint8, device=g.device)
            scratch, nbytes = L.ptr(self._norm_scratch), self._norm_scratch.numel()
        max_norm = C.c_float(clip or 0.0)

        def norm4():          # (allocated with the first norm: last_grad_norm() is None until a step has one)
            if self.norm4 is None or self.norm4.device != g.device:
                self.norm4 = torch.zeros(4, dtype=torch.float32, device=g.device)
            return L.ptr(self.norm4)
        if K == 1:
            L.check(lib.sr3_grad_norm(L.ptr(g), n, max_norm, scratch, nbytes, norm4(), stream))
            return g
        first, last = accumulate_schedule(self.micro_count, K)
        self.micro_count += 1
        if self.grad_acc is None or self.grad_acc.device != g.device:
            self.grad_acc = torch.empty_like(g)
        dp = un.dp_reducing()
        fused = last and clip is not None and not dp          # the norm of the sum from the pass that forms it
        L.check(lib.sr3_grad_accumulate(L.ptr(self.grad_acc), L.ptr(g), n, int(first), max_norm, scratch, nbytes,
                                        norm4() if fused else None, stream))
        if not last:
            return None
        if dp:
            un.reduce_arena(self.grad_acc)
        if clip is not None and not fused:
            L.check(lib.sr3_grad_norm(L.ptr(self.grad_acc), n, max_norm, scratch, nbytes, norm4(), stream))
        return self.grad_acc

    def step(self):
        """One micro-batch.  accumulate = K > 1: the first K - 1 calls of every K only add `grad_arena` to the sum (no update, no
        weights_changed(), step_count untouched); the K-th applies one optimizer step on the sum -- the mean over the K
        micro-batches, as train_step scales each by 1 / K.  clip_grad_norm = c: the step runs sr3_adam_ema_step_scaled on the
        norm / coef / flag sr3_grad_norm left on the device -- torch.nn.utils.clip_grad_norm_(params, c) over the whole parameter
        set, except that a non-finite norm skips the update on the device (weights, moments and EMA keep their bits) instead of
        writing NaN; step_count advances all the same, as nothing is read back."""
        un = self.netG.denoise_fn
        arena = un.arena.data
        if getattr(un, 'grad_arena', None) is None:
            raise L.Sr3Error('optimizer step without gradients: call netG(data) first')
        stream = C.c_void_p(torch.cuda.current_stream(arena.device).cuda_stream)
        grads = un.grad_arena
        if self.accumulate > 1 or self.clip_grad_norm is not None:
            grads = self._gradient(un, stream)
            if grads is None:
                return
        self._moments(arena)
        self.step_count += 1
        d = self.defaults
        lr = warmup_lr(d['lr'], self.step_count, self.warmup_steps)
        e = self.ema
        if e is not None and (un.ema_arena is None or un.ema_arena.device != arena.device):
            raise L.Sr3Error('EMA is enabled but the UNet holds no EMA arena on %s (EngineUNet.enable_ema)' % arena.device)
        mode = 0 if e is None else ema_mode(self.step_count, e['step_start_ema'], e['update_ema_every'])
        lib = L.load()
        state = (L.ptr(arena), L.ptr(grads), L.ptr(self.exp_avg), L.ptr(self.exp_avg_sq))
        hyper = (arena.numel(), C.c_float(lr), C.c_float(d['betas'][0]), C.c_float(d['betas'][1]), C.c_float(d['eps']), self.step_count)
        ema = (None if e is None else L.ptr(un.ema_arena),) + hyper + (C.c_float(0.0 if e is None else e['ema_decay']), mode)
        if self.clip_grad_norm is not None:
            L.check(lib.sr3_adam_ema_step_scaled(*state, *ema, L.ptr(self.norm4), stream))
        elif e is None:
            L.check(lib.sr3_adam_step(*state, *hyper, stream))
        else:
            L.check(lib.sr3_adam_ema_step(*state, *ema, stream))
        un.weights_changed()            # the Winograd filters of the inference plan are stale now

    # ---- checkpoint format: torch.optim.Adam's (model/model.py:137-142, 160-163) --------------------------
    # One state entry per parameter in `netG.parameters()` order (= the plan table order, which is the
    # reference's registration order), moments in the reference shapes (OIHW), so `*_opt.pth` files are
    # interchangeable with the reference in both directions.
    def state_dict(self):
        un = self.netG.denoise_fn
        plan = un.plan
        state = {}
        if self.exp_avg is not None and self.step_count > 0:
            for i, e in enumerate(plan.table):
                state[i] = {'step': torch.tensor(float(self.step_count)),
                            'exp_avg': plan.view(self.exp_avg, e).detach().cpu().clone().contiguous(),
                            'exp_avg_sq': plan.view(self.exp_avg_sq, e).detach().cpu().clone().contiguous()}
        d = self.defaults
        group = {'lr': d['lr'], 'betas': tuple(d['betas']), 'eps': d['eps'], 'weight_decay': 0, 'amsgrad': False,
                 'maximize': False, 'foreach': None, 'capturable': False, 'differentiable': False, 'fused': None,
                 'params': list(range(len(plan.table)))}
        return {'state': state, 'param_groups': [group]}

    def load_state_dict(self, sd):
        un = self.netG.denoise_fn
        plan = un.plan
        groups = sd.get('param_groups') or [{}]
        for k in ('lr', 'eps'):
            if k in groups[0]:
                self.defaults[k] = groups[0][k]
        if 'betas' in groups[0]:
            self.defaults['betas'] = tuple(groups[0]['betas'])
        self.micro_count = 0            # (a checkpoint carries no partial sum: the accumulation starts afresh)
        state = sd.get('state', {})
        if not state:
            self.step_count = 0
            return
        if len(state) != len(plan.table):
            raise ValueError('optimizer state has %d entries, the model has %d parameters' % (len(state), len(plan.table)))
        arena = un.arena.data
        self.exp_avg = torch.zeros_like(arena)
        self.exp_avg_sq = torch.zeros_like(arena)
        steps = set()
        for i, e in enumerate(plan.table):
            st = state[i] if i in state else state[str(i)]
            if tuple(st['exp_avg'].shape) != tuple(e['shape']):
                raise ValueError('optimizer state %d (%s): shape %s vs %s' % (i, e['name'], tuple(st['exp_avg'].shape), e['shape']))
            plan.view(self.exp_avg, e).copy_(st['exp_avg'].to(arena.device, torch.float32))
            plan.view(self.exp_avg_sq, e).copy_(st['exp_avg_sq'].to(arena.device, torch.float32))
            steps.add(int(float(st['step'])))
        if len(steps) != 1:
            raise ValueError('per-parameter Adam step counts differ: %s' % sorted(steps))
        self.step_count = steps.pop()


def make_optimizer(netG, lr, warmup_steps=0, ema=None, accumulate=None, clip_grad_norm=None):
    return EngineAdam(netG, lr=lr, warmup_steps=warmup_steps, ema=ema, accumulate=accumulate, clip_grad_norm=clip_grad_norm)
