"""Optimizer face for the engine (reference: torch.optim.Adam in model/model.py:39-40,54-55).

The gradients are produced by the engine's fused forward+backward (`EngineUNet.train_step`, called from
`GaussianDiffusion.p_losses`); this object owns Adam's moments as two arena-shaped buffers and applies
the update with one fused kernel over the whole parameter arena (sr3_adam_step) -- or, with the EMA of the weights
enabled (config train.ema_scheduler.enabled), sr3_adam_ema_step: the same pass with the EMA arena as one more stream.
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


class EngineAdam(object):
    def __init__(self, netG, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, warmup_steps=0, ema=None):
        """`ema`: None (no EMA: `step` is the plain sr3_adam_step call) or a dict with step_start_ema, update_ema_every and
        ema_decay (config train.ema_scheduler with `enabled`); the EMA tensor itself belongs to the UNet (EngineUNet.ema_arena).
        Neither setting is part of state_dict(): both come from the config, and the step count they depend on is Adam's."""
        self.netG = netG
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

    def step(self):
        un = self.netG.denoise_fn
        arena = un.arena.data
        if getattr(un, 'grad_arena', None) is None:
            raise L.Sr3Error('optimizer step without gradients: call netG(data) first')
        self._moments(arena)
        self.step_count += 1
        d = self.defaults
        lr = warmup_lr(d['lr'], self.step_count, self.warmup_steps)
        stream = C.c_void_p(torch.cuda.current_stream(arena.device).cuda_stream)
        if self.ema is None:
            L.check(L.load().sr3_adam_step(L.ptr(arena), L.ptr(un.grad_arena), L.ptr(self.exp_avg), L.ptr(self.exp_avg_sq),
                                           arena.numel(), C.c_float(lr), C.c_float(d['betas'][0]),
                                           C.c_float(d['betas'][1]), C.c_float(d['eps']), self.step_count, stream))
        else:
            e = self.ema
            if un.ema_arena is None or un.ema_arena.device != arena.device:
                raise L.Sr3Error('EMA is enabled but the UNet holds no EMA arena on %s (EngineUNet.enable_ema)' % arena.device)
            mode = ema_mode(self.step_count, e['step_start_ema'], e['update_ema_every'])
            L.check(L.load().sr3_adam_ema_step(L.ptr(arena), L.ptr(un.grad_arena), L.ptr(self.exp_avg), L.ptr(self.exp_avg_sq),
                                               L.ptr(un.ema_arena), arena.numel(), C.c_float(lr), C.c_float(d['betas'][0]),
                                               C.c_float(d['betas'][1]), C.c_float(d['eps']), self.step_count,
                                               C.c_float(e['ema_decay']), mode, stream))
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


def make_optimizer(netG, lr, warmup_steps=0, ema=None):
    return EngineAdam(netG, lr=lr, warmup_steps=warmup_steps, ema=ema)
