"""Progressive distillation (Salimans & Ho 2022): train an N-step student from a 2N-step teacher.

A round has a teacher walk `tau2` of 2N timesteps (strictly increasing, the last one T - 1) with the nodes n_0 = 1 (clean) and
n_i = alphas_cumprod[tau2[i - 1]], i = 1 .. 2N.  The student walks `tau_s = tau2[1::2]`: its step k = 1 .. N goes from node 2k to node
2k - 2, which the frozen teacher covers in two deterministic DDIM steps through node 2k - 1.  With alpha = sqrt(n), sigma = sqrt(1 - n)
and the subscripts t, m, e for the nodes 2k, 2k - 1, 2k - 2, the x0 the student must predict at z_t to land where the teacher lands is

    D  = alpha_e - (sigma_e / sigma_t) alpha_t
    w1 = ((sigma_e / sigma_m) alpha_m - (sigma_e / sigma_t) alpha_t) / D
    w2 = (alpha_e - (sigma_e / sigma_m) alpha_m) / D                  (w1 + w2 = 1, both in [0, 1]; k = 1: 0 and 1)
    x~ = w1 x1 + w2 x2                                                  (x1, x2: the teacher's x0 predictions at t and at m)
    eps~ = (z_t - alpha_t x~) / sigma_t = s1 z_t - s2 x~

-- the teacher's end point z_e eliminated from the textbook target (z_e - (sigma_e / sigma_t) z_t) / D, whose numerator subtracts two
nearly equal numbers and whose 1 / D reaches the thousands on a fine walk.  Every coefficient is computed here in float64 and rounded
once to fp32; the device multiplies, adds, subtracts and clamps (csrc/distill.hip).

The student's step is the existing training step on (hr := x~, z := eps~, q_ca = alpha_t, q_cb = sigma_t): its q_sample rebuilds
alpha_t x~ + sigma_t eps~ = z_t to one rounding, and tgt_z eps~ + tgt_x0 x~ is the eps / v / x0 target of the student's own prediction
kind, so every loss and weight of `set_objective` applies unchanged.  v-prediction under the uniform weight is the paper's "SNR + 1"
weighting of the x0 error.
"""
import ctypes as C

import numpy as np
import torch

from . import lib as L
from .diffusion import EngineDiffusion
from .schedules import prediction_coefs, sampler_walk


def halve_walk(tau):
    """The student's walk of a teacher's: every second timestep, the last one kept (tau[1::2]); the length must be even."""
    tau = np.asarray(tau)
    if tau.ndim != 1 or tau.shape[0] < 2 or tau.shape[0] % 2:
        raise ValueError('halve_walk: a walk of an even number of timesteps is expected (got %r)' % (tau.tolist(),))
    return tau[1::2].astype(np.int64)


def distill_walks(alphas_cumprod, student_steps, walk='logsnr'):
    """(tau2, tau_s): the teacher's walk of 2 * student_steps timesteps -- `sampler_walk`'s 'time' / 'logsnr', or an explicit list (an
    earlier round's student walk) -- and the student's, tau2[1::2].  Pure numpy, no device."""
    if isinstance(student_steps, bool) or not isinstance(student_steps, (int, np.integer)) or int(student_steps) < 1:
        raise ValueError('distillation steps must be a positive integer (got %r)' % (student_steps,))
    T = int(np.asarray(alphas_cumprod).reshape(-1).shape[0])
    if 2 * int(student_steps) > T:
        raise ValueError('distillation to %d steps needs a teacher walk of %d timesteps, more than the schedule\'s %d'
                         % (student_steps, 2 * int(student_steps), T))
    tau2 = sampler_walk(alphas_cumprod, 2 * int(student_steps), walk)
    return tau2, halve_walk(tau2)


def _ddim_c(ab, ap):
    """c1, c2 of the deterministic DDIM step ab -> ap (`sampler_tables` with eta = 0)."""
    d = np.sqrt(np.maximum(1.0 - ap, 0.0))
    return np.sqrt(ap) - d * np.sqrt(ab) / np.sqrt(1.0 - ab), d / np.sqrt(1.0 - ab)


COEF_ROWS = ('alpha_t', 'sigma_t', 'alpha_m', 'a1', 'b1', 'c1', 'c2', 'a2', 'b2', 'w1', 'w2', 's1', 's2')      # the fp32 rows on the device


def distill_coefs(alphas_cumprod, tau2, k, prediction='eps'):
    """The coefficients of student step k (an int or an array of them, each in 1 .. N) on the teacher walk tau2, float64, no device:

        alpha_t, sigma_t, alpha_m, sigma_m, alpha_e, sigma_e    the three nodes 2k, 2k - 1, 2k - 2
        a1, b1, c1, c2        the teacher's first step, t -> m:  x0 = a1 z - b1 out ; z_m = c1 x0 + c2 z
        a2, b2, c1b, c2b      its second, m -> e (c1b, c2b: the end point the device never forms)
        w1, w2, s1, s2        the target (module docstring)
        t_node, t_mid         int64: the timesteps of the nodes t and m (what a DDPM network is conditioned on)

    a, b are `prediction_coefs` of the TEACHER's prediction kind."""
    ac = np.asarray(alphas_cumprod, dtype=np.float64).reshape(-1)
    tau2 = sampler_walk(ac, None, np.asarray(tau2))
    if tau2.shape[0] % 2:
        raise ValueError('distill_coefs: the teacher walk must have an even number of timesteps (got %d)' % tau2.shape[0])
    N = tau2.shape[0] // 2
    k = np.asarray(k)
    if k.dtype == np.bool_ or not np.issubdtype(k.dtype, np.integer) or (k.size and (k.min() < 1 or k.max() > N)):
        raise ValueError('distill_coefs: k must be integers in [1, %d] (got %r)' % (N, k.tolist()))
    node = np.append(1.0, ac[tau2])
    nt, nm, ne = node[2 * k], node[2 * k - 1], node[2 * k - 2]
    at, st, am, sm, ae, se = np.sqrt(nt), np.sqrt(1.0 - nt), np.sqrt(nm), np.sqrt(1.0 - nm), np.sqrt(ne), np.sqrt(1.0 - ne)
    a1, b1 = prediction_coefs(prediction, at, st)[:2]
    a2, b2 = prediction_coefs(prediction, am, sm)[:2]
    c1, c2 = _ddim_c(nt, nm)
    c1b, c2b = _ddim_c(nm, ne)
    D = ae - (se / st) * at
    w1 = ((se / sm) * am - (se / st) * at) / D
    w2 = (ae - (se / sm) * am) / D
    out = dict(alpha_t=at, sigma_t=st, alpha_m=am, sigma_m=sm, alpha_e=ae, sigma_e=se, a1=a1, b1=b1, c1=c1, c2=c2, a2=a2, b2=b2, c1b=c1b,
               c2b=c2b, w1=w1, w2=w2, s1=1.0 / st, s2=at / st)
    if not all(np.all(np.isfinite(v)) for v in out.values()):
        raise ValueError('distillation coefficients are not finite')
    out['t_node'], out['t_mid'] = tau2[2 * k - 1], tau2[2 * k - 2]
    return out


def _same_network(s, t):
    ps, pt = s.denoise_fn.plan, t.denoise_fn.plan
    return ([(e['name'], tuple(e['shape'])) for e in ps.table] == [(e['name'], tuple(e['shape'])) for e in pt.table]
            and ps.in_channel == pt.in_channel and ps.out_channel == pt.out_channel)


def _refuse_cond_augment(student, teacher):
    """noise conditioning augmentation is not built into the distillation step (when a Distiller is made, and again at every step: the
    setting may be switched on behind it)"""
    for what, m in (('student', student), ('teacher', teacher)):
        if getattr(m, 'cond_augment', None) is not None:
            raise NotImplementedError('cond_augment with train.distill: teacher and student read the conditioning batch as it is given '
                                      '(Distiller.step draws no level and makes no augmented tensor, and both would have to read the '
                                      'same one); switch noise conditioning augmentation off (set_cond_augment(None)) on the %s' % what)


def _refuse_feature_cache(student, teacher):
    """feature-cached sampling is a setting of the sampling loop (refused like cond_augment: when a Distiller is made, and at every step)"""
    for what, m in (('student', student), ('teacher', teacher)):
        if getattr(m, 'feature_cache', None) is not None:
            raise NotImplementedError('feature_cache with train.distill: the teacher\'s two steps are the whole network\'s at two nodes of '
                                      'its walk, with no step between them to take a cache from, and the student trains through the training '
                                      'plan, which has no shallow form; switch it off (set_feature_cache(None)) on the %s' % what)


class Distiller(object):
    """One round of progressive distillation: `step` trains `student` (an EngineDiffusion on a GPU) to do in one DDIM step what the
    frozen `teacher` -- a second network of the same variant, geometry and conditioning, with its own plan, arena and derived weights --
    does in two.  steps: N, the student's chain; walk: the teacher's walk of 2N timesteps ('time', 'logsnr' or an explicit list -- the
    student walk of the round before); guidance_scale: the teacher's output is the classifier-free-guided one at that scale (two
    teacher forwards per node; the student then needs one forward per step); clip: the teacher's x0 predictions are clamped to
    [-1, 1], as its sampling loop clamps them.  The teacher runs through its inference forward only and is never written."""

    def __init__(self, student, teacher, steps, walk='logsnr', guidance_scale=None, clip=True):
        for what, m in (('student', student), ('teacher', teacher)):      # (a setting is refused before the device is looked at)
            if getattr(m, 'self_condition', None) is not None:
                raise NotImplementedError('self-conditioning with train.distill: the teacher\'s two steps and the student\'s pass run without a '
                                          'first pass and write no x0 back (sr3_teacher_step_f32, sr3_distill_target_f32); switch '
                                          'self-conditioning off (set_self_condition(None)) on the %s' % what)
        _refuse_cond_augment(student, teacher)
        _refuse_feature_cache(student, teacher)
        for what, m in (('student', student), ('teacher', teacher)):
            if not isinstance(m, EngineDiffusion) or getattr(m, '_alphas_cumprod64', None) is None:
                raise ValueError('Distiller: the %s must be an EngineDiffusion with a noise schedule' % what)
            if m.betas.device.type != 'cuda' or m.denoise_fn.arena.device.type != 'cuda':
                raise L.Sr3Error('Distiller: the %s is on %s; distillation needs both models on a GPU, there is no CPU fallback'
                                 % (what, m.betas.device))
        if student is teacher or student.denoise_fn is teacher.denoise_fn:
            raise ValueError('Distiller: the teacher must be a network of its own (it is frozen while the student trains)')
        if student.variant != teacher.variant:
            raise ValueError('Distiller: the student is a %r model and the teacher a %r one' % (student.variant, teacher.variant))
        if student.conditional != teacher.conditional or student.channels != teacher.channels or not _same_network(student, teacher):
            raise ValueError('Distiller: student and teacher differ in network shape or conditioning')
        acs, act = student._alphas_cumprod64, teacher._alphas_cumprod64
        if acs.shape != act.shape or not np.array_equal(acs, act):
            raise ValueError('Distiller: student and teacher differ in noise schedule')
        if guidance_scale is not None:
            if isinstance(guidance_scale, bool) or not isinstance(guidance_scale, (int, float, np.integer, np.floating)) \
                    or not np.isfinite(float(guidance_scale)):
                raise ValueError('Distiller: guidance_scale must be a finite number (got %r)' % (guidance_scale,))
            if not teacher.conditional:
                raise ValueError('Distiller: guidance_scale on an unconditional model: there is no conditioning image to drop')
        self.student, self.teacher = student, teacher
        self.tau2, self.tau_s = distill_walks(acs, steps, walk)
        self.steps = int(steps)
        self.guidance_scale = None if guidance_scale is None else float(guidance_scale)
        self.clip = bool(clip)
        self.device = student.betas.device
        co = distill_coefs(acs, self.tau2, np.arange(1, self.steps + 1), teacher.prediction)
        self.coefs = co
        # row r of the device table: COEF_ROWS[r] at k = column + 1, the float64 values rounded once
        self._table = torch.tensor(np.stack([co[r] for r in COEF_ROWS]), dtype=torch.float32).to(self.device)
        self._level_host = torch.tensor(co['alpha_t'], dtype=torch.float32)
        self._t_node = torch.tensor(co['t_node'], dtype=torch.long).to(self.device)
        self._t_mid = torch.tensor(co['t_mid'], dtype=torch.long).to(self.device)
        self._bufs = {}

    def student_sampler(self):
        """The "sampler" dict the student is sampled with: DDIM, N steps, eta 0, on its own walk."""
        return dict(type='ddim', steps=self.steps, eta=0.0, walk=[int(v) for v in self.tau_s])

    def state(self):
        """What a checkpoint records of the round (`engine.distill` of *_opt.pth): the student's chain."""
        return dict(steps=self.steps, walk=[int(v) for v in self.tau_s])

    def _buffers(self, shape, cond_shape):
        key = (tuple(shape), None if cond_shape is None else tuple(cond_shape))
        bufs = self._bufs.get(key)
        if bufs is None:
            dev = self.device
            bufs = {n: torch.empty(shape, device=dev) for n in ('z_t', 'x_mid', 'x0_first', 'out_c', 'x_tgt', 'eps_tgt')}
            bufs['out_u'] = bufs['cond0'] = None
            if self.guidance_scale is not None and self.guidance_scale != 1.0:      # (scale 1: the conditional output alone, as set_guidance)
                bufs['out_u'] = torch.empty(shape, device=dev)
                bufs['cond0'] = torch.zeros(cond_shape, device=dev)
            self._bufs = {key: bufs}
        return bufs

    def _teacher_forwards(self, x, time, cond, bufs):
        un = self.teacher.denoise_fn
        un(x, time, cond=cond, out=bufs['out_c'])
        if bufs['out_u'] is not None:
            un(x, time, cond=bufs['cond0'], out=bufs['out_u'])

    def step(self, data, *, k=None, noise=None, drop_seed=None):
        """One training step of the student on the batch data = {'HR', 'SR'} (as p_losses takes it): draws k ~ randint(1, N + 1) per
        image and noise ~ randn from torch's RNG unless injected, forms z_t at node 2k, runs the teacher's two steps and the target
        kernels, then the student's train_step.  Returns the sum-reduced loss (0-dim device tensor) and leaves the gradients in the
        student's grad_arena, exactly as p_losses does."""
        st, te = self.student, self.teacher
        _refuse_cond_augment(st, te)
        _refuse_feature_cache(st, te)
        dev = self.device
        x_start = data['HR']
        if not torch.is_tensor(x_start) or x_start.device != dev or x_start.dim() != 4 or x_start.dtype != torch.float32:
            raise L.Sr3Error('Distiller.step: HR must be a (B, C, H, W) fp32 tensor on %s; there is no CPU fallback' % (dev,))
        x_start = x_start.contiguous()
        b, c, h, w = x_start.shape
        cond = None
        if st.conditional:
            cond = data['SR'].contiguous()
            if cond.device != dev or cond.shape[0] != b or tuple(cond.shape[2:]) != (h, w):
                raise L.Sr3Error('Distiller.step: the conditioning batch %s must be on %s with the batch and image size of HR %s'
                                 % (tuple(cond.shape), dev, tuple(x_start.shape)))
        if k is None:
            k = torch.randint(1, self.steps + 1, (b,))
        k = torch.as_tensor(k).reshape(-1).long().cpu()
        if k.numel() != b or int(k.min()) < 1 or int(k.max()) > self.steps:
            raise L.Sr3Error('Distiller.step: k must hold one student step in [1, %d] per image (got %s)' % (self.steps, k.tolist()))
        if noise is None:
            noise = torch.randn_like(x_start)
        noise = noise.contiguous()
        if tuple(noise.shape) != tuple(x_start.shape) or noise.device != dev:
            raise L.Sr3Error('Distiller.step: the noise %s must have the shape and device of HR %s' % (tuple(noise.shape), tuple(x_start.shape)))
        col = (k - 1).to(dev)
        rows = dict(zip(COEF_ROWS, self._table.index_select(1, col)))      # one gather: [rows, B], every row contiguous
        bufs = self._buffers(x_start.shape, None if cond is None else cond.shape)
        lib = L.load()
        per = c * h * w
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        ca, cb = rows['alpha_t'], rows['sigma_t']
        level = tstep = gamma = None
        if st.variant == 'sr3':
            level, time_t, time_m = ca, ca, rows['alpha_m']
            gamma = self._level_host[k - 1]
        else:
            tstep = time_t = self._t_node[col]
            time_m = self._t_mid[col]
        scale = 1.0 if bufs['out_u'] is None else self.guidance_scale
        clip = 1 if self.clip else 0
        L.check(lib.sr3_q_sample(L.ptr(x_start), L.ptr(noise), L.ptr(ca), L.ptr(cb), b, per, L.ptr(bufs['z_t']), stream))
        self._teacher_forwards(bufs['z_t'], time_t, cond, bufs)
        L.check(lib.sr3_teacher_step_f32(L.ptr(bufs['z_t']), L.ptr(bufs['out_c']), L.ptr(bufs['out_u']), scale, L.ptr(rows['a1']),
                                         L.ptr(rows['b1']), L.ptr(rows['c1']), L.ptr(rows['c2']), b, per, clip, L.ptr(bufs['x_mid']),
                                         L.ptr(bufs['x0_first']), stream))
        self._teacher_forwards(bufs['x_mid'], time_m, cond, bufs)
        L.check(lib.sr3_distill_target_f32(L.ptr(bufs['z_t']), L.ptr(bufs['x_mid']), L.ptr(bufs['out_c']), L.ptr(bufs['out_u']), scale,
                                           L.ptr(bufs['x0_first']), L.ptr(rows['a2']), L.ptr(rows['b2']), L.ptr(rows['w1']),
                                           L.ptr(rows['w2']), L.ptr(rows['s1']), L.ptr(rows['s2']), b, per, clip, L.ptr(bufs['x_tgt']),
                                           L.ptr(bufs['eps_tgt']), stream))
        return st.denoise_fn.train_step(bufs['x_tgt'], cond, bufs['eps_tgt'], ca, cb, level, tstep,
                                        grad_scale=1.0 / float(b * c * h * w), drop_seed=drop_seed,
                                        objective=st._train_objective(tstep, gamma, dev))
