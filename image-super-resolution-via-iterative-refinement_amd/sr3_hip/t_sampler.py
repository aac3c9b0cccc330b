"""Loss-aware timestep sampling (Nichol & Dhariwal 2021, "Improved DDPM", section 3.3; improved-diffusion's LossSecondMomentResampler):
L_vlb is a very noisy objective under a uniform t, so t is drawn with p_t proportional to sqrt(E[L_t^2]) and the loss of a drawn step is
weighted by 1 / (T p_t), which keeps the objective's expectation -- both terms of the hybrid loss: the weight goes into the objective's
per-image weight table (L_simple) and into sr3_train_step_ex3's vlb_weight (lambda L_vlb and the variance head's gradient).  E[L_t^2] is estimated from the last `history` per-image terms of
every step, which the training step returns (sr3_train_step_ex3: per_image_out[:, 0]).

Config key model.diffusion.t_sampler: {"type": "loss_second_moment", "history": 10, "uniform": 0.001}, or
EngineDiffusion.set_t_sampler.  Pure NumPy, float64, on the host; each data-parallel rank keeps its own history."""
import numpy as np

T_SAMPLER_TYPES = ('loss_second_moment',)
T_SAMPLER_HISTORY = 10
T_SAMPLER_UNIFORM = 0.001


def parse_t_sampler(spec):
    """The config key model.diffusion.t_sampler -> the keyword arguments of set_t_sampler, or None (absent / null / false: off)."""
    if spec is None or spec is False:
        return None
    if not isinstance(spec, dict):
        raise ValueError('t_sampler: a dict with "type" is expected (got %r)' % (spec,))
    for k in spec:
        if k not in ('type', 'history', 'uniform'):
            raise ValueError('t_sampler: unknown key %r (known: "type", "history", "uniform")' % (k,))
    kind = spec.get('type', 'loss_second_moment')
    if kind not in T_SAMPLER_TYPES:
        raise ValueError('t_sampler: unknown type %r (known: %s)' % (kind, ', '.join('"%s"' % t for t in T_SAMPLER_TYPES)))
    history, uniform = spec.get('history', T_SAMPLER_HISTORY), spec.get('uniform', T_SAMPLER_UNIFORM)
    if isinstance(history, bool) or not isinstance(history, int) or history < 1:
        raise ValueError('t_sampler: history must be an integer >= 1 (got %r)' % (history,))
    if isinstance(uniform, bool) or not isinstance(uniform, (int, float)) or not 0.0 <= float(uniform) <= 1.0:
        raise ValueError('t_sampler: uniform must be a number in [0, 1] (got %r)' % (uniform,))
    return dict(type=kind, history=int(history), uniform=float(uniform))


class LossSecondMomentResampler:
    """A [T, history] ring of per-step losses.  Uniform until every step has `history` entries; after that
    p = (1 - uniform) sqrt(mean(L^2)) / sum(...) + uniform / T."""

    def __init__(self, num_timesteps, history=T_SAMPLER_HISTORY, uniform=T_SAMPLER_UNIFORM):
        self.T, self.history, self.uniform = int(num_timesteps), int(history), float(uniform)
        self.losses = np.zeros((self.T, self.history), dtype=np.float64)
        self.counts = np.zeros(self.T, dtype=np.int64)

    def warmed_up(self):
        return bool((self.counts >= self.history).all())

    def probabilities(self):
        """p [T], float64, sums to 1."""
        if not self.warmed_up():
            return np.full(self.T, 1.0 / self.T)
        w = np.sqrt(np.mean(self.losses ** 2, axis=1))
        total = w.sum()
        if not (np.isfinite(total) and total > 0.0):      # (all-zero or non-finite history: nothing to prefer)
            return np.full(self.T, 1.0 / self.T)
        p = w / total
        p = p * (1.0 - self.uniform) + self.uniform / self.T
        return p / p.sum()

    def weights(self, t, p=None):
        """1 / (T p_t) of the steps t (0-based): the weights whose mean under p is 1."""
        p = self.probabilities() if p is None else p
        return 1.0 / (self.T * p[np.asarray(t, dtype=np.int64)])

    def update(self, t, losses):
        """Append loss k to step t[k]'s ring, in order; the oldest entry of a full ring is overwritten.  A non-finite loss is dropped."""
        t = np.asarray(t, dtype=np.int64).reshape(-1)
        losses = np.asarray(losses, dtype=np.float64).reshape(-1)
        if t.shape != losses.shape:
            raise ValueError('t_sampler: %d steps for %d losses' % (t.shape[0], losses.shape[0]))
        for k, v in zip(t, losses):
            if not 0 <= k < self.T:
                raise ValueError('t_sampler: step %d is outside [0, %d)' % (k, self.T))
            if not np.isfinite(v):
                continue
            self.losses[k, self.counts[k] % self.history] = v
            self.counts[k] += 1

    def state_dict(self):
        return dict(type='loss_second_moment', history=self.history, uniform=self.uniform, losses=self.losses.copy(), counts=self.counts.copy())

    def load_state_dict(self, state):
        losses, counts = np.asarray(state['losses'], dtype=np.float64), np.asarray(state['counts'], dtype=np.int64)
        if losses.shape != (self.T, self.history) or counts.shape != (self.T,):
            raise ValueError('t_sampler: the saved history %s / %s does not fit %d steps x %d entries'
                             % (losses.shape, counts.shape, self.T, self.history))
        self.losses, self.counts = losses.copy(), counts.copy()
