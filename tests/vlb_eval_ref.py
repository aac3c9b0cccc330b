"""Restatements for the variational bound by timestep and the loss-aware timestep sampler (tests/test_t_sampler_cpu.py,
tests/test_gpu_vlb_eval.py).  The per-element term is learned_var_ref's (`vlb_bits` in float64, `vlb_f32` in fp32 NumPy in
the kernels' operation order), imported, not restated; what is new here stands around it:

  * the clamp of x0^ before mu_theta: `vlb_bits` / `vlb_f32` form x0^ = a x_t - b out themselves, so they are handed out = x0^ (clamped
    here) under rows with a = 0, b = -1 -- 0 x_t - (-1) x0^ is x0^ exactly, in float64 and in fp32
  * the fixed-variance modes: v = -1 (log sigma^2 = log beta~) and v = +1 (log beta)
  * the per-image means, the prior term, and the resampler of Nichol & Dhariwal 2021, section 3.3"""
import math

import numpy as np
import torch

import learned_var_ref as R

F = np.float32
LN2 = math.log(2.0)


def _split(out, C, var_mode):
    """(prediction planes, v) of `out` [B, OC, ...] under var_mode 0 (learned: OC = 2C), 1 (v = -1) or 2 (v = +1)."""
    pred = out[:, :C]
    if var_mode == 0:
        return pred, out[:, C:]
    fill = -1.0 if var_mode == 1 else 1.0
    return pred, (torch.full_like(pred, fill) if torch.is_tensor(pred) else np.full_like(pred, fill))


def _x0_rows(scal):
    """The rows with the x0 rule replaced by the identity on `out`: a = 0, b = -1."""
    s = np.array(scal, dtype=np.float64, copy=True)
    s[:, 0], s[:, 1] = 0.0, -1.0
    return s


def terms64(x0, xt, out, scal, var_mode=0, clip=True):
    """(vlb [B, C, ...] in bits, (x0 - x0^)^2) per element in float64; scal: [B, 8] rows, one per image."""
    x0, xt, out = x0.double(), xt.double(), out.double()
    pred, v = _split(out, x0.shape[1], var_mode)
    s = torch.as_tensor(np.asarray(scal), dtype=torch.float64)
    shape = (-1,) + (1,) * (x0.dim() - 1)
    x0h = s[:, 0].reshape(shape) * xt - s[:, 1].reshape(shape) * pred
    if clip:
        x0h = x0h.clamp(-1.0, 1.0)
    return R.vlb_bits(x0, xt, x0h, v, _x0_rows(scal)), (x0 - x0h) ** 2


def terms32(x0, xt, out, scal, var_mode=0, clip=True):
    """The same in fp32 NumPy, the kernel's operation order: what the tolerance is measured with."""
    x0, xt, out = (np.asarray(t, dtype=F) for t in (x0, xt, out))
    pred, v = _split(out, x0.shape[1], var_mode)
    s = np.asarray(scal, dtype=F)
    shape = (-1,) + (1,) * (x0.ndim - 1)
    x0h = s[:, 0].reshape(shape) * xt - s[:, 1].reshape(shape) * pred
    if clip:
        x0h = np.minimum(np.maximum(x0h, F(-1.0)), F(1.0))
    vlb, _ = R.vlb_f32(x0, xt, x0h, v, _x0_rows(np.asarray(scal, dtype=F).astype(np.float64)))
    d = x0 - x0h
    assert vlb.dtype == F and d.dtype == F
    return vlb, d * d


def per_image(t):
    """Mean over everything but the batch axis, float64 [B]."""
    t = torch.as_tensor(np.asarray(t), dtype=torch.float64) if not torch.is_tensor(t) else t.double()
    return t.reshape(t.shape[0], -1).mean(1)


def nll_cond_per_image(x0, xt, out, scal, var_mode=0, clip=True):
    """learned_var_ref.nll_conditioning per image, as a bound on the image's MEAN: [B] float64 (0 for the KL rows)."""
    x0, xt, out = x0.double(), xt.double(), out.double()
    pred, v = _split(out, x0.shape[1], var_mode)
    s = torch.as_tensor(np.asarray(scal), dtype=torch.float64)
    shape = (-1,) + (1,) * (x0.dim() - 1)
    x0h = s[:, 0].reshape(shape) * xt - s[:, 1].reshape(shape) * pred
    if clip:
        x0h = x0h.clamp(-1.0, 1.0)
    rows = _x0_rows(scal)
    n = x0[0].numel()
    return torch.tensor([R.nll_conditioning(x0[b:b + 1], xt[b:b + 1], x0h[b:b + 1], v[b:b + 1], rows[b:b + 1]) / n
                         for b in range(x0.shape[0])], dtype=torch.float64)


def prior_scalars(abar):
    """(sqrt(abar), 1 - abar, log(1 - abar)) in float64: what the host hands sr3_prior_bpd_f32, rounded once."""
    return math.sqrt(abar), 1.0 - abar, math.log(1.0 - abar)


def prior64(x0, abar):
    """KL(N(sqrt(abar) x0, 1 - abar) || N(0, 1)) in bits per element, float64."""
    sa, var, lv = prior_scalars(abar)
    return 0.5 * (-1.0 - lv + var + (sa * x0.double()) ** 2) / LN2


def prior32(x0, abar):
    sa, var, lv = (F(v) for v in prior_scalars(abar))
    m = sa * np.asarray(x0, dtype=F)
    out = F(0.5) * (F(-1.0) - lv + var + m * m) * F(1.4426950408889634)
    assert out.dtype == F
    return out


class Resampler:
    """The loss-second-moment resampler, restated with per-step Python lists: the last `history` losses of every step; uniform until
    each step has that many; then p = (1 - u) sqrt(mean(L^2)) / sum + u / T."""

    def __init__(self, T, history=10, uniform=0.001):
        self.T, self.history, self.uniform = T, history, uniform
        self.seen = [[] for _ in range(T)]

    def update(self, t, losses):
        for k, v in zip(t, losses):
            self.seen[int(k)] = (self.seen[int(k)] + [float(v)])[-self.history:]

    def probabilities(self):
        if any(len(s) < self.history for s in self.seen):
            return np.full(self.T, 1.0 / self.T)
        w = np.array([math.sqrt(sum(v * v for v in s) / self.history) for s in self.seen])
        p = w / w.sum()
        return p * (1.0 - self.uniform) + self.uniform / self.T

    def weights(self, t):
        p = self.probabilities()
        return np.array([1.0 / (self.T * p[int(k)]) for k in t])
