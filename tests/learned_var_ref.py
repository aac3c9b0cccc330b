"""Float64 restatements for the learned reverse-process variance (tests/test_learned_var_cpu.py, tests/test_gpu_learned_var.py), written
from the formulas of Nichol & Dhariwal 2021 ("Improved DDPM") as DESIGN.md 3.3h states them: the respaced walk's tables, the hybrid
loss L_simple + lambda L_vlb with its gradient from autograd (mu_theta detached), one ancestral step -- and the same per-element
arithmetic in NumPy fp32, in the kernels' operation order, which is what the GPU tests' tolerances are measured with.

The network's output is [B, 2C, H, W]: C prediction channels, then C raw variance channels v;  f = (v + 1) / 2,
log sigma^2 = f log beta + (1 - f) log beta~."""
import math

import numpy as np
import torch

F = np.float32
LN2 = math.log(2.0)
K = math.sqrt(2.0 / math.pi)


# ---- the walk ---------------------------------------------------------------------------------------------------------------------------

def walk_tables(ac, S):
    """The respaced DDPM walk over tau = round(linspace(0, T - 1, S)), evaluated entry by entry in float64: dict of [S] arrays tau, beta,
    beta_tilde, c1, c2, log_beta, log_beta_tilde (entry 0 := entry 1), a, b (eps-prediction)."""
    ac = np.asarray(ac, dtype=np.float64)
    T = ac.shape[0]
    tau = np.round(np.linspace(0, T - 1, S)).astype(np.int64) if S > 1 else np.array([T - 1], dtype=np.int64)
    out = {k: np.zeros(S) for k in ('beta', 'beta_tilde', 'c1', 'c2', 'log_beta', 'log_beta_tilde', 'a', 'b')}
    for j in range(S):
        ab = ac[tau[j]]
        ap = ac[tau[j - 1]] if j > 0 else 1.0
        beta = 1.0 - ab / ap
        out['beta'][j] = beta
        out['beta_tilde'][j] = beta * (1.0 - ap) / (1.0 - ab)
        out['c1'][j] = beta * math.sqrt(ap) / (1.0 - ab)
        out['c2'][j] = (1.0 - ap) * math.sqrt(1.0 - beta) / (1.0 - ab)
        out['log_beta'][j] = math.log(beta)
        out['log_beta_tilde'][j] = math.log(out['beta_tilde'][j]) if j > 0 else 0.0
        out['a'][j] = math.sqrt(1.0 / ab)
        out['b'][j] = math.sqrt(1.0 / ab - 1.0)
    out['log_beta_tilde'][0] = out['log_beta_tilde'][1] if S > 1 else out['log_beta'][0]
    out['tau'] = tau
    return out


def step_scalars(tabs, t):
    """[n, 8] float64 rows {a, b, c1, c2, log beta, log beta~, last, 0} of the steps t of `walk_tables`."""
    t = np.asarray(t, dtype=np.int64).reshape(-1)
    rows = np.zeros((t.shape[0], 8))
    for k, name in enumerate(('a', 'b', 'c1', 'c2', 'log_beta', 'log_beta_tilde')):
        rows[:, k] = tabs[name][t]
    rows[:, 6] = (t == 0)
    return rows


# ---- the loss, float64 torch ------------------------------------------------------------------------------------------------------------

def approx_cdf(u):
    return 0.5 * (1.0 + torch.tanh(K * (u + 0.044715 * u ** 3)))


def _cols(scal, like):
    s = torch.as_tensor(scal, dtype=torch.float64)
    return [s[:, k].reshape(-1, *([1] * (like.dim() - 1))) for k in range(7)]


def vlb_bits(x0, xt, out_c, v, scal):
    """Per-element L_vlb term in bits, float64 [B, C, ...]: the KL of the true posterior against N(mu_theta, sigma_theta^2) where the
    row's `last` is 0, the negative discretised-Gaussian log-likelihood of x0 where it is not.  mu_theta is detached."""
    a, b, c1, c2, lb, lt, last = _cols(scal, x0)
    x0h = a * xt - b * out_c                                   # no clamp, as in the paper's training
    mu_t = (c1 * x0h + c2 * xt).detach()
    mu_q = c1 * x0 + c2 * xt
    f = (v + 1.0) / 2.0
    lv = f * lb + (1.0 - f) * lt
    kl = 0.5 * (-1.0 + lv - lt + torch.exp(lt - lv) + (mu_q - mu_t) ** 2 * torch.exp(-lv)) / LN2
    cx = x0 - mu_t
    inv = torch.exp(-0.5 * lv)
    cp, cm = approx_cdf(inv * (cx + 1.0 / 255.0)), approx_cdf(inv * (cx - 1.0 / 255.0))
    lp = torch.where(x0 < -0.999, torch.log(cp.clamp(min=1e-12)),
                     torch.where(x0 > 0.999, torch.log((1.0 - cm).clamp(min=1e-12)), torch.log((cp - cm).clamp(min=1e-12))))
    return torch.where(last != 0, -lp / LN2, kl)


def nll_conditioning(x0, xt, out_c, v, scal, ulps=4.0):
    """How far an fp32 evaluation of the last-step term may move, summed over the elements, in bits: the argument of the log is a CDF
    value or a difference of two, each an fp32 number near 1 known to `ulps` units of 2^-23 (tanh to a few ulp), so the log moves by
    (ulps 2^-23 / argument) / ln 2.  The reference's own conditioning; 0 for the KL rows.  float64."""
    a, b, c1, c2, lb, lt, last = _cols(scal, x0)
    x0, xt, out_c, v = x0.double(), xt.double(), out_c.double(), v.double()
    mu_t = c1 * (a * xt - b * out_c) + c2 * xt
    f = (v + 1.0) / 2.0
    inv = torch.exp(-0.5 * (f * lb + (1.0 - f) * lt))
    cp, cm = approx_cdf(inv * (x0 - mu_t + 1.0 / 255.0)), approx_cdf(inv * (x0 - mu_t - 1.0 / 255.0))
    arg = torch.where(x0 < -0.999, cp, torch.where(x0 > 0.999, 1.0 - cm, cp - cm)).clamp(min=1e-12)
    return float((torch.where(last != 0, ulps * 2.0 ** -23 / arg, torch.zeros_like(arg)) / LN2).sum())


def rho(d, kind, delta=1.0):
    if kind == 'l1':
        return d.abs()
    if kind == 'l2':
        return d ** 2
    a = d.abs()
    return torch.where(a <= delta, 0.5 * a ** 2, delta * (a - 0.5 * delta))


def hybrid_loss(z, hr, xt, out, scal, lam, kind='l1', delta=1.0, tgt=None, weight=None):
    """(sum w rho(d) + lam sum vlb, sum vlb) in float64; out [B, 2C, ...] may require grad.  tgt: (tgt_z [B], tgt_x0 [B]) or None (z)."""
    C = hr.shape[1]
    z, hr, xt = z.double(), hr.double(), xt.double()
    pred, v = out[:, :C], out[:, C:]
    shape = (-1,) + (1,) * (hr.dim() - 1)
    target = z if tgt is None else tgt[0].double().reshape(shape) * z + tgt[1].double().reshape(shape) * hr
    w = 1.0 if weight is None else weight.double().reshape(shape)
    simple = (w * rho(target - pred, kind, delta)).sum()
    vlb = vlb_bits(hr, xt, pred, v, scal).sum()
    return simple + lam * vlb, vlb


# ---- the loss's variance term, NumPy fp32 in the kernel's operation order (k_hybrid_loss_grad) -----------------------------------------

def vlb_f32(x0, xt, out_c, v, scal):
    """(vlb, d vlb / d v) per element in fp32 NumPy: what the tolerance of the GPU test is measured with."""
    s = np.asarray(scal, dtype=F)
    a, b, c1, c2, lb, lt, last = [s[:, k].reshape(-1, *([1] * (x0.ndim - 1))) for k in range(7)]
    x0, xt, out_c, v = (np.asarray(t, dtype=F) for t in (x0, xt, out_c, v))
    RLN2 = F(1.4426950408889634)
    x0h = a * xt - b * out_c
    f = F(0.5) * (v + F(1.0))
    lv = f * lb + (F(1.0) - f) * lt
    dlv = F(0.5) * (lb - lt)
    d = c1 * (x0 - x0h)
    r, q = np.exp(lt - lv), d * d * np.exp(-lv)
    kl = F(0.5) * (F(-1.0) + lv - lt + r + q) * RLN2
    dkl = F(0.5) * (F(1.0) - r - q) * dlv * RLN2
    cx = x0 - (c1 * x0h + c2 * xt)
    inv = np.exp(F(-0.5) * lv)
    up, um = inv * (cx + F(1.0) / F(255.0)), inv * (cx - F(1.0) / F(255.0))

    def cdf(u):
        th = np.tanh(F(K) * (u + F(0.044715) * u * u * u))
        return F(0.5) * (F(1.0) + th), F(0.5) * (F(1.0) - th * th) * F(K) * (F(1.0) + F(3.0) * F(0.044715) * u * u)
    (cp, pp), (cm, pm) = cdf(up), cdf(um)
    lo, hi = x0 < F(-0.999), x0 > F(0.999)
    arg = np.where(lo, cp, np.where(hi, F(1.0) - cm, cp - cm))
    darg = np.where(lo, pp * (F(-0.5) * up), np.where(hi, pm * (F(0.5) * um), pp * (F(-0.5) * up) + pm * (F(0.5) * um)))
    opened = arg >= F(1e-12)
    safe = np.where(opened, arg, F(1.0))
    nll = -np.log(np.where(opened, arg, F(1e-12))) * RLN2
    dnll = np.where(opened, -(darg / safe) * dlv * RLN2, F(0.0))
    is_last = np.broadcast_to(last != 0, x0.shape)
    out, dv = np.where(is_last, nll, kl), np.where(is_last, dnll, dkl)
    assert out.dtype == F and dv.dtype == F
    return out, dv


# ---- one ancestral step ----------------------------------------------------------------------------------------------------------------

def ancestral_step(x, out, z, row, clip=True, last=False):
    """x_{j-1} of one learned-variance step in float64: row = (a, b, c1, c2, log beta, log beta~) of step j; `last`: no noise."""
    a, b, c1, c2, lb, lt = (float(v) for v in row)
    C = x.shape[1]
    x, out = x.double(), out.double()
    x0 = a * x - b * out[:, :C]
    if clip:
        x0 = x0.clamp(-1.0, 1.0)
    mean = c1 * x0 + c2 * x
    if last or z is None:
        return mean
    f = (out[:, C:] + 1.0) / 2.0
    return mean + torch.exp(0.5 * (f * lb + (1.0 - f) * lt)) * z.double()


def sigma_f32(v, lb, lt):
    """sigma of k_learned_var_step in fp32 NumPy, the kernel's operation order."""
    v = np.asarray(v, dtype=F)
    f = F(0.5) * (v + F(1.0))
    s = np.exp(F(0.5) * (f * F(lb) + (F(1.0) - f) * F(lt)))
    assert s.dtype == F
    return s


# ---- fixtures --------------------------------------------------------------------------------------------------------------------------

def widen_rows(sd, seed=11, spread=0.5):
    """A 3-row state dict -> a 6-row one whose first three filter rows are the old ones and whose variance rows are seeded: the
    checkpoint of a learned-variance network that shares its prediction with the 3-row network."""
    sd = dict(sd)
    gen = torch.Generator().manual_seed(seed)
    for k in list(sd):
        if k.endswith('final_conv.block.3.weight') or k.endswith('final_conv.block.3.bias'):
            w = sd[k]
            extra = torch.randn(w.shape, generator=gen) * (w.std() if w.dim() > 1 else 1.0) * spread
            sd[k] = torch.cat([w, extra.to(w.dtype)], 0).contiguous()
    return sd
