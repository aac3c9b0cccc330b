"""CPU restatements for self-conditioning (tests/test_selfcond_cpu.py, tests/test_gpu_selfcond.py): the write-back kernel's arithmetic in
NumPy fp32, the two-pass training step and one self-conditioned reverse step on the unchanged oracle (oracle/sr3_oracle.py, whose UNet
and losses are generic in in_channel and in the conditioning tensor's channel count), and the fixtures: the golden 6-channel models
widened to in_channel = 9.

Channel order of a self-conditioned network's input, as the engine's virtual concat reads it: [LR (Cl) | last x0 (C) | x (C)]."""
import numpy as np
import torch

from helpers import DESCS, load_golden, opt_for
from oracle import sr3_oracle as O

F = np.float32
FIRST = 'denoise_fn.downs.0.weight'


def desc9(name):
    return dict(DESCS[name], in_channel=9)


def widened(name, seed=7):
    """(golden record, state dict) of fixture `name` with its first conv widened from [LR | x] to [LR | self-cond | x]: the golden
    filters where they were, seeded filters of the same spread for the three new input channels."""
    g, sd = load_golden(name)
    w = sd[FIRST]
    gen = torch.Generator().manual_seed(seed)
    extra = torch.randn(w.shape[0], 3, 3, 3, generator=gen) * w.std()
    sd = dict(sd)
    sd[FIRST] = torch.cat([w[:, :3], extra, w[:, 3:]], dim=1).contiguous()
    return g, sd


def opt9(name, phase='val', prob=0.5, gpu=True, **diffusion):
    """opt_for(name) as a self-conditioned model: in_channel 9 and the model.diffusion.self_condition key (prob None: key absent)."""
    opt = opt_for(name, phase=phase, gpu=gpu)
    opt['model']['unet']['in_channel'] = 9
    if prob is not None:
        opt['model']['diffusion']['self_condition'] = {'prob': prob}
    opt['model']['diffusion'].update(diffusion)
    return opt


# ---- the write-back -------------------------------------------------------------------------------------------------------------------

def x0_f32(a, b, x, out, clip):
    """step_x0 of csrc/sr3_common.h on fp32 arrays: two products and a difference, each rounded on its own, then the clamp.
    a, b: scalars, or [B] arrays (one row per image)."""
    a, b = np.asarray(a, dtype=F), np.asarray(b, dtype=F)
    if a.ndim:
        a, b = a.reshape(-1, 1, 1, 1), b.reshape(-1, 1, 1, 1)
    x0 = a * np.asarray(x, dtype=F) - b * np.asarray(out, dtype=F)
    if clip:
        x0 = np.clip(x0, F(-1.0), F(1.0))
    assert x0.dtype == F
    return x0


def write_back(dst, x, out, a, b, keep, clip, first):
    """What sr3_selfcond_x0_f32 leaves in dst [B, Cd, H, W]: channels first .. first + C - 1 <- keep[b] ? x0 : +0.0, the rest as it was."""
    want = np.array(dst, dtype=F, copy=True)
    x0 = x0_f32(a, b, x, out, clip)
    if keep is not None:
        x0 = np.where(np.asarray(keep).reshape(-1, 1, 1, 1) != 0, x0, F(0.0))
    want[:, first:first + x0.shape[1]] = x0
    return want


def x0_coefs(prediction, ca):
    """a, b of x0 = a x - b out at the levels ca = sqrt(abar) (float64 in, rounded once to fp32): eps 1 / ca, cb / ca; v ca, cb; x0 0, -1."""
    ca = np.asarray(ca, dtype=np.float64)
    cb = np.sqrt(np.maximum(1.0 - ca ** 2, 0.0))
    a, b = {'eps': (1.0 / ca, cb / ca), 'v': (ca, cb), 'x0': (np.zeros_like(ca), -np.ones_like(ca))}[prediction]
    return a.astype(F), b.astype(F)


# ---- training: the two-pass step ------------------------------------------------------------------------------------------------------

def p_losses_two_pass(sd, desc, hr, sr, gamma, z, flags, prediction='eps'):
    """The self-conditioned SR3 training step in float64 on the oracle's UNet: a first pass under no_grad on cat(LR, 0, x_noisy), its
    clamped x0 kept for the flagged images, then the step itself on cat(LR, x0, x_noisy) under autograd (L1, sum-reduced; target z
    or v = ca z - cb x0).  -> (loss, {key: d(loss / numel) / d param}, the self-conditioning channels [B, C, H, W])"""
    sdr = {k: (v.double().clone().requires_grad_(k.startswith('denoise_fn.')) if v.is_floating_point() else v) for k, v in sd.items()}
    b = hr.shape[0]
    hr, sr, z = hr.double(), sr.double(), z.double()
    g = gamma.double().view(b, 1)
    g4 = g.view(-1, 1, 1, 1)
    x_noisy = O.q_sample_sr3(hr, g4, z)
    a, bb = (torch.from_numpy(t).double().view(-1, 1, 1, 1) for t in x0_coefs(prediction, gamma.double().numpy()))
    with torch.no_grad():
        out1 = O.unet_forward(sdr, desc, torch.cat([sr, torch.zeros_like(hr), x_noisy], dim=1), g)
        sc = (a * x_noisy - bb * out1).clamp(-1.0, 1.0) * torch.as_tensor(flags, dtype=torch.float64).view(-1, 1, 1, 1)
    out = O.unet_forward(sdr, desc, torch.cat([sr, sc, x_noisy], dim=1), g)
    target = z if prediction == 'eps' else g4 * z - (1 - g4 ** 2).sqrt() * hr
    loss = (target - out).abs().sum()
    params = {k: v for k, v in sdr.items() if v.is_floating_point() and v.requires_grad}
    grads = torch.autograd.grad(loss / hr.numel(), list(params.values()))
    return float(loss.detach()), {k[len('denoise_fn.'):]: gr for k, gr in zip(params, grads)}, sc


# ---- sampling: one self-conditioned step ----------------------------------------------------------------------------------------------

KEYS = ('a', 'b', 'c1', 'c2', 'sigma')


def sample_step(sd, desc, lr, sc, x, level, tabs, j, z, hist=None, x0_rule=None):
    """One reverse step of a self-conditioned SR3 chain at step index j, from the state before it: the oracle's UNet (fp32) on
    cat(LR, sc, x) at `level`, the raw clamped x0 = what is fed back, then the tail in the kernels' operations and association
    (tabs: fp32 arrays a, b, c1, c2, sigma, and c3 with `hist`; x0_rule: a function on the clamped x0 -- a rule on x0 -- or None).
    -> (x', the self-conditioning channels for the next step, hist' or None, the network's output), NumPy fp32."""
    B = x.shape[0]
    inp = torch.cat([t for t in (lr, sc, x) if t is not None], dim=1)
    with torch.no_grad():
        out = O.unet_forward(sd, desc, inp, torch.full((B, 1), float(level), dtype=torch.float32)).numpy()
    xn = x.numpy()
    a, b, c1, c2, sg = (F(tabs[k][j]) for k in KEYS)
    x0 = x0_f32(a, b, xn, out, True)
    x0p = x0 if x0_rule is None else x0_rule(x0)
    mean = c1 * x0p + c2 * xn
    if hist is not None:
        mean = mean + F(tabs['c3'][j]) * np.asarray(hist, dtype=F)
    new = mean + (np.zeros_like(xn) if z is None else np.asarray(z, dtype=F)) * sg
    assert new.dtype == F
    return new, x0, (x0p if hist is not None else None), out
