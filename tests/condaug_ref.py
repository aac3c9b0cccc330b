"""CPU restatements for noise conditioning augmentation (tests/test_condaug_cpu.py, tests/test_gpu_condaug.py): the kernel's arithmetic in
NumPy fp32, the training step and one reverse step on the unchanged oracle (oracle/sr3_oracle.py, whose UNet and losses are generic in
in_channel), and the fixtures: the golden 6-channel models widened to in_channel = 7.

Channel order of the network's input under the level channel, as the engine's virtual concat reads it: [LR (Cl) | level (1) | x (C)]."""
import numpy as np
import torch

from helpers import DESCS, load_golden, opt_for
from oracle import sr3_oracle as O

F = np.float32
FIRST = 'denoise_fn.downs.0.weight'


def desc7(name):
    return dict(DESCS[name], in_channel=7)


def widened(name, seed=11):
    """(golden record, state dict) of fixture `name` with its first conv widened from [LR | x] to [LR | level | x]: the golden filters
    where they were, seeded filters of the same spread for the new input plane."""
    g, sd = load_golden(name)
    w = sd[FIRST]
    gen = torch.Generator().manual_seed(seed)
    extra = torch.randn(w.shape[0], 1, 3, 3, generator=gen) * w.std()
    sd = dict(sd)
    sd[FIRST] = torch.cat([w[:, :3], extra, w[:, 3:]], dim=1).contiguous()
    return g, sd


def opt7(name, phase='val', aug=None, gpu=True, in_channel=7, **diffusion):
    """opt_for(name) with in_channel 7 and the model.diffusion.cond_augment key (aug None: key absent)."""
    opt = opt_for(name, phase=phase, gpu=gpu)
    opt['model']['unet']['in_channel'] = in_channel
    if aug is not None:
        opt['model']['diffusion']['cond_augment'] = aug
    opt['model']['diffusion'].update(diffusion)
    return opt


# ---- the coefficients and the kernel ----------------------------------------------------------------------------------------------------

def level_coefs(s):
    """(a, s) as fp32 arrays: s rounded to fp32, then a = sqrt(1 - s^2) in float64 of that fp32 s, rounded once."""
    s32 = np.asarray(s, dtype=F).reshape(-1)
    a32 = np.sqrt(1.0 - s32.astype(np.float64) ** 2).astype(F)
    return a32, s32


def augment_f32(src, eps, a, s):
    """a c + s eps per image on fp32 arrays: two products and a sum, each rounded on its own; an image at level 0 is src itself.
    eps None: src."""
    src = np.asarray(src, dtype=F)
    if eps is None:
        return src.copy()
    a4, s4 = (np.asarray(t, dtype=F).reshape(-1, 1, 1, 1) for t in (a, s))
    with np.errstate(invalid='ignore'):
        out = a4 * src + s4 * np.asarray(eps, dtype=F)
    assert out.dtype == F
    return np.where(s4 == 0, src, out)


def augment(dst, src, eps, a, s, keep, level_channel, first):
    """What sr3_cond_augment_f32 leaves in dst [B, Cd, H, W]: channels first .. first + Cl - 1 <- keep[b] ? a c + s eps : +0.0, channel
    first + Cl <- keep[b] ? s[b] : +0.0 with the level channel, the rest as it was."""
    want = np.array(dst, dtype=F, copy=True)
    cl = src.shape[1]
    k4 = np.ones((src.shape[0], 1, 1, 1), bool) if keep is None else np.asarray(keep).reshape(-1, 1, 1, 1) != 0
    want[:, first:first + cl] = np.where(k4, augment_f32(src, eps, a, s), F(0.0))
    if level_channel:
        want[:, first + cl] = np.where(k4[:, 0], np.asarray(s, dtype=F).reshape(-1, 1, 1), F(0.0))
    return want


def network_cond(sr, eps, levels, keep=None, level_channel=True):
    """The conditioning tensor the network reads, as a torch fp32 tensor: the kernel's output on a fresh [B, Cl (+ 1), H, W] buffer."""
    a, s = level_coefs(levels)
    sr = sr.numpy()
    dst = np.zeros((sr.shape[0], sr.shape[1] + (1 if level_channel else 0)) + sr.shape[2:], F)
    return torch.from_numpy(augment(dst, sr, None if eps is None else eps.numpy(), a, s, keep, level_channel, 0))


# ---- training ---------------------------------------------------------------------------------------------------------------------------

def p_losses(sd, desc, hr, cond, gamma, z, prediction='eps'):
    """The SR3 training step in float64 on the oracle's UNet under autograd, on the conditioning tensor `cond` as the network reads it
    (L1, sum-reduced; target z or v = ca z - cb x0).  -> (loss, {key: d(loss / numel) / d param})"""
    sdr = {k: (v.double().clone().requires_grad_(k.startswith('denoise_fn.')) if v.is_floating_point() else v) for k, v in sd.items()}
    b = hr.shape[0]
    hr, cond, z = hr.double(), cond.double(), z.double()
    g = gamma.double().view(b, 1)
    g4 = g.view(-1, 1, 1, 1)
    x_noisy = O.q_sample_sr3(hr, g4, z)
    out = O.unet_forward(sdr, desc, torch.cat([cond, x_noisy], dim=1), g)
    target = z if prediction == 'eps' else g4 * z - (1 - g4 ** 2).sqrt() * hr
    loss = (target - out).abs().sum()
    params = {k: v for k, v in sdr.items() if v.is_floating_point() and v.requires_grad}
    grads = torch.autograd.grad(loss / hr.numel(), list(params.values()))
    return float(loss.detach()), {k[len('denoise_fn.'):]: gr for k, gr in zip(params, grads)}


# ---- sampling: one step -----------------------------------------------------------------------------------------------------------------

KEYS = ('a', 'b', 'c1', 'c2', 'sigma')


def sample_step(sd, desc, cond, x, level, tabs, j, z, hist=None):
    """One reverse step of an SR3 chain at step index j, from the state before it: the oracle's UNet (fp32) on cat(cond, x) at `level`,
    the clamped x0, then the tail in the kernels' operations and association (tabs: fp32 arrays a, b, c1, c2, sigma, and c3 with
    `hist`).  -> (x', hist' or None), NumPy fp32."""
    B = x.shape[0]
    with torch.no_grad():
        out = O.unet_forward(sd, desc, torch.cat([cond, x], dim=1), torch.full((B, 1), float(level), dtype=torch.float32)).numpy()
    xn = x.numpy()
    a, b, c1, c2, sg = (F(tabs[k][j]) for k in KEYS)
    x0 = np.clip(a * xn - b * out, F(-1.0), F(1.0))
    mean = c1 * x0 + c2 * xn
    if hist is not None:
        mean = mean + F(tabs['c3'][j]) * np.asarray(hist, dtype=F)
    new = mean + (np.zeros_like(xn) if z is None else np.asarray(z, dtype=F)) * sg
    assert new.dtype == F
    return new, (x0 if hist is not None else None)
