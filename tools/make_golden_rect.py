#!/usr/bin/env python3
"""Generate tests/golden/sr3_rect.npz: the REFERENCE's own UNet / GaussianDiffusion (CPU, fp32) on rectangular inputs, with
the `sr3_tiny` weights that are already committed (tests/golden/sr3_tiny.npz).  The fixture pins oracle/sr3_oracle.py to the
reference at image sizes other than the config's image_size; the GPU tests then check the engine against the oracle there.

    python tools/make_golden_rect.py /path/to/reference/checkout

The reference is imported, never modified or copied: the random draws of its reverse loop are made reproducible by swapping
torch.randn / torch.randn_like for functions that replay a pre-drawn sequence while it runs (as oracle/make_golden.py does).
Only data goes into the fixture (inputs, noise, outputs)."""
import contextlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from helpers import DESCS, SCHEDS, load_golden      # noqa: E402

SHAPES = [(16, 24), (24, 16)]
BATCH = 2


@contextlib.contextmanager
def replay_randn(seq):
    it = iter(seq)
    o_randn, o_like = torch.randn, torch.randn_like

    def randn(*a, **k):
        return next(it).clone()

    def randn_like(x, **k):
        z = next(it).clone()
        assert z.shape == x.shape
        return z
    torch.randn, torch.randn_like = randn, randn_like
    try:
        yield
    finally:
        torch.randn, torch.randn_like = o_randn, o_like


def main(ref):
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref)
    import model.networks as networks            # the reference package
    d, s = DESCS['sr3_tiny'], SCHEDS['sr3_tiny']
    opt = {'phase': 'val', 'gpu_ids': None, 'distributed': False,
           'model': {'which_model_G': 'sr3', 'finetune_norm': False,
                     'unet': dict(in_channel=d['in_channel'], out_channel=d['out_channel'], inner_channel=d['inner_channel'],
                                  norm_groups=d['norm_groups'], channel_multiplier=d['channel_mults'], attn_res=d['attn_res'],
                                  res_blocks=d['res_blocks'], dropout=0),
                     'beta_schedule': {'train': dict(s), 'val': dict(s)},
                     'diffusion': dict(image_size=d['image_size'], channels=3, conditional=True)}}
    torch.set_num_threads(1)
    torch.manual_seed(20240607)
    netG = networks.define_G(opt)
    _, sd = load_golden('sr3_tiny')
    netG.set_new_noise_schedule(s, 'cpu')          # (registers the schedule buffers the committed state dict carries too)
    netG.load_state_dict(sd, strict=True)
    netG.eval()
    T = s['n_timestep']
    out = {}
    for H, W in SHAPES:
        k = '%dx%d/' % (H, W)
        x = torch.randn(BATCH, d['in_channel'], H, W).clamp(-3, 3)
        level = torch.rand(BATCH, 1) * 0.98 + 0.01
        with torch.no_grad():
            eps = netG.denoise_fn(x, level)
        out[k + 'unet/x'], out[k + 'unet/time'], out[k + 'unet/eps'] = x.numpy(), level.numpy(), eps.numpy()
        sr = torch.rand(BATCH, 3, H, W) * 2 - 1
        x_T = torch.randn(BATCH, 3, H, W)
        zs = [torch.randn(BATCH, 3, H, W) for _ in range(T)]                 # zs[i] is consumed at step i
        xs = torch.randn(BATCH, 3, H, W)
        t = T // 2
        with replay_randn([zs[t]]), torch.no_grad():
            step = netG.p_sample(xs, t, condition_x=sr)
        order = [x_T] + [zs[i] for i in reversed(range(T)) if i > 0]         # the reference draws nothing at t == 0
        with replay_randn(order), torch.no_grad():
            loop = netG.super_resolution(sr, continous=True)
        out[k + 'step/x'], out[k + 'step/t'], out[k + 'step/out'] = xs.numpy(), np.int64(t), step.numpy()
        out[k + 'loop/sr'], out[k + 'loop/x_T'], out[k + 'loop/zs'] = sr.numpy(), x_T.numpy(), torch.stack(zs).numpy()
        out[k + 'loop/ret_continous'] = loop.numpy()
    path = os.path.join(ROOT, 'tests', 'golden', 'sr3_rect.npz')
    np.savez_compressed(path, **out)
    print(path, '%.1f KB' % (os.path.getsize(path) / 1024))


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
