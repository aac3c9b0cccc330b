#!/usr/bin/env python3
"""Generate tests/golden/sr3_long.npz: the REFERENCE's own UNet / GaussianDiffusion (CPU, fp32) at image sizes whose attention
level has more tokens than a 32-query score strip over all keys holds in LDS (80 x 64 -> 1280 tokens, 96 x 96 -> 2304 tokens),
with the `sr3_tiny` weights that are already committed (tests/golden/sr3_tiny.npz).  The fixture pins oracle/sr3_oracle.py to
the reference there; the GPU tests check the key-blocked attention kernel (plan option attn_long) against it.

    python tools/make_golden_long.py /path/to/reference/checkout

The reference is imported, never modified or copied; the one random draw of its p_sample is made reproducible by swapping
torch.randn_like for a function that replays a pre-drawn tensor while it runs (as tools/make_golden_rect.py does).  Only data goes
into the fixture, batch 1 and no full loop to keep it small: the UNet's input, noise level and output, and one p_sample step whose
inputs are the two halves of the UNet input (condition = channels 0-2, x_t = channels 3-5), its noise and its output."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from helpers import DESCS, SCHEDS, load_golden      # noqa: E402
from make_golden_rect import replay_randn           # noqa: E402

SHAPES = [(80, 64), (96, 96)]
BATCH = 1


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
    torch.manual_seed(20240611)
    netG = networks.define_G(opt)
    _, sd = load_golden('sr3_tiny')
    netG.set_new_noise_schedule(s, 'cpu')          # (registers the schedule buffers the committed state dict carries too)
    netG.load_state_dict(sd, strict=True)
    netG.eval()
    t = s['n_timestep'] // 2
    out = {}
    for H, W in SHAPES:
        k = '%dx%d/' % (H, W)
        x = torch.randn(BATCH, d['in_channel'], H, W).clamp(-3, 3)
        level = torch.rand(BATCH, 1) * 0.98 + 0.01
        with torch.no_grad():
            eps = netG.denoise_fn(x, level)
        out[k + 'unet/x'], out[k + 'unet/time'], out[k + 'unet/eps'] = x.numpy(), level.numpy(), eps.numpy()
        z = torch.randn(BATCH, 3, H, W)
        with replay_randn([z]), torch.no_grad():
            step = netG.p_sample(x[:, 3:].contiguous(), t, condition_x=x[:, :3].contiguous())
        out[k + 'step/t'], out[k + 'step/z'], out[k + 'step/out'] = np.int64(t), z.numpy(), step.numpy()
    path = os.path.join(ROOT, 'tests', 'golden', 'sr3_long.npz')
    np.savez_compressed(path, **out)
    print(path, '%.1f KB' % (os.path.getsize(path) / 1024))


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
