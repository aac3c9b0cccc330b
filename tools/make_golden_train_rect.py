#!/usr/bin/env python3
"""Generate tests/golden/train_rect.part<i>.npz (one part per case, read back as one record by helpers.load_golden('train_rect'):
the whole record is over the size limit of a committed file): the REFERENCE's own autograd training step (CPU, fp32;
`l_pix = netG(data); l_pix.backward(); Adam.step()` of model/model.py:50-55) on batches whose image size is NOT the config's image_size, with the
tiny weights that are already committed (tests/golden/sr3_tiny.npz, ddpm_tiny.npz).  The reference's p_losses trains on whatever
size the loader yields; the fixture pins oracle/sr3_oracle.py to it there, and the GPU tests check the engine's fused
forward + backward (plan option train_geom) against it.

    python tools/make_golden_train_rect.py /path/to/reference/checkout

The reference is imported, never modified or copied: dropout is 0, the noise z is injected by swapping torch.randn_like for a
function that replays it while p_losses runs, and the draw of gamma (SR3, numpy's global generator) / t (DDPM, torch's) is made
reproducible by seeding that generator and drawing the same values a second time for the record.  Cases: sr3_tiny at 16x24 and
24x16, ddpm_tiny at 16x24, sr3_tiny at 80x64 (its attention level is 40x32 = 1280 tokens: beyond the LDS score strip).  Only
data goes into the fixture: inputs, the loss sum, every parameter gradient, the weights after one Adam step."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from helpers import CONDITIONAL, DESCS, SCHEDS, load_golden      # noqa: E402
from make_golden_rect import replay_randn                         # noqa: E402

CASES = [('sr3_tiny', 16, 24, 2), ('sr3_tiny', 24, 16, 2), ('ddpm_tiny', 16, 24, 2), ('sr3_tiny', 80, 64, 1)]      # (network, H, W, batch)
SEED = 20241017


def reference_net(networks, name):
    d, s = DESCS[name], SCHEDS[name]
    opt = {'phase': 'train', 'gpu_ids': None, 'distributed': False,
           'model': {'which_model_G': d['variant'], 'finetune_norm': False,
                     'unet': dict(in_channel=d['in_channel'], out_channel=d['out_channel'], inner_channel=d['inner_channel'],
                                  norm_groups=d['norm_groups'], channel_multiplier=d['channel_mults'], attn_res=d['attn_res'],
                                  res_blocks=d['res_blocks'], dropout=0),
                     'beta_schedule': {'train': dict(s), 'val': dict(s)},
                     'diffusion': dict(image_size=d['image_size'], channels=3, conditional=CONDITIONAL[name])}}
    netG = networks.define_G(opt)
    _, sd = load_golden(name)
    netG.set_loss('cpu')
    netG.set_new_noise_schedule(s, 'cpu')
    netG.load_state_dict(sd, strict=True)
    netG.train()
    return netG


def main(ref):
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref)
    import model.networks as networks            # the reference package
    torch.set_num_threads(1)
    for i, (name, H, W, B) in enumerate(CASES):
        out = {}
        k = '%s/%dx%d/' % (name, H, W)
        T = SCHEDS[name]['n_timestep']
        torch.manual_seed(SEED + i)
        netG = reference_net(networks, name)
        hr = torch.rand(B, 3, H, W) * 2 - 1
        sr = torch.rand(B, 3, H, W) * 2 - 1
        z = torch.randn(B, 3, H, W)
        data = {'HR': hr, 'SR': sr}
        if DESCS[name]['variant'] == 'sr3':
            np.random.seed(SEED + i)
            t_draw = np.random.randint(1, T + 1)
            gam = np.random.uniform(netG.sqrt_alphas_cumprod_prev[t_draw - 1], netG.sqrt_alphas_cumprod_prev[t_draw], size=B)
            out[k + 'gamma'] = torch.FloatTensor(gam).numpy()
            np.random.seed(SEED + i)
        else:
            torch.manual_seed(SEED + 100 + i)
            out[k + 't'] = torch.randint(0, T, (B,)).long().numpy()
            torch.manual_seed(SEED + 100 + i)
        with replay_randn([z]):
            loss = netG(data)
        optim = torch.optim.Adam(list(netG.parameters()), lr=1e-4)
        optim.zero_grad()
        l_pix = loss.sum() / int(hr.numel())          # model/model.py:52-53
        l_pix.backward()
        out[k + 'hr'], out[k + 'sr'], out[k + 'z'] = hr.numpy(), sr.numpy(), z.numpy()
        out[k + 'loss_sum'] = loss.detach().numpy()
        out[k + 'l_pix'] = l_pix.detach().numpy()
        for key, p in netG.named_parameters():
            out[k + 'grad/' + key] = p.grad.detach().numpy().copy()
        optim.step()
        for key, p in netG.named_parameters():
            out[k + 'adam1/' + key] = p.detach().numpy().copy()
        path = os.path.join(ROOT, 'tests', 'golden', 'train_rect.part%d.npz' % i)
        np.savez_compressed(path, **out)
        print(path, '%.1f KB' % (os.path.getsize(path) / 1024))
        assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
