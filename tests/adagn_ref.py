"""A res block with scale-shift time conditioning (config key model.unet.scale_shift_norm; ADM's use_scale_shift_norm) restated, in the
dtype of its inputs -- float64 weights give the float64 reference.

    e = Linear(temb) (SR3) | Linear(swish(temb)) (DDPM), of width 2 Cout
    scale, shift = e[:, :Cout], e[:, Cout:]
    h  = conv1(silu(GN1(x)))                                   (bias only: no row is added)
    h2 = GN2(h) * (1 + scale[:, :, None, None]) + shift[:, :, None, None]
    out = conv2(dropout(silu(h2))) + res(x)

* `resnet_block(sd, p, x, temb, groups, variant, drop=None)`: the block, in oracle.sr3_oracle.resnet_block's signature.  unet_forward
  resolves resnet_block as a module global, so `monkeypatch.setattr(O, 'resnet_block', adagn_ref.resnet_block)` yields the whole-UNet
  reference of such a network and, through p_losses_sr3 / p_losses_ddpm, its float64 autograd reference;
* `scale_shift(sd, p, temb, variant)`: the block's two rows;
* `modulated_norm(h, groups, gamma, beta, scale, shift)`: the normalisation alone, what the per-op entries fold and differentiate.
"""
import torch
import torch.nn.functional as F

from oracle import sr3_oracle as O


def scale_shift(sd, p, temb, variant):
    if variant == 'sr3':
        e = F.linear(temb, sd[p + '.noise_func.noise_func.0.weight'], sd[p + '.noise_func.noise_func.0.bias'])
    else:
        e = F.linear(O.swish(temb), sd[p + '.mlp.1.weight'], sd[p + '.mlp.1.bias'])
    e = e.reshape(temb.shape[0], -1)
    return torch.chunk(e, 2, dim=1)


def modulated_norm(h, groups, gamma, beta, scale, shift):
    """GN(h) (1 + scale) + shift on an NCHW tensor; scale, shift: [B, C]."""
    n = F.group_norm(h, groups, gamma, beta, eps=1e-5)
    return n * (1 + scale[:, :, None, None]) + shift[:, :, None, None]


def resnet_block(sd, p, x, temb, groups, variant, drop=None):
    h = O.block(sd, p + '.block1', x, groups)
    scale, shift = scale_shift(sd, p, temb, variant)
    h = modulated_norm(h, groups, sd[p + '.block2.block.0.weight'], sd[p + '.block2.block.0.bias'], scale, shift)
    h = O.swish(h)
    if drop is not None:
        h = h * O.dropout_mask(tuple(h.shape), *drop).to(h.device)
    h = F.conv2d(h, sd[p + '.block2.block.3.weight'], sd[p + '.block2.block.3.bias'], padding=1)
    if (p + '.res_conv.weight') in sd:
        res = F.conv2d(x, sd[p + '.res_conv.weight'], sd[p + '.res_conv.bias'])
    else:
        res = x
    return h + res
