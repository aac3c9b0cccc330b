"""The feature-cached forward restated on the CPU oracle (checker only; tests/test_gpu_feature_cache*.py).

A cached forward of depth d is the UNet with everything below its last d up blocks frozen at an earlier input: `oracle.unet_forward`
at input A yields the branch tensor -- what enters the d-th last up block -- through its taps, and the shallow blocks are then run by
hand with `oracle.resnet_block` / `self_attention` on input B at level B."""
import torch
import torch.nn.functional as F

from oracle import sr3_oracle as O

TOL = 2e-5           # the project's step tolerance: err <= TOL * max(1, |ref|max)
# the case at a real width (tests/test_gpu_feature_cache.py): attention on the top resolution level, so the branch tensor of depth 1 / 2
# comes out of an attention's out projection and the shallow list holds an attention launch
WIDE = dict(variant='sr3', in_channel=6, out_channel=3, inner_channel=64, norm_groups=32, channel_mults=[1, 2], attn_res=[32],
            res_blocks=2, image_size=32)


def inputs(desc, B=2):
    """Two independent inputs A, B of a network (conditioning channels in front), at two different levels / timesteps."""
    g = torch.Generator().manual_seed(29)
    size = desc['image_size']
    xa, xb = (torch.randn(B, desc['in_channel'], size, size, generator=g) for _ in range(2))
    if desc['variant'] == 'sr3':
        ta, tb = torch.tensor([[0.93], [0.71]][:B]), torch.tensor([[0.35], [0.52]][:B])
    else:
        ta, tb = torch.tensor([5, 3][:B], dtype=torch.long), torch.tensor([1, 4][:B], dtype=torch.long)
    return xa, ta, xb, tb


def branch_name(desc, depth):
    """The tap that holds the branch tensor of depth `depth`: the output of the layer in front of the d-th last up block."""
    ups = O.unet_topology(desc)['ups']
    assert 1 <= depth <= desc['res_blocks'] + 1 and all(l['kind'] == 'res' for l in ups[len(ups) - depth:])
    first = len(ups) - depth
    return ups[first - 1]['name'] if first > 0 else 'mid.1'


def _temb(sd, desc, time, P):
    inner = desc['inner_channel']
    if desc['variant'] == 'sr3':
        e = O.positional_encoding(time, inner)
        e = F.linear(e, sd[P + 'noise_level_mlp.1.weight'], sd[P + 'noise_level_mlp.1.bias'])
        return F.linear(O.swish(e), sd[P + 'noise_level_mlp.3.weight'], sd[P + 'noise_level_mlp.3.bias'])
    e = O.time_embedding(time, inner, sd.get(P + 'time_mlp.0.inv_freq'))
    e = F.linear(e, sd[P + 'time_mlp.1.weight'], sd[P + 'time_mlp.1.bias'])
    return F.linear(O.swish(e), sd[P + 'time_mlp.3.weight'], sd[P + 'time_mlp.3.bias'])


def shallow_forward(sd, desc, depth, branch, x, time, prefix='denoise_fn.'):
    """eps of the shallow forward of depth `depth` on (x, time) -- x with the conditioning channels in front, as the UNet reads it --
    from a given branch tensor."""
    P, groups, variant = prefix, desc['norm_groups'], desc['variant']
    topo = O.unet_topology(desc)
    temb = _temb(sd, desc, time, P)

    def res(layer, h):
        n = P + layer['name']
        h = O.resnet_block(sd, n + '.res_block', h, temb, groups, variant)
        return O.self_attention(sd, n + '.attn', h, groups) if layer['attn'] else h
    feats, h = [], x
    for layer in topo['downs'][:depth]:
        n = P + layer['name']
        h = F.conv2d(h, sd[n + '.weight'], sd[n + '.bias'], padding=1) if layer['kind'] == 'conv' else res(layer, h)
        feats.append(h)
    h = branch
    for layer in topo['ups'][len(topo['ups']) - depth:]:
        h = res(layer, torch.cat((h, feats.pop()), dim=1))
    assert not feats
    return O.block(sd, P + 'final_conv', h, groups)


@torch.no_grad()
def cached_forward(sd, desc, depth, x_a, time_a, x_b, time_b, prefix='denoise_fn.'):
    """(eps of the full forward at A, eps of the cached forward at B on A's branch tensor, eps of the full forward at B)."""
    taps = {}
    full_a = O.unet_forward(sd, desc, x_a, time_a, prefix=prefix, taps=taps)
    cached_b = shallow_forward(sd, desc, depth, taps[branch_name(desc, depth)], x_b, time_b, prefix)
    return full_a, cached_b, O.unet_forward(sd, desc, x_b, time_b, prefix=prefix)
