"""The reference's multi-head SelfAttention.forward (model/sr3_modules/unet.py:113-142, n_head heads) restated, in the dtype of its
inputs -- float64 weights give the float64 reference.

* `self_attention(sd, p, x, groups, n_head)`: the whole module, in oracle.sr3_oracle.self_attention's signature plus the head count
  (n_head = 1 is that function, operation for operation);
* `patched(n_head=..., head_dim=...)`: the same with the head count bound, to stand in for oracle.sr3_oracle.self_attention (which
  unet_forward resolves as a module global) -- the whole-UNet reference of a multi-head network;
* `core(qkv, C, n_head)`: the attention core alone on the engine's NHWC tensor [B][N][3C] -> [B][N][C], what the per-op entries compute.
"""
import math

import torch
import torch.nn.functional as F


def self_attention(sd, p, x, groups, n_head=1):
    b, c, hh, ww = x.shape
    norm = F.group_norm(x, groups, sd[p + '.norm.weight'], sd[p + '.norm.bias'], eps=1e-5)
    qkv = F.conv2d(norm, sd[p + '.qkv.weight'])
    q, k, v = qkv.view(b, n_head, 3 * (c // n_head), hh, ww).chunk(3, dim=2)
    attn = torch.einsum('bnchw,bncyx->bnhwyx', q, k).contiguous() / math.sqrt(c)
    attn = torch.softmax(attn.view(b, n_head, hh, ww, -1), -1).view(b, n_head, hh, ww, hh, ww)
    out = torch.einsum('bnhwyx,bncyx->bnchw', attn, v).contiguous()
    out = F.conv2d(out.view(b, c, hh, ww), sd[p + '.out.weight'], sd[p + '.out.bias'])
    return out + x


def patched(n_head=None, head_dim=None):
    assert (n_head is None) != (head_dim is None)

    def fn(sd, p, x, groups):
        return self_attention(sd, p, x, groups, n_head if head_dim is None else x.shape[1] // head_dim)
    return fn


def core(qkv, C, n_head):
    """qkv [B][N][3C], head h on channels [3 d h, 3 d (h + 1)) as q | k | v; out [B][N][C], head h on [d h, d (h + 1))."""
    B, N, _ = qkv.shape
    q, k, v = qkv.view(B, N, n_head, 3 * (C // n_head)).chunk(3, dim=3)           # each [B][N][H][d]
    p = torch.softmax(torch.einsum('bmhc,bnhc->bhmn', q, k) / math.sqrt(C), -1)
    return torch.einsum('bhmn,bnhc->bmhc', p, v).reshape(B, N, C)
