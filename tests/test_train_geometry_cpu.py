"""Training at an image size other than the config's image_size (plan option train_geom): host-only inspection of the training
plan's workspace, and the oracle's autograd step pinned to the reference's at rectangular shapes (tests/golden/train_rect.part*.npz,
tools/make_golden_train_rect.py).  CPU only: nothing here launches a kernel."""
import numpy as np
import pytest
import torch

from helpers import CONDITIONAL, DESCS, SCHEDS, load_golden
from oracle import sr3_oracle as O
from sr3_hip import engine as E

FULL = ('sr3', 6, 3, 64, 32, [1, 2, 4, 8, 8], [16], 2, 128)      # the headline SR3 16 -> 128 network
CASES = [('sr3_tiny', 16, 24), ('sr3_tiny', 24, 16), ('ddpm_tiny', 16, 24), ('sr3_tiny', 80, 64)]
TOL = 2e-6          # tests/test_oracle_golden.py: same torch CPU ops in a different call order


def train_ws(p, batch=2, cond=3):
    return int(p.lib.sr3_train_workspace_bytes(p.handle, batch, cond))


def test_training_workspace_follows_the_geometry():
    p = E.Plan(*FULL)
    native = train_ws(p)
    assert native > 0
    assert p.set_option('train_geom', 1) == 0
    assert train_ws(p) == native
    p.set_geometry(128, 192)
    rect = train_ws(p)
    assert rect > 0 and rect != native
    assert train_ws(p, batch=4) > rect            # the key covers the batch at this geometry too
    assert train_ws(p) == rect
    p.set_geometry(192, 128)
    assert train_ws(p) > 0
    p.set_geometry(0, 0)
    assert train_ws(p) == native
    # ... and without the option the refusal is what it was
    p.set_option('train_geom', 0)
    p.set_geometry(128, 192)
    assert train_ws(p) == 0
    assert b'image_size x image_size only' in p.lib.sr3_last_error()


@pytest.mark.parametrize('name', ['full', 'sr3_tiny', 'ddpm_tiny'])
def test_native_training_plan_is_the_same_under_the_option(name):
    def plan():
        if name == 'full':
            return E.Plan(*FULL), 3
        d = DESCS[name]
        return E.Plan(d['variant'], d['in_channel'], d['out_channel'], d['inner_channel'], d['norm_groups'], d['channel_mults'],
                      d['attn_res'], d['res_blocks'], d['image_size']), (3 if CONDITIONAL[name] else 0)
    a, cond = plan()
    b, _ = plan()
    b.set_option('train_geom', 1)
    assert a.op_list(2) == b.op_list(2)
    for batch in (1, 2, 16):
        assert train_ws(a, batch, cond) == train_ws(b, batch, cond) > 0
    assert a.workspace_bytes(2) == b.workspace_bytes(2)


def test_long_attention_levels_need_attn_long():
    p = E.Plan(*FULL)
    p.set_option('train_geom', 1)
    p.set_geometry(384, 384)
    assert train_ws(p) == 0
    msg = p.lib.sr3_last_error()
    assert b'attention' in msg and b'2304 tokens' in msg, msg
    p.set_option('attn_long', 1)
    sized = train_ws(p)
    assert sized > 0
    # the dK / dV slabs of the key-blocked backward: ceil(N / 32) query blocks x [B, N, 2 C] floats for the 48 x 48 level
    N, Cc, B = 48 * 48, 512, 2
    assert sized > (N // 32) * B * N * 2 * Cc * 4
    p.set_geometry(0, 0)
    q = E.Plan(*FULL)
    assert train_ws(p) == train_ws(q)


@pytest.fixture(scope='module')
def fixture():
    g, _ = load_golden('train_rect')
    return g


@pytest.mark.parametrize('name,H,W', CASES, ids=['%s_%dx%d' % c for c in CASES])
def test_oracle_autograd_step_matches_reference(fixture, name, H, W):
    k = '%s/%dx%d/' % (name, H, W)
    g = fixture
    _, sd = load_golden(name)
    d = DESCS[name]
    hr, sr, z = (torch.from_numpy(g[k + n]) for n in ('hr', 'sr', 'z'))
    assert tuple(hr.shape[2:]) == (H, W)
    sdr = {n: v.clone().requires_grad_(v.is_floating_point() and n.startswith('denoise_fn.')) for n, v in sd.items()}
    if d['variant'] == 'sr3':
        loss = O.p_losses_sr3(sdr, d, hr, sr, torch.from_numpy(g[k + 'gamma']), z, conditional=CONDITIONAL[name])
    else:
        loss = O.p_losses_ddpm(sdr, d, O.schedule_tables(SCHEDS[name]), hr, sr, torch.from_numpy(g[k + 't']), z, conditional=CONDITIONAL[name])
    (loss / hr.numel()).backward()
    loss = loss.detach()
    ref = float(g[k + 'loss_sum'])
    assert abs(float(loss) - ref) <= 1e-5 * abs(ref)
    assert abs(float(loss) / hr.numel() - float(g[k + 'l_pix'])) <= 1e-5 * abs(float(g[k + 'l_pix']))
    n = 0
    for key in g:
        if not key.startswith(k + 'grad/'):
            continue
        got = sdr[key[len(k + 'grad/'):]].grad
        want = g[key]
        assert got is not None and tuple(got.shape) == want.shape, key
        assert np.abs(got.numpy() - want).max() <= TOL * max(1.0, np.abs(want).max()), key
        n += 1
    assert n > 20
