"""The generalised loss / gradient kernel alone (sr3_loss_grad_f32, k_loss_grad of train_kernels.hip) against float64 on the same
fp32 inputs:  d = (ta z + tb hr) - e ;  loss = sum w rho(d) ;  g = -w rho'(d) scale  (NHWC, 4 lanes), rho = L1 | L2 | Huber.

Bounds (derived, not tuned).  d is three fp32 products / sums of terms of size S = |ta z| + |tb hr| + |e|: at most 3 roundings of 2^-24 S,
and rho' scales that by c = 2 (L2) or 1; the products with w scale add 2^-24 |g| <= 2^-24 c S w scale each.  4 * 2^-23 S w scale c covers
the sum with room.  For L1 |g| = w scale whatever S is, so the bound speaks of d alone: w has 3 significant bits and scale is a power of
two here, which makes w scale exact in fp32 (otherwise its own rounding, 2^-24 w scale, exceeds the bound wherever S < 1/8).  An L1
element whose float64 |d| is below 4 * 2^-23 S has an undetermined sign in fp32 and is left out; at most 1e-4 of the elements may be.
The loss is accumulated in double from the fp32 d: relative 1e-6."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import gpu_util as G                                             # noqa: E402
from sr3_hip import lib as L                                    # noqa: E402

SHAPES = [(3, 3, 16, 16),        # one trip of the grid-stride loop, a pad lane
          (3, 3, 160, 160),      # 76 800 pixels over 65 536 threads: a second, ragged trip
          (2, 4, 8, 8)]          # no pad lane, fewer pixels than threads
KINDS = {'l1': 0, 'l2': 1, 'huber': 2}
DELTA = 1.0
SCALE = 2.0 ** -10
TA, TB, W = (0.9, 0.5, 0.2), (-0.4, -0.85, 0.97), (0.75, 1.5, 0.375)      # per image; w: 3 significant bits (see above)
EPS32 = 2.0 ** -23

_cases = {}


def case(shape):
    """Inputs (fp32) and the float64 reference of every kind for one shape, computed once."""
    if shape in _cases:
        return _cases[shape]
    B, Cc, H, Wd = shape
    gen = torch.Generator().manual_seed(1000 + H)
    z = torch.randn(shape, generator=gen)
    hr = torch.rand(shape, generator=gen) * 2 - 1
    e = torch.randn(shape, generator=gen) * 0.8
    ta, tb, w = (torch.tensor(v[:B], dtype=torch.float32) for v in (TA, TB, W))
    bc = lambda t: t.double().view(B, 1, 1, 1)
    d = bc(ta) * z.double() + bc(tb) * hr.double() - e.double()
    S = (bc(ta) * z.double()).abs() + (bc(tb) * hr.double()).abs() + e.double().abs()
    tol_d = 4 * EPS32 * S
    ref = {}
    for kind in KINDS:
        if kind == 'l1':
            rho, drho, c = d.abs(), d.sign(), 1.0
        elif kind == 'l2':
            rho, drho, c = d * d, 2 * d, 2.0
        else:
            inside = d.abs() <= DELTA
            share = inside.double().mean().item()
            assert 0.2 < share < 0.8, share          # both branches of the Huber loss occur
            rho, drho, c = torch.where(inside, 0.5 * d * d, DELTA * (d.abs() - 0.5 * DELTA)), d.clamp(-DELTA, DELTA), 1.0
        ref[kind] = dict(loss=(bc(w) * rho).sum().item(), g=-bc(w) * drho * SCALE, tol=tol_d * bc(w).abs() * SCALE * c)
    keep = d.abs() >= tol_d                          # L1: the elements whose sign fp32 can be held to
    assert (~keep).double().mean().item() <= 1e-4, (~keep).sum().item()
    _cases[shape] = dict(z=z, hr=hr, e=e, ta=ta, tb=tb, w=w, ref=ref, keep=keep)
    return _cases[shape]


def run(c, shape, kind, tables=True, delta=DELTA):
    B, Cc, H, Wd = shape
    d = G.dev()
    lib = L.load()
    t = {k: c[k].to(d) for k in ('z', 'hr', 'e', 'ta', 'tb', 'w')}
    g = torch.full((B, H * Wd, 4), float('nan'), device=d)
    loss = torch.full((1,), float('nan'), device=d)
    scratch = torch.empty(int(lib.sr3_loss_grad_scratch_bytes()), dtype=torch.uint8, device=d)
    tz, tx, w = (t['ta'], t['tb'], t['w']) if tables else (None, None, None)
    L.check(lib.sr3_loss_grad_f32(L.ptr(t['z']), L.ptr(t['e']), L.ptr(t['hr']), L.ptr(tz), L.ptr(tx), L.ptr(w), B, Cc, H * Wd, KINDS[kind],
                                  C.c_float(delta), C.c_float(SCALE), L.ptr(g), L.ptr(loss), L.ptr(scratch), G.stream()))
    torch.cuda.synchronize()
    return g.cpu(), float(loss)


@pytest.mark.parametrize('kind', list(KINDS))
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_loss_grad_matches_float64(shape, kind):
    B, Cc, H, Wd = shape
    c = case(shape)
    r = c['ref'][kind]
    g, loss = run(c, shape, kind)
    assert bool(torch.isfinite(g).all()), 'an element of g was not written'
    if Cc < 4:
        assert bool((g[:, :, Cc:] == 0).all()), 'pad lanes must be written 0'
    got = g[:, :, :Cc].reshape(B, H, Wd, Cc).permute(0, 3, 1, 2).double()
    excess = (got - r['g']).abs() - r['tol']
    if kind == 'l1':
        excess = excess[c['keep']]
    print('%s %s: worst |err| - bound = %.3e (bound max %.3e), loss %.9g ref %.9g' % (shape, kind, excess.max().item(), r['tol'].max().item(), loss, r['loss']))
    assert excess.max().item() <= 0.0, 'gradient off its rounding bound by %.3e' % excess.max().item()
    assert abs(loss - r['loss']) <= 1e-6 * abs(r['loss']), (loss, r['loss'])
    g2, loss2 = run(c, shape, kind)
    assert torch.equal(g, g2) and loss == loss2, 'two calls on the same inputs differ'


@pytest.mark.parametrize('kind', list(KINDS))
def test_null_tables_are_target_z_weight_one(kind):
    """tgt_z = tgt_x0 = weight = NULL: target z, weight 1 -- the gradient bits of the tables (1, 0, 1) through the generalised kernel.  L1 /
    L2 with NULL tables run the training step's own kernel, k_l1_loss_grad, which adds the same doubles in another grouping: its loss
    is held to the double sum's 1e-6, Huber's (one kernel either way) to the same bits."""
    shape = SHAPES[0]
    B = shape[0]
    c = dict(case(shape))
    c.update(ta=torch.ones(B), tb=torch.zeros(B), w=torch.ones(B))
    g1, l1 = run(c, shape, kind, tables=True)
    g0, l0 = run(c, shape, kind, tables=False)
    assert torch.equal(g0, g1) and (l0 == l1 if kind == 'huber' else abs(l0 - l1) <= 1e-6 * abs(l1))
    d = c['z'].double() - c['e'].double()
    rho = {'l1': d.abs(), 'l2': d * d, 'huber': torch.where(d.abs() <= DELTA, 0.5 * d * d, DELTA * (d.abs() - 0.5 * DELTA))}[kind]
    assert abs(l0 - rho.sum().item()) <= 1e-6 * rho.sum().item()
