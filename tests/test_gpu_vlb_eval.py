"""The variational bound by timestep on the GPU: sr3_vlb_terms_f32, sr3_q_sample_step_f32 and sr3_prior_bpd_f32 on
caller-owned tensors, sr3_train_step_ex3 against sr3_train_step_ex2 / _ex, calc_bpd_loop against its parts, and three optimizer steps
under the loss-aware timestep sampler.

Tolerances follow the project's rule for new fp32 arithmetic: 4 x the worst error of the same formulas evaluated in
fp32 NumPy (learned_var_ref.vlb_f32 through vlb_eval_ref.terms32) against float64 on the test's own inputs, computed here on the CPU.
A per-image output is a mean of such terms, so its error cannot exceed the worst element's: the bound of image b is 4 x the worst
absolute element error within image b, plus learned_var_ref.nll_conditioning of its last-step rows (what fp32 can know of a log of a
difference of two CDF values; 0 for a KL row) divided by the element count, plus one rounding of the fp32 result (2^-24 |ref|).
Measured on an MI355X against these bounds: see DESIGN.md 3.3i."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import DESCS, CONDITIONAL, opt_for             # noqa: E402
import gpu_util as G                                         # noqa: E402
import learned_var_ref as R                                  # noqa: E402
import vlb_eval_ref as V                                     # noqa: E402
from test_learned_var_cpu import _ac                         # noqa: E402

from sr3_hip import diffusion as D                           # noqa: E402
from sr3_hip import lib as L                                 # noqa: E402

S100 = 100
ROWS = (0, 1, 50, 99)                                        # the last step of the walk (the NLL), the first KL step, the middle, S - 1
SHAPES = [(1, 5, 7), (3, 8, 12), (3, 16, 16), (3, 64, 64)]   # 35 elements: the one-float path; 3 * 64 * 64 / 4 groups: three per thread slice
SCHED20 = dict(schedule='linear', n_timestep=20, linear_start=1e-6, linear_end=1e-2)


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def _tabs():
    tabs = R.walk_tables(_ac(S100), S100)
    return tabs, R.step_scalars(tabs, np.arange(S100))


@functools.lru_cache(maxsize=None)
def _inputs(C_, H, W, rows):
    """x0 reaching +-1 (beyond +-0.999), x_t on the rows' levels, a prediction near the noise, v in [-1.5, 1.5]: made once per case."""
    B = len(rows)
    gen = torch.Generator().manual_seed(7 + C_ * H * W)
    x0 = (torch.randn(B, C_, H, W, generator=gen) * 0.6).clamp(-1.0, 1.0)
    z = torch.randn(B, C_, H, W, generator=gen)
    ab = torch.tensor(_ac(S100)[np.asarray(rows)], dtype=torch.float64).reshape(-1, 1, 1, 1)
    xt = (ab.sqrt() * x0.double() + (1.0 - ab).sqrt() * z.double()).float()
    pred = z + 0.3 * torch.randn(B, C_, H, W, generator=gen)
    v = torch.rand(B, C_, H, W, generator=gen) * 3.0 - 1.5
    assert bool((x0.abs() > 0.999).any()) and float(v.min()) < -1.4 and float(v.max()) > 1.4
    return x0, xt, torch.cat([pred, v], 1).contiguous()


def _bounds(x0, xt, out, scal32, var_mode, clip):
    """(ref vb [B], ref mse [B], tol vb [B], tol mse [B]) in float64 from the fp32 rows the kernel reads."""
    s64 = scal32.double().numpy()
    vlb64, mse64 = V.terms64(x0, xt, out, s64, var_mode, clip)
    vlb32, mse32 = V.terms32(x0.numpy(), xt.numpy(), out.numpy(), scal32.numpy(), var_mode, clip)
    B = x0.shape[0]
    e_v = (torch.from_numpy(vlb32).double() - vlb64).abs().reshape(B, -1).max(1).values
    e_m = (torch.from_numpy(mse32).double() - mse64).abs().reshape(B, -1).max(1).values
    ref_v, ref_m = V.per_image(vlb64), V.per_image(mse64)
    cond = V.nll_cond_per_image(x0, xt, out, s64, var_mode, clip)
    return ref_v, ref_m, 4.0 * e_v + cond + 2.0 ** -24 * ref_v.abs(), 4.0 * e_m + 2.0 ** -24 * ref_m.abs()


def _terms_call(x0, xt, out, table, rows=None, step2=None, var_mode=0, clip=True, scratch=None, S=None, outs=None, C_=None):
    """One call on device tensors -> (rc, vb, mse)."""
    lib, dev = L.load(), G.dev()
    B, Cc = x0.shape[0], (x0.shape[1] if C_ is None else C_)
    P = x0[0].numel() // x0.shape[1]
    S = table.shape[0] if S is None else S
    nb = int(lib.sr3_vlb_terms_partials_bytes(B))
    if scratch is None:
        scratch = torch.empty(nb // 8, dtype=torch.float64, device=dev)
    if outs is None:
        n = B if step2 is None else S * B
        outs = (torch.full((n,), float('nan'), device=dev), torch.full((n,), float('nan'), device=dev))
    rc = lib.sr3_vlb_terms_f32(L.ptr(x0), L.ptr(xt), L.ptr(out), out.shape[1], L.ptr(table), S, L.ptr(rows), L.ptr(step2), var_mode,
                               1 if clip else 0, B, Cc, P, L.ptr(outs[0]), L.ptr(outs[1]), L.ptr(scratch), nb, G.stream())
    torch.cuda.synchronize()
    return rc, outs[0], outs[1]


def _shifted(t):
    """The same values at an address that is 4 bytes off a 16-byte boundary: the one-float path."""
    buf = torch.empty(t.numel() + 4, device=t.device, dtype=t.dtype)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    return view


# ---- 1. sr3_vlb_terms_f32 -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('clip', [True, False])
@pytest.mark.parametrize('var_mode', [0, 1, 2])
@pytest.mark.parametrize('C_,H,W', SHAPES)
def test_vlb_terms_rows_per_image(C_, H, W, var_mode, clip):
    dev = G.dev()
    _, scal = _tabs()
    table = torch.tensor(scal, dtype=torch.float32)
    worst = 0.0
    for rows in ((0, 1, 50), (99, 50, 0)):
        x0, xt, out6 = _inputs(C_, H, W, rows)
        out = out6 if var_mode == 0 else out6[:, :C_].contiguous()
        ref_v, ref_m, tol_v, tol_m = _bounds(x0, xt, out, table[list(rows)], var_mode, clip)
        rd = torch.tensor(rows, dtype=torch.int32, device=dev)
        rc, vb, mse = _terms_call(x0.to(dev), xt.to(dev), out.to(dev), table.to(dev), rows=rd, var_mode=var_mode, clip=clip)
        assert rc == 0, L.load().sr3_last_error()
        ev, em = (vb.cpu().double() - ref_v).abs(), (mse.cpu().double() - ref_m).abs()
        print('C P %d x %d, mode %d, clip %d, rows %s: vb %s err %s (bound %s); mse err %s (bound %s)'
              % (C_, H * W, var_mode, clip, rows, ref_v.tolist(), ev.tolist(), tol_v.tolist(), em.tolist(), tol_m.tolist()))
        assert bool((ev <= tol_v).all()) and bool((em <= tol_m).all())
        worst = max(worst, float((ev / tol_v).max()), float((em / tol_m.clamp(min=1e-300)).max()))
        assert float(ref_v.abs().min()) > 1e-4              # (every term is well above its bound: the check sees something)
    print('worst error / bound: %.3f' % worst)


@pytest.mark.parametrize('clip', [True, False])
@pytest.mark.parametrize('var_mode', [0, 1, 2])
@pytest.mark.parametrize('C_,H,W', SHAPES)
def test_vlb_terms_on_the_step_counter(C_, H, W, var_mode, clip):
    dev = G.dev()
    _, scal = _tabs()
    table = torch.tensor(scal, dtype=torch.float32)
    B = 3
    vb = torch.full((S100 * B,), float('nan'), device=dev)
    mse = torch.full((S100 * B,), float('nan'), device=dev)
    for j in ROWS:
        x0, xt, out6 = _inputs(C_, H, W, (j,) * B)
        out = out6 if var_mode == 0 else out6[:, :C_].contiguous()
        ref_v, ref_m, tol_v, tol_m = _bounds(x0, xt, out, table[[j] * B], var_mode, clip)
        step2 = torch.tensor([-5, j], dtype=torch.int32, device=dev)
        rc, _, _ = _terms_call(x0.to(dev), xt.to(dev), out.to(dev), table.to(dev), step2=step2, var_mode=var_mode, clip=clip, outs=(vb, mse))
        assert rc == 0, L.load().sr3_last_error()
        assert step2.tolist() == [-5, j - 1]                # slot 1: the next step; slot 0 is not this entry's
        got_v, got_m = vb.view(S100, B)[j].cpu().double(), mse.view(S100, B)[j].cpu().double()
        assert bool(((got_v - ref_v).abs() <= tol_v).all()) and bool(((got_m - ref_m).abs() <= tol_m).all()), (j, got_v, ref_v, tol_v)
    written = torch.isfinite(vb.view(S100, B)).all(1).cpu()
    assert written.nonzero().flatten().tolist() == sorted(ROWS)      # row j alone is written


@pytest.mark.parametrize('C_,H,W', SHAPES)
def test_vlb_terms_same_bits_every_run_whatever_the_scratch_held_on_either_path(C_, H, W):
    dev = G.dev()
    _, scal = _tabs()
    table = torch.tensor(scal, dtype=torch.float32).to(dev)
    rows = (0, 50, 99)
    x0, xt, out = (t.to(dev) for t in _inputs(C_, H, W, rows))
    rd = torch.tensor(rows, dtype=torch.int32, device=dev)
    nb = int(L.load().sr3_vlb_terms_partials_bytes(3))
    assert nb == 3 * 16 * 2 * 8
    first = _terms_call(x0, xt, out, table, rows=rd)
    again = _terms_call(x0, xt, out, table, rows=rd)
    assert first[0] == 0 and torch.equal(first[1], again[1]) and torch.equal(first[2], again[2])
    # exactly the queried size, pre-filled with NaN patterns: the same bits
    for pattern in (0x7FF8000000000000, 0xFFFFFFFFFFFFFFFF):
        scr = torch.full((nb // 8,), pattern - (1 << 64) if pattern >= (1 << 63) else pattern, dtype=torch.int64, device=dev).view(torch.float64)
        assert bool(torch.isnan(scr).all())
        got = _terms_call(x0, xt, out, table, rows=rd, scratch=scr)
        assert got[0] == 0 and torch.equal(first[1], got[1]) and torch.equal(first[2], got[2])
    # the one-float path (misaligned pointers) gives the bits of the 16-byte path
    if (C_ * H * W) % 4 == 0:
        got = _terms_call(_shifted(x0), _shifted(xt), _shifted(out), table, rows=rd)
        assert got[0] == 0 and torch.equal(first[1], got[1]) and torch.equal(first[2], got[2])
    # a row the table does not have: that image's terms are NaN, the others are untouched by it
    bad = torch.tensor([0, S100, 99], dtype=torch.int32, device=dev)
    got = _terms_call(x0, xt, out, table, rows=bad)
    assert got[0] == 0 and bool(torch.isnan(got[1][1])) and torch.equal(got[1][[0, 2]], first[1][[0, 2]])


def test_vlb_terms_refusals_launch_nothing():
    lib, dev = L.load(), G.dev()
    _, scal = _tabs()
    table = torch.tensor(scal, dtype=torch.float32).to(dev)
    x0, xt, out = (t.to(dev) for t in _inputs(3, 8, 12, (0, 1, 50)))
    rows = torch.tensor([0, 1, 50], dtype=torch.int32, device=dev)
    step2 = torch.tensor([7, 7], dtype=torch.int32, device=dev)
    nb = int(lib.sr3_vlb_terms_partials_bytes(3))
    scr = torch.zeros(nb // 8 + 1, dtype=torch.float64, device=dev)
    vb, mse = torch.full((S100 * 3,), 3.5, device=dev), torch.full((S100 * 3,), 4.5, device=dev)
    base = dict(x0=L.ptr(x0), xt=L.ptr(xt), out=L.ptr(out), oc=6, table=L.ptr(table), S=S100, rows=L.ptr(rows), step2=None, mode=0, B=3, Cc=3,
                P=96, vb=L.ptr(vb), mse=L.ptr(mse), scr=L.ptr(scr), nb=nb)

    def call(**kw):
        a = dict(base, **kw)
        return lib.sr3_vlb_terms_f32(a['x0'], a['xt'], a['out'], a['oc'], a['table'], a['S'], a['rows'], a['step2'], a['mode'], 1, a['B'],
                                     a['Cc'], a['P'], a['vb'], a['mse'], a['scr'], a['nb'], G.stream())
    off8 = C.c_void_p(scr.data_ptr() + 4)
    big = torch.full((1024,), 7, dtype=torch.int32, device=dev)      # (room for [S, B] floats: the overlap found is the counter's)
    cases = [(dict(x0=None), -1, 'x0 is NULL'), (dict(xt=None), -1, 'x_t is NULL'), (dict(out=None), -1, 'out is NULL'),
             (dict(table=None), -1, 'table is NULL'), (dict(vb=None), -1, 'vb_out is NULL'), (dict(mse=None), -1, 'x0_mse_out is NULL'),
             (dict(scr=None), -1, 'scratch is NULL'),
             (dict(step2=L.ptr(step2)), -1, 'exactly one of rows_per_image and step2_dev selects the rows (both given)'),
             (dict(rows=None), -1, 'exactly one of rows_per_image and step2_dev selects the rows (neither given)'),
             (dict(B=0), -1, 'must be positive'), (dict(P=-1), -1, 'must be positive'), (dict(S=0), -1, 'must be positive'),
             (dict(mode=3), -1, 'var_mode 3 is outside 0..2'), (dict(mode=1), -1, 'out_channels 6 does not go with var_mode 1'),
             (dict(oc=3), -1, 'out_channels 3 does not go with var_mode 0'),
             (dict(B=1 << 20, P=1 << 10), -2, 'image batch too large'),
             (dict(nb=nb - 1), -4, 'scratch too small'),
             (dict(mse=L.ptr(vb)), -1, 'vb_out overlaps x0_mse_out'), (dict(vb=L.ptr(x0)), -1, 'vb_out overlaps x0'),
             (dict(scr=L.ptr(out)), -1, 'scratch overlaps out'),
             (dict(rows=None, step2=L.ptr(big), vb=L.ptr(big)), -1, 'vb_out overlaps step2_dev'),
             (dict(scr=off8), -3, 'scratch is not 8-byte aligned')]
    for kw, code, text in cases:
        rc = call(**kw)
        assert rc == code and text in lib.sr3_last_error().decode(), (kw, rc, lib.sr3_last_error())
    torch.cuda.synchronize()
    assert bool((vb == 3.5).all()) and bool((mse == 4.5).all()) and not scr.any() and step2.tolist() == [7, 7] and bool((big == 7).all())


@pytest.mark.parametrize('row', ['vlb_terms', 'prior_bpd'])
def test_scratch_contract_in_guarded_buffers(row):
    """tests/test_gpu_scratch_contract.py's check on this feature's rows: a guarded scratch of exactly the queried size under three fills,
    guarded inputs and outputs -- the same bits, every band intact, and the float64 comparison."""
    import test_gpu_scratch_contract as GC
    from vlb_scratch_rows import ROWS as CONTRACT
    GC.test_per_op_scratch_contract(next(r for r in CONTRACT if r.id == row))


# ---- 2. sr3_q_sample_step_f32, sr3_prior_bpd_f32 -------------------------------------------------------------------------------------

def test_q_sample_step_is_q_sample_at_the_counters_row():
    lib, dev = L.load(), G.dev()
    B, n = 3, 3 * 16 * 16
    x0, z = _rand(B, n, seed=1).to(dev), _rand(B, n, seed=2).to(dev)
    ab = _ac(S100)
    ca, cb = torch.tensor(np.sqrt(ab), dtype=torch.float32).to(dev), torch.tensor(np.sqrt(1.0 - ab), dtype=torch.float32).to(dev)
    for j in ROWS:
        step = torch.tensor([j], dtype=torch.int32, device=dev)
        want, got = torch.empty_like(x0), torch.full_like(x0, float('nan'))
        caj, cbj = ca[j].repeat(B).contiguous(), cb[j].repeat(B).contiguous()      # (named: alive until the kernel has run)
        L.check(lib.sr3_q_sample(L.ptr(x0), L.ptr(z), L.ptr(caj), L.ptr(cbj), B, n, L.ptr(want), G.stream()))
        L.check(lib.sr3_q_sample_step_f32(L.ptr(x0), L.ptr(z), L.ptr(ca), L.ptr(cb), S100, L.ptr(step), B, n, L.ptr(got), G.stream()))
        torch.cuda.synchronize()
        assert torch.equal(got, want) and step.tolist() == [j]
        # ... and on the one-float path: misaligned pointers, and a size that is no multiple of 4
        sx, sz, so = _shifted(x0), _shifted(z), _shifted(torch.full_like(x0, float('nan')))
        L.check(lib.sr3_q_sample_step_f32(L.ptr(sx), L.ptr(sz), L.ptr(ca), L.ptr(cb), S100, L.ptr(step), B, n, L.ptr(so), G.stream()))
        odd = torch.full((B * 35,), float('nan'), device=dev)
        L.check(lib.sr3_q_sample_step_f32(L.ptr(x0), L.ptr(z), L.ptr(ca), L.ptr(cb), S100, L.ptr(step), B, 35, L.ptr(odd), G.stream()))
        torch.cuda.synchronize()
        assert torch.equal(so, want) and torch.equal(odd, want.flatten()[:B * 35])
    # a counter outside the table writes nothing; the refusals launch nothing
    got = torch.full_like(x0, 2.5)
    for j in (-1, S100):
        step = torch.tensor([j], dtype=torch.int32, device=dev)
        L.check(lib.sr3_q_sample_step_f32(L.ptr(x0), L.ptr(z), L.ptr(ca), L.ptr(cb), S100, L.ptr(step), B, n, L.ptr(got), G.stream()))
    args = lambda **kw: [kw.get('x0', L.ptr(x0)), L.ptr(z), kw.get('ca', L.ptr(ca)), L.ptr(cb), kw.get('S', S100), kw.get('step', L.ptr(step)),
                         kw.get('B', B), n, kw.get('out', L.ptr(got)), G.stream()]
    for kw, code, text in ((dict(x0=None), -1, 'x0 is NULL'), (dict(ca=None), -1, 'tab_ca is NULL'), (dict(step=None), -1, 'step_dev is NULL'),
                           (dict(out=None), -1, 'out is NULL'), (dict(S=0), -1, 'must be positive'), (dict(B=0), -1, 'must be positive'),
                           (dict(B=1 << 22), -2, 'image batch too large'), (dict(out=L.ptr(x0)), -1, 'out overlaps x0')):
        assert lib.sr3_q_sample_step_f32(*args(**kw)) == code and text in lib.sr3_last_error().decode(), kw
    torch.cuda.synchronize()
    assert bool((got == 2.5).all())


@pytest.mark.parametrize('n', [35, 3 * 16 * 16, 3 * 64 * 64])
def test_prior_bpd_against_float64(n):
    lib, dev = L.load(), G.dev()
    B = 3
    x0 = (_rand(B, n, seed=n) * 0.6).clamp(-1.0, 1.0)
    nb = int(lib.sr3_vlb_terms_partials_bytes(B))
    for abar in (float(_ac(S100)[-1]), 0.5, 1e-4):                          # the 100-step schedule's own last step, and two others
        sa, var, lv = V.prior_scalars(abar)
        p64, p32 = V.prior64(x0, abar), V.prior32(x0.numpy(), abar)
        ref = V.per_image(p64)
        tol = 4.0 * (torch.from_numpy(p32).double() - p64).abs().reshape(B, -1).max(1).values + 2.0 ** -24 * ref.abs()
        xd = x0.to(dev)
        outs = []
        for src in (xd, _shifted(xd)) if n % 4 == 0 else (xd,):
            out = torch.full((B,), float('nan'), device=dev)
            scr = torch.full((nb // 8,), float('nan'), dtype=torch.float64, device=dev)
            L.check(lib.sr3_prior_bpd_f32(L.ptr(src), B, n, C.c_float(sa), C.c_float(var), C.c_float(lv), L.ptr(out), L.ptr(scr), nb, G.stream()))
            torch.cuda.synchronize()
            outs.append(out)
        err = (outs[0].cpu().double() - ref).abs()
        print('n %d abar %.4g: prior %s err %s (bound %s)' % (n, abar, ref.tolist(), err.tolist(), tol.tolist()))
        assert bool((err <= tol).all()) and all(torch.equal(o, outs[0]) for o in outs)
    t = torch.full((B,), 1.5, device=dev)
    scr = torch.zeros(nb // 8, dtype=torch.float64, device=dev)
    args = lambda **kw: [kw.get('x0', L.ptr(xd)), kw.get('B', B), n, C.c_float(kw.get('sa', 0.5)), C.c_float(0.75), C.c_float(-0.3),
                         kw.get('out', L.ptr(t)), kw.get('scr', L.ptr(scr)), kw.get('nb', nb), G.stream()]
    for kw, code, text in ((dict(x0=None), -1, 'x0 is NULL'), (dict(out=None), -1, 'out is NULL'), (dict(scr=None), -1, 'scratch is NULL'),
                           (dict(B=0), -1, 'must be positive'), (dict(sa=float('nan')), -1, 'must be finite'), (dict(nb=nb - 8), -4, 'scratch too small'),
                           (dict(out=L.ptr(scr)), -1, 'out overlaps scratch')):
        assert lib.sr3_prior_bpd_f32(*args(**kw)) == code and text in lib.sr3_last_error().decode(), kw
    torch.cuda.synchronize()
    assert bool((t == 1.5).all()) and not scr.any()


# ---- 3. the models ---------------------------------------------------------------------------------------------------------------------

def build(name, rows=6, phase='val', sched=None, prediction=None, t_sampler=None, lam=0.05, seed=1234):
    """The tiny net `name` with seeded weights; rows = 6: widened to a variance head (learned_var_ref.widen_rows), sharing its
    prediction rows with the 3-row net of the same seed.  -> (model, its state dict on the CPU)."""
    import model as Model
    opt = opt_for(name, phase=phase, gpu=True)
    if sched is not None:
        opt['model']['beta_schedule'] = {'train': dict(sched), 'val': dict(sched)}
    if prediction is not None:
        opt['model']['diffusion']['prediction'] = prediction
    torch.manual_seed(seed)
    m3 = Model.create_model(opt)
    gen = torch.Generator().manual_seed(seed + 1)
    sd = {k: v.cpu() for k, v in m3.netG.state_dict().items()}
    for k, v in sd.items():          # (the train phase's init zeroes every bias: seeded values)
        if k.startswith('denoise_fn.') and v.dim() == 1 and '.block.0.' not in k and '.norm.' not in k and v.is_floating_point() and 'inv_freq' not in k:
            sd[k] = torch.randn(v.shape, generator=gen) * 0.1
    if rows == 6:
        sd = R.widen_rows(sd)
        opt['model']['unet']['out_channel'] = 6
        opt['model']['diffusion']['learned_variance'] = {'lambda': lam}
    if t_sampler is not None:
        opt['model']['diffusion']['t_sampler'] = t_sampler
    m = Model.create_model(opt) if (rows == 6 or t_sampler is not None) else m3
    m.netG.load_state_dict(sd, strict=True)
    m.netG.show_progress = False
    return m, sd


def _images(B, H, W):
    hr = (_rand(B, 3, H, W, seed=31) * 0.5).clamp(-1, 1)
    sr = (_rand(B, 3, H, W, seed=32) * 0.5).clamp(-1, 1)
    return hr, sr, _rand(B, 3, H, W, seed=33)


def _step_args(netG, name, t):
    """What p_losses hands the engine for the injected steps t (0-based, one per image)."""
    dev = G.dev()
    t = np.asarray(t)
    if netG._hyb_table is None:
        tabs = D.ancestral_tables(netG._alphas_cumprod64, netG.num_timesteps, prediction=netG.prediction)
        netG._hyb_table = torch.tensor(D.hybrid_step_scalars(tabs, np.arange(netG.num_timesteps)), dtype=torch.float32).to(dev)
    td = torch.as_tensor(t, dtype=torch.long, device=dev)
    scal = netG._hyb_table[td].contiguous()
    if DESCS[name]['variant'] == 'sr3':
        g = torch.FloatTensor(netG.sqrt_alphas_cumprod_prev[t + 1]).to(dev)
        return g, (1 - g ** 2).sqrt(), g, None, scal
    return netG.sqrt_alphas_cumprod[td].contiguous(), netG.sqrt_one_minus_alphas_cumprod[td].contiguous(), None, td, scal


class _NullPerImage:
    """The library with sr3_train_step_ex3's per_image_out replaced by NULL."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, k):
        return getattr(self._lib, k)

    def sr3_train_step_ex3(self, *a):
        a = list(a)
        a[-5] = None        # (..., per_image_out, scratch, scratch_bytes, vlb_weight, stream)
        return self._lib.sr3_train_step_ex3(*a)


def _oracle_terms(name, sd, rows, hr, sr, z, ca, cb, time, scal32, var_mode):
    """(the float64 per-image terms on the float64 oracle's output at the step's x_noisy, their fp32-formula bounds, and -- the oracle's
    output is not the device's -- what the engine's forward tolerance, 2e-5 max(1, |out|) (test_gpu_unet.py), can move a term by: sum |d
    vb_b / d out| x that).  The derivatives are autograd's: to v directly; to the prediction through x0, because the restatement
    detaches mu_theta -- both branches read x0 - x0^ (the KL as c1 (x0 - x0^), the NLL as x0 - mu_theta = ... - c1 x0^), so d / d x0^ is
    -d / d x0 (times c1 on a last-step row), and d x0^ / d out = -b."""
    from oracle import sr3_oracle as O
    xt = ca.double().view(-1, 1, 1, 1).cpu() * hr.double() + cb.double().view(-1, 1, 1, 1).cpu() * z.double()
    inp = torch.cat([sr.double(), xt], 1) if CONDITIONAL[name] else xt
    sdd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    with torch.no_grad():
        out = O.unet_forward(sdd, dict(DESCS[name], out_channel=rows), inp, time)
    out = out.clone().requires_grad_(True)
    x0 = hr.double().clone().requires_grad_(True)
    s64 = scal32.double()
    vlb, _ = V.terms64(x0, xt, out, s64.numpy(), var_mode, False)
    per = V.per_image(vlb)
    chain = (s64[:, 1].abs() * torch.where(s64[:, 6] != 0, s64[:, 2].abs(), torch.ones_like(s64[:, 2]))).view(-1, 1, 1, 1)
    sens = []
    for b in range(hr.shape[0]):
        g_out, g_x0 = torch.autograd.grad(per[b], [out, x0], retain_graph=True, allow_unused=True)
        sens.append((g_x0.abs() * chain).sum() + (0.0 if g_out is None else g_out.abs().sum()))
    fwd = 2e-5 * max(1.0, float(out.detach().abs().max()))
    _, _, tol_v, _ = _bounds(hr, xt.float(), out.detach().float(), scal32, var_mode, False)
    return per.detach(), tol_v, torch.stack(sens).detach() * fwd


@pytest.mark.parametrize('name,H,W,t', [('sr3_tiny', 16, 16, (3, 3, 3, 3)), ('sr3_tiny', 16, 32, (0, 0, 0, 0)), ('ddpm_tiny', 16, 16, (0, 4, 2, 5)),
                                        ('ddpm_tiny', 16, 32, (3, 0, 1, 1))])
def test_train_step_ex3_is_ex2_plus_the_terms(name, H, W, t):
    dev = G.dev()
    B, lam = 4, 0.05
    hr, sr, z = _images(B, H, W)
    hd, zd = hr.to(dev), z.to(dev)
    cd = sr.to(dev) if CONDITIONAL[name] else None
    n = 3 * H * W
    for rows in (6, 3):
        m, sd = build(name, rows=rows, phase='train', lam=lam)
        netG, un = m.netG, m.netG.denoise_fn
        ca, cb, level, tstep, scal = _step_args(netG, name, t)
        kw = dict(grad_scale=1.0 / hr.numel(), drop_seed=0)
        if rows == 6:
            kw['hybrid'] = (scal, lam)
        old = un.train_step(hd, cd, zd, ca, cb, level, tstep, **kw)          # sr3_train_step_ex2 / _ex
        torch.cuda.synchronize()
        old = (float(old), None if rows == 3 else float(un.last_vlb), un.grad_arena.clone())
        assert un.last_per_image is None
        new = un.train_step(hd, cd, zd, ca, cb, level, tstep, per_image=scal, **kw)
        torch.cuda.synchronize()
        per = un.last_per_image.clone()
        assert float(new) == old[0] and torch.equal(un.grad_arena, old[2]) and bool(torch.isfinite(per).all())
        if rows == 6:
            assert float(un.last_vlb) == old[1]
        # per_image_out NULL: the old launches, and nothing is written to the buffer
        real = un.plan.lib
        un.plan.lib = _NullPerImage(real)
        buf = torch.full((B, 2), 7.25, device=dev)
        try:
            un.grad_arena.fill_(float('nan'))
            null = un.train_step(hd, cd, zd, ca, cb, level, tstep, per_image=(scal, buf), **kw)
            torch.cuda.synchronize()
        finally:
            un.plan.lib = real
        assert float(null) == old[0] and torch.equal(un.grad_arena, old[2]) and bool((buf == 7.25).all())
        un.train_step(hd, cd, zd, ca, cb, level, tstep, per_image=(scal, buf), **kw)       # ... and given, the caller's buffer receives the terms
        torch.cuda.synchronize()
        assert torch.equal(buf, per) and un.last_per_image is buf
        # the same bits on a second run
        again = un.train_step(hd, cd, zd, ca, cb, level, tstep, per_image=scal, **kw)
        torch.cuda.synchronize()
        assert float(again) == old[0] and torch.equal(un.last_per_image, per)
        time = level.double().view(-1, 1).cpu() if level is not None else tstep.cpu()
        ref_v, tol_v, tol_fwd = _oracle_terms(name, sd, rows, hr, sr, z, ca, cb, time, scal.cpu(), 0 if rows == 6 else 1)
        got = per[:, 0].cpu().double()
        print('%s %dx%d rows %d t %s: vb %s, float64 on the oracle\'s output %s (formula bound %s, forward bound %s)'
              % (name, H, W, rows, t, got.tolist(), ref_v.tolist(), tol_v.tolist(), tol_fwd.tolist()))
        assert bool(((got - ref_v).abs() <= tol_v + tol_fwd).all()), (got, ref_v, tol_v, tol_fwd)
        if rows == 6:
            # n sum_b vb_b is the loss kernel's vlb sum: two kernels add the same fp32 terms of the same device tensors, so the forward
            # plays no part and the bound is the formula's (measured on the oracle's output, which is the device's to 2e-5)
            total, bound = n * float(got.sum()), n * float(tol_v.sum())
            print('n sum vb %.9g, vlb_sum_out %.9g, bound %.3g' % (total, old[1], bound))
            assert abs(total - old[1]) <= bound, (total, old[1], bound)
            _check_vlb_weight(un, (hd, cd, zd, ca, cb, level, tstep), kw, scal, lam, old, got, tol_v, n)


def _check_vlb_weight(un, args, kw, scal, lam, old, vb, tol_v, n):
    """sr3_train_step_ex3's vlb_weight: lambda w_b stands where lambda does.  old = (loss, vlb sum, gradient arena) of the unweighted step;
    vb, tol_v: its per-image terms and their formula bounds."""
    dev = G.dev()
    B = scal.shape[0]
    KW, KB = 'final_conv.block.3.weight', 'final_conv.block.3.bias'

    def run(w):
        loss = un.train_step(*args, per_image=scal, vlb_weight=None if w is None else torch.tensor(w, dtype=torch.float32, device=dev), **kw)
        torch.cuda.synchronize()
        g = dict(un.named_gradients())
        return float(loss), float(un.last_vlb), g[KW].clone(), g[KB].clone(), un.grad_arena.clone(), un.last_per_image.clone()
    one = run([1.0] * B)
    assert one[0] == old[0] and one[1] == old[1] and torch.equal(one[4], old[2])          # weight 1 is no weight, bit for bit
    # a power of two scales the variance rows' gradient exactly and leaves the prediction rows, the plain vlb sum and the terms alone
    two = run([2.0] * B)
    assert torch.equal(two[2][3:], 2.0 * one[2][3:]) and torch.equal(two[3][3:], 2.0 * one[3][3:]) and float(one[2][3:].abs().max()) > 0.0
    assert torch.equal(two[2][:3], one[2][:3]) and torch.equal(two[3][:3], one[3][:3]) and two[1] == one[1] and torch.equal(two[5], one[5])
    zero = run([0.0] * B)
    assert not zero[2][3:].any() and not zero[3][3:].any() and torch.equal(zero[2][:3], one[2][:3])
    # per image: loss(w) - loss(1) = lambda sum_b (w_b - 1) n vb_b, each vb_b known to its formula bound; both losses are fp32 (2^-24 each)
    w = [0.5, 4.0, 1.0, 0.0][:B]
    per = run(w)
    dw = torch.tensor(w, dtype=torch.float64) - 1.0
    want = lam * n * float((dw * vb).sum())
    bound = lam * n * float((dw.abs() * tol_v).sum()) + 2.0 ** -24 * (abs(per[0]) + abs(one[0]))
    print('vlb_weight %s: loss %.9g - %.9g = %.6g, lambda sum (w - 1) n vb = %.6g (bound %.3g)' % (w, per[0], one[0], per[0] - one[0], want, bound))
    assert abs((per[0] - one[0]) - want) <= bound and abs(want) > 4 * bound
    assert not torch.equal(per[2][3:], one[2][3:])          # (the variance rows' gradient reads the same per-image lambda)


def test_train_step_ex3_refusals():
    dev = G.dev()
    m, _ = build('sr3_tiny', rows=6, phase='train')
    netG, un = m.netG, m.netG.denoise_fn
    hr, sr, z = (t.to(dev) for t in _images(2, 16, 16))
    ca, cb, level, tstep, scal = _step_args(netG, 'sr3_tiny', (1, 1))
    real = un.plan.lib

    class Bad(_NullPerImage):
        def __init__(self, lib, **kw):
            super().__init__(lib)
            self.kw = kw

        def sr3_train_step_ex3(self, *a):
            a = list(a)
            if 'scratch' in self.kw:
                a[-4] = self.kw['scratch']
            if 'bytes' in self.kw:
                a[-3] = self.kw['bytes']
            if 'scal' in self.kw:
                a[-8] = self.kw['scal']
            return self._lib.sr3_train_step_ex3(*a)
    try:
        for kw, text in ((dict(scratch=None), 'scratch is NULL with per_image_out given'), (dict(bytes=8), 'scratch too small'),
                         (dict(scal=None), 'step_scalars is NULL')):
            un.plan.lib = Bad(real, **kw)
            with pytest.raises(L.Sr3Error, match=text):
                un.train_step(hr, sr, z, ca, cb, level, tstep, grad_scale=1.0, drop_seed=0, hybrid=(scal, 0.1), per_image=scal)
    finally:
        un.plan.lib = real


# ---- 4. calc_bpd_loop ------------------------------------------------------------------------------------------------------------------

def _eager_parts(netG, name, x0, cond, zs, S, clip=True):
    """vb / mse [B, S] in float64 from the loop's parts run one by one: sr3_q_sample, sr3_unet_forward_full, then the float64
    restatement on the device's own x_t and output -- with the bounds of these very inputs."""
    dev = G.dev()
    lib, un = L.load(), netG.denoise_fn
    B = x0.shape[0]
    tabs = D.ancestral_tables(netG._alphas_cumprod64, S, prediction=netG.prediction)
    scal = torch.tensor(D.hybrid_step_scalars(tabs, np.arange(S)), dtype=torch.float32)
    ab = np.asarray(tabs['level'])[1:] ** 2
    ca, cb = torch.tensor(tabs['level'][1:], dtype=torch.float32).to(dev), torch.tensor(np.sqrt(1.0 - ab), dtype=torch.float32).to(dev)
    var_mode = 0 if netG.learned_variance is not None else 1
    ref = {k: torch.zeros(B, S, dtype=torch.float64) for k in ('vb', 'mse', 'tol_vb', 'tol_mse')}
    for j in range(S):
        xt = torch.empty_like(x0)
        caj, cbj = ca[j].repeat(B).contiguous(), cb[j].repeat(B).contiguous()      # (named: alive until the kernel has run)
        L.check(lib.sr3_q_sample(L.ptr(x0), L.ptr(zs[j]), L.ptr(caj), L.ptr(cbj), B, x0[0].numel(), L.ptr(xt), G.stream()))
        if DESCS[name]['variant'] == 'sr3':
            time = torch.tensor(tabs['level'], dtype=torch.float32)[j + 1].repeat(B).to(dev)
        else:
            time = torch.full((B,), int(tabs['tau'][j]), dtype=torch.long, device=dev)
        out = un(xt, time, cond=cond, full=True)
        torch.cuda.synchronize()
        ref['vb'][:, j], ref['mse'][:, j], ref['tol_vb'][:, j], ref['tol_mse'][:, j] = _bounds(x0.cpu(), xt.cpu(), out.cpu(), scal[[j] * B], var_mode, clip)
    return ref


@pytest.mark.parametrize('name,rows,prediction', [('sr3_tiny', 6, None), ('sr3_tiny', 3, None), ('ddpm_tiny', 6, None), ('ddpm_tiny', 3, 'v'),
                                                  ('sr3_tiny', 6, 'v')])
@pytest.mark.parametrize('S', [10, 20])
def test_calc_bpd_loop(name, rows, prediction, S):
    dev = G.dev()
    m, _ = build(name, rows=rows, sched=SCHED20, prediction=prediction)
    netG = m.netG
    assert netG.num_timesteps == 20
    B = 2
    hr, sr, _ = _images(B, 16, 16)
    x_in = {'HR': hr.to(dev), 'SR': sr.to(dev)} if CONDITIONAL[name] else hr.to(dev)
    cond = sr.to(dev) if CONDITIONAL[name] else None
    zs = _rand(S, B, 3, 16, 16, seed=5).to(dev)
    # eager, noise injected: every step equals its parts
    got = netG.calc_bpd_loop(x_in, steps=S, noise_seq=zs)
    torch.cuda.synchronize()
    assert {k: tuple(v.shape) for k, v in got.items()} == dict(vb=(B, S), x0_mse=(B, S), prior_bpd=(B,), total_bpd=(B,))
    ref = _eager_parts(netG, name, hr.to(dev), cond, zs, S)
    ev, em = (got['vb'].cpu().double() - ref['vb']).abs(), (got['x0_mse'].cpu().double() - ref['mse']).abs()
    print('%s rows %d %s S %d: total bpd %s, prior %s, worst vb err / bound %.3f, mse %.3f'
          % (name, rows, prediction, S, got['total_bpd'].tolist(), got['prior_bpd'].tolist(), float((ev / ref['tol_vb']).max()), float((em / ref['tol_mse']).max())))
    assert bool((ev <= ref['tol_vb']).all()) and bool((em <= ref['tol_mse']).all())
    assert bool(torch.isfinite(got['total_bpd']).all()) and bool((got['vb'] > 0).all())
    # the prior and the total
    tabs = D.ancestral_tables(netG._alphas_cumprod64, S, prediction=netG.prediction)
    abar = float(tabs['level'][-1] ** 2)
    p64 = V.prior64(hr, abar)
    tol = 4.0 * (torch.from_numpy(V.prior32(hr.numpy(), abar)).double() - p64).abs().reshape(B, -1).max(1).values + 2.0 ** -24 * V.per_image(p64).abs()
    assert bool(((got['prior_bpd'].cpu().double() - V.per_image(p64)).abs() <= tol).all())
    want_total = (got['vb'].cpu().double().sum(1) + got['prior_bpd'].cpu().double()).float()
    assert torch.equal(got['total_bpd'].cpu(), want_total)
    key = [k for k in netG._loop_cache if k[0] == 'bpd']
    assert len(key) == 1 and netG._loop_cache[key[0]]['graph'] is None and netG._loop_cache[key[0]]['step'].tolist() == [S - 1, -1]
    # captured equals eager, bit for bit, on the same seed; a repeated call replays the same graph and gives the same bits
    outs = []
    for use_graph in (False, True, True):
        netG.use_graph = use_graph
        torch.manual_seed(17)
        outs.append({k: v.clone() for k, v in netG.calc_bpd_loop(x_in, steps=S).items()})
        if use_graph:
            st = netG._loop_cache[key[0]]
            outs[-1]['graph'] = st['graph']
    assert outs[1]['graph'] is not None and outs[2]['graph'] is outs[1]['graph'] and st['replays'] == 2 * S
    for k in ('vb', 'x0_mse', 'prior_bpd', 'total_bpd'):
        assert torch.equal(outs[0][k], outs[1][k]) and torch.equal(outs[1][k], outs[2][k]), k
    assert [k for k in netG._loop_cache if k[0] == 'bpd'] == key
    assert not torch.equal(outs[0]['vb'], got['vb'])        # (another noise than the injected one)


def test_calc_bpd_loop_item_seeds_and_cond_augment():
    dev = G.dev()
    m, _ = build('sr3_tiny', rows=6, sched=SCHED20)
    netG = m.netG
    hr, sr, _ = _images(2, 16, 16)
    x2 = {'HR': hr.to(dev), 'SR': sr.to(dev)}
    x1 = {'HR': hr[1:].to(dev), 'SR': sr[1:].to(dev)}
    seen = {}
    real = netG._bpd_step

    def spy(st, draw_noise=True):
        real(st, draw_noise)
        seen.setdefault(st['x0'].shape[0], []).append(st['xt'].clone())
    netG._bpd_step = spy
    netG.use_graph = False
    both = netG.calc_bpd_loop(x2, steps=10, item_seeds=[101, 202])
    alone = netG.calc_bpd_loop(x1, steps=10, item_seeds=[202])
    netG._bpd_step = real
    # the image's x_t of every step, and with it its terms, are the same bits whatever batch it rode in (the tiny net's forward runs the
    # same kernels at batch 1 and 2)
    assert len(seen[2]) == len(seen[1]) == 10 and all(torch.equal(a[1:], b) for a, b in zip(seen[2], seen[1]))
    assert torch.equal(both['vb'][1:], alone['vb']) and torch.equal(both['x0_mse'][1:], alone['x0_mse'])
    assert not torch.equal(both['vb'][0], both['vb'][1])
    netG.use_graph = True
    a = netG.calc_bpd_loop(x2, steps=10, item_seeds=[101, 202])
    assert torch.equal(a['vb'], both['vb'])                # (the captured loop registers the per-image generators)
    with pytest.raises(L.Sr3Error, match='exclude each other'):
        netG.calc_bpd_loop(x2, steps=10, item_seeds=[1, 2], noise_seq=torch.zeros(10, 2, 3, 16, 16, device=dev))
    with pytest.raises(ValueError, match='steps must lie in'):
        netG.calc_bpd_loop(x2, steps=21)
    # noise conditioning augmentation: the conditioning image is diffused once, at sample_level, and the loop runs
    netG.set_cond_augment(0.5, 0.25, False)
    torch.manual_seed(3)
    aug = netG.calc_bpd_loop(x2, steps=10)
    torch.manual_seed(3)
    aug2 = netG.calc_bpd_loop(x2, steps=10)
    assert bool(torch.isfinite(aug['total_bpd']).all()) and torch.equal(aug['vb'], aug2['vb']) and not torch.equal(aug['vb'], a['vb'])


def test_drop_in_calc_bpd_uses_the_fed_batch():
    m, _ = build('ddpm_tiny', rows=3, sched=SCHED20)
    hr, sr, _ = _images(2, 16, 16)
    m.feed_data({'HR': hr, 'SR': sr})
    torch.manual_seed(9)
    a = m.calc_bpd(steps=10)
    torch.manual_seed(9)
    b = m.netG.calc_bpd_loop(hr.to(G.dev()), steps=10)
    assert torch.equal(a['total_bpd'], b['total_bpd']) and tuple(a['vb'].shape) == (2, 10) and m.netG.training


# ---- 5. training under the timestep sampler -----------------------------------------------------------------------------------------

def _three_steps(name, rows):
    m, _ = build(name, rows=rows, phase='train', t_sampler={'type': 'loss_second_moment', 'history': 2, 'uniform': 0.01})
    netG = m.netG
    fed = []
    real = netG.t_sampler.update
    netG.t_sampler.update = lambda t, losses: (fed.append((np.array(t), np.array(losses))), real(t, losses))[1]
    hr, sr, _ = _images(4, 16, 16)
    np.random.seed(3)
    torch.manual_seed(3)
    torch.cuda.manual_seed(3)
    logs, per = [], []
    for _ in range(3):
        m.feed_data({'HR': hr, 'SR': sr})
        m.optimize_parameters()
        per.append(netG.denoise_fn.last_per_image.cpu().numpy().copy())
        logs.append(dict(m.get_current_log()))
    return m, fed, logs, per


@pytest.mark.parametrize('name,rows', [('ddpm_tiny', 3), ('ddpm_tiny', 6), ('sr3_tiny', 6)])
def test_three_optimizer_steps_under_the_t_sampler(name, rows):
    m, fed, logs, per = _three_steps(name, rows)
    ts = m.netG.t_sampler
    assert len(fed) == 3 and int(ts.counts.sum()) == 12
    for (t, losses), p in zip(fed, per):
        assert losses.shape == (4,) and np.array_equal(losses, p[:, 0].astype(np.float64)) and np.all(np.isfinite(losses)) and np.all(losses > 0)
        assert np.all((0 <= t) & (t < ts.T))
        if name == 'sr3_tiny':
            assert len(set(t.tolist())) == 1               # one step per batch
    ref = V.Resampler(ts.T, ts.history, ts.uniform)         # the history holds the device's values: the last `history` of every step
    for t, losses in fed:
        ref.update(t, losses)
    for k in range(ts.T):
        kept = sorted(ts.losses[k].tolist())[ts.history - len(ref.seen[k]):] if ref.seen[k] else []
        assert int(ts.counts[k]) == sum(int((t == k).sum()) for t, _ in fed) and sorted(ref.seen[k]) == kept, k
    assert all(np.isfinite(v) for log in logs for v in log.values()) and all('l_pix' in log for log in logs)
    m2, fed2, logs2, per2 = _three_steps(name, rows)
    assert logs2 == logs and all(np.array_equal(a, b) for a, b in zip(per, per2))
    assert np.array_equal(m2.netG.t_sampler.losses, ts.losses) and np.array_equal(m2.netG.t_sampler.counts, ts.counts)
    assert torch.equal(m2.netG.denoise_fn.arena.data, m.netG.denoise_fn.arena.data)


def test_image_nll_tool_on_a_made_up_validation_set(tmp_path):
    """tools/image_nll.py end to end: five images, the tiny SR3 config, a four-step walk over three of them in batches of two -- one JSON
    line whose parts add up; and the same three images one by one give the same means (the per-item noise streams)."""
    import json
    import os
    import subprocess
    import sys
    from helpers import ROOT
    from test_oracle_io import _write_triplets
    _write_triplets(str(tmp_path / 'ds'), 5, l=4, r=16)
    opt = opt_for('sr3_tiny', phase='val', gpu=True)
    opt['datasets'] = {'val': dict(name='t', mode='LRHR', dataroot=str(tmp_path / 'ds'), datatype='img', l_resolution=4, r_resolution=16, data_len=-1)}
    cfg = tmp_path / 'cfg.json'
    cfg.write_text('// tiny\n' + json.dumps(opt, indent=1))
    recs = []
    for batch in ('2', '1'):
        out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'image_nll.py'), '-c', str(cfg), '--steps', '4', '--max-images', '3',
                              '--seed', '5', '--batch', batch], check=True, stdout=subprocess.PIPE, timeout=120).stdout.decode()
        recs.append(json.loads(out.strip().splitlines()[-1]))
    rec = recs[0]
    assert rec['metric'] == 'bpd' and rec['images'] == 3 and rec['steps'] == 4 and len(rec['vb']) == len(rec['x0_mse']) == 4
    assert all(np.isfinite(v) and v > 0 for v in rec['vb']) and abs(sum(rec['vb']) + rec['prior_bpd'] - rec['value']) <= 1e-5 * rec['value']
    assert recs[1]['vb'] == rec['vb'] and recs[1]['prior_bpd'] == rec['prior_bpd']
