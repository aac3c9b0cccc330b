"""The users of the shared step-tail frame (csrc/step_tail.h: prologue, element I/O) against one another on the GPU: with nothing for
their own rule to do, sr3_guided_step (no second forward, mode 1 = the static clamp / mode 0 = none), sr3_tiled_step_hist (one tile that
covers the image) and sr3_p_sample_step_hist + sr3_step_decrement are the same step, so x, the history and the counter come out equal
bit for bit -- on the 16-byte path (8 x 12) and on the scalar one (6 x 10: a width that is no multiple of 4), with and without a history
buffer, clip_denoised on and off, z given and NULL."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

import gpu_util as G                  # noqa: E402
from sr3_hip import lib as L          # noqa: E402

B, CH, ROWS, J = 2, 3, 3, 1           # batch, channels, rows of the tables, the step index


@pytest.mark.parametrize('hw', [(8, 12), (6, 10)], ids=['8x12-vec', '6x10-scalar'])
def test_rule_tails_share_one_frame(hw):
    H, W = hw
    d = G.dev()
    lib = L.load()
    gen = torch.Generator().manual_seed(100 * H + W)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    x_in, eps, z_in, hist_in = (rnd(B, CH, H, W).to(d) for _ in range(4))
    x_in = x_in * 1.5                                                     # (x0 = a x - b eps leaves [-1, 1] often: the clamp has work)
    tabs = [(0.5 + torch.rand(ROWS, generator=gen)).to(d) for _ in range(6)]      # a, b, c1, c2, sigma, c3
    ones_y, ones_x = torch.ones(H, device=d), torch.ones(W, device=d)
    origin = torch.zeros(1, dtype=torch.int32, device=d)
    st = G.stream()

    def fresh(with_hist):
        return x_in.clone(), hist_in.clone() if with_hist else None, torch.tensor([-7, J], dtype=torch.int32, device=d)

    for with_hist, clip, with_z in itertools.product((False, True), repeat=3):
        z = z_in if with_z else None
        c3 = tabs[5] if with_hist else None
        five = [L.ptr(t) for t in tabs[:5]]
        results = {}
        x, hist, step2 = fresh(with_hist)
        L.check(lib.sr3_guided_step(L.ptr(x), L.ptr(eps), None, 1.0, L.ptr(z), B, CH, H, W, *five, L.ptr(c3), L.ptr(hist), L.ptr(step2),
                                    1 if clip else 0, 0, 0.0, None, None, 0, None, st))
        results['guided'] = (x, hist, step2)
        x, hist, step2 = fresh(with_hist)
        L.check(lib.sr3_tiled_step_hist(L.ptr(x), L.ptr(eps), B, CH, H, W, L.ptr(origin), 1, L.ptr(origin), 1, L.ptr(ones_y), L.ptr(ones_x),
                                        H, W, None, None, L.ptr(z), *five, L.ptr(step2), 1 if clip else 0, None, st, L.ptr(c3), L.ptr(hist)))
        results['tiled'] = (x, hist, step2)
        x, hist, step2 = fresh(with_hist)
        L.check(lib.sr3_p_sample_step_hist(L.ptr(x), L.ptr(eps), L.ptr(z), *five, L.ptr(step2[1:]), None, 0, B, CH * H * W, 1 if clip else 0,
                                           L.ptr(c3), L.ptr(hist), st))
        L.check(lib.sr3_step_decrement(L.ptr(step2[1:]), st))
        results['p_sample'] = (x, hist, step2)
        torch.cuda.synchronize()
        case = dict(hw=hw, hist=with_hist, clip=clip, z=with_z)
        gx, gh, gs = results['guided']
        assert bool(torch.isfinite(gx).all()) and not torch.equal(gx, x_in), case
        assert gs.tolist() == [J, J - 1], case                            # (slot 0: the step's copy of j; slot 1: the next step's index)
        assert torch.equal(results['tiled'][2], gs) and results['p_sample'][2][1].item() == J - 1, case
        for name in ('tiled', 'p_sample'):
            ox, oh, _ = results[name]
            assert torch.equal(ox, gx), (name, case)
            if with_hist:
                assert torch.equal(oh, gh) and not torch.equal(oh, hist_in), (name, case)
