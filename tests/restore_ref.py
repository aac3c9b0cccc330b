"""The NumPy float32 restatement of csrc/restore.hip (a plain helper module): both operators of sr3_restore_step inside the step's tail,
the jump of sr3_travel_back_f32 and sr3_gray_f32.  Every product, sum and difference is one np.float32 operation, in the kernel's order,
so the results are the kernel's bit for bit (the kernel rounds each on its own: no fma).

Also here: the bound on the gray residual |a . x0' - y| at strength 1 that tests/test_restore_cpu.py checks the restatement against and
tests/test_gpu_restore.py the kernel and the chains."""
import numpy as np

F = np.float32
KEYS = ('a', 'b', 'c1', 'c2', 'sigma')
EPS = 2.0 ** -24          # the unit roundoff of fp32: |fl(v) - v| <= EPS |v|


def gray(x, a):
    """g = ((a0 x_0 + a1 x_1) + a2 x_2) + ... over the channel axis of x [B, C, H, W] -> [B, 1, H, W]"""
    x = np.asarray(x, dtype=F)
    a = np.asarray(a, dtype=F)
    g = a[0] * x[:, 0]
    for c in range(1, x.shape[1]):
        g = g + a[c] * x[:, c]
    assert g.dtype == F
    return g[:, None]


def pinv(a):
    """p = a / sum a^2 in float64, rounded once"""
    a64 = np.asarray(a, dtype=F).astype(np.float64)
    return (a64 / (a64 ** 2).sum()).astype(F)


def project_mask(x0, y, m, lam):
    """w = lam m ; x0' = (w y) + ((1 - w) x0); m [B, 1 or C, H, W] broadcasts over the channels"""
    x0, y, m = (np.asarray(t, dtype=F) for t in (x0, y, m))
    w = F(lam) * m
    out = w * y + (F(1.0) - w) * x0
    assert out.dtype == F
    return out


def project_gray(x0, y, a, p, lam):
    """r = y - a . x0 ; x0'_c = x0_c + ((lam p[c]) r)"""
    x0 = np.asarray(x0, dtype=F)
    r = np.asarray(y, dtype=F) - gray(x0, a)
    lp = F(lam) * np.asarray(p, dtype=F)
    out = x0 + lp[None, :, None, None] * r
    assert out.dtype == F
    return out


def restore_step(x, eps, z, op, target, mask, a, p, lam, tabs, j, clip, hist=None):
    """One restoring step in the kernel's operations and association.  tabs: dict of fp32 arrays a, b, c1, c2, sigma (and c3 when hist
    is given), read at row j.  op 0: target = known, mask; op 1: target = the gray image, weights a, p.  -> (x', hist') with hist' = x0'
    (None without history)"""
    x, eps = np.asarray(x, dtype=F), np.asarray(eps, dtype=F)
    ta, tb, c1, c2, sg = (F(tabs[k][j]) for k in KEYS)
    x0 = ta * x - tb * eps
    if clip:
        x0 = np.clip(x0, F(-1.0), F(1.0))
    x0p = project_mask(x0, target, mask, lam) if op == 0 else project_gray(x0, target, a, p, lam)
    mean = c1 * x0p + c2 * x
    if hist is not None:
        mean = mean + F(tabs['c3'][j]) * np.asarray(hist, dtype=F)
    zz = np.zeros_like(x) if z is None else np.asarray(z, dtype=F)
    out = mean + zz * sg
    assert out.dtype == F and x0p.dtype == F
    return out, (x0p if hist is not None else None)


def travel_back(x, z, ra, rs, to, c):
    """the jump at counter c (row r = c + 1): x' = (ra[r] x) + (rs[r] z), the counter -> to[r]"""
    r = c + 1
    out = F(ra[r]) * np.asarray(x, dtype=F) + F(rs[r]) * np.asarray(z, dtype=F)
    assert out.dtype == F
    return out, int(to[r])


def gray_bound(a, p, x0_max, y_max):
    """A bound on |a . x0' - y| after project_gray at strength 1, from the roundings involved, with u = EPS and, in exact arithmetic,
    a . p = 1 (p is a / |a|^2 rounded: a . p = 1 + e_p, |e_p| <= u sum |a_c p_c| / ... carried below as its own term):

      the computed g~ = a . x0 + e_g,   |e_g| <= gamma_C sum |a_c x0_c|           C products and C - 1 sums: gamma_C = C u / (1 - C u)
      the computed r~ = (y - g~)(1 + d),  |d| <= u
      x0'_c = (x0_c + p_c r~ (1 + d1)(1 + d2))(1 + d3)                            lam p_c (lam = 1: exact), the product, the sum
      a . x0' - y = (a . x0 - y) + (a . p) r~ + E
                  = -r + e_g + (1 + e_p)(r - e_g)(1 + d) + E,   r = y - a . x0 exactly
      |a . x0' - y| <= |r| (u + |e_p| (1 + u)) + |e_g| (u + |e_p| (1 + u)) + |E|
      |E| <= sum |a_c| (2 u (1 + u) |p_c r~| + u |x0'_c|)                         the product's and the sum's roundings, per channel
      |e_p| <= u sum |a_c p_c|                                                    p_c rounded once from float64

    evaluated in float64 with |x0_c| <= x0_max, |y| <= y_max, |r| <= y_max + sum |a_c| x0_max, |x0'_c| <= x0_max + 1.01 |p_c| |r|."""
    a64, p64 = np.abs(np.asarray(a, dtype=F).astype(np.float64)), np.abs(np.asarray(p, dtype=F).astype(np.float64))
    Cn, u = a64.shape[0], EPS
    gam = Cn * u / (1.0 - Cn * u)
    sa = a64.sum() * x0_max
    e_g = gam * sa
    r = y_max + sa + e_g
    e_p = u * (a64 * p64).sum() + abs((a64 * p64).sum() - 1.0)      # (the second term: what a . p misses 1 by, as computed in float64)
    rt = r * (1.0 + u)
    x0p = x0_max + 1.01 * p64 * rt
    E = (a64 * (2.0 * u * (1.0 + u) * p64 * rt + u * x0p)).sum()
    k = u + e_p * (1.0 + u)
    return float(r * k + e_g * (1.0 + k) + E)
