"""The host tables of the diffusion (sr3_hip/diffusion.py, their old home, still exports every name): pure float64 maths and the
config keys' parsers; no device, no engine call.

Sampler (engine extension, `"sampler": {"type": "ddim", "steps": S, "eta": e}` in the schedule dict or `set_sampler`): the same
captured step replayed S times over a strided walk through the schedule -- `sampler_tables` restates the DDIM update in the fused
tail's linear form, so a sampler is five other coefficient tables, another level table and (DDPM) a step-index -> timestep map.
`"type": "dpmpp_2m"` is the second-order multistep solver DPM-Solver++(2M) on a walk uniform in log-SNR (`"walk": "logsnr"`, its
default; DDIM takes the key too): one more table, c3, and one image-sized buffer that carries the previous step's x0 (st['hist']).
"walk" may also be an explicit list of timesteps (strictly increasing, ending at T - 1): the chain of a distilled student (sr3_hip/distill.py).

Objective (engine extension, `"prediction": "eps" | "v" | "x0"` and `"loss": {"type", "delta", "weight", "gamma"}` in model.diffusion, or
`set_prediction` / `set_objective`): what the network's output stands for and how the training loss weighs it.  Training hands per-image
target coefficients and weights to sr3_train_step_ex (`prediction_coefs`, `loss_weights`); sampling changes the two tables a, b of the
step tail's x0c = clip(a x - b out) and nothing else, in every loop.
"""
import numpy as np
import torch


def make_beta_schedule(schedule, n_timestep, linear_start=1e-4, linear_end=2e-2, cosine_s=8e-3):
    """float64 beta schedules named as in the reference (diffusion.py:12-49)."""
    if schedule == 'linear':
        return np.linspace(linear_start, linear_end, n_timestep, dtype=np.float64)
    if schedule == 'quad':
        return np.linspace(linear_start ** 0.5, linear_end ** 0.5, n_timestep, dtype=np.float64) ** 2
    if schedule in ('warmup10', 'warmup50'):
        frac = 0.1 if schedule == 'warmup10' else 0.5
        betas = np.full(n_timestep, linear_end, dtype=np.float64)
        n = int(n_timestep * frac)
        betas[:n] = np.linspace(linear_start, linear_end, n, dtype=np.float64)
        return betas
    if schedule == 'const':
        return np.full(n_timestep, linear_end, dtype=np.float64)
    if schedule == 'jsd':
        return 1.0 / np.linspace(n_timestep, 1, n_timestep, dtype=np.float64)
    if schedule == 'cosine':
        steps = torch.arange(n_timestep + 1, dtype=torch.float64) / n_timestep + cosine_s
        ac = torch.cos(steps / (1 + cosine_s) * np.pi / 2).pow(2)
        ac = ac / ac[0]
        return (1 - ac[1:] / ac[:-1]).clamp(max=0.999).numpy()
    raise NotImplementedError(schedule)


def _check_walk_args(alphas_cumprod, steps):
    ac = np.asarray(alphas_cumprod, dtype=np.float64).reshape(-1)
    T = int(ac.shape[0])
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)):
        raise ValueError('sampler steps must be an integer (got %r)' % (steps,))
    if T < 1 or not np.all(np.isfinite(ac)) or not np.all((ac > 0.0) & (ac < 1.0)):
        raise ValueError('alphas_cumprod must be finite values in (0, 1)')
    S = int(steps)
    if S < 1 or S > T:
        raise ValueError('sampler steps must lie in [1, %d] (got %d)' % (T, S))
    return ac, T, S


def _half_logsnr(ac):
    """lambda = log(alpha / sigma) = 0.5 log(ac / (1 - ac)): what a DPM-Solver steps in."""
    return 0.5 * np.log(ac / (1.0 - ac))


WALKS = ('time', 'logsnr')


def _explicit_walk(alphas_cumprod, steps, walk):
    """A walk given as a list or array of timesteps: checked, returned as int64 [S].  `steps` None: the list's length."""
    try:
        arr = np.asarray(walk)
    except (TypeError, ValueError):
        arr = None
    if arr is None or arr.ndim != 1 or arr.size == 0 or arr.dtype == np.bool_ or not np.issubdtype(arr.dtype, np.integer):
        raise ValueError('sampler walk must be one of %s or a non-empty list of integer timesteps (got %r)'
                         % (', '.join(repr(w) for w in WALKS), walk))
    tau = arr.astype(np.int64)
    ac, T, S = _check_walk_args(alphas_cumprod, int(tau.shape[0]) if steps is None else steps)
    if tau.shape[0] != S:
        raise ValueError('sampler walk has %d timesteps but steps is %d' % (tau.shape[0], S))
    if tau.min() < 0 or tau.max() > T - 1:
        raise ValueError('sampler walk must lie in [0, %d] (got %s)' % (T - 1, tau.tolist()))
    if np.any(np.diff(tau) <= 0):
        raise ValueError('sampler walk must be strictly increasing (got %s)' % (tau.tolist(),))
    if tau[-1] != T - 1:
        raise ValueError('sampler walk must end at T - 1 = %d (got %d)' % (T - 1, tau[-1]))
    return tau


def sampler_walk(alphas_cumprod, steps, walk='time'):
    """The timesteps a sampler visits: tau, int64 [S], strictly increasing, tau[0] = 0 and tau[S-1] = T - 1 (S = 1: [T - 1]).

    walk = a list or array of timesteps: that walk itself, checked -- strictly increasing integers in [0, T - 1], the last one T - 1, as
    many as `steps` (None: however many there are); a ValueError names the fault.  Its first timestep need not be 0: the walk of a
    distilled student (sr3_hip.distill) is every second timestep of its teacher's.

    walk = 'time': uniform in the timestep, round(linspace(0, T - 1, S)).  walk = 'logsnr': uniform in lambda_t = 0.5 log(ac_t /
    (1 - ac_t)) -- tau[i] is the timestep whose lambda is nearest the i-th of S evenly spaced targets between lambda_0 and
    lambda_{T-1}; both ends are pinned, one forward pass (tau[i] >= tau[i-1] + 1) makes the walk strictly increasing where the schedule
    is too coarse for the targets (its first timesteps, where lambda moves fastest) and one backward pass (tau[i] <= tau[i+1] - 1)
    takes back what the forward pass pushed past the top.  A multistep solver's extrapolation is only as good as the ratio of
    consecutive lambda intervals is tame; on the 'time' walk the last intervals are enormous in lambda."""
    if not isinstance(walk, str):
        return _explicit_walk(alphas_cumprod, steps, walk)
    ac, T, S = _check_walk_args(alphas_cumprod, steps)
    if walk not in WALKS:
        raise ValueError('sampler walk must be one of %s (got %r)' % (', '.join(repr(w) for w in WALKS), walk))
    if S == 1:
        return np.array([T - 1], dtype=np.int64)
    if walk == 'time':
        tau = np.round(np.linspace(0, T - 1, S)).astype(np.int64)
    else:
        lam = _half_logsnr(ac)
        target = np.linspace(lam[0], lam[T - 1], S)
        tau = np.array([int(np.argmin(np.abs(lam - v))) for v in target], dtype=np.int64)
        tau[0], tau[S - 1] = 0, T - 1
        for i in range(1, S):
            tau[i] = max(tau[i], tau[i - 1] + 1)
        tau[S - 1] = T - 1
        for i in range(S - 2, -1, -1):
            tau[i] = min(tau[i], tau[i + 1] - 1)
    assert tau[-1] == T - 1 and tau[0] == 0 and np.all(np.diff(tau) > 0), 'sampler walk is not strictly increasing'
    return tau


SAMPLER_KINDS = ('ddim', 'dpmpp_2m')


def _check_sampler_kind(kind):
    if kind not in SAMPLER_KINDS:
        raise NotImplementedError('sampler type %r (only %s)' % (kind, ', '.join('"%s"' % k for k in SAMPLER_KINDS)))


PREDICTIONS = ('eps', 'v', 'x0')
LOSS_TYPES = ('l1', 'l2', 'huber')          # the loss_kind numbers of sr3_train_step_ex, in order
LOSS_WEIGHTS = ('uniform', 'min_snr')


def _check_prediction(kind):
    if kind not in PREDICTIONS:
        raise ValueError('prediction must be one of %s (got %r)' % (', '.join(repr(k) for k in PREDICTIONS), kind))


def _positive(name, v):
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError('%s must be a number (got %r)' % (name, v))
    if isinstance(v, bool) or not np.isfinite(f) or not f > 0.0:
        raise ValueError('%s must be finite and > 0 (got %r)' % (name, v))
    return f


SELF_CONDITION_PROB = 0.5      # the default of the config key (Chen et al. 2022 train half of the batch self-conditioned)


def parse_self_condition(spec):
    """The config key model.diffusion.self_condition -> the argument of set_self_condition: {"prob": p} -> p, true or {} -> the default
    0.5, absent / null / false -> None (off)."""
    if spec is None or spec is False:
        return None
    if spec is True:
        return SELF_CONDITION_PROB
    if not hasattr(spec, 'get') or not hasattr(spec, 'keys'):
        raise ValueError('self_condition: true or a dict with "prob" is expected (got %r)' % (spec,))
    for k in spec.keys():
        if k != 'prob':
            raise ValueError('self_condition: unknown key %r (known: "prob")' % (k,))
    p = spec.get('prob')
    return SELF_CONDITION_PROB if p is None else p


FEATURE_CACHE_KEYS = ('interval', 'depth', 'full_last')


def parse_feature_cache(spec):
    """The config key "feature_cache" of a phase's beta_schedule block -> the keyword arguments of set_feature_cache: {"interval": N,
    "depth": d, "full_last": k} ("interval" required; depth 1 and full_last 0 where absent), absent / null -> interval None (off)."""
    if spec is None:
        return dict(interval=None)
    if not hasattr(spec, 'get') or not hasattr(spec, 'keys'):
        raise ValueError('feature_cache: a dict with "interval" is expected (got %r)' % (spec,))
    for k in spec.keys():
        if k not in FEATURE_CACHE_KEYS:
            raise ValueError('feature_cache: unknown key %r (known: %s)' % (k, ', '.join('"%s"' % n for n in FEATURE_CACHE_KEYS)))
    if spec.get('interval') is None:
        raise ValueError('feature_cache: "interval" is required')
    return dict(interval=spec['interval'], depth=spec.get('depth', 1), full_last=spec.get('full_last', 0))


def feature_cache_refresh(k, total, interval, full_last=0):
    """THE refresh schedule of feature-cached sampling: does step k of a chain of `total` steps (k = 0 the chain's first, at the highest
    noise) run the full forward and refill the cache?  The first step and every interval-th behind it, and the last full_last steps;
    every other step runs the shallow forward on the cache of the last full one.  interval 1: every step is full."""
    k, total, interval, full_last = int(k), int(total), int(interval), int(full_last)
    if not 0 <= k < total:
        raise ValueError('feature_cache_refresh: step %d outside a chain of %d steps' % (k, total))
    if interval < 1 or full_last < 0:
        raise ValueError('feature_cache_refresh: interval >= 1 and full_last >= 0 are expected (got %d, %d)' % (interval, full_last))
    return k % interval == 0 or k >= total - full_last


COND_AUGMENT_KEYS = ('max_level', 'sample_level', 'level_channel')


def parse_cond_augment(spec):
    """The config key model.diffusion.cond_augment -> the keyword arguments of set_cond_augment: {"max_level": m, "sample_level": s,
    "level_channel": bool} ("max_level" required; sample_level 0.0 and level_channel true where absent), absent / null -> max_level
    None (off)."""
    if spec is None:
        return dict(max_level=None)
    if not hasattr(spec, 'get') or not hasattr(spec, 'keys'):
        raise ValueError('cond_augment: a dict with "max_level" is expected (got %r)' % (spec,))
    for k in spec.keys():
        if k not in COND_AUGMENT_KEYS:
            raise ValueError('cond_augment: unknown key %r (known: %s)' % (k, ', '.join('"%s"' % n for n in COND_AUGMENT_KEYS)))
    if spec.get('max_level') is None:
        raise ValueError('cond_augment: "max_level" is required')
    return dict(max_level=spec['max_level'], sample_level=spec.get('sample_level', 0.0), level_channel=spec.get('level_channel', True))


def cond_level_coefs(s):
    """(a, s) of the augmented conditioning image a c + s eps as two fp32 tensors: s (numbers or a tensor, on any device) rounded to fp32
    first, then a = sqrt(1 - s^2) in float64 of that fp32 s, rounded once -- so a^2 + s^2 is 1 to fp32 rounding, and s = 0 gives a = 1
    exactly.  Every operation is a correctly rounded IEEE one: the host and the device give the same bits."""
    s32 = torch.as_tensor(s, dtype=torch.float32).reshape(-1).contiguous()
    a32 = (1.0 - s32.double() ** 2).sqrt().float()
    return a32, s32


def prediction_coefs(kind, ca, cb):
    """What the network's output `out` stands for at the noise level x = ca x0 + cb z (ca = sqrt(abar), cb = sqrt(1 - abar)), as the four
    coefficients the engine reads:  x0 = x0_a x - x0_b out  (the step tail's a, b) and the training target  tgt_z z + tgt_x0 x0.

        eps (the reference's; Ho et al. 2020):    out ~ z                 a, b = 1 / ca, cb / ca     target (1, 0)
        v   (Salimans & Ho 2022):                 out ~ ca z - cb x0      a, b = ca, cb              target (ca, -cb)
        x0:                                       out ~ x0                a, b = 0, -1               target (0, 1)

    Pure numpy, float64, no device; ca and cb broadcast.  Returns (x0_a, x0_b, tgt_z, tgt_x0) as arrays of their shape.  (The eps row is
    the schedule buffers' sqrt(1 / abar), sqrt(1 / abar - 1) as quotients: equal once rounded to the fp32 the engine's tables hold.)"""
    _check_prediction(kind)
    ca, cb = np.broadcast_arrays(np.asarray(ca, dtype=np.float64), np.asarray(cb, dtype=np.float64))
    one, zero = np.ones_like(ca), np.zeros_like(ca)
    if kind == 'eps':
        return 1.0 / ca, cb / ca, one, zero
    if kind == 'v':
        return ca.copy(), cb.copy(), ca.copy(), -cb
    return zero, -one, zero, one


def loss_weights(kind, weight, gamma, ca):
    """Per-noise-level weight of the training loss.  'uniform': 1.  'min_snr' (Min-SNR-gamma, Hang et al. 2023): min(SNR, gamma) divided
    by SNR, SNR + 1 or 1 for an eps-, v- or x0-predicting network, SNR = ca^2 / (1 - ca^2) -- which weighs the implied x0 error by
    min(SNR, gamma) whatever the network predicts.  Written as closed forms in g2 = ca^2 so that ca = 1 (SNR infinite: the first entry of
    SR3's level table) stays finite:  eps  min(1, gamma (1 - g2) / g2);  v  min(g2, gamma (1 - g2));  x0  min(g2 / (1 - g2), gamma), gamma
    at g2 = 1.  Pure numpy, float64, no device; `gamma` is read for 'min_snr' only."""
    _check_prediction(kind)
    if weight not in LOSS_WEIGHTS:
        raise ValueError('loss weight must be one of %s (got %r)' % (', '.join(repr(k) for k in LOSS_WEIGHTS), weight))
    g2 = np.asarray(ca, dtype=np.float64) ** 2
    if weight == 'uniform':
        return np.ones_like(g2)
    gamma = _positive('loss gamma', gamma)
    with np.errstate(divide='ignore', invalid='ignore'):
        if kind == 'eps':
            return np.minimum(1.0, gamma * (1.0 - g2) / g2)
        if kind == 'v':
            return np.minimum(g2, gamma * (1.0 - g2))
        return np.where(1.0 - g2 > 0.0, np.minimum(g2 / (1.0 - g2), gamma), gamma)


def sampler_tables(alphas_cumprod, steps, eta, *, kind='ddim', walk='time', prediction='eps'):
    """Tables of a sampler over a walk through the schedule (`sampler_walk`) in the form of the engine's fused step tail,

        x0c = clip(a x - b eps) ;  x_new = c1 x0c + c2 x + c3 x0c_prev + sigma z.

    kind = 'ddim' (Song et al. 2021, eq. 12 and 16; c3 = 0): the textbook update  sqrt(ap) x0c + d eps' + sigma z  with
    eps' = (x - sqrt(ab) x0c) / sqrt(1 - ab) re-derived from the
    clipped x0 (the reference's clip_denoised semantics), d = sqrt(1 - ap - sigma^2): collecting x0c and x gives
    c1 = sqrt(ap) - d sqrt(ab) / sqrt(1 - ab), c2 = d / sqrt(1 - ab).  ab = alphas_cumprod[tau[j]], ap = that of the next (smaller)
    timestep of the walk and 1 after the last; sigma = eta sqrt((1 - ap) / (1 - ab)) sqrt(1 - ab / ap).  With steps = T and eta = 1 these
    are the reference's posterior_mean_coef1/2 and sqrt(posterior_variance).

    kind = 'dpmpp_2m' (DPM-Solver++(2M), Lu et al. 2022, Algorithm 2, data prediction; eta must be 0): with lambda = 0.5 log(ac /
    (1 - ac)), h = lambda(ap) - lambda(ab) and r = (the previous step's h) / h, the update is
    x_new = sqrt(1 - ap) / sqrt(1 - ab) x - sqrt(ap) expm1(-h) D with D = (1 + 1 / (2r)) x0c - 1 / (2r) x0c_prev, so with
    k = -sqrt(ap) expm1(-h): c1 = k (1 + 1 / (2r)), c2 = sqrt(1 - ap) / sqrt(1 - ab), c3 = -k / (2r).  The first step taken has no
    history (c1 = k, c3 = 0: DDIM's step), and the last one goes to ap = 1, where lambda is infinite: c1 = 1, c2 = c3 = 0, DDIM's too.

    prediction ('eps' | 'v' | 'x0', `prediction_coefs`): what the network's output stands for.  Only a and b change with it -- c1, c2, c3,
    sigma, level and tau do not: DDIM re-derives eps from the clipped x0, and the multistep solver is already in data-prediction form.

    Pure numpy, float64, no device.  The step index j counts like the device counter: j = steps - 1 is the first step taken, j = 0 the
    last.  Returns a dict: tau (`sampler_walk`), a, b, c1, c2, c3,
    sigma ([S]) and level ([S + 1]: level[j + 1] = sqrt(alphas_cumprod[tau[j]]), the reference's sqrt_alphas_cumprod_prev[t + 1] at
    t = tau[j]; level[0] = 1).  walk: 'time', 'logsnr' or an explicit list of timesteps (`sampler_walk`; `steps` may then be None)."""
    if not isinstance(walk, str):
        walk = _explicit_walk(alphas_cumprod, steps, walk)
        steps = int(walk.shape[0])
    ac, T, S = _check_walk_args(alphas_cumprod, steps)
    try:
        eta = float(eta)
    except (TypeError, ValueError):
        raise ValueError('sampler eta must be a number (got %r)' % (eta,))
    if not np.isfinite(eta) or not 0.0 <= eta <= 1.0:
        raise ValueError('sampler eta must lie in [0, 1] (got %r)' % (eta,))
    if kind not in SAMPLER_KINDS:
        raise ValueError('sampler kind must be one of %s (got %r)' % (', '.join(repr(k) for k in SAMPLER_KINDS), kind))
    if kind == 'dpmpp_2m' and eta != 0.0:
        raise ValueError('sampler kind \'dpmpp_2m\' is the deterministic solver: eta must be 0 (got %r)' % (eta,))
    _check_prediction(prediction)
    tau = sampler_walk(ac, S, walk)
    ab = ac[tau]
    ap = np.append(1.0, ab[:-1])
    if kind == 'ddim':
        sigma = eta * np.sqrt((1.0 - ap) / (1.0 - ab)) * np.sqrt(1.0 - ab / ap)
        d = np.sqrt(np.maximum(1.0 - ap - sigma ** 2, 0.0))
        c1, c2, c3 = np.sqrt(ap) - d * np.sqrt(ab) / np.sqrt(1.0 - ab), d / np.sqrt(1.0 - ab), np.zeros(S)
    else:
        sigma, c1, c2, c3 = np.zeros(S), np.ones(S), np.zeros(S), np.zeros(S)
        lam = _half_logsnr(ab)
        for j in range(1, S):
            h = _half_logsnr(ap[j]) - lam[j]
            k = -np.sqrt(ap[j]) * np.expm1(-h)
            c2[j] = np.sqrt(1.0 - ap[j]) / np.sqrt(1.0 - ab[j])
            if j == S - 1:
                c1[j] = k
            else:
                r = (lam[j] - lam[j + 1]) / h
                c1[j], c3[j] = k * (1.0 + 1.0 / (2.0 * r)), -k / (2.0 * r)
    a, b = np.sqrt(1.0 / ab), np.sqrt(1.0 / ab - 1)
    if prediction != 'eps':
        a, b = prediction_coefs(prediction, np.sqrt(ab), np.sqrt(1.0 - ab))[:2]
    out = dict(tau=tau, a=a, b=b, c1=c1, c2=c2, c3=c3, sigma=sigma, level=np.append(1.0, np.sqrt(ab)))
    if not all(np.all(np.isfinite(v)) for v in out.values()):
        raise ValueError('sampler tables are not finite')
    return out


LEARNED_VARIANCE_LAMBDA = 0.001      # the default of the config key (Nichol & Dhariwal 2021, section 3.1)


def parse_learned_variance(spec):
    """The config key model.diffusion.learned_variance -> the argument of set_learned_variance: {"lambda": l} -> l, true or {} -> the
    default 0.001, absent / null / false -> None (off)."""
    if spec is None or spec is False:
        return None
    if spec is True:
        return LEARNED_VARIANCE_LAMBDA
    if not hasattr(spec, 'get') or not hasattr(spec, 'keys'):
        raise ValueError('learned_variance: true or a dict with "lambda" is expected (got %r)' % (spec,))
    for k in spec.keys():
        if k != 'lambda':
            raise ValueError('learned_variance: unknown key %r (known: "lambda")' % (k,))
    lam = spec.get('lambda')
    return LEARNED_VARIANCE_LAMBDA if lam is None else lam


def ancestral_tables(alphas_cumprod, steps, *, walk='time', prediction='eps'):
    """Tables of the respaced DDPM walk (Nichol & Dhariwal 2021, section 4) over `sampler_walk`'s timesteps tau, in the form of the
    step tail: with ab_j = alphas_cumprod[tau[j]] and ab_{-1} = 1,

        beta'_j = 1 - ab_j / ab_{j-1} ;  beta~'_j = beta'_j (1 - ab_{j-1}) / (1 - ab_j)
        c1 = beta'_j sqrt(ab_{j-1}) / (1 - ab_j) ;  c2 = (1 - ab_{j-1}) sqrt(1 - beta'_j) / (1 - ab_j)      the posterior's mean

    a, b as `sampler_tables` (by `prediction`); sigma = sqrt(beta~'), 0 at j = 0 -- the fixed small variance, which the learned-variance
    tail reads only for that zero: the mark of the walk's last step; log_beta = log beta', log_beta_tilde = log beta~' with entry 0
    set to entry 1 (beta~'_0 = 0; the Improved-DDPM convention, not log 1e-20; a one-step walk: log beta'_0).  steps = T gives the
    schedule's own betas and posterior_mean_coef1/2.  Pure numpy, float64, no device.  Returns a dict: tau, a, b, c1, c2, sigma,
    log_beta, log_beta_tilde ([S]) and level ([S + 1], as `sampler_tables`)."""
    if not isinstance(walk, str):
        walk = _explicit_walk(alphas_cumprod, steps, walk)
        steps = int(walk.shape[0])
    ac, T, S = _check_walk_args(alphas_cumprod, steps)
    _check_prediction(prediction)
    tau = sampler_walk(ac, S, walk)
    ab = ac[tau]
    ap = np.append(1.0, ab[:-1])
    beta = 1.0 - ab / ap
    bt = beta * (1.0 - ap) / (1.0 - ab)
    c1, c2 = beta * np.sqrt(ap) / (1.0 - ab), (1.0 - ap) * np.sqrt(1.0 - beta) / (1.0 - ab)
    sigma = np.sqrt(bt)
    sigma[0] = 0.0
    log_beta = np.log(beta)
    with np.errstate(divide='ignore'):
        log_bt = np.log(bt)
    log_bt[0] = log_bt[1] if S > 1 else log_beta[0]
    a, b = np.sqrt(1.0 / ab), np.sqrt(1.0 / ab - 1)
    if prediction != 'eps':
        a, b = prediction_coefs(prediction, np.sqrt(ab), np.sqrt(1.0 - ab))[:2]
    out = dict(tau=tau, a=a, b=b, c1=c1, c2=c2, sigma=sigma, log_beta=log_beta, log_beta_tilde=log_bt, level=np.append(1.0, np.sqrt(ab)))
    if not all(np.all(np.isfinite(v)) for v in out.values()):
        raise ValueError('ancestral tables are not finite')
    return out


def hybrid_step_scalars(tables, t):
    """The rows of sr3_train_step_ex2's step_scalars for the steps `t` (ints, 0-based, into `ancestral_tables(ac, T)`): float64 [n, 8]
    = {a, b, c1, c2, log beta, log beta~ (clipped), last, 0}, last = 1 at t = 0."""
    t = np.asarray(t, dtype=np.int64).reshape(-1)
    out = np.zeros((t.shape[0], 8), dtype=np.float64)
    for k, name in enumerate(('a', 'b', 'c1', 'c2', 'log_beta', 'log_beta_tilde')):
        out[:, k] = np.asarray(tables[name], dtype=np.float64)[t]
    out[:, 6] = (t == 0).astype(np.float64)
    return out


def widen_for_learned_variance(state):
    """An existing checkpoint -> one a learned-variance network of twice the output rows loads: C zero rows are appended to
    final_conv.block.3.weight and to its bias (C = the rows they have; v = 0 everywhere: sigma^2 the geometric midpoint of beta and beta~),
    every other entry is kept.  `state`: a *_gen.pth state dict (any key prefix), or the dict of a *_opt.pth -- there the Adam moments
    of those two parameters, the last two of the parameter table, are widened with zeros.  Returns a new dict; tensors that do not
    change are shared with the input."""
    def rows(t):
        return torch.cat([t, torch.zeros_like(t)], 0)
    if isinstance(state, dict) and 'optimizer' in state:
        out = dict(state)
        opt = dict(state['optimizer'])
        st = dict(opt.get('state') or {})
        for i in sorted(st.keys())[-2:]:       # final_conv.block.3.weight, .bias: the last two entries of the table
            st[i] = {k: (rows(v) if k in ('exp_avg', 'exp_avg_sq') else v) for k, v in st[i].items()}
        opt['state'] = st
        out['optimizer'] = opt
        return out
    out = type(state)()
    hit = 0
    for k, v in state.items():
        if k.endswith('final_conv.block.3.weight') or k.endswith('final_conv.block.3.bias'):
            v = rows(v)
            hit += 1
        out[k] = v
    if hit == 0:
        raise ValueError('widen_for_learned_variance: no final_conv.block.3.weight / .bias in the state dict')
    return out


_SAMPLER_TABLES = ('a', 'b', 'c1', 'c2', 'c3', 'sigma', 'level', 'tau', 'log_beta', 'log_beta_tilde')

_BUFFERS = ('betas', 'alphas_cumprod', 'alphas_cumprod_prev', 'sqrt_alphas_cumprod',
            'sqrt_one_minus_alphas_cumprod', 'log_one_minus_alphas_cumprod', 'sqrt_recip_alphas_cumprod',
            'sqrt_recipm1_alphas_cumprod', 'posterior_variance', 'posterior_log_variance_clipped',
            'posterior_mean_coef1', 'posterior_mean_coef2')
