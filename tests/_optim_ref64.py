"""The optimizer step restated with numpy: once in float64 (the yardstick) and once in float32 in the written order of
torch.optim.AdamW's single-tensor path (torch/optim/adam.py _single_tensor_adam, decoupled weight decay), after
torch.nn.utils.clip_grad_norm_(max_norm, 2), followed by ModelEMA.update (mmdet3d/core/hook/ema.py:48-59).
tests/test_optim_ref64_cpu.py proves both against torch itself on the CPU; tests/test_gpu_optim.py measures the kernels
(preworld_amd/csrc/pw_optim.hip) against the float64 form with the float32 form's own error as the scale.

A row is a dict: p, g, m, v, e (numpy arrays; g / m / v None: an EMA-only row, p is only read; e None: no shadow) and its
group's lr, wd, b1, b2, eps.  `step` returns new rows plus (t, u, skipped, total); its inputs stay untouched.

The written order (all scalars are formed in Python floats = float64 and rounded to the array type ONCE, as torch does when it
hands a Python scalar to a float32 kernel):
    total = sqrt(sum over all g of g*g);  coef = min(1, max_norm / (total + 1e-6))           clip_grad_norm_
    g' = coef * g                                                                             (coef = 1 exactly without clipping)
    p  = p * (1 - lr*wd)                                                                      param.mul_(1 - lr * weight_decay)
    m  = m + (g' - m) * (1 - b1)                                                              exp_avg.lerp_(grad, 1 - beta1)
    v  = v * b2 + ((1 - b2) * g') * g'                                                        mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    den = sqrt(v) / sqrt(1 - b2^t) + eps                                                      (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
    p  = p + ((-lr / (1 - b1^t)) * m) / den                                                   param.addcdiv_(exp_avg, denom, value=-step_size)
    e  = e * d + (1 - d) * p,  d = decay * (1 - exp(-u / 2000))                               v *= d; v += (1.0 - d) * msd[k]
with t and u the counters AFTER their increment.  skip_nonfinite: a non-finite total changes nothing and counts in `skipped`.
"""
import math

import numpy as np

F32, F64 = np.float32, np.float64
MAX_NORM, DECAY, INIT_UPDATES = 5.0, 0.9990, 10560      # bevstereo-occ.py:235-236; MEGVIIEMAHook(init_updates=10560)


def total_norm(rows, dtype):
    """float64: sqrt of the one sum.  float32: clip_grad_norm_'s own route, a float32 norm per tensor and the norm of those"""
    gs = [r['g'] for r in rows if r['g'] is not None]
    if dtype is F64:
        return math.sqrt(sum(float(np.sum(np.asarray(g, F64) ** 2)) for g in gs)) if gs else 0.0
    with np.errstate(over='ignore', invalid='ignore'):
        norms = np.array([np.sqrt(np.sum(g * g, dtype=F32), dtype=F32) for g in gs], F32)
        return np.sqrt(np.sum(norms * norms, dtype=F32), dtype=F32) if gs else F32(0)


def clip_coef(total, max_norm, dtype):
    """max_norm / (total + 1e-6) clamped to <= 1 in `dtype`; a NaN stays a NaN (torch.clamp).  In float32 the quotient is formed as
    torch forms `float / tensor` (Tensor.__rtruediv__): the reciprocal, rounded, times max_norm"""
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        x = dtype(total) + dtype(1e-6)
        c = (dtype(1.0) / x) * dtype(max_norm) if dtype is F32 else dtype(max_norm) / x
    return dtype(1.0) if c > 1.0 else dtype(c)


def step(rows, t, u, dtype, max_norm=MAX_NORM, decay=DECAY, skip_nonfinite=False, coef=None, total=None):
    """one optimizer step in `dtype` (F64 or F32).  max_norm None: no clipping; decay None: no EMA.  coef / total: taken as given
    when passed (the CPU test hands torch's own coefficient to the float32 form to compare the update alone).
    Returns (rows', t', u', skipped (0 / 1), total)."""
    if total is None:
        total = total_norm(rows, dtype) if (max_norm is not None or skip_nonfinite) else None
    if skip_nonfinite and not np.isfinite(total):
        return [dict(r) for r in rows], t, u, 1, total
    if coef is None:
        coef = clip_coef(total, max_norm, dtype) if max_norm is not None else dtype(1.0)
    coef = dtype(coef)
    any_opt = any(r['g'] is not None and r['p'].size for r in rows)
    t1 = t + 1 if any_opt else t
    u1 = u + 1 if decay is not None else u
    if decay is not None:
        dd = decay * (1.0 - math.exp(-u1 / 2000.0))
        d, omd = dtype(dd), dtype(1.0 - dd)
    out = []
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        for r in rows:
            n = dict(r)
            p = np.asarray(r['p'], dtype)
            if r['g'] is not None:
                lr, wd, b1, b2, eps = r['lr'], r['wd'], r['b1'], r['b2'], r['eps']
                g, m, v = (np.asarray(r[k], dtype) for k in 'gmv')
                gg = coef * g
                p = p * dtype(1.0 - lr * wd)
                m = m + (gg - m) * dtype(1.0 - b1)
                v = v * dtype(b2) + (dtype(1.0 - b2) * gg) * gg
                den = np.sqrt(v) / dtype((1.0 - b2 ** float(t1)) ** 0.5) + dtype(eps)
                p = p + (dtype(-(lr / (1.0 - b1 ** float(t1)))) * m) / den
                n.update(p=p, m=m, v=v)
            if decay is not None and r['e'] is not None:
                n['e'] = np.asarray(r['e'], dtype) * d + omd * p
            out.append(n)
    return out, t1, u1, 0, total


def q_of(got, ref64):
    """max |got - ref64| in units of 2^-24 max |ref64| (half an ulp of the largest entry); where the reference is all zero the
    result has to be zero too (0, else inf); a non-finite reference has to be matched in kind, entry by entry"""
    got, ref64 = np.asarray(got, F64), np.asarray(ref64, F64)
    fin = np.isfinite(ref64)
    if not fin.all():
        same = np.array_equal(np.isnan(got), np.isnan(ref64)) and np.array_equal(got[np.isinf(ref64)], ref64[np.isinf(ref64)])
        if not same:
            return math.inf
        got, ref64 = got[fin], ref64[fin]
    if got.size == 0:
        return 0.0
    scale = float(np.max(np.abs(ref64)))
    err = float(np.max(np.abs(got - ref64)))
    if scale == 0.0:
        return 0.0 if err == 0.0 else math.inf
    return err / (2.0 ** -24 * scale)


def bound(q32):
    """q <= 2 q32 + 1 (the rule of _forecast_ref64.bound): twice what the float32 form of the same arithmetic loses on the same
    inputs (another libm pow / exp behind the scalars, a norm summed in another order), plus one rounding of the output"""
    return 2.0 * q32 + 1.0


# ------------------------------------------------------------------------------------------ the adversarial tensor list
GROUPS = (dict(lr=1e-4, weight_decay=1e-2), dict(lr=1e-4, weight_decay=0.0), dict(lr=1e-3, weight_decay=1e-2))
BETAS, EPS = (0.9, 0.999), 1e-8


def adversarial(chunk):
    """[(name, numel, group, kind)]; kind: 'param', 'view4' (a parameter that is a view starting 4 bytes past a 16-byte boundary),
    'nograd' (grad stays None), 'buffer' (float buffer: EMA only), 'ibuffer' (int64 buffer: nobody's business).
    `chunk` is the plan's chunk size: the largest tensor spans more than two chunks whatever it is."""
    big = max(70001, 2 * chunk + 5)
    spec = [('w%02d' % i, n, 0, 'param') for i, n in enumerate((1, 3, 5, 64, 255, 256, 257, 1023, 4099, big))]
    spec += [('s%02d' % i, 5 + i, i % 3, 'param') for i in range(40)]          # more rows than any by-value table held
    spec += [('view4', 301, 0, 'view4'), ('view4b', 2, 2, 'view4')]
    spec += [('frozen0', 7, 0, 'nograd'), ('frozen1', 130, 1, 'nograd')]
    spec += [('running_mean', 9, 0, 'buffer'), ('running_var', 515, 0, 'buffer'), ('num_batches_tracked', 1, 0, 'ibuffer')]
    return spec


def build_model(spec, device, seed=0):
    """an nn.Module holding the list (parameters and buffers under their names, in order) and the AdamW parameter groups"""
    import torch
    gen = torch.Generator().manual_seed(seed)
    model = torch.nn.Module()
    groups = [dict(params=[], **g) for g in GROUPS]
    model._bases = []
    for name, n, grp, kind in spec:
        if kind == 'ibuffer':
            model.register_buffer(name, torch.full((n,), 3, dtype=torch.int64, device=device))
            continue
        val = (torch.randn(n, generator=gen) * 0.5).to(device)
        if kind == 'buffer':
            model.register_buffer(name, val)
            continue
        if kind == 'view4':
            base = torch.zeros(n + 8, device=device)
            model._bases.append(base)
            val = base[1:1 + n].copy_(val)
            assert device == 'cpu' or val.data_ptr() % 16 == 4
        p = torch.nn.Parameter(val)
        model.register_parameter(name, p)
        groups[grp]['params'].append(p)
    return model, groups


def grads(spec, seed, norm=None):
    """seeded float32 gradients by name (None for 'nograd'); scaled to the global L2 norm `norm` when given; norm == 0: zeros"""
    rng = np.random.default_rng(1000 + seed)
    out = {}
    for name, n, _, kind in spec:
        if kind in ('param', 'view4'):
            out[name] = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 0)).astype(F32)
    if norm is not None:
        tot = math.sqrt(sum(float(np.sum(g.astype(F64) ** 2)) for g in out.values()))
        out = {k: (g * F32(norm / tot)).astype(F32) if norm else np.zeros_like(g) for k, g in out.items()}
    return out


def set_grads(model, gr):
    """copy into existing .grad buffers (their addresses stay) or create them"""
    import torch
    for name, p in model.named_parameters():
        if name in gr:
            g = torch.from_numpy(gr[name]).to(p.device)
            if p.grad is None:
                p.grad = g.clone()
            else:
                p.grad.copy_(g)


def rows_of(model, groups, moments, shadow, betas=BETAS, eps=EPS):
    """the rows of the restatement from live torch objects (copied to numpy): moments(p) -> (m, v) tensors or None when p has no
    state yet (zeros), shadow: state dict of the EMA model or None.  Returns (rows, names): optimizer rows then EMA-only rows."""
    import torch
    cpu = lambda t: t.detach().cpu().numpy().copy()
    gid = {id(p): g for g in groups for p in g['params']}
    rows, names = [], []
    for name, t in model.state_dict(keep_vars=True).items():
        if not t.dtype.is_floating_point:
            continue
        e = cpu(shadow[name]) if shadow is not None else None
        if isinstance(t, torch.nn.Parameter) and t.grad is not None:
            g = gid[id(t)]
            mv = moments(t)
            m, v = (cpu(mv[0]), cpu(mv[1])) if mv is not None else (np.zeros(t.numel(), F32), np.zeros(t.numel(), F32))
            rows.append(dict(p=cpu(t), g=cpu(t.grad), m=m, v=v, e=e, lr=g['lr'], wd=g['weight_decay'], b1=betas[0], b2=betas[1], eps=eps))
        elif e is not None:
            rows.append(dict(p=cpu(t), g=None, m=None, v=None, e=e))
        else:
            continue
        names.append(name)
    return rows, names
