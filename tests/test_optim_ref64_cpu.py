"""The optimizer step, CPU side: the numpy restatements of tests/_optim_ref64.py are proven against torch's own
clip_grad_norm_ + torch.optim.AdamW(foreach=False) + the three lines of ModelEMA.update (mmdet3d/core/hook/ema.py:56-59) on the
adversarial tensor list; the plan layout and the argument validation of the C entry points are exercised through the raw
library with made-up addresses (nothing is dereferenced, no kernel runs); FusedAdamW's state dict goes to torch.optim.AdamW
and back.

What "bit for bit where torch's own op order allows" comes to on the CPU (measured here, asserted below):
  * the clipped gradient and, at the first step (v = 0 before it), exp_avg_sq (v): equal bit for bit;
  * the weight decay, which can be seen alone in a parameter whose gradient is zero: equal bit for bit;
  * exp_avg (m) at every step and v from the second step on: torch's CPU lerp_ and addcmul_ are ONE fused multiply-add each
    (ATen's vectorised fmadd: weight * (end - self) + self, (value * t1) * t2 + self with a single rounding), the written form
    rounds the product first, as the kernels do (they are built without contraction): at most one rounding of m / v apart;
  * p and e: sqrt, div and the addcdiv follow, and p inherits m's and v's last bits.
For the second kind every tensor is held to the float64 form instead: the float32 form must be as close to it as torch is
(q32 <= 2 q_torch + 1), and torch itself within 8 half-ulps of the largest entry: a handful of roundings per element (decay,
difference, product, two sums, the quotient and the final add: each half an ulp of a value no larger than the result's largest),
and two more in m and four in v for the clipping coefficient, which torch forms from a float32 norm.
"""
import ctypes
import copy

import numpy as np
import pytest
import torch

import _optim_ref64 as R
from preworld_amd import _lib

CHUNK = _lib.PW_OPTIM['PW_OPTIM_CHUNK']
SPEC = R.adversarial(CHUNK)
TORCH_Q = 8.0


def _torch_ema_update(ema_model, model, updates, decay=R.DECAY):
    import math
    with torch.no_grad():
        d = decay * (1 - math.exp(-updates / 2000))
        msd = model.state_dict()
        for k, v in ema_model.state_dict().items():
            if v.dtype.is_floating_point:
                v *= d
                v += (1.0 - d) * msd[k].detach()


def _run(steps, t0):
    """torch's composition for `steps` steps from step count t0 (t0 > 0: a loaded state), every step checked against both forms"""
    model, groups = R.build_model(SPEC, 'cpu')
    opt = torch.optim.AdamW(groups, betas=R.BETAS, eps=R.EPS, foreach=False)
    ema = copy.deepcopy(model).eval()
    u = t0
    if t0:
        R.set_grads(model, R.grads(SPEC, 99))
        opt.step()                                        # creates the state
        rng = np.random.default_rng(5)
        sd = opt.state_dict()
        for st in sd['state'].values():
            st['step'] = torch.tensor(float(t0))
            st['exp_avg'] = torch.from_numpy((rng.standard_normal(st['exp_avg'].numel()) * 0.05).astype(np.float32))
            st['exp_avg_sq'] = torch.from_numpy((rng.standard_normal(st['exp_avg_sq'].numel()) ** 2 * 0.01).astype(np.float32))
        opt.load_state_dict(sd)
    params = [p for g in groups for p in g['params']]
    worst = {}
    for s in range(steps):
        # the norm is above 5 at the first step (the coefficient bites), below it afterwards (coefficient exactly 1)
        R.set_grads(model, R.grads(SPEC, s, norm=(40.0, 3.0, 0.7)[s % 3]))
        moments = lambda p: (opt.state[p]['exp_avg'], opt.state[p]['exp_avg_sq']) if 'exp_avg' in opt.state[p] else None
        rows, names = R.rows_of(model, opt.param_groups, moments, ema.state_dict())
        t = int(opt.state[params[0]]['step']) if 'step' in opt.state[params[0]] else 0
        # torch, with the gradients kept to read the coefficient back
        before = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        tot = torch.nn.utils.clip_grad_norm_(params, R.MAX_NORM, norm_type=2)
        coef = np.float32(min(1.0, float(R.MAX_NORM / (tot + 1e-6))))
        opt.step()
        u += 1
        _torch_ema_update(ema, model, u)
        for n, g in before.items():
            model.get_parameter(n).grad.copy_(g)
        r64, t64, u64, _, tot64 = R.step(rows, t, u - 1, R.F64)
        r32, t32, u32, _, tot32 = R.step(rows, t, u - 1, R.F32, coef=coef)
        r32own = R.step(rows, t, u - 1, R.F32)
        assert t64 == t32 == t + 1 == int(opt.state[params[0]]['step']) and u64 == u32 == u
        assert abs(float(tot) - tot64) <= 4 * 2.0 ** -24 * tot64 and abs(float(r32own[4]) - tot64) <= 4 * 2.0 ** -24 * tot64
        got = dict(model.state_dict())
        esd = ema.state_dict()
        for row64, row32, name in zip(r64, r32, names):
            tp = got[name].numpy()
            if row64['g'] is not None:
                st = opt.state[model.get_parameter(name)]
                tm, tv = st['exp_avg'].numpy(), st['exp_avg_sq'].numpy()
                if t == 0:
                    assert np.array_equal(row32['v'], tv), '%s: exp_avg_sq of the first step is not torch\'s bit for bit' % name
                for a, b in ((row32['m'], tm), (row32['v'], tv)):
                    assert np.max(np.abs(a.astype(np.float64) - b)) <= 2.0 ** -23 * np.max(np.abs(b)), name
                triples = (('p', tp), ('m', tm), ('v', tv), ('e', esd[name].numpy()))
            else:
                assert np.array_equal(row32['p'], tp)
                triples = (('e', esd[name].numpy()),)
            for k, tt in triples:
                qt, q32 = R.q_of(tt, row64[k]), R.q_of(row32[k], row64[k])
                key = (k, row64['g'] is not None)
                worst[key] = max(worst.get(key, (0, 0)), (qt, q32))
                assert qt <= TORCH_Q, '%s.%s: torch is %.2f half-ulps from the float64 form' % (name, k, qt)
                assert q32 <= R.bound(qt), '%s.%s: float32 form q = %.2f, torch %.2f' % (name, k, q32, qt)
    print('worst (q torch, q float32 form) by tensor kind:', worst)


def test_restatements_equal_torch_steps_1_to_3():
    _run(3, 0)


def test_restatements_equal_torch_from_loaded_step_10560():
    _run(1, R.INIT_UPDATES)


def test_weight_decay_alone_is_bit_exact_and_skip_rule():
    """a zero gradient leaves m = v = 0 and the addcdiv adds -0/eps: p is the decay alone; and the skip rule of the restatement"""
    p = np.random.default_rng(0).standard_normal(1000).astype(np.float32)
    z = np.zeros_like(p)
    row = dict(p=p, g=z, m=z, v=z, e=p.copy(), lr=1e-4, wd=1e-2, b1=0.9, b2=0.999, eps=1e-8)
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    tp.grad = torch.zeros(1000)
    torch.optim.AdamW([tp], lr=1e-4, weight_decay=1e-2, foreach=False).step()
    out, t, u, skipped, tot = R.step([row], 0, 0, R.F32)
    assert np.array_equal(out[0]['p'], tp.detach().numpy()) and (t, u, skipped, float(tot)) == (1, 1, 0, 0.0)
    bad = dict(row, g=z.copy())
    bad['g'][17] = np.inf
    out, t, u, skipped, tot = R.step([bad], 3, 4, R.F64, skip_nonfinite=True)
    assert (t, u, skipped) == (3, 4, 1) and not np.isfinite(tot) and all(out[0][k] is bad[k] for k in 'pmve')
    out, t, u, skipped, tot = R.step([bad], 3, 4, R.F32)
    assert (t, u, skipped) == (4, 5, 0) and np.isnan(out[0]['p'][17]) and np.isfinite(np.delete(out[0]['p'], 17)).all()


# ------------------------------------------------------------------------------------------ the plan, through the raw library
def _tab(vals):
    return (ctypes.c_void_p * len(vals))(*[v or None for v in vals])


def _layout(numel, p, g, m, v, e, wd=None, group=None):
    l = _lib.lib()
    n = len(numel)
    N = (ctypes.c_int64 * n)(*numel)
    tabs = [_tab(x) for x in (p, g, m, v, e)]
    l.pw_optim_plan_bytes.restype = ctypes.c_int64
    nbytes = l.pw_optim_plan_bytes(n, N, *tabs)
    assert nbytes > 0, l.pw_last_error()
    plan = (ctypes.c_int64 * (nbytes // 8 + 1))()
    plan[nbytes // 8] = 0x5a5a
    nc = ctypes.c_int64(-1)
    W = (ctypes.c_double * n)(*(wd or [0.01] * n))
    L = (ctypes.c_double * n)(*([1.0] * n))
    G = (ctypes.c_int32 * n)(*(group or [0] * n))
    rc = l.pw_optim_plan_layout(n, N, *tabs, W, L, G, plan, nbytes, ctypes.byref(nc))
    assert rc == 0, l.pw_last_error()
    assert plan[nbytes // 8] == 0x5a5a, 'the layout wrote past plan_bytes'
    return np.array(plan[:nbytes // 8], dtype=np.int64), nc.value, nbytes


def test_plan_layout_covers_every_element_once_and_flags_only_aligned_chunks():
    PW = _lib.PW_OPTIM
    H, RW, CW = PW['PW_OPTIM_HEADER_WORDS'], PW['PW_OPTIM_ROW_WORDS'], PW['PW_OPTIM_CHUNK_WORDS']
    rng = np.random.default_rng(3)
    numel, cols = [], [[], [], [], [], []]
    addr = 1 << 40
    for name, n, grp, kind in SPEC + [('empty', 0, 0, 'param'), ('allmis', 4 * CHUNK + 3, 0, 'allmis'), ('mis8', 77, 0, 'mis8')]:
        if kind == 'ibuffer':
            continue
        numel.append(n)
        for k in range(5):
            present = k in (0, 4) if kind in ('buffer', 'nograd') else (k < 4 or rng.random() < 0.7)
            a = addr
            addr += 16 * ((n + 3) // 4 + int(rng.integers(1, 5)))
            if kind == 'allmis' or (kind == 'view4' and k == 0):
                a += 4                                        # allmis: every address 4 bytes off -> a 3-element head, then vectors
            if kind == 'mis8' and k in (0, 1):
                a += 8
            cols[k].append(a if present else 0)
    plan, nc, nbytes = _layout(numel, *cols)
    n = len(numel)
    assert nbytes == 8 * (H + n * RW + nc * CW)
    assert plan[1] == n and plan[2] == nc and plan[3] == CHUNK and plan[4] == nbytes // 8
    assert plan[5] == sum(1 for i in range(n) if cols[1][i] and numel[i])
    rows = plan[H:H + n * RW].reshape(n, RW)
    for k in range(5):
        assert rows[:, k].tolist() == cols[k]
    assert rows[:, 5].tolist() == numel and (rows[:, 9] == [0 if g else 1 for g in cols[1]]).all()
    assert rows[0, 6] == np.float64(0.01).view(np.int64) and rows[0, 7] == np.float64(1.0).view(np.int64)
    chunks = plan[H + n * RW:].reshape(nc, CW)
    cover = [np.zeros(x, np.int32) for x in numel]
    vec_elems = 0
    for w0, start, cnt in chunks.tolist():
        r, vec = w0 & 0xffffffff, (w0 >> 32) & 1
        assert (w0 >> 33) == 0 and 0 <= r < n and 0 < cnt <= CHUNK and 0 <= start and start + cnt <= numel[r]
        cover[r][start:start + cnt] += 1
        if vec:
            vec_elems += cnt
            assert all((cols[k][r] + 4 * start) % 16 == 0 for k in range(5) if cols[k][r]), 'vector flag on a misaligned chunk'
    assert all((c == 1).all() for c in cover), 'an element is covered twice or not at all'
    # alignment is used where it exists: everything but the mixed-misalignment rows, the heads and nothing else is scalar
    scalar_rows = sum(x for x, k in zip(numel, [s[3] for s in SPEC if s[3] != 'ibuffer'] + ['param', 'allmis', 'mis8']) if k in ('view4', 'mis8'))
    assert sum(numel) - vec_elems == scalar_rows + 3
    assert _lib.lib().pw_optim_grid(nc) == min(nc, PW['PW_OPTIM_MAX_BLOCKS'])
    # near-equal pieces: the chunks of the largest tensor differ by at most 4 elements but for the last
    big = [c[2] for c in chunks.tolist() if (c[0] & 0xffffffff) == 9]
    assert len(big) == -(-numel[9] // CHUNK) and max(big[:-1]) - min(big[:-1]) == 0 and big[-1] <= big[0]


def test_optimizer_header_parses_like_the_main_header():
    """include/preworld_hip_optim.h (included by preworld_hip.h) under the rules tests/test_abi.py and tests/test_marshal_cpu.py hold
    the main header to: every pw_*( parses, every pointer parameter has a converter, the library exports every name"""
    import re
    text = open(_lib.OPTIM_HEADER_PATH).read()
    protos = _lib.parse_header(_lib.OPTIM_HEADER_PATH)
    declared = set(re.findall(r'\b(pw_\w+)\s*\(', text))
    assert declared == set(protos) == {'pw_optim_grid', 'pw_optim_plan_bytes', 'pw_optim_plan_layout', 'pw_optim_sqnorm', 'pw_optim_update'}
    assert '#include "preworld_hip_optim.h"' in open(_lib.HEADER_PATH).read()
    l = _lib.lib()
    code = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    for fn, (_, argtypes, argnames) in protos.items():
        assert hasattr(l, fn) and fn in _lib.protos()
        params = re.search(r'\b%s\s*\(([^;{]*?)\)\s*;' % fn, code).group(1).split(',')
        assert len(params) == len(argtypes) == len(argnames), fn
        for ptext, a, name in zip(params, argtypes, argnames):
            assert ('*' in ptext) == isinstance(a, _lib._PtrArg), (fn, name)
            if '*' in ptext:
                assert a.table == (ptext.count('*') == 2) and a.host == (name.endswith('_host') and not a.table), (fn, name)
        assert ctypes.c_void_p not in _lib._fns[fn].argtypes and argnames[-1] in ('stream', 'n_chunks', 'e', 'n_chunks_host'), fn


def test_entry_points_validate_before_any_hip_call():
    l = _lib.lib()
    l.pw_optim_plan_bytes.restype = ctypes.c_int64
    one = (ctypes.c_int64 * 1)(8)
    neg = (ctypes.c_int64 * 1)(-5)
    t = _tab([1 << 30])
    assert l.pw_optim_plan_bytes(-1, one, t, t, t, t, None) == -1 and b'pw_optim_plan_bytes' in l.pw_last_error()
    assert l.pw_optim_plan_bytes(1, neg, t, t, t, t, None) == -1 and b'pw_optim_plan_bytes' in l.pw_last_error()
    assert l.pw_optim_plan_bytes(1, one, t, t, None, None, None) == -1 and b'pw_optim_plan_bytes' in l.pw_last_error()
    W, G, nc = (ctypes.c_double * 1)(0.0), (ctypes.c_int32 * 1)(0), ctypes.c_int64(0)
    buf = (ctypes.c_int64 * 64)()
    assert l.pw_optim_plan_layout(1, one, t, t, t, t, None, W, W, G, None, 8 * 21, ctypes.byref(nc)) == -1
    assert b'pw_optim_plan_layout' in l.pw_last_error()
    assert l.pw_optim_plan_layout(1, neg, t, t, t, t, None, W, W, G, buf, 8 * 21, ctypes.byref(nc)) == -1
    assert b'pw_optim_plan_layout' in l.pw_last_error()
    assert l.pw_optim_plan_layout(1, one, t, t, t, t, None, W, W, G, buf, 8 * 20, ctypes.byref(nc)) == -1      # wrong size
    assert l.pw_optim_plan_layout(1, one, t, t, t, t, None, W, W, G, buf, 8 * 21, ctypes.byref(nc)) == 0 and nc.value == 1
    assert l.pw_optim_grid(-1) == -1 and b'pw_optim_grid' in l.pw_last_error()
    # the launches: a NULL plan, negative counts and a size that does not fit the counts are refused before any HIP call
    x = ctypes.c_void_p(1 << 30)
    assert l.pw_optim_sqnorm(None, 8 * 21, 1, 1, x, None) == -1 and b'pw_optim_sqnorm' in l.pw_last_error()
    assert l.pw_optim_sqnorm(x, 8 * 21, -1, 1, x, None) == -1 and b'pw_optim_sqnorm' in l.pw_last_error()
    assert l.pw_optim_sqnorm(x, 8 * 21, 1, -1, x, None) == -1
    assert l.pw_optim_sqnorm(x, 8 * 22, 1, 1, x, None) == -1
    assert l.pw_optim_sqnorm(x, 8 * 21, 1, 1, None, None) == -1 and b'slab' in l.pw_last_error()
    upd = lambda plan, nb, nr, nch, hyper, ng, slab, un, cl, ue, sk, ctr, eu, no: l.pw_optim_update(plan, nb, nr, nch, hyper, ng, slab, un, cl, ue, sk, ctr, eu, no, None)
    assert upd(None, 8 * 21, 1, 1, x, 1, x, 1, 1, 0, 0, x, None, x) == -1 and b'pw_optim_update' in l.pw_last_error()
    assert upd(x, 8 * 21, -1, 1, x, 1, x, 1, 1, 0, 0, x, None, x) == -1 and b'pw_optim_update' in l.pw_last_error()
    assert upd(x, 8 * 21, 1, 1, None, 1, x, 1, 1, 0, 0, x, None, x) == -1
    assert upd(x, 8 * 21, 1, 1, x, 65, x, 1, 1, 0, 0, x, None, x) == -1
    assert upd(x, 8 * 21, 1, 1, x, 1, None, 1, 1, 0, 0, x, None, x) == -1
    assert upd(x, 8 * 21, 1, 1, x, 1, None, 0, 1, 0, 0, x, None, None) == -1           # clipping without the norm
    assert upd(x, 8 * 21, 1, 1, x, 1, x, 1, 1, 1, 0, x, None, x) == -1 and b'ema_updates' in l.pw_last_error()


# ------------------------------------------------------------------------------------------ state dict
def test_state_dict_round_trip_through_torch_adamw():
    """FusedAdamW -> torch.optim.AdamW -> FusedAdamW; no kernel runs: the moments are built and filled on the host"""
    from preworld_amd.optim import FusedAdamW
    model, groups = R.build_model(SPEC, 'cpu')
    R.set_grads(model, R.grads(SPEC, 0))
    ours = FusedAdamW(groups, betas=R.BETAS, eps=R.EPS, grad_clip=dict(max_norm=5, norm_type=2))
    ours.init_state()
    gen = torch.Generator().manual_seed(1)
    for st in ours.state.values():
        st['exp_avg'].copy_(torch.randn(st['exp_avg'].shape, generator=gen))
        st['exp_avg_sq'].copy_(torch.rand(st['exp_avg_sq'].shape, generator=gen))
    ours._t_host = R.INIT_UPDATES
    sd = ours.state_dict()
    n_grad = sum(1 for s in SPEC if s[3] in ('param', 'view4'))
    assert len(sd['state']) == n_grad and all(set(st) == {'step', 'exp_avg', 'exp_avg_sq'} for st in sd['state'].values())

    model2, groups2 = R.build_model(SPEC, 'cpu', seed=1)
    ref = torch.optim.AdamW(groups2, foreach=False)
    ref.load_state_dict(sd)
    sd2 = ref.state_dict()
    assert sd2['param_groups'] == sd['param_groups'] and set(sd2['state']) == set(sd['state'])
    for i, st in sd['state'].items():
        assert float(sd2['state'][i]['step']) == R.INIT_UPDATES
        for k in ('exp_avg', 'exp_avg_sq'):
            assert torch.equal(sd2['state'][i][k], st[k]) and sd2['state'][i][k].shape == st[k].shape
    R.set_grads(model2, R.grads(SPEC, 0))
    ref.step()                                               # torch accepts the loaded state as its own
    assert all(float(st['step']) == R.INIT_UPDATES + 1 for st in ref.state.values())

    model3, groups3 = R.build_model(SPEC, 'cpu', seed=2)
    back = FusedAdamW(groups3)
    back.load_state_dict(ref.state_dict())
    assert back.step_count == R.INIT_UPDATES + 1
    sd3 = back.state_dict()
    assert sd3['param_groups'] == ref.state_dict()['param_groups'] and set(sd3['state']) == set(sd['state'])
    for i, st in ref.state_dict()['state'].items():
        assert float(sd3['state'][i]['step']) == R.INIT_UPDATES + 1 and sd3['state'][i]['step'].dtype == torch.float32
        for k in ('exp_avg', 'exp_avg_sq'):
            assert torch.equal(sd3['state'][i][k], st[k])
    # a reference checkpoint of an older torch keeps `step` as a Python int and fewer group keys: it loads too
    old = copy.deepcopy(ref.state_dict())
    for st in old['state'].values():
        st['step'] = 10560
    old['param_groups'] = [{k: g[k] for k in ('lr', 'betas', 'eps', 'weight_decay', 'amsgrad', 'params')} for g in old['param_groups']]
    back.load_state_dict(old)
    assert back.step_count == 10560
    # states that disagree on the step are refused: one counter serves all parameters
    old['state'][0]['step'] = 3
    with pytest.raises(ValueError):
        back.load_state_dict(old)


def test_constructor_refuses_what_the_kernels_do_not_do():
    from preworld_amd.optim import FusedAdamW
    p = [torch.nn.Parameter(torch.zeros(4))]
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(grad_clip=dict(max_norm=5, norm_type=1)),
               dict(grad_clip=dict(max_norm=5, norm_type='inf')), dict(grad_clip=dict(norm_type=2))):
        with pytest.raises(ValueError):
            FusedAdamW(p, **kw)
    with pytest.raises(ValueError):
        FusedAdamW([torch.nn.Parameter(torch.zeros(4, dtype=torch.bfloat16))])
    opt = FusedAdamW(p, grad_clip=dict(max_norm=5, norm_type=2))
    assert opt.max_norm == 5.0
    p[0].grad = torch.sparse_coo_tensor(torch.tensor([[1]]), torch.tensor([1.0]), (4,))
    with pytest.raises(ValueError):
        opt.step()
