"""The optimizer step on the device: preworld_amd.optim.FusedAdamW / ModelEMA (pw_optim_sqnorm + pw_optim_update) against the
float64 restatement of tests/_optim_ref64.py (proven against torch on the CPU in tests/test_optim_ref64_cpu.py) on the adversarial
tensor list: every path of the plan (vector chunks, scalar rows, heads and tails, a tensor of several chunks, more rows than a
by-value table held, EMA-only rows, parameters without gradient).

Tolerance: none is fixed in advance.  For every tensor a launch wrote,  q = max|got - ref64| / (2^-24 max|ref64|)  and q32, the same
figure of the float32 restatement (torch's own fp32 arithmetic) on the same inputs; asserted is  q <= 2 q32 + 1  (_optim_ref64.bound);
the norm scalar likewise.  Every step's reference starts from the kernel's own previous fp32 state, so no drift enters a bound.
Measured on an MI355X (profiles/optim_step.md, every test prints its own with -s): the largest q of any tensor in any case is 2.75
where the float32 form has 2.75 (bound 6.5); per case 1.50 ... 2.75 against q32 of 1.50 ... 2.75; the norm scalar q = 0.000 against
q32 up to 1.68.
"""
import copy

import numpy as np
import pytest
import torch

import _optim_ref64 as R
from _derived_util import randomise, same
from preworld_amd import _lib, modules as M, ops
from preworld_amd.optim import FusedAdamW, ModelEMA

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CHUNK = _lib.PW_OPTIM['PW_OPTIM_CHUNK']
SPEC = R.adversarial(CHUNK)
CLIP = dict(max_norm=R.MAX_NORM, norm_type=2)


def _make(clip=True, ema=True, skip=False, seed=0, updates=0):
    model, groups = R.build_model(SPEC, DEV, seed)
    e = ModelEMA(model, decay=R.DECAY, updates=updates) if ema else None
    opt = FusedAdamW(groups, betas=R.BETAS, eps=R.EPS, grad_clip=CLIP if clip else None, ema=e, skip_nonfinite=skip)
    return model, opt, e


def _moments(opt):
    return lambda p: (opt.state[p]['exp_avg'], opt.state[p]['exp_avg_sq']) if 'exp_avg' in opt.state[p] else None


def _snapshot(model, opt, ema):
    return R.rows_of(model, opt.param_groups, _moments(opt), ema.ema.state_dict() if ema is not None else None)


def _tensors(model, opt, ema, names, rows):
    """what the device holds now, in the rows' order: [(name, key, array)]"""
    sd = model.state_dict()
    esd = ema.ema.state_dict() if ema is not None else None
    out = []
    for name, r in zip(names, rows):
        if r['g'] is not None:
            st = opt.state[model.get_parameter(name)]
            out += [(name, 'p', sd[name]), (name, 'm', st['exp_avg']), (name, 'v', st['exp_avg_sq'])]
        if r['e'] is not None:
            out.append((name, 'e', esd[name]))
    return [(n, k, t.detach().cpu().numpy()) for n, k, t in out]


def _check(model, opt, ema, rows, names, t, u, clip=True, skip=False, what=''):
    """the device state after one step() from `rows` against both restatements; returns (t, u) after the step"""
    kw = dict(max_norm=R.MAX_NORM if clip else None, decay=R.DECAY if ema is not None else None, skip_nonfinite=skip)
    r64, t64, u64, sk, tot64 = R.step(rows, t, u, R.F64, **kw)
    r32, _, _, _, tot32 = R.step(rows, t, u, R.F32, **kw)
    got = _tensors(model, opt, ema, names, rows)
    by = {n: (a, b) for n, a, b in zip(names, r64, r32)}
    worst = (0.0, 0.0, '')
    for name, k, arr in got:
        q, q32 = R.q_of(arr, by[name][0][k]), R.q_of(by[name][1][k], by[name][0][k])
        worst = max(worst, (q, q32, name + '.' + k))
        assert q <= R.bound(q32), '%s %s.%s: q = %.3f, float32 form %.3f' % (what, name, k, q, q32)
    if clip or skip:
        qn, qn32 = R.q_of(opt.last_grad_norm.item(), tot64), R.q_of(float(tot32), tot64)
        print('%s norm %.6g: q = %.3f (float32 form %.3f)' % (what, tot64, qn, qn32))
        assert qn <= R.bound(qn32)
    print('%s worst q = %.3f (float32 form %.3f) at %s' % (what, *worst))
    assert opt.step_count == t64 and (ema is None or ema.updates == u64)
    return t64, u64


@pytest.mark.parametrize('norm', [3.0, 40.0, 0.0])
def test_one_step_norm_below_above_and_zero(norm):
    """coefficient exactly 1 (norm 3 < 5), clipping (40), and all-zero gradients (coefficient min(1, 5 / 1e-6) = 1, m = v = 0)"""
    model, opt, ema = _make()
    R.set_grads(model, R.grads(SPEC, 0, norm=norm))
    rows, names = _snapshot(model, opt, ema)
    before = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    opt.step()
    _check(model, opt, ema, rows, names, 0, 0, what='norm %g' % norm)
    # the gradients are not scaled in place (unlike clip_grad_norm_), and nothing touched what nobody owns
    assert all(torch.equal(model.get_parameter(n).grad, g) for n, g in before.items())
    assert model.get_parameter('frozen0').grad is None and int(model.num_batches_tracked) == 3 and int(ema.ema.num_batches_tracked) == 3
    assert model.get_parameter('view4').data_ptr() % 16 == 4


def test_steps_1_to_3_from_zero_state():
    model, opt, ema = _make()
    t = u = 0
    for s, norm in enumerate((40.0, 3.0, 7.0)):
        R.set_grads(model, R.grads(SPEC, s, norm=norm))
        rows, names = _snapshot(model, opt, ema)
        opt.step()
        t, u = _check(model, opt, ema, rows, names, t, u, what='step %d' % (s + 1))
    assert (t, u) == (3, 3)


def _load_10560(model, opt, ema):
    R.set_grads(model, R.grads(SPEC, 7, norm=9.0))
    opt.init_state()
    sd = opt.state_dict()
    gen = torch.Generator().manual_seed(5)
    for st in sd['state'].values():
        st['step'] = torch.tensor(float(R.INIT_UPDATES))
        st['exp_avg'] = torch.randn(st['exp_avg'].shape, generator=gen) * 0.05
        st['exp_avg_sq'] = torch.randn(st['exp_avg_sq'].shape, generator=gen) ** 2 * 0.01
    opt.load_state_dict(sd)


def test_one_step_from_a_loaded_state_at_step_10560():
    model, opt, ema = _make(updates=R.INIT_UPDATES)
    _load_10560(model, opt, ema)
    rows, names = _snapshot(model, opt, ema)
    opt.step()
    t, u = _check(model, opt, ema, rows, names, R.INIT_UPDATES, R.INIT_UPDATES, what='loaded')
    assert (t, u) == (R.INIT_UPDATES + 1, R.INIT_UPDATES + 1)
    assert float(opt.state_dict()['state'][0]['step']) == R.INIT_UPDATES + 1 and ema.checkpoint(3)['updates'] == R.INIT_UPDATES + 1
    assert set(ema.checkpoint(3)) == {'epoch', 'state_dict', 'updates'} and list(ema.state_dict()) == list(model.state_dict())


def test_clipping_off_runs_one_launch():
    model, opt, ema = _make(clip=False)
    R.set_grads(model, R.grads(SPEC, 0, norm=40.0))
    rows, names = _snapshot(model, opt, ema)
    n0 = dict(ops.OPTIM_LAUNCHES)
    opt.step()
    assert ops.OPTIM_LAUNCHES['sqnorm'] == n0['sqnorm'] and ops.OPTIM_LAUNCHES['update'] == n0['update'] + 1
    _check(model, opt, ema, rows, names, 0, 0, clip=False, what='no clip')
    model, opt, ema = _make(clip=True)
    R.set_grads(model, R.grads(SPEC, 0, norm=40.0))
    n0 = dict(ops.OPTIM_LAUNCHES)
    opt.step()
    assert ops.OPTIM_LAUNCHES['sqnorm'] == n0['sqnorm'] + 1 and ops.OPTIM_LAUNCHES['update'] == n0['update'] + 1


def test_without_ema():
    model, opt, _ = _make(ema=False)
    R.set_grads(model, R.grads(SPEC, 1, norm=40.0))
    rows, names = _snapshot(model, opt, None)
    buf = model.running_var.clone()
    opt.step()
    _check(model, opt, None, rows, names, 0, 0, what='no ema')
    assert torch.equal(model.running_var, buf)


def test_ema_only_update():
    """ModelEMA.update on its own: every floating entry blended, the model untouched, integer buffers left alone"""
    model, groups = R.build_model(SPEC, DEV)
    ema = ModelEMA(model, decay=R.DECAY, updates=R.INIT_UPDATES)
    with torch.no_grad():
        for t in model.state_dict().values():
            if t.is_floating_point():
                t.mul_(1.5).add_(0.25)
    msd = {k: v.clone() for k, v in model.state_dict().items()}
    u = R.INIT_UPDATES
    for _ in range(2):
        rows = [dict(p=msd[k].cpu().numpy(), g=None, m=None, v=None, e=v.cpu().numpy().copy()) for k, v in ema.state_dict().items()
                if v.is_floating_point()]
        names = [k for k, v in ema.state_dict().items() if v.is_floating_point()]
        vers = [v._version for v in ema.ema.state_dict(keep_vars=True).values() if v.is_floating_point()]
        n0 = dict(ops.OPTIM_LAUNCHES)
        ema.update(model)
        assert ops.OPTIM_LAUNCHES == dict(n0, update=n0['update'] + 1)
        r64, _, u, _, _ = R.step(rows, 0, u, R.F64, max_norm=None)
        r32 = R.step(rows, 0, u - 1, R.F32, max_norm=None)[0]
        esd = ema.state_dict()
        for name, a, b in zip(names, r64, r32):
            q, q32 = R.q_of(esd[name].cpu().numpy(), a['e']), R.q_of(b['e'], a['e'])
            assert q <= R.bound(q32), (name, q, q32)
        assert ema.updates == u
        assert all(v._version > v0 for v, v0 in zip((v for v in ema.ema.state_dict(keep_vars=True).values() if v.is_floating_point()), vers))
    assert all(torch.equal(v, msd[k]) for k, v in model.state_dict().items()) and int(ema.ema.num_batches_tracked) == 3


def _state(model, opt, ema):
    out = [t.clone() for t in model.state_dict().values()]
    for g in opt.param_groups:
        for p in g['params']:
            if 'exp_avg' in opt.state[p]:
                out += [opt.state[p]['exp_avg'].clone(), opt.state[p]['exp_avg_sq'].clone()]
    if ema is not None:
        out += [t.clone() for t in ema.state_dict().values()]
    return out


def test_run_to_run_bits():
    res = []
    for _ in range(2):
        model, opt, ema = _make()
        for s in range(2):
            R.set_grads(model, R.grads(SPEC, s, norm=40.0))
            opt.step()
        res.append(_state(model, opt, ema) + [opt.last_grad_norm.clone()])
    assert same(res[0], res[1])


def test_nonfinite_default_propagates_like_torch():
    """one Inf: the norm is Inf, the coefficient 5 / Inf = 0, 0 * Inf = NaN in that element, 0 in every other: p turns NaN exactly
    where torch's does (its element), every other element still decays"""
    model, opt, ema = _make()
    gr = R.grads(SPEC, 0, norm=40.0)
    gr['w08'][100] = np.inf
    R.set_grads(model, gr)
    ref_model, ref_groups = R.build_model(SPEC, DEV)
    R.set_grads(ref_model, gr)
    ref = torch.optim.AdamW(ref_groups, betas=R.BETAS, eps=R.EPS, foreach=False)
    torch.nn.utils.clip_grad_norm_([p for g in ref_groups for p in g['params']], R.MAX_NORM)
    ref.step()
    rows, names = _snapshot(model, opt, ema)
    opt.step()
    for (n, p), (_, q) in zip(model.named_parameters(), ref_model.named_parameters()):
        assert torch.equal(torch.isfinite(p), torch.isfinite(q)), n
    assert not torch.isfinite(model.w08[100]) and int(torch.isfinite(model.w08).sum()) == model.w08.numel() - 1
    assert torch.isinf(opt.last_grad_norm) and opt.step_count == 1 and int(opt.skipped) == 0
    _check(model, opt, ema, rows, names, 0, 0, what='inf')


def test_skip_nonfinite_changes_nothing_and_counts():
    model, opt, ema = _make(skip=True)
    R.set_grads(model, R.grads(SPEC, 0, norm=40.0))
    opt.step()                                               # a clean step first: non-trivial moments
    gr = R.grads(SPEC, 1, norm=40.0)
    gr['w08'][100] = np.inf
    R.set_grads(model, gr)
    before = _state(model, opt, ema)
    opt.step()
    assert same(_state(model, opt, ema), before), 'a skipped step wrote something'
    assert opt.step_count == 1 and ema.updates == 1 and int(opt.skipped) == 1 and torch.isinf(opt.last_grad_norm)
    R.set_grads(model, R.grads(SPEC, 2, norm=40.0))
    rows, names = _snapshot(model, opt, ema)
    opt.step()
    _check(model, opt, ema, rows, names, 1, 1, skip=True, what='after skip')
    assert int(opt.skipped) == 1


def test_lr_change_takes_effect_without_a_new_plan():
    model, opt, ema = _make()
    R.set_grads(model, R.grads(SPEC, 0, norm=40.0))
    opt.step()
    plan = opt._plan.dev
    ptr, ver = plan.data_ptr(), plan._version
    opt.param_groups[0]['lr'] = 3e-3
    R.set_grads(model, R.grads(SPEC, 1, norm=3.0))
    rows, names = _snapshot(model, opt, ema)
    assert rows[0]['lr'] == 3e-3
    opt.step()
    _check(model, opt, ema, rows, names, 1, 1, what='lr 3e-3')
    assert opt._plan.dev is plan and plan.data_ptr() == ptr and plan._version == ver
    # and it is the new lr that was used: the old one misses the bound by far
    old = R.step([dict(r, lr=1e-4) if r['g'] is not None and r['lr'] == 3e-3 else r for r in rows], 1, 1, R.F64)[0]
    assert R.q_of(model.w09.detach().cpu().numpy(), old[names.index('w09')]['p']) > 100


def test_replan_after_set_to_none():
    """new gradient tensors at new addresses give the same bits as gradients copied into stable buffers"""
    res = []
    for to_none in (False, True):
        model, opt, ema = _make()
        hold = []
        for s in range(2):
            if to_none:
                hold += [p.grad for p in model.parameters() if p.grad is not None]       # keep the old blocks: the new ones must differ
                opt.zero_grad(set_to_none=True)
                assert all(p.grad is None for p in model.parameters())
            else:
                opt.zero_grad()
            R.set_grads(model, R.grads(SPEC, s, norm=40.0))
            plan = opt._plan
            opt.step()
            assert s == 0 or (opt._plan is not plan) == to_none
        res.append(_state(model, opt, ema))
    assert same(res[0], res[1])


@pytest.mark.parametrize('precision', ['h2', 'f32'])
def test_version_contract_next_forward_uses_the_new_weights(precision, monkeypatch):
    """the kernels write parameters through raw pointers; the convs' packed operands are cached under modules.tensor_key, which
    holds _version.  Without the bump in FusedAdamW.step the second forward runs on the first forward's packed weights and equals
    it (tried by hand: with the bump removed this test fails at its first assertion, the second output being the stale one)."""
    monkeypatch.setenv('PW_PRECISION', precision)
    x = torch.from_numpy(np.random.RandomState(0).standard_normal((1, 4, 8, 8, 32)).astype(np.float32)).to(DEV)

    def run(mod):
        with torch.no_grad():
            out = ops.ranged(lambda: mod.forward_cl(x), ops.RangeCtx(DEV)) if M.precision() == 'h2' else mod.forward_cl(x)
        torch.cuda.synchronize()
        return out
    blk = randomise(M.BasicBlock3D(32, 32)).to(DEV).eval()
    ema = ModelEMA(blk)
    opt = FusedAdamW(blk.parameters(), lr=1e-2, grad_clip=CLIP, ema=ema)
    first, first_ema = run(blk), run(ema.ema)
    gen = torch.Generator().manual_seed(3)
    for p in blk.parameters():
        p.grad = torch.randn(p.shape, generator=gen).to(DEV)
    written = list(blk.parameters()) + [t for t in ema.ema.state_dict(keep_vars=True).values() if t.is_floating_point()]
    vers = [t._version for t in written]
    opt.step()
    second, second_ema = run(blk), run(ema.ema)
    fresh = M.BasicBlock3D(32, 32).to(DEV).eval()
    fresh.load_state_dict(blk.state_dict())
    assert same(second, run(fresh)) and not same(second, first)
    fresh.load_state_dict(ema.state_dict())
    assert same(second_ema, run(fresh)) and not same(second_ema, first_ema)
    assert all(t._version > v for t, v in zip(written, vers))
    assert all(st[k]._version > 0 for st in opt.state.values() for k in ('exp_avg', 'exp_avg_sq'))


def test_captured_step_replays_like_eager_steps():
    """one eager warm-up step, then step() captured in a torch.cuda.graph: three replays with fresh gradients copied into the same
    .grad buffers equal three eager steps bit for bit (default queue count, no runtime graph switches)"""
    res = []
    for captured in (False, True):
        model, opt, ema = _make()
        R.set_grads(model, R.grads(SPEC, 0, norm=40.0))
        opt.step()
        graph = None
        if captured:
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                opt.step()                                   # recorded, not run
        for s in range(1, 4):
            R.set_grads(model, R.grads(SPEC, s, norm=(3.0, 40.0)[s % 2]))
            if s == 3:                                       # a new lr reaches the recorded launches through the device tensor
                opt.param_groups[2]['lr'] = 5e-4
            if captured:
                opt.upload_hyper()
                graph.replay()
                opt.mark_written()
            else:
                opt.step()
        torch.cuda.synchronize()
        assert opt.step_count == 4 and ema.updates == 4
        res.append(_state(model, opt, ema) + [opt.last_grad_norm.clone()])
    assert same(res[0], res[1])


def test_interchange_with_torch_adamw_both_ways():
    """torch step -> our state -> fused step, and fused step -> torch state -> torch step: each within the bound of two float64 steps"""
    for ours_first in (False, True):
        model, groups = R.build_model(SPEC, DEV)
        a = (FusedAdamW if ours_first else torch.optim.AdamW)(groups, betas=R.BETAS, eps=R.EPS)
        params = [p for g in groups for p in g['params']]
        R.set_grads(model, R.grads(SPEC, 0, norm=3.0))
        rows0, names = R.rows_of(model, groups, lambda p: None, None)
        a.step()
        b = (torch.optim.AdamW if ours_first else FusedAdamW)(groups, betas=R.BETAS, eps=R.EPS)
        b.load_state_dict(a.state_dict())
        R.set_grads(model, R.grads(SPEC, 1, norm=3.0))
        g1 = {n: p.grad.detach().cpu().numpy().copy() for n, p in model.named_parameters() if p.grad is not None}
        b.step()
        assert all(float(st['step']) == 2 for st in b.state_dict()['state'].values())
        outs = []
        for dt in (R.F64, R.F32):
            r1 = R.step(rows0, 0, 0, dt, max_norm=None, decay=None)[0]
            r1 = [dict(r, g=g1[n].astype(dt)) for r, n in zip(r1, names)]
            outs.append(R.step(r1, 1, 0, dt, max_norm=None, decay=None)[0])
        sd = model.state_dict()
        for name, r64, r32 in zip(names, *outs):
            st = b.state[model.get_parameter(name)]
            for k, t in (('p', sd[name]), ('m', st['exp_avg']), ('v', st['exp_avg_sq'])):
                q, q32 = R.q_of(t.detach().cpu().numpy(), r64[k]), R.q_of(r32[k], r64[k])
                assert q <= R.bound(q32), (ours_first, name, k, q, q32)
