"""GPU: k_render_rays (preworld_amd/csrc/pw_render.hip) in all twelve instantiations -- NP in {2, 4, 7} passes x {forward on an fp32
grid, forward on a bf16-stored grid, backward with float atomics, backward emitting entries for the sorted form} -- and the sorted
form's k_rb_* kernels, long-voxel path included, against the float64 yardstick of tests/_render_ref64.py on small anisotropic grids.

Bounds are 4 x FLOORS / GRAD_FLOORS (the error of the existing fp32 CPU checker against the same yardstick, asserted on the CPU by
test_render_ref64_cpu.py), never a number taken from a kernel.  Every call asserts the instantiation that ran (pw_last_kernel).
Each test prints what the kernel achieved as a fraction of its bound ('[pin]' lines)."""
import numpy as np
import pytest
import torch

import _render_ref64 as Y
from preworld_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PRE = 4.0                    # allowed multiple of the CPU checker's floor


def T(a):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(DEV)


def ran():
    return _lib.lib().pw_last_kernel().decode()


def n_passes(S):
    return 2 if S <= 128 else (4 if S <= 256 else 7)


def dev_inputs(name):
    x = Y.inputs(name)
    lay = Y.CASES[name]['layout']
    kw = dict(c_sigma=lay[1], c_sem=lay[2], n_sem=Y.N_SEM, c_rgb=lay[3])
    return x, T(x['rays_o']), T(x['rays_d']), T(x['t']), T(x['grid']), [float(v) for v in x['consts']], kw


def check_forward(name, tag, out, ref, bf16):
    """kernel outputs (want_debug) against the yardstick `ref`"""
    R, S = ref['mask'].shape
    assert ran() == 'k_render_rays<%d, 0, %s>' % (n_passes(S), 'true' if bf16 else 'false'), ran()
    mask, w, counts = out['mask'].cpu(), out['weights'].cpu().double(), out['counts'].cpu().long()
    tie, mtie = ref['tie'], ref['mask_tie']
    ok = ~tie
    assert not ((mask != ref['mask']).any(1) & ~mtie).any(), (name, tag, 'sample mask differs off the mask-tie rays')
    assert not (((w > 0) != ref['kept']).any(1) & ok).any(), (name, tag, 'kept set differs off the tie rays')
    assert torch.equal(counts[ok], ref['counts'][ok]), (name, tag)
    # the counts the kernel reports are the ones it wrote
    assert torch.equal(counts[:, 0], mask.sum(1)) and torch.equal(counts[:, 2], (w > 0).sum(1)), (name, tag)
    assert bool((counts[:, 2] <= counts[:, 1]).all() and (counts[:, 1] <= counts[:, 0]).all())
    assert all(bool(torch.isfinite(out[k]).all()) for k in Y.OUTPUTS)
    err = Y.output_errors({k: out[k] for k in Y.OUTPUTS}, ref)
    err['weights_elem'] = Y.weight_element_error(out['weights'], ref)
    frac = {k: err[k] / (PRE * f) for k, f in zip(Y.FLOOR_KEYS, Y.FLOORS[name])}
    print('[pin] %-16s %-9s %s  (%d tie rays)' % (name, tag, ' '.join('%s %.2e=%.0f%%' % (k, err[k], 100 * frac[k]) for k in Y.FLOOR_KEYS),
                                                 int(tie.sum())))
    # a near-tie ray may gain or lose one sample of weight <= 1.1e-3 (tests/test_gpu_render.py::_check_terminating_forward)
    near = tie & ~mtie
    if near.any():
        assert float((w[near] - ref['weights'][near]).abs().max()) <= 1.1e-3, (name, tag)
        for k, wide in (('depth', 1.1e-3 * 39), ('semantic', 5e-3), ('color', 5e-3)):
            assert float((out[k].cpu().double()[near] - ref[k][near]).abs().max()) <= wide + 2e-4 * float(ref[k].abs().max()), (name, tag, k)
    for k in Y.FLOOR_KEYS:
        assert frac[k] <= 1.0, (name, tag, k, err[k], 'bound', PRE * dict(zip(Y.FLOOR_KEYS, Y.FLOORS[name]))[k])
    return frac


def check_grad(name, tag, gg, ref):
    lay = Y.CASES[name]['layout']
    assert bool(torch.isfinite(gg).all()), (name, tag)
    used = torch.zeros(lay[0], dtype=torch.bool)
    for sl in Y.group_slices(lay).values():
        used[sl] = True
    assert float(gg.cpu()[..., ~used].abs().max()) == 0.0, (name, tag, 'a channel no attribute uses got a gradient')
    err = Y.grad_errors(gg, ref, lay)
    frac = {k: err[k] / (PRE * f) for k, f in zip(Y.GROUPS, Y.GRAD_FLOORS[name])}
    print('[pin] %-16s %-9s %s' % (name, tag, ' '.join('%s %.2e=%.0f%%' % (k, err[k], 100 * frac[k]) for k in Y.GROUPS)))
    for k in Y.GROUPS:
        assert frac[k] <= 1.0, (name, tag, k, err[k], 'bound', PRE * dict(zip(Y.GROUPS, Y.GRAD_FLOORS[name]))[k])


@pytest.mark.parametrize('name', list(Y.CASES))
def test_forward_fp32_and_bf16_storage(name):
    """<NP, 0, false> against the yardstick; <NP, 0, true> bit-equal to the fp32 kernel on the bf16-rounded grid and within the same
    bounds of the yardstick on that rounded grid"""
    x, ro, rd, t, grid, consts, kw = dev_inputs(name)
    out = ops.render_rays(ro, rd, t, grid, consts, want_debug=True, **kw)
    check_forward(name, 'fwd', out, Y.reference(name), False)
    g16 = grid.to(torch.bfloat16)
    out16 = ops.render_rays(ro, rd, t, g16, consts, want_debug=True, **kw)
    check_forward(name, 'fwd-bf16', out16, Y.reference(name, bf16=True), True)
    outr = ops.render_rays(ro, rd, t, g16.float(), consts, want_debug=True, **kw)
    for k in Y.OUTPUTS + ('counts', 'mask'):
        assert torch.equal(out16[k], outr[k]), (name, k)
    # without the debug outputs: the same four results
    plain = ops.render_rays(ro, rd, t, grid, consts, **kw)
    for k in ('depth', 'semantic', 'color', 'alphainv_last'):
        assert torch.equal(plain[k], out[k]), (name, k)


@pytest.mark.parametrize('name', list(Y.CASES))
def test_backward_atomics_and_sorted(name):
    """<NP, 1, false> and <NP, 2, false> + k_rb_*: both within 4 x GRAD_FLOORS of the yardstick's gradient (upstream gradients zeroed
    on tie rays); the sorted form bit-equal run to run, between its two entry bounds, and through ops.RenderRays"""
    x, ro, rd, t, grid, consts, kw = dev_inputs(name)
    ref = Y.reference(name)
    S = t.numel()
    cf = {k: T(v.float()) for k, v in ref['coef'].items()}                     # zeroed on tie rays by the yardstick
    up = (cf['depth'], cf['semantic'], cf['color'], cf['alphainv_last'], cf['weights'])
    ga = ops.render_rays_backward(ro, rd, t, grid, consts, *up, algo='atomics', **kw)
    assert ran() == 'k_render_rays<%d, 1, false>' % n_passes(S), ran()
    check_grad(name, 'atomics', ga, ref)
    gs = ops.render_rays_backward(ro, rd, t, grid, consts, *up, algo='sorted', max_entries=0, **kw)
    assert ran() == 'k_render_rays<%d, 2, false>' % n_passes(S), ran()
    check_grad(name, 'sorted', gs, ref)
    if Y.CASES[name].get('long_path'):
        assert int(ref['entries'].max()) > Y.RB_LONG
    assert torch.equal(ops.render_rays_backward(ro, rd, t, grid, consts, *up, algo='sorted', max_entries=0, **kw), gs), 'run to run'
    kept = int(ops.render_rays(ro, rd, t, grid, consts, want_debug=True, **kw)['counts'][:, 1].sum())
    assert torch.equal(ops.render_rays_backward(ro, rd, t, grid, consts, *up, algo='sorted', max_entries=8 * max(kept, 1), **kw), gs), 'entry bound'
    if Y.CASES[name]['layout'] == Y.DEFAULT_LAYOUT:
        gr = grid.clone().requires_grad_(True)
        outs = ops.RenderRays.apply(gr, ro, rd, t, consts)
        torch.autograd.backward(outs, list(up))
        assert torch.equal(gr.grad, gs), 'ops.RenderRays'


@pytest.mark.parametrize('name', ['c5_96_mixed', 's200_mixed'])            # NP 2 and NP 4
def test_backward_accumulates_into_grad_grid(name):
    x, ro, rd, t, grid, consts, kw = dev_inputs(name)
    ref = Y.reference(name)
    up = tuple(T(ref['coef'][k].float()) for k in Y.OUTPUTS)
    for algo in ('atomics', 'sorted'):
        a = ops.render_rays_backward(ro, rd, t, grid, consts, *up, algo=algo, **kw)
        base = torch.full_like(grid, 0.5)
        acc = ops.render_rays_backward(ro, rd, t, grid, consts, *up, algo=algo, grad_grid=base, **kw)
        assert acc.data_ptr() == base.data_ptr()
        # 0.5 + a rounds to half an ulp of [0.5, 1) = 3e-8 (larger |a| to its own ulp; atomics add in arrival order)
        err = float(((acc - 0.5) - a).abs().max())
        assert err <= 1e-6 * max(1.0, float(a.abs().max())), (name, algo, err)
        assert float((acc - 0.5).abs().max()) > 0


def test_refusals_raise_before_any_launch():
    x, ro, rd, t, grid, consts, kw = dev_inputs('c5_96_mixed')
    R = ro.shape[0]
    up = (torch.ones(R, device=DEV), torch.ones(R, 17, device=DEV), torch.ones(R, 3, device=DEV), torch.ones(R, device=DEV))
    ops.render_rays(ro, rd, t, grid, consts, **kw)
    sentinel = ran()
    gg = torch.full_like(grid, 7.0)

    def refused(fn):
        with pytest.raises(_lib.PreworldHipError):
            fn()
        torch.cuda.synchronize()
        assert ran() == sentinel and bool((gg == 7.0).all())

    for S_bad in (1, 449):
        tb = torch.linspace(0.01, 2.0, S_bad, device=DEV)
        refused(lambda: ops.render_rays(ro, rd, tb, grid, consts, want_debug=True, **kw))
        for algo in ('atomics', 'sorted'):
            refused(lambda: ops.render_rays_backward(ro, rd, tb, grid, consts, *up, algo=algo, grad_grid=gg, **kw))
    for algo in ('atomics', 'sorted'):
        refused(lambda: ops.render_rays_backward(ro, rd, t, grid.to(torch.bfloat16), consts, *up, algo=algo, grad_grid=gg, **kw))
        refused(lambda: ops.render_rays_backward(ro, rd, t, grid.permute(0, 2, 1, 3), consts, *up, algo=algo, grad_grid=gg, **kw))
    refused(lambda: ops.render_rays(ro, rd, t, grid.permute(0, 2, 1, 3), consts, **kw))
    refused(lambda: ops.render_rays(ro, rd, t, grid.double(), consts, **kw))


@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
@pytest.mark.parametrize('where', ['g_sem', 'g_depth'])
@pytest.mark.parametrize('name', ['c5_96_mixed', 'full417_mixed'])
def test_nonfinite_upstream_gradient_reaches_the_grid(name, where, bad):
    """one NaN / Inf in the upstream gradient of ONE ray that keeps samples: both backward forms return a gradient grid with a non-finite
    value (optim.py's skip_nonfinite reads it off the gradient norm), as the reference's autograd does; in the atomic form the voxels no
    sample of that ray touches equal the clean run"""
    x, ro, rd, t, grid, consts, kw = dev_inputs(name)
    ref = Y.reference(name)
    r = int(torch.argmax(ref['counts'][:, 2] * (~ref['tie'])))                # a non-tie ray that keeps the most samples
    assert int(ref['counts'][r, 2]) > 8
    up = {k: T(ref['coef'][k].float()) for k in Y.OUTPUTS}
    clean = ops.render_rays_backward(ro, rd, t, grid, consts, *[up[k] for k in Y.OUTPUTS], algo='atomics', **kw)
    if where == 'g_sem':
        up['semantic'][r, 3] = bad
    else:
        up['depth'][r] = bad
    args = [up[k] for k in Y.OUTPUTS]
    # voxels the ray's masked samples reach through a trilinear corner
    A = ref['A']
    rows = torch.nonzero(ref['sample_ray'] == r)[:, 0]
    touched = torch.zeros(A.shape[1], dtype=torch.bool)
    idx = A.indices()
    touched[idx[1][torch.isin(idx[0], rows)]] = True
    assert 0 < int(touched.sum()) < touched.numel()
    for algo in ('atomics', 'sorted'):
        gg = ops.render_rays_backward(ro, rd, t, grid, consts, *args, algo=algo, **kw)
        assert not bool(torch.isfinite(gg).all()), (name, where, bad, algo, 'the non-finite upstream gradient did not reach the gradient grid')
        if algo == 'atomics':
            a, b = gg.reshape(touched.numel(), -1).cpu()[~touched], clean.reshape(touched.numel(), -1).cpu()[~touched]
            assert bool(torch.isfinite(a).all())
            # the float atomics' arrival order is all that may differ (cf. the 2e-5 of the sorted-vs-atomics test in test_gpu_render.py)
            assert float((a - b).abs().max()) <= 2e-5 * float(b.abs().max()), (name, where, bad)
