"""The optimizer step at the model's real parameter set: preworld_amd.optim.FusedAdamW (+ ModelEMA inside its update launch)
against what a user would write with PyTorch today,

    clip_grad_norm_(params, 5) ; torch.optim.AdamW(foreach=True).step() ; ModelEMA.update (core/hook/ema.py:56-59 restated)

Parameters: the C3 PreWorld4DTraj detector (full grid) plus the image side (Swin-B, FPN_LSS, DepthNet), seeded gradients.  Both
sides own a copy of the model, start from the same state and alternate in ONE process after warm-up; every step is timed with
device events.  Reported: median and spread (p90 - p10) of each, kernel launches per step of each, the fused step's algorithmic
bytes per second (40 B per optimised element: g read twice, p / m / v / e read and written; 12 B per EMA-only element) as a share of
the HBM rates in MI355X_MICROARCH.md, the fused step replayed from a torch.cuda.graph, and the largest difference between the two
sides' parameters after the first step.  Writes the section between the bench_optim markers of --out (profiles/optim_step.md).

    python tools/bench_optim.py [--steps 40] [--warmup 5] [--out profiles/optim_step.md] [--small]
"""
import argparse
import copy
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from preworld_amd import harness, image_encoder as IE, ops, synth as S      # noqa: E402
from preworld_amd.optim import FusedAdamW, ModelEMA                          # noqa: E402

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12          # MI355X_MICROARCH.md: HBM3E peak, measured float4 copy
BEGIN, END = '<!-- bench_optim:begin -->', '<!-- bench_optim:end -->'
MAX_NORM, DECAY, UPDATES = 5.0, 0.9990, 10560


def build(dev, small):
    torch.manual_seed(0)
    model = torch.nn.Module()
    model.net = harness.build_model(harness.model_cfg(S.GRID_CONFIG_C1 if small else S.GRID_CONFIG_FULL), S.synth_state_dict(0), dev)
    if not small:
        model.branch = IE.ImageBranch(**IE.preworld_image_cfg()).to(dev)
    with torch.no_grad():
        for p in model.parameters():
            if not p.is_contiguous():
                p.data = p.data.contiguous()
    return model


def seed_grads(model, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    for p in model.parameters():
        if p.grad is None:
            p.grad = torch.empty_like(p, memory_format=torch.contiguous_format)
        p.grad.copy_(torch.randn(p.shape, generator=g, device=p.device) * 1e-3)


def torch_ema_update(ema_model, model, updates):
    with torch.no_grad():
        d = DECAY * (1 - math.exp(-updates / 2000))
        msd = model.state_dict()
        for k, v in ema_model.state_dict().items():
            if v.dtype.is_floating_point:
                v *= d
                v += (1.0 - d) * msd[k].detach()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    s = sorted(ms)
    q = lambda f: s[min(len(s) - 1, int(round(f * (len(s) - 1))))]
    return dict(median=q(0.5), spread=q(0.9) - q(0.1), min=s[0], max=s[-1])


def kernel_launches(fn):
    """device kernels one call of fn enqueues, from torch.profiler's device events; None where the profiler reports none"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith('CUDA') and 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower())
        return n or None
    except Exception as ex:                                   # the number is an aid; the timings do not depend on it
        print('kernel count not available:', ex)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'optim_step.md'))
    ap.add_argument('--small', action='store_true', help='C1 grid, no image side: a rehearsal of the script, not a measurement')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_optim needs a GPU'
    dev = 'cuda:0'

    ours = build(dev, a.small)
    theirs = copy.deepcopy(ours)
    ema = ModelEMA(ours, decay=DECAY, updates=UPDATES)
    fused = FusedAdamW(ours.parameters(), lr=1e-4, weight_decay=1e-2, grad_clip=dict(max_norm=MAX_NORM, norm_type=2), ema=ema)
    their_ema = copy.deepcopy(theirs).eval()
    their_params = list(theirs.parameters())
    adamw = torch.optim.AdamW(their_params, lr=1e-4, weight_decay=1e-2, foreach=True)
    state = dict(updates=UPDATES)
    seed_grads(ours, 1)
    seed_grads(theirs, 1)
    saved = [p.grad.clone() for p in their_params]

    def step_fused():
        fused.step()

    def step_torch():
        # clip_grad_norm_ scales the gradients in place: restore them outside the timed call so every step clips the same values
        torch.nn.utils.clip_grad_norm_(their_params, MAX_NORM, norm_type=2, foreach=True)
        adamw.step()
        state['updates'] += 1
        torch_ema_update(their_ema, theirs, state['updates'])

    def restore():
        torch._foreach_copy_([p.grad for p in their_params], saved)

    n_opt = sum(p.numel() for p in ours.parameters())
    n_ema_only = sum(s.numel() for s, _ in ema.pairs) - n_opt
    n_tensors = len(list(ours.parameters()))

    # the first step of both from the same state: results must agree to fp32 rounding
    step_fused()
    step_torch()
    restore()
    torch.cuda.synchronize()
    worst = 0.0
    for p, q in zip(ours.parameters(), their_params):
        worst = max(worst, float((p.detach() - q.detach()).abs().max() / q.detach().abs().max().clamp_min(1e-30)))
    worst_e = 0.0
    for (k, x), y in zip(ema.state_dict().items(), their_ema.state_dict().values()):
        if x.is_floating_point() and x.numel():
            worst_e = max(worst_e, float((x - y).abs().max() / y.abs().max().clamp_min(1e-30)))

    for _ in range(a.warmup):
        step_fused()
        step_torch()
        restore()
    torch.cuda.synchronize()
    t_f, t_t = [], []
    for _ in range(a.steps):
        t_f.append(timed(step_fused))
        t_t.append(timed(step_torch))
        restore()
    sf, st = stats(t_f), stats(t_t)

    n0 = dict(ops.OPTIM_LAUNCHES)
    step_fused()
    fused_launches = sum(ops.OPTIM_LAUNCHES.values()) - sum(n0.values())
    fused_kernels = kernel_launches(step_fused)
    torch_kernels = kernel_launches(step_torch)
    restore()

    # the fused step replayed from a graph (default queue count, no runtime switches)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fused.step()
    for _ in range(a.warmup):
        graph.replay()
    torch.cuda.synchronize()
    t_g = [timed(graph.replay) for _ in range(a.steps)]
    sg = stats(t_g)
    fused.mark_written()

    nbytes = 40.0 * n_opt + 12.0 * n_ema_only
    rate = nbytes / (sf['median'] * 1e-3)
    rate_g = nbytes / (sg['median'] * 1e-3)
    margin = st['median'] - max(sf['spread'], st['spread'])
    verdict = 'holds' if sf['median'] <= margin else 'DOES NOT hold'
    size = 'C1 grid without the image side (--small: a rehearsal, not the measurement)' if a.small else \
        'C3 PreWorld4DTraj (full grid) + image side (Swin-B, FPN_LSS, DepthNet)'
    fmt = lambda s: '%.3f | %.3f | %.3f | %.3f' % (s['median'], s['spread'], s['min'], s['max'])
    lines = [
        BEGIN,
        '## Timing (tools/bench_optim.py, %s, %s)' % (getattr(torch.cuda.get_device_properties(0), 'gcnArchName', torch.cuda.get_device_name(0)), size),
        '',
        '%d parameter tensors, %.2f M optimised elements, %.3f M EMA-only elements (floating buffers); %d alternating steps after %d '
        'warm-up steps, device events around each step, one process.  Spread = p90 - p10.' % (n_tensors, n_opt / 1e6, n_ema_only / 1e6, a.steps, a.warmup),
        '',
        '| one optimizer step | median ms | spread ms | min ms | max ms | launches per step |',
        '|---|---|---|---|---|---|',
        '| FusedAdamW.step() (norm + update/EMA) | %s | %d through the wrappers (%s device kernels in torch.profiler) |' % (fmt(sf), fused_launches, fused_kernels if fused_kernels is not None else 'not measured'),
        '| clip_grad_norm_ + AdamW(foreach=True) + EMA loop | %s | %s device kernels in torch.profiler |' % (fmt(st), torch_kernels if torch_kernels is not None else 'not measured'),
        '| FusedAdamW.step() replayed from a torch.cuda.graph | %s | 2 kernel nodes |' % fmt(sg),
        '',
        'Acceptance: fused median <= PyTorch median - max(spreads) = %.3f - %.3f = %.3f ms: %s (fused median %.3f ms).' % (st['median'], max(sf['spread'], st['spread']), margin, verdict, sf['median']),
        '',
        'Algorithmic bytes of the fused step: 40 B x %.2f M + 12 B x %.3f M = %.1f MB.  Over the median: %.2f TB/s eager (%.0f %% of the 8.0 TB/s HBM3E '
        'peak, %.0f %% of the 6.29 TB/s float4-copy rate of MI355X_MICROARCH.md), %.2f TB/s replayed (%.0f %% / %.0f %%).  This is an '
        'algorithmic-bytes figure over the whole step (both kernels, launch gaps and host enqueue included), not a kernel\'s measured traffic; '
        'the second read of g may be served from the L2 / MALL for the small tensors.' % (
            n_opt / 1e6, n_ema_only / 1e6, nbytes / 1e6, rate / 1e12, 100 * rate / HBM_SPEC, 100 * rate / HBM_COPY, rate_g / 1e12,
            100 * rate_g / HBM_SPEC, 100 * rate_g / HBM_COPY),
        '',
        'Same results: after the first step from one state the two sides\' parameters differ by at most %.2e of a tensor\'s largest entry, '
        'the EMA shadows by %.2e (fp32 rounding is 6e-8; the PyTorch side forms the norm in float32 and contracts multiply-adds).' % (worst, worst_e),
        END,
    ]
    text = '\n'.join(lines) + '\n'
    print(text)
    old = open(a.out).read() if os.path.exists(a.out) else '# The optimizer step (FusedAdamW + ModelEMA)\n\n'
    if BEGIN in old and END in old:
        new = old[:old.index(BEGIN)] + text.rstrip('\n') + old[old.index(END) + len(END):]
    else:
        new = old + text
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(new)


if __name__ == '__main__':
    main()
