"""The optimizer step of the reference's recipe on two HIP launches: FusedAdamW and ModelEMA.

The six configs train with `AdamW(lr=1e-4, weight_decay=1e-2)`, `grad_clip=dict(max_norm=5, norm_type=2)` and `MEGVIIEMAHook`
(mmdet3d/core/hook/ema.py).  From PyTorch that is `clip_grad_norm_` (a norm per tensor, a stack, a coefficient) + `AdamW.step()`
(a handful of foreach passes) + `ModelEMA.update` (two elementwise launches per state-dict entry).  Here `step()` enqueues
pw_optim_sqnorm and pw_optim_update (csrc/pw_optim.hip) over a device-resident plan and returns: no value is read back, so it
never synchronises and can be captured in a `torch.cuda.graph`.

Differences from the PyTorch composition, all deliberate:
  * gradients are NOT scaled in place: the clipping coefficient is applied as each gradient is read.  After `step()` `p.grad`
    still holds what backward wrote; the norm that was used is `optimizer.last_grad_norm` (a device scalar, mmcv's `grad_norm`).
  * one step counter for all parameters, on the device.  torch keeps one per parameter, so a parameter that first receives a
    gradient later than the others would lag there; here it shares the count.  `state_dict()` writes the shared count into
    every entry, `load_state_dict()` refuses a state whose entries disagree.
  * `skip_nonfinite=True` (off by default, the reference propagates a NaN norm): a step whose norm is not finite writes nothing
    and counts itself in `optimizer.skipped`.

The version contract: the kernels write through raw pointers, which autograd's version counters do not see, and the derived
operands of every conv (packed / folded / split-fp16 weights) are cached under `modules.tensor_key`, which holds `_version`.
So after every `step()` every tensor the launches may have written -- parameters, moments, shadow tensors -- has its version
advanced with `torch.autograd.graph.increment_version`; the next forward repacks.  tests/test_gpu_optim.py pins this.

Lifetime: the plan holds raw addresses.  This object keeps every tensor whose address is in the plan alive (`_Plan.keep`), and
compares the addresses at every `step()`: a parameter, gradient or shadow that moved gives a new plan (one pinned-memory copy).
"""
import copy

import torch

from . import _lib, ops

_f32 = torch.float32
_GLOBAL = _lib.PW_OPTIM['PW_OPTIM_HYPER_GLOBAL']
_GROUP = _lib.PW_OPTIM['PW_OPTIM_HYPER_GROUP']
_MAX_GROUPS = _lib.PW_OPTIM['PW_OPTIM_MAX_GROUPS']
_MAX_BLOCKS = _lib.PW_OPTIM['PW_OPTIM_MAX_BLOCKS']
_CTR = _lib.PW_OPTIM['PW_OPTIM_CTR_WORDS']


class _Plan:
    """rows -> the device plan; keeps the rows' tensors alive for as long as their addresses sit in it"""

    def __init__(self, p, g, m, v, e, wd, lr_mul, group, device):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('the optimizer plan changed during stream capture (a parameter, gradient or shadow moved): '
                               'run one eager step() first and keep zero_grad(set_to_none=False)')
        self.keep = (p, g, m, v, e)
        self.n_rows = len(p)
        self.host, self.n_chunks = ops.optim_plan(p, g, m, v, e, wd, lr_mul, group)
        self.dev = torch.empty(self.host.numel(), dtype=torch.int64, device=device)
        self.dev.copy_(self.host, non_blocking=True)
        self.written = [t for col in (m, v, e) for t in col if t is not None] + [t for t, gi in zip(p, g) if gi is not None]


class _DeviceState:
    """what both launches share besides the plan: hyper-parameters, counters, the slab of partial sums, the norm"""

    def __init__(self, device, n_groups):
        self.device = device
        self.hyper = torch.zeros(_GLOBAL + _GROUP * n_groups, dtype=torch.float64, device=device)
        self.hyper_vals = None
        self.ctr = torch.zeros(_CTR, dtype=torch.int64, device=device)
        self.slab = torch.zeros(_MAX_BLOCKS, dtype=torch.float64, device=device)
        self.norm = torch.zeros((), dtype=torch.float64, device=device)

    def upload(self, vals):
        """the hyper-parameters as the host sees them now; a copy is enqueued only when one changed (from pinned memory: no sync)"""
        if vals == self.hyper_vals:
            return
        if len(vals) != self.hyper.numel():
            self.hyper = torch.zeros(len(vals), dtype=torch.float64, device=self.device)
        self.staging = torch.tensor(vals, dtype=torch.float64).pin_memory()        # kept: a captured copy reads it at every replay
        self.hyper.copy_(self.staging, non_blocking=True)
        self.hyper_vals = vals


def _check_f32(t, what):
    if t.dtype is not _f32:
        raise ValueError('%s must be float32, got %s (bf16 / fp16 parameters are not supported)' % (what, t.dtype))
    if not t.is_contiguous():
        raise ValueError('%s must be contiguous' % what)


class ModelEMA:
    """The reference's ModelEMA (mmdet3d/core/hook/ema.py:17-59): a deep-copied eval-mode shadow of `model`; every floating entry of
    the state dict is blended as `e = e d + (1 - d) p`, d = decay (1 - exp(-updates / 2000)); integer entries (num_batches_tracked)
    stay as copied.  Passed as `ema=` to FusedAdamW the blend happens inside the optimizer's update launch, on the weights that
    launch has just written; `update()` on its own is the same kernel over EMA-only rows (one launch)."""

    def __init__(self, model, decay=0.9990, updates=0):
        self.ema = copy.deepcopy(model).eval()
        for q in self.ema.parameters():
            q.requires_grad_(False)
        self.decay = float(decay)
        self._bind(model)
        self._updates_host = int(updates)
        self._u = None
        self._own = None                 # (_DeviceState, _Plan, signature) of update() on its own

    def _bind(self, model):
        msd, esd = model.state_dict(keep_vars=True), self.ema.state_dict(keep_vars=True)
        if list(msd) != list(esd):
            raise ValueError('ModelEMA: the model and the shadow have different state-dict keys')
        self.model = model
        self.pairs = [(msd[k], esd[k]) for k in esd if esd[k].dtype.is_floating_point]

    def counter(self, device):
        """the device-resident update counter (int64[1])"""
        if self._u is None:
            self._u = torch.full((1,), self._updates_host, dtype=torch.int64, device=device)
        return self._u

    @property
    def updates(self):
        """number of blends so far; reads the device counter (synchronises)"""
        return self._updates_host if self._u is None else int(self._u.item())

    @updates.setter
    def updates(self, n):
        self._updates_host = int(n)
        if self._u is not None:
            self._u.fill_(int(n))

    def state_dict(self):
        return self.ema.state_dict()

    def checkpoint(self, epoch):
        """what MEGVIIEMAHook.save_checkpoint stores (ema.py:106-112)"""
        return {'epoch': epoch, 'state_dict': self.ema.state_dict(), 'updates': self.updates}

    def load_checkpoint(self, cpt):
        """MEGVIIEMAHook's resume (ema.py:93-97)"""
        self.ema.load_state_dict(cpt['state_dict'])
        self.updates = cpt['updates']

    def signature(self):
        return tuple((s.data_ptr(), e.data_ptr()) for s, e in self.pairs)

    @torch.no_grad()
    def update(self, model=None):
        """one blend of `model`'s state into the shadow, for use without FusedAdamW"""
        if model is not None and model is not self.model:
            self._bind(model)
            self._own = None
        if not self.pairs:
            return
        dev = self.pairs[0][1].device
        sig = self.signature()
        if self._own is None or self._own[2] != sig:
            for s, e in self.pairs:
                _check_f32(s, 'ModelEMA: a floating state-dict entry')
                _check_f32(e, 'ModelEMA: a shadow tensor')
            n = len(self.pairs)
            none = [None] * n
            plan = _Plan([s for s, _ in self.pairs], none, none, none, [e for _, e in self.pairs], [0.0] * n, [1.0] * n, [0] * n, dev)
            self._own = (self._own[0] if self._own else _DeviceState(dev, 0), plan, sig)
        st, plan, _ = self._own
        st.upload([0.0, self.decay] + [0.0] * (_GLOBAL - 2))
        ops.optim_update(plan.dev, plan.n_rows, plan.n_chunks, st.hyper, 0, None, st.ctr, self.counter(dev), None,
                         use_norm=False, clip=False, use_ema=True, skip_nonfinite=False)
        torch.autograd.graph.increment_version(plan.written)


class FusedAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW + clip_grad_norm_(max_norm, 2) + ModelEMA.update in two launches (one without clipping); see the module
    docstring.  `grad_clip` is the reference's optimizer_config dict, `dict(max_norm=5, norm_type=2)`; `ema` a ModelEMA of the model
    whose parameters these are.  param_groups carry torch.optim.AdamW's keys, so `state_dict()` loads into torch.optim.AdamW and back."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_clip=None, ema=None,
                 skip_nonfinite=False, amsgrad=False, maximize=False):
        if amsgrad or maximize:
            raise ValueError('FusedAdamW: amsgrad and maximize are not supported')
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= weight_decay or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError('FusedAdamW: lr, eps, weight_decay must be >= 0 and the betas in [0, 1)')
        self.max_norm = None
        if grad_clip is not None:
            extra = set(grad_clip) - {'max_norm', 'norm_type'}
            if extra or 'max_norm' not in grad_clip:
                raise ValueError('FusedAdamW: grad_clip takes max_norm and norm_type, got %s' % sorted(grad_clip))
            if float(grad_clip.get('norm_type', 2)) != 2.0:
                raise ValueError('FusedAdamW: only norm_type=2 is implemented, got %r' % (grad_clip['norm_type'],))
            self.max_norm = float(grad_clip['max_norm'])
        if ema is not None and not isinstance(ema, ModelEMA):
            raise ValueError('FusedAdamW: ema must be a preworld_amd.optim.ModelEMA')
        self.ema = ema
        self.skip_nonfinite = bool(skip_nonfinite)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True)
        self._dev = None                  # _DeviceState
        self._plan = None
        self._sig = None
        self._t_host = 0                  # the step count until the device counter exists
        super().__init__(params, defaults)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        g = self.param_groups[-1]
        if g.get('amsgrad') or g.get('maximize'):
            raise ValueError('FusedAdamW: amsgrad and maximize are not supported')
        for p in g['params']:
            if p.dtype is not _f32:
                raise ValueError('FusedAdamW: parameters must be float32, got %s' % p.dtype)
        if len(self.param_groups) > _MAX_GROUPS:
            raise ValueError('FusedAdamW: at most %d parameter groups' % _MAX_GROUPS)
        self._sig = None

    # ------------------------------------------------------------------ state
    def _moments(self, p):
        st = self.state[p]
        if 'exp_avg' not in st:
            st['exp_avg'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        return st['exp_avg'], st['exp_avg_sq']

    def init_state(self):
        """allocate the moments of every parameter that has a gradient now (step() does this itself; no kernel runs)"""
        for g in self.param_groups:
            for p in g['params']:
                if p.grad is not None:
                    self._moments(p)

    @property
    def step_count(self):
        """optimizer steps taken; reads the device counter (synchronises)"""
        return self._t_host if self._dev is None else int(self._dev.ctr[0].item())

    @property
    def last_grad_norm(self):
        """device scalar (float64): the global gradient L2 norm the last step() with clipping or skip_nonfinite computed"""
        return None if self._dev is None else self._dev.norm

    @property
    def skipped(self):
        """device scalar (int64): steps skipped for a non-finite norm (skip_nonfinite=True)"""
        return None if self._dev is None else self._dev.ctr[1]

    def state_dict(self):
        """torch.optim.AdamW's format: state[i] = {step, exp_avg, exp_avg_sq} + param_groups; `step` is the device counter"""
        t = float(self.step_count)
        for st in self.state.values():
            if 'exp_avg' in st:
                st['step'] = torch.tensor(t, dtype=_f32)
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        steps = set()
        for p, st in self.state.items():
            steps.add(float(st['step']))
            for k in ('exp_avg', 'exp_avg_sq'):
                st[k] = st[k].to(device=p.device, dtype=_f32).contiguous()
        for g in self.param_groups:
            if g.get('amsgrad') or g.get('maximize'):
                raise ValueError('FusedAdamW: amsgrad and maximize are not supported')
        if len(steps) > 1:
            raise ValueError('FusedAdamW keeps one step count for all parameters; the loaded state has %s' % sorted(steps))
        t = int(steps.pop()) if steps else 0
        self._t_host = t
        if self._dev is not None:
            self._dev.ctr[0] = t
        self._sig = None

    def zero_grad(self, set_to_none=False):
        """set_to_none=False by default: the gradients keep their addresses and the plan stays; True works and costs a new plan"""
        super().zero_grad(set_to_none=set_to_none)

    # ------------------------------------------------------------------ step
    def _signature(self):
        sig = []
        for g in self.param_groups:
            sig.append(g['weight_decay'])
            for p in g['params']:
                gr = p.grad
                if gr is None:
                    sig.append((p.data_ptr(), 0))
                else:
                    if gr.is_sparse:
                        raise ValueError('FusedAdamW does not support sparse gradients')
                    sig.append((p.data_ptr(), gr.data_ptr()))
        if self.ema is not None:
            sig.append(self.ema.signature())
        return sig

    def _replan(self, sig):
        shadow = {}
        if self.ema is not None:
            shadow = {id(s): (s, e) for s, e in self.ema.pairs}
        P, G, M, V, E, wd, mul, grp = [], [], [], [], [], [], [], []
        device = None
        for gi, g in enumerate(self.param_groups):
            for p in g['params']:
                if p.grad is None:
                    continue
                _check_f32(p, 'FusedAdamW: a parameter')
                _check_f32(p.grad, 'FusedAdamW: a gradient')
                if p.grad.shape != p.shape:
                    raise ValueError('FusedAdamW: a gradient has another shape than its parameter')
                m, v = self._moments(p)
                device = device or p.device
                P.append(p), G.append(p.grad), M.append(m), V.append(v), E.append(shadow.pop(id(p), (None, None))[1])
                wd.append(float(g['weight_decay'])), mul.append(1.0), grp.append(gi)
        for s, e in shadow.values():          # what the optimizer does not write and ModelEMA still blends: buffers, frozen parameters
            _check_f32(s, 'ModelEMA: a floating state-dict entry')
            P.append(s), G.append(None), M.append(None), V.append(None), E.append(e)
            wd.append(0.0), mul.append(1.0), grp.append(0)
            device = device or s.device
        for e in E:
            if e is not None:
                _check_f32(e, 'ModelEMA: a shadow tensor')
        if device is None:
            self._plan, self._sig = None, sig
            return
        if self._dev is None:
            self._dev = _DeviceState(device, len(self.param_groups))
            self._dev.ctr[0] = self._t_host
        self._plan = _Plan(P, G, M, V, E, wd, mul, grp, device)
        self._sig = sig

    def _hyper(self):
        vals = [self.max_norm if self.max_norm is not None else 0.0, self.ema.decay if self.ema is not None else 0.0]
        vals += [0.0] * (_GLOBAL - 2)
        for g in self.param_groups:
            vals += [float(g['lr']), float(g['betas'][0]), float(g['betas'][1]), float(g['eps'])] + [0.0] * (_GROUP - 4)
        return vals

    @torch.no_grad()
    def step(self, closure=None):
        """norm launch (with clipping or skip_nonfinite) + update launch.  Reads no device value: no synchronisation."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        sig = self._signature()
        if sig != self._sig:
            self._replan(sig)
        plan, st = self._plan, self._dev
        if plan is None:
            return loss
        st.upload(self._hyper())
        clip = self.max_norm is not None
        use_norm = clip or self.skip_nonfinite
        if use_norm:
            ops.optim_sqnorm(plan.dev, plan.n_rows, plan.n_chunks, st.slab)
        ops.optim_update(plan.dev, plan.n_rows, plan.n_chunks, st.hyper, len(self.param_groups), st.slab if use_norm else None, st.ctr,
                         self.ema.counter(st.device) if self.ema is not None else None, st.norm if use_norm else None,
                         use_norm=use_norm, clip=clip, use_ema=self.ema is not None, skip_nonfinite=self.skip_nonfinite)
        torch.autograd.graph.increment_version(plan.written)
        return loss

    def upload_hyper(self):
        """send lr / betas / eps / max_norm / decay as param_groups hold them now to the device tensor the kernels read (step() does
        this itself when one changed).  For a captured step(): set param_groups[i]['lr'], call this, replay."""
        if self._dev is not None:
            self._dev.upload(self._hyper())

    def mark_written(self):
        """advance the version of every tensor the launches write, as step() does itself.  For the caller of a captured step():
        a graph replay runs the kernels without this Python, so call this after every replay (before the next forward)."""
        if self._plan is not None:
            torch.autograd.graph.increment_version(self._plan.written)
