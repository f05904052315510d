"""What tests/test_derived_cpu.py and tests/test_gpu_derived.py share: parameters that make every operand depend on every
source, the perturbation that must invalidate them, and exact comparison of nested operand tuples."""
import torch


def randomise(module, seed=0):
    """every floating-point parameter and buffer away from its init (BatchNorm starts at mean 0 / bias 0, where doubling is a
    no-op): matrices ~ N(0, 0.2), vectors in [0.5, 1.5) (a positive running_var among them)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for t in list(module.parameters()) + list(module.buffers()):
            if t.is_floating_point():
                new = torch.randn(t.shape, generator=g) * 0.2 if t.dim() > 1 else torch.rand(t.shape, generator=g) + 0.5
                t.copy_(new.to(t.dtype))
    return module


def factor(name):
    """x2, exact in every format; x4 for a running variance, so that the folded scale moves by about 2 as well"""
    return 4.0 if name.endswith('running_var') else 2.0


def perturbed_state(module):
    """the module's state dict with every floating-point entry scaled by factor(its name): new tensors, the module untouched"""
    return {k: v.detach().clone() * factor(k) if v.is_floating_point() else v.detach().clone()
            for k, v in module.state_dict().items()}


def name_of(module, tensor):
    """state-dict name of a parameter / buffer object of `module`"""
    for k, v in list(module.named_parameters()) + list(module.named_buffers()):
        if v is tensor:
            return k
    raise KeyError('not a tensor of this module')


def same(a, b):
    """exact equality of operands: tensors by torch.equal (dtype and shape included), sequences element-wise, host numbers by =="""
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        return isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b


def snapshot(a):
    """a copy of nested operands that later in-place edits cannot reach (fp32 operands may be views of the parameters themselves)"""
    if isinstance(a, torch.Tensor):
        return a.detach().clone()
    return type(a)(snapshot(x) for x in a) if isinstance(a, (tuple, list)) else a
