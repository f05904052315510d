"""GPU: the h2 residual epilogue of k_conv3d_h2 (EPI == 2: conv2(y) + identity, ReLU, as BasicBlock3D ends) against the generic
epilogue (EPI == 0) of the same kernel on the same inputs.

Every case runs ops.conv3d_h2 twice with out_h2 = (True, True) and relu0 = True: once with the residual as ops.H2 (the pipelined
EPI == 2 passes, which fetch the residual rows ahead of the pass that adds them) and once with the same residual converted by
ops.h2_to_f32 and passed as an fp32 tensor (EPI == 0, which loads each residual row right where it uses it).  Both evaluate
fmaf(acc, scale, bias) -> fmaf(residual, res_mul, v) -> clamp -> split with the residual and res_mul differing by exact powers of
two only, so the hi and lo planes and the recorded range maximum must agree bit for bit.  The residual is about 8x the conv output
with mixed signs: a wrong, stale or missing residual row cannot hide under rounding.

Shapes are the smallest that reach each path (tile = 4x8x8 voxels, 256 blocks on a 256-CU device):
  tiny      one partial tile, D < 4: only the rest path (no next stage to ride on)
  wr        32 -> 32 resident-weight kernel, 400 items on 256 blocks: passes ride on a next stage, last tile through the rest path
  inplace   the same with residual is out0 = channels 32..63 of a 64-channel buffer (row stride 64), pre_process_net's form
  c128      NT = 1, four input chunks (stages with nothing parked between the tiles), one item per block
  c64       NT = 1, two N-groups, 2-3 items per block
  nt2       676 tiles: two N-tiles per wave, eight passes per tile
  batch2    c64 with a batch of two"""
import functools

import pytest
import torch

from preworld_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

CASES = {  # name: (B, D, H, W, C, in place)
    'tiny': (1, 3, 5, 6, 32, False),
    'wr': (1, 16, 75, 75, 32, False),
    'inplace': (1, 16, 75, 75, 32, True),
    'c128': (1, 4, 50, 50, 128, False),
    'c64': (1, 8, 100, 100, 64, False),
    'nt2': (1, 16, 100, 100, 64, False),
    'batch2': (2, 8, 100, 100, 64, False),
}


def slot(e):
    s = torch.zeros(ops.RNG_ROW, dtype=torch.int32, device=DEV)
    s[0] = int(e)
    return s


def ran():
    return _lib.lib().pw_last_kernel().decode()


def bits(h):
    return h.buf.contiguous().view(torch.int32)


def expected_kernel(B, D, H, W, C, epi):
    """what pw_conv3d_h2's dispatcher picks (3x3x3 stride 1, C -> C)"""
    cus = ops.device_info()['cu_count']
    ntiles = C // 32
    nblk = B * ((D + 3) // 4) * ((H + 7) // 8) * ((W + 7) // 8)
    nt = 2 if ntiles % 2 == 0 and nblk * (ntiles // 2) >= 2 * cus else 1
    wr = nt == 1 and ntiles == 1 and epi > 0
    return 'k_conv3d_h2<%d, %d, %s>' % (nt, epi, 'true' if wr else 'false')


@functools.lru_cache(maxsize=None)
def operands(B, D, H, W, C):
    """seeded inputs of a shape, shared by the cases that use it and never written to"""
    g = torch.Generator(device='cpu').manual_seed(1000 * D + 10 * H + C + B)
    sigma = 0.05 * (27.0 * C) ** 0.5                       # standard deviation of the conv output
    x = torch.randn(B, D, H, W, C, generator=g)
    w = torch.randn(C, C, 3, 3, 3, generator=g) * 0.05
    scale = torch.rand(C, generator=g) + 0.5
    bias = torch.randn(C, generator=g)
    res = torch.randn(B, D, H, W, C, generator=g) * (8.0 * sigma)
    wpk, inv = ops.pack_conv_weight_h2(w.to(DEV))
    # exponents the way a calibrated RangeCtx leaves them: the largest magnitude in [2^12, 2^13) stored units.  5.5 sigma covers
    # the largest of these 10^4 .. 10^7 normal samples; the sum's deviation is sqrt(65) sigma
    e_res = ops.RangeCtx.ideal_exp(float(res.abs().max()))
    e_out = ops.RangeCtx.ideal_exp(5.5 * 65.0 ** 0.5 * sigma)
    return dict(x=ops.f32_to_h2(x.to(DEV)), wpk=wpk, scale=(scale.to(DEV) * inv).contiguous(), bias=bias.to(DEV), res=res.to(DEV),
                e_res=e_res, e_out=e_out)


@pytest.mark.parametrize('name', list(CASES))
def test_h2_residual_matches_generic_epilogue(name):
    B, D, H, W, C, inplace = CASES[name]
    P = operands(B, D, H, W, C)
    conv = lambda residual, out0: ops.conv3d_h2(P['x'], P['wpk'], P['scale'], P['bias'], residual=residual, relu0=True, out0=out0,
                                                out_h2=(True, True))
    with torch.no_grad():
        if inplace:
            # BasicBlock3D's form: the identity lives in the destination, here the upper half of a 64-channel buffer
            wide = torch.randn(B, D, H, W, 2 * C, device=DEV)
            keep = wide[..., :C].clone()
            res_h2 = ops.f32_to_h2(P['res'], out=ops.H2(wide[..., C:], slot(P['e_out'])))
            ops.slot_state(res_h2.rng)           # fold away what writing the identity recorded: the slot is compared as the
            res_h2.rng[1] = 0                    # conv leaves it
        else:
            res_h2 = ops.f32_to_h2(P['res'], out=ops.H2(torch.empty(B, D, H, W, C, device=DEV), slot(P['e_res'])))
        res_f32 = ops.h2_to_f32(res_h2)
        ref = conv(res_f32, ops.H2(torch.empty(B, D, H, W, C, device=DEV), slot(P['e_out'])))
        k_ref = ran()
        got = conv(res_h2, res_h2 if inplace else ops.H2(torch.empty(B, D, H, W, C, device=DEV), slot(P['e_out'])))
        k_got = ran()
    assert k_ref == expected_kernel(B, D, H, W, C, 0), (name, k_ref)
    assert k_got == expected_kernel(B, D, H, W, C, 2), (name, k_got)
    s_ref, s_got = ops.slot_state(ref.rng), ops.slot_state(got.rng)
    differ = int((bits(got) != bits(ref)).sum())
    print('[res] %-8s %s vs %s: %d of %d words differ, recorded maxima %r / %r' % (name, k_got, k_ref, differ, bits(ref).numel(),
                                                                                    s_got, s_ref))
    assert differ == 0, (name, 'EPI 2 output differs from the generic epilogue', differ)
    assert s_got == s_ref and s_ref[1] > 0.0, (name, 'range slot', s_got, s_ref)
    assert bool((bits(ref) != 0).any()), (name, 'all-zero output')
    if inplace:
        assert torch.equal(wide[..., :C].contiguous().view(torch.int32), keep.view(torch.int32)), (name, 'wrote outside its channels')
