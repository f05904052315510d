"""The reference's ShiftWindowMSA (mmdet3d/models/backbones/swin.py:244-513) from the qkv Linear's output to the proj Linear's input,
restated in float64 torch -- the yardstick pw_swin_window_attention (csrc/pw_swin_attn.hip, behind ops.swin_window_attention and
ShiftWindowMSA(attn_impl='hip')) answers to.

A plain composition, as the reference model does it: F.pad of the map, torch.roll, window partition, an img_mask filled through the
h_slices / w_slices loops (swin.py:422-444), table[relative_position_index] built with double_step_seq, explicit matmul and softmax,
window reverse, roll back, crop.  No per-token formula, nothing borrowed from the kernel or from preworld_amd/image_encoder.py.
Because the qkv Linear acts per token, padding the Linear's INPUT with zero tokens (what the reference does) is padding its output
with the Linear's bias: `pad_qkv`.

THE CASES are the smallest maps at which the kernel can still go wrong (see CASES).  Inputs are seeded; qkv and pad_qkv are float32
values (bf16 cases: rounded to bf16), so the float64 reference, the torch path and the kernel read the same numbers.

THE BOUND.  Per case 4 x FLOORS[case], relative to max |out64|: the floor is max |out32 - out64| / max |out64| of the EXISTING torch
path (IE.ShiftWindowMSA, proj = identity) on the CPU in float32 (bf16 cases: in bf16) fed the same qkv, measured by
tests/test_swin_attn_cpu.py, which asserts the torch path stays under each entry (rounded up to two digits) -- never taken from the
kernel.  The factor covers device expf, a different summation order and the matrix-core products.  No element is excluded.

Nothing in swin_attn_ref64 calls project code; `attention_module` (the harness that feeds a case's qkv through the project's module)
is kept apart at the bottom."""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

Case = collections.namedtuple('Case', 'B H W heads d ws shift bias_pad qkv_scale pad_scale dtype seed')


def _c(B, H, W, heads, d, ws, shift, bias_pad=True, qkv_scale=1.0, pad_scale=1.0, dtype='f32', seed=0):
    return Case(B, H, W, heads, d, ws, shift, bias_pad, qkv_scale, pad_scale, dtype, seed)


CASES = collections.OrderedDict([
    # the real tile (ws 12, d 32), padding on both axes: 13 x 25 -> 24 x 36, most of the last window row and column is padding
    ('tile_pad_s0', _c(2, 13, 25, 4, 32, 12, 0, seed=1)),
    ('tile_pad_s6', _c(2, 13, 25, 4, 32, 12, 6, seed=2)),
    ('tile_nopad_s0', _c(2, 24, 36, 4, 32, 12, 0, seed=3)),
    ('tile_nopad_s6', _c(2, 24, 36, 4, 32, 12, 6, seed=4)),
    # one window that holds all nine regions of the shift mask
    ('one_window_nine_regions', _c(1, 12, 12, 1, 32, 12, 6, seed=5)),
    # N = 49: no multiple of the 16-wide tile; qkv_bias=False (pad vector NULL)
    ('ws7_no_bias', _c(2, 7, 10, 2, 32, 7, 3, bias_pad=False, seed=6)),
    # narrow heads (zero-filled to the k-step), the toy Swin's window
    ('narrow_d8_s2', _c(2, 5, 9, 2, 8, 4, 2, seed=7)),
    ('narrow_d8_s0', _c(2, 5, 9, 2, 8, 4, 0, seed=8)),
    ('narrow_d16_s2', _c(2, 5, 9, 2, 16, 4, 2, seed=9)),
    # stage 3's real map: 32 heads, 16 x 44 -> 24 x 48
    ('many_heads_s6', _c(2, 16, 44, 32, 32, 12, 6, seed=10)),
    # logits reach +-60: the -100 offset and the max subtraction must hold
    ('peaked_s6', _c(2, 13, 25, 4, 32, 12, 6, qkv_scale=3.3, seed=11)),
    # padded tokens as keys and values: a large pad vector; dropping the padded keys changes the output by far more than the bound
    ('padded_keys_matter', _c(2, 13, 25, 4, 32, 12, 6, pad_scale=3.0, seed=12)),
    # dynamic range (fp32): the same draw scaled by powers of two
    ('range_2m12', _c(2, 13, 25, 4, 32, 12, 6, qkv_scale=2.0 ** -12, seed=2)),
    ('range_2p8', _c(2, 13, 25, 4, 32, 12, 6, qkv_scale=2.0 ** 8, seed=2)),
    ('bf16_tile_pad_s0', _c(2, 13, 25, 4, 32, 12, 0, dtype='bf16', seed=1)),
    ('bf16_tile_pad_s6', _c(2, 13, 25, 4, 32, 12, 6, dtype='bf16', seed=2)),
    ('bf16_tile_nopad_s0', _c(2, 24, 36, 4, 32, 12, 0, dtype='bf16', seed=3)),
    ('bf16_tile_nopad_s6', _c(2, 24, 36, 4, 32, 12, 6, dtype='bf16', seed=4)),
])

# max |out_torch - out64| / max |out64| of the torch path on the CPU (see the module docstring), rounded up to two digits
FLOORS = {
    'tile_pad_s0': 3.7e-07,                # measured 3.654e-07
    'tile_pad_s6': 4.0e-07,                # measured 3.971e-07
    'tile_nopad_s0': 4.2e-07,              # measured 4.128e-07
    'tile_nopad_s6': 3.1e-07,              # measured 3.068e-07
    'one_window_nine_regions': 3.1e-07,    # measured 3.080e-07
    'ws7_no_bias': 2.9e-07,                # measured 2.802e-07
    'narrow_d8_s2': 1.4e-07,               # measured 1.376e-07
    'narrow_d8_s0': 2.4e-07,               # measured 2.301e-07
    'narrow_d16_s2': 2.7e-07,              # measured 2.618e-07
    'many_heads_s6': 3.1e-07,              # measured 3.014e-07
    'peaked_s6': 2.0e-06,                  # measured 1.947e-06
    'padded_keys_matter': 4.9e-07,         # measured 4.877e-07
    'range_2m12': 4.5e-07,                 # measured 4.484e-07
    'range_2p8': 2.3e-07,                  # measured 2.215e-07
    'bf16_tile_pad_s0': 2.5e-03,           # measured 2.465e-03
    'bf16_tile_pad_s6': 3.3e-03,           # measured 3.243e-03
    'bf16_tile_nopad_s0': 2.8e-03,         # measured 2.790e-03
    'bf16_tile_nopad_s6': 2.9e-03,         # measured 2.867e-03
}

# the real-width model of the GPU test (embed_dims 128, depths [1, 1, 2, 1], ws 12, input 96 x 160): per output map,
# max |out32 - out64| / max |out64| of the torch model on the CPU, rounded up to two digits
MODEL_CFG = dict(embed_dims=128, depths=[1, 1, 2, 1], num_heads=[4, 8, 16, 32], window_size=12, patch_size=4, strides=(4, 2, 2, 2),
                 out_indices=(0, 1, 2, 3), drop_path_rate=0.0)
MODEL_FLOORS = (3.7e-07, 5.4e-07, 5.6e-07, 7.1e-07)      # measured 3.642e-07, 5.374e-07, 5.510e-07, 7.084e-07


def torch_dtype(case):
    return torch.bfloat16 if case.dtype == 'bf16' else torch.float32


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(qkv (B, H, W, 3C), pad_qkv (3C) or None, bias_table ((2 ws - 1)^2, heads), scale) of a case: float32 CPU tensors whose
    values are representable in the case's dtype"""
    c = CASES[name]
    rs = np.random.RandomState(1000 + c.seed)
    C = c.heads * c.d
    qkv = torch.from_numpy(rs.standard_normal((c.B, c.H, c.W, 3 * C)).astype(np.float32)) * c.qkv_scale
    pad = torch.from_numpy(rs.standard_normal(3 * C).astype(np.float32)) * (c.qkv_scale * c.pad_scale) if c.bias_pad else None
    table = torch.from_numpy((0.5 * rs.standard_normal(((2 * c.ws - 1) ** 2, c.heads))).astype(np.float32))
    if c.dtype == 'bf16':
        qkv = qkv.bfloat16().float()
        pad = None if pad is None else pad.bfloat16().float()
    return qkv, pad, table, float(c.d) ** -0.5


# ---------------------------------------------------------------------------------------------------------------- the yardstick
def _double_step_seq(step1, len1, step2, len2):
    seq1 = torch.arange(0, step1 * len1, step1)
    seq2 = torch.arange(0, step2 * len2, step2)
    return (seq1[:, None] + seq2[None, :]).reshape(1, -1)


def relative_position_index(ws):
    """WindowMSA.__init__ (swin.py:281-287)"""
    rel_index_coords = _double_step_seq(2 * ws - 1, ws, 1, ws)
    rel_position_index = rel_index_coords + rel_index_coords.T
    return rel_position_index.flip(1).contiguous()


def _window_partition(x, ws):
    B, H, W, C = x.shape
    x = x.view(B, H // ws, ws, W // ws, ws, C)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, ws, ws, C)


def _window_reverse(windows, H, W, ws):
    B = int(windows.shape[0] / (H * W / ws / ws))
    x = windows.view(B, H // ws, W // ws, ws, ws, -1)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(B, H, W, -1)


def swin_attn_ref64(qkv, pad_qkv, table, heads, ws, shift, scale, drop_padded_keys=False, return_logits=False):
    """qkv (B, H, W, 3C), pad_qkv (3C) or None, table ((2 ws - 1)^2, heads) -> (B, H, W, C), all float64.
    drop_padded_keys=True is NOT the reference: it removes the padded tokens from every softmax, to show on the reference alone
    that they matter (tests/test_swin_attn_cpu.py)."""
    qkv, table = qkv.double(), table.double()
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    pad_r = (ws - W % ws) % ws
    pad_b = (ws - H % ws) % ws
    # the reference pads the Linear's input with zero tokens: their qkv is the Linear's bias
    x = F.pad(qkv, (0, 0, 0, pad_r, 0, pad_b))
    real = F.pad(torch.ones(1, H, W, 1, dtype=torch.float64), (0, 0, 0, pad_r, 0, pad_b))
    if pad_qkv is not None:
        x = x + (1.0 - real) * pad_qkv.double().view(1, 1, 1, C3)
    Hp, Wp = x.shape[1], x.shape[2]
    if shift > 0:
        x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
        real = torch.roll(real, shifts=(-shift, -shift), dims=(1, 2))
        img_mask = torch.zeros((1, Hp, Wp, 1), dtype=torch.float64)
        h_slices = (slice(0, -ws), slice(-ws, -shift), slice(-shift, None))
        w_slices = (slice(0, -ws), slice(-ws, -shift), slice(-shift, None))
        cnt = 0
        for h in h_slices:
            for w in w_slices:
                img_mask[:, h, w, :] = cnt
                cnt += 1
        mask_windows = _window_partition(img_mask, ws).view(-1, ws * ws)
        attn_mask = mask_windows.unsqueeze(1) - mask_windows.unsqueeze(2)
        attn_mask = attn_mask.masked_fill(attn_mask != 0, float(-100.0)).masked_fill(attn_mask == 0, float(0.0))
    else:
        attn_mask = None
    N = ws * ws
    xw = _window_partition(x, ws).view(-1, N, C3)                       # nW*B, N, 3C
    Bw = xw.shape[0]
    t = xw.reshape(Bw, N, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    q, k, v = t[0], t[1], t[2]
    attn = (q * scale) @ k.transpose(-2, -1)
    bias = table[relative_position_index(ws).view(-1)].view(N, N, -1).permute(2, 0, 1).contiguous()
    attn = attn + bias.unsqueeze(0)
    if attn_mask is not None:
        nW = attn_mask.shape[0]
        attn = attn.view(Bw // nW, nW, heads, N, N) + attn_mask.unsqueeze(1).unsqueeze(0)
        attn = attn.view(-1, heads, N, N)
    if drop_padded_keys:
        realw = _window_partition(real.expand(B, Hp, Wp, 1).contiguous(), ws).view(Bw, 1, 1, N)
        attn = attn.masked_fill(realw == 0, float('-inf'))
    logits = attn
    attn = torch.softmax(attn, dim=-1)
    out = (attn @ v).transpose(1, 2).reshape(Bw, N, C)
    out = _window_reverse(out.view(-1, ws, ws, C), Hp, Wp, ws)
    if shift > 0:
        out = torch.roll(out, shifts=(shift, shift), dims=(1, 2))
    out = out[:, :H, :W, :].contiguous()
    return (out, logits) if return_logits else out


@functools.lru_cache(maxsize=None)
def reference(name):
    """the float64 output of a case, computed once and shared (do not modify)"""
    c = CASES[name]
    qkv, pad, table, scale = inputs(name)
    return swin_attn_ref64(qkv, pad, table, c.heads, c.ws, c.shift, scale)


def rel_err(out, ref):
    """max |out - ref| / max |ref| over every element"""
    return float((out.double() - ref).abs().max() / ref.abs().max())


# ------------------------------------------------------------------------------------ harness (project code from here on)
class QkvLookup(torch.nn.Module):
    """stands in for the qkv Linear of a ShiftWindowMSA so that the module computes on EXACTLY a case's qkv: the module's input
    carries token number + 1 in channel 0 (0 in the zero tokens the torch path pads with) and this looks the row up; row 0 is
    pad_qkv, what a Linear gives for a zero token.  `bias` is what the fused path takes for padded tokens."""

    def __init__(self, qkv, pad_qkv):
        super().__init__()
        C3 = qkv.shape[-1]
        row0 = torch.zeros(1, C3, dtype=qkv.dtype, device=qkv.device) if pad_qkv is None else pad_qkv.view(1, C3)
        self.register_buffer('rows', torch.cat([row0, qkv.reshape(-1, C3)]))
        self.register_buffer('bias', pad_qkv)

    def forward(self, x):
        return self.rows[x[..., 0].long()]


def attention_module(name, attn_impl, device='cpu', dtype=None):
    """(ShiftWindowMSA of the case with its qkv Linear replaced by the lookup and proj by the identity, its input, hw_shape);
    module(input, hw_shape).view(B, H, W, C) is the attention output on the case's qkv"""
    from preworld_amd import image_encoder as IE
    c = CASES[name]
    dtype = torch_dtype(c) if dtype is None else dtype
    qkv, pad, table, scale = inputs(name)
    C = c.heads * c.d
    m = IE.ShiftWindowMSA(C, c.heads, c.ws, c.shift, qkv_bias=c.bias_pad, attn_impl=attn_impl).eval()
    assert m.w_msa.scale == scale
    with torch.no_grad():
        m.w_msa.relative_position_bias_table.copy_(table)
    m.w_msa.qkv = QkvLookup(qkv.to(dtype), None if pad is None else pad.to(dtype))
    m.w_msa.proj = torch.nn.Identity()
    if dtype != torch.float32:
        m.w_msa.relative_position_bias_table.data = m.w_msa.relative_position_bias_table.data.to(dtype)
    m = m.to(device)
    x = torch.zeros(c.B, c.H * c.W, C, dtype=torch.float32, device=device)       # float32 whatever the case: it only carries indices
    x[..., 0] = torch.arange(1, c.B * c.H * c.W + 1, dtype=torch.float32, device=device).view(c.B, c.H * c.W)
    return m, x, (c.H, c.W)


def build_model(attn_impl='torch', dtype=torch.float32):
    """the real-width model of MODEL_CFG with seeded weights, and its input"""
    from preworld_amd import image_encoder as IE
    torch.manual_seed(77)
    net = IE.SwinTransformer(**MODEL_CFG, attn_impl=attn_impl).eval()
    g = torch.Generator().manual_seed(78)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if n.endswith('relative_position_bias_table'):
                p.copy_(0.2 * torch.randn(p.shape, generator=g))
    x = torch.randn(2, 3, 96, 160, generator=g)
    return net.to(dtype), x.to(dtype)
