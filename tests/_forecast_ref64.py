"""Float64 restatement of the forecast recursion and the attribute MLPs (preworld_temporal_traj.py:81-132, 231-250, 329-368), the
scale-free normaliser their kernels are judged by, a float32 restatement of the same step as the yardstick, and the operand regimes
of tests/test_gpu_forecast_ref64.py.  Plain numpy; no GPU, no reference source.

    e      = plan_head(ego)                       21 -> 256 ReLU -> 256 ReLU -> 32
    c1     = W1[:, 32:] e + b1
    v'     = v + W2 softplus_t20(W1a v + c1) + b2                    W1a = W1[:, :32]

ONE STEP AT A TIME: the reference for state k + 1 is step64(state k as the kernel produced it), so every error is local and the
recursion's own amplification (max|v| grows ~12x over 6 steps with the base weights) is in no bound.

NORMALISER.  A first-order forward bound of one step whose every operand and intermediate carries a relative error of one unit:

    Bd = |v| + |b2| + |W2| @ ( softplus(z) + sigmoid(z) (|W1a| @ |v| + |c1|) ),     z = W1a v + c1
    q  = max |got - ref| / (2^-24 Bd)

softplus(z) is the hidden value's own rounding, sigmoid(z) = softplus'(z) carries the error of z.  Nothing in it depends on the scale
of the features or on the kernel.  The attribute MLPs use the same form without the residual |v|; with the final density softplus
channels 0 and 1 add |out| (that softplus' own rounding)."""
import numpy as np

C, HID = 32, 128
EPS = 2.0 ** -24
F64, F32 = np.float64, np.float32


def softplus(z):
    """nn.Softplus(beta=1, threshold=20) in the precision of z"""
    z = np.asarray(z)
    return np.where(z > 20, z, np.log1p(np.exp(np.minimum(z, z.dtype.type(20)))))


def sigmoid(z):
    return 0.5 * (1.0 + np.tanh(0.5 * np.asarray(z, F64)))


def _c1b(c1, v):
    """c1 (128,) or per sample (S, 128) against v (..., 32) / (S, n, 32)"""
    return c1[:, None, :] if c1.ndim == 2 and v.ndim == 3 else c1


# ------------------------------------------------------------------------------------------ prologue
def plan_head64(ego, w0, b0, w2, b2, w4, b4):
    """ego (B, 21) -> (ego_feat (B, 32), the sum of |terms| of the last layer's dot products: the normaliser.  The two layers before it
    contribute through h2; what they cost is in the float32 restatement's figure, which the kernel is judged by)"""
    x, w0, b0, w2, b2, w4, b4 = [np.asarray(a, F64) for a in (ego, w0, b0, w2, b2, w4, b4)]
    h1 = np.maximum(x @ w0.T + b0, 0)
    h2 = np.maximum(h1 @ w2.T + b2, 0)
    e = h2 @ w4.T + b4
    return e, h2 @ np.abs(w4).T + np.abs(b4)


def _seq_dot32(x, w, b):
    """float32 multiply-add chain in index order, the order of the prologue kernel's loops (without its fused rounding)"""
    acc = np.broadcast_to(b.astype(F32), (x.shape[0], w.shape[0])).copy()
    for i in range(x.shape[1]):
        acc = (acc + (x[:, i:i + 1] * w[None, :, i]).astype(F32)).astype(F32)
    return acc


def plan_head32(ego, w0, b0, w2, b2, w4, b4):
    x, w0, b0, w2, b2, w4, b4 = [np.asarray(a, F32) for a in (ego, w0, b0, w2, b2, w4, b4)]
    h1 = np.maximum(_seq_dot32(x, w0, b0), 0)
    h2 = np.maximum(_seq_dot32(h1, w2, b2), 0)
    return _seq_dot32(h2, w4, b4)


def c1_64(e, W1, b1):
    """e (B, 32), W1 = fusion_head.0.weight (128, 64) -> (c1 (B, 128), sum of |terms|)"""
    e, We, b1 = np.asarray(e, F64), np.asarray(W1, F64)[:, C:], np.asarray(b1, F64)
    return e @ We.T + b1, np.abs(e) @ np.abs(We).T + np.abs(b1)


def c1_32(e, W1, b1):
    return _seq_dot32(np.asarray(e, F32), np.asarray(W1, F32)[:, C:], np.asarray(b1, F32))


def c1_to_c1p(c1):
    """natural order -> the accumulator order the kernels consume:  c1p[s][h][tile*16 + r] = c1[s][tile*32 + (r&3) + 8*(r>>2) + 4*h]"""
    h, tile, r = np.meshgrid(np.arange(2), np.arange(4), np.arange(16), indexing='ij')
    src = (tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * h).reshape(-1)
    return np.ascontiguousarray(np.asarray(c1)[..., src])


# ------------------------------------------------------------------------------------------ one recursion step
def step64(v, W1a, c1, W2, b2):
    v, W1a, c1, W2, b2 = [np.asarray(a, F64) for a in (v, W1a, c1, W2, b2)]
    z = v @ W1a.T + _c1b(c1, v)
    return v + softplus(z) @ W2.T + b2


def step_bound(v, W1a, c1, W2, b2):
    """Bd of the module docstring, in the units of v"""
    v, W1a, c1, W2, b2 = [np.asarray(a, F64) for a in (v, W1a, c1, W2, b2)]
    c = _c1b(c1, v)
    z = v @ W1a.T + c
    hid = softplus(z) + sigmoid(z) * (np.abs(v) @ np.abs(W1a).T + np.abs(c))
    return np.abs(v) + np.abs(b2) + hid @ np.abs(W2).T


def step32(v, W1a, c1, W2, b2):
    """the same step with float32 operands and results (numpy's float32 matmul, libm's float32 exp / log1p)"""
    v, W1a, c1, W2, b2 = [np.asarray(a, F32) for a in (v, W1a, c1, W2, b2)]
    z = (v @ W1a.T + _c1b(c1, v)).astype(F32)
    hs = softplus(z).astype(F32)
    out = ((hs @ W2.T).astype(F32) + b2).astype(F32) + v
    assert out.dtype == F32
    return out


def chain64(v0, W1a, c1, W2, b2, n_steps):
    out, v = [], np.asarray(v0, F64)
    for _ in range(n_steps):
        v = step64(v, W1a, c1, W2, b2)
        out.append(v)
    return np.stack(out)


def q_of(got, ref, bd):
    return float((np.abs(np.asarray(got, F64) - ref) / (EPS * bd)).max())


def step_q(got_next, got_prev, W1a, c1, W2, b2):
    """(q of the kernel's state k+1 given ITS state k, q32 of the float32 restatement on the same input)"""
    ref = step64(got_prev, W1a, c1, W2, b2)
    bd = step_bound(got_prev, W1a, c1, W2, b2)
    return q_of(got_next, ref, bd), q_of(step32(got_prev, W1a, c1, W2, b2), ref, bd)


def bound(q32):
    """q <= 2 q32 + 1: the factor 2 for a summation order and a softplus (MFMA, hardware exp2 / log2) other than numpy's BLAS and
    libm, the 1 for one rounding of the output"""
    return 2.0 * q32 + 1.0


# ------------------------------------------------------------------------------------------ attribute MLPs
def _attr_dense(blocks):
    """[(W1 (64,32), b1, W2 (n,64), b2)] -> block-diagonal (W1 (64k,32), b1, W2 (24,64k), b2 (24)); unused output rows are zero"""
    k = len(blocks)
    W1 = np.concatenate([np.asarray(b[0], F64) for b in blocks])
    b1 = np.concatenate([np.asarray(b[1], F64) for b in blocks])
    W2, b2, row = np.zeros((24, 64 * k)), np.zeros(24), 0
    for i, b in enumerate(blocks):
        n = np.asarray(b[2]).shape[0]
        W2[row:row + n, 64 * i:64 * i + 64] = b[2]
        b2[row:row + n] = b[3]
        row += n
    return W1, b1, W2, b2


def attr64(v, blocks, final_softplus):
    """v (n, 32) -> (packed grid (n, 24), its normaliser)"""
    W1, b1, W2, b2 = _attr_dense(blocks)
    v = np.asarray(v, F64)
    z = v @ W1.T + b1
    out = softplus(z) @ W2.T + b2
    bd = np.abs(b2) + (softplus(z) + sigmoid(z) * (np.abs(v) @ np.abs(W1).T + np.abs(b1))) @ np.abs(W2).T
    if final_softplus:
        out[:, :2] = softplus(out[:, :2])
        bd[:, :2] += np.abs(out[:, :2])
    return out, bd


def attr32(v, blocks, final_softplus):
    W1, b1, W2, b2 = [a.astype(F32) for a in _attr_dense(blocks)]
    v = np.asarray(v, F32)
    hs = softplus((v @ W1.T + b1).astype(F32)).astype(F32)
    out = ((hs @ W2.T).astype(F32) + b2).astype(F32)
    if final_softplus:
        out[:, :2] = softplus(out[:, :2])
    return out


def attr_blocks(seed, n_outs):
    rs = np.random.RandomState(seed)
    return [((rs.standard_normal((64, 32)) * 0.2).astype(F32), (rs.standard_normal(64) * 0.3).astype(F32),
             (rs.standard_normal((n, 64)) * 0.2).astype(F32), (rs.standard_normal(n) * 0.1).astype(F32)) for n in n_outs]


# ------------------------------------------------------------------------------------------ regimes
# (scale of W1, scale of W2, scale of c1, shift of c1) on the base draw W1 = 0.15 N, W2 = 0.08 N, b2 = 0.1 N, c1 = 0.5 N, v0 = N(0, 1)
REGIMES = {
    'base': (1.0, 1.0, 1.0, 0.0),
    'w1x8': (8.0, 1.0 / 8, 1.0, 0.0),
    'w1x64': (64.0, 1.0 / 64, 1.0, 0.0),           # row L1 norm of W1a about 330
    'w1/64': (1.0 / 64, 8.0, 1.0, 0.0),
    'ego_x64': (1.0, 1.0 / 16, 64.0, 0.0),         # |c1| up to about 100
    'dead': (1.0, 1.0, 1.0, -30.0),                # every hidden unit ~ 0
    'linear': (1.0, 1.0 / 16, 1.0, 30.0),          # most hidden units on the identity branch
    'mixed_samples': None,                         # three samples in ONE launch: the c1 of base, ego_x64 and dead
}
MIXED = ('base', 'ego_x64', 'dead')
SEED = 20
N_STEPS = 6


def draw(n_samples, n_vox, seed=SEED):
    """the base draw: dict of float32 arrays W1 (128, 64), W2 (32, 128), b2 (32), c1 (S, 128), v0 (S, n_vox, 32)"""
    rs = np.random.RandomState(seed)
    W1 = (rs.standard_normal((HID, 2 * C)) * 0.15).astype(F32)
    W2 = (rs.standard_normal((C, HID)) * 0.08).astype(F32)
    b2 = (rs.standard_normal(C) * 0.1).astype(F32)
    c1 = (rs.standard_normal((max(64, n_samples), HID)) * 0.5).astype(F32)[:n_samples]      # sample s has the same c1 at every S <= 64
    v0 = rs.standard_normal((n_samples, n_vox, C)).astype(F32)
    return dict(W1=W1, W2=W2, b2=b2, c1=np.ascontiguousarray(c1), v0=v0)


def regime(name, n_vox=105):
    """the operands of one regime at 2 x n_vox voxels (mixed_samples: 3 x n_vox), float32"""
    if name == 'mixed_samples':
        d = draw(3, n_vox)
        # W2 at ego_x64's 1/16, or the large-ego sample alone would grow past the regime conditions' factor 32
        s1, s2 = 1.0, 1.0 / 16
        d['c1'] = np.stack([(d['c1'][i] * F32(REGIMES[r][2]) + F32(REGIMES[r][3])).astype(F32) for i, r in enumerate(MIXED)])
    else:
        d = draw(2, n_vox)
        s1, s2, sc, sh = REGIMES[name]
        d['c1'] = (d['c1'] * F32(sc) + F32(sh)).astype(F32)
    d['W1'] = (d['W1'] * F32(s1)).astype(F32)
    d['W2'] = (d['W2'] * F32(s2)).astype(F32)
    d['W1a'] = np.ascontiguousarray(d['W1'][:, :C])
    return d


def regime_stats(d, n_steps=N_STEPS):
    """float64 facts about a regime: growth of the state, shares of hidden units beyond the softplus threshold on either side"""
    st = chain64(d['v0'], d['W1a'], d['c1'], d['W2'], d['b2'], n_steps)
    vs = np.concatenate([np.asarray(d['v0'], F64)[None], st])
    z = np.stack([vs[k] @ d['W1a'].astype(F64).T + d['c1'].astype(F64)[:, None, :] for k in range(n_steps)])
    per_sample = lambda f: [float(f(z[:, s])) for s in range(z.shape[1])]            # noqa: E731
    return dict(growth=float(np.abs(st[-1]).max() / np.abs(vs[0]).max()), hi=float((z > 20).mean()), lo=float((z < -20).mean()),
                hi_s=per_sample(lambda a: (a > 20).mean()), lo_s=per_sample(lambda a: (a < -20).mean()),
                v0_max=float(np.abs(vs[0]).max()), st_max=float(np.abs(st).max()), states=st)
