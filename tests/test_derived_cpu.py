"""modules.tensor_key / tensors_of / Derived and every site that keeps derived operands in one: what the key sees, which tensors
each site keys on, and that a change of ANY of them is followed by operands equal to a newly built module's.  CPU tensors, pure
torch packers, no kernel library."""
import gc
import weakref

import pytest
import torch
import torch.nn as nn

from preworld_amd import builder, modules as M
from _derived_util import factor, name_of, randomise, same, snapshot

BN = dict(type='BN3d')


# --------------------------------------------------------------------------------------------------------- Derived
class _Count:
    def __init__(self):
        self.n = 0

    def __call__(self):
        self.n += 1
        return self.n


def test_same_tensors_build_once_and_names_are_independent():
    lin, d, a, b = nn.Linear(3, 2), M.Derived(), _Count(), _Count()
    assert [d.get('a', (lin,), a) for _ in range(3)] == [1, 1, 1]
    assert d.get('b', (lin.weight, None), b) == 1 and d.get('b', (None, lin.weight), b) == 1          # None stands for nothing
    with torch.no_grad():
        lin.bias.add_(1)                                      # a source of 'a' only
    assert d.get('a', (lin,), a) == 2 and d.get('b', (lin.weight,), b) == 1
    assert (a.n, b.n) == (2, 1)


def test_build_runs_without_autograd():
    w = nn.Parameter(torch.ones(2))
    assert M.Derived().get('x', (w,), lambda: (w * 2).requires_grad) is False


def _swap_data(m):
    m.weight.data = torch.zeros(2, 3)


def _new_parameter(m):
    m.weight = nn.Parameter(m.weight.detach().clone())


@pytest.mark.parametrize('change', [
    lambda m: m.weight.detach().add_(1),
    lambda m: m.load_state_dict({k: v + 1 for k, v in m.state_dict().items()}),
    _swap_data,
    _new_parameter,
    lambda m: m.to(torch.float64),
], ids=['add_', 'load_state_dict', 'data=', 'new Parameter', 'to(float64)'])
def test_each_kind_of_change_rebuilds_exactly_once(change):
    lin, d, c = nn.Linear(3, 2), M.Derived(), _Count()
    d.get('w', (lin,), c)
    change(lin)
    assert [d.get('w', (lin,), c) for _ in range(3)] == [2, 2, 2]


def test_entry_keeps_its_sources_alive():
    d, t = M.Derived(), torch.ones(3)
    d.get('x', (t,), lambda: 0)
    r = weakref.ref(t)
    del t
    gc.collect()
    assert r() is not None                       # neither its id nor its address can be handed to another tensor under the entry
    d.get('x', (torch.ones(3),), lambda: 1)      # the entry is replaced: the old source goes with it
    gc.collect()
    assert r() is None


def test_tensor_key_sees_identity_version_storage_and_device():
    t = torch.ones(3)
    assert M.tensor_key([t]) == ((id(t), t._version, t.data_ptr(), t.device),)
    k0 = M.tensor_key([t])
    t.add_(1)
    k1 = M.tensor_key([t])
    t.data = torch.ones(3)
    assert len({k0, k1, M.tensor_key([t]), M.tensor_key([t.clone()])}) == 4


# --------------------------------------------------------------------------------------------------------- tensors_of
def _ids(ts):
    return [id(t) for t in ts]


def test_tensors_of_a_conv_module_is_its_key_set():
    cm = M.ConvModule3d(32, 32, 3, padding=1, bias=False, norm_cfg=BN)
    conv, bn = cm.conv, cm.bn
    want = [conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var]
    assert _ids(M.tensors_of(conv, bn)) == _ids(want) == _ids(M.tensors_of(cm))
    assert all(t is not bn.num_batches_tracked for t in M.tensors_of(cm))
    cb = M.ConvModule3d(32, 32, 3, padding=1, bias=True, norm_cfg=BN)
    assert _ids(M.tensors_of(cb.conv, cb.bn)) == _ids([cb.conv.weight, cb.conv.bias, cb.bn.weight, cb.bn.bias, cb.bn.running_mean,
                                                      cb.bn.running_var])
    plain = M.ConvModule3d(32, 32, 3, padding=1)             # bias='auto' without a norm: a bias, no bn
    assert _ids(M.tensors_of(plain.conv, None)) == _ids([plain.conv.weight, plain.conv.bias])
    t = torch.ones(1)
    assert _ids(M.tensors_of(None, t, None)) == [id(t)] and M.tensors_of() == []


def test_tensors_of_recurses_into_the_neck_conv():
    neck = M.LSSFPN3D(224, 32)
    cm = neck.conv
    assert _ids(M.tensors_of(cm)) == _ids([cm.conv.weight, cm.bn.weight, cm.bn.bias, cm.bn.running_mean, cm.bn.running_var])
    neck.operands('f32', 32, 64)
    (_, live, _), = neck._derived._entries.values()
    assert _ids(live) == _ids(M.tensors_of(cm))


# --------------------------------------------------------------------------------------------------------- the sweep
GRID = dict(x=[-4., 4., 1.], y=[-4., 4., 1.], z=[-1., 1., 1.], depth=[1., 5., 1.])


def _detector(kind):
    """the smallest detector that has the MLP heads (the encoder is only constructed)"""
    enc = dict(type='CustomResNet3D', numC_input=32, num_layer=[1], num_channels=[32], stride=[1], backbone_output_ids=[0])
    return builder.build(dict(
        type=kind, img_bev_encoder_backbone=enc, img_bev_encoder_neck=dict(type='LSSFPN3D', in_channels=224, out_channels=32),
        img_view_transformer=dict(type='LSSViewTransformer', grid_config=GRID, input_size=(32, 32), in_channels=8, out_channels=32,
                                  collapse_z=False)))


def _block(stride=1):
    return M.BasicBlock3D(32, 32, stride=stride, downsample=M.ConvModule3d(32, 32, 3, stride=stride, padding=1, bias=False,
                                                                          norm_cfg=BN, act_cfg=None))


def _mlps(net):
    return [m[i] for m in (net.density_mlp, net.semantic_mlp, net.color_mlp) for i in (0, 2)]


# (id, constructor, the tensors the site must key on -- stated here, not read from the cache --, {entry: call})
SITES = [
    ('conv+bn', lambda: M.ConvModule3d(32, 32, 3, padding=1, bias=False, norm_cfg=BN), lambda m: M.tensors_of(m),
     {k: (lambda m, k=k: m.operands(k)) for k in ('f32', 'wino', 'h2')}),
    ('conv+bias', lambda: M.ConvModule3d(32, 32, 3, padding=1), lambda m: [m.conv.weight, m.conv.bias],
     {'f32': lambda m: m.folded(), 'wino': lambda m: m.operands('wino'), 'h2': lambda m: m.folded_h2()}),
    ('block pair', _block, lambda m: M.tensors_of(m.conv1, m.downsample),
     {k: (lambda m, k=k: m.pair_operands(k)) for k in ('f32', 'wino', 'h2')}),
    ('neck', lambda: M.LSSFPN3D(224, 32), lambda m: M.tensors_of(m),
     {k: (lambda m, k=k: m.operands(k, 32, 64)) for k in ('f32', 'h2')}),
    ('occ head', lambda: M.OccHead(32, 18, norm_cfg=dict(type='BN3d')), lambda m: M.tensors_of(m.occ_convs, m.occ_pred_conv),
     {'f32': lambda m: [m._folded(t, w) for t in (False, True) for w in (False, True)],
      'h2': lambda m: [m._folded_h2(t) for t in (False, True)]}),
    ('downscale', lambda: M.DownScaleModule3DCustom(32), lambda m: [m.downscale1.weight, m.downscale2.weight, m.downscale3.weight],
     {'f32': lambda m: m._packed()}),
    ('predicter', lambda: _detector('BEVStereo4DOCC'), lambda m: M.tensors_of(m.predicter), {'pred': lambda m: m._predicter_packed()}),
    ('attributes', lambda: _detector('PreWorld'), lambda m: M.tensors_of(*_mlps(m)), {'attr': lambda m: m._attr_packed()}),
    ('forecast h2', lambda: _detector('PreWorld4DTraj'), lambda m: [m.fusion_head[0].weight, m.fusion_head[2].weight],
     {'fc_h2': lambda m: m._forecast_weights('fc_h2')}),
]


@pytest.mark.parametrize('make,sources,entries', [s[1:] for s in SITES], ids=[s[0] for s in SITES])
def test_every_source_invalidates_every_entry(make, sources, entries):
    """doubling (running_var: x4) each source tensor in turn, in place: every entry then returns what a newly constructed module
    with the same state returns, and not what it returned before"""
    mod = randomise(make()).eval()
    srcs = sources(mod)
    assert len(srcs) == len(set(_ids(srcs))) > 0
    before = {k: snapshot(call(mod)) for k, call in entries.items()}
    for k in entries:                                              # the site keys on exactly the stated tensors
        live = [t for name, (_, live, _) in mod._derived._entries.items() if (name if isinstance(name, str) else name[0]) == k for t in live]
        assert sorted(_ids(live)) == sorted(_ids(srcs)), k
    for t in srcs:
        with torch.no_grad():
            t.mul_(factor(name_of(mod, t)))
        fresh = make().eval()
        fresh.load_state_dict(mod.state_dict())
        for k, call in entries.items():
            after = call(mod)
            assert same(after, call(fresh)), (k, name_of(mod, t))
            assert not same(after, before[k]), (k, name_of(mod, t))
            before[k] = snapshot(after)


def test_fusion_head_bias_is_no_source_of_the_forecast_pack():
    """the biases reach the forecast kernels live: changing one must not repack the weights"""
    net = randomise(_detector('PreWorld4DTraj')).eval()
    packed = net._forecast_weights('fc_h2')
    with torch.no_grad():
        net.fusion_head[0].bias.mul_(2)
        net.fusion_head[2].bias.mul_(2)
    assert net._forecast_weights('fc_h2') is packed
    with torch.no_grad():
        net.fusion_head[2].weight.mul_(2)
    assert net._forecast_weights('fc_h2') is not packed
