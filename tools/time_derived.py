"""Timings behind profiles/derived_cache.md, one tree per process so that two checkouts can be run alternately:

    python tools/time_derived.py eager TREE C3|C1 [CALLS]     eager simple_test_from_lift on the device, ms per call
    python tools/time_derived.py hits TREE                    per-lookup hit cost of three cached operand sets, CPU tensors

TREE is the checkout whose preworld_amd is imported (its libpreworld_hip.so built), e.g. `.` or a worktree of another commit."""
import json
import os
import sys
import time
import timeit

mode, tree = sys.argv[1], os.path.abspath(sys.argv[2])
sys.path.insert(0, tree)
import torch                                              # noqa: E402
import preworld_amd                                       # noqa: E402
from preworld_amd import harness, modules as M, synth as S  # noqa: E402
assert os.path.dirname(os.path.dirname(os.path.abspath(preworld_amd.__file__))) == tree, preworld_amd.__file__


def eager(grid, calls):
    gc, cams = (S.GRID_CONFIG_C1, 1) if grid == 'C1' else (S.GRID_CONFIG_FULL, 6)
    net = harness.build_model(harness.model_cfg(gc), S.synth_state_dict(0), 'cuda:0')
    frames = harness.lifted_frames(1, cams, 'cuda:0')
    ego = torch.from_numpy(S.ego_state(1)).to('cuda:0')
    with torch.no_grad():
        for _ in range(30):
            net.simple_test_from_lift(frames, ego, n_steps=6)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            net.simple_test_from_lift(frames, ego, n_steps=6)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    return dict(grid=grid, calls=calls, ms_per_call=round(1e3 * dt / calls, 4))


def hits():
    bn = dict(type='BN3d')
    cm = M.ConvModule3d(32, 32, 3, padding=1, bias=False, norm_cfg=bn).eval()
    head = M.OccHead(32, 18, norm_cfg=bn).eval()
    blk = M.BasicBlock3D(32, 32, downsample=M.ConvModule3d(32, 32, 3, padding=1, bias=False, norm_cfg=bn, act_cfg=None)).eval()
    if hasattr(blk, 'pair_operands'):
        def pair():
            return blk.pair_operands('h2')
    else:                                   # trees before pair_operands: the lookup as BasicBlock3D._forward_cl_h2 spelled it
        c1, ds = blk.conv1, blk.downsample

        def pair():
            params = [c1.conv.weight, c1.bn.weight, c1.bn.bias, c1.bn.running_mean, c1.bn.running_var,
                      ds.conv.weight, ds.bn.weight, ds.bn.bias, ds.bn.running_mean, ds.bn.running_var]
            if not hasattr(blk, '_h2cache'):
                blk._h2cache = M._PackedCache()
            return blk._h2cache.get(params, lambda: 0)
    res = {}
    for name, fn in (('ConvModule3d.folded_h2', cm.folded_h2), ('OccHead._folded_h2', head._folded_h2), ('BasicBlock3D pair h2', pair)):
        fn()
        res[name] = round(min(timeit.repeat(fn, number=10000, repeat=5)) / 10000 * 1e6, 3)
    return dict(us_per_hit=res)


out = eager(sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 300) if mode == 'eager' else hits()
print(json.dumps(dict(tree=tree, **out)), flush=True)
