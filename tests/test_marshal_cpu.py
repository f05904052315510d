"""The argument converters of _lib.call: every pointer parameter of include/preworld_hip.h is checked against its declaration
(device / host memory, element type, contiguity) before the C function is entered.  No GPU: every call here is refused in Python,
or by the C side's own validation (NULL pointers)."""
import ast
import ctypes
import glob
import os
import re

import pytest
import torch

from preworld_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'preworld_hip.h')).read()


def _param(fn, name):
    _, argtypes, argnames = _lib.parse_header()[fn]
    return argtypes[argnames.index(name)]


def test_table_from_the_header_on_named_examples():
    assert _param('pw_conv3d_h2', 'x_rng').dtype == torch.int32
    assert _param('pw_voxel_loss_stats', 'stats').dtype == torch.float64
    assert _param('pw_voxel_loss_stats', 'target').dtype == torch.uint8
    assert _param('pw_alpha2weight', 'i_start').dtype == torch.int64
    lower = _param('pw_lss_lift_pool', 'lower3_host')
    assert lower.host and lower.dtype == torch.float32
    ws = _param('pw_lss_lift_pool', 'workspace')
    assert ws.elem == 'void' and ws.dtype is None and not ws.host
    src = _param('pw_copy_many', 'src')
    assert src.table and not _param('pw_conv3d_h2', 'x').table


def test_every_pointer_parameter_has_a_converter():
    protos = _lib.parse_header()
    n_ptr = 0
    for fn, (_, argtypes, argnames) in protos.items():
        decl = re.search(r'\b%s\s*\(([^;{]*?)\)\s*;' % fn, re.sub(r'/\*.*?\*/', ' ', HEADER, flags=re.S)).group(1)
        params = [] if decl.strip() in ('', 'void') else decl.split(',')
        assert len(params) == len(argtypes) == len(argnames), fn
        for text, a, name in zip(params, argtypes, argnames):
            assert ('*' in text) == isinstance(a, _lib._PtrArg), (fn, name)
            if '*' in text:
                n_ptr += 1
                assert (a.fn, a.name) == (fn, name) and a.table == (text.count('*') == 2)
                assert a.host == (name.endswith('_host') and not a.table)
    assert len(protos) == 100 and n_ptr == 570
    _lib.lib()
    for fn, (_, argtypes, _) in protos.items():          # what _lib.call goes through carries them; none is a bare c_void_p
        assert [type(a) for a in _lib._fns[fn].argtypes] == [type(a) for a in argtypes], fn
        assert ctypes.c_void_p not in _lib._fns[fn].argtypes, fn


def _refused(fn, *args):
    """the PreworldHipError of a call that must not enter the C function: pw_last_error() is as it was"""
    l = _lib.lib()
    before = l.pw_last_error()
    with pytest.raises(_lib.PreworldHipError) as e:
        _lib.call(fn, *args)
    assert l.pw_last_error() == before
    return str(e.value)


def test_host_tensor_for_a_device_parameter():
    l = _lib.lib()
    assert l.pw_lss_camera_matrices(0, None, None, None, None, None, None, None) == -1       # leaves a known pw_last_error()
    cpu = torch.zeros(1, 4, 4)
    msg = _refused('pw_lss_camera_matrices', 1, cpu, cpu, cpu, cpu, cpu, cpu, None)
    assert msg.startswith('pw_lss_camera_matrices: sensor2ego must be a CUDA(HIP) tensor'), msg
    assert b'pw_lss_camera_matrices' in l.pw_last_error()


def test_host_parameter_checks_dtype_and_place():
    f = [None] * 6
    ok3 = torch.zeros(3)
    msg = _refused('pw_lss_voxel_index', 1, 1, 1, 1, 1, *f, ok3.double(), ok3, 1, 1, 1, None, None, None)
    assert msg == 'pw_lss_voxel_index: lower3_host must be torch.float32, got torch.float64', msg
    # a float32 host tensor and a ctypes array both pass the converter: the C side then refuses the NULL device pointers
    for lower in (ok3, (ctypes.c_float * 3)(0, 0, 0)):
        with pytest.raises(_lib.PreworldHipError, match='failed'):
            _lib.call('pw_lss_voxel_index', 1, 1, 1, 1, 1, *f, lower, ok3, 1, 1, 1, None, None, None)


def test_none_reaches_the_c_side():
    with pytest.raises(_lib.PreworldHipError, match=r'pw_lss_camera_matrices failed \(-1\)'):
        _lib.call('pw_lss_camera_matrices', 0, None, None, None, None, None, None, None)


def test_bare_int_only_for_the_stream():
    msg = _refused('pw_lss_camera_matrices', 1, 0x1000, None, None, None, None, None, None)
    assert msg == 'pw_lss_camera_matrices: sensor2ego takes a tensor, got int', msg
    with pytest.raises(_lib.PreworldHipError, match='failed'):                       # stream = 0 passes, the NULL pointers do not
        _lib.call('pw_lss_camera_matrices', 1, None, None, None, None, None, None, 0)
    assert 'src takes a _lib.table of tensors' in _refused('pw_copy_many', torch.zeros(1), None, None, 1, None)
    assert 'src must be a CUDA(HIP) tensor' in _refused('pw_copy_many', _lib.table([torch.zeros(1)]), None, None, 1, None)


def test_constants_come_from_the_header():
    defines = dict(re.findall(r'^#define\s+(PW_\w+)\s+\(?(-?\d+)\)?', HEADER, re.M))
    assert defines and {k: int(v) for k, v in defines.items()} == _lib.PW
    assert ops.RNG_ROW == int(defines['PW_RNG_ROW']) == 1056
    from preworld_amd import losses
    assert losses._NS == int(defines['PW_VOXEL_LOSS_NSTATS'])
    assert ops.IMAGE_PREP_NPARAM == int(defines['PW_IMAGE_PREP_NPARAM'])
    assert ops.IMAGE_PREP_TILE == (int(defines['PW_IMAGE_PREP_TH']), int(defines['PW_IMAGE_PREP_TW']))


def test_no_address_is_taken_outside_lib():
    for path in sorted(glob.glob(os.path.join(ROOT, 'preworld_amd', '*.py'))):
        if os.path.basename(path) == '_lib.py':
            continue
        tree = ast.parse(open(path).read())
        for node in ast.walk(tree):
            if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
                assert node.name not in ('_p', '_ptr', '_chk', '_Ptr', '_cl'), (path, node.name)
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in ('call', 'call_size') \
                    and isinstance(node.func.value, ast.Name) and node.func.value.id == '_lib':
                for arg in node.args:
                    for sub in ast.walk(arg):
                        assert not (isinstance(sub, ast.Attribute) and sub.attr == 'data_ptr'), (path, node.lineno)
