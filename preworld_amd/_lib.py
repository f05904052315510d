"""ctypes binding of libpreworld_hip.so (the C ABI declared in include/preworld_hip.h).

The prototypes are parsed from the header itself, so the Python side cannot drift from
the C declarations.  There is NO fallback: if the library is missing or a call fails,
this raises -- the product path never routes through a CPU or PyTorch implementation.

Pointer arguments of `call` / `call_size` are the torch tensors themselves.  Each pointer parameter has a converter (`_PtrArg`)
built from its declaration: the tensor must live where the header says (device memory, or host memory for a `*_host` parameter),
hold the declared element type (`void*` takes any) and be contiguous, or the call raises PreworldHipError naming the entry point
and the parameter before the C function is entered.  `strided(t)` passes a view whose layout the wrapper has validated itself;
`table(tensors)` fills a `T* const*` parameter; None is NULL; `STREAM` is torch's current stream; ctypes objects (host arrays, byref
outputs, a stream handle) pass as given.

Lifetime rule: a tensor handed to `call` is referenced by the argument tuple until the launch has been enqueued, temporaries such
as `x.contiguous()` included, and after the enqueue a reuse of its block is stream-ordered behind the kernel.  So nothing outside
this file turns a tensor into an address.  (It used to: a wrapper took `data_ptr()` of a `.contiguous()` temporary, the temporary
was freed before the call, and the caching allocator handed the same block to the next temporary of the same call, whose copy
overwrote the first -- the four camera tensors of a B = 2 batch aliased one buffer.)

`lib()` is the raw library with plain `void*` prototypes: the tests of the C side's own argument validation call through it.
"""
import ctypes
import os
import re

import torch      # before the library is loaded, see lib()

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('PW_LIB_PATH') or os.path.join(_HERE, 'csrc', 'libpreworld_hip.so')      # PW_LIB_PATH: A/B builds (tools/build_variant.py)
HEADER_PATH = os.path.join(_HERE, '..', 'include', 'preworld_hip.h')
OPTIM_HEADER_PATH = os.path.join(_HERE, '..', 'include', 'preworld_hip_optim.h')      # the part preworld_hip.h includes (pw_optim_*)
RAYS_HEADER_PATH = os.path.join(_HERE, '..', 'include', 'preworld_hip_rays.h')        # ... and the ray-supervision part (pw_ray_*)

SWIN_HEADER_PATH = os.path.join(_HERE, '..', 'include', 'preworld_hip_swin.h')        # ... and the Swin window attention (pw_swin_*)
SWIN_BWD_HEADER_PATH = os.path.join(_HERE, '..', 'include', 'preworld_hip_swin_bwd.h')      # ... and its gradient
SWIN_LINEAR_HEADER_PATH = os.path.join(_HERE, '..', 'include', 'preworld_hip_swin_linear.h')      # ... and the Swin blocks' fused Linears
SWIN_LINEAR_BWD_HEADER_PATH = os.path.join(_HERE, '..', 'include', 'preworld_hip_swin_linear_bwd.h')      # ... and their gradient
CONV2D_HEADER_PATH = os.path.join(_HERE, '..', 'include', 'preworld_hip_conv2d.h')      # ... and the FPN_LSS / DepthNet convolutions (pw_conv2d*)

_CTYPES = {
    'int': ctypes.c_int, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64,
    'size_t': ctypes.c_size_t, 'float': ctypes.c_float, 'double': ctypes.c_double,
}
# element type of a pointer parameter -> the dtype its tensor must have (None: any)
_DTYPES = {
    'float': torch.float32, 'double': torch.float64, 'int32_t': torch.int32, 'int': torch.int32, 'int64_t': torch.int64,
    'uint8_t': torch.uint8, 'int8_t': torch.int8, 'char': torch.int8, 'uint32_t': torch.uint32, 'size_t': torch.uint64, 'void': None,
}
_CDATA = (ctypes._SimpleCData, ctypes.Array, ctypes._Pointer, type(ctypes.byref(ctypes.c_int())))


class PreworldHipError(RuntimeError):
    pass


class strided:
    """marks a tensor argument whose (non-contiguous) layout the wrapper has validated and passes to the kernel as strides"""
    __slots__ = ('t',)

    def __init__(self, t):
        self.t = t


# the `stream` argument: torch's current HIP stream, looked up when the call is made -- `stream` is the last parameter, so a call
# that is refused for one of its tensors never touches the device
STREAM = object()


class table:
    """the argument of a pointer-table parameter (`T* const*`): a list of tensors, None entries are NULL"""
    __slots__ = ('tensors',)

    def __init__(self, tensors):
        self.tensors = list(tensors)


class _PtrArg:
    """argtypes entry of one pointer parameter: ctypes calls from_param on every argument.  from_param is one closure per parameter
    over what the declaration says, with the passing case of a tensor first (an eager training step converts some 5 000 pointers)"""
    __slots__ = ('fn', 'name', 'elem', 'dtype', 'host', 'table', 'from_param')

    def __init__(self, fn, name, elem, is_table):
        self.fn, self.name, self.elem, self.dtype = fn, name, elem, _DTYPES[elem]
        self.host, self.table = name.endswith('_host') and not is_table, is_table        # a table's ENTRIES are device pointers
        self.from_param = self._converter()

    def _converter(self):
        dtype, host, is_table, is_stream = self.dtype, self.host, self.table, self.name == 'stream'
        Tensor, c_void_p = torch.Tensor, ctypes.c_void_p

        def fail(what):
            raise PreworldHipError('%s: %s %s' % (self.fn, self.name, what))

        def check(t, contiguous=True):
            if t.is_cuda is host:
                fail('must be in host memory' if host else 'must be a CUDA(HIP) tensor')
            if dtype is not None and t.dtype is not dtype:
                fail('must be %s, got %s' % (dtype, t.dtype))
            if contiguous and not t.is_contiguous():
                fail('must be contiguous')

        def from_param(v):
            if v is None:
                return None
            if isinstance(v, Tensor) and not is_table:
                if v.is_cuda is host or (v.dtype is not dtype and dtype is not None) or not v.is_contiguous():
                    check(v)                    # raises, saying which
                return c_void_p(v.data_ptr())
            if type(v) is strided and not is_table:
                check(v.t, contiguous=False)
                return c_void_p(v.t.data_ptr())
            if type(v) is table and is_table:
                for t in v.tensors:
                    if t is not None:
                        check(t)
                return (c_void_p * len(v.tensors))(*[None if t is None else t.data_ptr() for t in v.tensors])
            if isinstance(v, _CDATA):
                return v
            if is_stream and type(v) is int:
                return c_void_p(v)
            fail('takes %s, got %s' % ('a _lib.table of tensors' if is_table else 'a tensor', type(v).__name__))

        def stream_from_param(v):
            return c_void_p(torch.cuda.current_stream().cuda_stream) if v is STREAM else from_param(v)
        return stream_from_param if is_stream else from_param


def _parse(path):
    src = open(path).read()
    src = re.sub(r'/\*.*?\*/', ' ', src, flags=re.S)
    src = re.sub(r'//[^\n]*', ' ', src)
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r'^[ \t]*#[ \t]*define[ \t]+(PW_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$', src, re.M)}
    src = re.sub(r'^[ \t]*#[^\n]*', ' ', src, flags=re.M)          # preprocessor lines
    protos = {}
    for m in re.finditer(r'([A-Za-z_][\w\s\*]*?)\b(pw_\w+)\s*\(([^;{]*?)\)\s*;', src):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        if ret.endswith('*'):
            restype = ctypes.c_char_p if 'char' in ret else ctypes.c_void_p
        else:
            restype = _CTYPES[ret.replace('const', '').strip()]
        argtypes, argnames = [], []
        if args and args != 'void':
            for a in args.split(','):
                toks = ' '.join(a.replace('*', ' * ').split()).replace('const ', '').split()      # 'const T* const* x' -> T * * x
                argnames.append(toks[-1])
                argtypes.append(_PtrArg(name, toks[-1], toks[0], toks.count('*') == 2) if '*' in toks else _CTYPES[toks[0]])
        protos[name] = (restype, argtypes, argnames)
    return protos, consts


def parse_header(path=HEADER_PATH):
    """Return {name: (restype, [argtypes], [argnames])} for every pw_* declaration; a pointer's argtype is its _PtrArg."""
    return _parse(path)[0]


_protos, PW = _parse(HEADER_PATH)       # PW: the header's integer `#define PW_*` values by name
_optim_protos, PW_OPTIM = _parse(OPTIM_HEADER_PATH)        # ... and those of the optimizer part (PW_OPTIM_*)
_protos.update(_optim_protos)
_rays_protos, PW_RAYS = _parse(RAYS_HEADER_PATH)           # ... and those of the ray-supervision part (PW_RAY_*)
_protos.update(_rays_protos)
_swin_protos, PW_SWIN = _parse(SWIN_HEADER_PATH)           # ... and those of the Swin window attention (PW_SWIN_*)
_protos.update(_swin_protos)
_swin_bwd_protos, PW_SWIN_BWD = _parse(SWIN_BWD_HEADER_PATH)      # ... and those of its gradient (PW_SWIN_BWD_*)
_protos.update(_swin_bwd_protos)
_swin_linear_protos, PW_SWIN_LINEAR = _parse(SWIN_LINEAR_HEADER_PATH)      # ... and those of the fused Linears (PW_SWIN_LINEAR_*)
_protos.update(_swin_linear_protos)
_swin_linear_bwd_protos, PW_SWIN_LINEAR_BWD = _parse(SWIN_LINEAR_BWD_HEADER_PATH)      # ... and those of their gradient (PW_SWIN_LINEAR_BWD_*)
_protos.update(_swin_linear_bwd_protos)
_conv2d_protos, PW_CONV2D = _parse(CONV2D_HEADER_PATH)     # ... and those of the image side's fused convolutions (PW_CONV2D_*)
_protos.update(_conv2d_protos)
_lib = None
_fns = {}


def lib():
    """Load the HIP library (once).  Raises PreworldHipError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PreworldHipError(
            'libpreworld_hip.so is missing (%s). Build it with `python -m preworld_amd.build` '
            '(hipcc --offload-arch=gfx950). There is no CPU/PyTorch fallback.' % LIB_PATH)
    # torch is imported first (top of this file): its wheel carries its own libamdhip64; if this library were loaded before it, the
    # process would hold two HIP runtimes and calls through this one would see no device
    # ("no ROCm-capable device is detected" -- hit by build() followed by smoke() in one process)
    l = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes, _) in _protos.items():
        try:
            raw, checked = getattr(l, name), l[name]            # two function objects of one symbol
        except AttributeError:
            raise PreworldHipError('libpreworld_hip.so does not export %s (stale build? '
                                   'run python -m preworld_amd.build --force)' % name)
        raw.restype = checked.restype = restype
        raw.argtypes = [ctypes.c_void_p if isinstance(a, _PtrArg) else a for a in argtypes]
        checked.argtypes = argtypes
        _fns[name] = checked
    _lib = l
    return _lib


def protos():
    return _protos


def _refused(e):
    """the PreworldHipError a _PtrArg raised, out of ctypes' wrapping ('argument 3: PreworldHipError: pw_x: y must be ...')"""
    if 'PreworldHipError: ' not in str(e):
        return e
    return PreworldHipError(str(e).split('PreworldHipError: ', 1)[1])


def call_size(name, *args):
    if _lib is None:
        lib()
    try:
        return _fns[name](*args)
    except ctypes.ArgumentError as e:
        raise _refused(e) from None


def call(name, *args):
    """Call an int-returning entry point; raise with pw_last_error() on failure."""
    if _lib is None:
        lib()
    try:
        rc = _fns[name](*args)
    except ctypes.ArgumentError as e:
        raise _refused(e) from None
    if rc != 0:
        msg = _lib.pw_last_error()
        raise PreworldHipError('%s failed (%d): %s' % (name, rc, msg.decode() if msg else ''))
