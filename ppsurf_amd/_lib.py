"""ctypes binding of the C ABI declared in include/ppsurf_amd.h and of its extension entries (prefix `ppsx_`) in include/ppsurf_amd_ext.h.

The product path has NO fallback: if libppsurf_amd.so is missing or fails to load, importing an op raises.
"""
import ctypes
import os
import re

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, 'libppsurf_amd.so')
if os.environ.get('PPS_LIB_VARIANT'):          # development aid: an ablation / tuning build made by `python -m ppsurf_amd.build --variant NAME`
    LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), 'libppsurf_amd_{}.so'.format(os.environ['PPS_LIB_VARIANT']))

HEADER_PATH = os.path.join(os.path.dirname(HERE), 'include', 'ppsurf_amd.h')
EXT_HEADER_PATH = os.path.join(os.path.dirname(HERE), 'include', 'ppsurf_amd_ext.h')          # entries added after ABI version 2

_SCALARS = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'size_t': ctypes.c_size_t, 'float': ctypes.c_float, 'double': ctypes.c_double,
            'uint32_t': ctypes.c_uint32, 'uint64_t': ctypes.c_uint64}


class PpsError(RuntimeError):
    pass


def parse_header(text, prefix='pps_'):
    """(SIGNATURES, PARAMS) of the `pps_*` declarations (of the `prefix*` ones) of a C header: name -> (restype, argtypes) and name ->
    parameter names.  No C grammar: one regex over the text without comments; a type with `*` or `[` is a pointer, any other must be in _SCALARS."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*|^[ \t]*#[^\n]*', ' ', text, flags=re.S | re.M)
    signatures, names = {}, {}
    for ret, name, params in re.findall(r'([\w \t*]+?)\b(' + re.escape(prefix) + r'\w+)\s*\(([^()]*)\)\s*;', text):
        params = [p.split() for p in params.split(',') if p.strip() not in ('', 'void')]
        try:
            argtypes = [ctypes.c_void_p if '*' in ''.join(p) or '[' in p[-1] else _SCALARS[' '.join(w for w in p[:-1] if w != 'const')] for p in params]
            signatures[name] = (_SCALARS[ret.strip()], argtypes)
        except KeyError as e:
            raise ValueError('{}: no ctypes type for "{}" in `{} {}({})`'.format(HEADER_PATH, e.args[0], ret.strip(), name, ', '.join(' '.join(p) for p in params)))
        names[name] = [re.match(r'\**(\w+)', p[-1]).group(1) for p in params]
    return signatures, names


with open(HEADER_PATH) as _f:
    SIGNATURES, PARAMS = parse_header(_f.read())          # read from include/ppsurf_amd.h, the header the library is compiled against
with open(EXT_HEADER_PATH) as _f:
    EXT_SIGNATURES, EXT_PARAMS = parse_header(_f.read(), prefix='ppsx_')

_lib = None            # the loaded library
_entries = None        # name -> (function, takes a stream): what `call` needs of an entry, resolved once by bind()
_ext_entries = {}      # the same for the extension entries, filled by lib(): empty while something else installs _entries directly


def _bind(handle, signatures, params, optional=False):
    """optional: an entry the library does not export is left out instead of raised (a PPS_LIB_VARIANT library built from an older tree)"""
    entries = {}
    for name, (res, args) in signatures.items():
        if optional and not hasattr(handle, name):
            continue
        fn = getattr(handle, name)          # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
        entries[name] = (fn, params[name][-1:] == ['stream'])
    return entries


def bind(handle):
    """Types every entry of `handle` that the main header declares and returns the table `call` dispatches through."""
    return _bind(handle, SIGNATURES, PARAMS)


def lib():
    global _lib, _entries, _ext_entries
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise PpsError('{} not found: build it with `python -m ppsurf_amd.build` (hipcc, gfx950). '
                           'There is no CPU fallback.'.format(LIB_PATH))
        handle = ctypes.CDLL(LIB_PATH)
        _entries = bind(handle)
        # a variant library (development aid, e.g. `--variant parent` built in a checkout of the parent commit and copied here for an A/B run)
        # may predate an extension entry: calling that entry then fails as undeclared; the product library must export every one
        _ext_entries = _bind(handle, EXT_SIGNATURES, EXT_PARAMS, optional=bool(os.environ.get('PPS_LIB_VARIANT')))
        _lib = handle
    return _lib


def check(rc, what):
    if rc != 0:
        raise PpsError('{} failed with status {} ({})'.format(what, rc, {1: 'bad argument', 2: 'launch failure'}.get(rc, '?')))


def _same_device(what, dev, d):
    if d.type != 'cuda':
        raise PpsError('{}: tensor on {}; inputs must be device tensors, there is no CPU path'.format(what, d))
    if dev is not None and d != dev:
        raise PpsError('{}: tensors on {} and {}; inputs must share one device'.format(what, dev, d))
    return d


def need_device(what, *tensors):
    """The device guard of a public function: every argument is a tensor on one GPU (None is skipped).  Returns that device."""
    dev = None
    for t in tensors:
        if t is not None:
            if not torch.is_tensor(t):
                raise PpsError('{}: got {}; inputs must be device tensors, there is no CPU path'.format(what, type(t).__name__))
            dev = _same_device(what, dev, t.device)
    return dev


def need_gpu(what, device=None):
    """PpsError unless a GPU is there (and `device`, where given, names one): the guard of the command lines and of the functions that upload
    host arrays."""
    if (device is not None and torch.device(device).type != 'cuda') or not torch.cuda.is_available():
        raise PpsError('{} runs on the GPU only{}; there is no CPU fallback'.format(what, '' if device is None else ' (device={!r})'.format(str(device))))


_PLAIN = frozenset((int, float, bool, type(None)))


def _stream_on(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def call(name, *args, on=None, unchecked=False):
    """Calls the status-returning entry `name` of the C ABI and raises PpsError unless it returns 0.

    Tensors are passed as their addresses and must share one GPU (checked before the library is loaded); None is NULL; everything
    else goes to ctypes as it is.  An entry whose last parameter is `stream` gets the current stream of the tensors' device -- of
    `on` (a tensor or a device) where every pointer comes in a host array.  Neither layout nor dtype is looked at.  unchecked: the
    status is returned instead (the budget searches probe with steps the library refuses)."""
    argv, dev = [], None
    for a in args:
        if type(a) not in _PLAIN and isinstance(a, torch.Tensor):          # (isinstance against torch.Tensor is slow for what is no tensor)
            if a.device != dev:
                dev = _same_device(name, dev, a.device)
            a = a.data_ptr()
        argv.append(a)
    if _entries is None:
        lib()
    try:
        fn, takes_stream = _entries[name]
    except KeyError:                                   # the main table, then the extension table: one set of rules for both
        if name not in _ext_entries:
            raise PpsError('{} is not declared in {}'.format(name, EXT_HEADER_PATH if name.startswith('ppsx_') else HEADER_PATH)) from None
        fn, takes_stream = _ext_entries[name]
    if takes_stream:
        if on is not None:
            dev = on.device if isinstance(on, torch.Tensor) else on
        if dev is None:
            raise PpsError('{}: no tensor argument to take the stream from; pass on='.format(name))
        argv.append(_stream_on(dev))
    rc = fn(*argv)
    if rc != 0 and not unchecked:
        check(rc, name)
    return rc
