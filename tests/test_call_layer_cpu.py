"""CPU checks of the one door between the Python package and the C ABI, `_lib.call`: what reaches the library (addresses, NULLs, scalars, the
stream), what is refused before the library is even looked for, and that every call site in the package names a declared entry."""
import ast
import ctypes
import glob
import os
import re

import pytest
import torch

from golden_util import REPO
from ppsurf_amd import _lib
from ppsurf_amd._lib import PpsError


class OnGpu(torch.Tensor):
    """A host tensor that says it lives on a GPU: all that `call` looks at of a device tensor is its device and its address."""
    gpu = 0

    @property
    def device(self):
        return torch.device('cuda', self.gpu)


class OnGpu1(OnGpu):
    gpu = 1


def gpu(t, cls=OnGpu):
    return t.as_subclass(cls)


class Recorder:
    """Stands in for the loaded library: every entry records its arguments and returns `status`."""

    def __init__(self, status=0):
        self.calls, self.status = [], status

    def __getattr__(self, name):
        if not name.startswith('pps_'):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name, args))
            return self.status
        return entry


@pytest.fixture
def stub(monkeypatch):
    rec = Recorder()
    monkeypatch.setattr(_lib, '_lib', rec)
    monkeypatch.setattr(_lib, '_entries', _lib.bind(rec))
    monkeypatch.setattr(_lib, '_stream_on', lambda dev: 0x5000 + (dev.index or 0))
    return rec


def test_tensors_become_addresses_and_everything_else_passes_through(stub):
    ids, order, offsets, ws = (gpu(torch.zeros(8, dtype=torch.int64)) for _ in range(4))
    nbytes = ctypes.c_size_t(64)
    assert _lib.call('pps_csr_build', ids, 8, 0, 0, 5, 1, None, order, offsets, ws, nbytes) == 0
    (name, args), = stub.calls
    assert name == 'pps_csr_build'
    assert args[:11] == (ids.data_ptr(), 8, 0, 0, 5, 1, None, order.data_ptr(), offsets.data_ptr(), ws.data_ptr(), nbytes)
    assert args[10] is nbytes and args[11:] == (0x5000,)                       # the stream of the tensors' device, last
    assert len(args) == len(_lib.SIGNATURES['pps_csr_build'][1])
    m, out = gpu(torch.zeros(4, dtype=torch.float64)), gpu(torch.zeros(3, dtype=torch.float64))
    _lib.call('pps_cloud_outlier_stats', m, 4, 2.5, out)
    assert stub.calls[-1] == ('pps_cloud_outlier_stats', (m.data_ptr(), 4, 2.5, out.data_ptr(), 0x5000))
    view = gpu(torch.zeros(6, 4)[:, 1:3])                                       # a strided view: its own address, layout not looked at
    _lib.call('pps_col_sum', view, 6, 2, 0, out, None)
    assert stub.calls[-1][1][0] == view.data_ptr() != view._base.data_ptr()


def test_the_stream_is_that_of_the_tensors_device(stub):
    a, b = gpu(torch.zeros(4), OnGpu1), gpu(torch.zeros(4), OnGpu1)
    _lib.call('pps_gather_max_f32', a, b, 1, 1, 4, a)
    assert stub.calls[-1][1][-1] == 0x5001


def test_entries_without_a_stream_get_none(stub):
    w = (ctypes.c_float * 4)()
    _lib.call('pps_pack_xyz_f32', ctypes.addressof(w), 1, ctypes.addressof(w))
    assert stub.calls[-1] == ('pps_pack_xyz_f32', (ctypes.addressof(w), 1, ctypes.addressof(w)))


def test_host_arrays_need_on(stub):
    arr = (ctypes.c_void_p * 1)()
    with pytest.raises(PpsError, match='pps_knn_multi_f32.*on='):
        _lib.call('pps_knn_multi_f32', 1, arr, arr, arr, arr, arr, arr)
    assert not stub.calls
    _lib.call('pps_knn_multi_f32', 1, arr, arr, arr, arr, arr, arr, on=gpu(torch.zeros(1), OnGpu1))
    _lib.call('pps_knn_multi_f32', 1, arr, arr, arr, arr, arr, arr, on=torch.device('cuda', 0))
    assert [c[1][-1] for c in stub.calls] == [0x5001, 0x5000] and stub.calls[0][1][1] is arr


def test_cpu_tensors_are_refused_with_or_without_the_library(stub, monkeypatch):
    x = gpu(torch.zeros(4))
    with pytest.raises(PpsError, match=r'pps_gather_max_f32.*cpu.*no CPU'):
        _lib.call('pps_gather_max_f32', x, torch.zeros(4, dtype=torch.int64), 1, 1, 4, x)
    assert not stub.calls
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, '_entries', None)
    monkeypatch.setattr(_lib, 'LIB_PATH', os.path.join(REPO, 'no_such_dir', 'libppsurf_amd.so'))
    with pytest.raises(PpsError, match='no CPU'):
        _lib.call('pps_gather_max_f32', torch.zeros(4), None, 1, 1, 4, None)
    with pytest.raises(PpsError, match='not found'):                           # device tensors get as far as the missing library
        _lib.call('pps_gather_max_f32', x, x, 1, 1, 4, x)


def test_tensors_on_two_devices_are_refused(stub):
    with pytest.raises(PpsError, match='cuda:0 and cuda:1'):
        _lib.call('pps_gather_max_f32', gpu(torch.zeros(4)), gpu(torch.zeros(4), OnGpu1), 1, 1, 4, None)
    assert not stub.calls


def test_a_status_raises_with_the_entry_name(stub):
    stub.status = 2
    x = gpu(torch.zeros(4))
    with pytest.raises(PpsError, match='pps_gather_max_f32 failed with status 2'):
        _lib.call('pps_gather_max_f32', x, x, 1, 1, 4, x)
    assert _lib.call('pps_gather_max_f32', x, x, 1, 1, 4, x, unchecked=True) == 2


def test_unknown_entries_are_refused(stub):
    with pytest.raises(PpsError, match='pps_gather_maxx_f32'):
        _lib.call('pps_gather_maxx_f32', 1)


def test_need_device():
    a, b = gpu(torch.zeros(2)), gpu(torch.zeros(2), OnGpu1)
    assert _lib.need_device('op', a, None, a) == torch.device('cuda', 0)
    with pytest.raises(PpsError, match='op.*no CPU path'):
        _lib.need_device('op', a, torch.zeros(2))
    with pytest.raises(PpsError, match='op.*no CPU path'):
        _lib.need_device('op', [1.0, 2.0])
    with pytest.raises(PpsError, match='one device'):
        _lib.need_device('op', a, b)


# entries that take no stream: the host-side weight packing
NO_STREAM = {'pps_pack_dense_f32', 'pps_pack_dense_f16x3', 'pps_pack_xyz_f32'}


def test_every_call_site_names_a_declared_entry():
    """A typo at a site that no GPU test reaches would only show when that site runs."""
    sites = []
    for path in sorted(glob.glob(os.path.join(REPO, 'ppsurf_amd', '*.py'))):
        text = open(path).read()
        sites += [(os.path.basename(path), n) for n in re.findall(r'\bcall\(\s*[\'"](pps_\w+)[\'"]', text)]
        sites += [(os.path.basename(path), n) for n in re.findall(r'\b_sweep\(\s*[\'"](pps_\w+)[\'"]', text)]      # geometry._sweep(entry, planner, ...)
        assert not re.search(r'_lib\.check\(', text), path + ' checks a status by hand'
    assert len(sites) > 100 and len({f for f, _ in sites}) >= 13
    for where, name in sites:
        assert name in _lib.SIGNATURES, '{}: {} is not declared'.format(where, name)
        assert _lib.SIGNATURES[name][0] is ctypes.c_int, '{}: {} returns no status'.format(where, name)
        assert (_lib.PARAMS[name][-1:] == ['stream']) != (name in NO_STREAM), '{}: {}'.format(where, name)


def test_every_call_site_passes_as_many_arguments_as_the_entry_declares():
    """(97 sites since train_ops.py calls each rows-layer / head entry from one place, 104 before; a site with a starred argument cannot be
    counted: there are three, none of them in train_ops.py, and no more may appear)"""
    checked, starred = 0, []
    for path in sorted(glob.glob(os.path.join(REPO, 'ppsurf_amd', '*.py'))):
        for node in ast.walk(ast.parse(open(path).read())):
            if (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == 'call' and node.args
                    and isinstance(node.args[0], ast.Constant) and str(node.args[0].value).startswith('pps_')):
                if any(isinstance(a, ast.Starred) for a in node.args):
                    starred.append(os.path.basename(path))
                    continue
                name = node.args[0].value
                declared = len(_lib.PARAMS[name]) - (_lib.PARAMS[name][-1:] == ['stream'])
                assert len(node.args) - 1 == declared, '{}:{}: {} takes {} arguments besides the stream'.format(path, node.lineno, name, declared)
                checked += 1
    assert checked > 90 and len(starred) <= 3 and 'train_ops.py' not in starred
