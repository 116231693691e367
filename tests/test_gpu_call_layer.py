"""`_lib.call` hands a kernel the stream that is current for its tensors' device: on a side stream, and while that stream is being captured."""
import pytest
import torch

from ppsurf_amd import _lib, train_ops

pytestmark = pytest.mark.gpu


class Recorder:
    """The loaded library with every call noted: (entry, arguments as ctypes received them)."""

    def __init__(self, handle):
        self.handle, self.calls = handle, []

    def __getattr__(self, name):
        fn = getattr(self.handle, name)

        def entry(*args):
            self.calls.append((name, args))
            return fn(*args)
        return entry


def test_gather_rows_runs_on_the_current_side_stream_eagerly_and_captured(monkeypatch):
    rec = Recorder(_lib.lib())
    monkeypatch.setattr(_lib, '_lib', rec)
    monkeypatch.setattr(_lib, '_entries', _lib.bind(rec))
    dev = torch.device('cuda', torch.cuda.current_device())
    x = torch.arange(16, dtype=torch.float32, device=dev).reshape(4, 4)
    idx = torch.tensor([3, 0, 2], device=dev)
    expected = x[idx]
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        out = train_ops.gather_rows(x, idx)
    side.synchronize()
    (name, args), = rec.calls
    assert name == 'pps_gather_rows_f32' and args[-1] == side.cuda_stream != torch.cuda.current_stream(dev).cuda_stream
    assert args[:5] == (x.data_ptr(), idx.data_ptr(), 3, 4, out.data_ptr())
    assert torch.equal(out, expected)

    # the same call captured on a side stream: the replay fills the captured output again
    graph = torch.cuda.CUDAGraph()
    capture = torch.cuda.Stream(device=dev)
    capture.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.graph(graph, stream=capture):
        out_g = train_ops.gather_rows(x, idx)
    assert rec.calls[-1][0] == 'pps_gather_rows_f32' and rec.calls[-1][1][-1] == capture.cuda_stream
    out_g.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_g, expected)
