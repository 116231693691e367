"""Records tests/golden/unpacked_valu.npz for tests/test_gpu_unpacked_valu.py: g, xbar, logits and occupancy of the f16x3 decoder at the cases of that
test, from whatever library is loaded -- run it on an MI355X at the commit whose bits are to be kept (the record in the repository: the parent of the
commit that compiled the split-precision kernels without packed fp32 VALU).

    python tests/golden/make_unpacked_valu.py [out.npz]

Every case is decoded under each of the test's switches; the recorder refuses to write unless all of them give the same bits, so one record per case
serves all."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import test_gpu_unpacked_valu as T  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
    record = {}
    for q, p, k in T.CASES:
        first = None
        for switch in sorted(T.SWITCHES):
            got, fallbacks = T.decode(q, p, k, T.SWITCHES[switch], os.environ.__setitem__, lambda n: os.environ.pop(n, None))
            assert fallbacks == 0, (q, p, k, switch)
            if first is None:
                first = got
            for n in T.NAMES:
                assert torch.isfinite(got[n]).all() and torch.equal(got[n], first[n]), (q, p, k, switch, n)
        for n in T.NAMES:
            record[T.key(q, p, k, n)] = first[n].cpu().numpy()
    np.savez_compressed(out, **record)
    print('wrote {}: {} arrays, {} bytes'.format(out, len(record), os.path.getsize(out)))


if __name__ == '__main__':
    main()
