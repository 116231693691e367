"""Records tests/golden/train_ops_bits.json for tests/test_gpu_train_ops_bits.py: the digests and launch sequences of every case of that test, from
whatever ppsurf_amd/train_ops.py is loaded -- run it on an MI355X at the commit whose bits are to be kept (the record in the repository: the file
before its marshalling was folded into shared helpers; the header keeps its git blob).

    python tests/golden/make_train_ops_bits.py [out.json]

Every case runs twice, and a case whose two runs differ in any digest or in the launch sequence is not written: it is named in `left_out` with what
differed.  More than two such cases, or one of the rows-layer family, and nothing is written at all."""
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import test_gpu_train_ops_bits as T  # noqa: E402


def source_ids(path):
    with open(path, 'rb') as f:
        data = f.read()
    return {'train_ops_blob': hashlib.sha1(b'blob %d\0' % len(data) + data).hexdigest(), 'train_ops_sha256': hashlib.sha256(data).hexdigest(),
            'train_ops_lines': data.count(b'\n')}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
    header = dict(source_ids(T.train_ops.__file__), device=torch.cuda.get_device_name(0), torch=torch.__version__)
    cases, left_out = {}, {}
    for name in sorted(T.CASES):
        first, second = (T.run(name, setattr, os.environ.__setitem__) for _ in range(2))
        if first == second:
            cases[name] = first
            continue
        keys = [k for k in first['tensors'] if first['tensors'][k] != second['tensors'].get(k)]
        left_out[name] = 'two runs on the recorded source differ: ' + (', '.join(keys) if keys else 'launch sequence')
        print('NOT RECORDED', name, left_out[name])
    family = [n for n in left_out if n.split('-')[0] in T.ROWS_FAMILY]
    if len(left_out) > 2 or family:
        sys.exit('{} cases differ from run to run ({} of the rows-layer family): nothing written'.format(len(left_out), len(family)))
    with open(out, 'w') as f:
        dumps = lambda o: json.dumps(o, sort_keys=True)
        f.write('{{"header": {},\n"left_out": {},\n"cases": {{\n{}\n}}}}\n'.format(                     # one case per line
            dumps(header), dumps(left_out), ',\n'.join('{}: {}'.format(dumps(n), dumps(cases[n])) for n in sorted(cases))))
    print('wrote {}: {} cases, {} left out, {} bytes, from blob {}'.format(out, len(cases), len(left_out), os.path.getsize(out), header['train_ops_blob']))


if __name__ == '__main__':
    main()
