"""Where the package calls the extension entries (`ppsx_*`), read from the syntax trees of every ppsurf_amd/*.py: shared by the call-site tests
of the stages."""
import ast
import glob
import os

from golden_util import REPO


def _forwarded_args():
    """Arguments after the entry name in the one `_lib.call(entry, ...)` of topology.sorted_keys, which passes its first parameter on."""
    tree = ast.parse(open(os.path.join(REPO, 'ppsurf_amd', 'topology.py')).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == 'sorted_keys']
    assert len(fn) == 1 and fn[0].args.args[0].arg == 'entry'
    calls = [n for n in ast.walk(fn[0]) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == 'call']
    assert len(calls) == 1 and isinstance(calls[0].args[0], ast.Name) and calls[0].args[0].id == 'entry'
    assert not any(isinstance(a, ast.Starred) for a in calls[0].args) and not calls[0].keywords
    return len(calls[0].args) - 1


def ext_call_sites(prefix):
    """{entry name: [(file, line, arguments passed to the entry, the stream not counted)]} for the entries whose name starts with `prefix`:
    every call that names one as its first argument, `_lib.call('ppsx_...', ...)` or `sorted_keys('ppsx_...', ...)` (topology.py)."""
    sites = {}
    for path in sorted(glob.glob(os.path.join(REPO, 'ppsurf_amd', '*.py'))):
        for node in ast.walk(ast.parse(open(path).read())):
            if (isinstance(node, ast.Call) and node.args and isinstance(node.args[0], ast.Constant) and isinstance(node.args[0].value, str)
                    and node.args[0].value.startswith(prefix)):
                where = '{}:{}'.format(os.path.basename(path), node.lineno)
                assert not any(isinstance(a, ast.Starred) for a in node.args), where
                called = node.func.attr if isinstance(node.func, ast.Attribute) else getattr(node.func, 'id', None)
                assert called in ('call', 'sorted_keys'), where
                nargs = len(node.args) - 1 if called == 'call' else _forwarded_args()
                sites.setdefault(node.args[0].value, []).append((os.path.basename(path), node.lineno, nargs))
    return sites
