"""CPU tier of the argument rule of the strict mesh stages (ppsurf_amd/params.py): the two helpers alone, and a table
over every `_checked_*` function of the stages -- for each parameter and each value of VALUES whether the call is accepted and what comes
back, or the full text of the ValueError.  The expected side was recorded from the functions as they stood before they shared the helper;
`remesh._checked_remesh` reached the rules of `flip_angle` and `max_faces` through `flip._checked_params(x, 1e-6, 100)[0]` and
`subdivide._checked_params(1.0, None, 100, x)[3]` then, which is how `flip._checked_angle` and `subdivide._checked_max_faces` were recorded."""
import math

import numpy as np
import pytest

from ppsurf_amd import decimate, denoise, fill, flip, intersect, normals, params, pieces, remesh, smooth, subdivide, weld

VALUES = {'True': True, 'np.bool_(True)': np.bool_(True), 'None': None, "'x'": 'x', 'nan': math.nan, 'inf': math.inf, '-inf': -math.inf,
          '-1': -1, '0': 0, '2**31': 2 ** 31, '1.5': 1.5, 'np.float32(0.5)': np.float32(0.5), 'np.int64(7)': np.int64(7)}


def same(got, want):
    """Equal values of equal Python types, through tuples."""
    if type(got) is not type(want):
        return False
    if isinstance(want, tuple):
        return len(got) == len(want) and all(same(g, w) for g, w in zip(got, want))
    return got == want


def test_integer():
    for key, value in VALUES.items():
        if key in ('0', 'np.int64(7)'):
            assert same(params.integer('n', value, 0, 2 ** 31 - 1), int(value))
            continue
        with pytest.raises(ValueError) as e:
            params.integer('n', value, 0, 2 ** 31 - 1, '0..2^31 - 1')
        assert str(e.value) == 'n must be an integer in 0..2^31 - 1, got {!r}'.format(value)
    assert same(params.integer('n', -1, -1, 0), -1) and same(params.integer('n', np.int8(3), 3, 3), 3)
    for value in (0, 8, np.int64(8)):
        with pytest.raises(ValueError) as e:
            params.integer('rounds', value, 1, 7)
        assert str(e.value) == 'rounds must be an integer in 1..7, got {!r}'.format(value)


def test_number():
    positive = lambda x: x > 0                                                                      # noqa: E731
    for key, value in VALUES.items():
        if key in ('2**31', '1.5', 'np.float32(0.5)', 'np.int64(7)'):
            assert same(params.number('x', value, positive, 'a finite number > 0'), float(value))
            continue
        with pytest.raises(ValueError) as e:
            params.number('x', value, positive, 'a finite number > 0')
        assert str(e.value) == 'x must be a finite number > 0, got {!r}'.format(value)
    seen = []
    assert same(params.number('x', np.int64(7), lambda x: seen.append(x) or True, 'any'), 7.0) and same(seen[0], 7.0)      # ok sees the float
    for value in (np.float64(math.nan), np.float32(math.inf)):
        with pytest.raises(ValueError):
            params.number('x', value, lambda x: True, 'a finite number')


# parameter -> the call with every other parameter at a good value
CALLS = {
    'decimate.max_faces': lambda x: decimate._checked_params(x, 1000),
    'decimate.max_rounds': lambda x: decimate._checked_params(100, x),
    'flip.max_angle': lambda x: flip._checked_params(x, 1e-6, 100),
    'flip.min_gain': lambda x: flip._checked_params(10.0, x, 100),
    'flip.max_rounds': lambda x: flip._checked_params(10.0, 1e-6, x),
    'flip._checked_angle': lambda x: flip._checked_angle(x),
    'subdivide.max_edge': lambda x: subdivide._checked_params(x, None, 100, None),
    'subdivide.factor': lambda x: subdivide._checked_params(None, x, 100, None),
    'subdivide.max_rounds': lambda x: subdivide._checked_params(1.0, None, x, None),
    'subdivide.max_faces': lambda x: subdivide._checked_params(1.0, None, 100, x),
    'subdivide._checked_max_faces': lambda x: subdivide._checked_max_faces(x),
    'remesh.collapse.min_edge': lambda x: remesh._checked_collapse(x, None, 1000),
    'remesh.collapse.max_edge': lambda x: remesh._checked_collapse(1.0, x, 1000),
    'remesh.collapse.max_rounds': lambda x: remesh._checked_collapse(1.0, None, x),
    'remesh.relax.iters': lambda x: remesh._checked_relax(x, 0.5),
    'remesh.relax.lam': lambda x: remesh._checked_relax(1, x),
    'remesh.target_edge': lambda x: remesh._checked_remesh(x, None, 5, 0.5, 10.0, None),
    'remesh.factor': lambda x: remesh._checked_remesh(None, x, 5, 0.5, 10.0, None),
    'remesh.iters': lambda x: remesh._checked_remesh(1.0, None, x, 0.5, 10.0, None),
    'remesh.relax_lam': lambda x: remesh._checked_remesh(1.0, None, 5, x, 10.0, None),
    'remesh.flip_angle': lambda x: remesh._checked_remesh(1.0, None, 5, 0.5, x, None),
    'remesh.max_faces': lambda x: remesh._checked_remesh(1.0, None, 5, 0.5, 10.0, x),
    'weld.eps': lambda x: weld._checked_eps(x),
    'denoise.threshold': lambda x: denoise._checked_params(x, 3, 3),
    'denoise.normal_iters': lambda x: denoise._checked_params(0.5, x, 3),
    'denoise.vertex_iters': lambda x: denoise._checked_params(0.5, 3, x),
    'pieces.min_faces': lambda x: pieces._checked_rules(x, 0.5, 2),
    'pieces.min_diag_frac': lambda x: pieces._checked_rules(3, x, 2),
    'pieces.keep_largest': lambda x: pieces._checked_rules(3, 0.5, x),
    'fill.max_edges': lambda x: fill._checked_max_edges(x),
    'fill.max_edges as --max_hole_edges': lambda x: fill._checked_max_edges(x, '--max_hole_edges'),
    'intersect.max_pairs': lambda x: intersect._checked_params(x),
    'normals.k': lambda x: normals._checked_k(x),
    'smooth.iters': lambda x: smooth._checked_params(x, 0.5, -0.53),
}

# parameter -> ({value: what comes back}, {text of the ValueError: the values that raise it}).  '{0!r}' in a text is the offending value and
# '{1!r}' its float(), formatted here from the value itself and not pasted, so that no cell depends on numpy's repr.
TABLE = {
    'decimate.max_faces': (
        {'np.int64(7)': (7, 1000)},
        {'max_faces must be an integer in 4..2^31 - 1, got {0!r}': "True | np.bool_(True) | None | 'x' | nan | inf | -inf | -1 | 0 | 2**31 | 1.5 | np.float32(0.5)"}),
    'decimate.max_rounds': (
        {'np.int64(7)': (100, 7)},
        {'max_rounds must be an integer in 1..2^31 - 1, got {0!r}': "True | np.bool_(True) | None | 'x' | nan | inf | -inf | -1 | 0 | 2**31 | 1.5 | np.float32(0.5)"}),
    'flip.max_angle': (
        {'1.5': (1.5, 1e-06, 100), 'np.float32(0.5)': (0.5, 1e-06, 100), 'np.int64(7)': (7.0, 1e-06, 100)},
        {'max_angle must be a finite number, got {0!r}': "True | np.bool_(True) | None | 'x' | nan | inf | -inf",
         'max_angle must lie in (0, 90], got {0!r}': '-1 | 0 | 2**31'}),
    'flip.min_gain': (
        {'0': (10.0, 0.0, 100), '2**31': (10.0, 2147483648.0, 100), '1.5': (10.0, 1.5, 100), 'np.float32(0.5)': (10.0, 0.5, 100), 'np.int64(7)': (10.0, 7.0, 100)},
        {'min_gain must be a finite number, got {0!r}': "True | np.bool_(True) | None | 'x' | nan | inf | -inf",
         'min_gain must be >= 0, got {0!r}': '-1'}),
    'flip.max_rounds': (
        {'np.int64(7)': (10.0, 1e-06, 7)},
        {'max_rounds must be an integer in 1..2^31 - 1, got {0!r}': "True | np.bool_(True) | None | 'x' | nan | inf | -inf | -1 | 0 | 2**31 | 1.5 | np.float32(0.5)"}),
    'flip._checked_angle': (
        {'1.5': 1.5, 'np.float32(0.5)': 0.5, 'np.int64(7)': 7.0},
        {'max_angle must be a finite number, got {0!r}': "True | np.bool_(True) | None | 'x' | nan | inf | -inf",
         'max_angle must lie in (0, 90], got {0!r}': '-1 | 0 | 2**31'}),
    'subdivide.max_edge': (
        {'2**31': (2147483648.0, None, 100, 1431655765), '1.5': (1.5, None, 100, 1431655765), 'np.float32(0.5)': (0.5, None, 100, 1431655765), 'np.int64(7)': (7.0, None, 100, 1431655765)},
        {'max_edge must be a finite number > 0, got {0!r}': "True | np.bool_(True) | 'x' | nan | inf | -inf | -1 | 0",
         'exactly one of max_edge and factor must be given, got None and None': 'None'}),
    'subdivide.factor': (
        {'2**31': (None, 2147483648.0, 100, 1431655765), '1.5': (None, 1.5, 100, 1431655765), 'np.float32(0.5)': (None, 0.5, 100, 1431655765), 'np.int64(7)': (None, 7.0, 100, 1431655765)},
        {'factor must be a finite number > 0, got {0!r}': "True | np.bool_(True) | 'x' | nan | inf | -inf | -1 | 0",
         'exactly one of max_edge and factor must be given, got None and None': 'None'}),
    'subdivide.max_rounds': (
        {'np.int64(7)': (1.0, None, 7, 1431655765)},
        {'max_rounds must be an integer in 1..2^31 - 1, got {0!r}': "True | np.bool_(True) | None | 'x' | nan | inf | -inf | -1 | 0 | 2**31 | 1.5 | np.float32(0.5)"}),
    'subdivide.max_faces': (
        {'None': (1.0, None, 100, 1431655765), '0': (1.0, None, 100, 0), 'np.int64(7)': (1.0, None, 100, 7)},
        {'max_faces must be an integer in 0..1431655765, got {0!r}': "True | np.bool_(True) | 'x' | nan | inf | -inf | -1 | 2**31 | 1.5 | np.float32(0.5)"}),
    'subdivide._checked_max_faces': (
        {'None': 1431655765, '0': 0, 'np.int64(7)': 7},
        {'max_faces must be an integer in 0..1431655765, got {0!r}': "True | np.bool_(True) | 'x' | nan | inf | -inf | -1 | 2**31 | 1.5 | np.float32(0.5)"}),
    'remesh.collapse.min_edge': (
        {'2**31': (2147483648.0, None, 1000), '1.5': (1.5, None, 1000), 'np.float32(0.5)': (0.5, None, 1000), 'np.int64(7)': (7.0, None, 1000)},
        {'min_edge must be a finite number > 0, got {0!r}': "True | np.bool_(True) | None | 'x' | nan | inf | -inf | -1 | 0"}),
    'remesh.collapse.max_edge': (
        {'None': (1.0, None, 1000), '2**31': (1.0, 2147483648.0, 1000), '1.5': (1.0, 1.5, 1000), 'np.int64(7)': (1.0, 7.0, 1000)},
        {'max_edge must be None or a finite number >= min_edge = 1.0, got {0!r}': "True | np.bool_(True) | 'x' | nan | inf | -inf | -1 | 0 | np.float32(0.5)"}),
    'remesh.collapse.max_rounds': (
        {'np.int64(7)': (1.0, None, 7)},
        {'max_rounds must be an integer in 1..2^31 - 1, got {0!r}': "True | np.bool_(True) | None | 'x' | nan | inf | -inf | -1 | 0 | 2**31 | 1.5 | np.float32(0.5)"}),
    'remesh.relax.iters': (
        {'0': (0, 0.5), 'np.int64(7)': (7, 0.5)},
        {'iters must be an integer in 0..1000, got {0!r}': "True | np.bool_(True) | None | 'x' | nan | inf | -inf | -1 | 2**31 | 1.5 | np.float32(0.5)"}),
    'remesh.relax.lam': (
        {'np.float32(0.5)': (1, 0.5)},
        {'lam must be a finite number in (0, 1], got {0!r}': "True | np.bool_(True) | None | 'x' | nan | inf | -inf | -1 | 0 | 2**31 | 1.5 | np.int64(7)"}),
    'remesh.target_edge': (
        {'2**31': (2147483648.0, None, 5, 0.5, 10.0, 1431655765), '1.5': (1.5, None, 5, 0.5, 10.0, 1431655765), 'np.float32(0.5)': (0.5, None, 5, 0.5, 10.0, 1431655765), 'np.int64(7)': (7.0, None, 5, 0.5, 10.0, 1431655765)},
        {'target_edge must be a finite number > 0, got {0!r}': "True | np.bool_(True) | 'x' | nan | inf | -inf | -1 | 0",
         'exactly one of target_edge and factor must be given, got None and None': 'None'}),
    'remesh.factor': (
        {'2**31': (None, 2147483648.0, 5, 0.5, 10.0, 1431655765), '1.5': (None, 1.5, 5, 0.5, 10.0, 1431655765), 'np.float32(0.5)': (None, 0.5, 5, 0.5, 10.0, 1431655765), 'np.int64(7)': (None, 7.0, 5, 0.5, 10.0, 1431655765)},
        {'factor must be a finite number > 0, got {0!r}': "True | np.bool_(True) | 'x' | nan | inf | -inf | -1 | 0",
         'exactly one of target_edge and factor must be given, got None and None': 'None'}),
    'remesh.iters': (
        {'0': (1.0, None, 0, 0.5, 10.0, 1431655765), 'np.int64(7)': (1.0, None, 7, 0.5, 10.0, 1431655765)},
        {'iters must be an integer in 0..1000, got {0!r}': "True | np.bool_(True) | None | 'x' | nan | inf | -inf | -1 | 2**31 | 1.5 | np.float32(0.5)"}),
    'remesh.relax_lam': (
        {'np.float32(0.5)': (1.0, None, 5, 0.5, 10.0, 1431655765)},
        {'relax_lam must be a finite number in (0, 1], got {0!r}': "True | np.bool_(True) | None | 'x' | nan | inf | -inf | -1 | 0 | 2**31 | 1.5 | np.int64(7)"}),
    'remesh.flip_angle': (
        {'1.5': (1.0, None, 5, 0.5, 1.5, 1431655765), 'np.float32(0.5)': (1.0, None, 5, 0.5, 0.5, 1431655765), 'np.int64(7)': (1.0, None, 5, 0.5, 7.0, 1431655765)},
        {'max_angle must be a finite number, got {0!r}': "True | np.bool_(True) | None | 'x' | nan | inf | -inf",
         'max_angle must lie in (0, 90], got {0!r}': '-1 | 0 | 2**31'}),
    'remesh.max_faces': (
        {'None': (1.0, None, 5, 0.5, 10.0, 1431655765), '0': (1.0, None, 5, 0.5, 10.0, 0), 'np.int64(7)': (1.0, None, 5, 0.5, 10.0, 7)},
        {'max_faces must be an integer in 0..1431655765, got {0!r}': "True | np.bool_(True) | 'x' | nan | inf | -inf | -1 | 2**31 | 1.5 | np.float32(0.5)"}),
    'weld.eps': (
        {'0': 0.0, '2**31': 2147483648.0, '1.5': 1.5, 'np.float32(0.5)': 0.5, 'np.int64(7)': 7.0},
        {'eps must be a finite number >= 0, got {0!r}': "True | np.bool_(True) | None | 'x' | nan | inf | -inf",
         'eps must be a finite number >= 0, got {1!r}': '-1'}),
    'denoise.threshold': (
        {'0': (0.0, 3, 3), 'np.float32(0.5)': (0.5, 3, 3)},
        {'threshold must be a number in [0, 1), got {0!r}': "True | np.bool_(True) | None | 'x'",
         'threshold must be a finite number in [0, 1), got {0!r}': 'nan | inf | -inf | 1.5',
         'threshold must be a finite number in [0, 1), got {1!r}': '-1 | 2**31 | np.int64(7)'}),
    'denoise.normal_iters': (
        {'0': (0.5, 0, 3), 'np.int64(7)': (0.5, 7, 3)},
        {'normal_iters must be an integer in 0..1000, got {0!r}': "True | np.bool_(True) | None | 'x' | nan | inf | -inf | -1 | 2**31 | 1.5 | np.float32(0.5)"}),
    'denoise.vertex_iters': (
        {'0': (0.5, 3, 0), 'np.int64(7)': (0.5, 3, 7)},
        {'vertex_iters must be an integer in 0..1000, got {0!r}': "True | np.bool_(True) | None | 'x' | nan | inf | -inf | -1 | 2**31 | 1.5 | np.float32(0.5)"}),
    'pieces.min_faces': (
        {'None': (None, 0.5, 2), 'np.int64(7)': (7, 0.5, 2)},
        {'min_faces must be an integer in 1..2^31 - 1, got {0!r}': "True | np.bool_(True) | 'x' | nan | inf | -inf | -1 | 0 | 2**31 | 1.5 | np.float32(0.5)"}),
    'pieces.min_diag_frac': (
        {'None': (3, None, 2), '0': (3, 0.0, 2), 'np.float32(0.5)': (3, 0.5, 2)},
        {'min_diag_frac must be a number in [0, 1], got {0!r}': "True | np.bool_(True) | 'x'",
         'min_diag_frac must be a finite number in [0, 1], got {0!r}': 'nan | inf | -inf | 1.5',
         'min_diag_frac must be a finite number in [0, 1], got {1!r}': '-1 | 2**31 | np.int64(7)'}),
    'pieces.keep_largest': (
        {'None': (3, 0.5, None), 'np.int64(7)': (3, 0.5, 7)},
        {'keep_largest must be an integer in 1..2^31 - 1, got {0!r}': "True | np.bool_(True) | 'x' | nan | inf | -inf | -1 | 0 | 2**31 | 1.5 | np.float32(0.5)"}),
    'fill.max_edges': (
        {'np.int64(7)': 7},
        {'max_edges must be an integer in 3..4096, got {0!r}': "True | np.bool_(True) | None | 'x' | nan | inf | -inf | -1 | 0 | 2**31 | 1.5 | np.float32(0.5)"}),
    'fill.max_edges as --max_hole_edges': (
        {'np.int64(7)': 7},
        {'--max_hole_edges must be an integer in 3..4096, got {0!r}': "True | np.bool_(True) | None | 'x' | nan | inf | -inf | -1 | 0 | 2**31 | 1.5 | np.float32(0.5)"}),
    'intersect.max_pairs': (
        {'0': 0, 'np.int64(7)': 7},
        {'max_pairs must be an integer in 0..2^31 - 1, got {0!r}': "True | np.bool_(True) | None | 'x' | nan | inf | -inf | -1 | 2**31 | 1.5 | np.float32(0.5)"}),
    'normals.k': (
        {'np.int64(7)': 7},
        {'k must be an integer in 1..256, got {0!r}': "True | np.bool_(True) | None | 'x' | nan | inf | -inf | -1 | 0 | 2**31 | 1.5 | np.float32(0.5)"}),
    'smooth.iters': (
        {'0': (0, 0.5, -0.53), 'np.int64(7)': (7, 0.5, -0.53)},
        {'iters must be an integer in 0..1000, got {0!r}': "True | np.bool_(True) | None | 'x' | nan | inf | -inf | -1 | 2**31 | 1.5 | np.float32(0.5)"}),
}


def cells():
    for name, (accepted, errors) in TABLE.items():
        for key, want in accepted.items():
            yield name, key, want, None
        for text, keys in errors.items():
            for key in keys.split(' | '):
                yield name, key, None, text


def test_the_table_covers_every_parameter_and_value():
    assert sorted(TABLE) == sorted(CALLS)
    seen = {}
    for name, key, _, _ in cells():
        seen.setdefault(name, []).append(key)
    assert all(sorted(keys) == sorted(VALUES) for keys in seen.values()) and sorted(seen) == sorted(CALLS)


@pytest.mark.parametrize('name', sorted(CALLS))
def test_checked_functions_answer_as_before(name):
    for cell, key, want, text in cells():
        if cell != name:
            continue
        value = VALUES[key]
        if text is None:
            got = CALLS[name](value)
            assert same(got, want), '{}({}): {!r}, not {!r}'.format(name, key, got, want)
            continue
        with pytest.raises(ValueError) as e:
            CALLS[name](value)
        as_float = float(value) if isinstance(value, (int, float, np.integer, np.floating)) else None
        assert str(e.value) == text.format(value, as_float), '{}({})'.format(name, key)
