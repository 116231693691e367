"""CPU checks of the host side of the decoder: C ABI loads and exports every declared symbol, the packing is a
bijection, and the folded/composed/packed weight images reproduce the reference's from_latent (golden fixture)."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest
import torch

from golden_util import REPO, load_golden, filled_sd
from ppsurf_amd import _lib
from ppsurf_amd.decoder import DecoderPlan, pack_dense, pack_xyz
from ppsurf_amd.synthetic import make_latents
import emulate


def _exported_symbols(path):
    """Names of the defined symbols in the dynamic symbol table of an ELF64 little-endian shared object."""
    blob = open(path, 'rb').read()
    assert blob[:6] == b'\x7fELF\x02\x01'
    shoff, = struct.unpack_from('<Q', blob, 0x28)
    shentsize, shnum = struct.unpack_from('<HH', blob, 0x3a)
    sections = [struct.unpack_from('<IIQQQQIIQQ', blob, shoff + i * shentsize) for i in range(shnum)]
    names = set()
    for _, kind, _, _, offset, size, link, _, _, entsize in sections:
        if kind == 11:                                                     # SHT_DYNSYM; `link` is its string table
            strtab = sections[link][4]
            for at in range(offset, offset + size, entsize):
                name, _, _, shndx = struct.unpack_from('<IBBH', blob, at)
                if shndx != 0:
                    names.add(blob[strtab + name:blob.index(b'\0', strtab + name)].decode())
    return names


def test_library_exports_every_declared_symbol():
    header = open(os.path.join(REPO, 'include', 'ppsurf_amd.h')).read()
    # _lib.SIGNATURES is parsed from the header, so the declared set comes from the library itself: everything it exports
    declared = {n for n in _exported_symbols(_lib.LIB_PATH) if n.startswith('pps_')}
    assert declared, 'no entry points found in the dynamic symbol table'
    assert declared == set(re.findall(r'\b(pps_[a-z0-9_]+)\s*\(', header))
    lib = _lib.lib()
    for name in sorted(declared):
        assert hasattr(lib, name), 'libppsurf_amd.so does not export ' + name
    assert declared == set(_lib.SIGNATURES.keys())
    assert lib.pps_abi_version() == 2


def test_signatures_parsed_from_the_header_have_the_declared_types():
    """Literal signatures covering every scalar kind of the header (float, double, uint32_t, uint64_t, size_t parameters; size_t and int64_t
    results; a `const T* const*` parameter): a parser that mapped int64_t to c_int, or double to c_float, would load and corrupt arguments."""
    c = ctypes
    P, I, I64 = c.c_void_p, c.c_int, c.c_int64
    expected = {
        'pps_voxel_sample_f32': (I, [P, I64, I64, c.c_float, P, I, c.c_uint32, P, P, P, P]),
        'pps_simplify_leaders': (I, [P, I64, P, P, c.c_double, c.c_double, P, P, I64, P, P, P]),
        'pps_eval_sample_surface': (I, [P, P, I64, I64, c.c_uint64, c.c_uint64, P, P, P]),
        'pps_csr_build': (I, [P, I64, I64, I64, I64, I, P, P, P, P, c.c_size_t, P]),
        'pps_csr_ws_bytes': (c.c_size_t, [I64, I64]),
        'pps_mc_cube_blocks': (I64, [I64, I64, I64]),
        'pps_knn_blocked_batch_f32': (I, [I, I64] + [P] * 13),
        'pps_abi_version': (I, []),
    }
    for name, sig in expected.items():
        assert _lib.SIGNATURES[name] == sig, name
    assert _lib.PARAMS['pps_csr_build'] == ['ids', 'entries', 'per_item', 'rows_per_item', 'rows', 'clamp_negative', 'flat', 'order', 'offsets',
                                            'ws', 'ws_bytes', 'stream']
    assert _lib.PARAMS['pps_pack_dense_f16x3'] == ['W', 'out', 'in', 'packed'] and _lib.PARAMS['pps_abi_version'] == []
    assert len(_lib.SIGNATURES) == 138


def test_header_parser_names_what_it_cannot_map():
    sig, names = _lib.parse_header('/* int pps_gone(int a); */\nint64_t pps_x(const float* const* a /* [host] */, uint64_t n, void* stream);  // int pps_y(void);')
    assert sig == {'pps_x': (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p])} and names == {'pps_x': ['a', 'n', 'stream']}
    for bad in ('int pps_x(long n);', 'unsigned pps_x(int n);', 'int pps_x(struct foo s);'):
        with pytest.raises(ValueError, match='pps_x'):
            _lib.parse_header(bad)


def test_pack_roundtrip_and_padding():
    rng = np.random.default_rng(0)
    for out, inp in ((256, 256), (64, 256), (128, 64), (2, 256), (4096, 64)):
        w = rng.standard_normal((out, inp)).astype(np.float32)
        p = pack_dense(w)
        assert p.shape[0] == _lib.lib().pps_packed_dense_floats(out, inp) == ((out + 31) // 32 * 32) * ((inp + 15) // 16 * 16)
        assert np.array_equal(emulate.unpack_dense(p, out, inp).astype(np.float32), w)
    w = rng.standard_normal((64, 3)).astype(np.float32)
    assert np.array_equal(emulate.unpack_xyz(pack_xyz(w), 64).astype(np.float32), w)
    # documented A-operand order: packed[ob][kb][l][s] = W[16 ob + (l & 15)][16 kb + 4 (l >> 4) + s]
    w = np.arange(32 * 32, dtype=np.float32).reshape(32, 32)
    p = pack_dense(w).reshape(2, 2, 64, 4)
    assert p[1, 0, 17, 2] == w[16 + 1, 4 * 1 + 2] and p[0, 1, 63, 3] == w[15, 16 + 12 + 3]


def test_folded_weights_reproduce_reference_from_latent():
    g = load_golden('ppsurf_from_latent')
    plan = DecoderPlan(filled_sd('', key='ppsurf'), 'cpu', dtype='f32')
    w = {k: v.numpy() for k, v in plan.w.items()}
    cloud = g['cloud']
    logits, _ = emulate.decode(w, make_latents(256, cloud.shape[0], 77)[0], cloud, g['query'], g['proj_ids'][0], g['patches'])
    np.testing.assert_allclose(logits, g['logits'][0].T, rtol=1e-4, atol=1e-4)
