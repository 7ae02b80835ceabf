"""CPU-side checks of the drop-in boundary: the C-ABI library builds for gfx950, loads, and exports every
symbol include/yolo2_hip.h declares; the product refuses CPU tensors (no fallback)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

import _hip
from _hip import c_int


@pytest.fixture(scope='module')
def built():
    if not os.path.exists(_hip.LIB_PATH):
        _hip.build()
    return _hip.LIB_PATH


def declared_symbols():
    text = open(os.path.join(ROOT, 'include', 'yolo2_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(y2_[a-z0-9_]+)\s*\(', text)))


def test_library_exports_every_declared_symbol(built):
    l = ctypes.CDLL(built)
    names = declared_symbols()
    assert len(names) >= 13
    for name in names:
        assert hasattr(l, name), name
    # and the Python binding knows every compute entry point
    for name in names:
        assert name in _hip.SIGNATURES or name == 'y2_build_info', name


def test_version_and_build_info(built):
    l = _hip.lib()
    assert l.y2_abi_version() == 2
    assert b'gfx950' in l.y2_build_info()


def test_conv_params_struct_layout():
    # 7 pointers + 12 int32 + 1 float + 1 int32 (112 bytes, 8-aligned) + workspace pointer + int64 size + residual pointer + 7 int32 (+ pad) + int64 w_plane
    assert ctypes.sizeof(_hip.ConvParams) == 176


# ---- the hand-written ctypes tables of _hip.py against the header, argument by argument (a wrong c_int / c_longlong / c_double corrupts a call silently)
C_TYPES = {'int': ('int', 4), 'int32_t': ('int', 4), 'long long': ('int', 8), 'int64_t': ('int', 8), 'float': ('float', 4), 'double': ('float', 8)}
POINTER = ('pointer', 8)


def header_text():
    text = open(os.path.join(ROOT, 'include', 'yolo2_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    return re.sub(r'//[^\n]*', ' ', text)


def c_kind(ctype):
    """(kind, bytes) of a C type as the header spells it; an unknown one is an error, not a skip."""
    t = ' '.join(ctype.replace('const', ' ').split())
    if '*' in t or t == 'y2_stream_t':
        return POINTER
    assert t in C_TYPES, 'the prototype parser does not know the type %r' % ctype
    return C_TYPES[t]


def py_kind(ctype):
    if ctype in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(ctype, ctypes._Pointer):
        return POINTER
    code = ctype._type_
    assert code in 'ilqfd', ctype
    return ('float' if code in 'fd' else 'int', ctypes.sizeof(ctype))


def prototypes():
    """name -> (return type, [argument kinds]) of every function the header declares."""
    out = {}
    for ret, name, args in re.findall(r'\b(int|long long|const char\s*\*)\s*(y2_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', header_text()):
        args = [a.strip() for a in args.split(',')] if args.strip() not in ('', 'void') else []
        kinds = []
        for a in args:
            m = re.match(r'^(.*?)([A-Za-z_][A-Za-z0-9_]*)$', a)          # the type, then the parameter's name
            assert m and m.group(1).strip(), 'cannot split the parameter %r of %s' % (a, name)
            kinds.append(c_kind(m.group(1)))
        assert name not in out, name
        out[name] = (' '.join(ret.split()), kinds)
    return out


def test_signatures_match_the_prototypes(built):
    protos = prototypes()
    assert sorted(protos) == declared_symbols() and len(protos) >= 96          # every declared function was parsed as a prototype
    assert set(protos) - set(_hip.SIGNATURES) == {'y2_build_info'} and not set(_hip.SIGNATURES) - set(protos)
    assert protos['y2_build_info'] == ('const char *', []) or protos['y2_build_info'] == ('const char*', [])
    for name, argtypes in _hip.SIGNATURES.items():
        want = protos[name][1]
        got = [py_kind(t) for t in argtypes]
        assert len(got) == len(want), '%s: %d arguments declared, %d in SIGNATURES' % (name, len(want), len(got))
        wrong = [(i, w, g) for i, (w, g) in enumerate(zip(want, got)) if w != g]
        assert not wrong, '%s: argument %d is %s in the header, %s in SIGNATURES' % ((name,) + wrong[0])
    l = _hip.lib()
    assert {n for n, (ret, _) in protos.items() if ret == 'long long'} == {n for n in _hip.SIGNATURES if getattr(l, n).restype is ctypes.c_longlong}
    assert all(getattr(l, n).restype is c_int for n, (ret, _) in protos.items() if ret == 'int') and l.y2_build_info.restype is ctypes.c_char_p


def test_the_parser_refuses_a_type_it_does_not_know():
    assert c_kind('const float* ') == POINTER and c_kind('y2_stream_t ') == POINTER and c_kind('long long ') == ('int', 8) and c_kind('int32_t ') == ('int', 4)
    with pytest.raises(AssertionError, match='does not know'):
        c_kind('size_t ')
    assert py_kind(ctypes.c_longlong) == py_kind(ctypes.c_int64) == ('int', 8) and py_kind(ctypes.POINTER(_hip.PrepItem)) == POINTER and py_kind(c_int) != py_kind(ctypes.c_longlong)


def header_structs():
    """name -> [(member, kind)] of every struct the header defines."""
    out = {}
    for body, name in re.findall(r'typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;', header_text(), flags=re.S):
        members = []
        for decl in [d.strip() for d in body.split(';') if d.strip()]:
            m = re.match(r'^(.*?)([A-Za-z_][A-Za-z0-9_]*(?:\s*,\s*[A-Za-z_][A-Za-z0-9_]*)*)$', decl, flags=re.S)          # the type, then one or more names
            assert m and m.group(1).strip(), decl
            members += [(n.strip(), c_kind(m.group(1))) for n in m.group(2).split(',')]
        out[name] = members
    return out


def test_struct_mirrors_have_the_headers_layout():
    structs = header_structs()
    for cname, mirror in (('y2_conv_params', _hip.ConvParams), ('y2_opt_tensor', _hip.OptTensor), ('y2_prep_item', _hip.PrepItem), ('y2_multi_item', _hip.MultiItem)):
        offset, align, offsets = 0, 1, {}
        for member, (kind, size) in structs[cname]:          # natural alignment, as the C ABI lays the struct out
            offset = (offset + size - 1) // size * size
            offsets[member], offset, align = offset, offset + size, max(align, size)
        assert ctypes.sizeof(mirror) == (offset + align - 1) // align * align, cname
        assert [(n, getattr(mirror, n).offset, py_kind(t)) for n, t in mirror._fields_] == [(n, offsets[n], k) for n, k in structs[cname]], cname


def test_mirrored_defines_equal_the_headers():
    defines = {n: int(v) for n, v in re.findall(r'#define\s+(Y2_[A-Z0-9_]+)\s+\(?(-?\d+)\)?', header_text())}
    groups = [n for n in defines if n.startswith(('Y2_PREP_', 'Y2_MULTI_', 'Y2_ALGO_')) and not n.endswith('_MAX_ITEMS')]          # (the item limits are the library's own)
    assert len([n for n in groups if n.startswith('Y2_ALGO_')]) == 8 and len(groups) == 16
    for name in groups + ['Y2_STATS_REPL', 'Y2_EVAL_MATCH_MAX_G', 'Y2_COLLATE_MAX_W', 'Y2_WARP_MAX_DIM', 'Y2_JITTER_MAX_BLUR', 'Y2_JPEG_MAX_DIM', 'Y2_JPEG_DESC_BYTES',
                          'Y2_KMEANS_MAX_K', 'Y2_OPT_MAX_TENSORS']:
        assert getattr(_hip, name[3:]) == defines[name], name
    assert sorted(getattr(_hip, n[3:]) for n in groups if n.startswith('Y2_ALGO_')) == list(range(8))


def test_no_cpu_fallback_on_the_gpu_path():
    """The convolution / decode / loss path refuses CPU tensors (only nms and the IoU helpers have host entry points, because
    the reference calls those on CPU tensors: train.py:209, utils/iou/torch.py:64-113)."""
    import configparser

    import detect
    import model
    import model.yolo2
    cfg = configparser.ConfigParser()
    cfg.read_dict({'batch_norm': {'enable': '1'}})
    anchors = torch.ones(5, 2)
    dnn = model.yolo2.Darknet(model.ConfigChannels(cfg), anchors, 20).eval()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        dnn(torch.zeros(1, 3, 32, 32))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        model.decode(torch.zeros(1, 1, 1, 125), anchors, 5)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        detect.filter_visible_batch(torch.zeros(1, 5), torch.zeros(1, 5), True, 0.005)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_hip, '_lib', None)
    monkeypatch.setattr(_hip, 'LIB_PATH', str(tmp_path / 'nope.so'))
    with pytest.raises(_hip.HipLibraryMissing):
        _hip.lib()
