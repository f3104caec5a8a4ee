"""The header reader (hd_yolo_amd/_header.py) on small header texts written here, one construct each, every strictness rule with the symbol it
must name; then the structures and macros it reads from the real include/hdyolo.h against the C compiler's own sizeof / offsetof / values.
Host only: nothing here loads the library or touches a GPU."""
import ctypes
import os
import subprocess
from ctypes import c_char_p, c_double, c_float, c_int, c_longlong, c_size_t, c_uint, c_ulonglong, c_void_p

import pytest

from hd_yolo_amd import _header
from hd_yolo_amd._header import HdyError, parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ functions
def test_prototype_wrapped_over_three_lines():
    h = parse('int hdy_foo(const void* x, int ldx,\n'
              '            float* const* out,\n'
              '            size_t n, void* stream);\n')
    assert h.functions == {'hdy_foo': (c_int, [c_void_p, c_int, c_void_p, c_size_t, c_void_p])}
    assert h.params['hdy_foo'] == [('x', True), ('ldx', False), ('out', False), ('n', False), ('stream', False)]


def test_char_pointers_void_and_every_scalar():
    h = parse('typedef struct hdy_d { int n; } hdy_d;\n'
              'const char* hdy_name(void);\n'
              'void hdy_reset(void);\n'
              'int hdy_set(const char* name, int value);\n'
              'size_t hdy_all(int a, unsigned b, long long c, unsigned long long d, size_t e, float f, double g);\n'
              'int hdy_ptrs(hdy_d* descs, const hdy_d* more, unsigned* magic, int* shift, const unsigned long long* program, const uint16_t* m,\n'
              '             unsigned char* idx, unsigned short* hit, const long long* labels, double* sums);\n')
    assert h.functions['hdy_name'] == (c_char_p, []) and h.functions['hdy_reset'] == (None, [])
    assert h.functions['hdy_set'] == (c_int, [c_char_p, c_int]) and h.params['hdy_set'] == [('name', True), ('value', False)]
    assert h.functions['hdy_all'] == (c_size_t, [c_int, c_uint, c_longlong, c_ulonglong, c_size_t, c_float, c_double])
    assert h.functions['hdy_ptrs'] == (c_int, [c_void_p] * 10)
    assert list(h.functions) == ['hdy_name', 'hdy_reset', 'hdy_set', 'hdy_all', 'hdy_ptrs']


def test_comments_and_preprocessor_lines_declare_nothing():
    h = parse('/* hdy_foo( looks like a call; and ends like a statement;\n'
              ' * int hdy_ghost(int a); */\n'
              '#ifndef T_H\n#define T_H\n#include <stddef.h>\n'
              '#ifdef __cplusplus\nextern "C" {\n#endif\n'
              'int hdy_real(int a); /* trailing; hdy_other( */\n'
              '// int hdy_line(int a);\n'
              '#ifdef __cplusplus\n}\n#endif\n#endif /* T_H */\n')
    assert h.functions == {'hdy_real': (c_int, [c_int])} and h.constants == {} and h.structs == {}


# ------------------------------------------------------------------------------------------ structures
def test_struct_body_forms():
    h = parse('typedef struct hdy_tagged {\n'
              '    const float* w_a;\n'
              '    void* out;\n'
              '    int K_a, K_b, Kl;        /* several declarators in one statement */\n'
              '    long long n;\n'
              '    int pad_;\n'
              '} hdy_tagged;\n'
              'typedef struct {\n'
              '    const void* y; int ldy;  /* two statements on one line */\n'
              '    const float *scale, *shift;\n'
              '    float* slabs;\n'
              '    float eps;\n'
              '} hdy_anon;\n')
    t, a = h.structs['hdy_tagged'], h.structs['hdy_anon']
    assert issubclass(t, ctypes.Structure) and list(h.structs) == ['hdy_tagged', 'hdy_anon']
    assert t._fields_ == [('w_a', c_void_p), ('out', c_void_p), ('K_a', c_int), ('K_b', c_int), ('Kl', c_int), ('n', c_longlong), ('pad_', c_int)]
    assert a._fields_ == [('y', c_void_p), ('ldy', c_int), ('scale', c_void_p), ('shift', c_void_p), ('slabs', c_void_p), ('eps', c_float)]
    assert ctypes.sizeof(t) == 48 and t.n.offset == 32 and ctypes.sizeof(a) == 48 and a.scale.offset == 16


# ------------------------------------------------------------------------------------------ constants
def test_macro_value_forms():
    h = parse('#define HDY_DEC 864\n'
              '#define HDY_ZERO 0   /* with a comment */\n'
              '#define HDY_HEX 0xF0F0F0F1ull\n'
              '#define HDY_U 7u\n'
              '#define HDY_LL 5LL\n'
              '#define HDY_SHIFT (1 << 24)\n'
              '#define HDY_SHIFT_LL (1LL << 30)\n'
              '#define OTHER_GUARD_H\n'
              '#define OTHER_VALUE 1.5f\n')
    assert h.constants == {'HDY_DEC': 864, 'HDY_ZERO': 0, 'HDY_HEX': 0xF0F0F0F1, 'HDY_U': 7, 'HDY_LL': 5, 'HDY_SHIFT': 1 << 24, 'HDY_SHIFT_LL': 1 << 30}
    assert all(type(v) is int for v in h.constants.values())


# ------------------------------------------------------------------------------------------ strictness
@pytest.mark.parametrize('text, named', [
    ('int hdy_f(int n, short k);', r'hdy_f, k.*short'),                                       # unknown type word
    ('int hdy_f(unsigned int n);', r'hdy_f, n.*unsigned int'),                                # a spelling the scalar table does not hold
    ('long hdy_f(int n);', r'hdy_f.*long'),                                                   # ... as a return type
    ('int hdy_f(hdy_nowhere* d);', r'hdy_f, d.*hdy_nowhere'),                                 # a pointer to something never declared
    ('int hdy_f(int a[4]);', r'hdy_f.*a\[4\]'),                                               # array parameter
    ('int hdy_f(const float x[], int n);', r'hdy_f.*x\[\]'),
    ('int hdy_f(void (*done)(int), void* stream);', r'hdy_f.*\(\*done\)'),                    # callback parameter
    ('int hdy_f(int);', r'hdy_f.*int'),                                                       # a parameter without a name
    ('int hdy_f();', r'hdy_f'),                                                               # an old-style empty list says nothing about the arguments
    ('typedef struct hdy_s { int n; int a[4]; } hdy_s;', r'hdy_s.*a\[4\]'),                   # array member
    ('typedef struct hdy_in { int n; } hdy_in;\ntypedef struct hdy_s { hdy_in inner; } hdy_s;', r'hdy_s, inner.*hdy_in'),   # nested struct member
    ('typedef struct hdy_s { int n; struct { int b; } inner; } hdy_s;', r'hdy_s'),            # ... declared in place
    ('typedef struct hdy_s { void (*cb)(int); } hdy_s;', r'hdy_s.*cb'),                       # function-pointer member
    ('typedef struct hdy_s { short k; } hdy_s;', r'hdy_s, k.*short'),
    ('#define HDY_X 1.5f', r'HDY_X.*1\.5f'),                                                  # not an integer
    ('#define HDY_X 1\n#define HDY_Y (HDY_X + 1)', r'HDY_Y.*HDY_X \+ 1'),                     # not one of the integer forms
    ('#define HDY_MAX(a, b) ((a) > (b) ? (a) : (b))', r'HDY_MAX'),                            # function-like macro
    ('#define HDY_OCT 010', r'HDY_OCT.*010'),
    ('int hdy_count;', r'hdy_count'),                                                         # a variable: neither prototype nor structure
    ('enum hdy_e { A, B };', r'hdy_e'),
])
def test_what_the_reader_cannot_classify_raises_with_the_symbol(text, named):
    with pytest.raises(HdyError, match=named):
        parse(text)


def test_missing_header_says_where_it_was_looked_for(tmp_path):
    path = str(tmp_path / 'include' / 'hdyolo.h')
    with pytest.raises(HdyError, match='include/hdyolo.h is missing'):
        _header.read(path)


# ------------------------------------------------------------------------------------------ the real header against the compiler
def test_structures_and_macros_agree_with_the_compiler(tmp_path):
    """A C program that includes hdyolo.h prints sizeof and every offsetof of every structure the reader found, and every macro as long long;
    compiled as host C by the compiler hd_yolo_amd/build.py uses (no offload architecture, no HIP runtime) and compared with ctypes."""
    h = _header.read()
    assert len(h.structs) == 5 and len(h.constants) == 25 and len(h.functions) == 110
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hdyolo.h"', 'int main(void) {']
    for name, cls in h.structs.items():
        lines.append(f'    printf("{name} sizeof %zu\\n", sizeof({name}));')
        lines += [f'    printf("{name} {f} %zu\\n", offsetof({name}, {f}));' for f, _ in cls._fields_]
    lines += [f'    printf("{name} value %lld\\n", (long long)({name}));' for name in h.constants]
    lines += ['    return 0;', '}']
    src, exe = tmp_path / 'layout.c', tmp_path / 'layout'
    src.write_text('\n'.join(lines) + '\n')
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    subprocess.run([hipcc, '-x', 'c', '-std=c11', '-Wall', '-Werror', '-I' + os.path.join(ROOT, 'include'), str(src), '-o', str(exe)],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {tuple(line.split()[:2]): int(line.split()[2]) for line in out.splitlines()}
    want = {}
    for name, cls in h.structs.items():
        want[(name, 'sizeof')] = ctypes.sizeof(cls)
        for f, _ in cls._fields_:
            want[(name, f)] = getattr(cls, f).offset
    for name, v in h.constants.items():
        want[(name, 'value')] = v
    assert got == want
    assert [ctypes.sizeof(c) for c in h.structs.values()] == [104, 56, 56, 24, 64]      # header order: pack, stat_req, bn_eval, roi_level, opt
