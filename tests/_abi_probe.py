"""include/yv4.h as a C compiler and as its own text see it, for the tests that hold the ctypes mirror (``_lib``) to it.

``probe()`` generates one C program from ``_lib.STRUCTS`` -- ``sizeof`` of every struct, ``offsetof`` and ``sizeof`` of
every field the ctypes classes name, the four ``YV4_*_SHAPE(i)`` macros over their pinned ranges -- compiles it once per
session with the host C compiler against the header and returns what it prints; without a compiler the calling test
skips.  ``header_structs()`` and ``header_constants()`` read the header's text and need no compiler."""
import collections
import ctypes
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from mmdet_yolov4_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, 'include')

Probe = collections.namedtuple('Probe', 'sizeof fields shapes')


@functools.lru_cache(maxsize=None)
def header_text():
    """The header without its comments."""
    text = open(os.path.join(INCLUDE, 'yv4.h')).read()
    return re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', text, flags=re.S))


def header_structs():
    """``{C type name: [member names in declaration order]}`` of every ``typedef struct`` of the header."""
    out = {}
    for body, name in re.findall(r'typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;', header_text(), flags=re.S):
        members = [part for decl in body.split(';') if decl.strip() for part in decl.split(',')]
        out[name] = [re.search(r'(\w+)\s*(?:\[[^\]]*\]\s*)*$', m.strip()).group(1) for m in members]
    return out


def header_constants():
    """``{name without YV4_: value}`` of every object-like ``#define YV4_*`` with a numeric value."""
    out = {}
    for name, expr in re.findall(r'^[ \t]*#[ \t]*define[ \t]+YV4_(\w+)[ \t]+(\S.*?)[ \t]*$', header_text(), flags=re.M):
        assert re.fullmatch(r'[0-9xXa-fA-F\s()<>+*-]+', expr), f'YV4_{name}: not a numeric expression: {expr!r}'
        out[name] = int(eval(expr, {'__builtins__': {}}))      # digits, parentheses and operators only (checked above)
    return out


@functools.lru_cache(maxsize=None)
def probe():
    """-> ``Probe(sizeof {C name: bytes}, fields {(C name, field): (offset, bytes)}, shapes {macro: [values]})``."""
    cc = shutil.which('cc') or shutil.which('gcc')
    if cc is None:
        pytest.skip('no C compiler')
    lines = []
    for cname, cls in _lib.STRUCTS.items():
        lines.append(f'printf("S {cname} - %zu 0\\n", sizeof({cname}));')
        lines += [f'printf("F {cname} {f[0]} %zu %zu\\n", offsetof({cname}, {f[0]}), sizeof((({cname}*)0)->{f[0]}));'
                  for f in cls._fields_]
    for macro, count in _lib.SHAPE_COUNTS.items():
        lines += [f'printf("M {macro} - %d {i}\\n", YV4_{macro}_SHAPE({i}));' for i in range(count)]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "yv4.h"\nint main(void) {\n' + '\n'.join(lines) + '\nreturn 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, 'probe.c'), os.path.join(d, 'probe')
        open(c, 'w').write(src)
        res = subprocess.run([cc, '-I', INCLUDE, c, '-o', exe], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr        # e.g. a ctypes field the header's struct does not have
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    p = Probe({}, {}, collections.defaultdict(list))
    for kind, owner, field, a, b in (line.split() for line in out.splitlines()):
        if kind == 'S':
            p.sizeof[owner] = int(a)
        elif kind == 'F':
            p.fields[owner, field] = (int(a), int(b))
        else:
            p.shapes[owner].append(int(a))
    return p


def mismatches():
    """Every disagreement between the compiler and ctypes over ``_lib.STRUCTS``, as readable lines; empty when the mirror
    is right."""
    p, bad = probe(), []
    for cname, cls in _lib.STRUCTS.items():
        if ctypes.sizeof(cls) != p.sizeof[cname]:
            bad.append(f'sizeof({cname}): header {p.sizeof[cname]}, ctypes {ctypes.sizeof(cls)}')
        for f in cls._fields_:
            d = getattr(cls, f[0])
            if (d.offset, d.size) != p.fields[cname, f[0]]:
                bad.append(f'{cname}.{f[0]}: header (offset, size) {p.fields[cname, f[0]]}, ctypes {(d.offset, d.size)}')
    return bad
