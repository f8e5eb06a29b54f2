"""qtos_amd.abi, the ctypes mirror of include/qtos_planner.h, held to the header as a whole (no GPU): every structure's size and
every field's name, offset and size, every #define's value, and every declaration's arguments and return value against
abi.PROTOTYPES.  The header is read with regular expressions -- its comments are /* */, every declaration starts a line -- and
one generated C program, compiled with cc against the header itself, prints the layouts and the constants."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "qtos_planner.h")
SCALAR = r"(?:unsigned\s+)?(?:long\s+long|int|double|char|void)"
# sizes that other tests, the documents or C callers pin as literals
SIZES = {"QtosStitch": 32, "QtosPathPlan": 72, "QtosTerrainEnv": 40, "QtosSelftest": 72, "QtosParams": 1448, "QtosDims": 128,
         "QtosCheckRecord": 24, "QtosPathGoal": 112, "QtosHandover": 120,
         "QtosForceFit": 8 + 4 + 4 + 8 + 8 + 4 * 8 + 4 * 8 + 12 * 8 + 4 * 8 + 2 * 8 + 4 * 8 + 8}


@pytest.fixture(scope="module")
def abi():
    from qtos_amd import abi
    return abi


@pytest.fixture(scope="module")
def header():
    """The header without its comments."""
    return re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)


def structures(abi):
    return {name: cls for name, cls in vars(abi).items()
            if isinstance(cls, type) and issubclass(cls, C.Structure) and not name.startswith("_")}


@pytest.fixture(scope="module")
def printed(abi, header, tmp_path_factory):
    """What the C compiler makes of the header: {"QtosX": (sizeof, 0), "QtosX.field": (offset, size), "QTOS_Y": (value, 0)}."""
    lines = []
    for name, cls in sorted(structures(abi).items()):
        lines.append('  printf("%s %%lld 0\\n", (long long)sizeof(%s));' % (name, name))
        for f, _ in cls._fields_:
            lines.append('  printf("%s.%s %%lld %%lld\\n", (long long)offsetof(%s, %s), (long long)sizeof(((%s *)0)->%s));'
                         % (name, f, name, f, name, f))
    for name in defines(header):
        lines.append('  printf("%s %%lld 0\\n", (long long)(%s));' % (name, name))
    d = tmp_path_factory.mktemp("abi")
    src, exe = d / "abi_layout.c", d / "abi_layout"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "qtos_planner.h"\nint main(void) {\n' + "\n".join(lines)
                   + "\n  return 0;\n}\n")
    r = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return {t[0]: (int(t[1]), int(t[2])) for t in (ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())}


def defines(header):
    return [n for n in re.findall(r"^#define\s+(QTOS_\w+)", header, flags=re.M) if n != "QTOS_PLANNER_H"]


def header_fields(header, name):
    """The field names of `typedef struct name { ... } name;` in order."""
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), header, flags=re.S).group(1)
    names = []
    for stmt in filter(None, (s.strip() for s in body.split(";"))):
        m = re.match(r"%s\s+(.*)$" % SCALAR, stmt, flags=re.S)
        assert m, (name, stmt)
        names += [re.match(r"\s*(\w+)", decl).group(1) for decl in m.group(1).split(",")]
    return names


def test_every_structure_has_the_headers_layout(abi, header, printed):
    in_header = re.findall(r"^\}\s*(Qtos\w+)\s*;", header, flags=re.M)        # (the opaque QtosPlanner has no body)
    mirrored = structures(abi)
    assert len(in_header) >= 17 and sorted(in_header) == sorted(mirrored)
    for name, cls in mirrored.items():
        fields = [f for f, _ in cls._fields_]
        assert fields == header_fields(header, name), name
        assert printed[name][0] == C.sizeof(cls), name
        for f in fields:
            assert printed["%s.%s" % (name, f)] == (getattr(cls, f).offset, getattr(cls, f).size), (name, f)
        assert type(cls().copy()) is cls
    for name, size in SIZES.items():
        assert C.sizeof(mirrored[name]) == size, name


def test_every_define_is_a_constant_with_its_value(abi, header, printed):
    names = defines(header)
    assert len(names) >= 26 and sorted(names) == sorted(abi.CONSTANTS)
    for n in names:
        assert printed[n][0] == abi.CONSTANTS[n] == getattr(abi, n[len("QTOS_"):]), n


def c_kind(text):
    """pointer, void, int, double, long long or unsigned long long of a C parameter or return type (a name may follow)."""
    if "*" in text:
        return "pointer"
    m = re.match(r"\s*(?:const\s+)?(%s)\b" % SCALAR, text)
    assert m, text
    return " ".join(m.group(1).split())


def ctypes_kind(t):
    if t is None:
        return "void"
    if issubclass(t, C._Pointer) or t in (C.c_void_p, C.c_char_p):
        return "pointer"
    return {C.c_int: "int", C.c_double: "double", C.c_longlong: "long long", C.c_ulonglong: "unsigned long long"}[t]


def test_every_declaration_has_its_prototype(abi, header):
    decls = re.findall(r"^((?:const\s+)?%s\s*\**)\s*(qtos_\w+)\s*\(([^()]*)\)\s*;" % SCALAR, header, flags=re.M)
    names = [name for _, name, _ in decls]
    assert len(names) >= 80 and len(set(names)) == len(names)
    assert sorted(names) == sorted(set(re.findall(r"\b(qtos_\w+)\s*\(", header)))      # (the pattern above misses none)
    assert sorted(names) == sorted(abi.PROTOTYPES) == sorted(abi.EXPORTS)
    for ret, name, params in decls:
        restype, argtypes = abi.PROTOTYPES[name]
        want = [c_kind(p) for p in params.split(",") if p.strip() != "void"]
        assert [ctypes_kind(t) for t in argtypes] == want, name
        if c_kind(ret) == "pointer":
            assert restype is C.c_char_p and re.match(r"const\s+char\s*\*$", ret.strip()), name
        else:
            assert ctypes_kind(restype) == c_kind(ret), name
