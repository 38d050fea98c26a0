"""The binding is read from include/icnn_be.h (icnn_amd/_header.py): the reader on header snippets written by hand -- the
smallest inputs at which it can go wrong, with the expected layouts and signatures typed here --, then the real header and the
built library: every prototype declared, every struct's size the library's own, a few signatures pinned by hand.  No GPU."""
import ctypes as C
import os
import re

import pytest

from icnn_amd import _header, _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = C.POINTER

SNIPPET = """
#define ICNN_BE_API __attribute__((visibility("default")))
#define ICNN_BE_K 4
#define ICNN_BE_BYTES (8 * ICNN_BE_K + 16)   /* uses the one above */
#define ICNN_BE_SCALE(x) (2 * (x))
typedef struct icnn_be_in {
    int a;              /* ; int ghost; */
    double d;
} icnn_be_in;
typedef struct icnn_be_s {
    int a, b[3];
    const float *p, *q;
    float *rows[ICNN_BE_K];
    unsigned char *t;
    unsigned long long seed;
    icnn_be_in in;
    int c;              // one int in front of a double: four bytes of padding
    double x;
    float f;
    size_t z;
    long long n;
} icnn_be_s;

/* an entry that left: ; ICNN_BE_API int fake(void); it must not come back */
ICNN_BE_API int icnn_be_go(const icnn_be_s *s, int out[3],
                           const float *const *w, long long *n,
                           double lr, void *stream);
ICNN_BE_API void f(long long *buf);
ICNN_BE_API const char *g(void);
ICNN_BE_API size_t h(unsigned long long seed, float *const dst[], long long off[ICNN_BE_K]);
"""


def layout(cls):
    return [(name, getattr(cls, name).offset, getattr(cls, name).size) for name, _ in cls._fields_]


def test_snippet_constants_and_structs():
    h = _header.parse(SNIPPET)
    assert h.constants == {"ICNN_BE_K": 4, "ICNN_BE_BYTES": 48}          # not the function-like macro, not ICNN_BE_API
    assert list(h.structs) == ["icnn_be_in", "icnn_be_s"]
    assert layout(h.structs["icnn_be_in"]) == [("a", 0, 4), ("d", 8, 8)] and C.sizeof(h.structs["icnn_be_in"]) == 16
    S = h.structs["icnn_be_s"]
    assert layout(S) == [("a", 0, 4), ("b", 4, 12), ("p", 16, 8), ("q", 24, 8), ("rows", 32, 32), ("t", 64, 8), ("seed", 72, 8),
                         ("in", 80, 16), ("c", 96, 4), ("x", 104, 8), ("f", 112, 4), ("z", 120, 8), ("n", 128, 8)]
    assert C.sizeof(S) == 136
    types = dict(S._fields_)
    assert types["b"] is C.c_int * 3 and types["p"] is C.c_void_p and types["rows"] is C.c_void_p * 4
    assert types["t"] is C.c_void_p and types["seed"] is C.c_ulonglong and types["in"] is h.structs["icnn_be_in"]
    assert types["z"] is C.c_size_t and types["n"] is C.c_longlong and types["f"] is C.c_float


def test_snippet_prototypes():
    h = _header.parse(SNIPPET)
    assert list(h.prototypes) == ["icnn_be_go", "f", "g", "h"]          # the commented-out `fake` is not among them
    go = h.prototypes["icnn_be_go"]
    assert go.argtypes == [P(h.structs["icnn_be_s"]), P(C.c_int * 3), P(C.c_void_p), C.c_void_p, C.c_double, C.c_void_p]
    assert go.restype is C.c_int
    assert go.params == ["const icnn_be_s *s", "int out[3]", "const float *const *w", "long long *n", "double lr", "void *stream"]
    assert (h.prototypes["f"].argtypes, h.prototypes["f"].restype) == ([C.c_void_p], None)
    assert (h.prototypes["g"].argtypes, h.prototypes["g"].restype) == ([], C.c_char_p)
    assert (h.prototypes["h"].argtypes, h.prototypes["h"].restype) == ([C.c_ulonglong, P(C.c_void_p), P(C.c_longlong * 4)], C.c_size_t)


@pytest.mark.parametrize("text, named", [
    ("typedef struct icnn_be_s { int a; short x; } icnn_be_s;", "short x"),
    ("typedef struct icnn_be_s { int a; int (*fn)(int); } icnn_be_s;", "fn"),
    ("typedef struct icnn_be_s { int a[ICNN_BE_NOWHERE]; } icnn_be_s;", "ICNN_BE_NOWHERE"),
    ("typedef struct { int a; } icnn_be_anon;", "typedef struct"),
    ("#define ICNN_BE_X (2 * ICNN_BE_LATER)\n#define ICNN_BE_LATER 1", "ICNN_BE_LATER"),
    ("#define ICNN_BE_X __import__('os')", "__import__"),
    ("ICNN_BE_API int icnn_be_a(int x)\nICNN_BE_API int icnn_be_b(void);", "icnn_be_a(int x)"),       # the semicolon is missing
    ("ICNN_BE_API int icnn_be_a(short x);", "short x"),
    ("ICNN_BE_API int icnn_be_a(int x, y);", "y"),
    ("ICNN_BE_API long icnn_be_a(int x);", "long icnn_be_a"),
    ("ICNN_BE_API int icnn_be_a(int x);\nICNN_BE_API int icnn_be_a(int y);", "icnn_be_a(int y)"),
])
def test_reader_refuses(text, named):
    with pytest.raises(ImportError) as e:
        _header.parse(text)
    assert named in str(e.value)


def test_missing_header_is_an_import_error(tmp_path):
    path = str(tmp_path / "nowhere" / "icnn_be.h")
    with pytest.raises(ImportError) as e:
        _header.read(path)
    assert path in str(e.value)


# ---- the real header and the built library ---------------------------------------------------------------------------------

def real_header():
    text = open(os.path.join(REPO, "include", "icnn_be.h")).read()
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def test_reader_finds_every_declaration_of_the_header():
    text = real_header()
    h = _header.read()
    assert len(h.prototypes) == len(re.findall(r"^\s*ICNN_BE_API\b", text, flags=re.M)) > 100
    assert len(h.structs) == len(re.findall(r"\btypedef\s+struct\b", text)) == len(_lib.STRUCTS) == 18
    assert _lib.EXPORTS == list(h.prototypes)
    assert "ICNN_BE_REPLAY_STAGE_BYTES" not in h.constants and "ICNN_BE_API" not in h.constants
    assert h.constants["ICNN_BE_RL_TD_WORK_BYTES"] == 8 * h.constants["ICNN_BE_RL_TD_MAX_BLOCKS"] + 16
    for name, value in h.constants.items():
        assert getattr(_lib, name[len("ICNN_BE_"):]) == value or name in ("ICNN_BE_NAF_BN_PASSES", "ICNN_BE_NAF_BN_VARS"), name
    assert (len(_lib.NAF_BN_PASSES), len(_lib.NAF_BN_VARS)) == (h.constants["ICNN_BE_NAF_BN_PASSES"], h.constants["ICNN_BE_NAF_BN_VARS"])


def test_struct_size_table_is_the_librarys():
    lib = _lib.load()
    by_index = {which: getattr(_lib, py_name) for py_name, which in _lib.STRUCTS.values()}
    assert sorted(by_index) == list(range(12)) + [13, 14, 16, 18, 20, 22]
    for which in range(24):
        assert lib.icnn_be_struct_size(which) == (C.sizeof(by_index[which]) if which in by_index else 0), which
    for c_name, (py_name, _) in _lib.STRUCTS.items():
        assert getattr(_lib, py_name) is _lib._H.structs[c_name] and getattr(_lib, py_name).__name__ == py_name


def test_every_export_is_declared_on_the_library():
    lib = _lib.load()
    scalars = (C.c_int, C.c_longlong, C.c_ulonglong, C.c_size_t, C.c_float, C.c_double)
    declared = {name: params for name, params in re.findall(r"ICNN_BE_API\s+[\w\s\*]+?\b(icnn_be_\w+)\s*\(([^()]*)\)\s*;", real_header())}
    assert sorted(declared) == sorted(_lib.EXPORTS)
    for name in _lib.EXPORTS:
        fn = getattr(lib, name)
        assert isinstance(fn.argtypes, list) and fn.restype in (None, C.c_int, C.c_size_t, C.c_char_p), name
        params = [] if declared[name].strip() == "void" else declared[name].split(",")
        assert len(fn.argtypes) == len(params), name
        for text, argtype in zip(params, fn.argtypes):
            if "*" in text or "[" in text:
                assert argtype not in scalars, (name, text)          # a 64-bit address never travels as a C int
            else:
                assert argtype in scalars, (name, text)
    for name in ("icnn_be_debug_profile", "icnn_be_debug_profile_fc", "icnn_be_debug_profile_conv", "icnn_be_debug_trace"):
        assert getattr(lib, name).argtypes == [C.c_void_p] and getattr(lib, name).restype is None, name


def test_signatures_pinned_by_hand():
    lib = _lib.load()
    FM, ST, NA, vp, i = P(_lib.FcModel), P(_lib.State), P(_lib.NafArgs), C.c_void_p, C.c_int
    want = {
        "icnn_be_solve_fc": [FM, vp, ST, vp, vp, vp],
        "icnn_be_fc_pack": [FM, P(vp), P(vp), vp],
        "icnn_be_debug_dual_plan": [ST, i, P(C.c_int * 8)],
        "icnn_be_naf_step": [NA, vp],
        "icnn_be_explore": [i, i, vp, i, vp, vp, C.c_double, C.c_double, C.c_ulonglong, i, vp, vp],
    }
    for name, argtypes in want.items():
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is C.c_int, name


def test_declare_names_a_symbol_the_library_lacks():
    class Stale:
        _name = "stale.so"
        icnn_be_abi_version = type("Fn", (), {})()

    _lib.declare(Stale, ["icnn_be_abi_version"])
    assert Stale.icnn_be_abi_version.argtypes == [] and Stale.icnn_be_abi_version.restype is C.c_int
    with pytest.raises(ImportError) as e:
        _lib.declare(Stale)
    assert "icnn_be_last_hip_error" in str(e.value) and "python -m icnn_amd.build" in str(e.value)
