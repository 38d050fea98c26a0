"""Reader of include/icnn_be.h: the header's constants, structs and prototypes as ctypes objects.

The header is the one statement of the library's contract; _lib.py binds whatever this reader finds in it, so a new entry
costs a header entry and its .hip file.  The reader knows the C the header is written in and no more: object-like
`#define ICNN_BE_<NAME> <integer expression>`, `typedef struct icnn_be_x { ... } icnn_be_x;` and
`ICNN_BE_API <ret> name(<params>);`.  Anything else in those three places is an ImportError that quotes the text -- it
never guesses.
"""
import collections
import ctypes as C
import os
import re

PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "icnn_be.h")

SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "long long": C.c_longlong,
           "unsigned long long": C.c_ulonglong, "unsigned char": C.c_ubyte, "size_t": C.c_size_t}
RETURNS = {"int": C.c_int, "size_t": C.c_size_t, "const char *": C.c_char_p, "void": None}

# name: C name; restype / argtypes: what ctypes takes; params: the declarations as the header writes them
Prototype = collections.namedtuple("Prototype", "name restype argtypes params")
# constants: ICNN_BE_<NAME> -> int; structs: icnn_be_x -> ctypes.Structure class; prototypes: name -> Prototype; each in header order
Header = collections.namedtuple("Header", "constants structs prototypes")

_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(ICNN_BE_\w+)(\([^)\n]*\))?[ \t]*(.*?)[ \t]*$", re.M)
_STRUCT = re.compile(r"\btypedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;")
_PROTOTYPE = re.compile(r"\bICNN_BE_API\s+([\w\s*]*?)(\w+)\s*\(([^()]*)\)\s*;")
_BASE = re.compile(r"unsigned long long\b|long long\b|unsigned char\b|\w*")
_DECLARATOR = re.compile(r"((?:\*\s*)*)(\w+)\s*(?:\[\s*(\w*)\s*\])?$")


def _fail(why, text):
    raise ImportError("icnn_be.h: %s: %r" % (why, " ".join(text.split())))


def strip_comments(text):
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def _split(decl, structs):
    """'const float *p, *q' -> (base ctype or Structure class or None for void / char, [(stars, name, array size), ...]); the array
    size is the text between the brackets: None without brackets, '' for `name[]`"""
    words = " ".join(re.sub(r"\bconst\b", " ", decl).split())
    base = _BASE.match(words).group(0)
    if base not in SCALARS and base not in structs and base not in ("void", "char"):
        _fail("unknown base type", decl)
    out = []
    for part in words[len(base):].split(","):
        m = _DECLARATOR.match(part.strip())
        if not m:
            _fail("cannot split the declarator", decl)
        out.append((m.group(1).count("*"), m.group(2), m.group(3)))
    return SCALARS.get(base) or structs.get(base), out


def _count(size, constants, decl):
    if size.isdigit():
        return int(size)
    if size not in constants:
        _fail("array size is neither a literal nor a constant defined above", decl)
    return constants[size]


def _constants(text):
    constants = {}
    for m in _DEFINE.finditer(text):
        name, params, body = m.groups()
        if params or not body or name == "ICNN_BE_API":          # the function-like macro, the include guard, the export attribute
            continue
        try:
            value = eval(body, {"__builtins__": {}}, dict(constants))     # noqa: S307: names are the constants above, nothing else
        except Exception:
            value = None
        if type(value) is not int:
            _fail("#define is not an integer expression of the constants above it", m.group(0))
        constants[name] = value
    return constants


def _structs(text, constants):
    structs = {}
    for m in _STRUCT.finditer(text):
        tag, body, name = m.groups()
        if tag != name:
            _fail("struct tag and typedef name differ", tag + " / " + name)
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            base, declarators = _split(decl, structs)
            for stars, field, size in declarators:
                if not stars and base is None or size == "":
                    _fail("member of type void or char, or array without a size", decl)
                ctype = C.c_void_p if stars else base
                fields.append((field, ctype * _count(size, constants, decl) if size else ctype))
        structs[name] = type(name, (C.Structure,), {"_fields_": fields, "__doc__": "struct " + name})
    for m in re.finditer(r"\btypedef\s+struct\s+(\w*)", text):
        if m.group(1) not in structs:
            _fail("typedef struct that did not become a class", text[m.start():m.start() + 80])
    return structs


def _argtype(decl, structs, constants):
    base, declarators = _split(decl, structs)
    if len(declarators) != 1:
        _fail("cannot split the declarator", decl)
    (stars, _, size), = declarators
    is_struct = isinstance(base, type) and issubclass(base, C.Structure)
    if size == "":                                                # T name[] is T *name
        stars, size = stars + 1, None
    if size:                                                      # T name[N]: a pointer to an array of N
        if stars or is_struct or base is None:
            _fail("array parameter of a type that is no scalar", decl)
        return C.POINTER(base * _count(size, constants, decl))
    if stars >= 2:
        return C.POINTER(C.c_void_p)
    if stars:
        return C.POINTER(base) if is_struct else C.c_void_p
    if is_struct or base is None:
        _fail("parameter passed by value that is no scalar", decl)
    return base


def _prototypes(text, structs, constants):
    text = _DEFINE.sub(" ", text)                                 # the two `#define ICNN_BE_API` lines
    prototypes, starts, argtypes = {}, set(), {}                 # argtypes: by declaration; `void *stream` comes a hundred times
    for m in _PROTOTYPE.finditer(text):
        ret, name, params = " ".join(m.group(1).split()), m.group(2), m.group(3).strip()
        if ret not in RETURNS:
            _fail("unknown return type", m.group(0))
        if name in prototypes:
            _fail("declared twice", m.group(0))
        decls = [] if params == "void" else [" ".join(p.split()) for p in params.split(",")]
        for d in decls:
            if d not in argtypes:
                argtypes[d] = _argtype(d, structs, constants)
        prototypes[name] = Prototype(name, RETURNS[ret], [argtypes[d] for d in decls], decls)
        starts.add(m.start())
    for m in re.finditer(r"\bICNN_BE_API\b", text):
        if m.start() not in starts:
            _fail("ICNN_BE_API that is no prototype `<ret> name(<params>);`", text[m.start():m.start() + 120])
    return prototypes


def parse(text):
    """Header of a header's text."""
    text = strip_comments(text)
    constants = _constants(text)
    structs = _structs(text, constants)
    return Header(constants, structs, _prototypes(text, structs, constants))


def read(path=PATH):
    """Header of the file at `path` (default: this tree's include/icnn_be.h)."""
    try:
        with open(path) as f:
            text = f.read()
    except OSError as e:
        raise ImportError("cannot read the library's header %s (%s): the binding is made from it" % (path, e.strerror))
    return parse(text)
