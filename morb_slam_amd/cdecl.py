"""Reader of the C declarations of include/morb_hip.h: the prototypes as ctypes signatures, the records as aligned numpy dtypes, the
MORB_* integer constants.  It reads the plain C the header is written in — prototypes, `typedef struct` records of scalars and
fixed-size arrays, forward typedefs, `#define NAME integer` — and never guesses: anything else raises ValueError naming the
declaration."""
import collections
import ctypes as C
import re

import numpy as np

Header = collections.namedtuple("Header", "prototypes records constants structures")

_SCALARS = {"int": C.c_int, "int32_t": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}
_POINTEES = set(_SCALARS) | {"void", "char", "unsigned char", "uint8_t"}
_DIRECTIVE = re.compile(r"\s*#\s*(include\b|ifndef\b|endif\b|define\b|ifdef\s+__cplusplus\s*$|pragma\s+once\s*$)")
_STATEMENT = r"(?:[^;{}]|\{[^{}]*\})*;"
_TYPE = r"(?:unsigned\s+char|[A-Za-z_]\w*)"
_PARAM = re.compile(rf"(const\s+)?({_TYPE})\s*(\**)\s*(?:const\s+)?(?:[A-Za-z_]\w*)?")
_PROTOTYPE = re.compile(rf"((?:const\s+)?{_TYPE}\s*\**)\s*\b([A-Za-z_]\w*)\s*\((.*)\)")
_RECORD = re.compile(r"typedef\s+struct\b\s*(\w*)\s*\{(.*)\}\s*(\w+)")
_FORWARD = re.compile(r"typedef\s+struct\s+(\w+)\s+(\w+)")
_FIELD = re.compile(r"([A-Za-z_]\w*)\s*(?:\[\s*(\d+)\s*\])?")


def _statements(text):
    """The header's declarations, one string each with single blanks, and its `#define NAME value` pairs."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", lambda m: " " + "\n" * m.group(0).count("\n"), text, flags=re.S)   # comments out, lines kept
    for line in re.findall(r"^[ \t]*#.*$", text, flags=re.M):
        if not _DIRECTIVE.match(line):
            raise ValueError(f"preprocessor line not understood: {line.strip()}")
    defines = dict(re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\S.*?)[ \t]*$", text, flags=re.M))
    code, nlinkage = re.subn(r'\bextern\s+"C"\s*\{', " ", re.sub(r"^[ \t]*#.*$", "", text, flags=re.M))
    rest = re.sub(_STATEMENT, "", code).split()
    if rest != ["}"] * nlinkage:     # beside the declarations there is only the brace that closes each `extern "C" {`
        raise ValueError(f"declaration not understood: {' '.join(rest)[:160]}")
    return [" ".join(s[:-1].split()) for s in re.findall(_STATEMENT, code)], defines


def _fields(decl, body):
    """[(name, ctypes scalar, () or (length,))] of a record's body."""
    out = []
    for member in filter(None, (s.strip() for s in body.split(";"))):
        m = re.fullmatch(rf"({_TYPE})\s+(.*)", member)
        items = [_FIELD.fullmatch(item.strip()) for item in m.group(2).split(",")] if m and m.group(1) in _SCALARS else [None]
        if not all(items):
            raise ValueError(f"field {member!r} not understood in declaration: {decl}")
        out += [(f.group(1), _SCALARS[m.group(1)], (int(f.group(2)),) if f.group(2) else ()) for f in items]
    return out


def _ctype(decl, text, h, opaque, ret=False):
    m = _PARAM.fullmatch(text.strip())
    const, base, stars = m.groups() if m else (None, "", "")
    if not stars and base in _SCALARS:
        return _SCALARS[base]
    if not stars and base == "void" and ret:
        return None
    if stars and (base in _POINTEES or base in opaque or base in h.records):
        if const and base == "char" and stars == "*":
            return C.c_char_p
        return C.POINTER(h.structures[base]) if base in h.structures and stars == "*" else C.c_void_p
    raise ValueError(f"type {text.strip()!r} not understood in declaration: {decl}")


def parse(text, structures=()):
    """Header(prototypes {name: (restype, [argtypes])}, records {name: numpy dtype, align=True}, constants {NAME: int},
    structures {name: ctypes.Structure}) of a header's text.  `structures` names the records that also get a ctypes.Structure; a
    pointer to one of them is POINTER(thatStructure) in the signatures, `const char*` is c_char_p, every other pointer c_void_p."""
    statements, defines = _statements(text)
    h, opaque = Header({}, {}, {}, {}), set()
    for name, value in defines.items():
        m = re.fullmatch(r"\(\s*(-?\d+)\s*\)|(-?\d+)", value)
        if name.startswith("MORB_") and not m:
            raise ValueError(f"#define {name} {value}: not an integer constant")
        if name.startswith("MORB_"):
            h.constants[name] = int(m.group(1) or m.group(2))
    for decl in statements:
        r, f, p = _RECORD.fullmatch(decl), _FORWARD.fullmatch(decl), _PROTOTYPE.fullmatch(decl)
        if r and r.group(1) in ("", r.group(3)):
            name, fields = r.group(3), _fields(decl, r.group(2))
            h.records[name] = np.dtype([(n, np.dtype(t), dims) for n, t, dims in fields], align=True)
            if name in structures:
                h.structures[name] = type(name, (C.Structure,), {"_fields_": [(n, t * dims[0] if dims else t) for n, t, dims in fields]})
        elif f and f.group(1) == f.group(2):
            opaque.add(f.group(1))
        elif p and not decl.startswith("typedef") and p.group(2) not in h.prototypes:
            params = [] if p.group(3).strip() == "void" else p.group(3).split(",")
            h.prototypes[p.group(2)] = (_ctype(decl, p.group(1), h, opaque, ret=True), [_ctype(decl, a, h, opaque) for a in params])
        else:
            raise ValueError(f"declaration not understood: {decl}")
    return h
