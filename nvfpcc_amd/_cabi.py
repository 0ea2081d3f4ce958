"""Reads a C ABI out of its header: the ctypes binding is computed from include/*.h, not written beside it.

``read(text)`` is a pure function from header text to prototypes, request structs and integer constants.  It
understands the small subset of C the project's headers are written in and raises ``ValueError``, quoting the
declaration, on anything else: it never guesses.  No shared object is loaded here.
"""
import collections
import ctypes as C
import os
import re

INCLUDE = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "include")

SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
           **{f"{u}int{n}_t": getattr(C, f"c_{u}int{n}") for u in ("", "u") for n in (8, 16, 32, 64)}}

Header = collections.namedtuple("Header", "prototypes structs constants")


def _constant(expr, known, line):
    """Value of an integer expression of literals, + - * << ( ) and names defined earlier."""
    operators = ("<<", "+", "-", "*", "(", ")")
    tokens = re.findall(r"0[xX][0-9a-fA-F]+|\d+|[A-Za-z_]\w*|<<|[-+*()]", expr)
    try:
        if not tokens or "".join(tokens) != "".join(expr.split()):
            raise ValueError
        # what reaches eval is made of the operators above and integers: an unknown name or a bad literal raises
        py = " ".join(t if t in operators else str(known[t] if t in known else int(t, 0)) for t in tokens)
        return int(eval(py, {"__builtins__": {}}))
    except (ValueError, SyntaxError, TypeError):
        raise ValueError(f"not an integer expression: {line!r}") from None


def _declarator(text, types, base=None):
    """'const float* const* xs' -> ('float', 2, 'xs', None); 'int32_t n[8]' -> ('int32_t', 0, 'n', 8).
    ``base`` is the type of an earlier declarator of the same line ('float a, b')."""
    tok = re.findall(r"\w+|\S", text)
    count = None
    if tok[-1:] == ["]"] and tok[-3:-2] == ["["] and tok[-2].isdigit():
        count, tok = int(tok[-2]), tok[:-3]
    stars = tok.index("*") if "*" in tok else len(tok) - 1
    words = [t for t in tok[:stars] if t != "const"] or ([base] if base else [])
    rest = [t for t in tok[stars:-1] if t not in ("*", "const")]
    name = tok[-1] if tok else ""
    if len(words) != 1 or words[0] not in types or rest or not re.fullmatch(r"[A-Za-z_]\w*", name) or name in types \
            or name == "const":
        raise ValueError(f"declaration outside the supported C subset: {text.strip()!r}")
    return words[0], tok.count("*"), name, count


def _ctype(base, stars, count, types, text, field):
    """Pointers are c_void_p (callers pass addresses); a scalar is its ctypes twin; T name[N] is T * N in a struct
    and an address as a parameter."""
    t = C.c_void_p if stars else types[base]
    if not isinstance(t, type):     # void, an opaque type or a struct by value
        raise ValueError(f"{base} by value is outside the supported C subset: {text.strip()!r}")
    if count is not None:
        t = t * count if field else C.c_void_p
    return t


def read(text):
    """Header text -> Header(prototypes {name: (restype, [argtypes])}, structs {name: Structure class},
    constants {NAME: int})."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    constants, code = {}, []
    for line in text.splitlines():
        if not line.lstrip().startswith("#"):
            code.append(line)
            continue
        if line.rstrip().endswith("\\"):
            raise ValueError(f"continued preprocessor line: {line!r}")
        m = re.match(r"\s*#\s*define\s+(\w+)(\(?)(.*)", line)
        if m and not m.group(2) and m.group(3).strip():      # not function-like, not an include guard
            constants[m.group(1)] = _constant(m.group(3), constants, line.strip())
    text, k = re.subn(r'extern\s+"C"\s*\{', " ", "\n".join(code))
    text = " ".join(text.rsplit("}", k))
    types = dict(SCALARS, void=None)      # None: void, opaque types and structs may only be pointed to
    structs = {}

    def typedef(m):
        name, body, alias = m.groups()
        if name != alias:
            raise ValueError(f"struct {name} is given another name: {' '.join(m.group(0).split())!r}")
        types[name] = None
        if body is not None:
            fields = []
            for decl in filter(str.strip, body.split(";")):
                base = None
                for part in decl.split(","):
                    base, stars, field, count = _declarator(part, types, base)
                    fields.append((field, _ctype(base, stars, count, types, decl, True)))
            structs[name] = type(name, (C.Structure,), {"_fields_": fields, "__doc__": f"typedef struct {name}."})
        return " "

    text = re.sub(r"typedef\s+struct\s+(\w+)\s*(?:\{([^{}]*)\})?\s*(\w+)\s*;", typedef, text)

    prototypes = {}
    *statements, tail = text.split(";")
    if tail.strip():
        raise ValueError(f"unfinished declaration: {tail.strip()!r}")
    for st in filter(str.strip, statements):
        m = re.fullmatch(r"\s*(.*?\bnvf_\w+)\s*\((.*)\)\s*", st, flags=re.S)
        base, stars, name, count = _declarator(m.group(1), types) if m else (None, 1, None, None)
        if stars or count is not None or "{" in st or "}" in st:      # no nvf_* function, or one that returns a pointer
            raise ValueError(f"declaration outside the supported C subset: {' '.join(st.split())!r}")
        res = None if base == "void" else _ctype(base, 0, None, types, st, False)
        params = m.group(2).strip()
        args = [] if params == "void" else [_ctype(b, s, c, types, p, False)
                                            for p in params.split(",") for b, s, _, c in [_declarator(p, types)]]
        prototypes[name] = (res, args)
    return Header(prototypes, structs, constants)


def read_header(name):
    """The parsed include/<name> of this tree (not of wherever a library under test was built)."""
    with open(os.path.join(INCLUDE, name)) as f:
        return read(f.read())


def bind(handle, prototypes):
    """Set restype / argtypes of every prototype on a loaded library; AttributeError if the library lacks one."""
    for name, (res, args) in prototypes.items():
        fn = getattr(handle, name)
        fn.restype = res
        fn.argtypes = args
    return handle
