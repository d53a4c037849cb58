"""Reader of include/agnn.h: the constants, struct layouts and prototypes of the C-ABI as ctypes objects, so that the binding
(_lib.py) holds no second copy of them.  It accepts exactly the forms the header uses and refuses everything else: a
declaration it does not understand stops the import, it is never silently absent.  `re` and `ctypes` only, no GPU.

Pointer rule.  In a struct every pointer member is c_void_p.  In a prototype a pointer to a declared struct is
POINTER(struct); a parameter followed by a comment that begins with `(host)` is a host array the library reads during the call:
POINTER(scalar), or POINTER(c_void_p) for an array of pointers; every other pointer is c_void_p (device memory, workspaces)."""
from __future__ import annotations

import ctypes as C
import os
import re

HEADER_PATH = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "agnn.h"))


class AgnnError(RuntimeError):
    pass


SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
           "uint8_t": C.c_uint8, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
STREAM = "agnn_stream_t"
_SKIPPED_DEFINES = ("AGNN_H_",)          # the include guard; the __cplusplus lines are no #define
_HOST = "@host"                          # what a `/* (host) ... */` comment becomes; no C token looks like it

_INT = r"(?:\(\s*([+-]?\d+)[uU]?\s*\)|([+-]?\d+)[uU]?)"
_DEFINE = re.compile(r"#\s*define\s+(\w+)\s*(.*)")
_STREAM_T = re.compile(r"typedef\s+void\s*\*\s*" + STREAM + r"\s*;")
_STRUCT = re.compile(r"typedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;")
_PROTO = re.compile(r"([\w\s\*]+?)\b(agnn_\w+)\s*\(([^(){};]*)\)\s*;")
_DECL = re.compile(r"(?:const\s+)?(\w+)\s*((?:\*\s*(?:const\b\s*)?)*)(\w+)\s*(?:\[([^\]]*)\])?")
_MORE = re.compile(r"(\w+)\s*(?:\[([^\]]*)\])?")      # `int64_t ld, ld_c;`: the names after the first share its type
_DIM = re.compile(r"(\d+|[A-Za-z_]\w*)(?:\s*\+\s*(\d+))?")
_WS = re.compile(r"\s*")


def _strip_comments(text: str) -> str:
    def keep(m):
        return f" {_HOST} " if m.group(1).lstrip().startswith("(host)") else " "
    return re.sub(r"/\*(.*?)\*/", keep, text, flags=re.S)


def _pointee(base: str, structs: dict, what: str) -> None:
    if base not in SCALARS and base not in structs and base not in ("void", "char"):
        raise AgnnError(f"agnn.h: unknown type `{base}` in `{what}`")


def _dim(expr: str, consts: dict, what: str) -> int:
    m = _DIM.fullmatch(expr.strip())
    if not m or not (m.group(1).isdigit() or m.group(1) in consts):
        raise AgnnError(f"agnn.h: array size `{expr}` in `{what}` is no integer, constant or constant + integer")
    return (int(m.group(1)) if m.group(1).isdigit() else consts[m.group(1)]) + int(m.group(2) or 0)


def _members(body: str, consts: dict, structs: dict) -> list:
    fields = []
    for decl in body.replace(_HOST, " ").split(";"):
        decl = decl.strip()
        if not decl:
            continue
        first, *more = [p.strip() for p in decl.split(",")]
        m = _DECL.fullmatch(first)
        if not m:
            raise AgnnError(f"agnn.h: struct member `{decl}` not understood")
        base, stars, name, dim = m.groups()
        if stars:
            _pointee(base, structs, decl)
            typ = C.c_void_p
        elif base in SCALARS or base in structs:
            typ = SCALARS.get(base) or structs[base]
        else:
            raise AgnnError(f"agnn.h: unknown type `{base}` in struct member `{decl}`")
        fields.append((name, typ * _dim(dim, consts, decl) if dim is not None else typ))
        for other in more:
            m = _MORE.fullmatch(other)
            if not m or stars:
                raise AgnnError(f"agnn.h: struct member `{decl}` not understood")
            fields.append((m.group(1), typ * _dim(m.group(2), consts, decl) if m.group(2) is not None else typ))
    return fields


def _param(text: str, structs: dict, proto: str):
    host = _HOST in text
    m = _DECL.fullmatch(text.replace(_HOST, " ").strip())
    if not m or m.group(4) is not None:
        raise AgnnError(f"agnn.h: parameter `{text.strip()}` of {proto} not understood")
    base, stars, _name, _ = m.groups()
    depth = stars.count("*")
    if depth == 0:
        if base == STREAM:
            return C.c_void_p
        if base not in SCALARS:
            raise AgnnError(f"agnn.h: unknown type `{base}` in parameter `{text.strip()}` of {proto}")
        return SCALARS[base]
    _pointee(base, structs, f"{text.strip()} of {proto}")
    if depth == 1 and base in structs:
        return C.POINTER(structs[base])
    if host and depth == 1 and base in SCALARS:
        return C.POINTER(SCALARS[base])
    if host and depth == 2:
        return C.POINTER(C.c_void_p)
    return C.c_void_p


def _restype(text: str, proto: str):
    text = " ".join(text.split())
    if text in ("const char*", "const char *"):
        return C.c_char_p
    if text not in SCALARS:
        raise AgnnError(f"agnn.h: return type `{text}` of {proto} not understood")
    return SCALARS[text]


def parse(text: str):
    """(CONSTS, STRUCTS, SIGNATURES) of a header text: {AGNN_NAME: int}, {name_t: ctypes.Structure class} and
    {entry point: (restype, [argtypes])}, each in the header's order.  AgnnError for anything outside the accepted forms."""
    consts, structs, sigs = {}, {}, {}
    lines = []
    for line in _strip_comments(text).split("\n"):
        if not line.lstrip().startswith("#"):
            lines.append(line)
            continue
        m = _DEFINE.fullmatch(line.strip())
        if not m or m.group(1) in _SKIPPED_DEFINES:
            continue                                     # #include, #ifndef / #ifdef / #endif, the include guard
        v = re.fullmatch(_INT, m.group(2).strip())
        if not m.group(1).startswith("AGNN_") or not v:
            raise AgnnError(f"agnn.h: `{line.strip()}` is no `#define AGNN_NAME <integer>`")
        consts[m.group(1)] = int(v.group(1) or v.group(2))
    body = "\n".join(lines)
    m = re.fullmatch(r'\s*extern\s+"C"\s*\{(.*)\}\s*', body, flags=re.S)
    if m:
        body = m.group(1)
    pos = 0
    while True:
        pos = _WS.match(body, pos).end()
        if pos == len(body):
            return consts, structs, sigs
        if (m := _STREAM_T.match(body, pos)):
            pass
        elif (m := _STRUCT.match(body, pos)):
            structs[m.group(2)] = type(m.group(2), (C.Structure,), {"_fields_": _members(m.group(1), consts, structs)})
        elif (m := _PROTO.match(body, pos)):
            name, params = m.group(2), m.group(3).strip()
            args = [] if params == "void" else [_param(p, structs, name) for p in params.split(",")]
            sigs[name] = (_restype(m.group(1), name), args)
        else:
            raise AgnnError(f"agnn.h: declaration not understood: `{' '.join(body[pos:pos + 120].split())} ...`")
        pos = m.end()


def read_header(path: str = HEADER_PATH):
    if not os.path.exists(path):
        raise AgnnError(f"{path} not found: the binding of libagnn_hip.so is read from it (the package needs include/agnn.h "
                        "beside it, as analysisgnn_amd/csrc/Makefile does)")
    with open(path) as f:
        return parse(f.read())
