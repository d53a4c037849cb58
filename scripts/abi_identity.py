#!/usr/bin/env python3
"""Refactor check for the ctypes binding: analysisgnn_amd/_lib.py must bind what it bound at <parent-rev>.
    scripts/abi_identity.py <parent-rev>
The parent's _lib.py is taken from `git show` and executed under a temporary module name (its `resident` import gets a stub:
nothing here calls into it), then compared with the working tree's module: every SIGNATURES entry type for type, every struct's
_fields_ (names, types, array lengths) and every integer constant.  Names only the new module has are not differences.  Prints
IDENTICAL or one line per difference and exits non-zero on any; needs no GPU and no built library (profiles/abi_binding.md).
A one-off for a parent whose _lib.py holds the tables itself (it needs only ctypes, torch and `resident`)."""
import ctypes as C
import os
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_parent(rev):
    src = subprocess.check_output(["git", "-C", ROOT, "show", f"{rev}:analysisgnn_amd/_lib.py"], text=True)
    pkg = types.ModuleType("_abi_parent")
    pkg.__path__ = []
    pkg.resident = types.ModuleType("_abi_parent.resident")
    mod = types.ModuleType("_abi_parent._lib")
    mod.__package__ = "_abi_parent"
    mod.__file__ = os.path.join(ROOT, "analysisgnn_amd", "_lib.py")
    sys.modules.update({"_abi_parent": pkg, "_abi_parent.resident": pkg.resident, "_abi_parent._lib": mod})
    exec(compile(src, f"{rev}:analysisgnn_amd/_lib.py", "exec"), mod.__dict__)
    return mod


def desc(t):
    """A ctypes type as a value that compares equal across two modules' struct classes."""
    if t is None or not isinstance(t, type):
        return repr(t)
    if issubclass(t, C.Structure):
        return ("struct", tuple((f[0], desc(f[1])) for f in t._fields_))
    if issubclass(t, C.Array):
        return ("array", desc(t._type_), t._length_)
    if issubclass(t, C._Pointer):
        return ("pointer", desc(t._type_))
    return t.__name__                                   # simple types: c_int, c_long, c_void_p ... (ctypes' own classes)


def show(d):
    if isinstance(d, tuple) and d[0] == "struct":
        return "struct{" + ", ".join(n for n, _ in d[1]) + "}"
    if isinstance(d, tuple) and d[0] == "array":
        return f"{show(d[1])}[{d[2]}]"
    if isinstance(d, tuple):
        return f"POINTER({show(d[1])})"
    return d


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.path.insert(0, ROOT)
    old = load_parent(sys.argv[1])
    from analysisgnn_amd import _lib as new
    diffs = []
    for name in sorted(set(old.SIGNATURES) | set(new.SIGNATURES)):
        if name not in old.SIGNATURES or name not in new.SIGNATURES:
            diffs.append(f"{name}: only in the {'new' if name in new.SIGNATURES else 'parent'} SIGNATURES")
            continue
        (r0, a0), (r1, a1) = old.SIGNATURES[name], new.SIGNATURES[name]
        if desc(r0) != desc(r1):
            diffs.append(f"{name}: restype {show(desc(r0))} -> {show(desc(r1))}")
        if len(a0) != len(a1):
            diffs.append(f"{name}: {len(a0)} -> {len(a1)} arguments")
        for i, (x, y) in enumerate(zip(a0, a1)):
            if desc(x) != desc(y):
                diffs.append(f"{name}: argument {i} {show(desc(x))} -> {show(desc(y))}")
    n_struct = n_const = 0
    for name, v in sorted(vars(old).items()):
        if isinstance(v, type) and issubclass(v, C.Structure):
            n_struct += 1
            w = getattr(new, name, None)
            if not (isinstance(w, type) and issubclass(w, C.Structure)):
                diffs.append(f"{name}: struct missing in the new module")
            elif desc(v) != desc(w) or C.sizeof(v) != C.sizeof(w):
                f0, f1 = desc(v)[1], desc(w)[1]
                where = [f"{a[0]}: {show(a[1])} -> {b[0]}: {show(b[1])}" for a, b in zip(f0, f1) if a != b]
                diffs.append(f"{name}: _fields_ differ ({len(f0)} -> {len(f1)} fields; " + "; ".join(where) + ")")
        elif name.isupper() and type(v) is int:
            n_const += 1
            if getattr(new, name, None) != v or type(getattr(new, name)) is not int:
                diffs.append(f"{name}: {v} -> {getattr(new, name, 'missing')}")
    print(f"compared {len(old.SIGNATURES)} signatures, {n_struct} structs, {n_const} constants against {sys.argv[1]}")
    print("\n".join(diffs) if diffs else "IDENTICAL")
    return 1 if diffs else 0


if __name__ == "__main__":
    sys.exit(main())
