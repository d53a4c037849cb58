"""The binding is read from include/agnn.h (analysisgnn_amd/_abi.py).  Checked here without a GPU: the struct layouts and
constants the reader derives are the ones a C compiler derives from the same header (which also proves the header is valid C on
its own); the reader refuses declarations outside the forms it knows instead of dropping them; and the argtypes it produces make
ctypes refuse a wrong call before any library code runs."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
SO = os.path.join(ROOT, "analysisgnn_amd", "libagnn_hip.so")


def _c_compiler():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for cand in ("cc", os.path.join(rocm, "llvm", "bin", "clang"), os.path.join(rocm, "lib", "llvm", "bin", "clang")):
        path = shutil.which(cand)
        if path:
            return path
    return None


def test_layout_and_constants_match_a_c_compiler(tmp_path):
    from analysisgnn_amd import _lib
    cc = _c_compiler()
    if cc is None:
        pytest.skip("no C compiler (cc, ROCm clang): the library cannot be built here either")
    expect = {}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "agnn.h"', "int main(void) {"]
    for name, cls in _lib.STRUCTS.items():
        expect[f"sizeof {name}"] = C.sizeof(cls)
        lines.append(f'  printf("sizeof {name} %zu\\n", sizeof({name}));')
        for field, _ in cls._fields_:
            d = getattr(cls, field)
            expect[f"member {name}.{field}"] = (d.offset, d.size)
            lines.append(f'  printf("member {name}.{field} %zu %zu\\n", offsetof({name}, {field}), sizeof((({name}*)0)->{field}));')
    for name, value in _lib.CONSTS.items():
        expect[f"const {name}"] = value
        lines.append(f'  printf("const {name} %lld\\n", (long long)({name}));')
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-std=c11", "-I", INCLUDE, "-o", str(exe), str(src)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        kind, key, *nums = line.split()
        got[f"{kind} {key}"] = int(nums[0]) if len(nums) == 1 else tuple(int(n) for n in nums)
    assert len(_lib.STRUCTS) >= 21 and len(_lib.CONSTS) >= 35
    assert got == expect


BAD_HEADERS = {
    "member of unknown type": "typedef struct { const float* x; agnn_thing_t t; } agnn_a_t;",
    "function-pointer parameter": "int agnn_f(void (*cb)(int), agnn_stream_t stream);",
    "non-integer define": "#define AGNN_X 1.5f\nint agnn_version(void);",
    "define of an expression": "#define AGNN_X (AGNN_Y + 1)\nint agnn_version(void);",
    "stray declaration": "int agnn_version(void);\nextern int agnn_counter;\nsize_t agnn_bytes(int32_t n);",
    "stray struct tag": "int agnn_version(void);\nstruct agnn_opaque;\nsize_t agnn_bytes(int32_t n);",
    "unknown parameter type": "int agnn_f(long n, agnn_stream_t stream);",
    "struct by value": "typedef struct { int32_t n; } agnn_a_t;\nint agnn_f(agnn_a_t a);",
    "array size that is an expression": "#define AGNN_N 4\ntypedef struct { int32_t v[AGNN_N * 2]; } agnn_a_t;",
    "array size of an unknown name": "typedef struct { int32_t v[AGNN_N]; } agnn_a_t;",
    "unknown return type": "long agnn_f(void);",
    "line comment": "int agnn_version(void);  // the version",
}


@pytest.mark.parametrize("what", list(BAD_HEADERS))
def test_reader_refuses_what_it_does_not_know(what):
    from analysisgnn_amd import _abi
    text = "typedef void* agnn_stream_t;\n" + BAD_HEADERS[what] + "\n"
    with pytest.raises(_abi.AgnnError):
        _abi.parse(text)
    with pytest.raises(_abi.AgnnError):                       # the same inside the header's frame
        _abi.parse('#ifndef AGNN_H_\n#define AGNN_H_\n#include <stdint.h>\n#ifdef __cplusplus\nextern "C" {\n#endif\n'
                   + text + "#ifdef __cplusplus\n}\n#endif\n#endif /* AGNN_H_ */\n")


def test_reader_on_a_good_fragment():
    from analysisgnn_amd import _abi
    consts, structs, sigs = _abi.parse("""
/* a comment that mentions arrays marked (host) is no marker */
#ifndef AGNN_H_
#define AGNN_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef void* agnn_stream_t; /* hipStream_t */
#define AGNN_N 3
#define AGNN_NEG (-22)  /* errno style */
#define AGNN_FLAG 8u
typedef struct {
  const float* p;      /* (device) */
  const void* const* pp;   /* (host) members stay c_void_p */
  int64_t ld, n;
  int32_t v[AGNN_N + 1];
  float* dst[AGNN_N];
  uint8_t tail[2];
} agnn_item_t;
typedef struct { agnn_item_t it[AGNN_N]; double d; size_t s; } agnn_outer_t;
const char* agnn_name(void);
size_t agnn_bytes(int32_t n, const agnn_item_t* items);
int agnn_call(int n, const agnn_item_t* items /* (host) */, const int32_t* offs /* (host) [n + 1] */, const int32_t* offs_dev,
              float* const* outs /* (host) */, const float* const* ins, void* workspace /* any */, uint32_t flags, float eps,
              agnn_stream_t stream);
#ifdef __cplusplus
}
#endif
#endif /* AGNN_H_ */
""")
    assert consts == {"AGNN_N": 3, "AGNN_NEG": -22, "AGNN_FLAG": 8}
    item, outer = structs["agnn_item_t"], structs["agnn_outer_t"]
    assert list(structs) == ["agnn_item_t", "agnn_outer_t"]
    assert item._fields_ == [("p", C.c_void_p), ("pp", C.c_void_p), ("ld", C.c_int64), ("n", C.c_int64), ("v", C.c_int32 * 4),
                             ("dst", C.c_void_p * 3), ("tail", C.c_uint8 * 2)]
    assert outer._fields_ == [("it", item * 3), ("d", C.c_double), ("s", C.c_size_t)]
    assert sigs == {
        "agnn_name": (C.c_char_p, []),
        "agnn_bytes": (C.c_size_t, [C.c_int32, C.POINTER(item)]),
        "agnn_call": (C.c_int, [C.c_int, C.POINTER(item), C.POINTER(C.c_int32), C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p,
                                C.c_void_p, C.c_uint32, C.c_float, C.c_void_p]),
    }


def test_missing_header_is_an_error_that_names_the_path(tmp_path):
    from analysisgnn_amd import _abi
    path = str(tmp_path / "include" / "agnn.h")
    with pytest.raises(_abi.AgnnError, match="agnn.h"):
        _abi.read_header(path)


def test_public_names_are_bound_from_the_header():
    from analysisgnn_amd import _abi, _lib
    assert _lib.AgnnError is _abi.AgnnError
    assert _lib.Rel is _lib.STRUCTS["agnn_rel_t"] and _lib.HgtDstItem is _lib.STRUCTS["agnn_hgt_dst_item_t"]
    assert _lib.MAX_SEG == 32 and _lib.EMBED_MAX_TABLES == 4 and _lib.WGRAD_BATCH_MAX_ITEMS == 24 and _lib.WGRAD_BATCH_MAX == 16
    assert (_lib.CONSTS["AGNN_OK"], _lib.CONSTS["AGNN_EINVAL"], _lib.CONSTS["AGNN_EALIGN"], _lib.CONSTS["AGNN_ENOMEM"],
            _lib.CONSTS["AGNN_ERUNTIME"]) == (0, -22, -14, -12, -5)
    assert _lib.SIGNATURES["agnn_hgt_attn_fwd_multi_f32"][1][1] is C.POINTER(_lib.HgtDstItem)
    assert _lib.SIGNATURES["agnn_embed_cat_fwd_f32"][1][5:8] == [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]


def _loaded():
    from analysisgnn_amd import _lib
    if not os.path.exists(SO):
        pytest.fail("libagnn_hip.so not built (run __graft_entry__.build())")
    return _lib, _lib.load()


def test_ctypes_refuses_an_extra_argument():
    """What ctypes guards about the NUMBER of arguments of a cdecl function, stated exactly: fewer than argtypes is a TypeError;
    an argument beyond argtypes is converted by ctypes' default rules, so one it cannot convert (a float, any object) is an
    ArgumentError, while an int, bytes, None or a ctypes instance there is passed on (CPython's `PyCFuncPtr_call`: "for cdecl
    functions, we allow more actual arguments than the length of the argtypes tuple").  Only a wrapper around every call could
    refuse those, and the call sites stay plain `lib.agnn_x(...)`; agnn_version(1) therefore returns the version."""
    _, lib = _loaded()
    with pytest.raises(C.ArgumentError):
        lib.agnn_version(1.0)
    with pytest.raises(TypeError):
        lib.agnn_csr_workspace_bytes(1)                       # a dropped argument


def test_ctypes_refuses_an_integer_for_a_host_array():
    _, lib = _loaded()
    with pytest.raises(C.ArgumentError):
        lib.agnn_embed_workspace_bytes(1, 12345, 64)


def test_ctypes_refuses_another_structs_array():
    _lib, lib = _loaded()
    with pytest.raises(C.ArgumentError):
        lib.agnn_csr_rowend_batch(1, (_lib.HgtRel * 1)(), None)
    with pytest.raises(C.ArgumentError):                      # items of agnn_hgt_dst_item_t
        lib.agnn_hgt_attn_fwd_multi_f32(1, (_lib.HgtRel * 1)(), 32, 4, None)
