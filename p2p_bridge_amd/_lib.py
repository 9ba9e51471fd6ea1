"""ctypes loader for libp2pb_hip.so (the C ABI declared in include/p2pb_hip.h).

The header is the only list of entry points: its declarations are parsed when this module is imported, and lib() gives
every declared symbol its `restype` and `argtypes`, so ctypes converts plain Python ints and floats to the declared C
types and refuses anything else. Adding an entry point means declaring it in the header and defining it in csrc/;
nothing is listed here. Package code reaches the library through call() and ask(), which also compare the argument
count (ctypes passes surplus arguments on silently).

There is NO CPU fallback: if the library is missing, was not built for gfx950, or a tensor is not on
a HIP device, the call raises. (tests/ check this; the CPU oracle under oracle/ is never imported here.)
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("P2PB_LIB_PATH") or os.path.join(_HERE, "libp2pb_hip.so")  # override: kernel experiments
HEADER = os.path.join(_HERE, "..", "include", "p2pb_hip.h")

_RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char *": ctypes.c_char_p}
_SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "long": ctypes.c_long, "long long": ctypes.c_longlong,
            "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double}


class P2PBError(RuntimeError):
    pass


def parse_header(text):
    """text of include/p2pb_hip.h -> ({entry point: (restype, [argtypes])}, P2PB_ABI_VERSION). Every `ret name(params);`
    must be typed by the two maps above (any parameter with a `*` is a pointer); a declaration that is not, or a
    p2pb_ name in front of a `(` without such a declaration, raises P2PBError naming it."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    version = re.search(r"^[ \t]*#[ \t]*define[ \t]+P2PB_ABI_VERSION[ \t]+(\d+)[ \t]*$", text, flags=re.M)
    if version is None:
        raise P2PBError("include/p2pb_hip.h: no `#define P2PB_ABI_VERSION <number>`")
    text = re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)
    table = {}
    for ret, name, params in re.findall(r"([\w \t\n*]+?)\b(p2pb_\w+)\s*\(([^()]*)\)\s*;", text):
        ret, params = " ".join(ret.split()), " ".join(params.split())
        decl = f"{ret} {name}({params})"
        if ret not in _RETURNS or name in table:
            raise P2PBError(f"include/p2pb_hip.h: cannot type the declaration `{decl}` (return type, or declared twice)")
        args = []
        for p in ([] if params == "void" else params.split(",")):
            words = [w for w in p.split() if w != "const"]
            if "*" in p:
                args.append(ctypes.c_void_p)
            elif len(words) >= 2 and words[-1].isidentifier() and " ".join(words[:-1]) in _SCALARS:
                args.append(_SCALARS[" ".join(words[:-1])])
            else:
                raise P2PBError(f"include/p2pb_hip.h: cannot type the parameter `{p.strip()}` of `{decl}`")
        table[name] = (_RETURNS[ret], args)
    for name in re.findall(r"\b(p2pb_\w+)\s*\(", text):
        if name not in table:
            raise P2PBError(f"include/p2pb_hip.h: `{name}(` is not part of a declaration `type {name}(params);`")
    return table, int(version.group(1))


with open(HEADER) as _header:
    SIGNATURES, ABI_VERSION = parse_header(_header.read())
SYMBOLS = sorted(SIGNATURES)

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise P2PBError(
                f"{LIB_PATH} not found: build it with `python -m p2p_bridge_amd.build` "
                "(p2p_bridge_amd has no CPU / eager fallback)")
        _lib = ctypes.CDLL(LIB_PATH)
        have = _lib.p2pb_version() if hasattr(_lib, "p2pb_version") else None
        if have != ABI_VERSION:
            bad, _lib = _lib, None
            del bad
            raise P2PBError(f"{LIB_PATH} is ABI version {have}, this package binds version {ABI_VERSION} (include/p2pb_hip.h): "
                            "rebuild it with `python -m p2p_bridge_amd.build`")
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(_lib, name)  # AttributeError here = stale library
            fn.restype, fn.argtypes = restype, argtypes
        # products per split operand pair (include/p2pb_hip.h; fused.conv_math / set_conv_math)
        _lib.p2pb_set_split_terms(6 if os.environ.get("P2PB_CONV_MATH") in ("bf16x6", "fp32") else 16)
    return _lib


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def check(t, dtype, name):
    """Same preconditions as the reference's CHECK_CUDA / CHECK_CONTIGUOUS / CHECK_IS_* (PN2/utils.hpp:7-18)."""
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous tensor")
    if t.dtype != dtype:
        raise RuntimeError(f"{name} must be a {'float' if dtype == torch.float32 else 'int'} tensor")


def ask(fn_name, *args):
    """the entry point's return value (a size, a count, a flag, a status the caller reads itself); a symbol the header does
    not declare (experiment builds behind P2PB_LIB_PATH) has no argtypes and is called unchecked"""
    declared = SIGNATURES.get(fn_name)
    if declared is not None and len(args) != len(declared[1]):
        raise P2PBError(f"{fn_name} takes {len(declared[1])} arguments (include/p2pb_hip.h), called with {len(args)}")
    return getattr(lib(), fn_name)(*args)


def call(fn_name, *args):
    rc = ask(fn_name, *args)
    if rc != 0:
        raise P2PBError(f"{fn_name} failed with code {rc}")
