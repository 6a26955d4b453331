"""ctypes binding of libscenesplat_hip.so (the C-ABI declared in include/scenesplat_hip.h).

Loading fails loudly: there is no CPU fallback behind these symbols."""
import ctypes
import os
import re

# torch first: PyTorch-ROCm ships its own libamdhip64; it must be the HIP runtime of the process
# before this library (linked against the same soname) is mapped, or kernels and streams would
# belong to two different runtimes and every launch fails.
import torch  # noqa: F401

from . import build

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libscenesplat_hip.so")

# C types of the header -> ctypes; anything with a `*` travels as c_void_p (it takes None, ints and the ctypes arrays of host values)
_CTYPES = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
           "size_t": ctypes.c_size_t, "unsigned long long": ctypes.c_ulonglong, "float": ctypes.c_float,
           "ss_stream_t": ctypes.c_void_p}
_DECL = re.compile(r"([\w\s]+?)\b(ss_[a-z0-9_]+)\s*\(([^()]*)\)\s*;")


def _ctype(c_type, name):
    if "*" in c_type:
        return ctypes.c_void_p
    c_type = " ".join(c_type.split())
    if c_type not in _CTYPES:
        raise ValueError(f"{name}: no ctypes type for the C type '{c_type}'")
    return _CTYPES[c_type]


def parse_header(text):
    """C header text -> ({name: (restype, [argtypes])} of its ss_* declarations, {name: value} of its integer enums and #defines).
    Strict: a type outside _CTYPES, or an ss_* name followed by `(` that did not parse as a declaration, raises (ctypes would pass
    the arguments of a function without a prototype as C ints)."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    constants = {m[1]: int(m[2]) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(-?\d+)[ \t]*$", text, flags=re.M)}
    for body in re.findall(r"\benum\s*\{([^}]*)\}", text):
        for item in body.split(","):
            m = re.fullmatch(r"\s*(\w+)\s*=\s*(-?\d+)\s*", item)
            if not m:
                raise ValueError(f"enum item '{item.strip()}' is not NAME = integer")
            constants[m[1]] = int(m[2])
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    prototypes = {}
    for ret, name, params in _DECL.findall(text):
        params = [] if params.strip() == "void" else params.split(",")
        # a parameter is a type and a name: the type is what stands in front of the last word
        prototypes[name] = (_ctype(ret, name), [_ctype(re.sub(r"\w+\s*$", "", p), name) for p in params])
    missed = set(re.findall(r"\b(ss_[a-z0-9_]+)\s*\(", text)) ^ set(prototypes)
    if missed:
        raise ValueError(f"not parsed as declarations: {sorted(missed)}")
    return prototypes, constants


with open(build.HEADER) as _f:
    PROTOTYPES, CONSTANTS = parse_header(_f.read())

_lib = None


def load():
    """Return the loaded library (cached).  Raises RuntimeError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m scenesplat_amd.build` "
            "(hipcc --offload-arch=gfx950). scenesplat_amd has no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class NativeError(RuntimeError):
    pass


_STATUS = {CONSTANTS["SS_ERR_ARG"]: "bad argument", CONSTANTS["SS_ERR_LAUNCH"]: "kernel launch failed",
           CONSTANTS["SS_ERR_WORKSPACE"]: "workspace too small"}


def check(rc, name):
    if rc != 0:
        raise NativeError(f"{name} failed: status {rc} ({_STATUS.get(rc, 'unknown')})")
