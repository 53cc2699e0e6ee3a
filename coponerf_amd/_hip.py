"""ctypes binding of libcoponerf_hip.so, derived from its C ABI: include/coponerf_hip.h.

The header is the only description of the interface.  It is parsed once at import (the built library is not needed for
that): every `<ret> cpn_<name>(<args>);` becomes a PROTOTYPES entry and every integer `#define CPN_<NAME>` a constant of this
module.  A new entry point is declared in the header and defined in a unit of csrc/ - nothing is added here.  A
declaration the parser does not understand raises: it is never skipped.

The library is the product's only compute path: if it is missing or a symbol
is absent this module raises — there is no PyTorch/CPU fallback.
"""
from __future__ import annotations

import ctypes
import os
import re
from typing import Dict, List, Tuple

_HERE = os.path.dirname(os.path.abspath(__file__))
# COPONERF_HIP_LIB: another build of the SAME library (kernel-variant experiments, tools/_build/); never a fallback
LIB_PATH = os.environ.get("COPONERF_HIP_LIB") or os.path.join(_HERE, "libcoponerf_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "coponerf_hip.h")

_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "long long": ctypes.c_longlong}


class HeaderError(ValueError):
    pass


def _ctype(decl: str, is_return: bool):
    """ctypes type of one return type or one parameter (`const` and the parameter's name are ignored)."""
    words = [w for w in decl.replace("*", " * ").split() if w != "const"]
    if not words or not all(w == "*" or re.fullmatch(r"\w+", w) for w in words):
        raise HeaderError(f"cannot classify {decl.strip()!r}")
    if is_return:
        if words == ["char", "*"]:
            return ctypes.c_char_p
    elif "*" in words:
        return ctypes.POINTER(ctypes.c_void_p) if words[:3] == ["void", "*", "*"] else ctypes.c_void_p
    elif " ".join(words) not in _SCALARS:
        words = words[:-1]                     # the parameter's name
    if " ".join(words) not in _SCALARS:
        raise HeaderError(f"unknown type in {decl.strip()!r}")
    return _SCALARS[" ".join(words)]


def parse_header(text: str) -> Tuple[Dict[str, Tuple[object, List]], Dict[str, int]]:
    """(name -> (restype, argtypes) of every cpn_ prototype, NAME -> value of every integer `#define CPN_NAME`) of a header."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    constants = {}
    for name, expr in re.findall(r"^[ \t]*#[ \t]*define[ \t]+CPN_(\w+)[ \t]+(.+?)[ \t]*$", text, flags=re.M):
        if re.fullmatch(r"[-0-9+*() \t]+", expr):
            constants[name] = int(eval(expr, {"__builtins__": {}}))
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    prototypes = {}
    for ret, name, args in re.findall(r"([\w\s*]+?)\b(cpn_\w+)\s*\(([^;{}]*)\)\s*;", text):
        if name in prototypes:
            raise HeaderError(f"{name} is declared twice")
        params = [] if args.strip() in ("", "void") else args.split(",")
        prototypes[name] = (_ctype(ret, True), [_ctype(p, False) for p in params])
    mentioned = re.findall(r"\b(cpn_\w+)\s*\(", text)
    if sorted(mentioned) != sorted(prototypes):
        raise HeaderError(f"not a prototype this parser reads: {sorted(set(mentioned) - set(prototypes)) or mentioned}")
    return prototypes, constants


with open(HEADER_PATH) as _f:
    PROTOTYPES, CONSTANTS = parse_header(_f.read())
if set(CONSTANTS) & set(globals()):
    raise HeaderError(f"CPN_ constants shadow names of this module: {sorted(set(CONSTANTS) & set(globals()))}")
globals().update(CONSTANTS)                    # every #define CPN_<NAME> <integer expression> is _hip.<NAME>

# name -> argtypes
SIGNATURES: Dict[str, List] = {name: argtypes for name, (_, argtypes) in PROTOTYPES.items()}

# the constants the package and the tests read, by name
ABI_VERSION = CONSTANTS["ABI_VERSION"]
CAM_STRIDE = CONSTANTS["CAM_STRIDE"]
CAM_TQ = CONSTANTS["CAM_TQ"]
CAM_M = CONSTANTS["CAM_M"]
CAM_AOWN = CONSTANTS["CAM_AOWN"]
CAM_AOTH = CONSTANTS["CAM_AOTH"]
CAM_KQ = CONSTANTS["CAM_KQ"]
CAM_KC = CONSTANTS["CAM_KC"]
CAM_KO = CONSTANTS["CAM_KO"]
CAM_KN = CONSTANTS["CAM_KN"]
TAB_LD = CONSTANTS["TAB_LD"]
ENC_FRAG_HALVES = CONSTANTS["ENC_FRAG_HALVES"]
RAYC_STRIDE = CONSTANTS["RAYC_STRIDE"]
LIGHTFIELD_PACK_FLOATS = CONSTANTS["LIGHTFIELD_PACK_FLOATS"]
ADAM_SEG_BYTES = CONSTANTS["ADAM_SEG_BYTES"]
POSE_TAIL_TENSORS = CONSTANTS["POSE_TAIL_TENSORS"]
LPIPS_LAYERS = CONSTANTS["LPIPS_LAYERS"]


def declared_symbols() -> List[str]:
    """Every function name include/coponerf_hip.h declares."""
    return sorted(PROTOTYPES)


class HipLibraryError(RuntimeError):
    pass


_lib = None


def lib() -> ctypes.CDLL:
    """Load (once) and type the shared library; raise loudly if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryError(
            f"{LIB_PATH} not found: build it with `python coponerf_amd/csrc/build.py` "
            "(or __graft_entry__.build()).  coponerf_amd has no non-HIP compute path.")
    try:
        handle = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover - depends on the machine
        raise HipLibraryError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (restype, argtypes) in PROTOTYPES.items():
        try:
            fn = getattr(handle, name)
        except AttributeError as e:
            raise HipLibraryError(f"{LIB_PATH} does not export {name}; rebuild it") from e
        fn.argtypes = argtypes
        fn.restype = restype
    got = handle.cpn_abi_version()
    if got != ABI_VERSION:
        raise HipLibraryError(f"{LIB_PATH} has ABI version {got}, binding expects {ABI_VERSION}; rebuild it")
    _lib = handle
    return _lib


def check(status: int, what: str) -> None:
    if status != 0:
        msg = lib().cpn_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what} failed (status {status}): {msg}")


_FN = {}


def call(name: str, *args) -> None:
    """Invoke an entry point; tensors are passed as .data_ptr() integers by the caller."""
    fn = _FN.get(name)
    if fn is None:
        fn = _FN[name] = getattr(lib(), name)
    status = fn(*args)
    if status != 0:
        check(status, name)


def stream_handle() -> int:
    """Raw handle of torch's current HIP stream on the current device.  The same lookup as
    `torch.cuda.current_stream().cuda_stream` without building a Stream object: that form cost 9 us of Python per launch —
    1.3 ms of the 6.5 ms of host time of one get_z, which had become the eager call's bound."""
    import torch
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())
