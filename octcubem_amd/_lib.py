"""ctypes binding of liboctmae.so (the C ABI declared in include/octmae.h).

There is NO fallback: if the shared library is missing or a symbol is absent the import of any
compute entry point raises.  PyTorch is used only for device memory, streams and autograd plumbing.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OCTMAE_LIB", os.path.join(_HERE, "liboctmae.so"))   # OCTMAE_LIB: A/B a variant build

_vp, _i, _f, _ll = C.c_void_p, C.c_int, C.c_float, C.c_longlong
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "octmae.h")


class OctmaeError(RuntimeError):
    pass


# the C spellings include/octmae.h uses, and nothing else: a declaration outside them is refused, never guessed
_PARAM = {"int": _i, "float": _f, "long long": _ll}                     # by value; anything with a * is a pointer
_RETURN = {"int": _i, "long long": _ll, "long long int": _ll}
_COMMENT = re.compile(r"/\*.*?\*/|//[^\n]*", re.S)
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(OCTMAE_\w+)[ \t]+(-?\d+)[ \t]*$", re.M)
_ENUM = re.compile(r"\benum\s*\{([^}]*)\}")
_PROTOTYPE = re.compile(r"(?:^|(?<=[;{}]))\s*([^;{}()]*?)\b(octmae_\w+)\s*\(([^)]*)\)\s*;", re.M)


def _argtype(fn: str, param: str):
    words = param.replace("*", " * ").split()
    if "*" in words:
        return C.c_char_p if words[:3] == ["const", "char", "*"] and words.count("*") == 1 else _vp
    for spelling in (" ".join(words), " ".join(words[:-1])):            # unnamed, or followed by the parameter's name
        if spelling in _PARAM:
            return _PARAM[spelling]
    raise OctmaeError(f"{fn}: no ctypes binding for the parameter {param.strip()!r}")


def parse_header(text: str):
    """(signatures, restypes, constants) of a C header in the style of include/octmae.h: every prototype
    ``int | long long [int]  octmae_<name>(...);`` as name -> ctypes argument list, the returns that are not ``int`` as name -> ctype, and
    the integer ``#define OCTMAE_*`` values and anonymous ``enum { OCTMAE_* = n }`` members as name -> int.  Comments are ignored."""
    text = _COMMENT.sub(" ", text)
    constants = {name: int(value) for name, value in _DEFINE.findall(text)}
    for body in _ENUM.findall(text):
        for member in filter(None, (m.strip() for m in body.split(","))):
            m = re.fullmatch(r"(OCTMAE_\w+)\s*=\s*(-?\d+)", member)
            if m is None:
                raise OctmaeError(f"enum member {member!r}: expected OCTMAE_<NAME> = <integer>")
            constants[m.group(1)] = int(m.group(2))
    signatures, restypes = {}, {}
    for ret, fn, params in _PROTOTYPE.findall(re.sub(r"^[ \t]*#[^\n]*", "", text, flags=re.M)):
        ret = " ".join(ret.split())
        if ret not in _RETURN:
            raise OctmaeError(f"{fn}: no ctypes binding for the return type {ret!r}")
        signatures[fn] = [] if params.strip() == "void" else [_argtype(fn, p) for p in params.split(",")]
        if _RETURN[ret] is not _i:
            restypes[fn] = _RETURN[ret]
    return signatures, restypes, constants


def _parse_header_file():
    try:
        with open(HEADER_PATH) as f:
            return parse_header(f.read())
    except OSError as e:
        raise OctmaeError(f"{HEADER_PATH} cannot be read ({e.strerror}): the ctypes bindings are derived from it") from e


# SIGNATURES: name -> argtypes; every function returns int (0 ok, <0 bad argument, >0 hipError_t) ...
# RESTYPES: ... except a workspace query whose value is long long in the header: a byte count for the two retrieval queries, a count of
# DOUBLES for octmae_bootstrap_moments_ws.  CONSTANTS: the header's integer #defines and enum members.
SIGNATURES, RESTYPES, CONSTANTS = _parse_header_file()

_lib = None
_on_load = []       # callbacks run once, right after the library has been loaded and bound (ops: operand-type check)


def expected_abi_version() -> int:
    """OCTMAE_ABI_VERSION as include/octmae.h defines it -- the single place the number is written."""
    if "OCTMAE_ABI_VERSION" not in CONSTANTS:
        raise OctmaeError(f"{HEADER_PATH} does not define OCTMAE_ABI_VERSION")
    return CONSTANTS["OCTMAE_ABI_VERSION"]


def load():
    """Load liboctmae.so and bind every declared symbol.  Raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OctmaeError(
            f"{LIB_PATH} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()' "
            "or make -C octcubem_amd/csrc).  There is no CPU or eager fallback.")
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:        # e.g. a copied .so on a box without the HIP runtime it links against
        raise OctmaeError(f"{LIB_PATH} could not be loaded: {e}") from e
    for name, argtypes in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:  # pragma: no cover
            raise OctmaeError(f"liboctmae.so does not export {name}") from e
        fn.argtypes = argtypes
        fn.restype = RESTYPES.get(name, C.c_int)
    if lib.octmae_abi_version() != expected_abi_version():
        raise OctmaeError(f"{LIB_PATH} reports ABI {lib.octmae_abi_version()}, include/octmae.h declares "
                          f"{expected_abi_version()}: rebuild (make -C octcubem_amd/csrc)")
    _lib = lib
    for cb in list(_on_load):
        cb(lib)
    return lib


_FN = {}


def call(name, *args):
    """Invoke a C-ABI entry point and turn its status code into an exception."""
    fn = _FN.get(name)
    if fn is None:
        fn = _FN[name] = getattr(load(), name)
    rc = fn(*args)
    if rc != 0:
        kind = ("bad argument" if rc == -1 else "unsupported combination" if rc == -2 else "librccl not found" if rc == -3
                else f"ncclResult_t {rc - 10000}" if rc >= 10000 else f"hipError_t {rc}")
        raise OctmaeError(f"{name} failed: {kind} (rc={rc})")
    return rc
