"""ctypes binding of libigcn.so (C ABI in include/igcn.h).  No torch types cross the boundary:
only raw device pointers (tensor.data_ptr()), sizes and the hipStream_t of the current torch stream.

There is NO fallback: if the library is missing or a call fails, an exception is raised.
"""
import ctypes
import os
import re
import sys

import torch

from . import switches

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libigcn.so")
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "igcn.h"))


class IgcnError(RuntimeError):
    pass


P, I, L, F, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_size_t
_RESTYPES = {"int": I, "size_t": Z, "constchar*": ctypes.c_char_p}     # (spaces removed)
_SCALARS = {"int": I, "int64_t": L, "size_t": Z, "float": F, "double": ctypes.c_double, "unsigned": ctypes.c_uint}
_COMMENT = re.compile(r"/\*.*?\*/|//[^\n]*", re.S)
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(IGCN_\w+)[ \t]+\(?[ \t]*(-?\d+)[ \t]*\)?[ \t]*$", re.M)
_DIRECTIVE = re.compile(r"^[ \t]*#.*$", re.M)
_DECLARATION = re.compile(r"([^;{}()]*?)\b(igcn_\w+)\s*\(([^()]*)\)\s*;")     # (return type, name, arguments)
_NAME = re.compile(r"\w+\Z")


def _argtype(name, arg):
    """ctypes type of one argument: `<type> [identifier]` with <type> one of _SCALARS (const ignored), or anything
    with a `*`.  `unsigned long n`, `float x[4]`, `long n` and the like raise: a guessed width would shift every
    argument behind it without a word."""
    words = [w for w in arg.split() if w != "const"]
    if "[" not in arg:
        if "*" in arg:
            return P
        if words and words[0] in _SCALARS and (len(words) == 1 or len(words) == 2 and _NAME.match(words[1])):
            return _SCALARS[words[0]]
    raise IgcnError(f"{name}: argument `{arg.strip()}` is neither a pointer nor `<type> [name]` with <type> one of "
                    f"{', '.join(_SCALARS)}")


def parse_header(text):
    """``(signatures, limits)`` of a header written like include/igcn.h.  limits: ``IGCN_NAME -> int`` for every
    ``#define IGCN_NAME <decimal literal>``; no expression is evaluated.  signatures: ``name -> (restype, [argtypes])``
    for every ``igcn_*(...);`` declaration.  Nothing is guessed and nothing is skipped: a return type other than int,
    size_t or const char*, an argument _argtype refuses, or an ``igcn_*(`` that is no such declaration (a definition, a
    function-pointer argument) raises IgcnError naming it."""
    text = _COMMENT.sub(" ", text)
    limits = {m.group(1): int(m.group(2)) for m in _DEFINE.finditer(text)}
    text = _DIRECTIVE.sub(" ", text)
    signatures = {}
    for m in _DECLARATION.finditer(text):
        ret, name, args = "".join(m.group(1).split()), m.group(2), m.group(3).strip()
        if ret not in _RESTYPES:
            raise IgcnError(f"{name}: return type `{' '.join(m.group(1).split())}` is none of int, size_t, const char*")
        args = [] if args in ("", "void") else args.split(",")
        signatures[name] = (_RESTYPES[ret], [_argtype(name, a) for a in args])
    unbound = [n for n in re.findall(r"\b(igcn_\w+)\s*\(", text) if n not in signatures]
    if unbound:
        raise IgcnError(f"{', '.join(unbound)}: not a plain `<type> igcn_name(<arguments>);` declaration")
    return signatures, limits


def read_header(path=HEADER_PATH):
    try:
        with open(path) as fh:
            return parse_header(fh.read())
    except OSError as e:
        raise IgcnError(f"{path}: the C header this binding is derived from cannot be read ({e.strerror})") from None


# name -> (restype, argtypes) and IGCN_NAME -> value: include/igcn.h is the only place either is written down
SIGNATURES, LIMITS = read_header()
ABI_VERSION = LIMITS["IGCN_ABI_VERSION"]
COPY_MULTI_MAX = LIMITS["IGCN_COPY_MULTI_MAX"]

_lib = None


def load():
    """Load libigcn.so once.  Raises IgcnError when it has not been built (python ig-gcn_amd/build.py)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise IgcnError(f"{LIB_PATH} is missing: build it with `python ig-gcn_amd/build.py` "
                        "(there is no CPU or PyTorch fallback for the HIP path)")
    lib = ctypes.CDLL(LIB_PATH)      # torch is imported above, so libamdhip64.so.7 resolves to torch's runtime
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)      # AttributeError if the header and the library disagree
        fn.restype = res
        fn.argtypes = args
    got = int(lib.igcn_version())
    if got != ABI_VERSION:           # a stale libigcn.so would take shifted arguments without a word
        raise IgcnError(f"{LIB_PATH} has ABI revision {got}, this binding is written for {ABI_VERSION}: "
                        "rebuild it with `python ig-gcn_amd/build.py --force`")
    # the library's A/B switches (switches.LIBRARY) and knobs: read from the environment HERE, once, and handed over
    # (no getenv in a launch path)
    lib.igcn_configure(switches.library_mask(), switches.knob("IGCN_GEMM_BN"), switches.knob("IGCN_ATTN_CHUNK"))
    _lib = lib
    return lib


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    """Device pointer of a contiguous CUDA tensor (or None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise IgcnError("libigcn operates on device memory only; got a CPU tensor")
    if not t.is_contiguous():
        raise IgcnError("libigcn needs contiguous tensors")
    return t.data_ptr()


_DEBUG_SYNC = os.environ.get("IGCN_DEBUG_SYNC", "0") == "1"


def call(name, *args):
    """Invoke an int-returning entry point; raise with igcn_last_error() on failure.

    IGCN_DEBUG_SYNC=1 (debugging a kernel fault): announce every entry point on stderr and synchronise the device
    after it, so that the last line printed names the faulting call (inside a stream capture: announced only)."""
    lib = load()
    if _DEBUG_SYNC:
        print(f"[igcn] {name} {args}", file=sys.stderr, flush=True)
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise IgcnError(f"{name} failed (rc={rc}): {lib.igcn_last_error().decode()}")
    if _DEBUG_SYNC:
        import torch
        if not torch.cuda.is_current_stream_capturing():    # (a capture refuses the synchronisation and is invalidated by it)
            torch.cuda.synchronize()


def copy_multi(pairs):
    """``dst.copy_(src)`` for every (dst, src) pair of same-shape, same-dtype contiguous DEVICE tensors as one launch
    per COPY_MULTI_MAX (16) pairs (igcn_copy_multi) on the current stream.  Anything else (a host tensor, a dtype change,
    a strided view) goes through ``Tensor.copy_``."""
    fast = []
    for dst, src in pairs:
        if (dst.is_cuda and src.is_cuda and dst.device == src.device and dst.dtype == src.dtype
                and dst.shape == src.shape and dst.is_contiguous() and src.is_contiguous()):
            if dst.numel() and dst.data_ptr() != src.data_ptr():
                fast.append((dst, src))
        else:
            dst.copy_(src, non_blocking=True)
    for k in range(0, len(fast), COPY_MULTI_MAX):
        chunk = fast[k:k + COPY_MULTI_MAX]
        n = len(chunk)
        d = (ctypes.c_void_p * n)(*[t.data_ptr() for t, _ in chunk])
        s = (ctypes.c_void_p * n)(*[t.data_ptr() for _, t in chunk])
        nb = (ctypes.c_int64 * n)(*[t.numel() * t.element_size() for t, _ in chunk])
        call("igcn_copy_multi", n, d, s, nb, stream_ptr())
