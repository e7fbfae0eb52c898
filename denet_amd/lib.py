"""ctypes binding of libdenet_hip.so, derived from include/denet_hip.h.

This is the only door from the Python host side to the HIP kernels: plain pointers, sizes and a stream.
There is deliberately NO fallback: if the library is missing or a call fails the caller gets an exception.
The header is the only statement of the ABI: SIGNATURES, DEFINES and BnLink are parsed from it at import, nothing is typed twice.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libdenet_hip.so")
HEADER_PATH = os.path.join(_HERE, "..", "include", "denet_hip.h")


class DenetHipError(RuntimeError):
    pass


P = ctypes.c_void_p
I = ctypes.c_int
L = ctypes.c_long
F = ctypes.c_float
Z = ctypes.c_size_t
U64 = ctypes.c_uint64
D = ctypes.c_double

# every scalar type the header may use; any pointer is a c_void_p, the one other return type is `const char*`
SCALARS = {"int": I, "long": L, "float": F, "double": D, "size_t": Z, "uint64_t": U64, "hipStream_t": P}


def _ctype(decl, where, returns=False):
    """ctypes type of one parameter `type name`, struct field `type name` or return type `type`. No default: what the map
    does not hold raises and names the declaration."""
    words = [w for w in decl.replace("*", " * ").split() if w != "const"]
    if returns and words == ["char", "*"]:
        return ctypes.c_char_p
    if "*" in words and not returns:
        return P
    kind = " ".join(words if returns else words[:-1])
    if kind not in SCALARS:
        raise DenetHipError("include/denet_hip.h: %s: no ctypes type for `%s`" % (where, decl.strip()))
    return SCALARS[kind]


def parse_header(text):
    """C text of the header -> (signatures {name: (restype, argtypes)}, defines {name: int}, structs {name: fields}).
    Strict: every `denet_<name>(` outside a comment has to be a whole `ret denet_<name>(args);` of known types."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(DENET_\w+)[ \t]*(.*?)[ \t]*$", text, re.M):
        if value:                                        # (the include guard has none)
            if not re.fullmatch(r"\(?-?\d+\)?", value):
                raise DenetHipError("include/denet_hip.h: #define %s: `%s` is not an integer" % (name, value))
            defines[name] = int(value.strip("()"))
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    structs = {}

    def take_struct(m):
        fields = [f for f in m.group(2).split(";") if f.strip()]
        structs[m.group(1)] = [(f.split()[-1].lstrip("*"), _ctype(f, "struct " + m.group(1))) for f in fields]
        return ""
    text = re.sub(r"typedef\s+struct\s+(denet_\w+)\s*\{([^}]*)\}\s*\1\s*;", take_struct, text)
    signatures = {}
    for statement in text.split(";"):
        named = re.search(r"\b(denet_\w+)\s*\(", statement)
        if not named:
            continue
        m = re.fullmatch(r"\s*([\w\s*]+?)\b(denet_\w+)\s*\(([^()]*)\)\s*", statement)
        if not m:
            raise DenetHipError("include/denet_hip.h: %s: not one whole declaration `ret %s(args);`" % ((named.group(1),) * 2))
        ret, name, args = m.groups()
        if name in signatures:
            raise DenetHipError("include/denet_hip.h: %s is declared twice" % name)
        args = [] if args.strip() == "void" else args.split(",")
        signatures[name] = (_ctype(ret, name, returns=True), [_ctype(a, name) for a in args])
    return signatures, defines, structs


def _read_header():
    if not os.path.exists(HEADER_PATH):
        raise DenetHipError("include/denet_hip.h is missing (%s): the binding is derived from it" % HEADER_PATH)
    with open(HEADER_PATH) as f:
        return parse_header(f.read())


# name -> (restype, argtypes) of every entry point; DENET_* -> value; the one struct that crosses the boundary, defined once
SIGNATURES, DEFINES, _STRUCTS = _read_header()


class BnLink(ctypes.Structure):
    """denet_bn_link"""
    _fields_ = _STRUCTS["denet_bn_link"]


_lib = None


def load():
    """Loads the library (once). Raises if it has not been built: there is no CPU fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DenetHipError(
            "libdenet_hip.so is missing (%s): run `python -m denet_amd.build` / __graft_entry__.build() first. "
            "The DeNet hot path has no CPU fallback." % LIB_PATH)
    # torch first: its wheel carries the HIP runtime (libamdhip64) that owns the streams and the memory this library is handed;
    # loaded the other way round the dynamic linker would bind the library to a second copy of the runtime (/opt/rocm) in which
    # torch's streams do not exist ("no ROCm-capable device" at the first launch)
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().denet_last_error().decode("utf-8", "replace")
        raise DenetHipError("%s failed (rc=%d): %s" % (what or "denet call", rc, msg))


def ptr(t):
    """device (or host) pointer of a torch tensor / None"""
    return None if t is None else t.data_ptr()


def stream_ptr():
    import torch
    return torch.cuda.current_stream().cuda_stream
