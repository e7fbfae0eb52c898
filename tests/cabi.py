"""A second reading of include/denet_hip.h, for the tests that compare the header with the binding: it shares no code with the
parser in denet_amd/lib.py, so `header and binding agree` stays a comparison of two things."""
import ctypes
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "denet_hip.h")
KINDS = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
         "uint64_t": ctypes.c_uint64, "hipStream_t": ctypes.c_void_p, "const char*": ctypes.c_char_p}


def _texts():
    """the header, and the same with every comment blanked character for character (offsets agree)"""
    hdr = open(HEADER).read()
    return hdr, re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), hdr, flags=re.S)


def _kind(arg):
    return ctypes.c_void_p if "*" in arg else KINDS[arg.replace("const ", "").split()[0]]


def _read(m, hdr):
    """(comment_text, restype, argtypes) of one matched declaration; comment_text: the words of the comment that ends right above
    it, without the line breaks and their ` * `, or "" """
    above = hdr[:m.start()].rstrip()
    comment = above[above.rindex("/*") + 2:-2] if above.endswith("*/") else ""
    args = [a.strip() for a in m.group(3).split(",")]
    return (" ".join(w for w in comment.split() if w != "*"), KINDS[" ".join(m.group(1).split())],
            [_kind(a) for a in args if a != "void"])


def declaration(name):
    hdr, bare = _texts()
    m = re.search(r"\n([a-z_ ]+?\**)\s*(%s)\s*\(([^)]*)\)\s*;" % name, bare)
    assert m, name
    return _read(m, hdr)


def declarations():
    """name -> (comment_text, restype, argtypes) of every declared entry point"""
    hdr, bare = _texts()
    return {m.group(2): _read(m, hdr) for m in re.finditer(r"\n([a-z_ ]+?\**)\s*(denet_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", bare)}


def bn_link_fields():
    """[(name, ctypes type)] of the header's `typedef struct denet_bn_link`"""
    m = re.search(r"typedef struct denet_bn_link \{(.*?)\} denet_bn_link;", _texts()[1], re.S)
    return [(f.split()[-1], _kind(f)) for f in m.group(1).split(";") if f.strip()]


def defines():
    """DENET_* -> value of every #define with an integer value"""
    return {n: int(v) for n, v in re.findall(r"\n#define (DENET_[A-Z0-9_]+) \(?(-?[0-9]+)\)?", _texts()[1])}
