"""The binding that denet_amd/lib.py derives from include/denet_hip.h (no GPU): known answers written out by hand for entries that
together use every type of the header, the parser's refusals, the integer defines and the one bound struct. That header and
binding agree in all declarations is tests/test_host.py::test_cabi_exports_every_declared_symbol."""
import ctypes

import pytest

import cabi
from denet_amd import lib as dlib, ops

P, I, L, F, Z, D, U64 = (ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_size_t, ctypes.c_double,
                         ctypes.c_uint64)
KNOWN = {
    "denet_last_error": (ctypes.c_char_p, []),                                           # const char* return, (void)
    "denet_loss_workspace_bytes": (Z, []),                                               # size_t return, (void)
    "denet_bn_workspace_bytes": (Z, [L, I]),
    "denet_device_info": (I, [I, P, P, P, I]),                                           # char*
    "denet_soft_nms_batch_host": (L, [P, P, P, P, I, I, I, F, F, P, P, P, P, L]),        # long return
    "denet_host_detect_targets": (I, [P, P, P, P, I, I, I, I, I, I, D, D, P, P, P, P]),  # doubles; a comment inside the list
    "denet_host_resample_coeffs": (I, [I, D, D, I, I, P, P, L]),
    "denet_dropout": (I, [P, P, I, I, I, I, F, U64, P]),                                 # uint64_t
    # const unsigned char* const*, unsigned long long*
    "denet_image_render_batch": (I, [I] + [P] * 13 + [I, I, P, P, Z, P, P, P, Z, P, P]),
    "denet_image_finish": (I, [P, P, I, I, I, I, P, P, P, P, I, P, P]),                  # unsigned long long*
    "denet_conv_wino_fwd_fold": (I, [P] * 7 + [I, P, Z, P, P, Z] + [I] * 6 + [P]),       # const denet_bn_link*
    "denet_bn_relu_pool_fwd_train": (I, [P] * 10 + [I, P] + [I] * 9 + [F, F, P]),        # unsigned char*, const double*, void*
    "denet_ema_update": (I, [P, P, L, F, P]),                                            # a long between pointers
}


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_answers(name):
    res, args = dlib.SIGNATURES[name]
    assert res is KNOWN[name][0] and list(args) == KNOWN[name][1], (name, res, args)


@pytest.mark.parametrize("text, entry", [
    ("int denet_good(int a);\nint denet_narrow(float* x, short n);\n", "denet_narrow"),          # a type outside the map
    ("int denet_open(int a)\nint denet_good(void);\n", "denet_open"),                             # no `;`
    ("struct pair denet_pair(int a);\n", "denet_pair"),                                           # unknown return type
    ("float* denet_buffer(int a);\n", "denet_buffer"),                                            # (only `const char*` is a known pointer return)
    ("int denet_unnamed(int);\n", "denet_unnamed"),                                               # a parameter without a name
    ("/* x */ int denet_twice(int a);\nint denet_twice(int a);\n", "denet_twice"),
])
def test_parser_refuses_and_names_the_entry(text, entry):
    with pytest.raises(dlib.DenetHipError, match=r"\b%s\b" % entry):
        dlib.parse_header(text)


def test_parser_reads_what_it_should_and_skips_comments():
    sigs, defs, structs = dlib.parse_header(
        "#define DENET_HIP_H\n#define DENET_ERR_ARG (-1000) /* denet_not_this( */\n#define DENET_ONE 1\n"
        "/* int denet_in_a_comment(short x); */\ntypedef struct denet_s { const float* p; int n; } denet_s;\n"
        "size_t denet_f(const denet_s* s, /* a, b */ long n,\n    hipStream_t stream);\n")
    assert sigs == {"denet_f": (Z, [P, L, P])} and defs == {"DENET_ERR_ARG": -1000, "DENET_ONE": 1}
    assert structs == {"denet_s": [("p", P), ("n", I)]}
    with pytest.raises(dlib.DenetHipError, match="DENET_HALF"):
        dlib.parse_header("#define DENET_HALF 0.5\n")


def test_missing_header_names_the_path(monkeypatch, tmp_path):
    gone = str(tmp_path / "include" / "denet_hip.h")
    monkeypatch.setattr(dlib, "HEADER_PATH", gone)
    with pytest.raises(dlib.DenetHipError, match="denet_hip.h is missing") as e:
        dlib._read_header()
    assert gone in str(e.value)


def test_defines():
    assert dlib.DEFINES == {"DENET_ERR_ARG": -1000, "DENET_TAP_THEANO": 0, "DENET_TAP_CUDA": 1, "DENET_TAP_BILINEAR": 2,
                            "DENET_ACT_SIGMOID": 1, "DENET_ACT_TANH": 2, "DENET_ACT_ELU": 3, "DENET_ACT_SOFTPLUS": 4,
                            "DENET_SOLVER_SGD": 0, "DENET_SOLVER_NESTEROV": 1}
    assert dlib.DEFINES == cabi.defines()
    assert ops.ACT_KINDS == {"sigmoid": dlib.DEFINES["DENET_ACT_SIGMOID"], "tanh": dlib.DEFINES["DENET_ACT_TANH"],
                             "elu": dlib.DEFINES["DENET_ACT_ELU"], "softplus": dlib.DEFINES["DENET_ACT_SOFTPLUS"]}
    assert list(ops.ACT_KINDS) == ["sigmoid", "tanh", "elu", "softplus"]


def test_bn_link_is_bound_once():
    fields = cabi.bn_link_fields()
    assert [n for n, _ in fields] == ["x", "aux", "y", "gamma", "beta", "mean", "invstd", "coef", "out", "relu"]
    assert list(dlib.BnLink._fields_) == fields
    assert all(t is P for _, t in fields[:-1]) and fields[-1][1] is I
    a = ops._bn_link_struct(None, None, None, None, None, None, None, None, None, True)
    b = ops._bn_link_struct(None, None, None, None, None, None, None, None, None, False)
    assert type(a) is type(b) is dlib.BnLink and (a.relu, b.relu, a.x) == (1, 0, None)
