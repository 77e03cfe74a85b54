"""ctypes binding of the C ABI declared in include/catfish_hip.h and, for the entry points added next to it,
include/catfish_hip_ext.h.

The headers are the only statement of that ABI: the signature tables, the constants and the layout of the four structs are read
from them once, at import (``parse_header``); nothing here restates a signature.

The product path has NO CPU fallback: if the HIP library has not been built
(``python -c "import __graft_entry__ as g; g.build()"`` or
``python -m catfish_amd.build``) importing a symbol from here raises.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB_PATH = os.path.join(_HERE, "csrc", "libcatfish_hip.so")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "catfish_hip.h")
EXT_HEADER = os.path.join(os.path.dirname(_HERE), "include", "catfish_hip_ext.h")


def debug_knobs_on():
    """``CATFISH_DEBUG_KNOBS=1``: the ONE switch behind which the A/B knobs of tools/ and tests live -- the library's
    ``CATFISH_*`` kernel-selection variables (csrc/catfish_hip.hip ``cf_knob``) and ``CATFISH_HIP_LIB`` here.  Without it a
    stray environment variable changes nothing; with it every knob that takes effect is named on stderr."""
    return os.environ.get("CATFISH_DEBUG_KNOBS", "0") not in ("", "0")


def _lib_path():
    override = os.environ.get("CATFISH_HIP_LIB")
    if override and debug_knobs_on():
        import sys
        sys.stderr.write("catfish_amd: debug knob CATFISH_HIP_LIB=%s is active (NOT the in-tree library)\n" % override)
        return override
    return DEFAULT_LIB_PATH


LIB_PATH = DEFAULT_LIB_PATH


class NativeLibraryMissing(RuntimeError):
    pass


class CatfishHipError(RuntimeError):
    def __init__(self, code, msg):
        RuntimeError.__init__(self, "catfish_hip error %d: %s" % (code, msg))
        self.code = code


# ---------------------------------------------------------------------- the header as the table
_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
            "float": C.c_float, "double": C.c_double}
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(-?\d+)[ \t]*$", re.M)
_STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*\w+\s*;")
_OPAQUE = re.compile(r"typedef\s+struct\s+\w+\s+\w+")
_DECLARATION = re.compile(r"([^()]*?)\b(cf_\w+)\s*\(([^()]*)\)")


def _ctype(text, where, is_return=False):
    """One return type, parameter or struct field of the header -> its ctypes type; ``const`` and the name are dropped.
    ``char*`` is ``c_char_p``, every other pointer or ``[]`` parameter ``c_void_p``, ``void`` as a return type None."""
    words = re.sub(r"\bconst\b", " ", text).split("[")[0].replace("*", " * ").split()
    stars = words.count("*") + ("[" in text)
    if stars:
        return C.c_char_p if stars == 1 and words[0] == "char" else C.c_void_p
    if is_return and words == ["void"]:
        return None
    if not words or words[0] not in _SCALARS or len(words) > (1 if is_return else 2):
        raise ValueError("catfish_hip.h: cannot type `%s` in `%s`" % (" ".join(text.split()), where))
    return _SCALARS[words[0]]


def parse_header(text):
    """The text of include/catfish_hip.h -> (symbols, constants, structs): ``{name: (restype, [argtypes])}`` of every
    ``ret cf_name(params);`` declaration, ``{NAME: value}`` of every ``#define NAME <integer>`` and ``{name: [(field, ctype)]}``
    of every ``typedef struct`` with a body (a pointer field is ``c_void_p``).  Comments and preprocessor lines are stripped
    first.  Anything else raises ValueError and names the declaration -- an unknown scalar type, a function-pointer parameter,
    a ``cf_*(`` without its ``);`` -- so that a header edit never drops a symbol silently."""
    text = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    constants = {m.group(1): int(m.group(2)) for m in _DEFINE.finditer(text)}
    text = re.sub(r'extern\s+"C"\s*\{', " ", re.sub(r"^[ \t]*#[^\n]*$", " ", text, flags=re.M))
    structs = {}
    for m in _STRUCT.finditer(text):
        fields = [f for f in m.group(2).split(";") if f.strip()]
        structs[m.group(1)] = [(f.split("[")[0].replace("*", " ").split()[-1], _ctype(f, "struct " + m.group(1))) for f in fields]
    symbols = {}
    for statement in _STRUCT.sub(" ", text).split(";"):
        statement = " ".join(statement.split())
        named = re.search(r"\b(cf_\w+)\s*\(", statement)
        if named is None:
            if statement not in ("", "}") and not _OPAQUE.fullmatch(statement):      # "}" closes extern "C"
                raise ValueError("catfish_hip.h: cannot parse `%s`" % statement[:160])
            continue
        m = _DECLARATION.fullmatch(statement)
        if m is None:
            raise ValueError("catfish_hip.h: cannot parse the declaration of %s: `%s`" % (named.group(1), statement[:160]))
        name, params = m.group(2), m.group(3).strip()
        symbols[name] = (_ctype(m.group(1), name, is_return=True),
                         [] if params in ("", "void") else [_ctype(p, name) for p in params.split(",")])
    return symbols, constants, structs


def _read_header(path=None):
    path = HEADER if path is None else path
    try:
        with open(path) as fh:
            return fh.read()
    except OSError as e:
        raise NativeLibraryMissing("%s cannot be read (%s): the binding takes every signature from it" % (path, e.strerror))


# name -> (restype, argtypes) of every symbol the header declares; parsed here, once per process
SYMBOLS, _CONSTANTS, _STRUCTS = parse_header(_read_header())

CF_ABI_VERSION = _CONSTANTS["CF_ABI_VERSION"]
CF_OK = _CONSTANTS["CF_OK"]
CF_ERR_INVALID = _CONSTANTS["CF_ERR_INVALID"]
CF_ERR_HIP = _CONSTANTS["CF_ERR_HIP"]
CF_ERR_NOMEM = _CONSTANTS["CF_ERR_NOMEM"]
CF_ERR_IO = _CONSTANTS["CF_ERR_IO"]
CF_WINDOW = _CONSTANTS["CF_WINDOW"]
CF_PROF_SLOTS = _CONSTANTS["CF_PROF_SLOTS"]
PRECISIONS = {"fp32": _CONSTANTS["CF_PREC_FP32"], "bf16x3": _CONSTANTS["CF_PREC_BF16X3"], "bf16": _CONSTANTS["CF_PREC_BF16"]}

# the second header's table: the core one above stays what include/catfish_hip.h declares, this one is everything next to it
EXT_SYMBOLS, _EXT_CONSTANTS, _ = parse_header(_read_header(EXT_HEADER))
CF_EXT_ABI_VERSION = _EXT_CONSTANTS["CF_EXT_ABI_VERSION"]
CF_CLIP_SCALE = _EXT_CONSTANTS["CF_CLIP_SCALE"]
CF_CLIP_SKIP_NONFINITE = _EXT_CONSTANTS["CF_CLIP_SKIP_NONFINITE"]
CF_CLIP_SKIPPED = _EXT_CONSTANTS["CF_CLIP_SKIPPED"]
CF_CLIP_CHUNK = _EXT_CONSTANTS["CF_CLIP_CHUNK"]

_f32p = C.POINTER(C.c_float)


# The four structs stay hand-written (build_weight_structs needs their typed pointers) and are held to the header below.
class cf_hparams(C.Structure):
    _fields_ = [("layer_size", C.c_int32), ("n_layers", C.c_int32),
                ("layer_size_res", C.c_int32), ("n_layers_res", C.c_int32),
                ("window", C.c_int32), ("bn_epsilon", C.c_float),
                ("max_windows_per_pass", C.c_int64), ("n_streams", C.c_int32), ("precision", C.c_int32), ("fuse_layers", C.c_int32)]


class cf_conv_bn(C.Structure):
    _fields_ = [("kernel", _f32p), ("bias", _f32p), ("gamma", _f32p), ("beta", _f32p),
                ("moving_mean", _f32p), ("moving_variance", _f32p),
                ("ksize", C.c_int32), ("cin", C.c_int32)]


class cf_gru_dir(C.Structure):
    _fields_ = [("gates_kernel", _f32p), ("gates_bias", _f32p),
                ("candidate_kernel", _f32p), ("candidate_bias", _f32p),
                ("cin", C.c_int32)]


class cf_weights(C.Structure):
    _fields_ = [("conv", C.POINTER(cf_conv_bn)), ("gru", C.POINTER(cf_gru_dir)),
                ("dense_kernel", _f32p), ("dense_bias", _f32p)]


def check_struct(cls, fields):
    """Raise unless the ctypes Structure ``cls`` has the fields the header gives (``parse_header``'s ``[(name, ctype)]``): the
    same names in the same order, each the same scalar type or, where the header has a pointer, a pointer."""
    mine = [(name, C.c_void_p if hasattr(kind, "contents") else kind) for name, kind in cls._fields_]
    if mine != fields:
        header, binding = (", ".join("%s %s" % (kind.__name__, name) for name, kind in rows) for rows in (fields, mine))
        raise ValueError("catfish_hip.h: struct %s is {%s} in the header, {%s} in the binding" % (cls.__name__, header, binding))


for _cls in (cf_hparams, cf_conv_bn, cf_gru_dir, cf_weights):
    if _cls.__name__ not in _STRUCTS:
        raise ValueError("catfish_hip.h: no typedef struct %s" % _cls.__name__)
    check_struct(_cls, _STRUCTS[_cls.__name__])

_lib = None


def _preload_torch_hip_runtime():
    """One process must hold ONE HIP/ROCr runtime.

    PyTorch-ROCm wheels bundle their own libamdhip64.so (soname libamdhip64.so.7).  If our
    library pulled in the system copy first, torch would later load its bundled copy next to
    it and the second ROCr instance finds no GPU ("No HIP GPUs are available").  Loading
    torch's copy first makes the dynamic linker satisfy our NEEDED libamdhip64.so.7 with
    that same object (soname match).  Without torch installed the system runtime is used.
    """
    try:
        import torch
    except ImportError:
        return
    cand = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def lib():
    """Load (once) and return the C-ABI library; raise loudly when it is absent."""
    global _lib, LIB_PATH
    if _lib is None:
        path = _lib_path()
        if not os.path.exists(path):
            raise NativeLibraryMissing(
                "%s not found: the HIP extension has not been built. Run "
                "`python -m catfish_amd.build` (needs hipcc). There is no CPU fallback." % path)
        _preload_torch_hip_runtime()
        handle = C.CDLL(path)
        for query, what, want in (("cf_abi_version", "ABI", CF_ABI_VERSION), ("cf_ext_abi_version", "extension ABI", CF_EXT_ABI_VERSION)):
            try:
                abi = getattr(handle, query)
            except AttributeError:
                abi = None
            built = int(abi()) if abi is not None else None
            if built != want:
                raise NativeLibraryMissing("%s was built for %s %s, this binding needs %d: rebuild it "
                                           "(`python -m catfish_amd.build --force`)" % (path, what, built, want))
        for name, (res, args) in list(SYMBOLS.items()) + list(EXT_SYMBOLS.items()):
            try:
                fn = getattr(handle, name)
            except AttributeError:                         # a library of the same ABI number from before the symbol was added
                raise NativeLibraryMissing("%s has no %s: rebuild it (`python -m catfish_amd.build --force`)" % (path, name))
            fn.restype = res
            fn.argtypes = args
        _lib, LIB_PATH = handle, path
    return _lib


def check(rc):
    if rc != CF_OK:
        msg = lib().cf_last_error().decode("utf-8", "replace")
        if rc == CF_ERR_INVALID:
            raise ValueError("catfish_hip: " + msg)
        if rc == CF_ERR_IO:
            raise OSError("catfish_hip: " + msg)
        raise CatfishHipError(rc, msg)


# ---------------------------------------------------------------------- the one way to pass a tensor, a stream or an array
def _p(t):
    """A torch tensor's first element as the ``void*`` the C ABI takes; None (an optional buffer left out) stays None = NULL."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream_ptr(stream):
    """A ``torch.cuda.Stream`` as the ``void* stream`` of the launch functions."""
    return C.c_void_p(stream.cuda_stream)


def current_stream_ptr(torch, dev):
    """torch's current stream on ``dev`` as the ``void* stream`` of the launch functions."""
    return stream_ptr(torch.cuda.current_stream(dev))


def np_ptr(a):
    """A contiguous numpy array's data as ``void*`` (the pointer keeps the array alive); None stays None = NULL."""
    if a is None:
        return None
    if not a.flags.c_contiguous:
        raise ValueError("np_ptr needs a C-contiguous array")
    return a.ctypes.data_as(C.c_void_p)


def _as_f32(a):
    arr = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    return arr, arr.ctypes.data_as(_f32p)


def conv_name(j):
    return "conv1d" if j == 0 else "conv1d_%d" % j


def bn_name(j):
    return "batch_normalization" if j == 0 else "batch_normalization_%d" % j


def gru_prefix(layer, direction):
    return "stack_bidirectional_rnn/cell_%d/bidirectional_rnn/%s/gru_cell" % (layer, direction)


def build_weight_structs(weights, n_layers, n_layers_res):
    """dict {TF variable name: array} -> (cf_weights, keepalive list).

    Variable names are the ones TF auto-assigns while RNN.__init__ builds the
    graph (reference rnn_class.py:37-39, resnet_class.py:17-25).
    """
    keep = []

    def ptr(name):
        if name not in weights:
            raise ValueError("checkpoint is missing tensor %r" % name)
        arr, p = _as_f32(weights[name])
        keep.append(arr)
        return arr, p

    convs = (cf_conv_bn * max(1, 4 * n_layers_res))()
    for j in range(4 * n_layers_res):
        k_arr, k_ptr = ptr(conv_name(j) + "/kernel")
        if k_arr.ndim != 3:
            raise ValueError("%s/kernel must be [K, Cin, Cout]" % conv_name(j))
        c = convs[j]
        c.kernel = k_ptr
        c.bias = ptr(conv_name(j) + "/bias")[1]
        c.gamma = ptr(bn_name(j) + "/gamma")[1]
        c.beta = ptr(bn_name(j) + "/beta")[1]
        c.moving_mean = ptr(bn_name(j) + "/moving_mean")[1]
        c.moving_variance = ptr(bn_name(j) + "/moving_variance")[1]
        c.ksize = k_arr.shape[0]
        c.cin = k_arr.shape[1]
    grus = (cf_gru_dir * (2 * n_layers))()
    for layer in range(n_layers):
        for d, dname in enumerate(("fw", "bw")):
            p = gru_prefix(layer, dname)
            gk_arr, gk_ptr = ptr(p + "/gates/kernel")
            ck_arr, ck_ptr = ptr(p + "/candidate/kernel")
            g = grus[2 * layer + d]
            g.gates_kernel = gk_ptr
            g.gates_bias = ptr(p + "/gates/bias")[1]
            g.candidate_kernel = ck_ptr
            g.candidate_bias = ptr(p + "/candidate/bias")[1]
            h = ck_arr.shape[1]
            if gk_arr.shape != (ck_arr.shape[0], 2 * h):
                raise ValueError("%s: gates/candidate kernel shapes disagree" % p)
            g.cin = ck_arr.shape[0] - h
    w = cf_weights()
    w.conv = convs
    w.gru = grus
    w.dense_kernel = ptr("final_fully_connected/kernel")[1]
    w.dense_bias = ptr("final_fully_connected/bias")[1]
    keep.extend([convs, grus])
    return w, keep
