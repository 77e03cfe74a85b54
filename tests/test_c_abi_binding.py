"""The binding's table is the header: what ``_native.parse_header`` makes of include/catfish_hip.h (host only, no library)."""
import ctypes as C
import os

import pytest

from catfish_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR, I64, I32, U32, F32 = C.c_void_p, C.c_int64, C.c_int32, C.c_uint32, C.c_float


@pytest.fixture(scope="module")
def real():
    with open(os.path.join(ROOT, "include", "catfish_hip.h")) as fh:
        return N.parse_header(fh.read())


# ---------------------------------------------------------------------- the parser on literal snippets
def test_multi_line_declaration_with_comment_inside_the_parameters():
    symbols, _, _ = N.parse_header("""
        int cf_span(cf_model* m, const float* probs, const float* signal /* NULL: no level sums */,
                    int64_t n_reads,   // trailing remark
                    float threshold, double* sums /* [max_runs][3]: sum p, sum x */,
                    void* stream);
    """)
    assert symbols == {"cf_span": (C.c_int, [PTR, PTR, PTR, I64, F32, PTR, PTR])}


def test_void_and_empty_parameter_lists_and_returns():
    symbols, _, _ = N.parse_header("int cf_chunk(void);\nint64_t cf_bytes();\nvoid cf_destroy(cf_model* m);\nuint32_t cf_crc(const void* d, uint32_t crc);")
    assert symbols == {"cf_chunk": (C.c_int, []), "cf_bytes": (I64, []), "cf_destroy": (None, [PTR]), "cf_crc": (U32, [PTR, U32])}


def test_char_pointers_are_c_char_p_as_return_and_as_parameter():
    symbols, _, _ = N.parse_header("const char* cf_name(int slot);\nint cf_open(const char* dir, char* out, const char** list, uint8_t* bytes);")
    assert symbols["cf_name"] == (C.c_char_p, [C.c_int])
    assert symbols["cf_open"] == (C.c_int, [C.c_char_p, C.c_char_p, PTR, PTR])


def test_array_parameters_are_pointers():
    symbols, _, _ = N.parse_header("#define CF_SLOTS 12\nint cf_regimes(const cf_model* m, int64_t out[4]);\n"
                                   "int cf_read(cf_model* m, double ms[CF_SLOTS], int64_t launches[CF_SLOTS]);")
    assert symbols == {"cf_regimes": (C.c_int, [PTR, PTR]), "cf_read": (C.c_int, [PTR, PTR, PTR])}


def test_define_directly_in_front_of_a_declaration():
    symbols, constants, _ = N.parse_header("/* timing */\n#define CF_PROF_SLOTS 12\nint cf_profile_enable(cf_model* m, int on);\n"
                                           "#define CF_ERR_IO -4          /* a file */\n#define CF_GUARD_H\nint cf_next(void);")
    assert symbols == {"cf_profile_enable": (C.c_int, [PTR, C.c_int]), "cf_next": (C.c_int, [])}
    assert constants == {"CF_PROF_SLOTS": 12, "CF_ERR_IO": -4}


def test_extern_c_guards_opaque_typedefs_and_structs():
    symbols, constants, structs = N.parse_header("""
        #ifndef X_H
        #define X_H
        #include <stdint.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        typedef struct cf_pair {
            const float* data;   /* [n] */
            int32_t n;
            int64_t cap; double scale;
        } cf_pair;
        typedef struct cf_model cf_model;
        int cf_make(const cf_pair* p, cf_model** out);
        #ifdef __cplusplus
        }
        #endif
        #endif /* X_H */
    """)
    assert symbols == {"cf_make": (C.c_int, [PTR, PTR])} and constants == {}
    assert structs == {"cf_pair": [("data", PTR), ("n", I32), ("cap", I64), ("scale", C.c_double)]}


@pytest.mark.parametrize("text, named", [
    ("int cf_good(int a);\nint cf_sized(cf_model* m, size_t n);", "cf_sized"),                      # an unknown scalar type
    ("int cf_wide(unsigned int n);", "cf_wide"),
    ("int cf_each(cf_model* m, void (*callback)(int, void*), void* arg);\nint cf_good(void);", "cf_each"),   # a function pointer
    ("int cf_open_end(cf_model* m, int64_t n\nint cf_good(void);", "cf_open_end"),                 # no closing ");"
    ("int cf_good(void);\nint cf_last(cf_model* m, int64_t n", "cf_last"),
    ("int cf_no_semicolon(int a)\nint cf_good(void);", "cf_no_semicolon"),
    ("size_t cf_count(void);", "cf_count"),                                                         # an unknown return type
])
def test_what_cannot_be_typed_raises_and_names_the_declaration(text, named):
    with pytest.raises(ValueError, match=named):
        N.parse_header(text)


def test_a_statement_that_is_no_declaration_raises():
    with pytest.raises(ValueError, match="cf_table"):
        N.parse_header("int cf_good(void);\nextern int cf_table[4];")


def test_missing_header_names_the_path(monkeypatch):
    monkeypatch.setattr(N, "HEADER", os.path.join(ROOT, "include", "no_such_header.h"))
    with pytest.raises(N.NativeLibraryMissing, match="no_such_header.h"):
        N._read_header()


# ---------------------------------------------------------------------- the real header
def test_real_header_is_what_the_module_holds(real):
    symbols, constants, structs = real
    assert len(symbols) == 103 and symbols == N.SYMBOLS
    assert set(structs) == {"cf_hparams", "cf_conv_bn", "cf_gru_dir", "cf_weights"}
    from catfish_amd import build
    assert build.HEADER is N.HEADER and os.path.samefile(N.HEADER, os.path.join(ROOT, "include", "catfish_hip.h"))


def test_real_header_pinned_signatures(real):
    symbols = real[0]
    assert symbols["cf_model_destroy"] == (None, [PTR])
    assert symbols["cf_infer"] == (C.c_int, [PTR, PTR, I64, PTR, PTR])
    assert symbols["cf_crc32c"] == (U32, [PTR, I64, U32])
    assert symbols["cf_stat_files"][1][0] is C.c_char_p
    assert symbols["cf_profile_slot_name"] == (C.c_char_p, [C.c_int])
    assert symbols["cf_validation_score_chunk"] == (C.c_int, [])
    res, args = symbols["cf_base_votes"]
    assert res is C.c_int and len(args) == 22
    assert [i for i, a in enumerate(args) if a is I64] == [2, 5, 7, 12, 13, 20]
    assert [i for i, a in enumerate(args) if a is I32] == [15, 16]
    assert all(a is PTR for i, a in enumerate(args) if i not in (2, 5, 7, 12, 13, 20, 15, 16))
    res, args = symbols["cf_gru_train_backward_dropout"]
    assert res is C.c_int and len(args) == 16 and args[11:14] == [F32, U32, I32]


def test_constants_come_from_the_header(real):
    constants = real[1]
    assert [constants[k] for k in ("CF_ABI_VERSION", "CF_OK", "CF_ERR_INVALID", "CF_ERR_HIP", "CF_ERR_NOMEM", "CF_ERR_IO", "CF_WINDOW",
                                   "CF_PROF_SLOTS")] == [9, 0, -1, -2, -3, -4, 35, 12]
    assert (N.CF_ABI_VERSION, N.CF_OK, N.CF_ERR_INVALID, N.CF_ERR_HIP, N.CF_ERR_NOMEM, N.CF_ERR_IO, N.CF_WINDOW, N.CF_PROF_SLOTS) == \
        (9, 0, -1, -2, -3, -4, 35, 12)
    assert N.PRECISIONS == {"fp32": 0, "bf16x3": 1, "bf16": 2}


# ---------------------------------------------------------------------- the hand-written structs are held to the header
STRUCTS = (N.cf_hparams, N.cf_conv_bn, N.cf_gru_dir, N.cf_weights)


def _copy(cls, fields):
    return type(cls.__name__, (C.Structure,), {"_fields_": fields})


@pytest.mark.parametrize("cls", STRUCTS, ids=lambda c: c.__name__)
def test_struct_check(real, cls):
    fields = real[2][cls.__name__]
    N.check_struct(cls, fields)
    N.check_struct(_copy(cls, list(cls._fields_)), fields)
    swapped = list(cls._fields_)
    swapped[0], swapped[1] = swapped[1], swapped[0]
    with pytest.raises(ValueError, match=cls.__name__):
        N.check_struct(_copy(cls, swapped), fields)
    with pytest.raises(ValueError, match=cls.__name__):
        N.check_struct(_copy(cls, list(cls._fields_)[:-1]), fields)


@pytest.mark.parametrize("cls", STRUCTS, ids=lambda c: c.__name__)
def test_struct_check_refuses_a_widened_field(real, cls):
    """An ``int32_t`` that became ``int64_t``; cf_weights has only pointers, so there a pointer becomes an ``int64_t``."""
    fields = list(cls._fields_)
    at = next((i for i, (_n, kind) in enumerate(fields) if kind is I32), 0)
    fields[at] = (fields[at][0], I64)
    with pytest.raises(ValueError, match=cls.__name__):
        N.check_struct(_copy(cls, fields), real[2][cls.__name__])


# ---------------------------------------------------------------------- one way to pass a tensor, a stream or an array
def test_pointer_helpers():
    import numpy as np

    class Tensor(object):
        def data_ptr(self):
            return 0x1000

    class Stream(object):
        cuda_stream = 0x2000

    assert N._p(None) is None and N.np_ptr(None) is None
    p = N._p(Tensor())
    assert isinstance(p, C.c_void_p) and p.value == 0x1000
    s = N.stream_ptr(Stream())
    assert isinstance(s, C.c_void_p) and s.value == 0x2000
    a = np.arange(6, dtype=np.int64)
    q = N.np_ptr(a)
    assert isinstance(q, C.c_void_p) and q.value == a.ctypes.data
    with pytest.raises(ValueError, match="contiguous"):
        N.np_ptr(a[::2])


def test_pointer_spelling_lives_in_the_binding_only():
    """``C.c_void_p(<something>)`` and ``ctypes.data_as`` occur in the package only inside _native.py; a null handle, ``C.c_void_p()``,
    is the one thing the other modules construct."""
    import re
    pkg = os.path.join(ROOT, "catfish_amd")
    for name in sorted(os.listdir(pkg)):
        if name.endswith(".py") and name != "_native.py":
            with open(os.path.join(pkg, name)) as fh:
                src = fh.read()
            assert not re.search(r"c_void_p\((?!\))", src), name
            assert "data_as(" not in src, name
