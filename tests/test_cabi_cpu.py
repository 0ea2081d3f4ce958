"""The header reader (nvfpcc_amd/_cabi.py) and what the package derives from include/*.h with it: exact results on
small C texts, refusals of everything outside its subset, struct layouts against the host C compiler, the two whole
headers, and the Python constants that are #defines.  Host code only; nothing here touches a GPU."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from nvfpcc_amd import _cabi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = C.c_void_p


def _fields(struct):
    return [(n, t) for n, t in struct._fields_]


# ---- the reader on snippets ---------------------------------------------------------------------------------------
def test_pointer_parameters_with_const_anywhere():
    h = _cabi.read("int nvf_f(const float* const* xs, float** ys, const void* t, void* stream);")
    assert h.prototypes == {"nvf_f": (C.c_int, [P, P, P, P])}


def test_void_parameter_list_void_return_and_size_t_return():
    h = _cabi.read("int nvf_version(void);\nvoid nvf_cancel(int* q);\nsize_t nvf_bytes(void);")
    assert h.prototypes == {"nvf_version": (C.c_int, []), "nvf_cancel": (None, [P]), "nvf_bytes": (C.c_size_t, [])}


def test_scalar_parameters_keep_their_width_and_register_class():
    h = _cabi.read("int nvf_f(uint64_t seed, float g, int64_t n, uint32_t m, int32_t k, size_t bytes, double d, int i);")
    assert h.prototypes["nvf_f"] == (C.c_int, [C.c_uint64, C.c_float, C.c_int64, C.c_uint32, C.c_int32, C.c_size_t,
                                               C.c_double, C.c_int])


def test_a_declaration_over_several_lines_inside_extern_c():
    h = _cabi.read('#ifdef __cplusplus\nextern "C" {\n#endif\n'
                   "int64_t nvf_long(const int16_t* symbols,\n                 int64_t n,   /* how many */\n"
                   "                 uint8_t* out);\n#ifdef __cplusplus\n}\n#endif\n")
    assert h.prototypes == {"nvf_long": (C.c_int64, [P, C.c_int64, P])}


def test_a_declaration_inside_a_comment_is_ignored():
    h = _cabi.read("/* see\n * nvf_fake(int);\n */\nint nvf_real(int a /* nvf_other(float); */);")
    assert h.prototypes == {"nvf_real": (C.c_int, [C.c_int])}


def test_array_parameters_are_addresses():
    assert _cabi.read("int nvf_f(const float* ws[8], int n[4]);").prototypes == {"nvf_f": (C.c_int, [P, P])}


def test_struct_with_comma_declarators_and_arrays():
    h = _cabi.read("typedef struct NvfJob {\n  const float* kernel[8];\n  int32_t n[8];\n  int32_t nlayers, reserved;\n"
                   "  float* part;   /* may be NULL */\n  float g, *h;\n  uint64_t bytes;\n} NvfJob;\n"
                   "int nvf_run(const NvfJob* job, void* stream);")
    assert list(h.structs) == ["NvfJob"] and issubclass(h.structs["NvfJob"], C.Structure)
    assert _fields(h.structs["NvfJob"]) == [("kernel", P * 8), ("n", C.c_int32 * 8), ("nlayers", C.c_int32),
                                            ("reserved", C.c_int32), ("part", P), ("g", C.c_float), ("h", P),
                                            ("bytes", C.c_uint64)]
    assert C.sizeof(h.structs["NvfJob"]) == 64 + 32 + 8 + 8 + 4 + 4 + 8 + 8
    assert h.prototypes == {"nvf_run": (C.c_int, [P, P])}


def test_an_opaque_typedef_can_only_be_pointed_to():
    h = _cabi.read("typedef struct NvfCtx NvfCtx;\nint nvf_init(NvfCtx* ctx);\nint nvf_peek(const NvfCtx* ctx);")
    assert h.structs == {} and h.prototypes == {"nvf_init": (C.c_int, [P]), "nvf_peek": (C.c_int, [P])}
    with pytest.raises(ValueError, match="NvfCtx ctx"):
        _cabi.read("typedef struct NvfCtx NvfCtx;\nint nvf_init(NvfCtx ctx);")


def test_constants():
    h = _cabi.read("#ifndef NVF_X_H\n#define NVF_X_H\n#define A 3\n#define B (A * 2 + (1 << 4))\n#define E (-2)  /* c */\n"
                   "#define H 0x10\n#define CUBE(bits) (1 << (3 * (bits)))\n#define D (B - A)\n#endif\n")
    assert h.constants == {"A": 3, "B": 22, "E": -2, "H": 16, "D": 19}


# ---- the reader refuses ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text, quoted", [
    ("int nvf_f(void (*done)(int), int n);", "void (*done)(int)"),                        # a function pointer
    ("int nvf_f(half_t x);", "half_t x"),                                                   # an unknown type name
    ("int nvf_f(unsigned int x);", "unsigned int x"),
    ("typedef struct NvfB { int32_t a : 3; } NvfB;", "int32_t a : 3"),                      # a bit-field
    ("typedef struct NvfN { struct { int a; } in; int b; } NvfN;", "typedef struct NvfN"),  # a nested struct
    ("typedef struct NvfI { int a; } NvfI;\ntypedef struct NvfO { NvfI in; } NvfO;", "NvfI in"),
    ("typedef union NvfU { int a; float b; } NvfU;", "typedef union NvfU"),                 # a union
    ("typedef struct NvfV { union { int a; float b; } u; } NvfV;", "typedef struct NvfV"),
    ("#define A (7 / 2)", "#define A (7 / 2)"),                                             # a token outside the set
    ("#define A sizeof(int)", "#define A sizeof(int)"),
    ("#define A 1u", "#define A 1u"),
    ("#define A B", "#define A B"),                                                         # a name not defined earlier
    ("float* nvf_f(void);", "float* nvf_f(void)"),                                          # a pointer return
    ("int other_f(int a);", "int other_f(int a)"),                                          # not an nvf_* function
    ("int nvf_f(int);", "int"),                                                             # an unnamed parameter
    ("int nvf_f(int a)", "int nvf_f(int a)"),                                               # no semicolon
])
def test_reader_refuses(text, quoted):
    with pytest.raises(ValueError) as e:
        _cabi.read(text)
    assert quoted in str(e.value)


# ---- layouts against the compiler -----------------------------------------------------------------------------------
HEADERS = ("nvf_hip.h", "nvf_codec.h")


def _host_cc():
    """cc, else the compiler nvfpcc_amd/build.py uses, in host mode."""
    return [shutil.which("cc")] if shutil.which("cc") else [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "c"]


def test_struct_layouts_match_the_host_compiler(tmp_path):
    structs = {n: s for h in HEADERS for n, s in _cabi.read_header(h).structs.items()}
    assert len(structs) >= 7
    lines = ["#include <stddef.h>", "#include <stdio.h>"] + ['#include "%s"' % h for h in HEADERS] + ["int main(void) {"]
    for name, s in structs.items():
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        lines += ['  printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (name, f, name, f, name, f)
                  for f, _ in s._fields_]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines + ["  return 0;", "}"]) + "\n")
    subprocess.run(_host_cc() + ["-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout
    theirs = {k: tuple(map(int, v)) for k, *v in (ln.split() for ln in out.splitlines())}
    ours = {}
    for name, s in structs.items():
        ours[name] = (C.sizeof(s),)
        ours.update({f"{name}.{f}": (getattr(s, f).offset, getattr(s, f).size) for f, _ in s._fields_})
    assert ours == theirs
    assert {n: v[0] for n, v in ours.items() if "." not in n} == {
        "NvfAdamFuse": 80, "NvfLayerDesc": 88, "NvfTrunkWgrads": 152, "NvfRateJob": 200, "NvfStepTail": 168,
        "NvfStemHead": 144, "NvfPcSparseIndex": 64}


# ---- whole headers --------------------------------------------------------------------------------------------------
def test_the_codec_header_gives_its_three_functions():
    L = C.c_int64
    assert _cabi.read_header("nvf_codec.h") == _cabi.Header(
        {"nvf_ac_encode": (L, [P, P, P, L, C.c_int, C.c_int, P, L]),
         "nvf_ac_decode": (C.c_int, [P, L, P, P, L, C.c_int, C.c_int, P]),
         "nvf_codec_version": (C.c_int, [])}, {}, {})


def test_the_library_header_is_what_lib_exposes():
    h = _cabi.read_header("nvf_hip.h")
    assert len(h.prototypes) >= 140 and h.prototypes == _lib.PROTOTYPES
    for name in ("NvfStepTail", "NvfRateJob", "NvfStemHead", "NvfAdamFuse", "NvfTrunkWgrads", "NvfPcSparseIndex",
                 "NvfLayerDesc"):
        assert _fields(getattr(_lib, name)) == _fields(h.structs[name]), name
    # a float where the table once could say int, a 64-bit size where it could say c_int
    assert _lib.PROTOTYPES["nvf_adam_coefficients"] == (C.c_int, [C.c_float, C.c_float, C.c_float, C.c_int, P])
    assert _lib.PROTOTYPES["nvf_uniform"] == (C.c_int, [P, C.c_int64, C.c_uint64, C.c_uint64, P])
    assert _lib.PROTOTYPES["nvf_latent_tail_cancel"] == (None, [P])


def test_the_layer_table_dtype_is_the_headers_struct():
    from nvfpcc_amd import engine
    d = engine._DESC
    assert d == np.dtype(_lib.NvfLayerDesc) and d.itemsize == C.sizeof(_lib.NvfLayerDesc) == 88
    assert d.names == ("kernel", "kernel_init", "b", "b_init", "w_fwd", "w_bwd", "b_eff", "dim0", "dim1", "k3", "kind",
                       "quantised", "layer_id", "nbias", "pad_")
    assert [d.fields[n][1] for n in d.names] == [8 * i for i in range(7)] + [56 + 4 * i for i in range(8)]


# ---- constants ------------------------------------------------------------------------------------------------------
def test_python_constants_are_the_headers():
    from nvfpcc_amd import ops, pc_metrics, preprocess
    k = _cabi.read_header("nvf_hip.h").constants
    assert k == _lib.CONSTANTS
    for mod, name, define, value in (
            (ops, "ACT_NONE", "NVF_ACT_NONE", 0), (ops, "ACT_RELU", "NVF_ACT_RELU", 1),
            (ops, "ACT_SIGMOID", "NVF_ACT_SIGMOID", 2), (ops, "OCC_RANS_MAX_GROUP", "NVF_OCC_RANS_MAX_GROUP", 1024),
            (ops, "OCC_RANS_PAST_END", "NVF_OCC_RANS_PAST_END", 1), (ops, "OCC_RANS_BAD_STATE", "NVF_OCC_RANS_BAD_STATE", 2),
            (ops, "OCC_RANS_WORDS_LEFT", "NVF_OCC_RANS_WORDS_LEFT", 4),
            (ops, "OCC_HIER_CONTEXTS", "NVF_OCC_HIER_CONTEXTS", 3072),
            (ops, "OCC_HIER_BLOCK_WORDS", "NVF_OCC_HIER_BLOCK_WORDS", 512 + 4096 + 32768),
            (ops, "OCC_HIER_MAX_BATCH", "NVF_OCC_HIER_MAX_BATCH", 32768),
            (ops, "OCC_NBR_CONTEXTS", "NVF_OCC_NBR_CONTEXTS", 3072 + 32 * 1024),
            (pc_metrics, "CELLS", "NVF_PC_CELLS", 128 ** 3), (preprocess, "META_INTS", "NVF_PP_META_INTS", 16),
            (preprocess, "WORK_WORDS", "NVF_PP_WORK_WORDS", 11264)):
        assert getattr(mod, name) == k[define] == value, name
    assert (k["NVF_OK"], k["NVF_EINVAL"], k["NVF_EWORKSPACE"]) == (0, -1, -2)
    with pytest.raises(_lib.NvfError, match="NVF_EWORKSPACE"):
        _lib.check(-2, "x")
    with pytest.raises(_lib.NvfError, match="NVF_EINVAL"):
        _lib.check(-1, "x")


def test_reading_the_header_needs_no_library(tmp_path):
    code = ("from nvfpcc_amd import _lib; assert _lib.CONSTANTS['NVF_PP_META_INTS'] == 16; "
            "assert len(_lib.PROTOTYPES) >= 140 and _lib._lib is None; print(_lib.LIB_PATH)")
    missing = str(tmp_path / "no_such_libnvf_hip.so")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, NVF_LIB=missing),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [missing]
