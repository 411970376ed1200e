"""CPU-side checks of the drop-in boundary.  include/parsenet_hip.h is the one place a signature is written: the
compiler holds every definition in csrc/ to it (csrc/common.h includes it), the ctypes table is parsed from it, and
the built library exports exactly what it declares."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "parsenet_hip.h")
CSRC = os.path.join(ROOT, "parsenet_codebase_amd", "csrc")
LLVM_NM = "/opt/rocm/llvm/bin/llvm-nm"


def _declarations():
    """{name: number of parameters}, counted by this file's own regex (not by the package's parser)."""
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {name: len([p for p in params.split(",") if p.strip() not in ("", "void")])
            for name, params in re.findall(r"\b(pn_[a-z0-9_]+)\s*\(([^)]*)\)", txt)}


def _declared():
    return sorted(_declarations())


@pytest.fixture(scope="module")
def lib_path():
    from parsenet_codebase_amd import build
    return build.build(verbose=False)


def test_header_declares_something():
    names = _declared()
    assert "pn_chamfer_nn_f32" in names and "pn_last_error" in names


def test_library_exports_every_declared_symbol(lib_path):
    """Both ways: the unmangled dynamic pn_* text symbols of the library are the header's declarations."""
    tool = shutil.which("nm") or (LLVM_NM if os.path.exists(LLVM_NM) else None)
    assert tool, "neither nm nor %s: cannot read the library's exports" % LLVM_NM
    out = subprocess.run([tool, "-D", "--defined-only", lib_path], check=True, capture_output=True, text=True).stdout
    rows = [line.split() for line in out.splitlines()]
    exported = sorted(r[2] for r in rows if len(r) == 3 and r[1] == "T" and r[2].startswith("pn_"))
    declared = _declared()
    assert not sorted(set(declared) - set(exported)), "declared in the header but not exported"
    assert not sorted(set(exported) - set(declared)), "exported but not declared in the header"
    lib = ctypes.CDLL(lib_path)
    assert all(hasattr(lib, n) for n in declared)


def _includes(path, seen):
    """The files of csrc/ that ``path`` includes, directly or through them."""
    for name in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(path).read(), flags=re.M):
        inc = os.path.join(CSRC, name)
        if name not in seen and os.path.exists(inc):
            seen.add(name)
            _includes(inc, seen)
    return seen


def test_every_definition_is_compiled_against_the_header():
    """csrc/common.h includes the public header, and every translation unit that defines an entry point includes
    common.h (some through split_common.h / knn_common.h)."""
    assert re.search(r'^#include "parsenet_hip.h"', open(os.path.join(CSRC, "common.h")).read(), flags=re.M)
    units = [f for f in sorted(os.listdir(CSRC)) if f.endswith(".hip")]
    defining = []
    for f in units:
        files = [f] + sorted(_includes(os.path.join(CSRC, f), set()))
        if any(re.search(r'^extern "C"', open(os.path.join(CSRC, g)).read(), flags=re.M) for g in files):
            defining.append(f)
            assert "common.h" in files, "%s defines entry points without csrc/common.h" % f
    assert len(defining) >= 18 and "meanshift_rows.hip" in defining


@pytest.mark.parametrize("params,ok", [("void", True), ("int", False)])
def test_the_compiler_refuses_a_definition_that_differs_from_the_header(tmp_path, params, ok):
    from parsenet_codebase_amd import build
    src = tmp_path / "unit.hip"
    src.write_text('#include "common.h"\nextern "C" int pn_abi_version(%s) { return 0; }\n' % params)
    flags = [f for f in build.FLAGS if f.startswith(("-std", "-I"))]
    r = subprocess.run([build.HIPCC, "--offload-arch=gfx950", "-fsyntax-only", "--cuda-host-only", "-I" + CSRC] +
                       flags + [str(src)], capture_output=True, text=True)
    if ok:
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode != 0 and "conflicting types for 'pn_abi_version'" in r.stderr, r.stderr


def test_parser_is_strict():
    from parsenet_codebase_amd._lib import parse_header
    c = ctypes
    sigs, consts = parse_header("""
        /* a comment with a declaration in it: int pn_not_this(int a); */
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define PN_ABI_VERSION 7
        #define PN_ERR_SOMETHING (-9)
        #define PN_TWO_LINES \\
            12
        const char* pn_name(void);   // int pn_nor_this(void);
        void pn_nothing(void);
        size_t pn_many(const float* const* xs, const int* cs, char* name, const char* text,
                       unsigned long long* out3, long long n, double eps, float f,
                       int k, size_t bytes, void** pp,
                       void* stream);
        char* pn_plain_pointer(unsigned char* sel);
        #ifdef __cplusplus
        }
        #endif
    """)
    assert consts == {"PN_ABI_VERSION": 7, "PN_ERR_SOMETHING": -9, "PN_TWO_LINES": 12}
    assert sigs == {
        "pn_name": (c.c_char_p, []),
        "pn_nothing": (None, []),
        "pn_many": (c.c_size_t, [c.c_void_p, c.c_void_p, c.c_char_p, c.c_void_p, c.c_void_p, c.c_longlong,
                                 c.c_double, c.c_float, c.c_int, c.c_size_t, c.c_void_p, c.c_void_p]),
        "pn_plain_pointer": (c.c_void_p, [c.c_void_p]),
    }
    for bad, named in [("int pn_f(unsigned n);", "pn_f"),                       # a scalar outside the map
                       ("int pn_f(short n);", "pn_f"),
                       ("int64_t pn_f(void);", "pn_f"),                         # ... as a return type too
                       ("int pn_f(int (*cb)(int, int), void* stream);", "pn_f"),  # function pointer
                       ("int pn_f;", "pn_f"),                                   # no parameter list
                       ("int pn_f(struct pn_opts opts);", "pn_f"),              # struct by value
                       ("struct pn_opts pn_f(void);", "pn_f"),
                       ("int pn_f(int);", "pn_f"),                              # parameters are named
                       ("int pn_f(float x[3]);", "pn_f"),
                       ("int pn_ok(int a); typedef int pn_t;", "pn_t")]:
        with pytest.raises(ValueError, match=named):
            parse_header(bad)


def test_ctypes_table_matches_header(lib_path):
    from parsenet_codebase_amd import _lib
    want = _declarations()
    assert sorted(_lib.SIGNATURES) == sorted(want) and len(want) >= 121
    assert {n: len(args) for n, (_, args) in _lib.SIGNATURES.items()} == want
    assert _lib.SIGNATURES["pn_prof_get"] == (ctypes.c_int, [ctypes.c_int, ctypes.c_char_p, ctypes.c_int,
                                                             ctypes.c_void_p, ctypes.c_void_p])
    assert _lib.SIGNATURES["pn_adam_flat_f32"][1][4:9] == [ctypes.c_longlong] + [ctypes.c_float] * 4
    assert _lib.CONSTANTS["PN_ERR_UNSUPPORTED"] == -4 and _lib.CONSTANTS["PN_MS_KERNEL_EPANECHNIKOV"] == 1
    lib = _lib.load()
    assert lib.pn_abi_version() == _lib.ABI_VERSION == _lib.CONSTANTS["PN_ABI_VERSION"] == 23
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_product_refuses_cpu_tensors(lib_path):
    import torch
    from parsenet_codebase_amd import kernels
    with pytest.raises(RuntimeError):
        kernels.chamfer_nn(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3))
