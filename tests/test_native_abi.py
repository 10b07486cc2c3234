"""C ABI checks that need no GPU: the library loads, exports every symbol include/oflow.h declares, and its
argument validation / helpers behave (no kernel is launched here)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from conftest import REPO
from optical_flow import _native


def _declared_symbols():
    text = open(os.path.join(REPO, "include", "oflow.h")).read()
    return sorted(set(re.findall(r"^\s*(?:[\w*]+\s+)+\**(oflow_\w+)\s*\(", text, flags=re.M)))


def test_header_and_binding_agree():
    assert _declared_symbols() == sorted(_native.SYMBOLS)


def _declared_arity():
    """name -> number of parameters of every function the header declares (comments stripped, the parenthesised list
    split on commas, `void` = none; the header has no function-pointer parameters)."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(os.path.join(REPO, "include", "oflow.h")).read(), flags=re.S)
    arity = {}
    for name, params in re.findall(r"^\s*(?:[\w*]+\s+)+\**(oflow_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.M):
        params = params.strip()
        arity[name] = 0 if params in ("", "void") else len(params.split(","))
    return arity


def test_every_declared_symbol_has_a_signature_of_the_headers_arity():
    """A function called through ctypes without argtypes gets its pointers passed as C int."""
    lib = _native.load()
    arity = _declared_arity()
    assert sorted(arity) == _declared_symbols()
    for name, n in arity.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None, f"{name}: no argtypes declared"
        assert len(fn.argtypes) == n, f"{name}: {len(fn.argtypes)} argtypes for the header's {n} parameters"


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(_native.library_path())
    for name in _declared_symbols():
        assert hasattr(lib, name), name


def test_split_k_is_gone():
    """Split-K (the ABI version 2 descriptor fields; it never had an exported symbol of its own) is in neither the
    header nor the binding, and a descriptor of the version 2 size is refused."""
    text = open(os.path.join(REPO, "include", "oflow.h")).read()
    assert "ksplit" not in text.lower() and "split-k" not in text.lower()
    assert not [n for n, _ in _native.ConvS32Desc._fields_ if "ksplit" in n] and not hasattr(_native, "KSplit")
    d = _native.ConvS32Desc()
    d.struct_size = ctypes.sizeof(_native.ConvS32Desc) + 24  # the three version 2 fields more
    assert _native.load().oflow_conv_s32(ctypes.byref(d), None) == MODE


def test_abi_version_and_status_strings():
    lib = _native.load()
    assert lib.oflow_abi_version() == _native.ABI_VERSION
    assert lib.oflow_status_string(0) == b"ok"
    assert b"2 pixels" in lib.oflow_status_string(_native.E_TINY)
    for code in range(-7, 0):
        assert lib.oflow_status_string(code) != b"unknown oflow status"


def test_pyramid_dims_floor_halving():
    # corr.py:53 avg_pool2d(2, stride=2): floor; Sintel 55x128 -> 27x64 -> 13x32 -> 6x16
    assert _native.pyramid_dims(55, 128, 4) == [(55, 128), (27, 64), (13, 32), (6, 16)]
    assert _native.pyramid_dims(47, 156, 4) == [(47, 156), (23, 78), (11, 39), (5, 19)]
    assert _native.pyramid_dims(135, 240, 4) == [(135, 240), (67, 120), (33, 60), (16, 30)]
    with pytest.raises(RuntimeError):
        _native.pyramid_dims(10, 10, 9)


def test_argument_errors_are_reported_without_launch():
    lib = _native.load()
    ptrs = (ctypes.c_void_p * 4)()
    assert lib.oflow_corr_pyramid_f32(None, None, 1, 256, 16, 16, 4, ptrs, None) == -1
    hs = (ctypes.c_int * 4)(16, 8, 4, 1)
    ws = (ctypes.c_int * 4)(16, 8, 4, 2)
    fake = (ctypes.c_void_p * 4)(4096, 4096, 4096, 4096)
    # level 3 is 1 px high: the reference would divide by H_l - 1 = 0 (Q3) -> OFLOW_E_TINY
    assert lib.oflow_corr_lookup_f32(fake, hs, ws, 4, 4096, 1, 16, 16, 4, 4096, None) == _native.E_TINY
    assert lib.oflow_corr_lookup_f32(fake, hs, ws, 4, 4096, 1, 16, 16, 9, 4096, None) == -5
    assert lib.oflow_grid_warp_f32(4096, 4096, 1, 3, 4, 4, 7, 0, 0, 4096, None) == -6
    assert lib.oflow_grid_warp_f32(4096, 4096, 1, 3, 4, 4, 0, 5, 0, 4096, None) == -6


# ---- oflow_conv_s32's descriptor: layout, struct_size, and the status of every kind of bad call (nothing launches) ----

Desc = _native.ConvS32Desc
NULL, SHAPE, MODE, ALIGN = -1, -2, -6, -7  # OFLOW_E_*
A = 4096  # a fake 16-byte-aligned device pointer


def _host_cc():
    for cand in (os.environ.get("CC"), "cc", "gcc"):
        if cand and shutil.which(cand.split()[0]):
            return cand.split()
    return [shutil.which("hipcc"), "-x", "c"] if shutil.which("hipcc") else None


def test_conv_desc_layout_matches_the_header(tmp_path):
    """sizeof and every offsetof of oflow_conv_s32_desc, from include/oflow.h compiled as C, equal the ctypes mirror's."""
    cc = _host_cc()
    if cc is None:
        pytest.skip("no host C compiler")
    names = [n for n, _ in Desc._fields_]
    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stddef.h>\n#include <stdio.h>\n#include "oflow.h"\nint main(void) {\n'
        '  printf("sizeof %zu\\n", sizeof(oflow_conv_s32_desc));\n'
        + "".join(f'  printf("{n} %zu\\n", offsetof(oflow_conv_s32_desc, {n}));\n' for n in names)
        + "  return 0;\n}\n"
    )
    exe = tmp_path / "layout"
    subprocess.run([*cc, "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out.pop("sizeof")) == ctypes.sizeof(Desc)
    assert {n: int(v) for n, v in out.items()} == {n: getattr(Desc, n).offset for n in names}
    # every member the header declares is mirrored (44 + struct_size), so none can hide in padding
    text = open(os.path.join(REPO, "include", "oflow.h")).read()
    body = text[text.index("typedef struct oflow_conv_s32_desc {"):text.index("} oflow_conv_s32_desc;")]
    decls = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    declared = [m for stmt in decls.split(";") for m in re.findall(r"\**(\w+)\s*(?:,|$)", stmt.strip())]
    assert declared == names and len(names) == 45


# one valid call per family; each case below changes a few fields of one of them
BASE = dict(d_x=A, x_pixel_stride=8 * 128, in_groups=8, d_wpack=A, n_pad=128, d_wscale=A, N=128, B=1, H=8, W=32, kh=3, kw=3,
            block_n=128, epilogue=0, activation=0, out_scale=1.0, d_f32=A)
GRU = dict(kh=1, kw=5, epilogue=1, d_f32=None, d_y0=A, y0_pixel_stride=256, d_gru_h=A, d_gru_z=A, gru_channels=64)
FH = dict(epilogue=3, N=256, n_pad=256, block_n=64, activation=1, d_f32=None, d_fh_weights=A, d_fh_partial=A, fh_slabs=4)
# The expected statuses are what the last positional entry point (ABI version 1) returned for the same arguments
# (recorded from that library; every case fails a check, or finds no kernel, before a launch).
STATUS_CASES = [
    ("n_pad not a multiple of block_n", dict(n_pad=160), SHAPE),
    ("activation 4", dict(activation=4), MODE),
    ("epilogue 4", dict(epilogue=4), MODE),
    ("misaligned d_x", dict(d_x=A + 8), ALIGN),
    ("no destination", dict(d_f32=None), NULL),
    ("epilogue 1 without GRU pointers", dict(kh=1, kw=5, epilogue=1), NULL),
    ("d_addend with epilogue 0", dict(d_addend=A, addend_pixel_stride=128), MODE),
    ("in_format 5", dict(in_format=5), MODE),
    ("7x7 kernel", dict(kh=7, kw=7), SHAPE),
    ("flow head with d_y0", dict(FH, d_y0=A, y0_pixel_stride=1024), MODE),
    ("flow head with fh_slabs 3", dict(FH, fh_slabs=3), SHAPE),
    ("flow head without d_fh_weights", dict(FH, d_fh_weights=None), NULL),
    # further single mutations
    ("d_wscale NULL", dict(d_wscale=None), NULL),
    ("B 0", dict(B=0), SHAPE),
    ("n_pad < N", dict(N=160, n_pad=128), SHAPE),
    ("res_activation 4", dict(res_activation=4), MODE),
    ("epilogue -1", dict(epilogue=-1), MODE),
    ("x_pixel_stride 8 mod 16", dict(x_pixel_stride=1032), ALIGN),
    ("x_pixel_stride 16 mod 128", dict(x_pixel_stride=1040), ALIGN),
    ("misaligned d_wpack", dict(d_wpack=A + 4), ALIGN),
    ("block_n 16", dict(block_n=16), SHAPE),
    ("weights of 2 GiB", dict(in_groups=14564), SHAPE),
    ("s2d with odd H", dict(d_y0=A, y0_pixel_stride=512, s2d=1, H=7), SHAPE),
    ("d_nhwc row shorter than N", dict(d_nhwc=A, nhwc_pixel_stride=64), ALIGN),
    ("d_y0 stride not whole groups", dict(d_y0=A, y0_pixel_stride=192), ALIGN),
    ("misaligned d_res", dict(d_res=A + 8, res_pixel_stride=512), ALIGN),
    ("misaligned d_wfrag", dict(d_wfrag=A + 8), ALIGN),
    ("GRU gates with N != 2 * gru_channels", dict(GRU, gru_channels=128), SHAPE),
    ("GRU candidate with N != gru_channels", dict(GRU, epilogue=2), SHAPE),
    ("GRU with misaligned d_gru_h", dict(GRU, d_gru_h=A + 4), ALIGN),
    ("GRU with gru_channels 12", dict(GRU, gru_channels=12), NULL),
    ("GRU with d_nhwc", dict(GRU, d_nhwc=A, nhwc_pixel_stride=128), MODE),
    ("GRU with block_n 64", dict(GRU, block_n=64), SHAPE),
    ("GRU with a 3x3 kernel", dict(GRU, kh=3, kw=3), SHAPE),
    ("GRU addend misaligned", dict(GRU, d_addend=A + 4, addend_pixel_stride=128), ALIGN),
    ("GRU addend row shorter than N", dict(GRU, d_addend=A, addend_pixel_stride=64), ALIGN),
    ("OFLOW_IN_F32_NORM without d_in_scale", dict(in_format=1, in_groups=4, x_pixel_stride=512, d_in_shift=A), NULL),
    ("OFLOW_IN_F32_NORM with a 1x1 kernel",
     dict(in_format=1, in_groups=4, x_pixel_stride=512, d_in_scale=A, d_in_shift=A, kh=1, kw=1), MODE),
    ("OFLOW_IN_F32_NORM with 8 groups", dict(in_format=1, d_in_scale=A, d_in_shift=A), MODE),
    ("OFLOW_IN_F32_NORM rows not dense", dict(in_format=1, in_groups=4, x_pixel_stride=1024, d_in_scale=A, d_in_shift=A), SHAPE),
    ("OFLOW_IN_F32 with a 3x3 kernel", dict(in_format=2, x_pixel_stride=1008), MODE),
    ("OFLOW_IN_F32 rows of too few channels", dict(in_format=2, x_pixel_stride=512, kh=1, kw=1), SHAPE),
    ("OFLOW_IN_IMG7S2 with a 3x3 kernel", dict(in_format=3, in_groups=5, block_n=64), MODE),
    ("OFLOW_IN_IMG7S2 with d_addend",
     dict(in_format=3, in_groups=5, block_n=64, kh=1, kw=1, d_addend=A, addend_pixel_stride=128), MODE),
    ("OFLOW_IN_FLOW7 with 5 groups", dict(in_format=4, in_groups=5, kh=1, kw=1), MODE),
    ("OFLOW_IN_FLOW7 with d_addend", dict(in_format=4, in_groups=4, kh=1, kw=1, d_addend=A, addend_pixel_stride=128), SHAPE),
    ("flow head without d_fh_partial", dict(FH, d_fh_partial=None), NULL),
    ("flow head with N 128", dict(FH, N=128), SHAPE),
    ("flow head with a 1x5 kernel", dict(FH, kh=1, kw=5), SHAPE),
    ("flow head with block_n 32", dict(FH, block_n=32), SHAPE),
    ("flow head with activation 0", dict(FH, activation=0), MODE),
    ("flow head with out_scale 2", dict(FH, out_scale=2.0), MODE),
    ("flow head with OFLOW_IN_F32", dict(FH, in_format=2), MODE),
    ("flow head with d_f32", dict(FH, d_f32=A), MODE),
    ("flow head with s2d", dict(FH, s2d=1), MODE),
    ("flow head with d_addend", dict(FH, d_addend=A, addend_pixel_stride=256), MODE),
    ("flow head with x_pixel_stride 16 mod 128", dict(FH, x_pixel_stride=1040), ALIGN),
    ("flow head with misaligned d_fh_partial", dict(FH, d_fh_partial=A + 2), ALIGN),
    ("flow head with d_x NULL", dict(FH, d_x=None), NULL),
    ("flow head with H 0", dict(FH, H=0), SHAPE),
    ("flow head with misaligned d_wpack", dict(FH, d_wpack=A + 8), ALIGN),
    ("flow head with misaligned d_wfrag", dict(FH, d_wfrag=A + 8), ALIGN),
    ("flow head with block_n 128 without d_wfrag", dict(FH, block_n=128), MODE),
    # several errors at once: the first check in the entry point's order decides
    ("d_x NULL and activation 4", dict(d_x=None, activation=4), NULL),
    ("B 0 and no destination", dict(B=0, d_f32=None), SHAPE),
    ("activation 4 and misaligned d_x", dict(activation=4, d_x=A + 8), MODE),
    ("misaligned d_x and no destination", dict(d_x=A + 8, d_f32=None), ALIGN),
    ("no destination and in_format 5", dict(d_f32=None, in_format=5), NULL),
    ("weights of 2 GiB and misaligned d_wfrag", dict(in_groups=14564, d_wfrag=A + 8), SHAPE),
    ("misaligned d_wfrag and in_format 5", dict(d_wfrag=A + 8, in_format=5), ALIGN),
    ("in_format 5 and d_addend with epilogue 0", dict(in_format=5, d_addend=A, addend_pixel_stride=128), MODE),
    ("epilogue 4 with the flow-head pointers", dict(FH, epilogue=4), MODE),
    ("GRU without pointers and misaligned d_x", dict(kh=1, kw=5, epilogue=1, d_x=A + 8), ALIGN),
    ("GRU with N != 2 * gru_channels and d_stats", dict(GRU, gru_channels=128, d_stats=A), SHAPE),
    ("flow head without d_fh_weights and fh_slabs 3", dict(FH, d_fh_weights=None, fh_slabs=3), NULL),
    ("flow head with fh_slabs 3 and d_y0", dict(FH, fh_slabs=3, d_y0=A, y0_pixel_stride=1024), SHAPE),
    ("flow head with d_y0 and x_pixel_stride 16 mod 128", dict(FH, d_y0=A, y0_pixel_stride=1024, x_pixel_stride=1040), MODE),
    ("flow head with misaligned d_fh_weights and d_x NULL", dict(FH, d_fh_weights=A + 2, d_x=None), ALIGN),
    ("flow head with d_wscale NULL and misaligned d_wfrag", dict(FH, d_wscale=None, d_wfrag=A + 8), NULL),
]


def _conv_status(fields):
    desc = Desc(struct_size=ctypes.sizeof(Desc), **fields)
    return _native.load().oflow_conv_s32(ctypes.byref(desc), None)


def test_conv_desc_struct_size_is_checked_first():
    lib = _native.load()
    assert lib.oflow_conv_s32(None, None) == NULL
    for size in (0, ctypes.sizeof(Desc) - 4, ctypes.sizeof(Desc) + 8):
        assert lib.oflow_conv_s32(ctypes.byref(Desc(struct_size=size, **BASE)), None) == MODE  # (BASE alone is valid)
        assert lib.oflow_conv_s32(ctypes.byref(Desc(struct_size=size)), None) == MODE
    assert _conv_status({}) == NULL  # zero-filled with the right size: the first required pointer is missing


@pytest.mark.parametrize("name,mutation,expected", STATUS_CASES, ids=[c[0] for c in STATUS_CASES])
def test_conv_desc_status_table(name, mutation, expected):
    assert _conv_status(dict(BASE, **mutation)) == expected
