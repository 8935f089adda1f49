"""CPU tests of the ray / camera-pose gradient entry points at the C-ABI boundary: the header
declares them, the built library exports them, the Python binding has them, and both reject a
NULL context without launching anything. No kernel runs here."""
import ctypes
import inspect
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "raymarch.h")
NAMES = ("rm_render_diff_backward_rays", "rm_render_diff_backward_cameras")


@pytest.fixture(scope="module")
def native():
    from burn_raymarching_amd import _build, native as nat
    _build.build_lib()
    return nat


def test_header_declares_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name


def test_library_exports_and_binding_has_them(native):
    lib = ctypes.CDLL(native.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in native.SIGNATURES, name
    # eleven arguments each, as declared
    assert len(native.SIGNATURES[NAMES[0]][1]) == 11
    assert len(native.SIGNATURES[NAMES[1]][1]) == 11


def test_null_context_is_rejected(native):
    lib = native.lib()
    assert lib.rm_render_diff_backward_rays(None, None, None, 0, None, None, None, None, None, None, 0) == 1
    assert lib.rm_render_diff_backward_cameras(None, None, 1, 8, 8, None, None, None, None, None, 0) == 1


def test_kernel_header_is_a_hashed_source():
    """The ray-gradient kernel lives in its own header, and the library's source hash covers it."""
    from burn_raymarching_amd import _build
    names = [os.path.basename(p) for p in _build.KERNEL_SOURCES]
    assert "rm_raygrad.h" in names
    src = open(os.path.join(ROOT, "burn_raymarching_amd", "csrc", "rm_kernels.hip")).read()
    assert '#include "rm_raygrad.h"' in src


def test_torch_interface_is_present():
    from burn_raymarching_amd import render
    for fn in ("render_diff_backward_rays", "render_diff_backward_cameras", "render_diff_cameras"):
        assert callable(getattr(render, fn)), fn
        assert "not the derivative of the image" in " ".join(inspect.getdoc(getattr(render, fn)).split()), fn
