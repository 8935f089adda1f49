"""CPU tests of the view-dependent colour's boundary: the four rm_render_diff_sh entry points reject a NULL
context, the header's degree limit is the binding's, and render.render_diff_sh checks its coefficient
tensor and its rays before anything reaches a device. No kernels run here."""
import os
import re

import pytest
import torch

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "raymarch.h")


@pytest.fixture(scope="module")
def native():
    from burn_raymarching_amd import _build, native as nat
    _build.build_lib()
    return nat


def test_null_context_is_rejected(native):
    lib = native.lib()
    assert lib.rm_render_diff_sh(None, None, None, 0, None, None, 1, None, None, None) == 1  # RM_ERR_INVALID_ARG
    assert lib.rm_render_diff_sh_camera(None, None, 1, 16, 16, None, None, 1, None, None, None) == 1
    assert lib.rm_render_diff_sh_backward(None, None, None, 0, None, None, 1, None, None, None, None, None, 0) == 1
    assert lib.rm_render_diff_sh_backward_camera(None, None, 1, 16, 16, None, None, 1, None, None, None, None, None, 0) == 1


def test_degree_limit_matches_the_header(native):
    text = open(HEADER).read()
    (value,) = re.findall(r"#define\s+RM_SH_MAX_DEGREE\s+(\d+)", text)
    assert native.RM_SH_MAX_DEGREE == int(value) == 2
    from burn_raymarching_amd import render
    assert render.SH_BANDS == {(d + 1) ** 2 - 1: d for d in range(native.RM_SH_MAX_DEGREE + 1)}


@pytest.mark.parametrize("bands", [1, 2, 4, 9, 15])
def test_render_diff_sh_rejects_other_band_counts(bands):
    from burn_raymarching_amd import render
    m, n = 3, 4
    z = torch.zeros
    with pytest.raises(ValueError, match="B = 0, 3"):
        render.render_diff_sh(z(n, 3), z(n, 3), z(m, 3), z(m, 3), z(m, bands, 3), z(m), z(3), z(1), 32.0)
    with pytest.raises(ValueError, match="B = 0, 3"):
        render.render_diff_sh(z(n, 3), z(n, 3), z(m, 3), z(m, 3), z(m, 3), z(m), z(3), z(1), 32.0)  # not [M, B, 3]


def test_render_diff_sh_refuses_ray_gradients():
    """Rays that require grad raise before any launch: ray gradients are not available with SH."""
    from burn_raymarching_amd import render
    m, n = 3, 4
    z = torch.zeros
    for which in (0, 1):
        rays = [z(n, 3), z(n, 3)]
        rays[which].requires_grad_(True)
        with pytest.raises(ValueError, match="ray gradients are not available with SH"):
            render.render_diff_sh(rays[0], rays[1], z(m, 3), z(m, 3), z(m, 3, 3), z(m), z(3), z(1), 32.0)
