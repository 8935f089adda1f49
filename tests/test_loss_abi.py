"""CPU tests of the image loss's boundary: rm_image_loss rejects a NULL context, rm_image_loss_default fills the
documented values, the header's flag is the binding's, and render.image_loss / render.image_metrics check their
images before anything reaches a device. No kernels run here."""
import ctypes
import os
import re

import numpy as np
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
    assert lib.rm_image_loss(None, None, None, 1, 16, 16, 1.0, None, None, None, None, None) == 1  # RM_ERR_INVALID_ARG


def test_defaults(native):
    p = native.RmImageLossParams(-1.0, -1.0, -1.0, -1.0, -1.0, -1)
    native.lib().rm_image_loss_default(ctypes.byref(p))
    assert (p.l1_weight, p.ssim_weight, p.progress, p.c1, p.c2, p.flags) == (
        np.float32(0.8), np.float32(0.2), 0.0, np.float32(1e-4), np.float32(9e-4), 0)
    native.lib().rm_image_loss_default(None)  # a NULL struct is ignored
    q = native.image_loss_params(ssim_weight=0.5, flags=native.RM_LOSS_PLAIN_L1)
    assert (q.l1_weight, q.ssim_weight, q.flags) == (np.float32(0.8), 0.5, 1)
    with pytest.raises(TypeError):
        native.image_loss_params(lambda_=0.2)


def test_flag_matches_the_header(native):
    (value,) = re.findall(r"#define\s+RM_LOSS_PLAIN_L1\s+(\d+)", open(HEADER).read())
    assert native.RM_LOSS_PLAIN_L1 == int(value) == 1


@pytest.mark.parametrize("fn", ["image_loss", "image_metrics"])
def test_images_are_checked_on_the_host(fn):
    """Host (CPU) tensors: a device error could only come after these checks, and the last one shows that
    well-formed host images are refused too (there is no CPU implementation)."""
    from burn_raymarching_amd import render
    call = getattr(render, fn)
    z = torch.zeros
    with pytest.raises(ValueError, match="V\\*H\\*W"):
        call(z(2 * 4 * 5 + 1, 3), z(2 * 4 * 5 + 1, 3), 5, 4)               # not a multiple of H * W
    with pytest.raises(ValueError, match="pixels"):
        call(z(2 * 4 * 5, 3), z(4 * 5, 3), 5, 4)                             # out and target differ
    with pytest.raises(ValueError, match=r"expected \[V, 4, 5, 3\]"):
        call(z(2, 5, 4, 3), z(2, 5, 4, 3), 5, 4)                             # [V, W, H, 3]
    with pytest.raises(TypeError, match="float32"):
        call(z(20, 3, dtype=torch.float64), z(20, 3), 5, 4)
    with pytest.raises(TypeError, match="float32"):
        call(z(20, 3), z(20, 3, dtype=torch.float16), 5, 4)
    with pytest.raises(ValueError, match="3 channels"):
        call(z(20, 4), z(20, 4), 5, 4)
    with pytest.raises(ValueError, match="3 channels"):
        call(z(1, 4, 5, 1), z(1, 4, 5, 1), 5, 4)
    with pytest.raises(ValueError, match="is on cpu and target on meta"):
        call(z(20, 3), z(20, 3, device="meta"), 5, 4)                        # mismatched devices
    with pytest.raises(TypeError, match="torch tensor"):
        call(np.zeros((20, 3), np.float32), z(20, 3), 5, 4)
    with pytest.raises(ValueError, match="no CPU implementation"):
        call(z(20, 3), z(20, 3), 5, 4)
