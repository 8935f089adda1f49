"""CPU tests of tests/autograd_layouts.py and of the two torch behaviours tests/test_gpu_autograd_contract.py
relies on.

The GPU file passes every tensor argument of the autograd layer in each layout and compares bits with the
contiguous run. That proves something only while every layout really is what its name says: here each one is
held to x's values, bit for bit, and to the property it claims (non-contiguous, a storage offset, a data pointer
that is 4-byte but not 8-byte aligned, a zero stride), so the GPU file cannot degrade to contiguous inputs
without this file failing.

The toy Function pins torch itself: a tensor saved through save_for_backward carries the version of the tensor
it is a detached alias of (an attribute of ctx does not), and a once-differentiable backward raises when its
result is differentiated again."""
import numpy as np
import pytest
import torch

import autograd_layouts as L


def inputs():
    rng = np.random.default_rng(4)
    t = lambda *s: torch.from_numpy(rng.normal(size=s).astype(np.float32))  # noqa: E731
    flat_colour = torch.from_numpy(rng.uniform(0.1, 0.9, (1, 3)).astype(np.float32)).repeat(6, 1)
    return {"rays [577,3]": t(577, 3), "centers [6,3]": t(6, 3), "one sphere [1,3]": t(1, 3), "sh [33,8,3]": t(33, 8, 3),
            "radius [6]": t(6), "radius [6,1]": t(6, 1), "light_dir [3]": t(3), "light_dir [1,3]": t(1, 3),
            "ambient [1]": t(1), "ambient 0-d": t(), "images [2,24,40,3]": t(2, 24, 40, 3),
            "one colour [6,3]": flat_colour, "ones [577,3]": torch.ones(577, 3)}


@pytest.mark.parametrize("what", list(inputs()))
def test_every_layout_has_the_values_and_the_property_it_claims(what):
    x = inputs()[what]
    ref = L.plain(x)
    assert L.same_bits(ref, x) and ref.data_ptr() != x.data_ptr()
    names = []
    for name, t in L.layouts(x):
        names.append(name)
        assert t.dtype == torch.float32 and tuple(t.shape) == tuple(x.shape), (what, name)
        assert L.same_bits(t, ref), (what, name, "values")
        assert L.claim_holds(name, t), (what, name, L.CLAIMS[name], t.stride(), t.storage_offset(), t.data_ptr() % 8)
    assert names[0] == "plain" and "offset1" in names
    if x.dim() >= 1 and x.shape[0] >= 2:
        assert {"col_slice", "row_stride"} <= set(names), (what, names)
    if x.dim() == 2 and min(x.shape) >= 2:
        assert "transposed" in names and dict(L.layouts(x))["transposed"].stride() == (1, x.shape[0])
    assert ("expanded" in names) == (what in ("one colour [6,3]", "ones [577,3]")), (what, names)


def test_layouts_are_what_a_kernel_would_misread():
    """A reader that ignored the strides (took numel() words from data_ptr) would see other values: the
    non-contiguous layouts are not accidentally dense."""
    x = inputs()["centers [6,3]"]
    for name, t in L.layouts(x):
        if L.CLAIMS[name] != "noncontiguous":
            continue
        dense = torch.as_strided(t, (t.numel(),), (1,), t.storage_offset())
        assert not L.same_bits(dense.reshape(x.shape), x), name


def test_packed_views_share_one_vector_in_model_order():
    x = inputs()
    scene = {"centers": x["centers [6,3]"], "colors": x["one colour [6,3]"], "radius": x["radius [6]"],
             "light_dir": x["light_dir [3]"], "ambient": x["ambient [1]"]}
    flat, views = L.packed(scene)
    assert flat.numel() == 1 + 7 * 6 + 4
    at = 1
    for k, v in views.items():
        assert L.same_bits(v, scene[k]) and L.claim_holds("packed", v), k
        assert v.storage_offset() == at and v.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr(), k
        at += v.numel()
    from burn_raymarching_amd import model
    want = model.pack(*(scene[k].numpy() for k in ("centers", "colors", "radius", "light_dir", "ambient")))
    assert flat[1:].numpy().tobytes() == want.tobytes()  # the order of model.pack
    flat[1] = 5.0  # a view, not a copy
    assert views["centers"][0, 0] == 5.0


def test_accepted_and_refused_shapes():
    x = inputs()
    got = {name: [(label, tuple(t.shape)) for label, t in L.shapes(name, x[key])]
           for name, key in (("radius", "radius [6]"), ("ambient", "ambient [1]"), ("light_dir", "light_dir [3]"),
                             ("centers", "centers [6,3]"))}
    assert got == {"radius": [("canonical", (6,)), ("M_by_1", (6, 1))], "ambient": [("canonical", (1,)), ("0d", ())],
                   "light_dir": [("canonical", (3,)), ("1_by_3", (1, 3))], "centers": [("canonical", (6, 3))]}
    for name, key in (("radius", "radius [6]"), ("ambient", "ambient [1]"), ("light_dir", "light_dir [3]")):
        ok = {tuple(t.shape) for _, t in L.shapes(name, x[key])}
        for label, t in L.shapes(name, x[key]):
            assert t.is_contiguous() and L.same_bits(t.reshape(-1), x[key].reshape(-1)), (name, label)
        bad = list(L.wrong_shapes(name, x[key]))
        assert bad and all(tuple(t.shape) not in ok and t.numel() == x[key].numel() for t in bad), name


# ---- torch's own behaviour, on a toy Function ----------------------------------------------------

class _Square(torch.autograd.Function):
    """y = x^2 computed from a detached, contiguous alias of x, the way the render Functions hold their scene:
    kept through save_for_backward (saved=True) or as an attribute of ctx (saved=False)."""

    @staticmethod
    def forward(ctx, x, saved):
        held = x.detach().contiguous().reshape(-1)  # an alias where x is contiguous, a copy where it is not
        if saved:
            ctx.save_for_backward(held)
        else:
            ctx.held = held
        ctx.shape = x.shape
        return (held * held).reshape(x.shape)

    @staticmethod
    def backward(ctx, g):
        held = ctx.saved_tensors[0] if ctx.saved_tensors else ctx.held
        return 2.0 * held.reshape(ctx.shape) * g, None


class _SquareOnce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x.detach())
        return x.detach() * x.detach()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return torch.from_numpy(2.0 * x.numpy() * g.numpy())  # a result autograd did not see made, as a kernel's is


class _SquareBlind(_SquareOnce):
    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return torch.from_numpy(2.0 * x.detach().numpy() * g.detach().numpy())


def test_saved_tensor_version_check_fires_through_a_detached_alias():
    x = torch.tensor([[1.0, 2.0, 3.0]], requires_grad=True)
    y = _Square.apply(x, True)
    with torch.no_grad():
        x.add_(1.0)  # what optimizer.step() or p.clamp_() does
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.sum().backward()
    # the same alias kept as an attribute: no error, and the gradient of values the forward never saw
    x = torch.tensor([[1.0, 2.0, 3.0]], requires_grad=True)
    y = _Square.apply(x, False)
    with torch.no_grad():
        x.add_(1.0)
    y.sum().backward()
    assert torch.equal(x.grad, torch.tensor([[4.0, 6.0, 8.0]]))
    # a non-contiguous input was copied: the saved copy has the forward's values and no version to check
    base = torch.tensor([[1.0, 9.0], [2.0, 9.0], [3.0, 9.0]])
    x = base[:, 0].detach().requires_grad_()
    assert not x.is_contiguous()
    y = _Square.apply(x, True)
    with torch.no_grad():
        x.add_(1.0)
    y.sum().backward()
    assert torch.equal(x.grad, torch.tensor([2.0, 4.0, 6.0]))


def test_once_differentiable_backward_raises_when_differentiated_again():
    """The incoming gradient must itself carry a graph for torch to arm the error (a loss that is not linear in
    the Function's output: the GPU file's double-backward loss is quadratic for that reason)."""
    x = torch.tensor([1.0, 2.0, 3.0], requires_grad=True)
    y = _SquareOnce.apply(x)
    (g,) = torch.autograd.grad((y * y).sum(), x, create_graph=True)
    assert g.requires_grad
    with pytest.raises(RuntimeError, match="once_differentiable"):
        (g.sum() + x.sum()).backward()
    # without the decorator the same backward hands back a gradient with no graph: the sum's backward succeeds
    # and the second-order term is silently missing
    x = torch.tensor([1.0, 2.0, 3.0], requires_grad=True)
    y = _SquareBlind.apply(x)
    (g,) = torch.autograd.grad((y * y).sum(), x, create_graph=True)
    assert not g.requires_grad
    (g.sum() + x.sum()).backward()
    assert torch.equal(x.grad, torch.ones(3))
