"""Storage layouts and accepted shapes for the tests of the torch autograd layer (render.render_diff,
render_diff_cameras, render_diff_sh, sdf_field, image_loss): TEST INFRASTRUCTURE ONLY (plain helpers, imported by
tests/test_autograd_layouts.py and tests/test_gpu_autograd_contract.py).

Every layout of a float32 tensor x holds x's values, bit for bit, in a storage an optimisation loop written in
torch hands a Function: a slice of a wider buffer, a transposed view, every second row, a view that starts one
element into its allocation, a slice of one packed parameter vector, rows that are one row expanded. The helpers
work on the device of x; nothing here needs a GPU."""
import torch

# what each layout claims (tests/test_autograd_layouts.py holds every entry to its claim)
CLAIMS = {"plain": "contiguous", "col_slice": "noncontiguous", "transposed": "noncontiguous",
          "row_stride": "noncontiguous", "offset1": "misaligned", "packed": "offset", "expanded": "zero_stride"}


def plain(x):
    return x.detach().clone(memory_format=torch.contiguous_format)


def col_slice(x):
    """Columns 1:1+C of a wider [..., C+4] buffer (a 1-D tensor: column 1 of [R, 5]). Tensors of more than
    one row only (a single row's slice is contiguous all the same)."""
    if x.dim() == 0 or x.shape[0] < 2:
        return None
    if x.dim() == 1:
        buf = x.new_full((x.shape[0], 5), float("nan"))
        buf[:, 1] = x
        return buf[:, 1]
    buf = x.new_full(tuple(x.shape[:-1]) + (x.shape[-1] + 4,), float("nan"))
    buf[..., 1:1 + x.shape[-1]] = x
    return buf[..., 1:1 + x.shape[-1]]


def transposed(x):
    """The storage of x.t() viewed back: strides (1, R). 2-D tensors with more than one row and column only
    (with one row or one column the view is contiguous all the same)."""
    if x.dim() != 2 or x.shape[0] < 2 or x.shape[1] < 2:
        return None
    return x.detach().t().contiguous().t()


def row_stride(x):
    """big[::2] of a buffer with twice the rows."""
    if x.dim() == 0 or x.shape[0] < 2:
        return None
    big = x.new_full((2 * x.shape[0],) + tuple(x.shape[1:]), float("nan"))
    big[::2] = x
    return big[::2]


def offset1(x):
    """A contiguous view that starts one element into its allocation: 4-byte aligned, not 8-byte aligned."""
    buf = x.new_full((x.numel() + 1,), float("nan"))
    buf[1:] = x.detach().reshape(-1)
    return buf[1:].view(x.shape)


def expanded(x):
    """Stride-0 rows, where the values allow it: every row equal to the first (a scene whose spheres share one
    colour; a grad_out of ones, as .sum() hands back)."""
    if x.dim() == 0 or x.shape[0] < 2 or not bool((x == x[:1]).all()):
        return None
    return x.detach()[:1].clone().expand(x.shape)


def layouts(x):
    """(name, tensor) for every single-tensor layout x admits; `packed` takes a call's tensors together."""
    for name, make in (("plain", plain), ("col_slice", col_slice), ("transposed", transposed),
                       ("row_stride", row_stride), ("offset1", offset1), ("expanded", expanded)):
        t = make(x)
        if t is not None:
            yield name, t


def packed(tensors, lead=1):
    """A call's tensors (a dict, in model.pack's order: centers, colors, radius, light_dir, ambient) back to back
    in one flat vector, after `lead` words that stand for whatever a larger parameter buffer holds before them:
    (flat, {name: view}). Every view is contiguous and starts inside the vector."""
    total = lead + sum(t.numel() for t in tensors.values())
    like = next(iter(tensors.values()))
    flat = like.new_full((total,), float("nan"))
    views, at = {}, lead
    for k, t in tensors.items():
        v = flat[at:at + t.numel()].view(t.shape)
        v.copy_(t.detach())
        views[k] = v
        at += t.numel()
    return flat, views


def claim_holds(name, t):
    """The property the layout's name claims."""
    what = CLAIMS[name]
    if what == "contiguous":
        return t.is_contiguous() and t.storage_offset() == 0
    if what == "noncontiguous":
        return not t.is_contiguous()
    if what == "misaligned":
        return t.is_contiguous() and t.storage_offset() == 1 and t.data_ptr() % 8 == 4
    if what == "offset":
        return t.is_contiguous() and t.storage_offset() > 0
    if what == "zero_stride":
        return 0 in t.stride()
    raise KeyError(what)


def shapes(name, x):
    """(label, tensor) for every shape the layer accepts for the argument `name` (x in its canonical shape:
    radius [M], light_dir [3], ambient [1]); contiguous clones."""
    alt = {"radius": lambda: x.reshape(-1, 1), "light_dir": lambda: x.reshape(1, 3), "ambient": lambda: x.reshape(())}
    yield "canonical", plain(x)
    if name in alt:
        yield {"radius": "M_by_1", "light_dir": "1_by_3", "ambient": "0d"}[name], plain(alt[name]())


def wrong_shapes(name, x):
    """Shapes of the right element count that the layer refuses for the argument `name`."""
    bad = {"radius": lambda: x.reshape(1, -1), "light_dir": lambda: x.reshape(3, 1), "ambient": lambda: x.reshape(1, 1),
           "centers": lambda: x.reshape(3, -1) if x.shape[0] != 3 else x.reshape(-1), "colors": lambda: x.reshape(-1)}
    if name in bad:
        yield plain(bad[name]())


def same_bits(a, b):
    """Equal shape and equal words (float32 compared as bytes: -0.0 differs from 0.0, a NaN equals itself)."""
    if tuple(a.shape) != tuple(b.shape) or a.dtype != b.dtype:
        return False
    return a.detach().cpu().contiguous().numpy().tobytes() == b.detach().cpu().contiguous().numpy().tobytes()
