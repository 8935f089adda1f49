"""The gradient reductions pinned to the fp64 sum of their block partials (DESIGN.md 5.2,
"Additivity"; the measure: tests/additivity_ref.py).

A call on one row's rays alone returns that row's partial record bit for bit, so a full call's
gradient G has its terms G_row on hand and must satisfy, elementwise and with no chosen tolerance,

    |G - sum_rows G_row (fp64)| <= gamma_(n-1) sum_rows |G_row|      (n non-zero rows)

A row is 256 consecutive rays (general kernel unsplit, small kernel at one lane per ray), 128 rays
(small kernel, two lanes per ray), 32 rays (split march) or one 16x16 tile of one view (tiled
camera mode). Where rows cannot be called alone as fixed ray sets (split continuations, frames of
several tiles) the calls that stand in for them carry sums of their own: A = sum_rays |g_ray| from
the fp64 oracle, bound 2 gamma_(n-1) A.

Before every full call and before every batch of one-row calls the context's workspace is
poisoned: a backward call with the same spheres and switches, the same number of rows, all live,
grad_out scaled by 2^40 -- a row or column read without having been written by the call under test
lands twelve orders of magnitude above the bound. Outputs start as NaN and must end finite.

light_dir goes through light_grad's projection and is additive only for the axis-aligned lights of
length 2 (the orthogonal components are r / 2 exactly, the parallel one exactly 0); the other cases
keep the synthetic scene's light and leave light_dir out.

Also here, all bit-exact: accumulate on a non-zero prior gradient (and the sub-launch chain),
NULL members of rm_grads with guard words around every buffer, and the per-view pose gradients of
rm_render_diff_backward_cameras against one-view calls.
"""
import ctypes
import time

import numpy as np
import pytest

import additivity_ref as A
from conftest import gpu_available, record_margin

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

SWITCHES = ("RM_SMALL", "RM_SPLIT", "RM_REDUCE_FUSED", "RM_MAX_BLOCKS_PER_LAUNCH", "RM_SMALL_LPR",
            "RM_SPLIT_CONT_LIST")
K = 32.0
POISON = 2.0 ** 40
GUARD = 12345.0
PROGRESS = 0.4


@pytest.fixture(scope="module")
def rm():
    import torch
    from burn_raymarching_amd import _build
    _build.build_lib()
    from burn_raymarching_amd import model, native, render
    torch.cuda.init()
    return render, model, native


def switches(monkeypatch, **kw):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, v in kw.items():
        monkeypatch.setenv(name, str(v))


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()


class Pool:
    """Rays of ring views that look at the scene (their line passes within 0.6 of the origin; the
    synthetic scenes fill the ball of radius 0.6), shuffled."""

    def __init__(self, oracle, model):
        import torch
        o, d = [], []
        for c in model.ring_cameras(12, fov=40.0):
            oo, dd = oracle.camera_rays(192, 192, *c, precision="f32")
            o.append(oo)
            d.append(dd)
        o, d = np.concatenate(o), np.concatenate(d)
        miss = np.linalg.norm(np.cross(o.astype(np.float64), d.astype(np.float64)), axis=1)
        keep = np.flatnonzero(miss < 0.6)
        keep = keep[np.random.default_rng(5).permutation(keep.size)]
        self.o_np, self.d_np = o[keep], d[keep]
        self.n = keep.size
        self.o, self.d = dev(self.o_np), dev(self.d_np)
        self.torch = torch

    def index(self, n, start=0):
        return (self.torch.arange(n, device="cuda") + start) % self.n

    def take(self, n, start=0):
        idx = self.index(n, start)
        return self.o[idx].contiguous(), self.d[idx].contiguous()


@pytest.fixture(scope="module")
def pool(rm, oracle):
    p = Pool(oracle, rm[1])
    assert p.n >= 100000
    return p


def randn(n, seed, cols=3):
    import torch
    return torch.randn((n, cols), device="cuda", generator=torch.Generator("cuda").manual_seed(seed))


class Caller:
    """The C ABI's backward / train calls of one scene on the context of torch's current stream,
    writing into slices of the caller's buffers."""

    def __init__(self, rm, sc, steps, poison_rpr=256):
        render, model, native = rm
        self.native = native
        self.sc = sc
        self.scene = model.scene_tensors(sc)
        self.m = sc["centers"].shape[0]
        self.E = 7 * self.m + 5
        self.steps = steps
        self.ctx = render.context()
        self.lib = self.ctx._lib
        self.march = self.scene.march_for(native.march_params(steps, K))
        self.cs = self.scene.c_struct()
        self.poison_rpr = poison_rpr
        self._poison = {}
        m = self.m
        self.packed = {"centers": 0, "colors": 3 * m, "radius": 6 * m, "light_dir": 7 * m, "ambient": 7 * m + 3,
                       "loss": 7 * m + 4}

    def new(self, rows=None, fill=float("nan")):
        import torch
        return torch.full((self.E,) if rows is None else (rows, self.E), fill, device="cuda")

    def grads(self, buf, null=(), offs=None):
        offs = self.packed if offs is None else offs
        base = buf.data_ptr()
        cg = self.native.RmGrads(*(None if k in null else base + 4 * offs[k] for k in A.KEYS))
        return cg, ctypes.c_void_p(base + 4 * offs["loss"])

    def bwd(self, o, d, g, buf, acc=0, null=(), offs=None):
        cg, _ = self.grads(buf, null, offs)
        self.ctx.check(self.lib.rm_render_diff_backward(self.ctx.handle, P(o), P(d), o.shape[0], ctypes.byref(self.cs),
                                                        ctypes.byref(self.march), P(g), None, ctypes.byref(cg), acc),
                       "rm_render_diff_backward")

    def train(self, o, d, tg, inv, buf, acc=0, null=(), offs=None, out=None):
        cg, lp = self.grads(buf, null, offs)
        self.ctx.check(self.lib.rm_train_step(self.ctx.handle, P(o), P(d), P(tg), o.shape[0], PROGRESS, inv,
                                              ctypes.byref(self.cs), ctypes.byref(self.march), ctypes.byref(cg), lp,
                                              P(out), acc), "rm_train_step")

    def bwd_cam(self, cams, w, h, g, buf, acc=0, null=(), offs=None):
        cg, _ = self.grads(buf, null, offs)
        self.ctx.check(self.lib.rm_render_diff_backward_camera(self.ctx.handle, self.native.cameras(cams), len(cams), w,
                                                               h, ctypes.byref(self.cs), ctypes.byref(self.march),
                                                               P(g), None, ctypes.byref(cg), acc),
                       "rm_render_diff_backward_camera")

    def train_cam(self, cams, w, h, tg, inv, buf, acc=0, null=(), offs=None, out=None):
        cg, lp = self.grads(buf, null, offs)
        self.ctx.check(self.lib.rm_train_step_camera(self.ctx.handle, self.native.cameras(cams), len(cams), w, h,
                                                     P(tg), PROGRESS, inv, ctypes.byref(self.cs),
                                                     ctypes.byref(self.march), ctypes.byref(cg), lp, P(out), acc),
                       "rm_train_step_camera")

    def poison(self, pool, nrows):
        """The poison pass: a backward call of nrows live rows (of poison_rpr rays, the row size of
        an array-mode backward call under the current switches), grad_out scaled by 2^40."""
        n = nrows * self.poison_rpr
        if n not in self._poison:
            o, d = pool.take(n, start=7919)
            self._poison[n] = (o, d, randn(n, 99) * POISON, self.new())
        o, d, g, sink = self._poison[n]
        self.bwd(o, d, g, sink)


def scene(rm, m, seed, light_axis=None):
    sc = rm[1].synthetic_scene(m, seed)
    if light_axis is not None:
        sc["light_dir"] = A.axis_light(light_axis)
    return sc


def selection(m, mode, light_axis):
    ix = A.index_sets(m)
    sel = np.zeros(7 * m + 5, bool)
    for k in ("centers", "colors", "radius", "ambient"):
        sel[ix[k]] = True
    if mode == "train":
        sel[ix["loss"]] = True
    if light_axis is not None:
        for c in range(3):
            sel[7 * m + c] = c != light_axis
    return sel


def judge(path, tag, m, mode, light_axis, G, rows, A_sum=None, factor=1.0, n=None):
    """Assert the measure on the checked elements and record the worst error-to-bound ratio."""
    sel = selection(m, mode, light_axis)
    written = slice(0, 7 * m + (5 if mode == "train" else 4))  # every output of the call, checked or not
    assert np.isfinite(G[written]).all() and np.isfinite(rows[:, written]).all(), (tag, "not finite after the poison call")
    if light_axis is not None:  # the component along the light is exactly zero
        assert G[7 * m + light_axis] == 0.0 and (rows[:, 7 * m + light_axis] == 0.0).all(), (tag, "light_dir parallel")
    ok, ratio, n = A.measure(G[sel], rows[:, sel], None if A_sum is None else A_sum[sel], n, factor)
    print(f"additivity {path} {tag}: n = {n}, worst err / bound = {ratio:.4g}")
    record_margin("additivity_" + path, ratio if np.isfinite(ratio) else 1e30, 1.0)
    assert ok, (path, tag, n, ratio)
    return n


def run_rows(c, pool, call, n, rpr, only_rows=None, min_poison_rows=0):
    """The full call on rays [0, n) and the one-row calls, each batch after a poison pass.
    call(lo, hi, buf) runs the call under test on rays [lo, hi) into buf."""
    import torch
    nrows = (n + rpr - 1) // rpr
    # at least the rows of the call under test
    prows = max(nrows, (n + c.poison_rpr - 1) // c.poison_rpr, min_poison_rows)
    full = c.new()
    c.poison(pool, prows)
    call(0, n, full)
    which = list(range(nrows)) if only_rows is None else list(only_rows)
    rows = c.new(len(which))
    c.poison(pool, prows)
    for i, r in enumerate(which):
        call(r * rpr, min(n, (r + 1) * rpr), rows[i])
    torch.cuda.synchronize()
    return full.cpu().numpy().astype(np.float64), rows.cpu().numpy().astype(np.float64)


def oracle_A(oracle, sc, steps, o, d, g=None, targets=None, inv=None):
    """A = sum_rays |g_ray| from the fp64 oracle, one call per ray (pack()'s layout)."""
    o64, d64 = np.asarray(o, np.float64), np.asarray(d, np.float64)
    m = sc["centers"].shape[0]
    acc = np.zeros(7 * m + 5)
    for i in range(o64.shape[0]):
        s = slice(i, i + 1)
        if g is not None:
            acc += np.abs(A.pack(oracle.render_diff_backward(o64[s], d64[s], sc, steps, K, np.asarray(g[s], np.float64))))
        else:
            _, loss, gr = oracle.train_step(o64[s], d64[s], np.asarray(targets[s], np.float64), sc, steps, K, PROGRESS,
                                            inv_count=inv)
            acc += np.abs(A.pack(gr, loss))
    return acc


def dead_rows(o, d, g, kinds, rpr):
    """Rows of kind 1 lose their seeds (grad_out rows zero), rows of kind 2 point away from the
    scene from the same eye (escaped: exact zeros by the header's contract); kind 0 stays live."""
    import torch
    kind = torch.as_tensor(np.asarray(kinds), device="cuda")[torch.arange(o.shape[0], device="cuda") // rpr]
    d = torch.where((kind == 2)[:, None], -d, d).contiguous()
    g = torch.where((kind == 1)[:, None], torch.zeros_like(g), g).contiguous()
    return d, g


# ---- 1. general kernel, unsplit, array mode, backward ------------------------------------------

@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("blocks", [1, 2, 128, 129, 256, 257, 385])
def test_general_rows(rm, pool, monkeypatch, blocks, fused):
    """Segment layouts of rm_reduce_partials: one row per segment up to 128 rows, seg_len 2 at 129,
    3 at 257 (86 segments used, 42 empty); all rows live, the last one ragged."""
    switches(monkeypatch, RM_SPLIT="0", RM_REDUCE_FUSED=fused)
    c = Caller(rm, scene(rm, 33, 21), 8)
    n = 256 * blocks - 100
    o, d = pool.take(n, start=blocks)
    g = randn(n, blocks)
    G, rows = run_rows(c, pool, lambda lo, hi, buf: c.bwd(o[lo:hi], d[lo:hi], g[lo:hi], buf), n, 256)
    assert judge("general", f"B={blocks} fused={fused}", 33, "bwd", None, G, rows) == blocks


# ---- 2. column-block edges ---------------------------------------------------------------------

@pytest.mark.parametrize("i,m,small_off", [(0, 1, True), (1, 31, True), (2, 32, True), (3, 33, False), (4, 64, False),
                                           (5, 65, False), (6, 300, False), (7, 1100, False)])
def test_general_column_blocks(rm, pool, monkeypatch, i, m, small_off):
    """Five rows and a ragged tail over the column layouts: 8 M' + 8 columns in blocks of 256 (at
    32 spheres the scalars open column block 1; 300 spheres: 11 column blocks; 1100: more than one
    LDS sphere tile), the axis-aligned lights in rotation so light_dir is checked too."""
    kw = {"RM_SMALL": "0"} if small_off else {}
    switches(monkeypatch, RM_SPLIT="0", **kw)
    axis = i % 3
    c = Caller(rm, scene(rm, m, 30 + m, axis), 8)
    n = 5 * 256 + 77
    o, d = pool.take(n, start=100 * i)
    g = randn(n, 40 + i)
    G, rows = run_rows(c, pool, lambda lo, hi, buf: c.bwd(o[lo:hi], d[lo:hi], g[lo:hi], buf), n, 256)
    assert judge("general", f"M={m} light axis {axis}", m, "bwd", axis, G, rows) == 6


# ---- 3. dead rows in the compaction ------------------------------------------------------------

def _patterns(b):
    alt = [r % 2 == 0 for r in range(b)]
    return {"alternating": alt, "first": [r == 0 for r in range(b)], "last": [r == b - 1 for r in range(b)],
            "none": [False] * b}


@pytest.mark.parametrize("dead_kind", [1, 2])
@pytest.mark.parametrize("pattern", ["alternating", "first", "last", "none"])
def test_general_dead_rows(rm, pool, monkeypatch, pattern, dead_kind):
    """40 rows of which some are dead -- no backward seed (kind 1) or escaped (kind 2): their rows
    of the workspace hold the poison call's values and only the live flag keeps them out."""
    switches(monkeypatch, RM_SPLIT="0")
    c = Caller(rm, scene(rm, 33, 22), 8)
    b = 40
    n = 256 * b
    live = _patterns(b)[pattern]
    o, d = pool.take(n, start=3)
    d, g = dead_rows(o, d, randn(n, 7), [0 if x else dead_kind for x in live], 256)
    G, rows = run_rows(c, pool, lambda lo, hi, buf: c.bwd(o[lo:hi], d[lo:hi], g[lo:hi], buf), n, 256)
    ix = A.index_sets(33)
    for r in range(b):  # a dead row alone returns exact zeros, a live one does not
        body = rows[r, :7 * 33 + 4]
        assert (np.all(body == 0.0)) == (not live[r]), (pattern, dead_kind, r)
    nz = judge("general", f"dead rows {pattern} kind {dead_kind}", 33, "bwd", None, G, rows)
    assert nz == sum(live)
    if pattern == "none":
        for k in A.KEYS:
            assert np.all(G[ix[k]] == 0.0), k


def test_general_dead_rows_train_seed_sign_zero(rm, pool, monkeypatch):
    """Train mode: on the chosen rows the targets equal the forward image, so the seed is sign(0) = 0
    (no seed, kind 1); other rows point away with non-zero targets (escaped, a loss but no gradient)."""
    import torch
    switches(monkeypatch, RM_SPLIT="0")
    c = Caller(rm, scene(rm, 33, 23), 8)
    b = 40
    n = 256 * b - 100
    kinds = [(0, 1, 0, 2)[r % 4] for r in range(b)]
    o, d = pool.take(n, start=11)
    d, _ = dead_rows(o, d, randn(n, 1), kinds, 256)
    tg = torch.rand((n, 3), device="cuda", generator=torch.Generator("cuda").manual_seed(8))
    out = torch.empty((n, 3), device="cuda")
    inv = 1.0 / (3.0 * n)
    c.train(o, d, tg, inv, c.new(), out=out)
    kind = torch.as_tensor(kinds, device="cuda")[torch.arange(n, device="cuda") // 256]
    tg = torch.where((kind == 1)[:, None], out, tg).contiguous()
    G, rows = run_rows(c, pool, lambda lo, hi, buf: c.train(o[lo:hi], d[lo:hi], tg[lo:hi], inv, buf), n, 256)
    for r in range(b):
        body = rows[r, :7 * 33 + 4]
        assert np.all(body == 0.0) == (kinds[r] != 0), r
        assert (rows[r, -1] == 0.0) == (kinds[r] == 1), r  # the loss: zero only where out == target
    judge("general", "dead rows train", 33, "train", None, G, rows)


# ---- 4. the full list and the large-launch branch ----------------------------------------------

def _large_live_rows(blocks):
    segs, seg_len = A.seg_layout(blocks)
    used = (blocks + seg_len - 1) // seg_len
    live = set()
    for s in (0, used // 2, used - 1):
        in_seg = min(seg_len, blocks - s * seg_len)
        for p in (0, 63, 64, 65, 127, 128, 191, 192, 255, in_seg - 1):
            if p < in_seg:
                live.add(s * seg_len + p)
    extra = np.random.default_rng(blocks).integers(0, blocks, 12)
    return sorted(live | {int(x) for x in extra})


@pytest.mark.parametrize("blocks,fused", [(32768, "1"), (32769, "1"), (32769, "0")])
def test_large_launch(rm, pool, monkeypatch, blocks, fused):
    """32,768 rows fill pass 1's 256-entry list exactly (seg_len 256); 32,769 take the large-launch
    branch (192 segments of 171 rows, two rounds in pass 2). About 40 live rows at the edges of the
    first, a middle and the last used segment among dead rows of both kinds."""
    import torch
    switches(monkeypatch, RM_SPLIT="0", RM_REDUCE_FUSED=fused)
    assert A.seg_layout(blocks) == ((128, 256) if blocks == 32768 else (192, 171))
    c = Caller(rm, scene(rm, 33, 24), 4)
    n = 256 * blocks - 100
    live = _large_live_rows(blocks)
    kinds = np.where(np.arange(blocks) % 2 == 0, 1, 2)
    kinds[live] = 0
    o, d = pool.take(n, start=17)
    d, g = dead_rows(o, d, randn(n, 3), kinds, 256)
    c.poison(pool, blocks)  # builds the poison call's arrays outside the timed part
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    c.poison(pool, blocks)
    c.bwd(o, d, g, c.new())
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    record_margin("additivity_large_launch_wall_s", wall, 2.0)  # "a second or two" with the poison call
    print(f"large launch B={blocks} fused={fused}: poison + call {wall:.3f} s")
    dead = [r for r in (1, 2, blocks // 2 + 1, blocks // 2 + 2, blocks - 2) if kinds[r] != 0]
    G, rows = run_rows(c, pool, lambda lo, hi, buf: c.bwd(o[lo:hi], d[lo:hi], g[lo:hi], buf), n, 256,
                       only_rows=live + dead)
    assert np.all(rows[len(live):, :7 * 33 + 4] == 0.0), "a dead row alone returns exact zeros"
    judge("large-launch", f"B={blocks} fused={fused}", 33, "bwd", None, G, rows[:len(live)])


# ---- 5. small kernel ---------------------------------------------------------------------------

@pytest.mark.parametrize("i,m", list(enumerate([1, 4, 7, 9, 15, 16, 31, 32])))
def test_small_rows(rm, pool, monkeypatch, i, m):
    """small_final's chains (8, 6, 4, 3, 2, 1, 1 and, at 32 spheres, 1 with two trips of the column
    loop) at 1, 3, 33, 128 rows; 129 rows leave the in-kernel final for the general reduction."""
    switches(monkeypatch)
    axis = i % 3
    c = Caller(rm, scene(rm, m, 50 + m, axis), 8)
    for nb in [1, 3, 33, 128, 129] + ([2, 4, 127] if m == 9 else []):
        n = 256 * nb - 100
        o, d = pool.take(n, start=nb + 13 * i)
        g = randn(n, 60 + nb)
        G, rows = run_rows(c, pool, lambda lo, hi, buf: c.bwd(o[lo:hi], d[lo:hi], g[lo:hi], buf), n, 256)
        assert judge("small", f"M={m} nb={nb} light axis {axis}", m, "bwd", axis, G, rows) == nb


@pytest.mark.parametrize("nb", [1, 127, 128])
def test_small_rows_train_two_lanes(rm, pool, monkeypatch, nb):
    """Train mode with two lanes per ray: 128 rays per row. 128 x 128 = 16,384 rays at 9 spheres is
    the reference's own batch, exactly kSmallFinalMaxBlocks rows."""
    import torch
    switches(monkeypatch, RM_SMALL_LPR="2")
    c = Caller(rm, scene(rm, 9, 70), 8)
    n = 128 * nb
    o, d = pool.take(n, start=nb)
    tg = torch.rand((n, 3), device="cuda", generator=torch.Generator("cuda").manual_seed(nb))
    tg = (tg * (torch.rand((n, 1), device="cuda", generator=torch.Generator("cuda").manual_seed(nb + 1)) > 0.3)).contiguous()
    inv = 1.0 / (3.0 * n)
    G, rows = run_rows(c, pool, lambda lo, hi, buf: c.train(o[lo:hi], d[lo:hi], tg[lo:hi], inv, buf), n, 128)
    assert judge("small", f"train two lanes nb={nb}", 9, "train", None, G, rows) == nb


# ---- 6. split march ----------------------------------------------------------------------------

SPLIT_M, SPLIT_STEPS = 256, 64
_split_cache = {}


def _split_inputs(rm, pool, oracle, want_A):
    """The rays and seeds of the largest split case (the smaller ones take prefixes) and, for the
    continuation runs, A = sum_rays |g_ray| from the oracle."""
    if "rays" not in _split_cache:
        n = 32 * 130 - 5
        o, d = pool.take(n, start=23)
        _split_cache["rays"] = (o, d, randn(n, 31))
    if want_A and "A" not in _split_cache:
        o, d, g = _split_cache["rays"]
        sc = scene(rm, SPLIT_M, 25)
        oh, dh, gh = (t.cpu().numpy() for t in (o, d, g))
        per_ray = np.zeros((oh.shape[0], 7 * SPLIT_M + 5))
        for i in range(oh.shape[0]):
            per_ray[i] = oracle_A(oracle, sc, SPLIT_STEPS, oh[i:i + 1], dh[i:i + 1], g=gh[i:i + 1])
        _split_cache["A"] = np.cumsum(per_ray, axis=0)
    return _split_cache["rays"], _split_cache.get("A")


@pytest.mark.parametrize("groups", [1, 9, 130])
@pytest.mark.parametrize("variant", ["one_launch", "continuations", "sub_launches"])
def test_split_rows(rm, pool, oracle, monkeypatch, variant, groups):
    """32-ray groups of the split march at 256 spheres, 64 steps: in one launch (no continuation),
    with continuations at steps 24 and 40 (groups deferred and resumed, their rays regrouped while
    they march: the oracle-A rule), and in sub-launches of 40 groups."""
    env = {"one_launch": {"RM_SPLIT_CONT_LIST": "0"}, "continuations": {"RM_SPLIT_CONT_LIST": "24,40"},
           "sub_launches": {"RM_SPLIT_CONT_LIST": "0", "RM_MAX_BLOCKS_PER_LAUNCH": "40"}}[variant]
    switches(monkeypatch, RM_SPLIT="1", **env)
    c = Caller(rm, scene(rm, SPLIT_M, 25), SPLIT_STEPS, poison_rpr=32)
    (o, d, g), A_cum = _split_inputs(rm, pool, oracle, variant == "continuations")
    n = 32 * groups - 5
    G, rows = run_rows(c, pool, lambda lo, hi, buf: c.bwd(o[lo:hi], d[lo:hi], g[lo:hi], buf), n, 32)
    tag = f"{variant} g={groups}"
    if variant == "continuations":
        judge("split", tag, SPLIT_M, "bwd", None, G, rows, A_sum=A_cum[n - 1], factor=2.0, n=groups)
    else:
        assert judge("split", tag, SPLIT_M, "bwd", None, G, rows) == groups


# ---- 7. camera mode ----------------------------------------------------------------------------

def _cams(model, v):
    return model.ring_cameras(v, fov=28.0)


@pytest.mark.parametrize("mode", ["bwd", "train"])
@pytest.mark.parametrize("m", [48, 12])
def test_camera_tile_rows(rm, pool, monkeypatch, m, mode):
    """V views of 16x16, one tile each: a one-view call is a row. 12 spheres run the small kernel,
    whose train mode is held to one lane per ray here so that a view stays one row."""
    import torch
    switches(monkeypatch, **({"RM_SMALL_LPR": "1"} if m == 12 and mode == "train" else {}))
    c = Caller(rm, scene(rm, m, 80 + m), 8)
    for v in (1, 2, 17, 128):
        cams = _cams(rm[1], v)
        n = 256 * v
        if mode == "bwd":
            g = randn(n, v)
            call = lambda lo, hi, buf: c.bwd_cam(cams[lo // 256:hi // 256], 16, 16, g[lo:hi], buf)  # noqa: E731
        else:
            tg = torch.rand((n, 3), device="cuda", generator=torch.Generator("cuda").manual_seed(v))
            inv = 1.0 / (3.0 * n)
            call = lambda lo, hi, buf: c.train_cam(cams[lo // 256:hi // 256], 16, 16, tg[lo:hi], inv, buf)  # noqa: E731
        G, rows = run_rows(c, pool, call, n, 256)
        assert judge("camera", f"M={m} {mode} V={v}", m, mode, None, G, rows) == v


def test_camera_small_train_default_lanes(rm, pool, oracle, monkeypatch):
    """The small kernel's camera train call as it runs by default: two lanes per ray, so a 16x16 view
    is two 128-ray rows and a one-view call carries a sum of its own -- the oracle-A rule over the
    n = 34 rows of 17 views."""
    import torch
    switches(monkeypatch)
    m, v = 12, 17
    sc = scene(rm, m, 80 + m)
    c = Caller(rm, sc, 8)
    cams = _cams(rm[1], v)
    n = 256 * v
    rays = [oracle.camera_rays(16, 16, *cam, precision="f32") for cam in cams]
    o, d = np.concatenate([r[0] for r in rays]), np.concatenate([r[1] for r in rays])
    tg = torch.rand((n, 3), device="cuda", generator=torch.Generator("cuda").manual_seed(v))
    inv = 1.0 / (3.0 * n)
    A_sum = oracle_A(oracle, sc, 8, o, d, targets=tg.cpu().numpy(), inv=inv)
    G, rows = run_rows(c, pool, lambda lo, hi, buf: c.train_cam(cams[lo // 256:hi // 256], 16, 16, tg[lo:hi], inv, buf),
                       n, 256, min_poison_rows=2 * v)
    judge("camera", "M=12 train V=17 two lanes", m, "train", None, G, rows, A_sum=A_sum, factor=2.0, n=2 * v)


@pytest.mark.parametrize("mode", ["bwd", "train"])
def test_camera_frames_of_several_tiles(rm, pool, oracle, monkeypatch, mode):
    """3 views of 48x32 (6 tiles each) against per-view calls: those carry sums of their own, so A
    comes from the oracle's per-ray gradients and the bound is 2 gamma_(n-1) A over the n = 18 tiles."""
    import torch
    switches(monkeypatch)
    m, w, h = 48, 48, 32
    sc = scene(rm, m, 90)
    c = Caller(rm, sc, 8)
    cams = _cams(rm[1], 3)
    npix = w * h
    n = 3 * npix
    rays = [oracle.camera_rays(w, h, *cam, precision="f32") for cam in cams]
    o, d = np.concatenate([r[0] for r in rays]), np.concatenate([r[1] for r in rays])
    if mode == "bwd":
        g = randn(n, 5)
        call = lambda lo, hi, buf: c.bwd_cam(cams[lo // npix:hi // npix], w, h, g[lo:hi], buf)  # noqa: E731
        A_sum = oracle_A(oracle, sc, 8, o, d, g=g.cpu().numpy())
    else:
        tg = torch.rand((n, 3), device="cuda", generator=torch.Generator("cuda").manual_seed(6))
        inv = 1.0 / (3.0 * n)
        call = lambda lo, hi, buf: c.train_cam(cams[lo // npix:hi // npix], w, h, tg[lo:hi], inv, buf)  # noqa: E731
        A_sum = oracle_A(oracle, sc, 8, o, d, targets=tg.cpu().numpy(), inv=inv)
    G, rows = run_rows(c, pool, call, n, npix)
    judge("camera", f"3 views of 48x32 {mode}", m, mode, None, G, rows, A_sum=A_sum, factor=2.0, n=18)


# ---- 8. accumulate and NULL outputs, bit for bit -----------------------------------------------

def _arena(c):
    """One arena filled with GUARD, 64 guard words around each of the five gradient buffers and the
    loss: (arena, offsets in floats, mask of the words inside the buffers)."""
    import torch
    m = c.m
    sizes = {"centers": 3 * m, "colors": 3 * m, "radius": m, "light_dir": 3, "ambient": 1, "loss": 1}
    offs, pos = {}, 64
    for k, s in sizes.items():
        offs[k] = pos
        pos += s + 64
    arena = torch.full((pos,), GUARD, device="cuda")
    return arena, offs, sizes


def _read(arena, offs, sizes, written):
    """The buffers' values by name after checking every word outside the written buffers."""
    a = arena.cpu().numpy()
    used = np.zeros(a.size, bool)
    for k in written:
        used[offs[k]:offs[k] + sizes[k]] = True
    assert (a[~used] == np.float32(GUARD)).all(), f"a write outside {sorted(written)}"
    return {k: a[offs[k]:offs[k] + sizes[k]].copy() for k in written}


def _abi_bits(c, call, n, rpr, mode, subs):
    """call(lo, hi, buf, acc, null, offs). accumulate on a non-zero prior, the sub-launch chain
    (subs: RM_MAX_BLOCKS_PER_LAUNCH setter and the three sub-ranges) and NULL members."""
    import torch
    names = list(A.KEYS) + (["loss"] if mode == "train" else [])

    def run(lo, hi, acc=0, null=(), prior=None):
        arena, offs, sizes = _arena(c)
        if prior is not None:
            for k in names:
                arena[offs[k]:offs[k] + sizes[k]] = torch.from_numpy(prior[k]).cuda()
        call(lo, hi, arena, acc, null, offs)
        torch.cuda.synchronize()
        return _read(arena, offs, sizes, [k for k in names if k not in null])

    base = run(0, n)
    assert all(np.isfinite(base[k]).all() for k in names)
    rng = np.random.default_rng(12)
    prior = {k: rng.standard_normal(base[k].shape).astype(np.float32) for k in names}
    got = run(0, n, acc=1, prior=prior)
    for k in names:  # accumulate: exactly float32(G0 + G)
        assert np.array_equal(got[k], prior[k] + base[k]), ("accumulate", k)
    for k in A.KEYS:  # each member NULL alone, and all but one NULL
        alone = run(0, n, null=(k,))
        only = run(0, n, null=tuple(x for x in A.KEYS if x != k))
        for x in names:
            if x != k:
                assert np.array_equal(alone[x], base[x]), ("NULL", k, x)
        assert np.array_equal(only[k], base[k]), ("all NULL but", k)
    set_sub, ranges = subs
    parts = [run(lo, hi) for lo, hi in ranges]  # the sub-ranges' own results
    set_sub()
    for acc in (0, 1):
        got = run(0, n, acc=acc, prior=prior if acc else None)
        for k in names:
            x = prior[k].copy() if acc else None
            for p in parts:  # the fp32 left-to-right chain, the prior first
                x = p[k].copy() if x is None else x + p[k]
            assert np.array_equal(got[k], x), ("sub-launch chain", acc, k)


def _thirds(n, rpr):
    """RM_MAX_BLOCKS_PER_LAUNCH and the ray ranges that cut n rays into three sub-launches."""
    rows = (n + rpr - 1) // rpr
    mb = (rows + 2) // 3
    assert (rows + mb - 1) // mb == 3
    return mb, [(i * mb * rpr, min(n, (i + 1) * mb * rpr)) for i in range(3)]


@pytest.mark.parametrize("path", ["general", "split", "small_bwd", "small_train", "camera"])
def test_accumulate_null_outputs_and_guards(rm, pool, monkeypatch, path):
    import torch
    env, m, steps, rpr, n = {"general": ({"RM_SPLIT": "0"}, 33, 8, 256, 5 * 256 - 100),
                             "split": ({"RM_SPLIT": "1"}, 256, 16, 32, 9 * 32 - 5),
                             "small_bwd": ({}, 9, 8, 256, 5 * 256 - 100),
                             "small_train": ({}, 9, 8, 128, 6 * 128 - 50),
                             "camera": ({}, 48, 8, 256, 3 * 256)}[path]
    switches(monkeypatch, **env)
    c = Caller(rm, scene(rm, m, 95), steps)
    mode = "train" if path == "small_train" else "bwd"
    if path == "camera":
        cams = _cams(rm[1], 3)
        g = randn(n, 2)
        call = lambda lo, hi, buf, acc, null, offs: c.bwd_cam(cams[lo // 256:hi // 256], 16, 16, g[lo:hi], buf, acc,  # noqa: E731
                                                              null, offs)
    elif mode == "train":
        o, d = pool.take(n, start=31)
        tg = torch.rand((n, 3), device="cuda", generator=torch.Generator("cuda").manual_seed(3))
        inv = 1.0 / (3.0 * n)
        call = lambda lo, hi, buf, acc, null, offs: c.train(o[lo:hi], d[lo:hi], tg[lo:hi], inv, buf, acc, null, offs)  # noqa: E731
    else:
        o, d = pool.take(n, start=37)
        g = randn(n, 4)
        call = lambda lo, hi, buf, acc, null, offs: c.bwd(o[lo:hi], d[lo:hi], g[lo:hi], buf, acc, null, offs)  # noqa: E731
    mb, ranges = _thirds(n, rpr)
    _abi_bits(c, call, n, rpr, mode, (lambda: monkeypatch.setenv("RM_MAX_BLOCKS_PER_LAUNCH", str(mb)), ranges))


# ---- 9. pose gradients -------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(16, 16), (72, 64)])
@pytest.mark.parametrize("v", [3, 128])
def test_pose_gradients_equal_one_view_calls(rm, monkeypatch, v, w, h):
    """grad_cams[v] of a V-view rm_render_diff_backward_cameras call has the bits of the one-view
    call (test_gpu_raygrad.py compares repeated views with each other, not with a call of their own)."""
    import torch
    switches(monkeypatch)
    render, model, _ = rm
    s = model.scene_tensors(scene(rm, 48, 96))
    cams = _cams(model, v)
    npix = w * h
    g = randn(v * npix, 9)
    full = render.render_diff_backward_cameras(cams, w, h, s, K, g, 8)
    rows = torch.empty((v, 7), device="cuda")
    for i in range(v):
        render.render_diff_backward_cameras(cams[i:i + 1], w, h, s, K, g[i * npix:(i + 1) * npix], 8,
                                            grad_cams=rows[i:i + 1])
    torch.cuda.synchronize()
    a, b = full.cpu().numpy(), rows.cpu().numpy()
    assert np.isfinite(a).all() and np.any(a != 0.0)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
