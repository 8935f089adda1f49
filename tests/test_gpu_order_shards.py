"""The sharded last cost class of the cost-ordered dispatch (kOrderShards, order_shard_policy; env
RM_ORDER_SHARDS) changes no bit: partial records are indexed by the logical block, so the image, the
loss and every gradient of a cost-ordered call equal (==) the static order's (RM_STATIC_ORDER=1) and
the one-list order's (RM_ORDER_SHARDS=0), and the per-class block counts a call leaves -- costs do
not depend on the order -- are the same either way (rm_debug_order_counts sums the shards).

Scenes: a small cluster at the origin seen from the ring (border tiles end in the last cost class,
centre tiles do not), the same cluster moved out of every view (the last class is the whole
launch), and a scene filling the view (the last class is empty). Launch totals and last-class
counts cover at least four residues mod 8 each: whole rounds of the XCD rotation and every remainder.

Before each series the context's workspace is poisoned as in tests/test_gpu_additivity.py: an
array-mode backward call with as many rows, all live, seeds times 2^40.
"""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

K, STEPS = 32.0, 32
LAST = 15  # the last cost class (kOrderClasses - 1)
# (views, W, H, spheres): 6 (under one round), 16, 45, 128 and 245 blocks
MIXED = [(1, 48, 32, 48), (1, 64, 64, 64), (3, 80, 48, 96), (2, 128, 128, 64), (5, 112, 112, 80)]
AWAY = (1, 80, 48, 64)   # 15 blocks, all of them in the last class
FULL = (1, 64, 64, 96)   # 16 blocks, none of them there


@pytest.fixture(scope="module")
def mods():
    import torch
    from burn_raymarching_amd import model, native, render
    torch.cuda.init()
    return torch, model, native, render


def _scene(model, m, kind, seed=11):
    sc = model.synthetic_scene(m, seed)
    if kind == "full":  # a ball of radius 1.8 around the origin: every ray of a ring view meets it
        sc["centers"] *= 3.0
        sc["radius"] *= 3.0
    else:               # a cluster of radius 0.2: the middle quarter of a ring view's width
        sc["centers"] *= 0.3
        sc["radius"] *= 0.5
    if kind == "away":  # far up the ring's axis: in no view
        sc["centers"][:, 1] += 40.0
    return sc


class Series:
    """Train calls of one shape on the context of torch's current stream."""

    def __init__(self, mods, shape, kind):
        torch, model, native, render = mods
        self.torch, self.render = torch, render
        v, self.w, self.h, m = shape
        self.cams = model.ring_cameras(max(10, v))[:v]
        self.sc = model.scene_tensors(_scene(model, m, kind), "cuda")
        tsc = _scene(model, m, kind, seed=12)
        self.tgt = render.render_diff_camera(self.cams, self.w, self.h, model.scene_tensors(tsc, "cuda"), K, STEPS)
        self.blocks = v * (self.w // 16) * (self.h // 16)
        # the poison call's rays: a narrow view of the cluster (or the ball), a row of 256 rays per block
        eye = [2.5, 40.5 if kind == "away" else 0.5, 0.0]
        at = [0.0, 40.0 if kind == "away" else 0.0, 0.0]
        po, pd = render.create_camera_rays(64, 64, eye, at, 4.0)
        idx = torch.arange(256 * self.blocks, device="cuda") % (64 * 64)
        self.po, self.pd = po[idx].contiguous(), pd[idx].contiguous()
        gen = torch.Generator("cuda").manual_seed(99)
        self.pg = torch.randn((256 * self.blocks, 3), device="cuda", generator=gen) * 2.0 ** 40

    def poison(self):
        self.render.render_diff_backward(self.po.view(-1, 3), self.pd.view(-1, 3), self.sc, K, self.pg, STEPS)

    def run(self):
        torch = self.torch
        out = torch.full_like(self.tgt, float("nan"))
        loss, g, _ = self.render.train_step_camera(self.cams, self.w, self.h, self.tgt, self.sc, K, 0.5, STEPS, out=out)
        torch.cuda.synchronize()
        counts, nxt = self.render.context().order_counts()
        self.lists = self.render.context().order_shard_counts()[(nxt + 2) % 3]  # the last class, list by list
        return loss.clone(), {k: v.clone() for k, v in g.items()}, out, counts[(nxt + 2) % 3]


def _same(torch, a, b, what):
    assert torch.equal(a[2], b[2]), (what, "image")
    assert torch.equal(a[0], b[0]), (what, "loss")
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), (what, k)


def _series(mods, monkeypatch, shape, kind, env=()):
    """The static order's result, three one-list calls and three sharded calls; returns the counts."""
    torch = mods[0]
    for name, v in env:
        monkeypatch.setenv(name, v)
    s = Series(mods, shape, kind)
    monkeypatch.setenv("RM_STATIC_ORDER", "1")
    s.poison()
    static = s.run()
    assert torch.isfinite(static[2]).all() and torch.isfinite(static[0]).all()
    monkeypatch.setenv("RM_STATIC_ORDER", "0")
    runs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("RM_ORDER_SHARDS", mode)
        s.poison()
        s.run()  # lays the cost history
        runs[mode] = [s.run() for _ in range(3)]
        # the path under test ran: the last class's appends went to several lists, or to the first alone
        # (five blocks have launch positions of at least two residues mod 4)
        last = runs[mode][2][3][LAST]
        assert sum(s.lists) == last, (mode, s.lists, last)
        if mode == "0":
            assert s.lists[1:] == [0] * (len(s.lists) - 1), s.lists
        elif last >= 5:
            assert sum(1 for n in s.lists if n) >= 2, s.lists
    for i in range(3):
        print(f"{kind} {shape} call {i}: class counts off {runs['0'][i][3]} on {runs['1'][i][3]}")
        _same(torch, runs["1"][i], static, f"sharded call {i} against the static order")
        _same(torch, runs["1"][i], runs["0"][i], f"sharded call {i} against the one-list order")
        assert runs["1"][i][3] == runs["0"][i][3], i
        assert sum(runs["1"][i][3]) == s.blocks
    return runs["1"][0][3]


_counts = {}


def _counts_of(mods, monkeypatch, shape, kind):
    if (shape, kind) not in _counts:
        _counts[(shape, kind)] = _series(mods, monkeypatch, shape, kind)
    return _counts[(shape, kind)]


@pytest.mark.parametrize("shape", MIXED)
def test_sharded_order_changes_no_bit(mods, monkeypatch, shape):
    counts = _counts_of(mods, monkeypatch, shape, "cluster")
    assert 0 < counts[LAST] < sum(counts), counts  # border tiles in the last class, centre tiles not


def test_last_class_is_the_whole_launch(mods, monkeypatch):
    counts = _counts_of(mods, monkeypatch, AWAY, "away")
    assert counts[LAST] == sum(counts), counts


def test_last_class_is_empty(mods, monkeypatch):
    counts = _counts_of(mods, monkeypatch, FULL, "full")
    assert counts[LAST] == 0, counts


def test_shapes_cover_the_rounds(mods, monkeypatch):
    """Totals and last-class counts of the shapes above: at least four residues mod 8 each."""
    cases = [(s, "cluster") for s in MIXED] + [(AWAY, "away"), (FULL, "full")]
    counts = [_counts_of(mods, monkeypatch, s, k) for s, k in cases]
    print("totals", [sum(c) for c in counts], "last class", [c[LAST] for c in counts])
    assert len({sum(c) % 8 for c in counts}) >= 4, [sum(c) for c in counts]
    assert len({c[LAST] % 8 for c in counts}) >= 4, [c[LAST] for c in counts]


@pytest.mark.parametrize("views,sharded", [(19, False), (20, True)])
def test_policy_threshold(mods, monkeypatch, views, sharded):
    """With the env unset the policy decides: 20 views of 512x512 (20,480 blocks) shard the last class,
    19 views keep one list; either way the result equals the static order's."""
    torch = mods[0]
    monkeypatch.delenv("RM_ORDER_SHARDS", raising=False)
    s = Series(mods, (views, 512, 512, 48), "cluster")
    monkeypatch.setenv("RM_STATIC_ORDER", "1")
    static = s.run()
    monkeypatch.setenv("RM_STATIC_ORDER", "0")
    s.run()
    got = s.run()
    _same(torch, got, static, f"{views} views against the static order")
    assert sum(got[3]) == s.blocks and sum(s.lists) == got[3][LAST] > 5, (got[3], s.lists)
    assert (sum(1 for n in s.lists if n) >= 2) == sharded, s.lists
    assert sharded or s.lists[1:] == [0] * (len(s.lists) - 1), s.lists


def test_proof_instance(mods, monkeypatch):
    """The proof instance of the kernel (128 spheres, the lattice forced): the same equalities, and
    the work counters of a call are the same with the shards on and off."""
    torch, model, native, render = mods
    monkeypatch.setenv("RM_PROOF_LATTICE", "1")
    s = Series(mods, (4, 64, 64, 128), "cluster")
    ctx = render.context()
    monkeypatch.setenv("RM_STATIC_ORDER", "1")
    s.poison()
    static = s.run()
    monkeypatch.setenv("RM_STATIC_ORDER", "0")
    got = {}
    ctx.stats(True)
    try:
        for mode in ("0", "1"):
            monkeypatch.setenv("RM_ORDER_SHARDS", mode)
            s.poison()
            s.run()
            ctx.collect_stats(reset=True)
            runs = [s.run() for _ in range(3)]
            got[mode] = (runs, ctx.collect_stats(reset=True))
    finally:
        ctx.stats(False)
    print("proof instance: counts", got["1"][0][0][3], "work", got["1"][1])
    for i in range(3):
        _same(torch, got["1"][0][i], static, i)
        _same(torch, got["1"][0][i], got["0"][0][i], i)
        assert got["1"][0][i][3] == got["0"][0][i][3]
    for k in ("blocks", "waves", "waves_exited", "steps_saved"):
        assert got["1"][1][k] == got["0"][1][k], (k, got["1"][1], got["0"][1])
    assert got["1"][1]["waves_exited"] > 0 and 0 < got["1"][0][0][3][LAST] < s.blocks
