"""One rm_context, every family of entry points: a call on a context that calls of other families have used
gives the bits it gives on a context nobody has used.

Every family's own suite makes its inputs, calls its own family and compares; a real caller renders with SH,
scores with image_loss, runs backward, steps the optimizer, queries the field and renders a viewer frame on one
context. The families share that context's grow-only buffers (the workspace and its sub-layouts, the record
buffer, the ray-gradient workspace, the coefficient records, the loss workspace, the continuation buffer, the
lattice and the tile proof, the drawn batch), its arrival counters, the cost-order lists with their device turn
word, the device camera table and the prepared optimizer hand-off (csrc/rm_context.h). The project states that a
call's outputs are a function of its arguments alone, so the oracle here is exact: the same call on a fresh
context, which the family's own parity file (or the node's `restate` check) ties to a high-precision reference.
Every comparison below is equality of words; there is no tolerance in this file.

tests/context_calls.py holds the catalogue of calls ("nodes"), one or two per family, small and large.

Measured on an MI355X (profiles/r33_context_families_times.txt): the whole file, 96 tests, runs in about 4 s; a
history of 61 calls with its clones and device compares takes 0.01 to 0.04 s, a fresh context's first call under
a millisecond to 6 ms, the catalogue's inputs half a second. profiles/r33_context_families_mutants.txt: a
prepare_records that skips rm_prep_finish after a call with more record blocks fails
test_node_among_all_others[a_m1100] at "g_rays_C10, right after a_m1100"."""
import ctypes

import numpy as np
import pytest

import context_calls as C
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]


@pytest.fixture(scope="module")
def rm():
    import torch
    from burn_raymarching_amd import _build
    _build.build_lib()
    from burn_raymarching_amd import model, native, render
    torch.cuda.init()
    return torch, render, model, native


def nodes_of(rm):
    return C.catalogue(*rm)


def node_of(rm, name):
    return nodes_of(rm)[C.NAMES.index(name)]


_REF = {}


def reference(rm, node):
    """The node's outputs on a context nobody has used: computed once per node, kept, finite and non-zero."""
    torch, render = rm[0], rm[1]
    if node.name not in _REF:
        with C.fresh_context(torch, render):
            ref = C._run(node)
        for t in ref:
            x = t.float()
            if node.name.startswith("j_view"):  # the depth of a viewer's miss is +inf
                x = x[x != float("inf")]
            assert torch.isfinite(x).all(), node
        assert any(t.float().abs().max() > 0 for t in ref), node
        _REF[node.name] = ref
    return _REF[node.name]


def run_history(rm, history, what):
    """The nodes of `history` in order on one fresh context, every call's outputs cloned and compared on the
    device with the node's reference; one synchronisation for the whole sequence. Returns the adjacent pairs."""
    torch, render = rm[0], rm[1]
    refs = [reference(rm, n) for n in history]
    with C.fresh_context(torch, render):
        got = [C._run(n) for n in history]
        ok = torch.stack([C.words_equal(g, r) for g, r in zip(got, refs)]).cpu().tolist()
    for i, good in enumerate(ok):
        if not good:
            before = history[i - 1].name if i else "(a fresh context)"
            C._same(got[i], refs[i], f"{what}: call {i} of {len(history)}, {history[i].name}, right after {before}")
    return {(a.name, b.name) for a, b in zip(history, history[1:])}


# ---- 2. every node runs the path it is named for ---------------------------------------------------------------

@pytest.mark.parametrize("name", C.NAMES)
def test_node_runs_its_path(rm, name):
    """The diagnostics of one run on a fresh context (work counters on, not bit-compared): the launch sizes say
    which kernel and how many rays a block, the order counts that a keyed launch appended its lists (node d: to
    the shards), the tile-proof bytes that the pre-pass ran (node d alone), the fused-Adam node's and the
    iterations' parameters moved. Then the reference: finite, non-zero and, for a shape no parity file pins,
    within its family's restatement's bounds."""
    torch, render = rm[0], rm[1]
    node = node_of(rm, name)
    ref = reference(rm, node)
    info = C.diagnostics(torch, render, node)
    if node.evidence is not None:
        node.evidence(info)
    else:  # a family without work counters (the field, the viewer, the loss): no per-ray launch at all
        assert info["stats"]["blocks"] == 0, info["stats"]
    if node.restate is not None:
        node.restate(ref)


# ---- 3. histories ----------------------------------------------------------------------------------------------

def history_around(nodes, a):
    """a, b1, a, b2, a, ..., bn, a: every node right before and right after `a`, `a` itself included."""
    h = [a]
    for b in nodes:
        h += [b, a]
    return h


_PAIRS, _RAN = set(), set()


@pytest.mark.parametrize("name", C.NAMES)
def test_node_among_all_others(rm, name):
    nodes = nodes_of(rm)
    _PAIRS.update(run_history(rm, history_around(nodes, node_of(rm, name)), f"around {name}"))
    _RAN.add(name)


def test_every_ordered_pair_is_exercised(rm):
    """The histories of test_node_among_all_others put every ordered pair of nodes next to each other on a used
    context; counted from the histories, and from what ran when every node's test did."""
    nodes = nodes_of(rm)
    planned = set()
    for a in nodes:
        h = history_around(nodes, a)
        planned.update((x.name, y.name) for x, y in zip(h, h[1:]))
    assert len(planned) == len(nodes) ** 2
    if _RAN == set(C.NAMES):
        assert len(_PAIRS) == len(nodes) ** 2, (len(_PAIRS), len(nodes) ** 2)


def test_reverse_and_shuffled_histories(rm):
    """One context: the catalogue in order, in reverse, then three seeded permutations of it."""
    nodes = nodes_of(rm)
    history = list(nodes) + list(reversed(nodes))
    for seed in (1, 2, 3):
        history += [nodes[i] for i in np.random.default_rng(seed).permutation(len(nodes))]
    run_history(rm, history, "catalogue, reverse, permutations 1 2 3")


# histories that found a fault keep a test of their own: test_replay_after_a_call_of_another_tiling below


# ---- the prepared optimizer hand-off with another family's call in between -----------------------------------

class PreparedStep:
    """rm_train_step_sampled_prepared -> (an intruder's call) -> rm_optimizer_step of a 7-sphere model on 8,000
    rays drawn from two 48x48 views (tests/test_gpu_small.py::test_prepared_step_dropped_by_another_call's shape),
    each run from the same start in buffers of its own."""

    def __init__(self, rm, m=7, seed=123):
        torch, render, model, native = rm
        self.rm, self.m, self.nu, self.nf = rm, m, 6000, 2000
        rays = [render.create_camera_rays(48, 48, *c) for c in model.ring_cameras(2)]
        self.o = torch.cat([r[0] for r in rays]).contiguous()
        self.d = torch.cat([r[1] for r in rays]).contiguous()
        self.tg = C.dev(np.random.default_rng(5).uniform(size=(self.o.shape[0], 3)))
        self.fg = torch.arange(0, self.o.shape[0], 2, dtype=torch.int32, device="cuda")
        sc = model.synthetic_scene(self.m, seed, radius_range=(0.08, 0.3))
        sm = model.SceneModel.from_activated(sc["centers"], sc["colors"], sc["radius"], sc["light_dir"], sc["ambient"])
        self.init = (sm.raw.clone(), sm.activated_packed().clone())
        torch.cuda.synchronize()

    def buffers(self):
        torch, model = self.rm[0], self.rm[2]
        npk = model.packed_size(self.m)
        return {"raw": self.init[0].clone(), "act": self.init[1].clone(), "grad": torch.zeros(npk, device="cuda"),
                "m1": torch.zeros(npk, device="cuda"), "m2": torch.zeros(npk, device="cuda"),
                "loss": torch.zeros(2, device="cuda")}

    def prepare(self, b, prepare=True):
        """The preparing sampled step on the buffers b; returns [gradient, losses] as the call left them."""
        _, render, _, native = self.rm
        p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
        ctx = render.context()
        s, g = native.RmScene(), native.RmGrads()
        ctx._lib.rm_scene_from_packed(p(b["act"]), self.m, ctypes.byref(s))
        ctx._lib.rm_grads_from_packed(p(b["grad"]), self.m, ctypes.byref(g))
        march = native.march_params(40, 20.0)
        with C.switches({"RM_OPT_PREPARE": "1" if prepare else "0"}):
            ctx.check(ctx._lib.rm_train_step_sampled_prepared(
                ctx.handle, p(self.o), p(self.d), p(self.tg), self.o.shape[0], p(self.fg), self.fg.numel(), self.nu,
                self.nf, 3, 1, 1, 0.5, 1.0 / (3 * (self.nu + self.nf)), ctypes.byref(s), ctypes.byref(march),
                ctypes.byref(g), p(b["loss"]), p(b["raw"]), 1, 1, ctypes.c_void_p(b["loss"].data_ptr() + 4)),
                "rm_train_step_sampled_prepared")
        return [b["grad"], b["loss"]]

    def run(self, prepare, intruder=None):
        """Returns the step's results, the intruder's outputs and the penalty loss as the sampled step left it:
        the extra block of a launch that prepares writes it (opt_small_pre), a step that does not prepare leaves
        it to the optimizer call -- the one trace of the hand-off a caller can see before that call."""
        _, render, _, _ = self.rm
        p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
        ctx = render.context()
        b = self.buffers()
        self.prepare(b, prepare)
        mid_penalty = b["loss"][1:].clone()
        between = C._run(intruder) if intruder is not None else None
        with C.switches({"RM_OPT_PREPARE": "1" if prepare else "0"}):
            ctx.check(ctx._lib.rm_optimizer_step(ctx.handle, p(b["raw"]), p(b["grad"]), p(b["m1"]), p(b["m2"]), self.m, 1,
                                                 0.01, 1e-5, 1, ctypes.c_void_p(b["loss"].data_ptr() + 4), p(b["act"])),
                      "rm_optimizer_step")
        return [b["raw"], b["act"], b["m1"], b["m2"], b["loss"], b["grad"]], between, mid_penalty


_PREPARED = {}


def prepared_reference(rm):
    """The unprepared pair (RM_OPT_PREPARE=0: the full optimizer step) on a fresh context, and the prepared pair
    with nothing in between: the two are equal (tests/test_gpu_small.py pins that), something happened, and the
    preparing step did prepare: it wrote the penalty loss itself, which the unprepared step leaves at zero."""
    torch, render = rm[0], rm[1]
    if not _PREPARED:
        step = PreparedStep(rm)
        with C.fresh_context(torch, render):
            plain, _, plain_mid = step.run(False)
        with C.fresh_context(torch, render):
            prepared, _, prepared_mid = step.run(True)
        C._same(prepared, plain, "the prepared pair against the unprepared one")
        assert all(torch.isfinite(t).all() for t in plain) and not torch.equal(plain[0], step.init[0]) and plain[4][1] > 0
        assert plain_mid.item() == 0.0 and prepared_mid.item() > 0.0 and torch.equal(prepared_mid, plain[4][1:])
        _PREPARED["step"], _PREPARED["ref"] = step, plain
    return _PREPARED["step"], _PREPARED["ref"]


@pytest.mark.parametrize("name", C.NAMES)
def test_prepared_optimizer_with_an_intruder(rm, name):
    """The node's call between the preparing step and its optimizer step: the raw parameters, the moments, the
    activated values and the penalty loss (and the gradient) are the unprepared pair's on a fresh context -- the
    hand-off is dropped, or still holds what the step prepared -- and the intruder's own outputs are its
    reference's. The node's buffers are its own: it changes no parameter of the step."""
    torch, render = rm[0], rm[1]
    step, ref = prepared_reference(rm)
    node = node_of(rm, name)
    node_ref = reference(rm, node)
    with C.fresh_context(torch, render):
        got, between, mid = step.run(True, node)
    assert mid.item() > 0.0  # the step prepared (see prepared_reference)
    C._same(got, ref, f"prepared step, {name}, optimizer step: (raw, act, adam_m, adam_v, loss, grad)")
    C._same(between, node_ref, f"{name} right after a preparing step")


def test_prepared_optimizer_after_another_models_preparing_step(rm):
    """The intruder is itself a preparing sampled step, on another model's parameters (9 spheres, buffers of its
    own): it overwrites the hand-off and leaves it marked as prepared -- for its own arguments. The first model's
    optimizer step must not take it: its results are the unprepared pair's, and the intruding step's gradient
    and losses are those it gives on a fresh context."""
    torch, render = rm[0], rm[1]
    step, ref = prepared_reference(rm)
    other = PreparedStep(rm, m=9, seed=77)
    with C.fresh_context(torch, render):
        alone = C._run(lambda: other.prepare(other.buffers()))
    assert alone[1][1] > 0  # it prepared too
    with C.fresh_context(torch, render):
        got, between, mid = step.run(True, lambda: other.prepare(other.buffers()))
    assert mid.item() > 0.0
    C._same(got, ref, "prepared step, another model's preparing step, optimizer step")
    C._same(between, alone, "another model's preparing step right after a preparing step")


# ---- two autograd graphs on one context ----------------------------------------------------------------------

def _leaves(sc, names):
    return {k: C.dev(sc[k]).requires_grad_(True) for k in names}


def test_two_autograd_graphs_in_flight(rm):
    """out1 = render_diff_sh on one scene, out2 = render_diff_cameras on another, then
    (image_loss(out1) + 2 image_loss(out2)).backward(): the two graphs' forwards and backwards interleave on one
    context. Every leaf gradient equals the one of its graph alone on a fresh context. Graph 2 alone is seeded by
    hand -- rm_image_loss's gradient times a float32 2, the multiply _ImageLossFn.backward makes -- so that a
    backward that ignored its incoming scalar would differ."""
    import sh_ref as R
    torch, render, model, native = rm
    c = R.case("m33_d2")
    w = R.WIDTH
    o, d = C.dev(c["org"]), C.dev(c["dir"])
    sc2 = model.synthetic_scene(64, 7)
    cams = model.ring_cameras(3)[:2]
    rng = np.random.default_rng(31)
    t1, t2 = C.dev(rng.uniform(size=(w * w, 3))), C.dev(rng.uniform(size=(2 * w * w, 3)))
    keys = ("centers", "colors", "radius", "light_dir", "ambient")

    def graph1():
        lv = _leaves(c["scene"], keys)
        lv["sh"] = C.dev(c["sh"]).requires_grad_(True)
        out = render.render_diff_sh(o, d, lv["centers"], lv["colors"], lv["sh"], lv["radius"], lv["light_dir"],
                                    lv["ambient"], c["k"], c["steps"], **R.CONSTS)
        return lv, out

    def graph2():
        lv = _leaves(sc2, keys)
        lv["eye"] = torch.tensor([cm[0] for cm in cams], dtype=torch.float32, device="cuda", requires_grad=True)
        lv["target"] = torch.tensor([cm[1] for cm in cams], dtype=torch.float32, device="cuda", requires_grad=True)
        lv["fov"] = torch.tensor([cm[2] for cm in cams], dtype=torch.float32, device="cuda", requires_grad=True)
        out = render.render_diff_cameras(lv["eye"], lv["target"], lv["fov"], w, w, lv["centers"], lv["colors"],
                                         lv["radius"], lv["light_dir"], lv["ambient"], 32.0, 24)
        return lv, out

    def grads(lv):
        assert all(v.grad is not None for v in lv.values()), [k for k, v in lv.items() if v.grad is None]
        return {k: v.grad.clone() for k, v in lv.items()}

    with C.fresh_context(torch, render):
        lv, out = graph1()
        render.image_loss(out, t1, w, w).backward()
        alone1 = grads(lv)
    with C.fresh_context(torch, render):
        lv, out = graph2()
        g = render.image_loss_call(out.detach(), t2, w, w, grad=True)["grad"]
        out.backward((g * torch.tensor(2.0, device="cuda")).reshape(out.shape))
        alone2 = grads(lv)
        unscaled = render.render_diff_backward_camera(cams, w, w, render.Scene(*(lv[k].detach() for k in keys)), 32.0,
                                                      g.reshape(-1, 3), 24)["centers"].clone()
    with C.fresh_context(torch, render):
        lv1, out1 = graph1()
        lv2, out2 = graph2()
        (render.image_loss(out1, t1, w, w) + 2 * render.image_loss(out2, t2, w, w)).backward()
        both1, both2 = grads(lv1), grads(lv2)
    for alone, both, tag in ((alone1, both1, "render_diff_sh"), (alone2, both2, "render_diff_cameras")):
        for k in alone:
            assert torch.isfinite(alone[k]).all() and alone[k].abs().max() > 0, (tag, k)
            C._same([both[k]], [alone[k]], f"{tag}: d loss / d {k}, both graphs in flight against the graph alone")
    # the factor 2 is in graph 2's gradients (the render's backward is linear in its seed: times 2 is exact)
    assert torch.equal(both2["centers"], unscaled * 2.0) and not torch.equal(both2["centers"], unscaled)


# ---- a captured call replayed after other families' calls ----------------------------------------------------

def replay_after(rm, captured, others):
    """After one eager run of everything on a fresh context (so nothing grows later: a captured call holds the
    buffers' addresses), capture each of `captured` in a hipGraph, run `others` eagerly, replay, and compare all
    of it with the references."""
    torch, render = rm[0], rm[1]
    refs = {n.name: reference(rm, n) for n in captured + others}
    with C.fresh_context(torch, render) as (s, ctx):
        for n in others + captured:  # the eager warm-up: every buffer at its final size
            C._same(C._run(n), refs[n.name], f"{n.name}, eager, before the captures")
        torch.cuda.synchronize()
        graphs = []
        for n in captured:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                out = n()
            graphs.append((n, g, out))
        for n in others:
            C._same(C._run(n), refs[n.name], f"{n.name}, eager, after the captures")
        for n, g, out in graphs:
            for t in out:
                t.fill_(float("nan")) if t.is_floating_point() else t.zero_()
            g.replay()
            torch.cuda.synchronize()
            C._same([t.clone() for t in out], refs[n.name], f"{n.name} replayed after {[o.name for o in others]}")


def test_replay_after_other_families(rm):
    """Node c (the tiled, cost-ordered train step) and node k (the image loss), each captured in a hipGraph after
    one eager run, then other nodes eagerly on the same context, then the replays: the references' bits. The
    nodes in between leave c's two views alone (the capture contract of upload_cams; c passes its cameras by
    value). They include a keyed launch of c's own key (n: the lists the replay reads are n's), the sharded one
    of another key (d: the replay finds the lists short and takes the static order) and unkeyed backward calls,
    which drop the host's cost_valid while the device turn word stays where the replay expects it."""
    captured = [node_of(rm, "c_m128_tiled"), node_of(rm, "k_image_loss_2x33x17")]
    others = [node_of(rm, n) for n in ("n_m128_f16_colours", "d_m128_lattice_shards", "h_sh_backward_camera_m33_d2",
                                       "i_sdf_all_m9", "a_bwd_300_rays_m40")]
    replay_after(rm, captured, others)


def test_replay_after_a_call_of_another_tiling(rm):
    """Regression: c (2 x 2 tiles of 256 rays) captured, then eager tiled calls of other tilings -- e (2 x 2 tiles
    in 32-ray blocks, a 32-entry order), f (1 x 1) and m (4 x 4) -- then the replay. The context used to keep
    one block-order table and rewrite it in place for each new tiling, so the replayed c, which holds the
    table's address, read another tiling's order: block numbers past its eight blocks. Every tiling now has a
    table of its own that is never rewritten (BlockOrder, csrc/rm_context.h)."""
    captured = [node_of(rm, "c_m128_tiled")]
    others = [node_of(rm, n) for n in ("e_m256_split_cont", "f_17_views", "m_fused_adam_m64")]
    replay_after(rm, captured, others)
