"""The tile proof on the GPU (rm_tile_proof_kernel, KArgs::tile_proof): a camera call with
the escape lattice marches one bound cone per wave tile before its per-ray launch, and a wave whose byte is set
stops where bound_proof would have stopped it. Exact: the train step with the tile proof (RM_PROOF_LATTICE=1),
with the soft ball alone (=0) and with the exit off gives the same bits; the rm_stats counters are never below
the soft ball's (a wave whose byte is 0 runs the soft-ball proof) and above them where the CPU restatement
(tests/test_tile_proof_reference.py) says so; and the bytes, read back, are the restatement's.

The cases are tests/test_gpu_escape_lattice.py's ten, at their sizes, and three more: a 90 degree field of view
(the widest cones), two views from different eyes in one call, and a 40x40 view. The 16x16 tiling admits no
partial block (a tiled view is whole 256-ray blocks), so the view with a partial last block is one in row order:
1600 rays, six blocks and a quarter. There a wave is no pixel rectangle: the launch takes no tile proof (no
bytes) and reads the lattice per ray inside bound_proof, which still proves more than the soft ball.
RM_SMALL=0 / RM_SPLIT=0: the general unsplit kernel, the proof's scope."""
import numpy as np
import pytest

from conftest import gpu_available
from escape_ref import CASES as LATTICE_CASES
from escape_ref import GAP_CAM, _train, cloud_scene, gap_scene, model_bytes, outlier_scene

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

CASES = dict(LATTICE_CASES)
CASES.update({
    "wide-fov": lambda: (cloud_scene(300), [([0.0, 0.5, 2.5], [2.2, 0.5, 0.0], 90.0)], (48, 80), 32, 32.0),
    "two-eyes": lambda: (gap_scene(128), [GAP_CAM, ([1.5, 0.4, 2.2], [0.0, 0.0, 0.0], 60.0)], (64, 64), 32, 32.0),
    "rows-40x40": lambda: (gap_scene(128), [GAP_CAM], (40, 40), 32, 32.0),
})


@pytest.fixture(scope="module")
def mods():
    import torch
    from burn_raymarching_amd import model, native, render
    torch.cuda.init()
    return torch, model, render, native


@pytest.fixture(autouse=True)
def general_kernel(monkeypatch):
    monkeypatch.setenv("RM_SMALL", "0")
    monkeypatch.setenv("RM_SPLIT", "0")
    monkeypatch.delenv("RM_PROOF_LATTICE", raising=False)
    monkeypatch.delenv("RM_NO_EARLY_EXIT", raising=False)


@pytest.fixture(scope="module")
def runs(mods):
    """per case, computed once: the train step and its counters with the tile proof (and the bytes its launch
    read), with the soft ball alone and with the exit off"""
    cache = {}

    def get(name, monkeypatch):
        if name not in cache:
            _, model, render, _ = mods
            scd, cams, (w, h), S, k = CASES[name]()
            sc = model.scene_tensors(scd, "cuda")
            res = {}
            for mode, env in (("tile", {"RM_PROOF_LATTICE": "1"}), ("ball", {"RM_PROOF_LATTICE": "0"}),
                              ("exit-off", {"RM_NO_EARLY_EXIT": "1", "RM_PROOF_LATTICE": "1"})):
                with monkeypatch.context() as mp:
                    for key, v in env.items():
                        mp.setenv(key, v)
                    res[mode] = _train(mods, sc, cams, w, h, S, k)
                if mode == "tile":
                    res["bytes"] = np.frombuffer(render.context().tile_proof(), np.uint8).copy()
            cache[name] = (res, len(cams), w, h, S)
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(CASES))
def test_tile_proof_changes_no_bit_and_saves_no_less(mods, runs, monkeypatch, name):
    torch = mods[0]
    res, views, w, h, S = runs(name, monkeypatch)
    (tile, st_tile), (ball, st_ball), (off, st_off) = res["tile"], res["ball"], res["exit-off"]
    for key in tile:
        assert torch.equal(tile[key], ball[key]) and torch.equal(tile[key], off[key]), key
        assert bool(torch.isfinite(tile[key]).all()), key
    print(name, "tile", st_tile, "ball", st_ball, "bytes set", int(res["bytes"].sum()), "of", len(res["bytes"]))
    blocks = (views * w * h + 255) // 256
    assert st_tile["waves"] == st_ball["waves"] == st_off["waves"] == 4 * blocks
    tiled = w % 16 == 0 and h % 16 == 0  # a launch in row order takes no tile proof: no bytes
    assert len(res["bytes"]) == (4 * blocks if tiled else 0) and set(np.unique(res["bytes"])) <= {0, 1}
    assert st_tile["steps_saved"] >= st_ball["steps_saved"]
    assert st_tile["waves_exited"] >= st_ball["waves_exited"]
    assert st_off["waves_exited"] == 0


@pytest.mark.parametrize("name", ["gap", "two-record-blocks"])
def test_the_cone_proves_strictly_more_than_the_soft_ball(runs, monkeypatch, name):
    """test_tile_proof_reference.test_counts_on_the_gpu_views: 50 waves against 0, and 55 against 49. The counter
    that can tell is steps_saved: waves_exited counts a wave whichever exit stops it, and a wave the proof takes
    is one the march's own escape exit would have stopped some steps later."""
    res = runs(name, monkeypatch)[0]
    assert res["tile"][1]["steps_saved"] > res["ball"][1]["steps_saved"]
    assert int(res["bytes"].sum()) > 0


def test_row_order_keeps_the_per_ray_lattice_proof(runs, monkeypatch):
    """40x40 is no multiple of the 16x16 tile: the call marches in row order, its launch takes no tile proof (no
    bytes) and reads the lattice per ray inside bound_proof instead, as every call with the lattice did before the
    tile proof. test_tile_proof_reference.test_rows_order_view_is_not_vacuous: the per-ray lattice proof takes
    waves of this view in row order and the soft ball none, so steps_saved tells them apart."""
    res = runs("rows-40x40", monkeypatch)[0]
    assert len(res["bytes"]) == 0
    assert res["tile"][1]["steps_saved"] > res["ball"][1]["steps_saved"]


def test_bytes_are_the_cpu_models(oracle, runs, monkeypatch):
    """the gap view, 48x80: byte w belongs to wave w & 3 of block w >> 2, the 8x8 quadrant (w & 1, (w >> 1) & 1) of
    16x16 tile w >> 2 in row order of the tiles"""
    res, views, w, h, S = runs("gap", monkeypatch)
    scd, cams, _, _, k = CASES["gap"]()
    want = model_bytes(oracle, scd, cams[0], w, h, S, k)[0]
    got = res["bytes"]
    wv = np.arange(len(got))
    tile, qd = wv >> 2, wv & 3
    ty, tx = tile // (w // 16), tile % (w // 16)
    in_rows = (2 * ty + (qd >> 1)) * (w // 8) + 2 * tx + (qd & 1)  # the tile's index in wave_tiles(w, h)
    assert 0 < want.sum() < len(want)
    assert np.array_equal(got.astype(bool), want[in_rows])


def test_graph_replay_rebuilds_the_bytes(mods, monkeypatch):
    """Two calls on two scenes captured in one graph and replayed twice, the scenes moved in place before every
    run: the replays give the eager runs' bits, so each call's lattice AND its tile bytes are made inside the
    replay from the scene as it then is (the gap's clusters move into the gap: bytes kept from the capture would
    stop waves whose pixels now show)."""
    torch, model, render, _ = mods
    monkeypatch.setenv("RM_PROOF_LATTICE", "1")
    w, h, S, k = 64, 64, 32, 32.0
    cams = [GAP_CAM]
    s = torch.cuda.Stream()
    results = {}
    with torch.cuda.stream(s):
        ctx = render.context()
        for mode in ("eager", "graph"):
            # the gap scene last: the bytes read back after a run are its call's
            scenes = [model.scene_tensors(outlier_scene(128), "cuda"), model.scene_tensors(gap_scene(128), "cuda")]
            tgt = torch.full((w * h, 3), 0.25, device="cuda")
            bufs = [torch.zeros(model.packed_size(128) + 1, device="cuda") for _ in scenes]
            outs = [torch.empty_like(tgt) for _ in scenes]

            def step():
                for sc, buf, out in zip(scenes, bufs, outs):
                    render.train_step_camera(cams, w, h, tgt, sc, k, 0.5, S, grads_packed=buf[:-1], loss=buf[-1:],
                                             out=out, ctx=ctx)

            def move():
                scenes[0].centers.add_(0.15)
                scenes[1].centers[:, 0].mul_(0.5)

            step()  # every buffer allocated before the capture
            torch.cuda.synchronize()
            seq = []
            if mode == "graph":
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=s):
                    step()
            for _ in range(2):
                move()
                if mode == "graph":
                    g.replay()
                else:
                    step()
                torch.cuda.synchronize()
                seq.append([t.clone() for t in bufs + outs] + [torch.frombuffer(bytearray(ctx.tile_proof()), dtype=torch.uint8)])
            results[mode] = seq
    for run, (a, b) in enumerate(zip(results["eager"], results["graph"])):
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), (run, i)
    assert not torch.equal(results["eager"][0][2], results["eager"][1][2])  # the scenes did move
    assert not torch.equal(results["eager"][0][-1], results["eager"][1][-1])  # and the bytes with them
