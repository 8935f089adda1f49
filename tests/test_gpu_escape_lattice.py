"""The escape lattice of the camera-mode escape proof (bound_proof in rm_ray.h,
rm_lattice_kernel): the bound march steps by the larger of the soft ball and the call's lattice of
cell-centre soft-min values. Exact: the train step with the lattice, with the soft ball alone
(RM_PROOF_LATTICE=0) and with the exit off (RM_NO_EARLY_EXIT=1) gives the same bits, and the rm_stats
counters show what the lattice adds. The calls here are far below kLatticeMinRays, so the lattice is
switched on by RM_PROOF_LATTICE=1 (the policy test leaves it unset). RM_SMALL=0 / RM_SPLIT=0: the
general unsplit kernel, the proof's scope."""
import pytest

from conftest import gpu_available
from escape_ref import CASES, GAP_CAM, _train, gap_scene, outlier_scene, wave_tiles

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]


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
    """per case, computed once: the train step and its counters with the lattice, with the soft ball alone and
    with the exit off"""
    cache = {}

    def get(name, monkeypatch):
        if name not in cache:
            torch, model, _, _ = mods
            scd, cams, (w, h), S, k = CASES[name]()
            sc = model.scene_tensors(scd, "cuda")
            res = {}
            for mode, env in (("lattice", {"RM_PROOF_LATTICE": "1"}), ("ball", {"RM_PROOF_LATTICE": "0"}),
                              ("exit-off", {"RM_NO_EARLY_EXIT": "1", "RM_PROOF_LATTICE": "1"})):
                with monkeypatch.context() as mp:
                    for key, v in env.items():
                        mp.setenv(key, v)
                    res[mode] = _train(mods, sc, cams, w, h, S, k)
            cache[name] = (res, len(cams), w, h, S)
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(CASES))
def test_lattice_changes_no_bit_and_saves_no_less(mods, runs, monkeypatch, name):
    torch = mods[0]
    res, views, w, h, S = runs(name, monkeypatch)
    (lat, st_lat), (ball, st_ball), (off, st_off) = res["lattice"], res["ball"], res["exit-off"]
    for key in lat:
        assert torch.equal(lat[key], ball[key]) and torch.equal(lat[key], off[key]), key
        assert bool(torch.isfinite(lat[key]).all()), key
    print(name, "lattice", st_lat, "ball", st_ball)
    assert st_lat["waves"] == st_ball["waves"] == st_off["waves"] == views * w * h // 64
    assert st_lat["steps_saved"] >= st_ball["steps_saved"]
    assert st_lat["waves_exited"] >= st_ball["waves_exited"]
    assert st_off["waves_exited"] == 0


@pytest.mark.parametrize("name", ["gap", "gap-two-views"])
def test_gap_scene_saves_more_and_exits_no_wave_that_shows(mods, runs, monkeypatch, name):
    res, views, w, h, S = runs(name, monkeypatch)
    (lat, st_lat), (_, st_ball) = res["lattice"], res["ball"]
    assert st_lat["steps_saved"] > st_ball["steps_saved"]
    # a wave is an 8x8 pixel tile of a view; one that holds a non-zero pixel was not exited (an exited wave
    # writes zeros: the bits equal the exit-off run's, test above), so at most the all-zero waves exited
    shown = (lat["out"].abs().amax(1) > 0).view(views, w * h).cpu().numpy()
    waves_shown = sum(int(shown[v][wave_tiles(w, h)].any(1).sum()) for v in range(views))
    assert waves_shown > 0
    assert st_lat["waves_exited"] <= st_lat["waves"] - waves_shown


def test_two_record_blocks_lattice_proves_strictly_more(mods, runs, monkeypatch):
    """the 520-sphere case is not vacuous: the CPU model (escape_ref.waves_taken) takes 55 of
    this view's 60 waves with the lattice and 49 with the soft ball alone, so a kernel that read the lattice
    geometry from the wrong offset cannot pass by proving nothing"""
    res = runs("two-record-blocks", monkeypatch)[0]
    st_lat, st_ball = res["lattice"][1], res["ball"][1]
    assert st_lat["steps_saved"] > st_ball["steps_saved"]


def test_inside_the_cloud_the_counters_are_the_soft_balls(mods, runs, monkeypatch):
    res = runs("inside-cloud", monkeypatch)[0]
    st_lat, st_ball = res["lattice"][1], res["ball"][1]
    assert (st_lat["waves_exited"], st_lat["steps_saved"]) == (st_ball["waves_exited"], st_ball["steps_saved"])


def test_policy_keeps_small_calls_on_the_soft_ball(mods, runs, monkeypatch):
    """a call below kLatticeMinRays, taken through the policy with no switch set, reports the soft ball's
    counters (and the lattice's differ on this scene, so the comparison can tell)"""
    _, model, _, _ = mods
    res = runs("gap", monkeypatch)[0]
    scd, cams, (w, h), S, k = CASES["gap"]()
    got, st = _train(mods, model.scene_tensors(scd, "cuda"), cams, w, h, S, k)
    assert st == res["ball"][1]
    assert st["steps_saved"] < res["lattice"][1]["steps_saved"]
    for key in got:
        assert mods[0].equal(got[key], res["ball"][0][key]), key


def test_graph_replay_rebuilds_the_lattice(mods, monkeypatch):
    """Two calls on two scenes captured in one graph and replayed twice, the scenes moved in place before
    every run: the replays give the eager runs' bits, so each call's lattice is built inside the replay from
    the scene as it then is. The gap scene's clusters move into the gap: a lattice kept from the capture, or
    the other call's, would still see the gap and prove waves whose pixels now show."""
    torch, model, render, _ = mods
    monkeypatch.setenv("RM_PROOF_LATTICE", "1")
    w, h, S, k = 64, 64, 32, 32.0
    cams = [GAP_CAM]
    s = torch.cuda.Stream()
    results = {}
    with torch.cuda.stream(s):
        ctx = render.context()
        for mode in ("eager", "graph"):
            scenes = [model.scene_tensors(gap_scene(128), "cuda"), model.scene_tensors(outlier_scene(128), "cuda")]
            tgt = torch.full((w * h, 3), 0.25, device="cuda")
            bufs = [torch.zeros(model.packed_size(128) + 1, device="cuda") for _ in scenes]
            outs = [torch.empty_like(tgt) for _ in scenes]

            def step():
                for sc, buf, out in zip(scenes, bufs, outs):
                    render.train_step_camera(cams, w, h, tgt, sc, k, 0.5, S, grads_packed=buf[:-1], loss=buf[-1:],
                                             out=out, ctx=ctx)

            def move():  # the gap's clusters move into the gap, the outlier scene drifts: other lattices every run
                scenes[0].centers[:, 0].mul_(0.5)
                scenes[1].centers.add_(0.15)

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
                seq.append([t.clone() for t in bufs + outs])
            torch.cuda.synchronize()
            results[mode] = seq
    for run, (a, b) in enumerate(zip(results["eager"], results["graph"])):
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), (run, i)
    # the runs differ from one another: the scenes did move
    assert not torch.equal(results["eager"][0][2], results["eager"][1][2])
