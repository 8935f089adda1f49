"""The additivity measure (tests/additivity_ref.py) tested without a GPU: on 12 rows of 256 rays
at 12 spheres from the fp64 oracle, rounded to fp32, every fp32 summation order passes it -- the
kernels' own (pass 1 / pass 2 of rm_reduce.h and small_final's chains, restated in numpy), the
reverse and random ones -- and every way a reduction loses, doubles, picks up or misplaces a row
fails it. The inputs carry a condition, not a tolerance: in at least one element every row
contributes at least 100 times the bound, so no row can vanish inside it."""
import numpy as np
import pytest

import additivity_ref as A

M, ROWS, RAYS, STEPS, K = 12, 12, 256, 8, 32.0


def _rays(oracle, model, seed):
    """Rays of ring views that look at the scene (closest approach to the origin < 0.6), shuffled."""
    o, d = [], []
    for c in model.ring_cameras(6, offset=seed % 3):
        oo, dd = oracle.camera_rays(64, 64, *c, precision="f32")
        o.append(oo)
        d.append(dd)
    o, d = np.concatenate(o), np.concatenate(d)
    miss = np.linalg.norm(np.cross(o.astype(np.float64), d.astype(np.float64)), axis=1)
    keep = np.flatnonzero(miss < 0.6)
    keep = keep[np.random.default_rng(seed).permutation(keep.size)]
    return o[keep], d[keep]


def _rows(oracle, model, scene_seed, ray_seed):
    sc = model.synthetic_scene(M, scene_seed)
    o, d = _rays(oracle, model, ray_seed)
    assert o.shape[0] >= ROWS * RAYS
    g = np.random.default_rng(100 + ray_seed).standard_normal((ROWS * RAYS, 3))
    rows = []
    for r in range(ROWS):
        s = slice(r * RAYS, (r + 1) * RAYS)
        gr = oracle.render_diff_backward(o[s].astype(np.float64), d[s].astype(np.float64), sc, STEPS, K, g[s])
        rows.append(A.record_row(gr, M))  # rounded to fp32, in the record's column layout
    return np.stack(rows)


@pytest.fixture(scope="module")
def data(oracle):
    from burn_raymarching_amd import model
    return _rows(oracle, model, 3, 1), _rows(oracle, model, 4, 2)


def test_input_condition_every_row_is_visible(data):
    """In at least one element every row contributes at least 100 times the bound."""
    P, _ = data
    assert np.all(np.any(P != 0.0, axis=1))
    bound = A.gamma(ROWS - 1) * np.abs(P.astype(np.float64)).sum(axis=0)
    visible = np.abs(P.astype(np.float64)).min(axis=0) >= 100.0 * bound
    assert visible[bound > 0].any(), "choose other rays: no element sees every row"


def test_gamma_and_single_row_is_bit_equality():
    assert A.gamma(0) == 0.0 and A.gamma(1) == A.U / (1 - A.U)
    v = np.array([1.0, -3.5, 0.0], np.float32)
    assert A.measure(v, v[None])[0]
    assert not A.measure(np.nextafter(v, np.float32(9), dtype=np.float32), v[None])[0]


def test_kernel_orders_pass(data):
    P, _ = data
    for name, G in (("general", A.general_order(P)), ("small", A.small_order(P, M)),
                    ("reverse", A.chain(P[::-1], P.shape[1]))):
        ok, ratio, n = A.measure(G, P)
        assert ok and n == ROWS and ratio <= 1.0, (name, ratio)
    # the orders are different trees: at least two of them differ in some bit
    assert not (np.array_equal(A.general_order(P), A.small_order(P, M)) and
                np.array_equal(A.general_order(P), A.chain(P[::-1], P.shape[1])))


def test_random_orders_pass(data):
    P, _ = data
    rng = np.random.default_rng(7)
    for _ in range(20):
        ok, ratio, _ = A.measure(A.chain(P[rng.permutation(ROWS)], P.shape[1]), P)
        assert ok, ratio


def test_restated_orders_at_their_edges():
    """The restatements themselves: segment layouts at the list's edges, dead rows skipped, the
    chain counts of small_final."""
    assert A.seg_layout(128) == (128, 1) and A.seg_layout(129) == (128, 2) and A.seg_layout(257) == (128, 3)
    assert A.seg_layout(32768) == (128, 256) and A.seg_layout(32769) == (192, 171)
    assert [A.small_chains(m) for m in (1, 4, 7, 9, 15, 16, 31, 32)] == [8, 6, 4, 3, 2, 1, 1, 1]
    rng = np.random.default_rng(0)
    P = rng.standard_normal((300, 24)).astype(np.float32)
    live = rng.random(300) < 0.5
    dead_poisoned = P.copy()
    dead_poisoned[~live] = 2.0 ** 40
    assert np.array_equal(A.general_order(dead_poisoned, live), A.general_order(np.where(live[:, None], P, 0)))
    assert A.measure(A.general_order(P), P)[0] and A.measure(A.small_order(P[:129], 2), P[:129])[0]


@pytest.mark.parametrize("order", ["general", "small"])
def test_mutants_fail(data, order):
    P, other = data
    red = (lambda X: A.general_order(X)) if order == "general" else (lambda X: A.small_order(X, M))
    assert A.measure(red(P), P)[0]
    # a row dropped, for every row in turn
    for r in range(ROWS):
        assert not A.measure(red(np.delete(P, r, axis=0)), P)[0], ("dropped", r)
    # a row added twice
    for r in (0, ROWS // 2, ROWS - 1):
        assert not A.measure(red(np.concatenate([P, P[r:r + 1]])), P)[0], ("doubled", r)
    # another scene's row (a stale row) added at weight 1
    assert not A.measure(red(np.concatenate([P, other[3:4]])), P)[0]
    # one row's columns shifted by one sphere
    Q = P.copy()
    Q[5, :M * 8] = np.roll(P[5, :M * 8].reshape(M, 8), 1, axis=0).reshape(-1)
    assert not A.measure(red(Q), P)[0]
    # one row's centre and colour columns exchanged
    Q = P.copy()
    body, src = Q[7, :M * 8].reshape(M, 8), P[7, :M * 8].reshape(M, 8)
    body[:, 0:3], body[:, 4:7] = src[:, 4:7], src[:, 0:3]
    assert not A.measure(red(Q), P)[0]
