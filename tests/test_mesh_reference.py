"""CPU tests of the mesh extraction (rmh_mesh_from_grid, the accessors, rmh_mesh_write_ply) on
lattices of the fp64 restatement's distances cast to float32 (tests/sdf_ref.py). No GPU call.

What a correct marching-tetrahedra extraction on the Kuhn decomposition must give, whatever the
field: every undirected edge in exactly two triangles, once in each direction (closed, consistently
wound), unless the surface leaves the grid; the Euler characteristic and component count of the
surface; outward normals; vertices on lattice edges whose ends straddle zero. The bounds are
derived, not measured:
  * one sphere, D = rho - r exact: along a lattice edge of length <= L = sqrt(3) spacing the second
    derivative of D is at most 1 / rho, so linear interpolation misplaces the zero by at most
    b = L^2 / (8 (r - L)) radially (0.00374 at spacing 1/16, r = 0.5; a numpy prototype of the same
    algorithm measured 0.00293), and the enclosed volume lies between the balls of radius r - 2b and
    r + b (prototype 0.5195 in [0.5004, 0.5355]);
  * any scene: D is 1-Lipschitz and a vertex lies on an edge of length <= L whose ends have D of
    opposite sign, so |D(v)| <= L / 2 (prototype 0.0040 against 0.027 on scene.json at 1/32)."""
import os

import numpy as np
import pytest

import sdf_ref as S
from conftest import final1_scene

ONE_C = np.array([0.01, 0.02, -0.03], np.float32)
ONE = {"centers": ONE_C.reshape(1, 3), "colors": np.array([[0.8, 0.3, 0.2]], np.float32),
       "radius": np.array([0.5], np.float32)}
TWO = {"centers": np.array([[-0.5, 0, 0], [0.5, 0, 0]], np.float32), "colors": np.eye(3, dtype=np.float32)[:2],
       "radius": np.array([0.3, 0.3], np.float32)}
K = 32.0


@pytest.fixture(scope="module")
def host():
    from burn_raymarching_amd import _build
    _build.build_host()
    from burn_raymarching_amd import host as h
    return h


_GRIDS = {}


def grid_of(name):
    """(dist [nz,ny,nx] float32, origin, spacing), computed once."""
    if name not in _GRIDS:
        if name == "one":
            spec = (ONE, (-0.987,) * 3, 1.0 / 16.0, (33, 33, 33))
        elif name == "half":  # the same lattice from its 17th x plane on: cuts the sphere in half
            spec = (ONE, (-0.987 + 1.0, -0.987, -0.987), 1.0 / 16.0, (17, 33, 33))
        elif name == "two":
            spec = (TWO, (-1.0,) * 3, 0.05, (41, 41, 41))
        else:
            spec = (final1_scene(), (-0.75,) * 3, 1.0 / 32.0, (49, 49, 49))
        sc, origin, spacing, shape = spec
        d = S.grid(sc, K, origin, spacing, shape)
        d.setflags(write=False)
        _GRIDS[name] = (d, origin, spacing, sc)
    return _GRIDS[name]


def extract(host, name):
    d, origin, spacing, sc = grid_of(name)
    return host.mesh_from_grid(d, origin, spacing), spacing, sc


def assert_closed(rep, mesh):
    assert rep["open_edges"] == 0 and mesh.open_edges == 0, rep
    assert rep["edge_counts"] == {2: rep["E"]} and rep["unpaired"] == 0 and rep["unused"] == 0, rep


def test_one_sphere(host):
    mesh, spacing, _ = extract(host, "one")
    rep = S.mesh_report(mesh.vertices, mesh.faces)
    print("one sphere:", rep)
    assert_closed(rep, mesh)
    assert rep["euler"] == 2 and rep["components"] == 1, rep
    v = mesh.vertices.astype(np.float64)
    c = ONE_C.astype(np.float64)
    tri = v[mesh.faces]
    normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    outward = np.einsum("ij,ij->i", normal, tri.mean(1) - c)
    assert (outward > 0).all(), int((outward <= 0).sum())
    r, L = 0.5, np.sqrt(3.0) * spacing
    b = L * L / (8.0 * (r - L))
    radial = np.abs(np.linalg.norm(v - c, axis=1) - r).max()
    print(f"one sphere: max | |v - c| - r | = {radial:.5f}, bound {b:.5f}; volume {rep['volume']:.4f}")
    assert radial <= b, (radial, b)
    ball = lambda x: 4.0 / 3.0 * np.pi * x ** 3
    assert ball(r - 2 * b) <= rep["volume"] <= ball(r + b), (rep["volume"], ball(r - 2 * b), ball(r + b))
    assert mesh.normals is None and mesh.colors is None


def test_two_disjoint_spheres(host):
    mesh, _, _ = extract(host, "two")
    rep = S.mesh_report(mesh.vertices, mesh.faces)
    print("two spheres:", rep)
    assert_closed(rep, mesh)
    assert rep["components"] == 2 and rep["euler"] == 4, rep
    assert rep["volume"] > 0


def test_golden_scene(host):
    mesh, spacing, sc = extract(host, "golden")
    rep = S.mesh_report(mesh.vertices, mesh.faces)
    print("scene.json:", rep)
    assert_closed(rep, mesh)
    assert rep["components"] == 1 and rep["euler"] == 2, rep
    dmax = np.abs(S.distance(mesh.vertices, sc, K)).max()
    L = np.sqrt(3.0) * spacing
    print(f"scene.json: max |D_fp64(v)| = {dmax:.5f}, bound L/2 = {L / 2:.5f}")
    assert dmax <= L / 2, (dmax, L / 2)


def test_surface_leaving_the_grid(host):
    mesh, _, _ = extract(host, "half")
    rep = S.mesh_report(mesh.vertices, mesh.faces)
    print("half sphere:", rep)
    assert rep["F"] > 0 and mesh.open_edges > 0 and mesh.open_edges == rep["open_edges"], rep
    # the rim edges lie in one triangle, every other edge in two, once in each direction
    assert set(rep["edge_counts"]) == {1, 2} and rep["unpaired"] == 0 and rep["components"] == 1, rep


def test_degenerate_grids(host):
    for value in (1.0, -1.0):
        m = host.mesh_from_grid(np.full((5, 4, 3), value, np.float32), (0, 0, 0), 0.5)
        assert m.vertices.shape == (0, 3) and m.faces.shape == (0, 3) and m.open_edges == 0
    for corner in range(8):
        d = np.ones((2, 2, 2), np.float32)
        d[(corner >> 2) & 1, (corner >> 1) & 1, corner & 1] = -1.0
        m = host.mesh_from_grid(d, (0, 0, 0), 1.0)
        rep = S.mesh_report(m.vertices, m.faces)  # asserts every index in range
        assert rep["F"] >= 1 and rep["unused"] == 0 and rep["components"] == 1, (corner, rep)
        assert (m.vertices >= 0).all() and (m.vertices <= 1).all()
        if corner in (0, 7):  # on all six tetrahedra: the fan of six triangles about the corner
            assert rep["F"] == 6 and rep["V"] == 7 and rep["edge_counts"] == {1: 6, 2: 6}, (corner, rep)
    with pytest.raises(host.HostError):
        host.mesh_from_grid(np.ones((1, 2, 2), np.float32), (0, 0, 0), 1.0)
    with pytest.raises(host.HostError):
        host.mesh_from_grid(np.ones((2, 2, 2), np.float32), (0, 0, 0), 0.0)


def test_deterministic(host):
    a, _, _ = extract(host, "golden")
    b, _, _ = extract(host, "golden")
    assert a.vertices.tobytes() == b.vertices.tobytes() and a.faces.tobytes() == b.faces.tobytes()
    # vertices are numbered at first use: face 0 uses vertices 0, 1, 2, and the first face that
    # uses a vertex never precedes the first face of a lower-numbered vertex
    assert sorted(a.faces[0].tolist()) == [0, 1, 2]
    first = np.full(len(a.vertices), -1, np.int64)
    flat = a.faces.reshape(-1)
    first[flat[::-1]] = np.arange(flat.size)[::-1] // 3
    assert (np.diff(first) >= 0).all()


def test_ply_round_trip(host, tmp_path):
    mesh, _, _ = extract(host, "one")
    path = os.path.join(tmp_path, "sub", "one.ply")
    host.mesh_write_ply(mesh, path)
    end, verts, faces = S.parse_ply(path)  # checks the header's properties and the file size
    V, F = len(mesh.vertices), len(mesh.faces)
    assert len(verts) == V and len(faces) == F
    assert os.path.getsize(path) == end + 27 * V + 13 * F
    xyz = np.stack([verts["x"], verts["y"], verts["z"]], 1)
    assert xyz.tobytes() == mesh.vertices.tobytes()
    assert (faces["n"] == 3).all() and np.array_equal(faces["v"], mesh.faces)
    # a mesh without normals / colours: zero normals, white
    assert not verts["nx"].any() and not verts["ny"].any() and not verts["nz"].any()
    assert (verts["red"] == 255).all() and (verts["green"] == 255).all() and (verts["blue"] == 255).all()

