"""Restatements for the distance-field query (rm_sdf_query / rm_sdf_grid) and the mesh extraction
(rmh_mesh_from_grid / rmh_mesh_extract): TEST INFRASTRUCTURE ONLY.

The field comes from oracle.autodiff_ref as it is: scene_sdf_value (scene.rs:60-79), its torch
autograd gradient (the clamp_min of scene.rs:72 has a zero Jacobian under the clamp, so a sphere
whose centre the point sits on contributes no term) and the colour blend of renderer_diff.rs:64-80
with burn_softmax. Every function takes a dtype: float64 is the anchor, float32 the run of the same
restatement whose own error sets the GPU bounds.

The mesh checker is pure Python / numpy: undirected-edge counts, directed-edge pairing, Euler
characteristic, components by union-find, signed volume."""
import numpy as np
import torch

from oracle import autodiff_ref as A


def _t(x, dtype):
    return torch.from_numpy(np.array(x, dtype=np.float32)).to(dtype)


def field(points, scene, k, csharp=10.0, dtype=torch.float64):
    """(D [N], grad D [N,3], colour [N,3]) of the restatement at points (float32 values), in dtype."""
    p = _t(points, dtype).reshape(-1, 3).clone().requires_grad_(True)
    c, col = _t(scene["centers"], dtype), _t(scene["colors"], dtype)
    r = _t(scene["radius"], dtype).reshape(-1, 1)
    d = A.scene_sdf_value(p, c, r, float(k))
    (g,) = torch.autograd.grad(d.sum(), p)
    with torch.no_grad():
        pd = p.detach()
        q = pd.pow(2).sum(1, keepdim=True) + c.pow(2).sum(1, keepdim=True).t() - (pd @ c.t()) * 2.0
        dists = q.clamp_min(1e-6).sqrt() - r.t()
        w = A.burn_softmax(dists * (-A._f32(csharp)), 1)
        mixed = (col.unsqueeze(0) * w.unsqueeze(2)).sum(1)
    return (d.detach().reshape(-1).double().numpy(), g.double().numpy(), mixed.double().numpy())


def distance(points, scene, k, dtype=torch.float64, chunk=1 << 16):
    """D alone, chunked (grids)."""
    c = _t(scene["centers"], dtype)
    r = _t(scene["radius"], dtype).reshape(-1, 1)
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    out = np.empty(pts.shape[0], np.float64)
    with torch.no_grad():
        for i in range(0, pts.shape[0], chunk):
            out[i:i + chunk] = A.scene_sdf_value(_t(pts[i:i + chunk], dtype), c, r, float(k)).reshape(-1).double().numpy()
    return out


def lattice(origin, spacing, shape):
    """The float32 lattice points of rm_sdf_grid / rmh_mesh_from_grid, [nz, ny, nx, 3]: per axis
    origin + float32(i) * spacing with the two roundings of the stated formula."""
    nx, ny, nz = shape
    o = np.asarray(origin, np.float32)
    s = np.float32(spacing)
    ax = [(o[k] + (np.arange(n, dtype=np.float32) * s).astype(np.float32)).astype(np.float32)
          for k, n in enumerate((nx, ny, nz))]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x, y, z], axis=-1).astype(np.float32)


def grid(scene, k, origin, spacing, shape):
    """The fp64 restatement's D on the lattice, cast to float32: [nz, ny, nx]."""
    pts = lattice(origin, spacing, shape)
    return distance(pts.reshape(-1, 3), scene, k).reshape(pts.shape[:3]).astype(np.float32)


# ---- mesh invariants ---------------------------------------------------------------------------
def mesh_report(vertices, faces):
    """Invariants of a triangle mesh. vertices [V,3], faces [F,3] (indices must be in range).
      V, E, F, euler = V - E + F
      edge_counts     {k: undirected edges lying in exactly k triangles}
      open_edges      undirected edges not in exactly two triangles
      unpaired        undirected edges in exactly two triangles that are not once in each direction
      components      connected components of the vertices that faces use (union-find)
      unused          vertices no face uses
      volume          signed volume sum det[v0, v1, v2] / 6 (positive: normals point outward)"""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    nv = v.shape[0]
    assert f.size == 0 or (f.min() >= 0 and f.max() < nv), "face index out of range"
    directed = {}
    for a, b, c in f.tolist():
        for e in ((a, b), (b, c), (c, a)):
            directed[e] = directed.get(e, 0) + 1
    undirected = {}
    for (a, b), n in directed.items():
        key = (a, b) if a < b else (b, a)
        undirected[key] = undirected.get(key, 0) + n
    counts = {}
    for n in undirected.values():
        counts[n] = counts.get(n, 0) + 1
    unpaired = sum(1 for (a, b), n in undirected.items()
                   if n == 2 and not (directed.get((a, b), 0) == 1 and directed.get((b, a), 0) == 1))
    parent = list(range(nv))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in undirected:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
    used = set(f.reshape(-1).tolist())
    comps = len({find(x) for x in used})
    vol = float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0) if f.size else 0.0
    e = len(undirected)
    return {"V": nv, "E": e, "F": f.shape[0], "euler": nv - e + f.shape[0], "edge_counts": counts,
            "open_edges": sum(n for k, n in counts.items() if k != 2), "unpaired": unpaired, "components": comps,
            "unused": nv - len(used), "volume": vol}


def parse_ply(path):
    """The binary little-endian PLY of rmh_mesh_write_ply: (header bytes, vertex records, face records)."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode("ascii").split("\n")
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0"
    nv = int([ln for ln in head if ln.startswith("element vertex")][0].split()[2])
    nf = int([ln for ln in head if ln.startswith("element face")][0].split()[2])
    props = [ln.split()[1:] for ln in head if ln.startswith("property")]
    vt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                   ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    ft = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    assert [p[-1] for p in props[:9]] == list(vt.names) and props[9] == ["list", "uchar", "int", "vertex_indices"]
    assert vt.itemsize == 27 and ft.itemsize == 13
    assert len(raw) == end + 27 * nv + 13 * nf, (len(raw), end, nv, nf)
    verts = np.frombuffer(raw, vt, nv, end)
    faces = np.frombuffer(raw, ft, nf, end + 27 * nv)
    return end, verts, faces


def srgb8(c):
    """The piecewise sRGB encode of rm_view's RGBA8 output, rounded to nearest."""
    c = np.clip(np.asarray(c, np.float64), 0.0, 1.0)
    e = np.where(c < 0.0031308, 12.92 * c, 1.055 * np.power(c, 1.0 / 2.4) - 0.055)
    return np.floor(e * 255.0 + 0.5).astype(np.uint8)
