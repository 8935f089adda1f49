// librm_host.so, part 5: the scene's zero set as a triangle mesh -- marching tetrahedra on a lattice
// of distances (rmh_mesh_from_grid), the mesh accessors and the PLY writer. CPU only: no GPU call
// in this file (rmh_mesh_extract, which evaluates the lattice on the GPU, is in driver.cpp).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <unordered_map>

#include "rmh_common.hpp"

using namespace rmh;

namespace {

// The Kuhn decomposition of the unit cube: corner bits x = 1, y = 2, z = 4; the tetrahedron of the
// axis order (a, b, c) is {0, a, a + b, 7}, the monotone path 000 -> 111 taking the axes in that
// order. Its orientation det[v1 - v0, v2 - v0, v3 - v0] is the parity of (a, b, c): the odd ones
// are listed with v1 and v2 swapped, so every row is positively oriented.
constexpr int kTets[6][4] = {
    {0, 1, 3, 7},  // x y z
    {0, 5, 1, 7},  // x z y (swapped)
    {0, 3, 2, 7},  // y x z (swapped)
    {0, 2, 6, 7},  // y z x
    {0, 4, 5, 7},  // z x y
    {0, 6, 4, 7},  // z y x (swapped)
};

// parity of a permutation of {0, 1, 2, 3}: true = even
bool even4(const int p[4]) {
  int inv = 0;
  for (int i = 0; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j) inv += p[i] > p[j];
  return (inv & 1) == 0;
}

struct Extractor {
  const float* D;
  int64_t nx, ny, nz;
  float origin[3], spacing;
  rmh_mesh* mesh;
  std::unordered_map<uint64_t, int32_t> ids;  // edge key -> vertex (numbered at first use)
  bool overflow = false;

  // the lattice point's coordinate as rm_sdf_grid forms it: two roundings (this file is compiled
  // without fp contraction)
  float coord(int axis, int64_t i) const { return origin[axis] + (float)i * spacing; }

  // The vertex on the lattice edge between corners ca and cb (bit sets, one a subset of the other:
  // the two lie on one monotone path) of the cube at (x, y, z). The key is the edge's lower end
  // and its direction, so every cube and tetrahedron that meets the edge finds the same vertex.
  int32_t vertex(int64_t x, int64_t y, int64_t z, int ca, int cb) {
    if ((ca & cb) != ca) std::swap(ca, cb);  // ca: the lower end
    const int dir = ca ^ cb;                 // 1 .. 7
    const int64_t ax = x + (ca & 1), ay = y + ((ca >> 1) & 1), az = z + ((ca >> 2) & 1);
    const int64_t ia = (az * ny + ay) * nx + ax;
    const uint64_t key = (uint64_t)ia * 8u + (uint64_t)dir;
    const auto it = ids.find(key);
    if (it != ids.end()) return it->second;
    const int64_t bx = ax + (dir & 1), by = ay + ((dir >> 1) & 1), bz = az + ((dir >> 2) & 1);
    const double da = D[ia], db = D[(bz * ny + by) * nx + bx];
    double t = da / (da - db);
    if (!(t >= 0.0 && t <= 1.0)) t = 0.5;  // a non-finite distance
    const double pa[3] = {coord(0, ax), coord(1, ay), coord(2, az)};
    const double pb[3] = {coord(0, bx), coord(1, by), coord(2, bz)};
    const size_t n = mesh->vertices.size() / 3;
    if (n >= (size_t)INT32_MAX) {
      overflow = true;
      return 0;
    }
    for (int k = 0; k < 3; ++k) mesh->vertices.push_back((float)(pa[k] + t * (pb[k] - pa[k])));
    ids.emplace(key, (int32_t)n);
    return (int32_t)n;
  }

  void triangle(int32_t a, int32_t b, int32_t c) {
    mesh->faces.push_back(a);
    mesh->faces.push_back(b);
    mesh->faces.push_back(c);
  }

  // One positively oriented tetrahedron with corner bits c[4] and inside flags in[4]. For an even
  // permutation (a, b, c, d) of its vertices the triangle (e_ab, e_ac, e_ad) of the edges leaving a
  // has its normal pointing away from a, and the quad (e_ac, e_ad, e_bd, e_bc) between {a, b} and
  // {c, d} has its normal pointing towards c and d.
  void tet(int64_t x, int64_t y, int64_t z, const int c[4], const bool in[4]) {
    int ins[4], outs[4], ni = 0, no = 0;
    for (int i = 0; i < 4; ++i) {
      if (in[i]) ins[ni++] = i;
      else outs[no++] = i;
    }
    if (ni == 0 || ni == 4) return;
    auto e = [&](int i, int j) { return vertex(x, y, z, c[i], c[j]); };
    if (ni == 2) {
      int p[4] = {ins[0], ins[1], outs[0], outs[1]};
      if (!even4(p)) std::swap(p[2], p[3]);
      const int32_t q0 = e(p[0], p[2]), q1 = e(p[0], p[3]), q2 = e(p[1], p[3]), q3 = e(p[1], p[2]);
      triangle(q0, q1, q2);
      triangle(q0, q2, q3);
      return;
    }
    // one vertex apart from the other three: inside (normal away from it) or outside (towards it)
    const int a = ni == 1 ? ins[0] : outs[0];
    int p[4] = {a, 0, 0, 0};
    for (int i = 0, k = 1; i < 4; ++i)
      if (i != a) p[k++] = i;
    if (!even4(p)) std::swap(p[2], p[3]);
    const int32_t t0 = e(p[0], p[1]), t1 = e(p[0], p[2]), t2 = e(p[0], p[3]);
    if (ni == 1) triangle(t0, t1, t2);
    else triangle(t0, t2, t1);
  }

  void run() {
    for (int64_t z = 0; z + 1 < nz; ++z)
      for (int64_t y = 0; y + 1 < ny; ++y)
        for (int64_t x = 0; x + 1 < nx; ++x) {
          bool in8[8];
          int count = 0;
          for (int c = 0; c < 8; ++c) {
            in8[c] = D[((z + ((c >> 2) & 1)) * ny + (y + ((c >> 1) & 1))) * nx + (x + (c & 1))] < 0.0f;
            count += in8[c];
          }
          if (count == 0 || count == 8) continue;
          for (int t = 0; t < 6; ++t) {
            const bool in[4] = {in8[kTets[t][0]], in8[kTets[t][1]], in8[kTets[t][2]], in8[kTets[t][3]]};
            tet(x, y, z, kTets[t], in);
          }
        }
  }
};

// undirected edges that do not lie in exactly two triangles
int64_t count_open_edges(const std::vector<int32_t>& faces) {
  std::vector<uint64_t> edges;
  edges.reserve(faces.size());
  for (size_t f = 0; f + 2 < faces.size(); f += 3)
    for (int k = 0; k < 3; ++k) {
      const uint32_t a = (uint32_t)faces[f + k], b = (uint32_t)faces[f + (k + 1) % 3];
      edges.push_back(((uint64_t)std::min(a, b) << 32) | std::max(a, b));
    }
  std::sort(edges.begin(), edges.end());
  int64_t open = 0;
  for (size_t i = 0; i < edges.size();) {
    size_t j = i;
    while (j < edges.size() && edges[j] == edges[i]) ++j;
    if (j - i != 2) ++open;
    i = j;
  }
  return open;
}

// the piecewise sRGB encode of rm_view's RGBA8 output, rounded to nearest (NaN -> 0)
uint8_t srgb8(float c) {
  c = c > 0.0f ? (c < 1.0f ? c : 1.0f) : 0.0f;
  const float e = c < 0.0031308f ? 12.92f * c : 1.055f * std::pow(c, 1.0f / 2.4f) - 0.055f;
  return (uint8_t)(int)(e * 255.0f + 0.5f);
}

}  // namespace

extern "C" {

int rmh_mesh_from_grid(const float* dist, int32_t nx, int32_t ny, int32_t nz, const float origin[3], float spacing,
                       rmh_mesh** out) {
  if (!out) return fail(RMH_ERR_INVALID_ARG, "out is NULL");
  *out = nullptr;
  if (!dist || !origin) return fail(RMH_ERR_INVALID_ARG, "dist / origin is NULL");
  if (nx < 2 || ny < 2 || nz < 2) return fail(RMH_ERR_INVALID_ARG, "grid %dx%dx%d: every extent must be >= 2", nx, ny, nz);
  if (!(spacing > 0.0f) || !std::isfinite(spacing)) return fail(RMH_ERR_INVALID_ARG, "spacing must be finite and > 0");
  if ((int64_t)nx * ny > (INT64_C(1) << 58) / nz) return fail(RMH_ERR_INVALID_ARG, "grid too large");
  std::unique_ptr<rmh_mesh> mesh(new rmh_mesh());
  Extractor ex;
  ex.D = dist;
  ex.nx = nx;
  ex.ny = ny;
  ex.nz = nz;
  for (int k = 0; k < 3; ++k) ex.origin[k] = origin[k];
  ex.spacing = spacing;
  ex.mesh = mesh.get();
  ex.run();
  if (ex.overflow) return fail(RMH_ERR_INVALID_ARG, "the mesh has more than 2^31 - 1 vertices");
  mesh->open_edges = count_open_edges(mesh->faces);
  *out = mesh.release();
  return RMH_OK;
}

void rmh_mesh_counts(const rmh_mesh* mesh, int64_t* vertices, int64_t* faces, int64_t* open_edges) {
  if (vertices) *vertices = mesh ? (int64_t)(mesh->vertices.size() / 3) : 0;
  if (faces) *faces = mesh ? (int64_t)(mesh->faces.size() / 3) : 0;
  if (open_edges) *open_edges = mesh ? mesh->open_edges : 0;
}

const float* rmh_mesh_vertices(const rmh_mesh* mesh) { return mesh && !mesh->vertices.empty() ? mesh->vertices.data() : nullptr; }
const float* rmh_mesh_normals(const rmh_mesh* mesh) { return mesh && !mesh->normals.empty() ? mesh->normals.data() : nullptr; }
const float* rmh_mesh_colors(const rmh_mesh* mesh) { return mesh && !mesh->colors.empty() ? mesh->colors.data() : nullptr; }
const int32_t* rmh_mesh_faces(const rmh_mesh* mesh) { return mesh && !mesh->faces.empty() ? mesh->faces.data() : nullptr; }

void rmh_mesh_timing(const rmh_mesh* mesh, double ms[4]) {
  if (!ms) return;
  for (int k = 0; k < 4; ++k) ms[k] = mesh ? mesh->ms[k] : 0.0;
}

void rmh_mesh_free(rmh_mesh* mesh) { delete mesh; }

int rmh_mesh_write_ply(const rmh_mesh* mesh, const char* path) {
  if (!mesh || !path) return fail(RMH_ERR_INVALID_ARG, "mesh / path is NULL");
  const size_t V = mesh->vertices.size() / 3, F = mesh->faces.size() / 3;
  const bool has_n = mesh->normals.size() == 3 * V && V > 0, has_c = mesh->colors.size() == 3 * V && V > 0;
  char header[512];
  const int hl = std::snprintf(header, sizeof header,
                               "ply\nformat binary_little_endian 1.0\ncomment burn_raymarching_amd mesh\n"
                               "element vertex %zu\nproperty float x\nproperty float y\nproperty float z\n"
                               "property float nx\nproperty float ny\nproperty float nz\n"
                               "property uchar red\nproperty uchar green\nproperty uchar blue\n"
                               "element face %zu\nproperty list uchar int vertex_indices\nend_header\n",
                               V, F);
  std::string data(header, (size_t)hl);
  data.resize((size_t)hl + 27 * V + 13 * F);
  char* w = &data[(size_t)hl];
  for (size_t v = 0; v < V; ++v) {
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    std::memcpy(w, &mesh->vertices[3 * v], 12);
    std::memcpy(w + 12, has_n ? &mesh->normals[3 * v] : zero, 12);
    for (int k = 0; k < 3; ++k) w[24 + k] = (char)(has_c ? srgb8(mesh->colors[3 * v + k]) : 255);
    w += 27;
  }
  for (size_t f = 0; f < F; ++f) {
    *w = 3;
    std::memcpy(w + 1, &mesh->faces[3 * f], 12);
    w += 13;
  }
  if (!make_parent_dirs(path)) return fail(RMH_ERR_IO, "cannot create the directory of %s", path);
  if (!write_file(path, data)) return fail(RMH_ERR_IO, "cannot write %s", path);
  return RMH_OK;
}

}  // extern "C"
