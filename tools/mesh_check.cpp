// mesh_check: a stand-alone host program over csrc/host/mesh.cpp for sanitizer builds (no GPU, no
// Python): one sphere on a 33^3 lattice (closed, V - E + F = 2, the PLY written and its size
// checked), the same sphere cut in half by the grid (open edges), and the degenerate grids
// (all-outside, all-inside, 2x2x2 with one inside corner, bad arguments). Build and run, e.g.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off \
//     -D__HIP_PLATFORM_AMD__ -I include -I /opt/rocm/include -I burn_raymarching_amd/csrc/host \
//     tools/mesh_check.cpp burn_raymarching_amd/csrc/host/mesh.cpp burn_raymarching_amd/csrc/host/io.cpp \
//     -lz -o /tmp/mesh_check && /tmp/mesh_check /tmp/mesh_check.ply
// Prints one line per case and "mesh_check: OK"; exits 1 at the first failed check.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

#include "rm_host.h"

namespace {

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "mesh_check: %s failed (line %d): %s\n", #cond, __LINE__, rmh_last_error()); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

std::vector<float> sphere_grid(int nx, int ny, int nz, const float origin[3], float spacing) {
  const double c[3] = {0.01, 0.02, -0.03}, r = 0.5;
  std::vector<float> d((size_t)nx * ny * nz);
  for (int z = 0; z < nz; ++z)
    for (int y = 0; y < ny; ++y)
      for (int x = 0; x < nx; ++x) {
        const double p[3] = {origin[0] + (float)x * spacing, origin[1] + (float)y * spacing, origin[2] + (float)z * spacing};
        d[((size_t)z * ny + y) * nx + x] =
            (float)(std::sqrt((p[0] - c[0]) * (p[0] - c[0]) + (p[1] - c[1]) * (p[1] - c[1]) + (p[2] - c[2]) * (p[2] - c[2])) - r);
      }
  return d;
}

struct Counts {
  int64_t v, f, open, edges;
};

Counts counts_of(const rmh_mesh* m) {
  Counts c{};
  rmh_mesh_counts(m, &c.v, &c.f, &c.open);
  const int32_t* faces = rmh_mesh_faces(m);
  std::set<std::pair<int32_t, int32_t>> edges;
  for (int64_t f = 0; f < c.f; ++f)
    for (int k = 0; k < 3; ++k) {
      const int32_t a = faces[3 * f + k], b = faces[3 * f + (k + 1) % 3];
      CHECK(a >= 0 && a < c.v && b >= 0 && b < c.v);
      edges.insert({a < b ? a : b, a < b ? b : a});
    }
  c.edges = (int64_t)edges.size();
  return c;
}

}  // namespace

int main(int argc, char** argv) {
  const char* ply = argc > 1 ? argv[1] : "mesh_check.ply";
  rmh_mesh* m = nullptr;
  {  // one sphere
    const float origin[3] = {-0.987f, -0.987f, -0.987f};
    const std::vector<float> d = sphere_grid(33, 33, 33, origin, 1.0f / 16.0f);
    CHECK(rmh_mesh_from_grid(d.data(), 33, 33, 33, origin, 1.0f / 16.0f, &m) == RMH_OK);
    const Counts c = counts_of(m);
    std::printf("one sphere: %lld vertices, %lld faces, %lld edges, %lld open\n", (long long)c.v, (long long)c.f,
                (long long)c.edges, (long long)c.open);
    CHECK(c.open == 0 && c.v - c.edges + c.f == 2);
    CHECK(rmh_mesh_normals(m) == nullptr && rmh_mesh_colors(m) == nullptr);
    double r_err = 0.0;
    const float* v = rmh_mesh_vertices(m);
    for (int64_t i = 0; i < c.v; ++i)
      r_err = std::fmax(r_err, std::fabs(std::sqrt((v[3 * i] - 0.01) * (v[3 * i] - 0.01) + (v[3 * i + 1] - 0.02) * (v[3 * i + 1] - 0.02) +
                                                   (v[3 * i + 2] + 0.03) * (v[3 * i + 2] + 0.03)) - 0.5));
    CHECK(r_err <= 0.00374);
    CHECK(rmh_mesh_write_ply(m, ply) == RMH_OK);
    std::FILE* f = std::fopen(ply, "rb");
    CHECK(f != nullptr);
    std::fseek(f, 0, SEEK_END);
    const long size = std::ftell(f);
    std::fclose(f);
    CHECK(size > 27 * c.v + 13 * c.f && size < 27 * c.v + 13 * c.f + 512);
    rmh_mesh_free(m);
  }
  {  // the grid cuts the sphere in half
    const float origin[3] = {0.013f, -0.987f, -0.987f};
    const std::vector<float> d = sphere_grid(17, 33, 33, origin, 1.0f / 16.0f);
    CHECK(rmh_mesh_from_grid(d.data(), 17, 33, 33, origin, 1.0f / 16.0f, &m) == RMH_OK);
    const Counts c = counts_of(m);
    std::printf("half sphere: %lld vertices, %lld faces, %lld open\n", (long long)c.v, (long long)c.f, (long long)c.open);
    CHECK(c.open > 0 && c.f > 0);
    rmh_mesh_free(m);
  }
  {  // degenerate grids
    const float origin[3] = {0.0f, 0.0f, 0.0f};
    for (float value : {1.0f, -1.0f}) {
      const std::vector<float> d(5 * 4 * 3, value);
      CHECK(rmh_mesh_from_grid(d.data(), 3, 4, 5, origin, 0.5f, &m) == RMH_OK);
      const Counts c = counts_of(m);
      CHECK(c.v == 0 && c.f == 0 && c.open == 0 && rmh_mesh_vertices(m) == nullptr && rmh_mesh_faces(m) == nullptr);
      rmh_mesh_free(m);
    }
    for (int corner = 0; corner < 8; ++corner) {
      std::vector<float> d(8, 1.0f);
      d[corner] = -1.0f;
      CHECK(rmh_mesh_from_grid(d.data(), 2, 2, 2, origin, 1.0f, &m) == RMH_OK);
      const Counts c = counts_of(m);
      CHECK(c.f >= 1 && (corner != 0 && corner != 7 ? true : c.f == 6 && c.v == 7));
      rmh_mesh_free(m);
    }
    const std::vector<float> d(8, 1.0f);
    CHECK(rmh_mesh_from_grid(d.data(), 1, 2, 2, origin, 1.0f, &m) == RMH_ERR_INVALID_ARG && m == nullptr);
    CHECK(rmh_mesh_from_grid(d.data(), 2, 2, 2, origin, 0.0f, &m) == RMH_ERR_INVALID_ARG);
    CHECK(rmh_mesh_from_grid(nullptr, 2, 2, 2, origin, 1.0f, &m) == RMH_ERR_INVALID_ARG);
    rmh_mesh_free(nullptr);
    std::printf("degenerate grids: empty meshes, the six-triangle fan, refused arguments\n");
  }
  std::printf("mesh_check: OK\n");
  return 0;
}
