// Internal helpers shared by the librm_host.so sources (include/rm_host.h is the API).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdarg>
#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "rm_host.h"

// The mesh behind rmh_mesh_* (mesh.cpp extracts it, driver.cpp's rmh_mesh_extract refines it and
// fills the normals and colours).
struct __attribute__((visibility("hidden"))) rmh_mesh {
  std::vector<float> vertices, normals, colors;  // [V][3] each; normals / colors may be empty
  std::vector<int32_t> faces;                    // [F][3]
  int64_t open_edges = 0;
  double ms[4] = {0.0, 0.0, 0.0, 0.0};  // rmh_mesh_timing
};

namespace rmh {

// Records the error text for rmh_last_error() and returns `code`.
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

bool read_file(const std::string& path, std::string& out);
bool write_file(const std::string& path, const std::string& data);
bool make_parent_dirs(const std::string& path);
bool make_dirs(const std::string& dir);
std::string dirname_of(const std::string& path);
std::string join_path(const std::string& dir, const std::string& name);

// ---- minimal JSON (RFC 8259 subset: no \u surrogate pairs beyond the BMP) ----------------
struct Json {
  enum Kind { Null, Bool, Number, String, Array, Object } kind = Null;
  bool b = false;
  double num = 0.0;
  std::string str;
  std::vector<Json> arr;
  std::vector<std::pair<std::string, Json>> obj;  // insertion order kept

  const Json* get(const std::string& key) const;
};
// Parses `text`; on error returns false and sets `err`.
bool json_parse(const std::string& text, Json& out, std::string& err);

// serde_json / ryu formatting of an f32 (shortest round trip, "1.0" for integral values).
std::string fmt_f32(float x);

// sigmoid / softplus(beta = 1) in f32, scene.rs:41-45 (softplus without the +0.01).
float sigmoid_f32(float x);
float softplus_f32(float x);

// ---- HIP plumbing of the sources that drive the GPU ----------------------------------------
// Returns fail(RMH_ERR_GPU, "<call>: <HIP error>") from the enclosing function when `call` fails.
#define HIPCHK(call)                                                                                  \
  do {                                                                                                \
    hipError_t e_ = (call);                                                                           \
    if (e_ != hipSuccess) return rmh::fail(RMH_ERR_GPU, "%s: %s", #call, hipGetErrorString(e_));      \
  } while (0)

// Page-locked host memory (the loss readback: an async copy the stream wait then covers)
struct __attribute__((visibility("hidden"))) PinnedBuf {
  void* p = nullptr;
  ~PinnedBuf() {
    if (p) (void)hipHostFree(p);
  }
  hipError_t alloc(size_t n) { return hipHostMalloc(&p, n, hipHostMallocDefault); }
  float* f() const { return (float*)p; }
};

// Device buffer owned by the host driver. (Both hidden: librm_host.so exports no C++ type of its own.)
struct __attribute__((visibility("hidden"))) DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  hipError_t alloc(size_t n) {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = n;
    return hipMalloc(&p, n ? n : 4);
  }
  float* f() const { return (float*)p; }
  int32_t* i() const { return (int32_t*)p; }
};

}  // namespace rmh
