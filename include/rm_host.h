/*
 * rm_host.h -- C ABI of librm_host.so: the host side of the reference's training and
 * target-generation programs, rebuilt in C++ over libraymarch_hip.so (include/raymarch.h).
 *
 * The reference's host code is Rust (no toolchain in this image); these entry points are
 * what its binaries do around the hot path:
 *   - util.rs:4-33          PNG save/load with the 2.2 gamma            -> rmh_image_*, rmh_png_*
 *   - camera.rs:30-90       create_camera_rays (host f32 loop)          -> rmh_camera_rays
 *   - train.rs:15-21, generate.rs:13-18, :107-109   cameras.json        -> rmh_cameras_*
 *   - train.rs:210-262      scene.json export                           -> rmh_scene_*
 *   - dataset.rs:4-82       SceneDataset fg/bg split + sample_batch     -> rmh_dataset_*
 *   - training.rs:87-238    prune_and_split                             -> rmh_prune_and_split
 *   - train.rs:23-330       the multi-stage training driver             -> rmh_train
 *   - train.rs:335-366      save_tiled_preview                          -> rmh_preview
 *   - generate.rs:20-112    the synthetic target generator              -> rmh_generate
 *
 * Everything except rmh_train / rmh_preview / rmh_generate is CPU-only. The reference's RNG
 * is unseeded (rand::rng(), dataset.rs:52, training.rs:93); here every random draw comes from
 * an explicit, seeded PCG32 stream (rmh_rng) so runs are reproducible.
 *
 * Return values: RMH_OK (0) or an RMH_ERR_* code; rmh_last_error() has the text (per thread).
 * Buffers returned through `**` out-parameters are malloc'd; release them with rmh_free().
 */
#ifndef RM_HOST_H_
#define RM_HOST_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RMH_OK 0
#define RMH_ERR_INVALID_ARG 1
#define RMH_ERR_IO 2
#define RMH_ERR_FORMAT 3
#define RMH_ERR_GPU 4

const char* rmh_last_error(void);
void rmh_free(void* p);
/* "burn_raymarching_amd host 0.1.0 src <16 hex>": the sha256 prefix of the host library's sources
 * (csrc/host/{io,data,driver,comm,mesh}.cpp, rmh_common.hpp, rm_host.h, raymarch.h), compiled in by
 * _build.py, so that a shipped librm_host.so names the tree it came from (rm_version() does the
 * same for libraymarch_hip.so). */
const char* rmh_version(void);

/* ---- util.rs: images ----------------------------------------------------------------- */
/* 8-bit PNG (grey, grey+alpha, RGB, RGBA, palette; non-interlaced) -> RGB8 [h][w][3]. */
int rmh_png_read(const char* path, int32_t* width, int32_t* height, uint8_t** rgb);
/* RGB8 -> PNG; creates missing parent directories (util.rs:14-18). */
int rmh_png_write(const char* path, const uint8_t* rgb, int32_t width, int32_t height);
/* util.rs:28-31: (x / 255) ^ 2.2 in f32. */
void rmh_srgb8_to_linear(const uint8_t* in, int64_t n, float* out);
/* util.rs:6-9: (x ^ (1/2.2)).clamp(0, 1) * 255 truncated to u8 (NaN -> 0). */
void rmh_linear_to_srgb8(const float* in, int64_t n, uint8_t* out);
/* load_image_as_tensor (util.rs:24-33): linear RGB [h*w][3]. */
int rmh_image_load(const char* path, int32_t* width, int32_t* height, float** linear_rgb);
/* save_tensor_as_image (util.rs:4-21) of a HOST buffer [h*w][3]. */
int rmh_image_save(const char* path, const float* linear_rgb, int32_t width, int32_t height);

/* ---- camera.rs:30-90 ----------------------------------------------------------------- */
/* org, dir: host [height*width][3], rows y then x (no half-pixel offset). */
void rmh_camera_rays(int32_t width, int32_t height, const float eye[3], const float target[3], float fov_deg,
                     float* org, float* dir);

/* ---- cameras.json: Vec<CameraConfig{file, origin, target, fov}> --------------------- */
#define RMH_PATH_MAX 512
typedef struct rmh_camera_entry {
  char file[RMH_PATH_MAX];
  float origin[3];
  float target[3];
  float fov;
} rmh_camera_entry;
int rmh_cameras_load(const char* path, rmh_camera_entry** cams, int32_t* count);
/* serde_json::to_writer_pretty layout (generate.rs:107-109). */
int rmh_cameras_save(const char* path, const rmh_camera_entry* cams, int32_t count);

/* ---- scene.json (train.rs:238-262): activated values, radius WITHOUT the +0.01 -------- */
int rmh_scene_save(const char* path, int32_t num_spheres, const float* centers, const float* colors,
                   const float* radii, const float* light_dir, const float* ambient);
int rmh_scene_load(const char* path, int32_t* num_spheres, float** centers, float** colors, float** radii,
                   float light_dir[3], float* ambient);

/* ---- seeded RNG (PCG32, O'Neill 2014) ------------------------------------------------ */
typedef struct rmh_rng {
  uint64_t state;
  uint64_t inc;
} rmh_rng;
void rmh_rng_seed(rmh_rng* rng, uint64_t seed, uint64_t stream);
uint32_t rmh_rng_u32(rmh_rng* rng);
/* Uniform integer in [0, n) (Lemire's unbiased bounded method); n >= 1. */
uint32_t rmh_rng_below(rmh_rng* rng, uint32_t n);
/* Uniform float in [lo, hi) with 24 random bits. */
float rmh_rng_uniform(rmh_rng* rng, float lo, float hi);

/* ---- dataset.rs: SceneDataset --------------------------------------------------------- */
typedef struct rmh_dataset rmh_dataset;
/* targets: host linear RGB [num_pixels][3]; fg = pixels with R+G+B > 0.05 (dataset.rs:26-35). */
int rmh_dataset_create(const float* targets, int64_t num_pixels, rmh_dataset** out);
void rmh_dataset_destroy(rmh_dataset* ds);
void rmh_dataset_counts(const rmh_dataset* ds, int64_t* num_fg, int64_t* num_bg);
/* sample_batch index draw (dataset.rs:47-73): floor(batch*ratio) uniform pixels, then the
 * rest uniformly from the foreground list (shrunk to |fg| when fg is smaller). *count gets
 * the number written: like the reference, a dataset without foreground gives a short batch. */
int rmh_dataset_sample(const rmh_dataset* ds, int32_t batch, float uniform_ratio, rmh_rng* rng, int32_t* indices,
                       int32_t* count);
/* The count rule of sample_batch alone (dataset.rs:54-67), shared by rmh_dataset_sample, the
 * device sampler (rm_sample_batch) and the driver's global ray count: *n_uniform uniform draws
 * and *n_fg foreground draws (0 without foreground: the short batch). */
void rmh_dataset_sample_count(const rmh_dataset* ds, int32_t batch, float uniform_ratio, int64_t* n_uniform,
                              int64_t* n_fg);
/* The foreground pixel list (ascending; valid while ds lives), for uploading to the device. */
void rmh_dataset_fg(const rmh_dataset* ds, const int32_t** fg, int64_t* num_fg);

/* ---- training.rs:87-238: prune_and_split ---------------------------------------------- */
/* raw_packed: the model's RAW params [centers 3M | colors 3M | radius M | light 3 | ambient 1];
 * init_centers [M][3]: the centres the stage started from. out_packed (capacity 14M+4 floats)
 * receives the next generation in the same layout, light/ambient carried over; out_M its M.
 * Returns RMH_ERR_INVALID_ARG if every sphere was pruned. */
int rmh_prune_and_split(const float* raw_packed, int32_t num_spheres, const float* init_centers, int32_t stage,
                        int32_t stages, rmh_rng* rng, float* out_packed, int32_t* out_num_spheres);
/* rmh_prune_and_split with the split rule's thresholds as knobs (growth runs such as
 * BASELINE configs[4], "4096 spheres after adaptive split/prune"): a sphere splits when
 * r > split_scale * 0.25 * 0.65^stage and its squared move exceeds split_move^2
 * (training.rs:185-188), and -- with max_spheres > 0 -- when the next generation then still fits
 * max_spheres counting every later sphere as kept (spheres are visited in order; a sphere that
 * would not fit is kept unsplit). split_scale = 1, split_move = 0.05, max_spheres = 0 is the
 * reference rule (exactly rmh_prune_and_split); split_scale = 0, split_move = 0 splits every
 * sphere that survives pruning. The pruning rules and the children (training.rs:167-222) are
 * unchanged. */
int rmh_prune_and_split_ex(const float* raw_packed, int32_t num_spheres, const float* init_centers, int32_t stage,
                           int32_t stages, float split_scale, float split_move, int32_t max_spheres, rmh_rng* rng,
                           float* out_packed, int32_t* out_num_spheres);
/* The initial 7-sphere raw model of train.rs:100-126 (out: 7*7+4 floats). */
void rmh_initial_model(float* raw_packed);

/* ---- data-parallel collectives --------------------------------------- */
/* The two collectives the multi-rank driver issues, on fp32 DEVICE buffers, asynchronously on
 * the driver's HIP stream (`stream` is a hipStream_t): an in-place sum all-reduce and an
 * in-place broadcast from `root`. Return RMH_OK or an error code. Any implementation works:
 * rmh_collective_rccl_create builds the RCCL one (one process per GPU, over xGMI); tests plug
 * in their own (e.g. gloo over host copies, to run two ranks on one GPU). */
typedef struct rmh_collective {
  void* state;
  int32_t rank;
  int32_t world;
  int (*all_reduce_sum)(void* state, float* buf, int64_t count, void* stream);
  int (*broadcast)(void* state, float* buf, int64_t count, int32_t root, void* stream);
  /* Nullable. Called by a rank that leaves rmh_train with an error after the collectives began:
   * it releases this rank's side of the collectives (the RCCL implementation aborts its
   * communicator, which ends its in-flight collectives). It does NOT reach the other ranks: a peer
   * blocked in a collective with this rank leaves it through its own `wait` timeout, or is ended
   * by the launcher (rm_train --ranks terminates the other ranks when one fails). */
  void (*abort)(void* state);
  /* Nullable. The driver's only way of waiting for its stream while collectives may be in
   * flight (instead of hipStreamSynchronize): returns RMH_OK once the stream drained, or an error
   * when it did not within the implementation's timeout -- the RCCL one then aborts its
   * communicator, so a rank whose peer died fails instead of spinning forever. rmh_train calls it
   * on every rank at least every 32 steps (and at stage ends and loss reads), so the queued work a
   * wait covers -- what its timeout must allow for -- is at most 32 steps. */
  int (*wait)(void* state, void* stream);
} rmh_collective;
/* RCCL communicator of rank `rank` of `world` on HIP device `device`. Rank 0 creates the
 * ncclUniqueId and publishes it at id_path (rmh_rendezvous_publish); the other ranks wait up to
 * timeout_s seconds for it (rmh_rendezvous_read) -- however late they start; rank 0 removes the
 * file once every rank has joined. run_id (nullable: env RMH_RUN_ID, else TORCHELASTIC_RUN_ID)
 * tags the file, so a file left by an earlier run with another id is never used; with world > 1 it
 * must name this run -- an empty id or torchrun's default "none" is refused (RMH_ERR_INVALID_ARG,
 * before any GPU call): a stale file of a crashed run would pass for such a run's. timeout_s is
 * also the watchdog of `wait`. id_path may be NULL when world == 1. */
int rmh_collective_rccl_create(int32_t rank, int32_t world, int32_t device, const char* id_path, const char* run_id,
                               double timeout_s, rmh_collective* out);
void rmh_collective_rccl_destroy(rmh_collective* c);
/* The file rendezvous of rmh_collective_rccl_create, on any payload: publish writes
 * [magic | run id | size | blob] to a temporary name and renames it to path (a stale file at path
 * is removed first); read polls path until a complete file with the same run id and payload size
 * appears (RMH_ERR_IO after timeout_s seconds, naming what the file there held). run_id as above
 * (an empty or "none" id: RMH_ERR_INVALID_ARG). */
int rmh_rendezvous_publish(const char* path, const char* run_id, const void* blob, int64_t size);
int rmh_rendezvous_read(const char* path, const char* run_id, void* blob, int64_t size, double timeout_s);

/* ---- train.rs: the driver ------------------------------------------------------------- */
typedef struct rmh_train_config {
  const char* cameras_json; /* data/cameras.json; image paths resolved against its directory */
  const char* out_dir;      /* scene.json and steps/ previews go here (NULL: no output files) */
  int32_t width, height;    /* 256 x 256 (train.rs:32-33) */
  int32_t stages;           /* 5 (train.rs:128) */
  int32_t steps_per_stage;  /* 700 (train.rs:129) */
  int32_t batch;            /* 16384 (train.rs:30) */
  int32_t march_steps;      /* 40 (renderer_diff.rs:22) */
  float max_smooth;         /* 32 (train.rs:131) */
  float base_lr;            /* 0.05 (train.rs:166) */
  float weight_decay;       /* 1e-5 (train.rs:161) */
  int32_t log_every;        /* 100 (train.rs:200); 0 = silent */
  int32_t previews;         /* write steps/stage_i.png and steps/final_1.png */
  uint64_t seed;
  int32_t device;
  /* Data parallelism (NULL: one rank). With comm->world = P ranks each rank samples its share
   * of the batch (batch / P rays, rank-distinct sampler streams) and runs the fused train step
   * with the global loss normalisation 1/(3 N_global); one all-reduce(sum) of the packed
   * [gradient | loss sum] (7M+5 floats) precedes the replicated optimizer step; rank 0 runs
   * prune_and_split and broadcasts the next generation (its size, then its 7M'+4 raw params);
   * only rank 0 logs and writes files. Every rank ends with the same parameters. */
  const rmh_collective* comm;
  /* Growth knobs of prune_and_split (rmh_prune_and_split_ex). A zeroed struct gets the reference
   * rule (training.rs:185-188): split_scale 0 = 1 (the threshold 0.25 * 0.65^stage times this),
   * split_move 0 = 0.05 (the minimum move); a negative value drops that condition (both negative:
   * every surviving sphere splits -- the growth runs of configs[4], rm_train --split-all);
   * max_spheres 0 = no cap. rmh_train_config_default sets 1, 0.05, 0. */
  float split_scale;
  float split_move;
  int32_t max_spheres;
  /* 1: fp16 colour / fp32 SDF (BASELINE configs[4], RM_MARCH_COLOR_F16): the renders read the
   * activated colours as IEEE binary16, written by rm_optimizer_step_f16; parameters, moments and
   * gradients stay fp32. 0: fp32 colours (the reference). */
  int32_t color_f16;
  /* Nullable. Called on every rank after each stage's training, before prune_and_split, with the
   * stage's trained RAW packed parameters (host memory, valid during the call). */
  void (*on_generation)(void* user, int32_t stage, int32_t num_spheres, const float* raw_packed);
  void* user;
} rmh_train_config;
void rmh_train_config_default(rmh_train_config* cfg);

typedef struct rmh_train_result {
  int32_t num_spheres;   /* M of the exported model */
  int32_t steps;         /* optimizer steps taken */
  float final_loss;      /* compute_loss of the last step */
  double seconds;        /* wall time of the stage loops (GPU synchronised) */
  double step_ms;        /* mean per-step time (sample + gather + train step + optimizer) */
} rmh_train_result;
/* raw_out (nullable, capacity 7*M_max+4) receives the final RAW packed params. */
int rmh_train(const rmh_train_config* cfg, rmh_train_result* result, float* raw_out, int32_t raw_capacity);

/* ---- train.rs:335-366: preview of a scene.json (render_diff, S=40, k=32) --------------- */
/* radius_offset: 0.01 reproduces the model's activation (scene.rs:43); scene.json stores
 * softplus(raw) without it. */
int rmh_preview(const char* scene_json, const char* png_path, int32_t width, int32_t height, const float eye[3],
                const float target[3], float fov_deg, float radius_offset, int32_t device);

/* ---- viewer.rs + shader.wgsl: the viewer's frames of a scene.json, headless -------------- */
/* A viewer pose: the layout of rm_view_camera (raymarch.h). */
typedef struct rmh_view_pose {
  float pos[3];
  float forward[3];
  float up[3];
} rmh_view_pose;
/* The viewer's camera (viewer.rs:65-86) from its position, yaw and pitch (radians):
 * forward = (cos yaw cos pitch, sin pitch, sin yaw cos pitch) normalised, right =
 * normalize(forward x Y), up = normalize(right x forward). The viewer starts at pos (0, 0, -2.5),
 * yaw pi/2, pitch 0. */
void rmh_view_camera(const float pos[3], float yaw, float pitch, rmh_view_pose* out);
/* Loads scene_json as viewer.rs does -- the stored radii, radius_offset (0 by default) added --
 * renders the `count` poses with rm_view and writes one RGBA PNG per frame from its RGBA8 output
 * (the bytes the viewer's sRGB surface shows). out_pattern names the files: a "%d" in it takes the
 * frame index; without one, a single frame goes to out_pattern itself and several frames get
 * "_<index>" before the extension. */
int rmh_view(const char* scene_json, const char* out_pattern, int32_t width, int32_t height,
             const rmh_view_pose* cams, int32_t count, float radius_offset, int32_t device);
/* RGBA8 [h][w][4] -> PNG (colour type 6); creates missing parent directories. */
int rmh_png_write_rgba(const char* path, const uint8_t* rgba, int32_t width, int32_t height);
/* 8-bit PNG -> RGBA8 [h][w][4] (alpha 255 where the file has none). */
int rmh_png_read_rgba(const char* path, int32_t* width, int32_t* height, uint8_t** rgba);

/* ---- the trained surface as a coloured triangle mesh ----------------------------------------- */
/* The scene's soft-min D (rm_sdf_grid / rm_sdf_query, raymarch.h) is an implicit surface; these
 * entry points turn its zero set into a mesh other tools open. The reference has no such export. */
typedef struct rmh_mesh rmh_mesh;
/* Marching tetrahedra on a lattice of distances (CPU only, no GPU call). dist: host [nz][ny][nx],
 * x fastest, the layout rm_sdf_grid writes; lattice point (ix, iy, iz) lies at origin + (float)i *
 * spacing per axis and is inside where D < 0. Every cube is cut into the same six tetrahedra (the
 * Kuhn decomposition: the six monotone lattice paths from corner 000 to corner 111), so
 * neighbouring cubes agree on their shared face diagonals and the surface is closed by
 * construction. One vertex per crossing lattice edge (axis edges, face and body diagonals), shared
 * through an edge key and placed at t = D_a / (D_a - D_b); triangles are wound so that the normal
 * points from inside to outside. The order is fixed -- cubes z, y, x, the six tetrahedra in a
 * fixed order, vertices numbered at first use -- so two runs give the same bytes. The mesh has no
 * normals or colours (rmh_mesh_normals / _colors return NULL). An all-inside or all-outside grid
 * gives an empty mesh and RMH_OK. nx, ny, nz >= 2, spacing > 0. Release with rmh_mesh_free. */
int rmh_mesh_from_grid(const float* dist, int32_t nx, int32_t ny, int32_t nz, const float origin[3], float spacing,
                       rmh_mesh** out);
typedef struct rmh_mesh_config {
  int32_t res;          /* cells along the longest extent of the box (128)                          */
  float margin;         /* the box is that of c_j +- (r_j + margin) (0.05)                           */
  float smooth_k;       /* soft-min sharpness (32)                                                   */
  float radius_offset;  /* added to scene.json's radii: 0.01 is the surface training fitted (0.01)   */
  int32_t refine;       /* Newton projections v -= D g / |g|^2 of the vertices onto D = 0 (2)        */
  int32_t device;
} rmh_mesh_config;
void rmh_mesh_config_default(rmh_mesh_config* cfg);
/* scene.json -> mesh: loads the scene (radii + radius_offset), takes the axis-aligned box of
 * c_j +- (r_j + margin) with cubic cells of (longest extent / res), evaluates D on its lattice with
 * rm_sdf_grid, copies the grid to the host and extracts (rmh_mesh_from_grid); then `refine` Newton
 * projections of the vertices through rm_sdf_query (a vertex with |g|^2 < 1e-12 keeps its place)
 * and one more query for the per-vertex normals g / |g| and the blended colours. cfg NULL = the
 * defaults. */
int rmh_mesh_extract(const char* scene_json, const rmh_mesh_config* cfg, rmh_mesh** out);
/* open_edges: the undirected edges that do not lie in exactly two triangles -- non-zero only where
 * the surface leaves the grid. The soft-min surface lies outside the spheres where they blend, by at
 * most ln(M) / k (D >= min_j d_j - ln(M) / k): a margin of that much always closes the mesh; the
 * default 0.05 does for scenes of a few spheres per neighbourhood (the grown 4096-sphere model
 * needs more). */
void rmh_mesh_counts(const rmh_mesh* mesh, int64_t* vertices, int64_t* faces, int64_t* open_edges);
/* Host arrays owned by the mesh: vertices [V][3], normals [V][3] (unit) and colours [V][3] (linear
 * RGB in [0, 1]; both NULL for a mesh of rmh_mesh_from_grid), faces [F][3] vertex indices. */
const float* rmh_mesh_vertices(const rmh_mesh* mesh);
const float* rmh_mesh_normals(const rmh_mesh* mesh);
const float* rmh_mesh_colors(const rmh_mesh* mesh);
const int32_t* rmh_mesh_faces(const rmh_mesh* mesh);
/* Milliseconds rmh_mesh_extract spent: ms[0] the grid evaluation, [1] its copy to the host, [2] the
 * extraction, [3] the refinement and the final query (zeros for a mesh of rmh_mesh_from_grid). */
void rmh_mesh_timing(const rmh_mesh* mesh, double ms[4]);
void rmh_mesh_free(rmh_mesh* mesh);
/* Binary little-endian PLY: per vertex x y z nx ny nz (float) and red green blue (uchar: the
 * piecewise sRGB encode of rm_view's RGBA8 output, rounded to nearest), per face uchar 3 + three
 * int -- 27 V + 13 F bytes after the header. A mesh without normals / colours writes zero normals
 * and white. Creates missing parent directories. */
int rmh_mesh_write_ply(const rmh_mesh* mesh, const char* path);

/* ---- generate.rs:20-112: target images + cameras.json ---------------------------------- */
/* Renders the three-sphere scene from the 10 generate.rs cameras with rm_render_camera and
 * writes out_dir/target_i.png plus out_dir/cameras.json ("file" entries are
 * "<file_prefix>target_i.png"; generate.rs uses "data/"). */
int rmh_generate(const char* out_dir, const char* file_prefix, int32_t width, int32_t height, int32_t device);

#ifdef __cplusplus
}
#endif

#endif /* RM_HOST_H_ */
