// dt_api_internal.h — what dt_api.cpp (the scene and render path) shares with dt_api_aux.cpp (the auxiliary
// entry points); not part of the C ABI. It needs HIP, unlike host_internal.h, which the pure-host units include.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <vector>

#include "dt_kernel_iface.h"
#include "host_internal.h"
#include "host_launch.h"

namespace dth {

// must match the device-side DScene (dt_kernels.hip)
struct HScene {
  const void* nodes;
  const void* fnodes;
  const uint32_t* sg_cells;
  const int32_t* sg_list;
  const int32_t* leaf_idx;
  const void* hdr;
  const double* geom;
  const void* mat;
  const void* lights;
  const uint8_t* tex;
  const float* cloud_z;
  unsigned long long* stats;
  unsigned long long* queue;
  const void* bnodes;       // motion-blur bump tree (host_fasttree.cpp)
  const int32_t* bparent;   // parent of every reference-tree node
  const uint32_t* pl_cells; // primary-ray candidate lists (host_primlists.cpp)
  const uint32_t* pl_list;
  uint8_t* sky_miss;
  void* dn_pool;
  uint32_t* again_list;
  unsigned int* again_n;
  const void* sub_nodes;      // shadow-grid block subtrees
  const uint32_t* sub_blocks;
  unsigned long long* clear0;   // the other parity's counters, zeroed by the launch (dt_kernels.hip)
  unsigned long long* clear1;
  int32_t n_clear0, n_clear1;
  double* chunk_cols;           // chunk items: per-pixel sample colours (dt_kernels.hip)
  uint32_t* item_cost;          // diagnostic builds: per-item durations (dt_debug_item_costs)
  double* accum;                // window launches: the caller's accumulator (dt_render_window)
};

// DT_N_STAMPS (dt_scene_dev.h): diagnostic counter slots of -DDT_STAMPS builds (dt_debug_counters):
// phases, then (waves, lanes, hits) per (light, shape) shadow test
enum { ST_RAYS = 0, ST_SHADOW = 1, ST_SKY = 2, ST_UV = 3, ST_GLOSSY = 4, ST_SPHL = 5, ST_PRISM = 6,
       ST_REFL = 7, ST_NAN = 8, ST_PIXELS = 9, ST_SAMPLES = 10, ST_STACK = 11, ST_TEX = 12, ST_BOX = 13, ST_PRIM = 14, ST_WNODES = 15,
       ST_DONATE = 16, ST_DN_OVF = 17, ST_N = 18 };

// (dt_api.cpp: msg into the one thread-local behind dt_last_error)
int fail(int code, const std::string& msg);

#define HIPCHK(expr)                                                                        \
  do {                                                                                      \
    hipError_t _e = (expr);                                                                 \
    if (_e != hipSuccess)                                                                   \
      return dth::fail(DT_E_NO_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

// the lazily grown device buffers of a scene (host_launch.h DevBuf) over the HIP calls
struct HipMem {
  typedef hipStream_t Stream;
  static int alloc(void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }
  static void free(void* p) { (void)hipFree(p); }
  static int sync(hipStream_t st) { return (int)hipStreamSynchronize(st); }
};
typedef DevBuf<HipMem> DevMem;

int max_resident_waves(const void* kernel_fn, int block);

}  // namespace dth

struct dt_scene {
  int device = 0;
  dth::FlatScene flat;
  void* d_nodes = nullptr;
  void* d_fnodes = nullptr;
  int n_fnodes = 0;
  void* d_bnodes = nullptr;    // bump tree for motion-blur passes (0 nodes: they walk the reference tree)
  void* d_bparent = nullptr;
  int n_bnodes = 0;
  float bump_pad = 0;          // y padding of its leaves: the largest |shift| a blur pass can draw
  bool bump_up_only = false;   // bump tree / blur-padded lists built for shifts >= 0 only
  bool no_cull = false;        // a RectPrismWithCylinder: no t-culling, no grid, no primary lists
  unsigned features = ~0u;     // the scene's feature mask (dt_scene_dev.h): which builds can render it
  int kernel = DT_KERNEL_AUTO; // dt_scene_set_kernel
  dth::ShadowGrid sg;
  void* d_sg_cells = nullptr;
  void* d_sg_list = nullptr;
  void* d_sub_nodes = nullptr;    // shadow-grid block subtrees (ShadowGrid::sub_*)
  void* d_sub_blocks = nullptr;
  int ftree_mode = 0;
  int boxes_ordered = 0;   // lb <= ub on every axis of every node (both trees), no NaN bound
  void* d_leaf = nullptr;
  void* d_hdr = nullptr;
  void* d_geom = nullptr;
  void* d_mat = nullptr;
  void* d_lights = nullptr;
  void* d_tex = nullptr;
  // the cloud z table (2048 floats); like every DevMem below grown by the launch that needs it
  // (host_launch.h DevBuf: a failed allocation leaves it empty, so the next launch allocates again)
  dth::DevMem zs;
  // ST_N counters + queue word (+ the stamps builds' slots), twice: launches alternate between the
  // two (parity), and each zeroes the other for the next one (HScene::clear0)
  unsigned long long* d_stats = nullptr;
  int n_launch = 0;     // trace launches enqueued (the parity of the next: n_launch & 1)
  int last_parity = 0;  // the parity of the last one (dt_collect_stats)
  // the launch record's device copy, one per parity, uploaded only when its bytes changed (a still
  // frame rendered again uploads nothing: no copy kernel between its launches)
  void* d_launch = nullptr;
  std::vector<uint8_t> rec_last[2], rec2_last[2];
  std::vector<uint8_t> zs_last;   // the z table in zs
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t ev_copy = nullptr;   // staging buffers may be rewritten once this has fired
  uint8_t* h_launch = nullptr;    // pinned staging for the launch record
  float* h_zs = nullptr;          // pinned staging for the cloud z sequence
  bool copy_pending = false;
  bool timed = false;
  bool launched = false;   // a trace launch was enqueued (may still read device-side lists)
  bool uploaded = false;   // dt_scene_upload ran (dt_scene_prepare builds on the host only)
  bool pl_dirty = false;   // the host primary lists changed since their last upload
  dth::Accel acc;          // host acceleration structures until the upload
  // primary-ray candidate lists, rebuilt when the camera / resolution changes (host_primlists.cpp)
  std::vector<dtd::DNodeDev> fnodes_host, bnodes_host;
  std::vector<std::vector<dth::P3>> fhull, bhull;   // leaf hull points per fast / bump tree node (host_hull.cpp)
  bool pl_bump = false;                             // lists for the blur passes follow the pass-0 lists
  std::vector<double> pl_key;
  dth::DevMem sky_miss;   // 1-spp launches: missed-pixel flags (dt_sky_miss_kernel clears them)
  // sky items (dt_kernels.hip DT_SKY_AGAIN): the list a still build leaves to its *_sky build, that
  // launch's record (pinned staging h_launch2, guarded by ev_copy like h_launch) and its counters
  dth::DevMem again;
  void* d_launch2 = nullptr;
  uint8_t* h_launch2 = nullptr;
  unsigned long long* d_stats2 = nullptr;   // ST_N counters + queue word + list count, twice (parity)
  bool again_used = false;                  // the last render ran the second launch
  dth::DevMem dn_pool;      // dt_trace_kernel_dn: DT_DN_POOL_REC work-sharing records per wave
  dth::DevMem chunk_cols;   // chunk items: spp sample colours (double) per pixel item
  dth::DevMem item_cost;    // DT_ITEM_COSTS=1 (diagnostic builds): per-item durations (uint32_t),
  int64_t item_cost_n = 0;  // of the last launch that recorded them
  dth::PrimLists pl;
  bool pl_ok = false;
  void* d_pl_cells = nullptr;
  void* d_pl_list = nullptr;
  dtd::DParams last;
  int last_px_samples = 0;   // samples per pixel of the last launch: spp, or a window's end - begin
  // adaptive window launches (dt_render_window_adaptive): the selection's buffers in one allocation
  // (the list's length, the list, the per-wave offsets and keep bits; adapt_layout); ev_sel fires
  // when the selection kernels have run (dt_adapt_select_ms)
  dth::DevMem adapt;
  hipEvent_t ev_sel = nullptr;
  bool last_adaptive = false;   // the last launch ran over the selection's list: stats.pixels is its length
};

// dt_api.cpp
int prepare_render(const dt_scene* sc, const dt_globals* g, int32_t frame, const dt_tiles* tiles, dtd::DParams& P,
                   std::vector<float>& zs);
int scene_upload(dt_scene* s);
int update_primary_lists(dt_scene* sc, dtd::DParams& P, bool upload_now);
void fill_hscene(const dt_scene* sc, dth::HScene& hs);
