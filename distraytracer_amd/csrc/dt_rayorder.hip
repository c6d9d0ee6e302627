// dt_ray_order / dt_permute_rows -- sorting caller-supplied rays into coherent waves (include/dt.h): a key
// per ray (the Morton cell of its start in a box and of its direction on the octahedral map, dt_order.h), the
// stable ascending order of the keys as a permutation, and the gather / scatter of rows by it. No reference
// counterpart. The specification is the comment block of dt_ray_order in include/dt.h; tests/rayorder_ref.py
// restates keys, box and order in numpy, and the host loop and the kernels agree with it bit for bit.
//
// The device path is a chain of kernels on one stream, none of which waits on another workgroup (no
// decoupled look-back, no flag, no spin; the only synchronisation is the kernel boundary):
//   ro_box_partial, ro_box_final   min / max of the non-void starts (exact, order-free), unless the box is given
//   ro_key                         one key per ray
//   per 8-bit digit of the B + 1 key bits, least significant first (an LSD radix sort of (key, index) pairs):
//     ro_hist                      digit counts of each workgroup's tile of RO_TILE keys, digit-major
//     ro_scan_reduce / ro_scan_apply   exclusive scan of the counts, chunk sums scanned recursively
//     ro_scatter                   in-wave stable rank of equal digits from wave64 ballots, per-wave LDS
//                                  counters, the tile staged in LDS in digit order, stores leaving in runs
// A translation unit of its own, compiled once for both libraries: no other object changes. The error
// prefix and the timed launch are dt_post.h's.
#include <algorithm>
#include <vector>

#include "dt_post.h"   // (first: the HIP runtime's __host__ __device__ for dt_order.h)

#include "dt_order.h"

namespace {

constexpr int RO_THREADS = 256;
constexpr int RO_WAVES = RO_THREADS / 64;
constexpr int RO_ITEMS = DT_RAY_ORDER_TILE / RO_THREADS;   // keys per thread
constexpr int RO_WAVE_KEYS = 64 * RO_ITEMS;                // consecutive keys one wave ranks
constexpr int RO_SCAN_ITEMS = 8;
constexpr int RO_SCAN_CHUNK = RO_THREADS * RO_SCAN_ITEMS;   // entries one scan workgroup covers
constexpr int RO_BOX_BLOCKS = 1024;
constexpr uint32_t RO_PAD = 0xFFFFFFFFu;   // past the end of the last tile: digit 255 in every pass, never a key (keys <= 2^30)
static_assert(DT_RAY_ORDER_TILE % RO_THREADS == 0 && RO_ITEMS >= 1, "tile");

struct OrderArgs {   // by value: the key's parameters travel with the launch
  int64_t n;
  int32_t ob, db, dir_major;
  const double* start;
  const double* dir;
  const double* box;   // 6 doubles on the device: lo, hi (read unless box_given)
  int32_t box_given;
  double given[6];
};

// ---- box ------------------------------------------------------------------------------------------

__device__ __forceinline__ void ro_block_minmax(double* lo, double* hi, double (*sh)[6])
{
  const int t = threadIdx.x;
  for (int k = 0; k < 3; ++k) {
    sh[t][k] = lo[k];
    sh[t][3 + k] = hi[k];
  }
  __syncthreads();
  for (int s = RO_THREADS / 2; s > 0; s >>= 1) {
    if (t < s)
      for (int k = 0; k < 3; ++k) {
        sh[t][k] = sh[t + s][k] < sh[t][k] ? sh[t + s][k] : sh[t][k];
        sh[t][3 + k] = sh[t + s][3 + k] > sh[t][3 + k] ? sh[t + s][3 + k] : sh[t][3 + k];
      }
    __syncthreads();
  }
}

// partial[6 * block]: min and max of the block's non-void starts (+inf / -inf: none)
__global__ __launch_bounds__(RO_THREADS) void ro_box_partial(OrderArgs a, double* partial)
{
  __shared__ double sh[RO_THREADS][6];
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t i = (int64_t)blockIdx.x * RO_THREADS + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * RO_THREADS) {
    double o[3], d[3];
    for (int k = 0; k < 3; ++k) {
      o[k] = a.start[3 * i + k];
      d[k] = a.dir[3 * i + k];
    }
    if (dto::order_void(o, d)) continue;
    for (int k = 0; k < 3; ++k) {
      lo[k] = o[k] < lo[k] ? o[k] : lo[k];
      hi[k] = o[k] > hi[k] ? o[k] : hi[k];
    }
  }
  ro_block_minmax(lo, hi, sh);
  if (threadIdx.x < 6) partial[6 * (int64_t)blockIdx.x + threadIdx.x] = sh[0][threadIdx.x];
}

// box[6] from the partials; no non-void ray: zeros. x + 0.0 reports a -0 as +0 whichever zero the
// reduction met first.
__global__ __launch_bounds__(RO_THREADS) void ro_box_final(const double* partial, int n_partial, double* box)
{
  __shared__ double sh[RO_THREADS][6];
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int b = threadIdx.x; b < n_partial; b += RO_THREADS)
    for (int k = 0; k < 3; ++k) {
      const double l = partial[6 * b + k], h = partial[6 * b + 3 + k];
      lo[k] = l < lo[k] ? l : lo[k];
      hi[k] = h > hi[k] ? h : hi[k];
    }
  ro_block_minmax(lo, hi, sh);
  if (threadIdx.x < 6) {
    const bool none = sh[0][0] > sh[0][3];
    box[threadIdx.x] = none ? 0.0 : sh[0][threadIdx.x] + 0.0;
  }
}

void host_box(int64_t n, const double* start, const double* dir, double* box)
{
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t i = 0; i < n; ++i) {
    if (dto::order_void(start + 3 * i, dir + 3 * i)) continue;
    for (int k = 0; k < 3; ++k) {
      lo[k] = start[3 * i + k] < lo[k] ? start[3 * i + k] : lo[k];
      hi[k] = start[3 * i + k] > hi[k] ? start[3 * i + k] : hi[k];
    }
  }
  const bool none = lo[0] > hi[0];
  for (int k = 0; k < 3; ++k) {
    box[k] = none ? 0.0 : lo[k] + 0.0;
    box[3 + k] = none ? 0.0 : hi[k] + 0.0;
  }
}

// ---- keys -----------------------------------------------------------------------------------------

__global__ __launch_bounds__(RO_THREADS) void ro_key(OrderArgs a, uint32_t* key, uint32_t* key_out)
{
  double lo[3], hi[3];
  for (int k = 0; k < 3; ++k) {
    lo[k] = a.box_given ? a.given[k] : a.box[k];
    hi[k] = a.box_given ? a.given[3 + k] : a.box[3 + k];
  }
  for (int64_t i = (int64_t)blockIdx.x * RO_THREADS + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * RO_THREADS) {
    double o[3], d[3];
    for (int k = 0; k < 3; ++k) {
      o[k] = a.start[3 * i + k];
      d[k] = a.dir[3 * i + k];
    }
    const uint32_t q = dto::order_key(a.ob, a.db, a.dir_major, lo, hi, o, d);
    key[i] = q;
    if (key_out) key_out[i] = q;
  }
}

// ---- radix sort -----------------------------------------------------------------------------------

// the lanes of this wave whose 8-bit digit equals mine (every lane takes part: padding has digit 255)
__device__ __forceinline__ unsigned long long ro_match(uint32_t digit)
{
  unsigned long long m = ~0ull;
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool bit = (digit >> b) & 1u;
    const unsigned long long bal = __ballot(bit);
    m &= bit ? bal : ~bal;
  }
  return m;
}

// A wave's keys are RO_WAVE_KEYS consecutive ones, item j of lane l at j*64 + l: memory order is (j, l) order.
__device__ __forceinline__ int64_t ro_item_index(int64_t tile, int wave, int lane, int j)
{
  return tile * DT_RAY_ORDER_TILE + (int64_t)wave * RO_WAVE_KEYS + j * 64 + lane;
}

// hist[digit * n_tiles + tile]: how many keys of the tile have the digit (the order in which the scan runs:
// all tiles of digit 0, then of digit 1, ...)
__global__ __launch_bounds__(RO_THREADS) void ro_hist(const uint32_t* key, int64_t n, int shift, uint32_t* hist,
                                                      int64_t n_tiles)
{
  __shared__ uint32_t count[256];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  count[t] = 0;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < RO_ITEMS; ++j) {
    const int64_t i = ro_item_index(blockIdx.x, wave, lane, j);
    const bool valid = i < n;
    const uint32_t digit = valid ? (key[i] >> shift) & 255u : 255u;
    const unsigned long long same = ro_match(digit) & __ballot(valid);
    if (valid && (same & ((1ull << lane) - 1ull)) == 0) atomicAdd(&count[digit], (uint32_t)__popcll(same));
  }
  __syncthreads();
  hist[(int64_t)t * n_tiles + blockIdx.x] = count[t];
}

// sums[block] = the sum of the block's chunk of v
__global__ __launch_bounds__(RO_THREADS) void ro_scan_reduce(const uint32_t* v, int64_t n, uint32_t* sums)
{
  __shared__ uint32_t sh[RO_THREADS];
  const int t = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * RO_SCAN_CHUNK + (int64_t)t * RO_SCAN_ITEMS;
  uint32_t s = 0;
#pragma unroll
  for (int j = 0; j < RO_SCAN_ITEMS; ++j) s += base + j < n ? v[base + j] : 0u;
  sh[t] = s;
  __syncthreads();
  for (int h = RO_THREADS / 2; h > 0; h >>= 1) {
    if (t < h) sh[t] += sh[t + h];
    __syncthreads();
  }
  if (t == 0) sums[blockIdx.x] = sh[0];
}

// the exclusive prefix sum of x over the workgroup's 256 threads (sh: 4 words)
__device__ __forceinline__ uint32_t ro_block_exclusive(uint32_t x, uint32_t* sh)
{
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  uint32_t inc = x;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(inc, d);
    if (lane >= d) inc += up;
  }
  if (lane == 63) sh[wave] = inc;
  __syncthreads();
  uint32_t before = 0;
  for (int w = 0; w < wave; ++w) before += sh[w];
  __syncthreads();   // (sh may be reused at once)
  return before + inc - x;
}

// v becomes its exclusive prefix sum within the block's chunk, plus offset[block] (the scanned chunk sums; null: 0)
__global__ __launch_bounds__(RO_THREADS) void ro_scan_apply(uint32_t* v, int64_t n, const uint32_t* offset)
{
  __shared__ uint32_t sh[RO_WAVES];
  const int t = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * RO_SCAN_CHUNK + (int64_t)t * RO_SCAN_ITEMS;
  uint32_t x[RO_SCAN_ITEMS], s = 0;
#pragma unroll
  for (int j = 0; j < RO_SCAN_ITEMS; ++j) {
    x[j] = base + j < n ? v[base + j] : 0u;
    s += x[j];
  }
  uint32_t run = ro_block_exclusive(s, sh) + (offset ? offset[blockIdx.x] : 0u);
#pragma unroll
  for (int j = 0; j < RO_SCAN_ITEMS; ++j) {
    if (base + j < n) v[base + j] = run;
    run += x[j];
  }
}

// One pass: (key, index) pairs of this tile go to their places in the order of the digit at `shift`, equal
// digits in the order they have. first: the index is the position (no index array is read); last: no key is
// written. offset: the scanned histogram.
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(RO_THREADS) void ro_scatter(const uint32_t* key_in, const uint32_t* idx_in, int64_t n,
                                                         int shift, const uint32_t* offset, int64_t n_tiles,
                                                         uint32_t* key_out, uint32_t* idx_out)
{
  __shared__ uint32_t wave_count[RO_WAVES][256];   // per wave and digit: the count, then the keys of the waves before
  __shared__ uint32_t first_of[256];               // the tile-local place of the digit's first key
  __shared__ uint32_t dest_of[256];                // the global place of the digit's first key, less first_of
  __shared__ uint32_t scan_sh[RO_WAVES];
  __shared__ uint32_t stage_key[DT_RAY_ORDER_TILE];
  __shared__ uint32_t stage_idx[DT_RAY_ORDER_TILE];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int64_t tile = blockIdx.x;
  const int64_t left = n - tile * DT_RAY_ORDER_TILE;
  const int n_valid = left < DT_RAY_ORDER_TILE ? (int)left : DT_RAY_ORDER_TILE;
  for (int w = 0; w < RO_WAVES; ++w) wave_count[w][t] = 0;
  __syncthreads();

  uint32_t key[RO_ITEMS], idx[RO_ITEMS], rank[RO_ITEMS];
#pragma unroll
  for (int j = 0; j < RO_ITEMS; ++j) {
    const int64_t i = ro_item_index(tile, wave, lane, j);
    key[j] = i < n ? key_in[i] : RO_PAD;
    idx[j] = i < n ? (FIRST ? (uint32_t)i : idx_in[i]) : 0u;
  }
  // the rank among the wave's keys of the same digit, in memory order: the keys of earlier items (the
  // wave's counter) and the lower lanes of this item (the ballots). One lane per digit and item adds.
#pragma unroll
  for (int j = 0; j < RO_ITEMS; ++j) {
    const uint32_t digit = (key[j] >> shift) & 255u;
    const unsigned long long same = ro_match(digit);
    const unsigned long long below = same & ((1ull << lane) - 1ull);
    uint32_t before = 0;
    if (below == 0) before = atomicAdd(&wave_count[wave][digit], (uint32_t)__popcll(same));
    before = __shfl(before, __ffsll((long long)same) - 1);
    rank[j] = before + (uint32_t)__popcll(below);
  }
  __syncthreads();

  // thread t owns digit t: the waves' counts become the counts of the waves before; the tile's count is scanned
  {
    uint32_t total = 0;
    for (int w = 0; w < RO_WAVES; ++w) {
      const uint32_t c = wave_count[w][t];
      wave_count[w][t] = total;
      total += c;
    }
    const uint32_t first = ro_block_exclusive(total, scan_sh);
    first_of[t] = first;
    dest_of[t] = offset[(int64_t)t * n_tiles + tile] - first;
  }
  __syncthreads();

#pragma unroll
  for (int j = 0; j < RO_ITEMS; ++j) {
    const uint32_t digit = (key[j] >> shift) & 255u;
    const uint32_t place = first_of[digit] + wave_count[wave][digit] + rank[j];   // < RO_TILE: a permutation of the tile
    stage_key[place] = key[j];
    stage_idx[place] = idx[j];
  }
  __syncthreads();

  // the padding sorts behind every key of the tile (digit 255, last in memory): places n_valid.. are not stored
#pragma unroll
  for (int j = 0; j < RO_ITEMS; ++j) {
    const int place = j * RO_THREADS + t;
    if (place < n_valid) {
      const uint32_t q = stage_key[place];
      const uint32_t dst = dest_of[(q >> shift) & 255u] + (uint32_t)place;
      if (!LAST) key_out[dst] = q;
      idx_out[dst] = stage_idx[place];
    }
  }
}

// ---- workspace ------------------------------------------------------------------------------------

inline int64_t align256(int64_t b) { return (b + 255) & ~(int64_t)255; }

struct Layout {
  int64_t n_tiles, hist_n;
  int64_t key_a, key_b, idx_a, hist, sums, partial, box, bytes;   // byte offsets
  std::vector<int64_t> level_n, level_off;                        // chunk sums per scan level (entries, offset in words)
};

Layout layout(int64_t n)
{
  Layout L;
  L.n_tiles = (n + DT_RAY_ORDER_TILE - 1) / DT_RAY_ORDER_TILE;
  L.hist_n = 256 * L.n_tiles;
  int64_t at = 0;
  auto take = [&](int64_t bytes) {
    const int64_t here = at;
    at += align256(bytes);
    return here;
  };
  L.key_a = take(4 * n);
  L.key_b = take(4 * n);
  L.idx_a = take(4 * n);
  L.hist = take(4 * L.hist_n);
  int64_t words = 0;
  for (int64_t m = L.hist_n; m > RO_SCAN_CHUNK;) {
    m = (m + RO_SCAN_CHUNK - 1) / RO_SCAN_CHUNK;
    L.level_n.push_back(m);
    L.level_off.push_back(words);
    words += (m + 63) & ~(int64_t)63;
  }
  L.sums = take(4 * words);
  L.partial = take(8 * 6 * RO_BOX_BLOCKS);
  L.box = take(8 * 6);
  L.bytes = at + 256;   // the caller's pointer is aligned up to 256 bytes
  return L;
}

// the exclusive scan of v[0..m) in place: chunk sums, their scan (recursively), then the chunks
hipError_t enqueue_scan(hipStream_t st, uint32_t* v, int64_t m, uint32_t* sums, const Layout& L, size_t level)
{
  const int64_t blocks = (m + RO_SCAN_CHUNK - 1) / RO_SCAN_CHUNK;
  if (blocks <= 1) {
    hipLaunchKernelGGL(ro_scan_apply, dim3(1), dim3(RO_THREADS), 0, st, v, m, (const uint32_t*)nullptr);
    return hipGetLastError();
  }
  uint32_t* mine = sums + L.level_off[level];
  hipLaunchKernelGGL(ro_scan_reduce, dim3((unsigned)blocks), dim3(RO_THREADS), 0, st, (const uint32_t*)v, m, mine);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = enqueue_scan(st, mine, blocks, sums, L, level + 1);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ro_scan_apply, dim3((unsigned)blocks), dim3(RO_THREADS), 0, st, v, m, (const uint32_t*)mine);
  return hipGetLastError();
}

template <bool FIRST, bool LAST>
hipError_t enqueue_scatter(hipStream_t st, unsigned tiles, const uint32_t* key_in, const uint32_t* idx_in, int64_t n,
                           int shift, const uint32_t* offset, int64_t n_tiles, uint32_t* key_out, uint32_t* idx_out)
{
  hipLaunchKernelGGL((ro_scatter<FIRST, LAST>), dim3(tiles), dim3(RO_THREADS), 0, st, key_in, idx_in, n, shift, offset,
                     n_tiles, key_out, idx_out);
  return hipGetLastError();
}

constexpr post::Fail ro_fail{"dt_ray_order"};
constexpr post::Fail pr_fail{"dt_permute_rows"};

// null: the parameters are fine; else what is wrong with them
std::string params_wrong(const dt_ray_order_params* p)
{
  if (p->origin_bits < 0 || p->origin_bits > 10)
    return "origin_bits " + std::to_string(p->origin_bits) + " outside 0..10";
  if (p->dir_bits < 0 || p->dir_bits > 8) return "dir_bits " + std::to_string(p->dir_bits) + " outside 0..8";
  const int B = 3 * p->origin_bits + 2 * p->dir_bits;
  if (B < 1 || B > 30)
    return "3*origin_bits + 2*dir_bits = " + std::to_string(B) + " key bits, outside 1..30";
  if (p->dir_major != 0 && p->dir_major != 1) return "dir_major is neither 0 nor 1";
  if (p->box_given != 0 && p->box_given != 1) return "box_given is neither 0 nor 1";
  if (p->box_given)
    for (int k = 0; k < 3; ++k) {
      if (!dto::order_finite(p->box_lo[k]) || !dto::order_finite(p->box_hi[k])) return "box_lo / box_hi is not finite";
      if (p->box_lo[k] > p->box_hi[k]) return "box_lo > box_hi on axis " + std::to_string(k);
    }
  return std::string();
}

// ---- rows -----------------------------------------------------------------------------------------

// rows of `units` words of type U: dst[i] = src[perm[i]], or dst[perm[i]] = src[i]
template <class U>
__global__ __launch_bounds__(RO_THREADS) void ro_permute(int64_t n, int units, const uint32_t* perm, const U* src, U* dst,
                                                         int inverse)
{
  for (int64_t i = (int64_t)blockIdx.x * RO_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * RO_THREADS) {
    const int64_t p = perm[i];
    const int64_t from = (inverse ? i : p) * units, to = (inverse ? p : i) * units;
    for (int w = 0; w < units; ++w) dst[to + w] = src[from + w];
  }
}

template <class U>
hipError_t enqueue_permute(hipStream_t st, int64_t n, int units, const uint32_t* perm, const void* src, void* dst,
                           int inverse)
{
  hipLaunchKernelGGL(ro_permute<U>, post::linear_grid(n, 1 << 20), dim3(RO_THREADS), 0, st, n, units, perm, (const U*)src,
                     (U*)dst, inverse);
  return hipGetLastError();
}

}  // namespace

extern "C" void dt_ray_order_params_default(dt_ray_order_params* p)
{
  if (!p) return;
  p->origin_bits = 5;
  p->dir_bits = 6;
  p->dir_major = 0;
  p->box_given = 0;
  for (int k = 0; k < 3; ++k) p->box_lo[k] = p->box_hi[k] = 0.0;
}

extern "C" int dt_ray_order_key(const dt_ray_order_params* p, const double lo[3], const double hi[3], const double start[3],
                                const double dir[3], uint32_t* key)
{
  constexpr post::Fail fail{"dt_ray_order_key"};
  if (!p) return fail("null params");
  if (!lo) return fail("null lo");
  if (!hi) return fail("null hi");
  if (!start) return fail("null start");
  if (!dir) return fail("null dir");
  if (!key) return fail("null key");
  const std::string wrong = params_wrong(p);
  if (!wrong.empty()) return fail(wrong);
  *key = dto::order_key(p->origin_bits, p->dir_bits, p->dir_major, lo, hi, start, dir);
  return DT_OK;
}

extern "C" int64_t dt_ray_order_workspace_bytes(int64_t n_rays)
{
  if (n_rays <= 0 || n_rays > ((int64_t)1 << 30)) return 0;
  return layout(n_rays).bytes;
}

extern "C" int dt_ray_order(int64_t n_rays, const double* start, const double* dir, const dt_ray_order_params* p,
                            uint32_t* perm, uint32_t* keys, double* box, void* workspace, int32_t on_device, void* stream,
                            float* kernel_ms)
{
  if (!start) return ro_fail("null start");
  if (!dir) return ro_fail("null dir");
  if (!p) return ro_fail("null params");
  if (!perm) return ro_fail("null perm");
  if (on_device && !workspace) return ro_fail("null workspace");
  if (n_rays < 0) return ro_fail("n_rays < 0");
  const std::string wrong = params_wrong(p);
  if (!wrong.empty()) return ro_fail(wrong);
  if (n_rays > ((int64_t)1 << 30)) {
    dth::set_error("dt_ray_order: n_rays " + std::to_string(n_rays) + " above 2^30");
    return DT_E_LIMIT;
  }
  if (kernel_ms) *kernel_ms = 0.0f;
  const int ob = p->origin_bits, db = p->dir_bits, B = 3 * ob + 2 * db;
  double given[6];
  for (int k = 0; k < 3; ++k) {
    given[k] = p->box_given ? p->box_lo[k] : 0.0;
    given[3 + k] = p->box_given ? p->box_hi[k] : 0.0;
  }
  if (n_rays == 0) {
    if (box) std::copy(given, given + 6, box);
    return DT_OK;
  }
  const int64_t n = n_rays;

  if (!on_device) {
    double bx[6];
    if (p->box_given)
      std::copy(given, given + 6, bx);
    else
      host_box(n, start, dir, bx);
    std::vector<uint32_t> own;
    uint32_t* q = keys;
    if (!q) {
      own.resize((size_t)n);
      q = own.data();
    }
    for (int64_t i = 0; i < n; ++i) q[i] = dto::order_key(ob, db, p->dir_major, bx, bx + 3, start + 3 * i, dir + 3 * i);
    for (int64_t i = 0; i < n; ++i) perm[i] = (uint32_t)i;
    std::stable_sort(perm, perm + n, [q](uint32_t a, uint32_t b) { return q[a] < q[b]; });
    if (box) std::copy(bx, bx + 6, box);
    return DT_OK;
  }

  const Layout L = layout(n);
  char* ws = (char*)(((uintptr_t)workspace + 255u) & ~(uintptr_t)255u);
  uint32_t* key_a = (uint32_t*)(ws + L.key_a);
  uint32_t* key_b = (uint32_t*)(ws + L.key_b);
  uint32_t* idx_a = (uint32_t*)(ws + L.idx_a);
  uint32_t* hist = (uint32_t*)(ws + L.hist);
  uint32_t* sums = (uint32_t*)(ws + L.sums);
  double* partial = (double*)(ws + L.partial);
  double* dbox = (double*)(ws + L.box);
  OrderArgs a;
  a.n = n;
  a.ob = ob;
  a.db = db;
  a.dir_major = p->dir_major;
  a.start = start;
  a.dir = dir;
  a.box = dbox;
  a.box_given = p->box_given;
  std::copy(given, given + 6, a.given);
  const int passes = (B + 1 + 7) / 8;
  const unsigned tiles = (unsigned)L.n_tiles;
  hipStream_t st = (hipStream_t)stream;
  const int rc = post::launch(st, kernel_ms, ro_fail.who, [&] {
    hipError_t e = hipSuccess;
    if (!p->box_given) {
      const dim3 grid = post::linear_grid(n, RO_BOX_BLOCKS);
      hipLaunchKernelGGL(ro_box_partial, grid, dim3(RO_THREADS), 0, st, a, partial);
      hipLaunchKernelGGL(ro_box_final, dim3(1), dim3(RO_THREADS), 0, st, (const double*)partial, (int)grid.x, dbox);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(ro_key, post::linear_grid(n, 1 << 20), dim3(RO_THREADS), 0, st, a, key_a, keys);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // the index arrays alternate so that the last pass writes perm
    const uint32_t* key_in = key_a;
    uint32_t* key_out = key_b;
    for (int pass = 0; pass < passes; ++pass) {
      const int shift = 8 * pass;
      const bool first = pass == 0, last = pass == passes - 1;
      uint32_t* idx_out = (passes - 1 - pass) % 2 == 0 ? perm : idx_a;
      const uint32_t* idx_in = idx_out == perm ? idx_a : perm;
      hipLaunchKernelGGL(ro_hist, dim3(tiles), dim3(RO_THREADS), 0, st, key_in, n, shift, hist, L.n_tiles);
      if ((e = hipGetLastError()) != hipSuccess) return e;
      if ((e = enqueue_scan(st, hist, L.hist_n, sums, L, 0)) != hipSuccess) return e;
      if (first && last)
        e = enqueue_scatter<true, true>(st, tiles, key_in, idx_in, n, shift, hist, L.n_tiles, key_out, idx_out);
      else if (first)
        e = enqueue_scatter<true, false>(st, tiles, key_in, idx_in, n, shift, hist, L.n_tiles, key_out, idx_out);
      else if (last)
        e = enqueue_scatter<false, true>(st, tiles, key_in, idx_in, n, shift, hist, L.n_tiles, key_out, idx_out);
      else
        e = enqueue_scatter<false, false>(st, tiles, key_in, idx_in, n, shift, hist, L.n_tiles, key_out, idx_out);
      if (e != hipSuccess) return e;
      const uint32_t* was = key_in;
      key_in = key_out;
      key_out = (uint32_t*)was;
    }
    if (box && !p->box_given) {   // the one wait of an untimed call: the box comes back to the host
      e = hipMemcpyAsync(box, dbox, 6 * sizeof(double), hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    return e;
  });
  if (rc == DT_OK && box && p->box_given) std::copy(given, given + 6, box);
  return rc;
}

extern "C" int dt_permute_rows(int64_t n, int32_t row_bytes, const uint32_t* perm, const void* src, void* dst,
                               int32_t inverse, int32_t on_device, void* stream)
{
  if (!perm) return pr_fail("null perm");
  if (!src) return pr_fail("null src");
  if (!dst) return pr_fail("null dst");
  if (n < 0) return pr_fail("n < 0");
  if (row_bytes < 1 || row_bytes > 64) return pr_fail("row_bytes " + std::to_string(row_bytes) + " outside 1..64");
  if (inverse != 0 && inverse != 1) return pr_fail("inverse is neither 0 nor 1");
  if (n > ((int64_t)1 << 32)) {
    dth::set_error("dt_permute_rows: n " + std::to_string(n) + " above 2^32");
    return DT_E_LIMIT;
  }
  {
    const uintptr_t s0 = (uintptr_t)src, d0 = (uintptr_t)dst, len = (uintptr_t)n * (uintptr_t)row_bytes;
    if (s0 < d0 + len && d0 < s0 + len && n > 0) return pr_fail("src and dst overlap");
  }
  if (n == 0) return DT_OK;
  // the widest word that divides the row and that both arrays are aligned to
  const uintptr_t both = (uintptr_t)src | (uintptr_t)dst | (uintptr_t)row_bytes;
  const int unit = both % 8 == 0 ? 8 : both % 4 == 0 ? 4 : 1;
  if (!on_device) {
    for (int64_t i = 0; i < n; ++i)
      if ((int64_t)perm[i] >= n)
        return pr_fail("perm[" + std::to_string(i) + "] = " + std::to_string(perm[i]) + " is not below n");
    const char* s = (const char*)src;
    char* d = (char*)dst;
    for (int64_t i = 0; i < n; ++i) {
      const int64_t from = inverse ? i : (int64_t)perm[i], to = inverse ? (int64_t)perm[i] : i;
      std::copy(s + from * row_bytes, s + (from + 1) * row_bytes, d + to * row_bytes);
    }
    return DT_OK;
  }
  hipStream_t st = (hipStream_t)stream;
  return post::launch(st, nullptr, pr_fail.who, [&] {   // untimed: nothing waits
    if (unit == 8) return enqueue_permute<uint64_t>(st, n, row_bytes / 8, perm, src, dst, inverse);
    if (unit == 4) return enqueue_permute<uint32_t>(st, n, row_bytes / 4, perm, src, dst, inverse);
    return enqueue_permute<uint8_t>(st, n, row_bytes, perm, src, dst, inverse);
  });
}
