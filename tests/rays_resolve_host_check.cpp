// rays_resolve_host_check.cpp — the host loop of dt_rays_resolve (csrc/dt_rays_resolve.h) alone, with no GPU
// code linked: built with ASan and UBSan by tests/test_camera_rays_host.py. Every array is a heap block of the
// exact size the call's contract gives it, so a read or a write one element past a row, a slot or a plane is
// reported. Checked against a second, plain summation written here: whole image and tile shares in both
// layouts, width 1..3, both modes, with and without shape, n_samples 1, 9 and 64.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dt_rays_resolve.h"

static int fails = 0;
#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);      \
      ++fails;                                                        \
    }                                                                 \
  } while (0)

static uint64_t rnd_state = 0x9E3779B97F4A7C15ull;
static double rnd()
{
  rnd_state ^= rnd_state << 13;
  rnd_state ^= rnd_state >> 7;
  rnd_state ^= rnd_state << 17;
  return (double)(int64_t)(rnd_state >> 11) / 9007199254740992.0 * 2000.0 - 1000.0;
}

static void tiles_of(rr::Args& a, int W, int H, int x0, int y0, int x1, int y1, int tw, int th, int rank, int world, int layout)
{
  a.xRes = W; a.yRes = H; a.x0 = x0; a.y0 = y0; a.x1 = x1; a.y1 = y1; a.tw = tw; a.th = th;
  a.rank = rank; a.world = world; a.layout = layout;
  a.tiles_x = (x1 - x0 + tw - 1) / tw;
  a.n_tiles = (int64_t)a.tiles_x * ((y1 - y0 + th - 1) / th);
  a.n_owned_tiles = (a.n_tiles + world - 1) / world;
  a.n_slots = layout ? a.n_owned_tiles * tw * th : (int64_t)W * H;
}

static void run(rr::Args a, int n, int width, int mode, bool with_shape, bool with_cov)
{
  a.n = n; a.width = width; a.mode = mode;
  const int64_t rows = a.n_slots * n;
  std::vector<double> values((size_t)(rows * width));
  std::vector<int32_t> shape((size_t)rows);
  for (double& v : values) v = rnd();
  for (int64_t r = 0; r < rows; ++r) shape[(size_t)r] = rnd() < -300.0 ? -1 : (int32_t)(r % 11);
  for (int i = 0; i < n && a.n_slots > 1; ++i) shape[(size_t)(n + i)] = -1;   // slot 1: no row counts
  std::vector<float> out((size_t)(a.n_slots * width), -3.0f), cov((size_t)a.n_slots, -3.0f);
  a.values = values.data();
  a.shape = with_shape ? shape.data() : nullptr;
  a.out = out.data();
  a.coverage = with_cov ? cov.data() : nullptr;
  rr::host_loop(a);
  int64_t owned = 0;
  for (int64_t q = 0; q < a.n_slots; ++q) {
    int x, y;
    const bool own = dtd::slot_pixel(a, q, x, y);
    owned += own;
    if (own) CHECK(x >= a.x0 && x < a.x1 && y >= a.y0 && y < a.y1);
    int H = 0;
    double S[3] = {0, 0, 0};
    for (int i = 0; i < n; ++i) {
      if (with_shape && shape[(size_t)(q * n + i)] < 0) continue;
      for (int k = 0; k < width; ++k) S[k] = S[k] + values[(size_t)((q * n + i) * width + k)];
      ++H;
    }
    for (int k = 0; k < width; ++k) {
      const float want = !own ? -3.0f : mode == rr::HIT_MEAN ? (H ? (float)(S[k] / (double)H) : 0.0f) : (float)(S[k] / (double)n);
      CHECK(std::memcmp(&want, &out[(size_t)(q * width + k)], sizeof(float)) == 0);
    }
    const float wc = own && with_cov ? (float)((double)H / (double)n) : -3.0f;
    CHECK(std::memcmp(&wc, &cov[(size_t)q], sizeof(float)) == 0);
  }
  // every pixel of the window has exactly one owner: this rank owns its share of them
  CHECK(owned > 0 && owned <= (int64_t)(a.x1 - a.x0) * (a.y1 - a.y0));
  if (a.world == 1) CHECK(owned == (int64_t)(a.x1 - a.x0) * (a.y1 - a.y0));
}

int main()
{
  rr::Args whole, img, slab, win;
  std::memset(&whole, 0, sizeof whole);
  img = slab = win = whole;
  tiles_of(whole, 70, 37, 0, 0, 70, 37, 32, 32, 0, 1, 0);
  tiles_of(img, 70, 37, 0, 0, 70, 37, 32, 32, 1, 2, 0);
  tiles_of(slab, 70, 37, 0, 0, 70, 37, 32, 32, 1, 2, 1);
  tiles_of(win, 33, 20, 3, 2, 31, 19, 16, 8, 2, 3, 1);
  const rr::Args* all[4] = {&whole, &img, &slab, &win};
  const int ns[3] = {1, 9, 64};
  for (const rr::Args* a : all)
    for (int n : ns)
      for (int width = 1; width <= 3; ++width)
        for (int mode = 0; mode < 2; ++mode)
          for (int sh = 0; sh < 2; ++sh) run(*a, n, width, mode, sh != 0, (n + width + mode + sh) % 2 == 0);
  // the shares of a split frame own every pixel once
  for (int layout = 0; layout < 2; ++layout) {
    std::vector<int> hits(70 * 37, 0);
    for (int rank = 0; rank < 3; ++rank) {
      rr::Args a;
      std::memset(&a, 0, sizeof a);
      tiles_of(a, 70, 37, 0, 0, 70, 37, 32, 32, rank, 3, layout);
      for (int64_t q = 0; q < a.n_slots; ++q) {
        int x, y;
        if (dtd::slot_pixel(a, q, x, y)) ++hits[(size_t)(y * 70 + x)];
      }
    }
    for (int h : hits) CHECK(h == 1);
  }
  if (!fails) std::printf("ok\n");
  return fails ? 1 : 0;
}
