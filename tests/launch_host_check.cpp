// launch_host_check.cpp — the device-free half of the render launch path (csrc/host_launch.h): the
// grow-only device buffer over a counting allocator, and the launch policy against the values the
// measurements in its comments settled on. Built and run by tests/test_launch_host.py under ASan and
// UBSan; exit status 0 and "ok" when every check holds.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>
#include <string>

#include "host_launch.h"

static int g_failed = 0;
#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                      \
    }                                                                  \
  } while (0)

// malloc/free that counts, records the order of its calls and can fail the next allocation
struct FakeMem {
  typedef int Stream;
  static int allocs, frees, drains;
  static bool fail_next;
  static std::string log;   // 'a' alloc, 'f' free, 'd' drain, 'x' failed alloc
  static int alloc(void** p, size_t bytes)
  {
    if (fail_next) {
      fail_next = false;
      log += 'x';
      return 2;   // (hipErrorOutOfMemory's value; any non-zero code)
    }
    *p = malloc(bytes);
    memset(*p, 0xab, bytes);   // the whole allocation is writable (ASan)
    ++allocs;
    log += 'a';
    return 0;
  }
  static void free(void* p)
  {
    ::free(p);
    ++frees;
    log += 'f';
  }
  static int sync(Stream)
  {
    ++drains;
    log += 'd';
    return 0;
  }
  static void reset()
  {
    allocs = frees = drains = 0;
    fail_next = false;
    log.clear();
  }
};
int FakeMem::allocs, FakeMem::frees, FakeMem::drains;
bool FakeMem::fail_next;
std::string FakeMem::log;

typedef dth::DevBuf<FakeMem> Buf;

static void check_buffer()
{
  const size_t n = 1000;
  FakeMem::reset();
  Buf b;
  bool grew = false;
  // a first reserve allocates once, drains nothing, reports the growth
  CHECK(b.reserve(n, 0, &grew) == 0);
  CHECK(grew && b.p && b.cap == n);
  CHECK(FakeMem::allocs == 1 && FakeMem::drains == 0 && FakeMem::frees == 0);
  // smaller or equal: nothing changes
  void* const p0 = b.p;
  for (size_t m : {n, n - 1, (size_t)1, (size_t)0}) {
    grew = false;
    CHECK(b.reserve(m, 0, &grew) == 0);
    CHECK(!grew && b.p == p0 && b.cap == n);
  }
  CHECK(FakeMem::log == "a");
  // larger: drain, then free, then allocate
  grew = false;
  CHECK(b.reserve(2 * n, 0, &grew) == 0);
  CHECK(grew && b.p && b.cap == 2 * n);
  CHECK(FakeMem::log == "adfa");
  CHECK(FakeMem::allocs == 2 && FakeMem::drains == 1 && FakeMem::frees == 1);
  // a growth whose allocation fails: the error, and an empty buffer (no pointer behind a capacity,
  // no capacity behind a null pointer)
  FakeMem::fail_next = true;
  grew = false;
  CHECK(b.reserve(4 * n, 0, &grew) == 2);
  CHECK(!grew && b.p == nullptr && b.cap == 0);
  CHECK(FakeMem::log == "adfadfx");
  // ... so the next, smaller reserve allocates again (and has nothing to drain or free)
  CHECK(b.reserve(n, 0, &grew) == 0);
  CHECK(grew && b.p && b.cap == n);
  CHECK(FakeMem::log == "adfadfxa");
  // a first allocation that fails, without the grew argument
  Buf c;
  FakeMem::fail_next = true;
  CHECK(c.reserve(n, 0) == 2 && c.p == nullptr && c.cap == 0);
  CHECK(c.reserve(n, 0) == 0 && c.p && c.cap == n);
  c.release();
  // release twice frees once
  const int frees = FakeMem::frees;
  b.release();
  CHECK(b.p == nullptr && b.cap == 0 && FakeMem::frees == frees + 1);
  b.release();
  CHECK(FakeMem::frees == frees + 1);
  CHECK(FakeMem::allocs == FakeMem::frees);   // (and LeakSanitizer looks at exit)
  // an empty buffer released, reserve(0) on an empty buffer: no calls
  FakeMem::reset();
  Buf e;
  e.release();
  CHECK(e.reserve(0, 0, &grew) == 0 && e.p == nullptr);
  CHECK(FakeMem::log.empty());
}

static const char* const ENV[] = {"DT_CHUNK_ITEMS", "DT_BATCH_ITEMS", "DT_BATCH_SIZE", "DT_QUEUE_SEGS", "DT_PRIO_STEPS"};
static void clear_env()
{
  for (const char* e : ENV) unsetenv(e);
}

static dtd::DParams params(int world, int chunks, int ppw, int64_t n_items)
{
  dtd::DParams P;
  memset(&P, 0, sizeof(P));
  P.world = world;
  P.chunks = chunks;
  P.ppw = ppw;
  P.spp = chunks > 1 ? 64 * chunks : 64 / ppw;
  P.n_items = n_items;
  return P;
}

static void check_policy()
{
  const int64_t grid = 1024;
  clear_env();
  // item_batch
  CHECK(dth::launch_policy(params(1, 1, 1, 0), 0, 32767, grid).item_batch == 1);
  CHECK(dth::launch_policy(params(1, 1, 1, 0), 0, 32768, grid).item_batch == 2);
  CHECK(dth::launch_policy(params(1, 1, 1, 0), 0, 262143, grid).item_batch == 2);
  CHECK(dth::launch_policy(params(1, 1, 1, 0), 0, 262144, grid).item_batch == 3);
  CHECK(dth::launch_policy(params(1, 4, 1, 0), 0, 262144, grid).item_batch == 1);
  setenv("DT_BATCH_SIZE", "2", 1);
  CHECK(dth::launch_policy(params(1, 4, 1, 0), 0, 262144, grid).item_batch == 2);
  clear_env();
  setenv("DT_BATCH_ITEMS", "1", 1);
  CHECK(dth::launch_policy(params(1, 1, 1, 0), 0, 1024, grid).item_batch == 2);
  clear_env();
  CHECK(dth::launch_policy(params(1, 1, 1, 0), 0, 1024, grid).item_batch == 1);   // (read again: nothing cached)
  // queue_segs
  CHECK(dth::launch_policy(params(1, 1, 1, 0), 0, 1024, grid).queue_segs == 1);
  CHECK(dth::launch_policy(params(8, 1, 1, 0), 0, 1024, grid).queue_segs == 8);
  CHECK(dth::launch_policy(params(8, 4, 1, 0), 0, 1024, grid).queue_segs == 1);
  CHECK(dth::launch_policy(params(8, 4, 1, 0), 1, 1024, grid).queue_segs == 8);
  setenv("DT_QUEUE_SEGS", "0", 1);
  CHECK(dth::launch_policy(params(8, 1, 1, 0), 0, 1024, grid).queue_segs == 1);
  setenv("DT_QUEUE_SEGS", "99", 1);
  CHECK(dth::launch_policy(params(1, 1, 1, 0), 0, 1024, grid).queue_segs == DT_QSEG_MAX);
  clear_env();
  // prio_steps
  CHECK(dth::launch_policy(params(8, 1, 1, 0), 0, 1024, grid).prio_steps == 8);
  CHECK(dth::launch_policy(params(1, 1, 4, 0), 0, 1024, grid).prio_steps == 2);
  CHECK(dth::launch_policy(params(1, 1, 1, 0), 0, 1024, grid).prio_steps == 0);
  setenv("DT_PRIO_STEPS", "5", 1);
  CHECK(dth::launch_policy(params(1, 1, 1, 0), 0, 1024, grid).prio_steps == 5);
  CHECK(dth::launch_policy(params(8, 1, 1, 0), 0, 1024, grid).prio_steps == 5);
  clear_env();
  // the policy hands the chunk-item mode on
  CHECK(dth::launch_policy(params(8, 4, 1, 0), 2, 1024, grid).chunk_items == 2);

  // chunk_items: the defaults
  const int T = 2 | 1;   // a build's traits with the chunk-item code (bit 1)
  CHECK(dth::launch_chunk_items(params(1, 4, 1, 1000), T, T, false) == 0);
  CHECK(dth::launch_chunk_items(params(8, 4, 1, 1000), T, T, false) == 1);
  setenv("DT_CHUNK_ITEMS", "2", 1);
  CHECK(dth::launch_chunk_items(params(1, 4, 1, 1000), T, T, false) == 2);
  CHECK(dth::launch_chunk_items(params(8, 4, 1, 1000), T, T, false) == 2);
  // either build without the code
  CHECK(dth::launch_chunk_items(params(8, 4, 1, 1000), T & ~2, T, false) == 0);
  CHECK(dth::launch_chunk_items(params(8, 4, 1, 1000), T, T & ~2, false) == 0);
  // one chunk, or more than the queue code's 255
  CHECK(dth::launch_chunk_items(params(8, 1, 1, 1000), T, T, false) == 0);
  CHECK(dth::launch_chunk_items(params(8, 256, 1, 1000), T, T, false) == 0);
  CHECK(dth::launch_chunk_items(params(8, 255, 1, 1000), T, T, false) == 2);
  // a window launch
  CHECK(dth::launch_chunk_items(params(8, 4, 1, 1000), T, T, true) == 0);
  // queue codes past 32 bits
  CHECK(dth::launch_chunk_items(params(8, 4, 1, (int64_t)1 << 30), T, T, false) == 0);
  CHECK(dth::launch_chunk_items(params(8, 4, 1, ((int64_t)1 << 30) - 1), T, T, false) == 2);
  // values outside 0..2
  setenv("DT_CHUNK_ITEMS", "3", 1);
  CHECK(dth::launch_chunk_items(params(8, 4, 1, 1000), T, T, false) == 0);
  setenv("DT_CHUNK_ITEMS", "-1", 1);
  CHECK(dth::launch_chunk_items(params(8, 4, 1, 1000), T, T, false) == 0);
  setenv("DT_CHUNK_ITEMS", "0", 1);
  CHECK(dth::launch_chunk_items(params(8, 4, 1, 1000), T, T, false) == 0);
  setenv("DT_CHUNK_ITEMS", "1", 1);
  CHECK(dth::launch_chunk_items(params(1, 4, 1, 1000), T, T, false) == 1);
  clear_env();
}

int main()
{
  check_buffer();
  check_policy();
  if (g_failed) {
    fprintf(stderr, "%d check(s) failed\n", g_failed);
    return 1;
  }
  puts("ok");
  return 0;
}
