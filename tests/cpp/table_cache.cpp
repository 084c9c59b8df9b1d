// Stand-alone driver of omgx_table_cache.h with a fake allocator (tests/test_table_cache_cpu.py builds it with
// -fsanitize=address,undefined and runs it).  Prints "ok <case>" per case, exits non-zero at the first failed check.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <thread>
#include <vector>
#include "../../omg-tools_amd/csrc/omgx_table_cache.h"

namespace {
struct Fake { std::atomic<long> live{0}, allocs{0}, frees{0}, copies{0}; int fail_alloc = 0, fail_copy = 0; };

int fake_alloc(void* ctx, int, size_t bytes, void** out) {
  Fake* f = (Fake*)ctx;
  if (f->fail_alloc) { *out = nullptr; return f->fail_alloc; }
  *out = aligned_alloc(256, (bytes + 255) & ~(size_t)255);
  ++f->live; ++f->allocs;
  return 0;
}
int fake_copy(void* ctx, int, void* dst, const void* src, size_t bytes) {
  Fake* f = (Fake*)ctx;
  if (f->fail_copy) return f->fail_copy;
  memcpy(dst, src, bytes); ++f->copies;
  return 0;
}
void fake_free(void* ctx, int, void* p) { Fake* f = (Fake*)ctx; free(p); --f->live; ++f->frees; }

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond); exit(1); } } while (0)

std::vector<char> image(size_t n, int seed) {
  std::vector<char> v(n);
  for (size_t i = 0; i < n; ++i) v[i] = (char)((i * 31 + seed) & 0xff);
  return v;
}
}  // namespace

int main() {
  using omgx::TableCache;
  Fake f;
  const omgx::TableCacheOps ops = {fake_alloc, fake_copy, fake_free, &f};
  const std::vector<char> a = image(4096, 1);
  {
    TableCache tc(ops);
    const TableCache::Entry* e1 = tc.take(0, a.data(), a.size());
    std::vector<char> a2 = a;      // equal content at another address
    const TableCache::Entry* e2 = tc.take(0, a2.data(), a2.size());
    CHECK(e1 && e1 == e2 && tc.refs(e1) == 2 && f.allocs == 1 && f.copies == 1 && tc.live() == 1);
    CHECK(((size_t)e1->dev & 255) == 0 && memcmp(e1->dev, a.data(), a.size()) == 0);
    puts("ok same_content_same_entry");

    std::vector<char> b = a; b[4095] ^= 1;      // one byte
    const TableCache::Entry* e3 = tc.take(0, b.data(), b.size());
    CHECK(e3 && e3 != e1 && tc.refs(e3) == 1 && tc.refs(e1) == 2 && f.allocs == 2);
    std::vector<char> b0 = a; b0[0] ^= 1;
    const TableCache::Entry* e3b = tc.take(0, b0.data(), b0.size());
    CHECK(e3b && e3b != e1 && e3b != e3 && f.allocs == 3);
    puts("ok one_byte_new_entry");

    const TableCache::Entry* e4 = tc.take(0, a.data(), a.size() - 256);      // a prefix: another size
    CHECK(e4 && e4 != e1 && tc.refs(e4) == 1 && f.allocs == 4);
    puts("ok other_size_new_entry");

    const TableCache::Entry* e5 = tc.take(1, a.data(), a.size());
    CHECK(e5 && e5 != e1 && e5->device == 1 && tc.refs(e5) == 1 && f.allocs == 5 && tc.live() == 5);
    puts("ok other_device_new_entry");

    // the last of several releases frees exactly once, whichever holder goes first
    tc.release(e1);
    CHECK(f.frees == 0 && tc.refs(e2) == 1);
    tc.release(e2);
    CHECK(f.frees == 1 && tc.live() == 4);
    const TableCache::Entry* g1 = tc.take(0, a.data(), a.size());      // take after free rebuilds
    CHECK(g1 && f.allocs == 6 && tc.refs(g1) == 1 && memcmp(g1->dev, a.data(), a.size()) == 0);
    puts("ok take_after_free_rebuilds");
    const TableCache::Entry* g2 = tc.take(0, a.data(), a.size());
    CHECK(g2 == g1 && tc.refs(g1) == 2);
    tc.release(g2);      // the other order: the second holder first
    CHECK(f.frees == 1);
    tc.release(g1);
    CHECK(f.frees == 2);
    puts("ok last_release_frees_once");

    tc.release(e3); tc.release(e3b); tc.release(e4); tc.release(e5);
    CHECK(tc.live() == 0 && f.live == 0 && f.allocs == f.frees);

    // a failing allocator / copy: no entry, nothing kept, the code handed through
    int err = 0, step = 0;
    f.fail_alloc = 2;
    CHECK(tc.take(0, a.data(), a.size(), &err, &step) == nullptr && err == 2 && step == TableCache::STEP_ALLOC && tc.live() == 0);
    f.fail_alloc = 0; f.fail_copy = 7;
    CHECK(tc.take(0, a.data(), a.size(), &err, &step) == nullptr && err == 7 && step == TableCache::STEP_COPY && tc.live() == 0 && f.live == 0);
    f.fail_copy = 0;
    puts("ok failures_leave_nothing");
  }
  {
    // 8 threads take and release the same three images concurrently
    TableCache tc(ops);
    const std::vector<char> imgs[3] = {image(4096, 1), image(4096, 2), image(1024, 1)};
    std::atomic<int> bad{0};
    std::vector<std::thread> th;
    for (int t = 0; t < 8; ++t)
      th.emplace_back([&, t] {
        for (int it = 0; it < 500; ++it) {
          const std::vector<char>& im = imgs[(t + it) % 3];
          const TableCache::Entry* e = tc.take(it & 1, im.data(), im.size());
          const TableCache::Entry* e2 = tc.take(it & 1, im.data(), im.size());
          if (!e || e != e2 || memcmp(e->dev, im.data(), im.size()) != 0) ++bad;
          if (it % 3 == 0) { tc.release(e); tc.release(e2); } else { tc.release(e2); tc.release(e); }
        }
      });
    for (auto& x : th) x.join();
    CHECK(bad == 0 && tc.live() == 0 && f.live == 0 && f.allocs == f.frees);
    puts("ok threads_end_with_nothing_live");
  }
  return 0;
}
