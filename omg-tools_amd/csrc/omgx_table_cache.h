// omgx_table_cache.h -- one device copy of a plan's tables per template and device.
//
// Every handle of a template walks the same ~60 read-only tables (omgx::Tables).  Handles of one process that are built from the
// same template on the same device -- the sub-batches of a StreamedP2P, a rollout handle beside a per-step handle -- share one
// device image of them: the first handle uploads it, the others take a reference, the last release frees it.
//
// Ownership rule: an image is owned by the cache, never by a handle.  A handle holds a reference from omgx_batch_create to
// omgx_batch_destroy and only reads through it; no kernel and no later call writes into an image.  Whatever a kernel or a call
// writes -- slabs, carried state, counters, staging buffers, everything allocated lazily -- stays with its handle.
//
// Entries are keyed by the device and by the full content of the image (the bytes are compared, a hash only narrows the search).
// Host code without HIP: allocation, copy and free are callbacks, so that the cache can be driven by a fake allocator on a CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <memory>
#include <mutex>
#include <vector>

namespace omgx {

// Device memory as the cache sees it.  alloc / copy return 0 or the allocator's error code (handed through by take); `ctx` is
// the caller's.  alloc returns memory aligned to at least 256 bytes (hipMalloc does).
struct TableCacheOps {
  int (*alloc)(void* ctx, int device, size_t bytes, void** out);
  int (*copy)(void* ctx, int device, void* dst, const void* src, size_t bytes);
  void (*free)(void* ctx, int device, void* ptr);
  void* ctx;
};

class TableCache {
 public:
  struct Entry {
    int device = 0;
    uint64_t hash = 0;
    std::vector<char> image;      // the host copy the key is compared against
    void* dev = nullptr;          // the device image: image.size() bytes, one allocation
    size_t refs = 0;
  };
  enum Step { STEP_NONE = 0, STEP_ALLOC = 1, STEP_COPY = 2 };      // where take failed

  explicit TableCache(const TableCacheOps& ops) : ops_(ops) {}
  TableCache(const TableCache&) = delete;
  TableCache& operator=(const TableCache&) = delete;

  // The entry of (device, image): the one that exists with a reference more, or a new one (one exact-size allocation, one copy)
  // with one reference.  nullptr on failure: *err is the allocator's code, *step says whose.
  const Entry* take(int device, const void* image, size_t bytes, int* err = nullptr, int* step = nullptr) {
    if (err) *err = 0;
    if (step) *step = STEP_NONE;
    const uint64_t h = hash_of(image, bytes);
    std::lock_guard<std::mutex> lock(mu_);
    for (auto& e : entries_)
      if (e->device == device && e->hash == h && e->image.size() == bytes && (bytes == 0 || memcmp(e->image.data(), image, bytes) == 0)) {
        ++e->refs;
        return e.get();
      }
    std::unique_ptr<Entry> e(new Entry());
    e->device = device; e->hash = h; e->refs = 1;
    e->image.assign((const char*)image, (const char*)image + bytes);
    int rc = ops_.alloc(ops_.ctx, device, bytes > 0 ? bytes : 1, &e->dev);
    if (rc != 0 || !e->dev) { if (err) *err = rc; if (step) *step = STEP_ALLOC; return nullptr; }
    if (bytes > 0 && (rc = ops_.copy(ops_.ctx, device, e->dev, e->image.data(), bytes)) != 0) {
      ops_.free(ops_.ctx, device, e->dev);
      if (err) *err = rc;
      if (step) *step = STEP_COPY;
      return nullptr;
    }
    entries_.push_back(std::move(e));
    return entries_.back().get();
  }

  // One reference less; the last one frees the device image and forgets the entry.
  void release(const Entry* entry) {
    if (!entry) return;
    std::lock_guard<std::mutex> lock(mu_);
    for (size_t i = 0; i < entries_.size(); ++i)
      if (entries_[i].get() == entry) {
        if (--entries_[i]->refs == 0) {
          ops_.free(ops_.ctx, entries_[i]->device, entries_[i]->dev);
          entries_.erase(entries_.begin() + i);
        }
        return;
      }
  }

  size_t live() const { std::lock_guard<std::mutex> lock(mu_); return entries_.size(); }
  size_t refs(const Entry* entry) const {
    std::lock_guard<std::mutex> lock(mu_);
    for (auto& e : entries_) if (e.get() == entry) return e->refs;
    return 0;
  }

 private:
  static uint64_t hash_of(const void* p, size_t n) {      // FNV-1a; narrows the search only
    uint64_t h = 1469598103934665603ull;
    const unsigned char* q = (const unsigned char*)p;
    for (size_t i = 0; i < n; ++i) { h ^= q[i]; h *= 1099511628211ull; }
    return h;
  }
  TableCacheOps ops_;
  mutable std::mutex mu_;
  std::vector<std::unique_ptr<Entry>> entries_;
};

}  // namespace omgx
