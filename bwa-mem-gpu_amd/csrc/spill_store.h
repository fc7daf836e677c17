// The host-side store of a device merger's spilled runs (spill_store.cpp): the record bytes of a run, by run number, either in memory
// from an injected allocator (malloc by default; the merger passes pinned allocation) or, once host_budget would be exceeded, whole in an
// unlinked file of tmp_dir.  No device, no HIP: the translation unit builds and runs with a plain C++ compiler.
#pragma once
#include <stdint.h>
#include <stddef.h>

struct SpillStore;
typedef void *(*spill_alloc_fn)(size_t bytes, void *user);          // nullptr: refused
typedef void (*spill_free_fn)(void *p, size_t bytes, void *user);

// host_budget >= 0: the bytes memory placement may take in all; tmp_dir may be null while no run needs a file.  alloc / free null: malloc / free
SpillStore *spill_store_new(int64_t host_budget, const char *tmp_dir, spill_alloc_fn alloc, spill_free_fn free_, void *user);
void spill_store_free(SpillStore *s);                               // drops every run
// A run's place is decided by its length alone: memory while host_bytes + len <= host_budget, a file otherwise (len == 0: neither).
// reserve: 0 and *mem = the run's memory (the caller fills it), or *mem = nullptr for a file the caller fills with spill_store_write in any
// order.  BWAHIP_EINVAL: id held already or len < 0; BWAHIP_EIO: the file cannot be made; BWAHIP_ENOMEM: the allocator refused.  After a
// refusal the store holds what it held before.
int spill_store_reserve(SpillStore *s, int64_t id, int64_t len, uint8_t **mem);
int spill_store_write(SpillStore *s, int64_t id, int64_t at, const uint8_t *bytes, int64_t len);   // file-backed runs; survives short writes
int spill_store_put(SpillStore *s, int64_t id, const uint8_t *bytes, int64_t len);                 // reserve + fill; on failure the run is dropped
const uint8_t *spill_store_mem(const SpillStore *s, int64_t id);                                   // the run's memory, or nullptr (a file, empty, unknown)
int spill_store_get(const SpillStore *s, int64_t id, int64_t at, int64_t len, uint8_t *dst);       // any slice within the run; survives short reads
int64_t spill_store_len(const SpillStore *s, int64_t id);                                          // -1: unknown
int spill_store_drop(SpillStore *s, int64_t id);
int64_t spill_store_host_bytes(const SpillStore *s);
int64_t spill_store_file_bytes(const SpillStore *s);
