// The one owner of a context's device and host allocations (sae_ctx::mem): every buffer the context holds is a pointer FIELD of the
// context, allocated through alloc / grow and released by free_all -- sae_destroy keeps no list of names.  Host code only and no HIP
// include: a memory kind is a pair of functions the user supplies (engine.hip: the HIP ones; tests/test_dev_mem_cpu.py: malloc-backed
// ones), so g++ compiles this header for a stand-alone test.
#pragma once
#include <stddef.h>
#include <stdio.h>

#include <vector>

enum DevMemKind {
  DM_DEVICE = 0,   // plain device memory
  DM_PEER,         // what the peers of a data-parallel run map (G, Gb, stats): fine-grained where the context asks for it, else plain
  DM_UNCACHED,     // uncached device memory (the flag block the peers write and this rank polls)
  DM_PINNED,       // pinned host memory
  DM_MAPPED,       // host memory mapped into the device's address space
  DM_KINDS
};

struct DevMemBackend {
  const char* (*alloc)(void** p, size_t bytes);   // null on success, else the reason (*p is not used then)
  void (*free)(void* p);
};

struct DevMem {
  struct Rec {
    void** field;
    size_t bytes;       // 0: the field is null (never filled, or its last allocation failed)
    int kind;
  };
  DevMemBackend kinds[DM_KINDS] = {};
  std::vector<Rec> recs;
  char err[256] = "";   // the message of the last failure

  // a new field: allocate, store the pointer into it and record it.  false: the field is null, `err` says why.
  template <typename T>
  bool alloc(T*& field, long long bytes, int kind, const char* name) {
    recs.push_back(Rec{(void**)&field, 0, kind});
    return fill(recs.back(), bytes, name);
  }

  // at least `bytes` behind the field: at once if the recorded size suffices, else the old block is freed, the field nulled and a
  // new block allocated (its contents are NOT carried over).  After a failure the field is null and its recorded size 0: the next
  // grow tries again.
  template <typename T>
  bool grow(T*& field, long long bytes, int kind, const char* name) {
    Rec* r = nullptr;
    for (Rec& q : recs)
      if (q.field == (void**)&field) r = &q;
    if (!r) return alloc(field, bytes, kind, name);
    if (r->bytes >= (size_t)bytes && r->bytes > 0) return true;
    release(*r);
    return fill(*r, bytes, name);
  }

  // every record released by its kind's free, every field nulled; the owner is empty afterwards
  void free_all() {
    for (Rec& r : recs) release(r);
    recs.clear();
  }

 private:
  void release(Rec& r) {
    if (r.bytes) kinds[r.kind].free(*r.field);
    *r.field = nullptr;
    r.bytes = 0;
  }
  bool fill(Rec& r, long long bytes, const char* name) {
    void* p = nullptr;
    if (const char* why = kinds[r.kind].alloc(&p, (size_t)bytes)) {
      snprintf(err, sizeof(err), "hipMalloc(%lld bytes) for %s failed: %s", bytes, name, why);
      *r.field = nullptr;
      return false;
    }
    *r.field = p;
    r.bytes = (size_t)bytes;
    return true;
  }
};
