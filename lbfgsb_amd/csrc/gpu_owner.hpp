// gpu_owner.hpp -- the one place of the host code that obtains and gives back device memory, pinned host memory
// and events (host-only; DESIGN.md "source layout" says how a new buffer is added).
//
// A GpuOwner does not hold the resources itself: the contexts keep their raw pointer and event members (the
// launches, lbk::Queue and WStore read them as they are).  It remembers WHERE each one it has filled lives -- the
// address of the member, its slot -- and of which kind it is, and gives back whatever the slots hold when it is
// told to or when it goes.  So a slot must outlive its owner's last use of it: members of a context that never
// moves (lbfgsb_hip_ctx::own), or locals declared in front of a local owner.  Never a static or global object: no
// GPU call may run from a static destructor.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <vector>

namespace lbs {

class GpuOwner {
 public:
  GpuOwner() = default;
  GpuOwner(const GpuOwner &) = delete;
  GpuOwner &operator=(const GpuOwner &) = delete;
  ~GpuOwner() { release_all(); }

  // Each of these frees what the slot holds, obtains the new resource into it and registers the slot on its first
  // use.  A failed call leaves the slot null (and registered: the next call fills it).
  template <typename P>
  hipError_t device(P **slot, size_t bytes) {
    void **s = take(slot, DEVICE);
    return nulled(s, hipMalloc(s, bytes));
  }
  // ... zero-filled on `stream`
  template <typename P>
  hipError_t device_zeroed(P **slot, size_t bytes, hipStream_t stream) {
    hipError_t e = device(slot, bytes);
    if (e == hipSuccess && (e = hipMemsetAsync(*slot, 0, bytes, stream)) != hipSuccess) drop(slot);
    return e;
  }
  template <typename P>
  hipError_t pinned(P **slot, size_t bytes, unsigned flags = hipHostMallocDefault) {
    void **s = take(slot, PINNED);
    return nulled(s, hipHostMalloc(s, bytes, flags));
  }
  hipError_t event(hipEvent_t *slot, unsigned flags = hipEventDefault) {
    take(slot, EVENT);
    const hipError_t e = hipEventCreateWithFlags(slot, flags);
    if (e != hipSuccess) *slot = nullptr;
    return e;
  }

  // free these slots early (they stay registered; a slot this owner has never filled is left alone)
  template <typename... P>
  void drop(P **...slot) {
    for (void **s : {reinterpret_cast<void **>(slot)...})
      for (const Slot &r : slots_)
        if (r.at == s) give_back(r);
  }
  // free every registered slot in order of registration, null it and forget it.  Errors of the frees are ignored:
  // a failing free leaves an error that the next allocation reports.
  void release_all() {
    for (const Slot &r : slots_) give_back(r);
    slots_.clear();
  }

 private:
  enum Kind { DEVICE, PINNED, EVENT };
  struct Slot {
    void **at;
    Kind kind;
  };
  std::vector<Slot> slots_;

  static void give_back(const Slot &r) {
    if (!*r.at) return;
    if (r.kind == DEVICE) (void)hipFree(*r.at);
    if (r.kind == PINNED) (void)hipHostFree(*r.at);
    if (r.kind == EVENT) (void)hipEventDestroy(static_cast<hipEvent_t>(*r.at));
    *r.at = nullptr;
  }
  template <typename P>
  void **take(P **slot, Kind kind) {
    void **s = reinterpret_cast<void **>(slot);
    for (const Slot &r : slots_)
      if (r.at == s) return give_back(r), s;
    slots_.push_back(Slot{s, kind});
    return s;
  }
  static hipError_t nulled(void **s, hipError_t e) {
    if (e != hipSuccess) *s = nullptr;
    return e;
  }
};

}  // namespace lbs
